"""ms per update of BootstrappedDQN (K = 1, 10) against DQN (listed as K = 0) on the same trunk
17 -> 128 x 128 x 128 -> A = 6 at B = 4096: graph-replayed, device events around every update, median / p10 / p90 of 300
updates after 20 warm-up updates (eager, captured, replayed), inputs already in the engine's static tensors; and the launch
list of one eager update by entry point.  Figures: profiles/NOTES_bootstrapped_dqn.md.

    python tools/boot_dqn_update_time.py                    # from the repository root; writes scratch_run/boot_measure_*.json
    MEASURE_KS=10 rocprofv3 --kernel-trace --stats -d scratch_run/prof -o boot --output-format csv -- python tools/boot_dqn_update_time.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchrl.networks as networks
import torchrl.policies as policies
from torchrl.algo import DQN, BootstrappedDQN
from torchrl_amd import _C
import gym

DEV = torch.device("cuda:0")
D, A, B, H = 17, 6, 4096, [128, 128, 128]

class Env: action_space = gym.spaces.Discrete(A)
class Stub: epoch_frames = 0
class Log:
    def add_update_info(self, d): pass

def batch(K):
    rs = np.random.RandomState(0)
    f = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).to(DEV)
    b = {"obs": f(B, D), "next_obs": f(B, D), "acts": torch.from_numpy(rs.randint(0, A, (B, 1)).astype(np.float32)).to(DEV),
         "rewards": f(B, 1), "terminals": (f(B, 1) > 0.8).float()}
    if K: b["masks"] = (f(B, K) > 0).float()
    return b

def make(K):
    torch.manual_seed(0)
    kw = dict(qlr=1e-3, env=Env(), replay_buffer=None, collector=Stub(), logger=Log(), discount=0.99, num_epochs=1,
              batch_size=B, device=DEV, save_dir=None, tau=0.005, use_soft_update=True, opt_times=1)
    if K == 0:
        qf = networks.Net(output_shape=A, base_type=networks.MLPBase, input_shape=D, hidden_shapes=H, append_hidden_shapes=[])
        pf = policies.EpsilonGreedyDQNDiscretePolicy(qf, 1, 0.1, 1000, A)
        return DQN(qf=qf, pf=pf, **kw)
    qf = networks.BootstrappedNet(output_shape=A, head_num=K, base_type=networks.MLPBase, input_shape=D, hidden_shapes=H)
    pf = policies.BootstrappedDQNDiscretePolicy(qf, K, A)
    return BootstrappedDQN(head_num=K, qf=qf, pf=pf, **kw)

def launches(agent, b):
    calls = []
    class Spy:
        def __init__(s, lib): s._lib = lib
        def __getattr__(s, name):
            if name.endswith(("_f32", "_i64")): calls.append(name)
            return getattr(s._lib, name)
    real = _C.lib()
    os.environ["TRL_NO_GRAPH"] = "1"
    _C._lib = Spy(real)
    agent.update(b)
    _C._lib = real
    del os.environ["TRL_NO_GRAPH"]
    return calls

out = {}
KS = [int(k) for k in os.environ.get("MEASURE_KS", "0,1,10").split(",")]
for K in KS:
    agent = make(K)
    b = batch(K)
    out["launches_K%d" % K] = launches(agent, b)
    st = agent.static_batch()                 # the fixed-address inputs themselves: no copies in the timed loop
    for k in st:
        st[k].copy_(b[k].reshape(st[k].shape))
    b = st
    for _ in range(20):                       # eager, captured, replayed warm-up
        h = agent.update_deferred(b)
    agent.resolve_updates([h])
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(300)]
    hs = []
    for s, e in ev:
        s.record(); hs.append(agent.update_deferred(b)); e.record()
        if len(hs) == 32:
            agent.resolve_updates(hs); hs = []
    if hs: agent.resolve_updates(hs)
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in ev)
    out["ms_K%d" % K] = {"median": ms[150], "p10": ms[30], "p90": ms[270]}
    assert len(agent.engine()._graphs) == 1
    print("K=%d median %.4f ms (p10 %.4f p90 %.4f) launches %d" % (K, ms[150], ms[30], ms[270], len(out["launches_K%d" % K])))
os.makedirs("scratch_run", exist_ok=True)
json.dump(out, open("scratch_run/boot_measure_%s.json" % "_".join(map(str, KS)), "w"), indent=1)
print("__MEASURE_OK__")
