"""ms per `VMPO.update` and per `TRPO.update` for the three policy heads at one shape -- 17 -> 64 x 64 -> 6 actions (the
state-dependent-std head is then 12 wide), B = 2048 (V-MPO's actor step sees the top 1024) -- and the launch list of one
update by entry point.  Host wall clock around each update with a device synchronisation (both updates read statistics
back, TRPO once per CG iteration and line-search trial, so the host is part of what an update costs); median / p10 / p90 of 50
updates after 5 warm-up updates.  Information only: figures in profiles/NOTES_vmpo_trpo_heads.md.

    python tools/time_vmpo_trpo_heads.py                     # from the repository root; prints one JSON line
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchrl.networks as networks                                           # noqa: E402
import torchrl.policies as policies                                           # noqa: E402
from torchrl.algo import TRPO, VMPO                                           # noqa: E402
from torchrl_amd import _C                                                    # noqa: E402
import gym                                                                    # noqa: E402  (the package's stand-in when gym is absent)

DEV = torch.device("cuda:0")
D, A, H, B = 17, 6, 64, 2048


class Stub:
    epoch_frames = 0


class Log:
    def add_update_info(self, d): pass


def make(algo, kind):
    torch.manual_seed(0)
    net = dict(hidden_shapes=[H, H], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    if kind == "cat":
        pf = policies.CategoricalDisPolicy(input_shape=D, output_shape=A, **net)
    elif kind == "sd":
        pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, **net)
    else:
        pf = policies.GuassianContPolicyBasicBias(input_shape=D, output_shape=A, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    with torch.no_grad():
        pf.seq_append_fcs[-1].weight.mul_(30.0)

    class Env:
        action_space = gym.spaces.Discrete(A) if kind == "cat" else gym.spaces.Box(-1, 1, (A,))

    kw = dict(pf=pf, vf=vf, plr=3e-4, vlr=3e-4, tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=B, gae=True,
              env=Env(), replay_buffer=None, collector=Stub(), logger=Log(), device=DEV, save_dir=None)
    if algo == "trpo":
        return TRPO(max_kl=0.01, cg_damping=0.1, cg_iters=10, residual_tol=1e-10, entropy_coeff=0.01, v_opt_times=1, **kw), pf
    agent = VMPO(opt_epochs=1, **kw)
    agent.engine().sync_target_pf()
    return agent, pf


def batch(kind, pf):
    rs = np.random.RandomState(0)
    f = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).to(DEV)
    obs = f(B, D)
    acts = torch.from_numpy(rs.randint(0, A, (B, 1)).astype(np.float32)).to(DEV) if kind == "cat" else 0.5 * f(B, A)
    return {"obs": obs, "acts": acts, "advs": 2 * f(B, 1) + 0.5, "values": f(B, 1), "estimate_returns": f(B, 1)}


def launches(agent, b):
    calls = []

    class Spy:
        def __init__(s, lib): s._lib = lib

        def __getattr__(s, name):
            if name.endswith(("_f32", "_f64", "_i64")):
                calls.append(name)
            return getattr(s._lib, name)

    real = _C.lib()
    _C._lib = Spy(real)
    try:
        agent.update(b)
    finally:
        _C._lib = real
    return calls


out = {"shape": [D, H, A, B]}
for algo in ("vmpo", "trpo"):
    for kind in ("gauss", "cat", "sd"):
        agent, pf = make(algo, kind)
        b = batch(kind, pf)
        calls = launches(agent, b)
        for _ in range(5):
            agent.update(b)
        torch.cuda.synchronize()
        ms = []
        for _ in range(50):
            t0 = time.perf_counter()
            agent.update(b)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        ms.sort()
        key = "%s_%s" % (algo, kind)
        out[key] = {"median_ms": round(ms[25], 4), "p10_ms": round(ms[5], 4), "p90_ms": round(ms[45], 4), "entry_point_calls": len(calls),
                    "loss_calls": sorted(set(c for c in calls if "vmpo_losses" in c or "trpo_surrogate" in c or "fisher_scale" in c
                                             or "logp" in c))}
        print("%-11s median %.3f ms (p10 %.3f, p90 %.3f), %d entry-point calls in one update" % (key, ms[25], ms[5], ms[45], len(calls)),
              file=sys.stderr)
print(json.dumps(out))
