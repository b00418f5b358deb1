"""Bootstrapped DQN over a conv trunk at the reference's shape (config/bootstrapped_dqn.json: 84 x 84 x 4 frames, convs
16/8/4 -> 32/4/2 -> 64/3/1, K = 10 heads 3136 -> 512 -> 6, RMSprop(alpha 0.95, eps 0.01), hard target copy), B = 512, 512 envs:

  head_dx    trl_boot_head_dx_f32 alone against the three launches it replaces (grouped input gradient into a (K, B, F) stack,
             trl_boot_fold_f32, trl_transpose_bpc_gate_f32), each captured as a graph, replayed alternately, device events
             around every replay; their outputs compared
  update     ms per update with either route (graph-replayed, inputs in the engine's static tensors)
  collect    ms per vector step of the per-step frame route on SynthAtari-v0 (host clock around a synchronised rollout)

Figures: profiles/NOTES_bootstrapped_dqn_conv.md.

    TRL_BOOT_CONV=1 python tools/time_boot_conv.py          # from the repository root; writes scratch_run/boot_conv_measure.json
"""
import functools
import json
import os
import sys
import time

import numpy as np
import torch

os.environ.setdefault("TRL_BOOT_CONV", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchrl.networks as networks                       # noqa: E402
import torchrl.policies as policies                       # noqa: E402
from torchrl.algo import BootstrappedDQN                  # noqa: E402
from torchrl.collector import VecCollector                # noqa: E402
from torchrl.replay_buffers import BaseReplayBuffer       # noqa: E402
from torchrl_amd import _C                                # noqa: E402
from torchrl_amd.algo.off_policy import bootstrapped_dqn as mod   # noqa: E402
from torchrl_amd.env.synth import SynthFrameVecEnv        # noqa: E402

DEV = torch.device("cuda:0")
K, B, A, H1, C, P, N = 10, 512, 6, 512, 64, 49, 512
SHAPE = (4, 84, 84)
CONVS = [[16, [8, 8], [4, 4], [0, 0]], [32, [4, 4], [2, 2], [0, 0]], [64, [3, 3], [1, 1], [0, 0]]]
REPS = int(os.environ.get("MEASURE_REPS", "200"))


def stats(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "p10": ms[len(ms) // 10], "p90": ms[(9 * len(ms)) // 10]}


def time_alternating(graphs, reps=REPS):
    """{name: stats} of graphs replayed in turn, device events around every replay."""
    for _ in range(5):
        for g in graphs.values():
            g.replay()
    torch.cuda.synchronize()
    ev = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for n in graphs}
    for i in range(reps):
        for n, g in graphs.items():
            s, e = ev[n][i]
            s.record(); g.replay(); e.record()
    torch.cuda.synchronize()
    return {n: stats([s.elapsed_time(e) for s, e in ev[n]]) for n in graphs}


def head_dx(out):
    rs = np.random.RandomState(0)
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).to(DEV)
    dzs = [t(B, H1) * (t(B, 1) > 0).float() for _ in range(K)]                # about half of the rows masked out per head
    gates = [torch.relu(t(B, H1)) for _ in range(K)]
    ws = [t(H1, C * P) / 22.0 for _ in range(K)]
    y_top = torch.relu(t(B, C, P))
    res = {}

    def new():
        res["new"] = _C.boot_head_dx(dzs, gates, _C.ACT_RELU, ws, y_top, _C.ACT_RELU, C, P, True)

    def old():
        stack = torch.empty((K, B, C * P), dtype=torch.float32, device=DEV)
        _C.linear_bwd_input_group(dzs, gates, _C.ACT_RELU, ws, dxs=list(stack.unbind(0)))
        res["old"] = _C.transpose_bpc(_C.boot_fold(stack).view(B, C, P), B, C, P, y_gate=y_top, gate_act=_C.ACT_RELU,
                                      gate_like_in=True)
    new(); old()
    torch.cuda.synchronize()
    a, b = res["new"].double().cpu().reshape(-1), res["old"].double().cpu().reshape(-1)     # (the eager results)
    graphs = {"head_dx": _C.capture_graph(new)[0], "three_launches": _C.capture_graph(old)[0]}
    out["head_dx_ms"] = time_alternating(graphs)
    out["head_dx_max_abs_diff"] = float((a - b).abs().max())
    out["head_dx_max_abs"] = float(b.abs().max())
    flop = 2.0 * B * C * P * K * H1
    out["head_dx_gflop"] = flop / 1e9
    for n, s in out["head_dx_ms"].items():
        print("%-15s median %.4f ms (p10 %.4f p90 %.4f)  %.1f TFLOP/s" % (n, s["median"], s["p10"], s["p90"],
                                                                        flop / s["median"] / 1e9))
    print("outputs differ by at most %.3g (largest value %.3g)" % (out["head_dx_max_abs_diff"], out["head_dx_max_abs"]))


class Log:
    def add_update_info(self, d): pass
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


def make_agent(env, buf=None, col_of=None):
    torch.manual_seed(0)
    qf = networks.BootstrappedNet(output_shape=A, head_num=K, append_hidden_shapes=[H1], activation_func=torch.nn.ReLU,
                                  base_type=functools.partial(networks.CNNBase, input_shape=SHAPE, hidden_shapes=CONVS)).to(DEV)
    pf = policies.BootstrappedDQNDiscretePolicy(qf, K, A)
    col = col_of(pf) if col_of else type("Stub", (), {"epoch_frames": 0})()
    agent = BootstrappedDQN(head_num=K, qf=qf, pf=pf, qlr=2.5e-4, env=env, replay_buffer=buf, collector=col, logger=Log(),
                            discount=0.99, num_epochs=1, batch_size=B, device=DEV, save_dir=None, tau=0.001,
                            use_soft_update=False, target_hard_update_period=10000, opt_times=1,
                            optimizer_class=torch.optim.RMSprop, optimizer_info=dict(alpha=0.95, eps=0.01))
    return agent, pf, col


def update(out):
    rs = np.random.RandomState(1)
    u8 = lambda: torch.from_numpy(rs.randint(0, 256, size=(B,) + SHAPE).astype(np.uint8)).to(DEV)
    f = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).to(DEV)
    batch = {"obs": u8(), "next_obs": u8(), "acts": torch.from_numpy(rs.randint(0, A, (B, 1)).astype(np.float32)).to(DEV),
             "rewards": f(B, 1), "terminals": (f(B, 1) > 0.8).float(), "masks": (f(B, K) > 0).float()}
    env = SynthFrameVecEnv(4, device=DEV)
    agents, default = {}, mod.HEAD_DX_FUSED
    for name, fused in (("fused", True), ("three_launches", False)):
        mod.HEAD_DX_FUSED = fused
        agent, _, _ = make_agent(env)
        agent.update(batch)
        st = agent.static_batch()
        for k in st:
            st[k].copy_(batch[k].reshape(st[k].shape))
        for _ in range(10):                                              # eager, captured, replayed
            h = agent.update_deferred(st)
        agent.resolve_updates([h])
        assert agent.engine().head_dx_fused == fused and len(agent.engine()._graphs) == 1
        agents[name] = (agent, st)
    mod.HEAD_DX_FUSED = default
    torch.cuda.synchronize()
    ev = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)] for n in agents}
    for i in range(REPS):
        for n, (agent, st) in agents.items():
            s, e = ev[n][i]
            s.record(); h = agent.update_deferred(st); e.record()
            if i % 32 == 31:
                agent.resolve_updates([h])
    torch.cuda.synchronize()
    out["update_ms"] = {n: stats([s.elapsed_time(e) for s, e in ev[n]]) for n in agents}
    for n, s in out["update_ms"].items():
        print("update %-15s median %.4f ms (p10 %.4f p90 %.4f)" % (n, s["median"], s["p10"], s["p90"]))


def collect(out):
    env, eval_env = SynthFrameVecEnv(N, device=DEV), SynthFrameVecEnv(N, device=DEV)
    steps = 16
    buf = BaseReplayBuffer(N * 64, env_nums=N)
    _, pf, col = make_agent(env, buf, lambda pf: VecCollector(env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=DEV,
                                                             epoch_frames=N * steps, max_episode_frames=999, eval_episodes=1))
    col.rollout(steps)
    torch.cuda.synchronize()
    times = []
    for _ in range(8):
        t0 = time.perf_counter()
        col.rollout(steps)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3 / steps)
    out["collect_ms_per_vector_step"] = stats(times)
    out["collect_envs"] = N
    s = out["collect_ms_per_vector_step"]
    print("collection: %.4f ms per vector step of %d envs (p10 %.4f p90 %.4f)" % (s["median"], N, s["p10"], s["p90"]))


def main():
    out = {"shape": dict(K=K, B=B, A=A, H1=H1, C=C, P=P, envs=N, reps=REPS)}
    head_dx(out)
    update(out)
    collect(out)
    os.makedirs("scratch_run", exist_ok=True)
    json.dump(out, open("scratch_run/boot_conv_measure.json", "w"), indent=1)
    print("__MEASURE_OK__")


if __name__ == "__main__":
    main()
