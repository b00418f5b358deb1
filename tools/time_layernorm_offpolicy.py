#!/usr/bin/env python
"""Time the grouped LayerNorm launches against back-to-back single-problem launches, and one TwinSACQ update at the
cfg-3 shape with and without `add_ln`, with device events (200 calls after 10 warm-up calls); one JSON line per figure.

    python tools/time_layernorm_offpolicy.py [--groups 6x4096x256,4x4096x256] [--iters 200] [--no-update]

Kernels.  G problems of (M, H): trl_layernorm_fwd_group_f32 / trl_layernorm_bwd_group_f32 (rows + one fold) against G
calls of trl_layernorm_fwd_f32 / trl_layernorm_bwd_f32 (G x (rows + fold)) -- the single-problem entry points are the
baseline.  Bytes a pass has to move (fp32), per problem: forward 8 M H + the (M, 2) statistics; backward 12 M H, the
statistics and its dgamma / dbeta slabs written and re-read.  The floor is those bytes over the 6.3 TB/s a float4 copy
reaches on an MI355X.

Update.  TwinSACQ, B = 4096, D 17, A 6, 256 x 256 ReLU nets, device noise, soft target updates: `engine.enqueue` on a
fixed batch -- after the second call a replayed graph -- with add_ln on policy and critics, and without it (the launch
sequence of a tree without the feature)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchrl_amd import _C                                                   # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def timed(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters                                 # microseconds per call


def kernels(G, M, H, iters, dev):
    a = [torch.relu(torch.randn(M, H, device=dev)) for _ in range(G)]
    dy = [torch.randn(M, H, device=dev) for _ in range(G)]
    gamma = [1 + 0.3 * torch.randn(H, device=dev) for _ in range(G)]
    beta = [0.2 * torch.randn(H, device=dev) for _ in range(G)]
    ys, sts = _C.layernorm_fwd_group(a, gamma, beta)
    dzs = [torch.empty_like(t) for t in a]
    dgs, dbs = [torch.empty(H, device=dev) for _ in range(G)], [torch.empty(H, device=dev) for _ in range(G)]
    lib = _C.lib()
    ws_g = torch.empty(lib.trl_layernorm_bwd_group_workspace(G, M, H), device=dev)
    ws_1 = torch.empty(lib.trl_layernorm_bwd_workspace(M, H), device=dev)
    act = _C.ACT_RELU

    def single_fwd():
        for g in range(G):
            _C.layernorm_fwd(a[g], gamma[g], beta[g], y=ys[g], stats=sts[g])

    def single_bwd():
        for g in range(G):
            _C.layernorm_bwd(dy[g], a[g], sts[g], gamma[g], act, dgs[g], dbs[g], dz=dzs[g], workspace=ws_1)
    res = {"G": G, "M": M, "H": H, "iters": iters,
           "fwd_group_us": round(timed(lambda: _C.layernorm_fwd_group(a, gamma, beta, ys=ys, statss=sts), iters), 2),
           "fwd_singles_us": round(timed(single_fwd, iters), 2),
           "bwd_group_us": round(timed(lambda: _C.layernorm_bwd_group(dy, a, sts, gamma, act, dgs, dbs, dzs=dzs, workspace=ws_g),
                                       iters), 2),
           "bwd_singles_us": round(timed(single_bwd, iters), 2)}
    fwd_bytes = G * (8 * M * H + 8 * M + 8 * H)
    res["fwd_floor_us"] = round(fwd_bytes / HBM_BYTES_PER_S * 1e6, 2)
    res["bwd_floor_group_us"] = round((G * (12 * M * H + 8 * M + 12 * H) + 8 * ws_g.numel()) / HBM_BYTES_PER_S * 1e6, 2)
    res["bwd_floor_singles_us"] = round(G * (12 * M * H + 8 * M + 12 * H + 8 * ws_1.numel()) / HBM_BYTES_PER_S * 1e6, 2)
    res["note"] = "device events around back-to-back calls: launch gaps and the Python wrappers included"
    print(json.dumps(res))


def update(add_ln, iters, dev):
    from torchrl_amd import networks, policies
    from torchrl_amd.algo import TwinSACQ
    from torchrl_amd.env.synth import SynthVecEnv
    B, D, A, H = 4096, 17, 6, 256
    os.environ["TRL_OFFPOLICY_LN"] = "1" if add_ln else "0"               # the engines' opt-in switch for `add_ln` nets
    torch.manual_seed(0)
    net = dict(hidden_shapes=[H, H], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.ReLU,
               **({"add_ln": True} if add_ln else {}))
    pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=True, **net)
    qf1, qf2 = (networks.QNet(input_shape=D + A, output_shape=1, **net) for _ in range(2))

    class Stub:
        epoch_frames = 0

    class Log:
        def add_update_info(self, d): pass
        def add_epoch_info(self, *a, **k): pass
        def log(self, *a): pass
        def finish(self): pass
    agent = TwinSACQ(pf=pf, qf1=qf1, qf2=qf2, plr=3e-4, qlr=3e-4, policy_std_reg_weight=0, policy_mean_reg_weight=0,
                     reparameterization=True, automatic_entropy_tuning=True, noise_mode="device", env=SynthVecEnv(4, device=dev),
                     replay_buffer=None, collector=Stub(), logger=Log(), discount=0.99, num_epochs=1, batch_size=B, device=dev,
                     save_dir=None, tau=0.005, use_soft_update=True, opt_times=64)
    eng = agent.engine()
    st = eng.static_batch(B)
    st["obs"].normal_(), st["next_obs"].normal_(), st["rewards"].normal_()
    st["acts"].uniform_(-1, 1)
    handles = []

    def one():
        agent.training_update_num += 1
        handles.append(eng.enqueue(st))
        if len(handles) == 32:                                              # (the statistics ring holds 64 updates)
            eng.resolve(handles)
            handles.clear()
    us = timed(one, iters)
    infos = eng.resolve(handles) if handles else []
    print(json.dumps({"update": "TwinSACQ", "B": B, "D": D, "A": A, "H": H, "add_ln": bool(add_ln), "iters": iters,
                      "us_per_update": round(us, 2), "graphs": len(eng._graphs),
                      "finite": all(all(v == v for v in i.values()) for i in infos),
                      "note": "engine.enqueue on a fixed batch, one read-back of the statistics per 32 updates included"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="6x4096x256,4x4096x256")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--no-update", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for spec in args.groups.split(","):
        G, M, H = (int(v) for v in spec.split("x"))
        kernels(G, M, H, args.iters, dev)
    if not args.no_update:
        for add_ln in (False, True):
            update(add_ln, args.iters, dev)


if __name__ == "__main__":
    main()
