#!/usr/bin/env python
"""Time trl_layernorm_fwd_f32 / trl_layernorm_bwd_f32 with device events and print them beside their HBM-byte floor.

    python tools/time_layernorm.py [--shapes 65536x64,8192x256] [--iters 200]

Bytes a pass has to move (fp32): forward reads a and writes y (8 M H) plus the (M, 2) statistics; backward reads dy and a,
writes dz (12 M H), reads the statistics and writes / re-reads its dgamma / dbeta slabs.  The floor is those bytes over the
6.3 TB/s a float4 copy reaches on an MI355X; the backward figure is both of its launches (rows, then the slab fold).
One JSON line per shape."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x64,8192x256")
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for shape in args.shapes.split(","):
        M, H = (int(v) for v in shape.split("x"))
        a = torch.tanh(torch.randn(M, H, device=dev))
        dy = torch.randn(M, H, device=dev)
        gamma, beta = 1 + 0.3 * torch.randn(H, device=dev), 0.2 * torch.randn(H, device=dev)
        y, stats = _C.layernorm_fwd(a, gamma, beta)
        dz, dg, db = torch.empty_like(a), torch.empty(H, device=dev), torch.empty(H, device=dev)
        ws = torch.empty(_C.lib().trl_layernorm_bwd_workspace(M, H), device=dev)
        fwd = timed(lambda: _C.layernorm_fwd(a, gamma, beta, y=y, stats=stats), args.iters)
        bwd = timed(lambda: _C.layernorm_bwd(dy, a, stats, gamma, _C.ACT_TANH, dg, db, dz=dz, workspace=ws), args.iters)
        fwd_bytes = 8 * M * H + 8 * M + 8 * H
        bwd_bytes = 12 * M * H + 8 * M + 4 * H + 2 * 4 * ws.numel() + 8 * H
        print(json.dumps({"M": M, "H": H, "iters": args.iters,
                          "fwd_us": round(fwd, 2), "fwd_floor_us": round(fwd_bytes / HBM_BYTES_PER_S * 1e6, 2),
                          "bwd_us": round(bwd, 2), "bwd_floor_us": round(bwd_bytes / HBM_BYTES_PER_S * 1e6, 2),
                          "note": "device events around back-to-back calls: launch gaps included"}))


if __name__ == "__main__":
    main()
