"""Phase clocks of the two single-network gradient launches (policy chain / value chain) at the benchmark shape, from a
-DTRL_EXP_CLK build (TRL_LIB=<path to .so>): the fixed part of a launch -- set-up (split into load issue, load latency
and the work behind the loads), row sums + accumulator exchange ("images"), fold + row store -- next to the tile loop.
The stamps are those of wave 0 of every workgroup of the LAST update of each chain.  Development aid, not part of the
product.
    python torchrl_amd/build.py --exp clk -DTRL_EXP_CLK
    TRL_LIB=torchrl_amd/lib/libtrl_hip_clk.so python tools/time_grad_fixed.py"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402

LOOP = (9, 10, 1, 11, 12, 2, 14, 18, 19, 20, 21, 15, 16, 3, 17, 4, 5, 6)


def main():
    dev = torch.device("cuda:0")
    agent, col = bench.build_agent(dev, 1, 0)
    col.env.reset()
    col.rollout(col.sample_epoch_frames)
    agent.current_epoch = 0
    np.random.seed(0)
    agent.update_per_epoch()
    eng = agent.engine()
    buf = agent.replay_buffer
    t = {"obs": buf._obs, "acts": buf._acts, "advs": buf._advs, "rets": buf._estimate_returns,
         "old_values": buf._values, "old_logp": buf._old_logp}
    idx = np.stack([np.random.RandomState(e).permutation(128).reshape(4, 32) for e in range(10)]).reshape(40, 32).astype(np.int64)
    assert eng.two_chains, "the single-network launches belong to the two-chain route"
    for _ in range(4):
        eng.run(t, idx, buf.env_nums)
    torch.cuda.synchronize()
    n_wg, n_pf = eng._n_wg(32 * buf.env_nums)
    ps = eng.p_stride
    print("lib %s  policy launch %d workgroups, value launch %d" % (os.environ.get("TRL_LIB", "default"), n_pf, n_wg - n_pf))
    for net, part, n in (("policy", eng.partial, n_pf), ("value", eng._chain_rows[0], n_wg - n_pf)):
        c = part[:n, ps - 40: ps - 16].double().cpu().numpy()
        m = c.mean(axis=0)
        loop = sum(m[k] for k in LOOP)
        print("  %-6s wave-0 ticks (mean over workgroups): issue %.0f  latency %.0f  post-load %.0f  | loop %.0f | images %.0f  "
              "fold+store %.0f | total %.0f" % (net, m[22], m[23], m[0], loop, m[7], m[8], m.sum()), flush=True)
        print("         min/max over workgroups: issue %.0f/%.0f latency %.0f/%.0f post-load %.0f/%.0f images %.0f/%.0f fold %.0f/%.0f"
              % (c[:, 22].min(), c[:, 22].max(), c[:, 23].min(), c[:, 23].max(), c[:, 0].min(), c[:, 0].max(),
                 c[:, 7].min(), c[:, 7].max(), c[:, 8].min(), c[:, 8].max()), flush=True)


if __name__ == "__main__":
    main()
