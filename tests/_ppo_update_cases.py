"""Seeded inputs of the shared-std PPO update kernels' tests (tests/test_ppo_update_kernels_{cpu,gpu}.py) -- test
infrastructure.  Everything is generated on the CPU from numpy seeds, so the CPU file can state its conditions on exactly
the inputs the GPU file runs, in float64 on the restatement (tests/_ppo_update_ref.py), over the minibatch's samples:

  * no ratio exp(log pi - log pi_old) within RATIO_MARGIN of 1 +- clip; for B >= 64 at least 10 % of the samples clipped
    on each side (log pi_old = log pi + 0.3 N(0, 1));
  * no |v - v_old| within VCLIP_MARGIN of clip; for B >= 64 at least 10 % beyond it on each side (v_old = v + 0.3 N(0, 1));
    the tie cases sit on the 1/8 grid by design and are exempt;
  * tanh actions have |a| <= 0.995;
  * ReLU nets: no hidden pre-activation within RELU_MARGIN of zero.

A case that fails one moves to its next seed; SEED_BUMP records how many seeds it skipped (at most MAX_BUMP).  No sample is
ever dropped from a comparison."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_ref as gr                                                       # noqa: E402
import _ppo_update_ref as ref                                                 # noqa: E402

H = 64
CLIP, TIE_CLIP, C_ENT = 0.2, 0.25, 0.01
RATIO_MARGIN, VCLIP_MARGIN = 1e-4, 1e-4
# 4 x the largest |z_float32 - z_float64| over the hidden pre-activations of every ReLU case, measured by
# tests/test_ppo_update_kernels_cpu.py::test_relu_margin (1.08e-6 on the CPU), rounded up
RELU_MARGIN = 4.4e-6
MAX_BUMP = 8
# The constants of the bounds: the smallest powers of two for which the restatement's float32 run on the CPU stays under a
# quarter of the bound on every element of every case (tests/test_ppo_update_kernels_cpu.py measures and asserts them).
# K_W: weights and biases of the gradient, K_LS: d_logstd; K_M, K_V, K_P: Adam's moments and the update part of the parameter
# bound; K_R = 4 is not measured: one rounding of the subtraction, u |param|, at the same margin.
K_W, K_LS = 128.0, 32.0
K_M, K_V, K_P, K_R = 16.0, 16.0, 16.0, 4.0
LS_HIGH, LS_LOW = 3.0, -25.0
# name -> (N, rows of the minibatch, n_wg, n_wg_pf); every stored buffer has rows + 3 time rows, row_idx is a shuffled subset of rows 1..
LAYOUTS = {
    "contig1": (16, 6, 2, 0),       # one tile per row
    "cols": (48, 11, 4, 0),         # 3 tiles per row, 33 tiles, stride 8: row step 2, column step 2, the column wraps
    "longrow": (160, 2, 2, 0),      # 10 tiles per row, stride 4: a wave walks across the row boundary
    "ragged": (12, 7, 2, 0),        # per-lane addressing, partial last tile
    "partial": (24, 2, 2, 0),       # a full and a partial tile per row
    "empty": (16, 1, 2, 0),         # three waves per network without a tile
    "uneven": (48, 11, 5, 3),       # odd n_wg, explicit split
    "tiny": (1, 2, 2, 0),           # B = 2
}
RT_SHAPES = [(17, 8, "tanh"), (16, 6, "relu"), (11, 3, "tanh"), (2, 1, "tanh"), (18, 2, "relu"), (27, 8, "tanh"), (32, 5, "tanh")]
LOSSES = [(gr.LOSS_PPO_CLIP, False), (gr.LOSS_PPO_CLIP, True), (gr.LOSS_A2C, False)]
# (D, A, activation, layout, kind); kind: plain | notanh (tanh_action = 0) | clamp | shard | tie
PLAIN_CASES = ([(17, 6, "tanh", lay, "plain") for lay in LAYOUTS]
               + [(17, 6, "relu", lay, "plain") for lay in ("cols", "ragged")]
               + [(D, A, act, lay, "plain") for (D, A, act) in RT_SHAPES for lay in ("cols", "ragged")]
               + [(18, 2, "relu", "partial", "plain"), (2, 1, "tanh", "tiny", "plain")])
NOTANH_CASES = [(17, 6, "tanh", "cols", "notanh"), (11, 3, "tanh", "ragged", "notanh")]
CLAMP_CASES = [(17, 6, "tanh", "cols", "clamp"), (11, 3, "tanh", "ragged", "clamp")]
SHARD_CASES = [(17, 6, "tanh", "cols", "shard"), (27, 8, "tanh", "ragged", "shard")]
TIE_CASES = [(17, 6, "tanh", "contig1", "tie"), (11, 3, "tanh", "ragged", "tie")]
GRAD_CASES = PLAIN_CASES + NOTANH_CASES + CLAMP_CASES + SHARD_CASES + TIE_CASES
WG_CASE = (17, 6, "tanh", "cols", "plain")
WG_SPLITS = [(2, 0), (5, 3), (16, 0)]
CHAIN_CASES = [(17, 6, "tanh", "cols", "plain"), (11, 3, "tanh", "ragged", "plain")]
# case id -> seeds skipped (see the module docstring)
SEED_BUMP = {"D17_A6_tanh_cols": 2, "D16_A6_relu_ragged": 1, "D11_A3_tanh_cols": 1, "D18_A2_relu_cols": 3,
             "D32_A5_tanh_ragged": 1}

# ---- the fold on synthetic rows: (n_wg, n_pf) -> 1, 2, 8, 9, 109, 128, 129, 147, 192 and 193 rows per network (the last two
# splits put a network exactly AT fold_rows_wave's 128 rows per round and fold_scalar_stats' 192)
FOLD_SHAPES = [(17, 6), (27, 8)]
FOLD_SPLITS = [(2, 1), (3, 1), (9, 8), (17, 9), (130, 129), (256, 147), (258, 129), (386, 193), (256, 128), (384, 192)]
# ---- clip + Adam
ADAM_LAYOUTS = [(1,), (255, 257), (2047, 0, 2049), (5708, 5377), (4097, 3, 64, 8192), (32768,), (32769,)]
ADAM_NORMS = [("big", 0.5), ("small", 0.5), ("big", 0.0)]     # (gradient scale, max_norm): norm >> 0.5, norm << 0.5, no clip
ADAM_SCALES, ADAM_STEPS = (1.0, 0.5), (1, 2, 1000)
ADAM_LRS = (3e-4, 1e-3, 2.5e-4, 7e-4)
TICK_SIZES = [32768, 32769]                                   # 128 blocks: the last block ticks; 129: the tick launch
POLYAK_BIG = 262144 + 7                                       # more than 1024 blocks of 256: the grid-stride loop


def case_id(c):
    return "D%d_A%d_%s_%s%s" % (c[0], c[1], c[2], c[3], "" if c[4] == "plain" else "_" + c[4])


def clamp_columns(A):
    """(the column clamped above, the column clamped below) of a clamp case."""
    return A - 1, 0


def p_sizes(D, A):
    return 64 * D + 64 + 4096 + 64 + 64 * A + 2 * A, 64 * D + 64 + 4096 + 64 + 64 + 1


def random_nets(rs, D, A):
    """([W1 b1 W2 b2 W3 b3] of the policy, the same of the value net), nn.Linear layout, float32."""
    def net(out):
        ps = []
        for (o, i) in [(H, D), (H, H), (out, H)]:
            ps.append(torch.from_numpy((rs.randn(o, i) / np.sqrt(i)).astype(np.float32)))
            ps.append(torch.from_numpy((rs.randn(o) * 0.1).astype(np.float32)))
        return ps
    return net(A), net(1)


def _grad_inputs(c, seed):
    D, A, act, lay, kind = c
    N, rows, n_wg, n_wg_pf = LAYOUTS[lay]
    tanh = kind not in ("notanh", "clamp")
    clip = TIE_CLIP if kind == "tie" else CLIP
    rs = np.random.RandomState(seed)
    R = rows + 3                                                              # stored time rows; the minibatch takes `rows` of them
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    pf, vf = random_nets(rs, D, A)
    logstd = torch.from_numpy(rs.uniform(-1.5, 0.5, (A,)).astype(np.float32))
    obs = t(R, N, D)
    eps = t(R * N, A)
    advs, rets = t(R, N, 1) * 2 + 0.5, t(R, N, 1)
    noise_lp, noise_v = t(R, N, 1), t(R, N, 1)
    extra = t(2 * rows * N) * 2 + 0.5                                         # shard: the other two thirds of the population
    # shuffled, and never stored row 0: lanes and tiles past the end of the minibatch read cell 0, which the GPU file fills
    # with NaN like every other stored row outside the minibatch
    row_idx = (1 + rs.permutation(R - 1)[:rows]).astype(np.int64)
    if kind == "clamp":
        hi, lo = clamp_columns(A)
        logstd[hi], logstd[lo] = LS_HIGH, LS_LOW
        pf[4][lo] = 0.0                                                       # its mean is the bias, exactly
    if kind == "tie":
        vf[4][:] = 0.0                                                        # v = b3 exactly, in any arithmetic
        vf[5][:] = 0.5
    flat_obs = obs.reshape(R * N, D)
    with torch.no_grad():
        mean = ref.layers(pf, flat_obs, act)[0]
        acts = gr.explore(mean, logstd, eps, tanh)[0]                         # drawn from the head itself
        if tanh:
            acts = acts.clamp(-0.995, 0.995)
        if kind == "clamp":
            acts[:, clamp_columns(A)[1]] = pf[5][clamp_columns(A)[1]]
        acts = acts.contiguous()
        mean64 = ref.layers([p.double() for p in pf], flat_obs.double(), act)[0]
        v64 = ref.layers([p.double() for p in vf], flat_obs.double(), act)[0]
        lp = gr.logp(mean64, logstd.double(), acts.double(), tanh).reshape(R, N, 1)
    old_logp = (lp + 0.3 * noise_lp.double()).float()                         # about a quarter of the samples clipped on each side
    old_values = (v64.reshape(R, N, 1) + 0.3 * noise_v.double()).float()
    if kind == "tie":
        tie = gr.value_tie_case(TIE_CLIP)
        k = torch.arange(R * N) % len(tie["v"])                               # the grid rows, shifted so that their v is b3
        old_values = (tie["v_old"][k] - tie["v"][k] + 0.5).reshape(R, N, 1)
        rets = (tie["rets"][k] - tie["v"][k] + 0.5).reshape(R, N, 1)
    x = dict(D=D, A=A, act=act, N=N, rows=rows, n_wg=n_wg, n_wg_pf=n_wg_pf, tanh=tanh, kind=kind, clip=clip, pf=pf, vf=vf,
             logstd=logstd, obs=obs, acts=acts.reshape(R, N, A), advs=advs, rets=rets, old_values=old_values,
             old_logp=old_logp, row_idx=row_idx, seed=seed)
    mb_advs = advs[torch.from_numpy(row_idx)].reshape(-1)
    B = rows * N
    if kind == "shard":                                                       # the launch sees the middle third of 3 B advantages
        x["adv_raw"] = gr.adv_raw_of(torch.cat([extra[:B], mb_advs, extra[B:]]))
        x["n_global"] = float(3 * B)
    else:
        x["adv_raw"], x["n_global"] = gr.adv_raw_of(mb_advs), float(B)
    return x


def minibatch(x):
    """The minibatch's samples of input set `x`, flattened in the kernel's order (row of row_idx, env)."""
    sel = lambda k: x[k][torch.from_numpy(x["row_idx"])].reshape(x["rows"] * x["N"], -1)
    return {k: sel(k) for k in ("obs", "acts", "advs", "rets", "old_values", "old_logp")}


def conditions(x):
    """-> list of the violated input conditions of the module docstring (empty: all hold), float64."""
    mb = minibatch(x)
    B, clip, bad = x["rows"] * x["N"], x["clip"], []
    obs = mb["obs"].double()
    mean, _, pz = ref.layers([p.double() for p in x["pf"]], obs, x["act"])
    v, _, vz = ref.layers([p.double() for p in x["vf"]], obs, x["act"])
    lp = gr.logp(mean, x["logstd"].double(), mb["acts"].double(), x["tanh"])
    if not bool(torch.isfinite(lp).all()):
        bad.append("log pi not finite")
    ratio = torch.exp(lp - mb["old_logp"].double().reshape(-1))
    if bool((((ratio - (1 - clip)).abs() <= RATIO_MARGIN) | ((ratio - (1 + clip)).abs() <= RATIO_MARGIN)).any()):
        bad.append("a ratio within %g of a clip boundary" % RATIO_MARGIN)
    if B >= 64:
        lo, hi = int((ratio < 1 - clip).sum()), int((ratio > 1 + clip).sum())
        if lo < 0.1 * B or hi < 0.1 * B:
            bad.append("clipped %d below, %d above of %d" % (lo, hi, B))
    if x["kind"] != "tie":
        d = v.reshape(-1) - mb["old_values"].double().reshape(-1)
        if bool(((d.abs() - clip).abs() <= VCLIP_MARGIN).any()):
            bad.append("|v - v_old| within %g of clip" % VCLIP_MARGIN)
        if B >= 64:
            lo, hi = int((d < -clip).sum()), int((d > clip).sum())
            if lo < 0.1 * B or hi < 0.1 * B:
                bad.append("value clip: %d below, %d above of %d" % (lo, hi, B))
    if x["tanh"] and float(mb["acts"].abs().max()) > float(np.float32(0.995)):
        bad.append("|a| > 0.995")
    if x["act"] == "relu":
        z = torch.cat([t.reshape(-1) for t in pz[:2] + vz[:2]])
        if float(z.abs().min()) <= RELU_MARGIN:
            bad.append("a hidden pre-activation within %g of zero" % RELU_MARGIN)
    return bad


def base_seed(c):
    return 9100 + 97 * GRAD_CASES.index(c)


def grad_inputs(c):
    return _grad_inputs(c, base_seed(c) + SEED_BUMP.get(case_id(c), 0))


# ------------------------------------------------------------------ the fold on synthetic rows
def fold_case(D, A, n_wg, n_pf, stride, seed):
    """partial (n_wg + 3, stride) float32 and scal_partial (n_wg + 3, 8) float64, filled directly: magnitudes 1e-3 .. 1e3
    with mixed signs; NaN in every pad column >= P_pf (policy rows) / P_vf (value rows), in every row >= n_wg and in the
    scalar rows' eighth column, which the Gaussian's fold does not read."""
    rs = np.random.RandomState(seed)
    rows = n_wg + 3
    part = (10.0 ** rs.uniform(-3, 3, (rows, stride)) * rs.choice([-1.0, 1.0], (rows, stride))).astype(np.float32)
    scal = 10.0 ** rs.uniform(-3, 3, (rows, 8)) * rs.choice([-1.0, 1.0], (rows, 8))
    p_pf, p_vf = p_sizes(D, A)
    part[:n_pf, p_pf:] = np.nan
    part[n_pf:n_wg, p_vf:] = np.nan
    part[n_wg:] = np.nan
    scal[n_wg:] = np.nan
    scal[:, 7] = np.nan
    logstd = rs.uniform(-1.5, 0.5, (A,)).astype(np.float32)
    return torch.from_numpy(part), torch.from_numpy(scal), torch.from_numpy(logstd)


def fold_info(scal, n_wg, n_pf, logstd):
    """The info row of the fold from the scalar rows (float64 numpy): policy rows -> slots 0..6, value rows -> 7, 12..15,
    the log-std tail -> 8..11, 16..19 (None: left alone); everything else keeps the sentinel."""
    s = scal.numpy()
    p, v = s[:n_pf], s[n_pf:n_wg]
    info = np.full(24, ref.SENTINEL)
    info[0:7] = [p[:, 6].sum(), p[:, 0].sum(), p[:, 1].sum(), p[:, 2].max(), p[:, 3].max(), p[:, 4].max(), p[:, 5].max()]
    info[7] = v[:, 6].sum()
    info[12:16] = [v[:, 0].sum(), v[:, 1].sum(), v[:, 2].max(), v[:, 3].max()]
    if logstd is not None:
        x = np.clip(logstd.double().numpy(), -20.0, 2.0)
        for base, t in ((8, x), (16, np.exp(x))):
            info[base:base + 4] = [t.mean(), t.std(ddof=1) if len(t) > 1 else np.nan, t.max(), t.min()]
    return info


FOLD_SUMS, FOLD_EXACT = (0, 1, 2, 7, 12, 13), (3, 4, 5, 6, 14, 15)


# ------------------------------------------------------------------ clip + Adam
def adam_case(sizes, kind, seed, zero_group=None):
    """Parameters 0.1 N(0, 1), non-trivial moments (m 1e-3 N(0, 1), v 1e-5 (0.1 + U)), gradients N(0, 1) x 10 ("big": every
    non-empty group's norm >> 0.5) or x 1e-4 ("small": << 0.5); zero_group: that group's gradient is all zero."""
    rs = np.random.RandomState(seed)
    n = int(sum(sizes))
    f = lambda a: a.astype(np.float32)
    p, m, v = f(rs.randn(n) * 0.1), f(rs.randn(n) * 1e-3), f((rs.rand(n) + 0.1) * 1e-5)
    g = f(rs.randn(n) * (10.0 if kind == "big" else 1e-4))
    if zero_group is not None:
        off = np.concatenate([[0], np.cumsum(sizes)])
        g[off[zero_group]:off[zero_group + 1]] = 0.0
    return dict(p=p, m=m, v=v, g=g)


def adam_combos(sizes):
    """(gradient kind, max_norm, grad_scale, step_count, group with an all-zero gradient or None) of the single-step checks:
    the cross product, and one combination with a zero gradient in a non-empty group."""
    out = [(kind, max_norm, gs, count, None) for kind, max_norm in ADAM_NORMS for gs in ADAM_SCALES for count in ADAM_STEPS]
    full = [k for k, n in enumerate(sizes) if n > 0]
    return out + [("big", 0.5, 1.0, 2, full[-1])]


def chain_steps(n, n_groups, steps=5, seed=23):
    """A chain on the device-resident state: step_count None, the learning rates change between launches."""
    return [(g, lrs, 0.5, 1.0, None) for g, lrs in zip(chain_grads(n, steps, seed), chain_lrs(steps, n_groups))]


def chain_grads(n, steps, seed):
    """`steps` gradients for a chain of updates: alternately large (clipped) and small."""
    rs = np.random.RandomState(seed)
    return [(rs.randn(n) * (10.0 if k % 2 else 1e-3)).astype(np.float32) for k in range(steps)]


def chain_lrs(steps, n_groups):
    """The learning rates of launch k, changed between launches (a linear schedule's)."""
    return [[np.float32(ADAM_LRS[g] * (1.0 - 0.1 * k)) for g in range(n_groups)] for k in range(steps)]
