"""Seeded inputs of the fused state-dependent-std update's tests (tests/test_gauss_sd_update_{cpu,gpu}.py) -- test
infrastructure.  Everything is generated on the CPU from numpy seeds, so the CPU test can state its conditions on exactly
the inputs the GPU tests run (checked on the float64 restatement, tests/_gauss_sd_ref.py):

  * no sample's ratio exp(log pi - log pi_old) lies within RATIO_MARGIN of 1 +- clip (such a sample may switch its gradient
    on or off between two fp32 implementations);
  * no raw log_std element lies within LS_MARGIN of -20 or 2 (the clamp's gate would be such a switch too);
  * the "clamp" cases have one whole log_std column at +3 (at least 10 % of the elements, well beyond the upper clamp) and
    one whole column at -25 (one column of every row below the lower clamp).

Where the first seed of a case violates a condition, SEED_BUMP moves the case to its next seed that does not.

A column clamped at -20 has std = e^-20: log pi is finite only where the action equals the mean to ~1e-9, which no two
implementations of the layers agree on.  The clamp cases therefore give that column's MEAN row zero weights as well (mean =
its bias, exactly, in every arithmetic), store the action equal to it and use plain (not tanh) actions."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_sd_ref as ref                                                   # noqa: E402
from _categorical_update_cases import LAYOUTS, PARTIAL_LAYOUT, act_fn, forward, linear_params  # noqa: E402,F401

H = 64
CLIP, C_ENT = 0.2, 0.01
RATIO_MARGIN, LS_MARGIN = 1e-4, 1e-3
LS_HIGH, LS_LOW = 3.0, -25.0
# (D, A, activation): the issue's shapes; both activations on two of them
SHAPES = [(2, 1, "tanh"), (11, 3, "tanh"), (11, 3, "relu"), (17, 6, "tanh"), (17, 8, "tanh"), (18, 2, "tanh"),
          (27, 8, "tanh"), (27, 8, "relu"), (32, 5, "tanh")]
LOSSES = [(ref.LOSS_PPO_CLIP, False), (ref.LOSS_PPO_CLIP, True), (ref.LOSS_A2C, False)]
# (D, A, activation, layout, clamp): every shape x layout with log_std inside the clamp, tanh actions
PLAIN_CASES = [(D, A, act, lay, False) for (D, A, act) in SHAPES for lay in LAYOUTS]
# ... and the clamp cases: both tiles, both addressings, a full tile (A = 8), waves without a tile
CLAMP_CASES = [(11, 3, "tanh", "ragged", True), (17, 6, "tanh", "empty", True), (17, 8, "tanh", "multi", True),
               (27, 8, "relu", "contig", True), (32, 5, "tanh", "multi", True), (18, 2, "tanh", "ragged", True)]
# the wide tile with ReLU on per-lane addressing (24 envs x 2 time rows, _categorical_update_cases.PARTIAL_LAYOUT) at the
# smallest and the largest head: branches of the tile / activation / head dispatch no case above reaches
PARTIAL_CASES = [(18, 1, "relu", "partial", False), (18, 8, "relu", "partial", False)]
GRAD_CASES = PLAIN_CASES + CLAMP_CASES + PARTIAL_CASES
# the single-network launches: both tiles, both addressings, a clamp case among them
NET_CASES = [(17, 6, "tanh", "multi", False), (27, 8, "relu", "ragged", False), (11, 3, "tanh", "empty", False),
             (17, 8, "tanh", "multi", True)]
# fused against generic engine: (D, A, seed)
ENGINE_CASES = [(11, 3, 31), (27, 8, 32)]
ENGINE_N, ENGINE_T, ENGINE_ROWS_MB = 16, 8, 2
# case id -> seeds skipped (see the module docstring)
SEED_BUMP = {"D11_A3_tanh_multi": 1, "D18_A2_tanh_multi": 1, "D27_A8_tanh_multi": 4, "D27_A8_tanh_empty": 1,
             "D17_A8_tanh_multi_clamp": 1, "D32_A5_tanh_multi_clamp": 1}


def case_id(c):
    return "D%d_A%d_%s_%s%s" % (c[0], c[1], c[2], c[3], "_clamp" if c[4] else "")


def clamp_columns(A):
    """(the column clamped above, the column clamped below) of a clamp case."""
    return A - 1, 0


def random_nets(rs, D, A, clamp):
    """([W1 b1 W2 b2 W3 b3] of the policy with its 2A head rows [mean | log_std], the same of the value net), nn.Linear
    layout, float32.  Raw log_std = -0.5 +- ~0.4 (inside the clamp, far from its edges)."""
    def net(out):
        ps = []
        for k, (o, i) in enumerate([(H, D), (H, H), (out, H)]):
            ps.append(torch.from_numpy((rs.randn(o, i) / np.sqrt(i)).astype(np.float32)))
            ps.append(torch.from_numpy((rs.randn(o) * 0.1).astype(np.float32)))
        return ps
    pf, vf = net(2 * A), net(1)
    pf[4][A:] *= 0.5
    pf[5][A:] -= 0.5
    if clamp:
        hi, lo = clamp_columns(A)
        pf[4][A + hi] = 0.0
        pf[5][A + hi] = LS_HIGH
        pf[4][A + lo] = 0.0
        pf[5][A + lo] = LS_LOW
        pf[4][lo] = 0.0                                                       # its mean is the bias, exactly
    return pf, vf


def _grad_inputs(c, seed):
    D, A, act, lay, clamp = c
    N, rows, n_wg = dict(LAYOUTS, **PARTIAL_LAYOUT)[lay]
    tanh = not clamp
    rs = np.random.RandomState(seed)
    R = rows + 3                                                              # stored time rows; the minibatch takes `rows` of them
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    pf, vf = random_nets(rs, D, A, clamp)
    obs = t(R, N, D)
    eps = t(R * N, A)
    advs, rets, old_values = t(R, N, 1) * 2 + 0.5, t(R, N, 1), t(R, N, 1)
    noise = t(R, N, 1)
    row_idx = rs.permutation(R)[:rows].astype(np.int64)                       # shuffled
    with torch.no_grad():
        head = forward(pf, obs.reshape(R * N, D), act)
        acts = ref.explore(head, eps, tanh)[0]                               # drawn from the head itself
        if tanh:
            acts = acts.clamp(-0.995, 0.995)
        if clamp:
            acts[:, clamp_columns(A)[1]] = pf[5][clamp_columns(A)[1]]
        acts = acts.contiguous()
        head64 = forward([p.double() for p in pf], obs.reshape(R * N, D).double(), act)
        lp = ref.logp(head64, acts.double(), tanh)[0].reshape(R, N, 1)
    old_logp = (lp + 0.15 * noise.double()).float()                           # ratios on both sides of the clip
    return dict(D=D, A=A, act=act, N=N, rows=rows, n_wg=n_wg, tanh=tanh, clamp=clamp, pf=pf, vf=vf, obs=obs,
                acts=acts.reshape(R, N, A), advs=advs, rets=rets, old_values=old_values, old_logp=old_logp, row_idx=row_idx,
                lp=lp, raw_ls=head64[:, A:].reshape(R, N, A))


def near_clip(lp, old_logp):
    """Samples whose ratio lies within RATIO_MARGIN of 1 - clip or 1 + clip."""
    ratio = torch.exp(lp.double() - old_logp.double()).reshape(-1)
    return int((((ratio - (1.0 - CLIP)).abs() <= RATIO_MARGIN) | ((ratio - (1.0 + CLIP)).abs() <= RATIO_MARGIN)).sum())


def near_clamp(raw_ls):
    """Raw log_std elements within LS_MARGIN of -20 or 2."""
    return int((((raw_ls + 20.0).abs() <= LS_MARGIN) | ((raw_ls - 2.0).abs() <= LS_MARGIN)).sum())


def grad_inputs(c):
    base = 7000 + 97 * GRAD_CASES.index(c)
    return _grad_inputs(c, base + SEED_BUMP.get(case_id(c), 0))


def minibatch(x):
    """The minibatch's samples of input set `x`, flattened in the kernel's order (row of row_idx, env)."""
    sel = lambda k: x[k][torch.from_numpy(x["row_idx"])].reshape(x["rows"] * x["N"], -1)
    return {k: sel(k) for k in ("obs", "acts", "advs", "rets", "old_values", "old_logp", "lp", "raw_ls")}


def engine_inputs(c):
    """A stored rollout of ENGINE_T x ENGINE_N samples for the engine tests and three epochs of minibatch row indices;
    log pi_old is the restatement's log pi of the INITIAL nets (`nets_of(D, A, seed)`) plus small noise: ratios stay well
    inside the clip range while the policy takes its few steps, so the two engines take the same branch everywhere."""
    D, A, seed = c
    rs = np.random.RandomState(9000 + seed)
    T, N = ENGINE_T, ENGINE_N
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    obs = t(T, N, D)
    acts = (t(T, N, A) * 0.5).clamp(-0.995, 0.995)
    advs, rets, old_values = t(T, N, 1) * 2 + 0.5, t(T, N, 1), t(T, N, 1)
    noise = t(T, N, 1)
    epochs = [np.stack(np.split(rs.permutation(T), T // ENGINE_ROWS_MB)).astype(np.int64) for _ in range(3)]
    return dict(D=D, A=A, seed=seed, obs=obs, acts=acts, advs=advs, rets=rets, old_values=old_values, noise=noise,
                epochs=epochs)


def nets_of(D, A, seed, act=torch.nn.Tanh, hidden=(64, 64), tanh=True):
    from torchrl_amd import networks, policies
    torch.manual_seed(seed)
    net = dict(hidden_shapes=list(hidden), append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=act)
    pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=tanh, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    return pf, vf


def engine_old_logp(x):
    """(log pi, log pi_old) of engine_inputs(x): the initial policy's log pi on the CPU restatement, + 0.03 * noise."""
    pf, _ = nets_of(x["D"], x["A"], x["seed"])
    T, N = x["obs"].shape[:2]
    with torch.no_grad():
        head = forward([p.detach() for p in linear_params(pf)], x["obs"].reshape(T * N, -1), "tanh")
        lp = ref.logp(head, x["acts"].reshape(T * N, -1), True)[0].reshape(T, N, 1)
    return lp, lp + 0.03 * x["noise"]
