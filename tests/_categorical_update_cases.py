"""Seeded inputs of the fused categorical update's tests (tests/test_categorical_update_{cpu,gpu}.py) -- test
infrastructure.  Everything is generated on the CPU from numpy seeds, so the CPU test can state a condition on exactly
the inputs the GPU tests run: no sample's ratio exp(log pi - log pi_old) lies within RATIO_MARGIN of 1 +- clip (such a
sample may switch its gradient on or off between two fp32 implementations).  Where the first seed of a case put a sample
there, SEED_BUMP moves the case to its next seed without one."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _categorical_ref as ref                                                # noqa: E402

H = 64
CLIP, C_ENT = 0.2, 0.01
RATIO_MARGIN = 1e-4
# (D, A, activation): the issue's shapes; both activations on three of them
SHAPES = [(2, 2, "tanh"), (11, 3, "tanh"), (11, 3, "relu"), (17, 6, "tanh"), (17, 6, "relu"), (17, 8, "tanh"),
          (18, 2, "tanh"), (27, 8, "tanh"), (27, 8, "relu"), (32, 5, "tanh")]
# name -> (N, rows of the minibatch, workgroups): whole tiles in one time row (scalar tile addressing); B = 84 with a
# partial last tile (per-lane addressing); three workgroups per network, 3-4 tiles per wave; waves without a tile
LAYOUTS = {"contig": (16, 6, 2), "ragged": (12, 7, 2), "multi": (16, 40, 6), "empty": (16, 1, 2)}
LOSSES = [(ref.LOSS_PPO_CLIP, False), (ref.LOSS_PPO_CLIP, True), (ref.LOSS_A2C, False)]
GRAD_CASES = [(D, A, act, lay) for (D, A, act) in SHAPES for lay in LAYOUTS]
# the wide tile with ReLU on per-lane addressing at the smallest head -- a branch of the tile / activation / head dispatch
# no case above reaches: 24 envs (one full and one partial 16-sample tile per time row), 2 time rows
PARTIAL_LAYOUT = {"partial": (24, 2, 2)}
GRAD_CASES.append((18, 2, "relu", "partial"))
# the single-network launches: both tiles, both addressings
NET_CASES = [(17, 6, "tanh", "multi"), (27, 8, "relu", "ragged"), (11, 3, "tanh", "empty")]
# fused against generic engine: (D, A, seed)
ENGINE_CASES = [(11, 3, 31), (27, 8, 32)]
ENGINE_N, ENGINE_T, ENGINE_ROWS_MB = 16, 8, 2
# case id -> seeds skipped: the first seed(s) of these cases put a sample within RATIO_MARGIN of a clip edge
SEED_BUMP = {"D2_A2_tanh_contig": 1, "D11_A3_relu_multi": 2, "D17_A6_tanh_multi": 1, "D17_A8_tanh_multi": 1,
             "D18_A2_tanh_ragged": 1, "D27_A8_tanh_contig": 1}


def case_id(c):
    return "D%d_A%d_%s_%s" % c


def act_fn(act):
    return torch.tanh if act == "tanh" else torch.relu


def random_nets(rs, D, A):
    """([W1 b1 W2 b2 W3 b3] of the policy, the same of the value net), nn.Linear layout, float32."""
    def net(out, head_gain):
        sizes = [(H, D), (H, H), (out, H)]
        ps = []
        for k, (o, i) in enumerate(sizes):
            gain = head_gain if k == 2 else 1.0
            ps.append(torch.from_numpy((rs.randn(o, i) * gain / np.sqrt(i)).astype(np.float32)))
            ps.append(torch.from_numpy((rs.randn(o) * 0.1).astype(np.float32)))
        return ps
    return net(A, 3.0), net(1, 1.0)


def forward(params, x, act):
    h = x
    for k in range(3):
        h = h @ params[2 * k].t() + params[2 * k + 1]
        if k < 2:
            h = act_fn(act)(h)
    return h


def _grad_inputs(c, seed):
    D, A, act, lay = c
    N, rows, n_wg = dict(LAYOUTS, **PARTIAL_LAYOUT)[lay]
    rs = np.random.RandomState(seed)
    R = rows + 3                                                              # stored time rows; the minibatch takes `rows` of them
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    pf, vf = random_nets(rs, D, A)
    obs = t(R, N, D)
    acts = torch.from_numpy(rs.randint(0, A, size=(R, N, 1)).astype(np.float32))
    advs, rets, old_values = t(R, N, 1) * 2 + 0.5, t(R, N, 1), t(R, N, 1)
    noise = t(R, N, 1)
    row_idx = rs.permutation(R)[:rows].astype(np.int64)                       # shuffled
    with torch.no_grad():
        logits = forward(pf, obs.reshape(R * N, D), act)
        lp = ref.cat_logp(logits, acts.reshape(-1))[0].reshape(R, N, 1)
    old_logp = lp + 0.15 * noise                                              # ratios on both sides of the clip
    return dict(D=D, A=A, act=act, N=N, rows=rows, n_wg=n_wg, pf=pf, vf=vf, obs=obs, acts=acts, advs=advs, rets=rets,
                old_values=old_values, old_logp=old_logp, row_idx=row_idx, lp=lp)


def near_clip(lp, old_logp):
    """Samples whose ratio lies within RATIO_MARGIN of 1 - clip or 1 + clip."""
    ratio = torch.exp(lp - old_logp).reshape(-1)
    return int((((ratio - (1.0 - CLIP)).abs() <= RATIO_MARGIN) | ((ratio - (1.0 + CLIP)).abs() <= RATIO_MARGIN)).sum())


def grad_inputs(c):
    base = 7000 + 97 * GRAD_CASES.index(c)
    return _grad_inputs(c, base + SEED_BUMP.get(case_id(c), 0))


def minibatch(x):
    """The minibatch's samples of input set `x`, flattened in the kernel's order (row of row_idx, env)."""
    sel = lambda k: x[k][torch.from_numpy(x["row_idx"])].reshape(x["rows"] * x["N"], -1)
    return {k: sel(k) for k in ("obs", "acts", "advs", "rets", "old_values", "old_logp", "lp")}


def engine_inputs(c):
    """A stored rollout of ENGINE_T x ENGINE_N samples for the engine tests and three epochs of minibatch row indices;
    log pi_old is the restatement's log pi of the INITIAL nets (`nets_of(D, A, seed)`) plus small noise: ratios stay well
    inside the clip range while the policy takes its few steps, so the two engines take the same branch everywhere."""
    D, A, seed = c
    rs = np.random.RandomState(9000 + seed)
    T, N = ENGINE_T, ENGINE_N
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    obs = t(T, N, D)
    acts = torch.from_numpy(rs.randint(0, A, size=(T, N, 1)).astype(np.float32))
    advs, rets, old_values = t(T, N, 1) * 2 + 0.5, t(T, N, 1), t(T, N, 1)
    noise = t(T, N, 1)
    epochs = [np.stack(np.split(rs.permutation(T), T // ENGINE_ROWS_MB)).astype(np.int64) for _ in range(3)]
    return dict(D=D, A=A, seed=seed, obs=obs, acts=acts, advs=advs, rets=rets, old_values=old_values, noise=noise,
                epochs=epochs)


def nets_of(D, A, seed, act=torch.nn.Tanh, hidden=(64, 64)):
    from torchrl_amd import networks, policies
    torch.manual_seed(seed)
    net = dict(hidden_shapes=list(hidden), append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=act)
    pf = policies.CategoricalDisPolicy(input_shape=D, output_shape=A, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    return pf, vf


def linear_params(mod):
    return [p for l in (list(mod.base.seq_fcs) + list(mod.seq_append_fcs)) if isinstance(l, torch.nn.Linear)
            for p in (l.weight, l.bias)]


def engine_old_logp(x):
    """log pi_old of engine_inputs(x): the initial policy's log pi on the CPU restatement + 0.03 * noise."""
    pf, _ = nets_of(x["D"], x["A"], x["seed"])
    T, N = x["obs"].shape[:2]
    with torch.no_grad():
        logits = forward([p.detach() for p in linear_params(pf)], x["obs"].reshape(T * N, -1), "tanh")
        lp = ref.cat_logp(logits, x["acts"].reshape(-1))[0].reshape(T, N, 1)
    return lp, lp + 0.03 * x["noise"]
