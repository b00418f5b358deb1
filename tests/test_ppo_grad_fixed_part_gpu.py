"""The fixed part of ppo_grad_wave_kernel behind its tile loop (torchrl_amd/csrc/k_ppo.hip): the four waves exchange
their accumulators in register layout, every wave folds the slots it owns and stores them straight into the partial row.

1. The cross-wave order is ((w0 + w1) + w2) + w3.  A ReLU value net whose every product is exact -- W1 = 0, b1 = b2 = 1,
   W2 = 0 but for W2[0][0] = 1, w3 = e_0, b3 = 0, observations of ones, n_global = 64 -- on four tiles (N = 16, 4 rows:
   one per wave) in each of which ONE sample has a return other than v = 2: the waves' d_v are (1, 2^-24, 2^-24, -1) / 16,
   and every gradient slot the value net fills is a power of two times d_v.  The stored float32 has to be the left-to-right
   sum (0); pairwise gives 2^-24 / 16, reversed 2^-23 / 16.  (With W2 all zero dZ1 would be zero, and dW1 with its 17th
   column could not tell any order from another, so ONE entry of W2 is 1: dZ1[0] = dZ2[0].)  A second order of the
   same four tiles, (2^-24, 2^-24, 1, -1), has a non-zero answer in the kernel's order (2^-23 / 16): the slots really
   receive the contributions.
2. Every float of the row is written once and waves without a tile fold as zeros: NaN-prefilled rows, N = 16 x 2 rows (waves
   2 and 3 idle) and N = 24 x 3 rows (per-lane addressing, a ragged fifth tile), one workgroup per network, for the Gaussian
   <17, 64, 6>, runtime dims (11, 3), the wide tile (27, 8), the categorical and the state-dependent-std head -- each
   against float64 within the bounds of its own kernel test (test_ppo_update_kernels_gpu.py: K u M_e + floor_e per element
   and 1e-4 of a block's largest entry; the categorical / SD files: 1e-4 of the network's largest entry)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _categorical_ref as cref                                               # noqa: E402
import _categorical_update_cases as cu                                        # noqa: E402
import _gauss_ref as gr                                                       # noqa: E402
import _gauss_sd_ref as sref                                                  # noqa: E402
import _gauss_sd_update_cases as su                                           # noqa: E402
import _ppo_update_cases as pc                                                # noqa: E402
import _ppo_update_ref as ref                                                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H = 64
NAN = float("nan")
# name -> (N, rows of the minibatch); one workgroup per network (n_wg = 2, n_wg_pf = 1)
SHAPES = {"idle": (16, 2), "ragged5": (24, 3)}
LOSS = (gr.LOSS_PPO_CLIP, True)


def dev(x, dtype=None):
    t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def adv_raw_of(advs):
    a = advs.double().reshape(-1)
    return torch.tensor([a.sum(), (a * a).sum(), a.max(), -a.min()], dtype=torch.float64)


def launch(x, flat, P_pf, head, loss_mode, clipv, raw, n_global, clip, c_ent):
    """One gradient launch (one workgroup per network) and its fold on NaN-filled buffers -> (grads, partial) on the host."""
    from torchrl_amd import _C
    grad_fn, reduce_fn, stride_fn = {"gauss": (_C.ppo_minibatch_grad, _C.ppo_reduce, _C.ppo_partial_stride),
                                     "cat": (_C.ppo_cat_minibatch_grad, _C.ppo_cat_reduce, _C.ppo_cat_partial_stride),
                                     "sd": (_C.ppo_sd_minibatch_grad, _C.ppo_sd_reduce, _C.ppo_sd_partial_stride)}[head]
    D, A = x["D"], x["A"]
    ps = stride_fn(D, H, A)
    sw = _C.ppo_sd_scalar_stride() if head == "sd" else 8
    t = {k: dev(x[k]) for k in ("obs", "acts", "advs", "rets", "old_values", "old_logp")}
    row_idx, raw_d, flat_d = dev(x["row_idx"]), dev(raw, torch.float64), dev(flat)
    partial = torch.full((2, ps), NAN, device=DEV)
    scal = torch.full((2 * sw,), NAN, dtype=torch.float64, device=DEV)
    grads = torch.full((flat_d.numel(),), NAN, device=DEV)
    info = torch.zeros(24, dtype=torch.float64, device=DEV)
    g = _C.PpoBatchArgs()
    for k, v in t.items():
        setattr(g, k, v.data_ptr())
    if loss_mode != gr.LOSS_PPO_CLIP:
        g.old_logp = None
    if not clipv:
        g.old_values = None
    g.row_idx, g.rows_mb, g.N = row_idx.data_ptr(), x["rows"], x["N"]
    g.adv_raw, g.n_global = raw_d.data_ptr(), float(n_global)
    g.pf_params, g.vf_params = flat_d.data_ptr(), flat_d.data_ptr() + 4 * P_pf
    g.D, g.H, g.A, g.act = D, H, A, (_C.ACT_TANH if x["act"] == "tanh" else _C.ACT_RELU)
    g.clip_para, g.entropy_coeff, g.clipped_value_loss, g.tanh_action = clip, c_ent, int(clipv), int(x.get("tanh", True))
    g.loss_mode = loss_mode
    g.partial, g.scal_partial, g.n_wg, g.n_wg_pf = partial.data_ptr(), scal.data_ptr(), 2, 1
    grad_fn(g, DEV)
    if head == "gauss":
        reduce_fn(partial, scal, 2, D, H, A, grads, info, pf_params=flat_d, n_wg_pf=1)
    else:
        reduce_fn(partial, scal, 2, D, H, A, grads, info)
    torch.cuda.synchronize()
    return grads.cpu(), partial.cpu()


def assert_row_written(partial, P_pf, P_vf):
    """No NaN anywhere in [0, p_stride) of either row; behind a network's block the row is zero."""
    assert not bool(torch.isnan(partial).any()), torch.isnan(partial).nonzero()[:8]
    assert bool(torch.isfinite(partial).all())
    assert bool((partial[0, P_pf:] == 0).all()) and bool((partial[1, P_vf:] == 0).all())


# ---------------------------------------------------------------- 1. the cross-wave order
EPS = 2.0 ** -24
ORDERS = {"issue": (1.0, EPS, EPS, -1.0), "control": (EPS, EPS, 1.0, -1.0)}


def left_to_right(c):
    s = np.float32(c[0])
    for v in c[1:]:
        s = np.float32(s + np.float32(v))
    return s


def test_the_inputs_tell_the_orders_apart():
    c = [np.float32(v) for v in ORDERS["issue"]]
    assert left_to_right(c) == np.float32(0.0)
    assert np.float32(np.float32(c[0] + c[1]) + np.float32(c[2] + c[3])) == np.float32(2.0 ** -24)
    assert left_to_right(c[::-1]) == np.float32(2.0 ** -23)
    assert left_to_right(ORDERS["control"]) == np.float32(2.0 ** -23)


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_cross_wave_order_is_pinned(order):
    D, A, N, rows = 17, 6, 16, 4
    R = rows + 3
    rs = np.random.RandomState(3)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    pf, _ = pc.random_nets(rs, D, A)                                          # (the policy pass runs beside it on finite inputs)
    logstd = f32(rs.uniform(-1.0, 0.0, (A,)))
    W2 = torch.zeros(H, H)
    W2[0, 0] = 1.0
    w3 = torch.zeros(1, H)
    w3[0, 0] = 1.0
    vf = [torch.zeros(H, D), torch.ones(H), W2, torch.ones(H), w3, torch.zeros(1)]
    # h1 = 1; z2 = [2, 1, 1, ..]; v = 2.  Sample 0 of minibatch row t (= tile t = wave t): R = 2 - 2 c_t, so that
    # d_v = 2 (v - R) / 64 = c_t / 16, exactly (c_t = 2^-24: R = 2 - 2^-23, the float below 2)
    c = ORDERS[order]
    row_idx = np.array([1, 2, 3, 4], dtype=np.int64)
    rets = torch.full((R, N, 1), 2.0)
    for t_, ct in enumerate(c):
        rets[row_idx[t_], 0, 0] = float(np.float32(2.0) - np.float32(2.0) * np.float32(ct))
        assert float(np.float32(2.0) - rets[row_idx[t_], 0, 0].numpy()) == 2.0 * ct    # representable, the difference exact
    x = dict(D=D, A=A, act="relu", N=N, rows=rows, tanh=True, obs=torch.ones(R, N, D), acts=f32(rs.uniform(-0.5, 0.5, (R, N, A))),
             advs=f32(rs.randn(R, N, 1)), rets=rets, old_values=torch.full((R, N, 1), 2.0), old_logp=f32(rs.randn(R, N, 1) - 5.0),
             row_idx=row_idx)
    flat = ref.flat_params(pf, logstd, vf)
    P_pf, P_vf = pc.p_sizes(D, A)
    raw = adv_raw_of(x["advs"][torch.from_numpy(row_idx)])
    grads, partial = launch(x, flat, P_pf, "gauss", gr.LOSS_PPO_CLIP, False, raw, 64.0, pc.CLIP, pc.C_ENT)
    assert_row_written(partial, P_pf, P_vf)
    want = float(left_to_right(c)) / 16.0                                    # (scaling by a power of two is exact)
    sl = ref.block_slices(D, A, False)
    row = partial[1].numpy()
    W1g, W2g = row[sl["W1"]].reshape(H, D), row[sl["W2"]].reshape(H, H)
    got = {"dW2 (MFMA tile), row 0": W2g[0], "dW1 (MFMA tile), row 0, k < 16": W1g[0, :16], "dW1[0][16] (17th column)": W1g[0, 16:17],
           "db1[0]": row[sl["b1"]][:1], "db2[0]": row[sl["b2"]][:1], "dW3[1:] (per lane, h2 = 1)": row[sl["W3"]][1:],
           "db3": row[sl["b3"]]}
    print(order, "want", want, {k: v[:2] for k, v in got.items()})
    for name, v in got.items():
        assert bool((v == np.float32(want)).all()), (order, name, v[:4], want)
    assert row[sl["W3"]][0] == np.float32(2.0 * want)                         # h2[0] = 2
    # everything else of the value row: no contribution at all
    assert bool((W2g[1:] == 0).all()) and bool((W1g[1:] == 0).all()) and bool((row[sl["b1"]][1:] == 0).all())
    assert bool((row[sl["b2"]][1:] == 0).all())
    # (a row of one workgroup: the fold hands it on unchanged)
    assert np.array_equal(grads[P_pf:].numpy(), row[:P_vf])


# ---------------------------------------------------------------- 2. every slot written once; idle waves fold as zeros
def _first_seed(make, ok, seed):
    for bump in range(pc.MAX_BUMP + 1):
        x = make(seed + bump)
        if ok(x):
            return x
    raise AssertionError("no seed in %d .. %d meets the input conditions" % (seed, seed + pc.MAX_BUMP))


def _with_layout(table, name, value, fn):
    table[name] = value
    try:
        return fn()
    finally:
        del table[name]


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("D,A", [(17, 6), (11, 3), (27, 8)], ids=["bench", "rt_11_3", "wide_27_8"])
def test_gaussian_rows_written_once_vs_float64(D, A, shape):
    N, rows = SHAPES[shape]
    loss_mode, clipv = LOSS
    c = (D, A, "tanh", "fixed_part", "plain")
    x = _with_layout(pc.LAYOUTS, "fixed_part", (N, rows, 2, 1),
                     lambda: _first_seed(lambda s: pc._grad_inputs(c, s), lambda x_: not pc.conditions(x_), 4100 + 10 * D + rows))
    mb = pc.minibatch(x)
    w = ref.minibatch_grads(x["pf"], x["logstd"], x["vf"], mb, x["adv_raw"], x["n_global"], loss_mode, clipv, x["tanh"], x["act"],
                            torch.float64, x["clip"], pc.C_ENT)
    floors = ref.grad_floor(mb, x["pf"], x["vf"], x["act"], x["n_global"])
    P_pf, P_vf = pc.p_sizes(D, A)
    grads, partial = launch(x, ref.flat_params(x["pf"], x["logstd"], x["vf"]), P_pf, "gauss", loss_mode, clipv, x["adv_raw"],
                            x["n_global"], x["clip"], pc.C_ENT)
    assert_row_written(partial, P_pf, P_vf)
    r = ref.grad_error_ratios(grads[:P_pf].double(), grads[P_pf:].double(), w, floors, pc.K_W, pc.K_LS, D, A)
    print("D%d A%d %s: element err / bound %.3f, d_logstd %.3f, worst block %.3f" % (D, A, shape, r["elem"], r["elem_ls"],
                                                                                  max(r["blocks"].values())))
    assert r["elem"] <= 1.0 and r["elem_ls"] <= 1.0, r
    assert all(v <= 1.0 for v in r["blocks"].values()), r["blocks"]


def _check_vs_autograd(grads, P_pf, want_pf, want_vf, label):
    got = grads.double()
    for name, gg, ww in (("pf", got[:P_pf], want_pf), ("vf", got[P_pf:], want_vf)):
        err, top = (gg - ww).abs().max().item(), ww.abs().max().item()
        print("%s %s: max abs err %.3e, max |grad| %.3e" % (label, name, err, top))
        assert err <= 1e-4 * top, (label, name, err, top)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_categorical_rows_written_once_vs_float64(shape):
    N, rows = SHAPES[shape]
    loss_mode, clipv = cref.LOSS_PPO_CLIP, True
    c = (17, 6, "tanh", "fixed_part")

    def ok(x_):
        mb_ = cu.minibatch(x_)
        return cu.near_clip(mb_["lp"], mb_["old_logp"]) == 0
    x = _with_layout(cu.PARTIAL_LAYOUT, "fixed_part", (N, rows, 2), lambda: _first_seed(lambda s: cu._grad_inputs(c, s), ok, 5100 + rows))
    mb = cu.minibatch(x)
    pf = [p.double().requires_grad_(True) for p in x["pf"]]
    vf = [p.double().requires_grad_(True) for p in x["vf"]]
    obs = mb["obs"].double()
    cref.objective(cu.forward(pf, obs, x["act"]), cu.forward(vf, obs, x["act"]), mb["acts"].reshape(-1), mb["advs"].double().reshape(-1),
                   mb["rets"].double(), mb["old_values"].double(), mb["old_logp"].double(), cu.CLIP, cu.C_ENT, clipv,
                   loss_mode).backward()
    flat = torch.cat([p.reshape(-1) for p in x["pf"] + x["vf"]])
    P_pf, P_vf = sum(p.numel() for p in x["pf"]), sum(p.numel() for p in x["vf"])
    grads, partial = launch(x, flat, P_pf, "cat", loss_mode, clipv, adv_raw_of(mb["advs"]), rows * N, cu.CLIP, cu.C_ENT)
    assert_row_written(partial, P_pf, P_vf)
    _check_vs_autograd(grads, P_pf, torch.cat([p.grad.reshape(-1) for p in pf]), torch.cat([p.grad.reshape(-1) for p in vf]),
                       "cat " + shape)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_state_std_rows_written_once_vs_float64(shape):
    N, rows = SHAPES[shape]
    loss_mode, clipv = sref.LOSS_PPO_CLIP, True
    c = (17, 6, "tanh", "fixed_part", False)

    def ok(x_):
        mb_ = su.minibatch(x_)
        return su.near_clip(mb_["lp"], mb_["old_logp"]) == 0 and su.near_clamp(mb_["raw_ls"]) == 0
    x = _with_layout(su.PARTIAL_LAYOUT, "fixed_part", (N, rows, 2), lambda: _first_seed(lambda s: su._grad_inputs(c, s), ok, 6100 + rows))
    mb = su.minibatch(x)
    pf = [p.double().requires_grad_(True) for p in x["pf"]]
    vf = [p.double().requires_grad_(True) for p in x["vf"]]
    obs = mb["obs"].double()
    pl, vl, _ = sref.objective(su.forward(pf, obs, x["act"]), su.forward(vf, obs, x["act"]), mb["acts"].double(),
                               mb["advs"].double().reshape(-1), mb["rets"].double(), mb["old_values"].double(),
                               mb["old_logp"].double(), su.CLIP, su.C_ENT, clipv, loss_mode, x["tanh"])
    (pl + vl).backward()
    flat = torch.cat([p.reshape(-1) for p in x["pf"] + x["vf"]])
    P_pf, P_vf = sum(p.numel() for p in x["pf"]), sum(p.numel() for p in x["vf"])
    grads, partial = launch(x, flat, P_pf, "sd", loss_mode, clipv, adv_raw_of(mb["advs"]), rows * N, su.CLIP, su.C_ENT)
    assert_row_written(partial, P_pf, P_vf)
    _check_vs_autograd(grads, P_pf, torch.cat([p.grad.reshape(-1) for p in pf]), torch.cat([p.grad.reshape(-1) for p in vf]),
                       "sd " + shape)
