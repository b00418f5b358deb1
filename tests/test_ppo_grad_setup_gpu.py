"""The set-up of ppo_grad_wave_kernel in front of its tile loop (torchrl_amd/csrc/k_ppo.hip): every parameter but W2 is loaded
once per workgroup with coalesced dword loads into an LDS image -- [W1 | b1 | b2 | W3 | b3 | logstd] at the actual dims -- and
each lane reads its register operands (w1 / w1b, w3h, w3t, b3, logstd) back from the image behind the set-up's barrier.

1. Dims at which a mask or an offset of those reads can go wrong, one launch (one workgroup per network) on N = 16 x 2 rows --
   two tiles, waves 2 and 3 idle -- against float64 within the bound of the head's own kernel test
   (test_ppo_update_kernels_gpu.py: K u M_e + floor_e per element and 1e-4 of a block's largest entry; the categorical / SD
   files: 1e-4 of the network's largest entry).  The parameters outside W2 are pairwise distinct floats of size O(1 / sqrt(fan
   in)): a misrouted operand is an O(1) error.  The float32 restatement alone holds every bound on the CPU (first test).
2. Nothing outside a network's block is used, at any alignment: the blocks live in [64 guard floats | pf | vf | 64 guard
   floats] shifted by 0 .. 3 floats, guards NaN and 1e30: gradients and partial rows are the same bits in all eight runs.
3. A second workgroup of a network sees the same operands.  (a) n_wg = 4, n_wg_pf = 2 on N = 16 x 4 rows: each network's two
   rows, summed in float64, against the single row of the n_wg = 2 launch within _ppo_update_ref.fold_bound.  With four tiles
   the second workgroup of a network has no tile, so (b) N = 16 x 8 rows: workgroup k of a network takes tiles 4k .. 4k + 3 =
   minibatch rows 4k .. 4k + 3, and a one-workgroup launch on those four rows alone (same advantage statistics, same
   n_global) runs the same arithmetic: the rows are equal bit for bit."""
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

gpu = pytest.mark.gpu
H = 64
NAN = float("nan")
LAY = "setup"
LOSS = (gr.LOSS_PPO_CLIP, True)

# (head, D, A, act): runtime dims, the compile-time 17 / 6, the wide tile; categorical; state-dependent std; ReLU once per head
GAUSS = ([("gauss", D, A, "tanh") for D in (2, 15, 16, 17) for A in (1, 5, 8)] + [("gauss", 17, 6, "tanh")]
         + [("gauss", D, A, "tanh") for D in (18, 31, 32) for A in (1, 8)] + [("gauss", 15, 5, "relu")])
CAT = [("cat", 11, 2, "tanh"), ("cat", 17, 8, "tanh"), ("cat", 11, 2, "relu")]
SD = [("sd", 11, 1, "tanh"), ("sd", 17, 8, "tanh"), ("sd", 17, 8, "relu")]
CASES = GAUSS + CAT + SD
GUARD_CASES = [("gauss", 15, 5, "tanh"), ("cat", 11, 2, "tanh"), ("sd", 17, 8, "tanh")]
WG_CASES = [("gauss", 17, 6, "tanh"), ("gauss", 15, 5, "tanh"), ("sd", 17, 8, "tanh")]


def cid(c):
    return "%s_D%d_A%d_%s" % c


def adv_raw_of(advs):
    a = advs.double().reshape(-1)
    return torch.tensor([a.sum(), (a * a).sum(), a.max(), -a.min()], dtype=torch.float64)


def _distinct_outside_w2(*nets):
    """Every parameter but the two W2 (index 2 of a net's list) is a float of its own."""
    v = torch.cat([p.reshape(-1) for net in nets for k, p in enumerate(net) if k != 2]).numpy()
    return np.unique(v).size == v.size


_INPUTS = {}


def inputs(c, rows=2):
    """The input set of case `c` on N = 16 x `rows` rows (first seed that meets the head's input conditions), once."""
    if (c, rows) in _INPUTS:
        return _INPUTS[(c, rows)]
    head, D, A, act = c
    base = 8200 + 131 * CASES.index(c) + rows
    if head == "gauss":
        table, value, make = pc.LAYOUTS, (16, rows, 2, 1), lambda s: pc._grad_inputs((D, A, act, LAY, "plain"), s)
        ok = lambda x: not pc.conditions(x) and _distinct_outside_w2(x["pf"] + [x["logstd"]], x["vf"])
    elif head == "cat":
        table, value, make = cu.PARTIAL_LAYOUT, (16, rows, 2), lambda s: cu._grad_inputs((D, A, act, LAY), s)

        def ok(x):
            mb = cu.minibatch(x)
            return cu.near_clip(mb["lp"], mb["old_logp"]) == 0 and _distinct_outside_w2(x["pf"], x["vf"])
    else:
        table, value, make = su.PARTIAL_LAYOUT, (16, rows, 2), lambda s: su._grad_inputs((D, A, act, LAY, False), s)

        def ok(x):
            mb = su.minibatch(x)
            return (su.near_clip(mb["lp"], mb["old_logp"]) == 0 and su.near_clamp(mb["raw_ls"]) == 0
                    and _distinct_outside_w2(x["pf"], x["vf"]))
    table[LAY] = value
    try:
        for bump in range(pc.MAX_BUMP + 1):
            x = make(base + bump)
            if ok(x):
                break
        else:
            raise AssertionError("%s: no seed in %d .. %d meets the input conditions" % (cid(c), base, base + pc.MAX_BUMP))
    finally:
        del table[LAY]
    x["head"] = head
    if head == "gauss":
        x["flat"] = torch.as_tensor(ref.flat_params(x["pf"], x["logstd"], x["vf"]))
        x["P_pf"], x["P_vf"] = pc.p_sizes(D, A)
        x["c_ent"] = pc.C_ENT
    else:
        m = cu if head == "cat" else su
        x["flat"] = torch.cat([p.reshape(-1) for p in x["pf"] + x["vf"]])
        x["P_pf"], x["P_vf"] = sum(p.numel() for p in x["pf"]), sum(p.numel() for p in x["vf"])
        mb = m.minibatch(x)
        x["adv_raw"], x["n_global"], x["clip"], x["c_ent"] = adv_raw_of(mb["advs"]), float(rows * 16), m.CLIP, m.C_ENT
        x.setdefault("tanh", True)
    _INPUTS[(c, rows)] = x
    return x


def reference(x, dtype):
    """(policy gradient, value gradient) of the restatement / of autograd on the head's objective, in `dtype`."""
    loss_mode, clipv = LOSS
    if x["head"] == "gauss":
        w = ref.minibatch_grads(x["pf"], x["logstd"], x["vf"], pc.minibatch(x), x["adv_raw"], x["n_global"], loss_mode, clipv,
                                x["tanh"], x["act"], dtype, x["clip"], pc.C_ENT)
        return w
    m = cu if x["head"] == "cat" else su
    mb = m.minibatch(x)
    pf = [p.detach().to(dtype).clone().requires_grad_(True) for p in x["pf"]]
    vf = [p.detach().to(dtype).clone().requires_grad_(True) for p in x["vf"]]
    obs = mb["obs"].to(dtype)
    t = lambda k: mb[k].to(dtype)
    if x["head"] == "cat":
        cref.objective(cu.forward(pf, obs, x["act"]), cu.forward(vf, obs, x["act"]), mb["acts"].reshape(-1), t("advs").reshape(-1),
                       t("rets"), t("old_values"), t("old_logp"), cu.CLIP, cu.C_ENT, clipv, loss_mode).backward()
    else:
        pl, vl, _ = sref.objective(su.forward(pf, obs, x["act"]), su.forward(vf, obs, x["act"]), t("acts"), t("advs").reshape(-1),
                                   t("rets"), t("old_values"), t("old_logp"), su.CLIP, su.C_ENT, clipv, loss_mode, x["tanh"])
        (pl + vl).backward()
    return {"pf": torch.cat([p.grad.reshape(-1) for p in pf]), "vf": torch.cat([p.grad.reshape(-1) for p in vf])}


_WANT = {}


def want64(c):
    if c not in _WANT:
        _WANT[c] = reference(inputs(c), torch.float64)
    return _WANT[c]


def check(c, x, got_pf, got_vf, label, scale=1.0):
    """The bound of the head's kernel test, taken at `scale` of it."""
    w = want64(c)
    if x["head"] == "gauss":
        floors = ref.grad_floor(pc.minibatch(x), x["pf"], x["vf"], x["act"], x["n_global"])
        r = ref.grad_error_ratios(got_pf.double(), got_vf.double(), w, floors, pc.K_W, pc.K_LS, x["D"], x["A"])
        print("%s %s: element err / bound %.3f, d_logstd %.3f, worst block %.3f" % (cid(c), label, r["elem"], r["elem_ls"],
                                                                                     max(r["blocks"].values())))
        assert r["elem"] <= scale and r["elem_ls"] <= scale, r
        assert all(v <= scale for v in r["blocks"].values()), r["blocks"]
        return
    for name, gg, ww in (("pf", got_pf.double(), w["pf"].double()), ("vf", got_vf.double(), w["vf"].double())):
        err, top = (gg - ww).abs().max().item(), ww.abs().max().item()
        print("%s %s %s: max abs err %.3e, max |grad| %.3e" % (cid(c), label, name, err, top))
        assert err <= scale * 1e-4 * top, (cid(c), name, err, top)


# ---------------------------------------------------------------- the cases on the CPU
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_float32_restatement_holds_the_bound_of_every_case(c):
    """The float32 run of the reference alone stays inside a quarter of the bound the kernel is held to."""
    x = inputs(c)
    g = reference(x, torch.float32)
    check(c, x, g["pf"], g["vf"], "float32 on the CPU", scale=0.25)


# ---------------------------------------------------------------- launches
def dev(x, dtype=None):
    t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
    return (t if dtype is None else t.to(dtype)).to(torch.device("cuda:0")).contiguous()


def launch(x, n_wg=2, n_wg_pf=1, shift=0, guard=None, row_idx=None):
    """One gradient launch and its fold on NaN-filled buffers -> (grads, partial rows) on the host.  `guard`: the parameter
    blocks sit in [64 + shift guard floats | pf | vf | 64 guard floats]."""
    from torchrl_amd import _C
    DEV = torch.device("cuda:0")
    head = x["head"]
    grad_fn, reduce_fn, stride_fn = {"gauss": (_C.ppo_minibatch_grad, _C.ppo_reduce, _C.ppo_partial_stride),
                                     "cat": (_C.ppo_cat_minibatch_grad, _C.ppo_cat_reduce, _C.ppo_cat_partial_stride),
                                     "sd": (_C.ppo_sd_minibatch_grad, _C.ppo_sd_reduce, _C.ppo_sd_partial_stride)}[head]
    loss_mode, clipv = LOSS
    D, A, P_pf = x["D"], x["A"], x["P_pf"]
    ps = stride_fn(D, H, A)
    sw = _C.ppo_sd_scalar_stride() if head == "sd" else 8
    t = {k: dev(x[k]) for k in ("obs", "acts", "advs", "rets", "old_values", "old_logp")}
    row_idx = x["row_idx"] if row_idx is None else row_idx
    row_idx_d, raw_d = dev(row_idx), dev(x["adv_raw"], torch.float64)
    if guard is None:
        buf, lead = dev(x["flat"]), 0
    else:
        lead = 64 + shift
        buf = dev(torch.cat([torch.full((lead,), guard), x["flat"], torch.full((64,), guard)]))
    flat_d = buf[lead: lead + x["flat"].numel()]
    partial = torch.full((n_wg, ps), NAN, device=DEV)
    scal = torch.full((n_wg * sw,), NAN, dtype=torch.float64, device=DEV)
    grads = torch.full((x["flat"].numel(),), NAN, device=DEV)
    info = torch.zeros(24, dtype=torch.float64, device=DEV)
    g = _C.PpoBatchArgs()
    for k, v in t.items():
        setattr(g, k, v.data_ptr())
    g.row_idx, g.rows_mb, g.N = row_idx_d.data_ptr(), len(row_idx), x["N"]
    g.adv_raw, g.n_global = raw_d.data_ptr(), float(x["n_global"])
    g.pf_params, g.vf_params = flat_d.data_ptr(), flat_d.data_ptr() + 4 * P_pf
    g.D, g.H, g.A, g.act = D, H, A, (_C.ACT_TANH if x["act"] == "tanh" else _C.ACT_RELU)
    g.clip_para, g.entropy_coeff, g.clipped_value_loss, g.tanh_action = x["clip"], x["c_ent"], int(clipv), int(x["tanh"])
    g.loss_mode = loss_mode
    g.partial, g.scal_partial, g.n_wg, g.n_wg_pf = partial.data_ptr(), scal.data_ptr(), n_wg, n_wg_pf
    grad_fn(g, DEV)
    if head == "gauss":
        reduce_fn(partial, scal, n_wg, D, H, A, grads, info, pf_params=flat_d, n_wg_pf=n_wg_pf)
    else:
        reduce_fn(partial, scal, n_wg, D, H, A, grads, info)
    torch.cuda.synchronize()
    return grads.cpu(), partial.cpu()


def assert_rows_written(partial, n_pf, P_pf, P_vf):
    assert not bool(torch.isnan(partial).any()), torch.isnan(partial).nonzero()[:8]
    assert bool(torch.isfinite(partial).all())
    assert bool((partial[:n_pf, P_pf:] == 0).all()) and bool((partial[n_pf:, P_vf:] == 0).all())


# ---------------------------------------------------------------- 1. masks and offsets
@gpu
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_operands_from_the_image_vs_float64(c):
    x = inputs(c)
    grads, partial = launch(x)
    assert_rows_written(partial, 1, x["P_pf"], x["P_vf"])
    check(c, x, grads[:x["P_pf"]], grads[x["P_pf"]:], "kernel")


# ---------------------------------------------------------------- 2. nothing outside the block, at any alignment
@gpu
@pytest.mark.parametrize("c", GUARD_CASES, ids=cid)
def test_nothing_outside_the_block_is_used(c):
    x = inputs(c)
    base = launch(x, shift=0, guard=NAN)
    assert_rows_written(base[1], 1, x["P_pf"], x["P_vf"])
    check(c, x, base[0][:x["P_pf"]], base[0][x["P_pf"]:], "guarded, shift 0")
    for shift in range(4):
        for guard in (NAN, 1e30):
            grads, partial = launch(x, shift=shift, guard=guard)
            assert np.array_equal(grads.numpy(), base[0].numpy()), (cid(c), shift, guard, "gradients")
            assert np.array_equal(partial.numpy(), base[1].numpy()), (cid(c), shift, guard, "partial rows")


# ---------------------------------------------------------------- 3. a network's second workgroup
@gpu
@pytest.mark.parametrize("c", WG_CASES, ids=cid)
def test_two_workgroups_of_a_network_sum_to_the_single_row(c):
    x = inputs(c, rows=4)
    P = (x["P_pf"], x["P_vf"])
    _, one = launch(x, n_wg=2, n_wg_pf=1)
    _, two = launch(x, n_wg=4, n_wg_pf=2)
    assert_rows_written(two, 2, *P)
    for net in (0, 1):
        pair = two[2 * net: 2 * net + 2, :P[net]]
        s, S = ref.fold(pair)
        err = (s - one[net, :P[net]].double()).abs()
        bound = ref.fold_bound(2, S)
        print("%s net %d: worst err / bound %.3f" % (cid(c), net, float((err / bound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all()), (cid(c), net, float(err.max()))


@gpu
@pytest.mark.parametrize("c", WG_CASES, ids=cid)
def test_each_workgroup_equals_a_launch_on_its_own_rows(c):
    x = inputs(c, rows=8)
    P = (x["P_pf"], x["P_vf"])
    _, two = launch(x, n_wg=4, n_wg_pf=2)
    assert_rows_written(two, 2, *P)
    for k in (0, 1):
        _, own = launch(x, n_wg=2, n_wg_pf=1, row_idx=x["row_idx"][4 * k: 4 * k + 4])
        for net in (0, 1):
            a, b = two[2 * net + k, :P[net]].numpy(), own[net, :P[net]].numpy()
            assert np.abs(b).max() > 0
            assert np.array_equal(a, b), (cid(c), "workgroup", k, "net", net, float(np.abs(a - b).max()))
