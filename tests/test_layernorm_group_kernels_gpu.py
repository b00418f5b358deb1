"""The grouped LayerNorm kernels (trl_layernorm_fwd_group_f32, trl_layernorm_bwd_group_f32 and its first launch alone,
trl_act2_{fwd,bwd}_group_f32) against the float64 restatement in tests/_layernorm_ref.py, at the bounds
tests/test_layernorm_gpu.py uses for the single-problem kernels, and against those kernels themselves: a problem of a
group is worked on by as many workgroups, in the same row order, as it would be alone (up to the shared cap), so y, the
row statistics, dz and -- below the cap -- dgamma / dbeta carry the single-problem launch's bits.  On a tree without the
grouped entry points every test fails on the missing symbols."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _layernorm_ref as ref                                                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ACTS = {"tanh": 0, "relu": 1, "none": 2}
GS, MS, HS = [1, 2, 6, 12, 13], [1, 7, 64, 300], [1, 3, 24, 64, 100, 256, 1000]


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV).contiguous()


def offset_copy(t):
    """A contiguous copy of t whose data pointer is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4
    out.copy_(t)
    return out


def xhat_scale(a64, mean, rstd):
    """|xhat| plus the size its float32 absolute error scales with (tests/test_layernorm_gpu.py)."""
    return np.abs((a64 - mean) * rstd) + rstd * (np.abs(a64) + np.abs(mean))


def group_case(G, M, H, act, seed=0):
    """Per problem: a = act(N(0, 1)), dy ~ N(0, 1), gamma = 1 + 0.3 N, beta = 0.2 N -- every problem its own draws."""
    rs = np.random.RandomState(100000 * G + 1000 * M + H + seed)
    f = np.float32
    return [(ref.act_fn(rs.randn(M, H).astype(f), act).astype(f), rs.randn(M, H).astype(f),
             (1 + 0.3 * rs.randn(H)).astype(f), (0.2 * rs.randn(H)).astype(f)) for _ in range(G)]


def check_forward(y, stats, a, gamma, beta):
    want, mean, rstd = ref.ln_fwd(a.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64))
    err = np.abs(y.cpu().numpy() - want)
    assert (err <= 1e-5 + 1e-4 * np.abs(want)).all()
    st = stats.cpu().numpy().astype(np.float64).reshape(-1, 2)
    assert (np.abs(st[:, :1] - mean) <= 1e-6 + 1e-6 * np.abs(mean)).all()
    assert (np.abs(st[:, 1:] - rstd) <= 1e-5 * rstd).all()
    return float((err / (1e-5 + 1e-4 * np.abs(want))).max())


def check_backward(dz, dg, db, a, dy, gamma, act, sum_tol=1e-5):
    """The bounds of test_layernorm_gpu.test_backward_kernel_vs_float64 (sum_tol 2e-5: of its several-rows-per-wave case).
    dg / db None: only dz is checked.  Returns the worst err / bound."""
    a64, dy64, g64 = a.astype(np.float64), dy.astype(np.float64), gamma.astype(np.float64)
    mean, rstd = ref.ln_stats(a64)
    w_dz, w_dg, w_db = ref.ln_bwd(dy64, a64, mean, rstd, g64, act)
    xhat = (a64 - mean) * rstd
    Gm = np.abs(dy64 * g64).max(axis=1, keepdims=True)
    err = np.abs(dz.cpu().numpy() - w_dz)
    tol = 1e-4 * np.abs(w_dz) + 1e-5 * rstd * Gm * (1 + np.abs(xhat))
    assert (err <= tol).all(), "dz"
    worst = float((err / np.maximum(tol, 1e-30)).max())
    if dg is None:
        return worst
    for name, got, want, l1 in (("dgamma", dg, w_dg, (np.abs(dy64) * xhat_scale(a64, mean, rstd)).sum(axis=0)),
                                 ("dbeta", db, w_db, np.abs(dy64).sum(axis=0))):
        e = np.abs(got.cpu().numpy() - want)
        t = 1e-4 * np.abs(want) + sum_tol * l1
        assert (e <= t).all(), name
        worst = max(worst, float((e / np.maximum(t, 1e-30)).max()))
    return worst


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("G", GS)
def test_forward_group_vs_float64(G, M, H):
    """y rel 1e-4 / abs 1e-5, mean abs 1e-6 + rel 1e-6, rstd rel 1e-5 for every problem (G = 13: two launches); the bits of
    the single-problem launch; H = 1: y = beta exactly."""
    from torchrl_amd import _C
    case = group_case(G, M, H, "tanh" if H % 2 else "relu")
    a_d, g_d, b_d = ([dev(c[i]) for c in case] for i in (0, 2, 3))
    ys, sts = _C.layernorm_fwd_group(a_d, g_d, b_d)
    torch.cuda.synchronize()
    assert len(ys) == len(sts) == G
    worst = 0.0
    for g, (a, _, gamma, beta) in enumerate(case):
        worst = max(worst, check_forward(ys[g], sts[g], a, gamma, beta))
        y1, st1 = _C.layernorm_fwd(a_d[g], g_d[g], b_d[g])
        assert torch.equal(ys[g], y1) and torch.equal(sts[g], st1)
        if H == 1:
            assert np.array_equal(ys[g].cpu().numpy(), np.broadcast_to(beta, (M, 1)))
    print("G=%d M=%d H=%d forward worst err / bound %.3f" % (G, M, H, worst))


# ---------------------------------------------------------------- backward
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("G", GS)
def test_backward_group_vs_float64(G, M, H):
    """Both activations: dz, dgamma, dbeta of every problem at the single-problem kernels' bounds, with the kernel's own
    forward statistics; two calls give the same bits; and -- M <= 300 is at most 75 workgroups a problem, below the cap of
    1024 / 12 -- the bits of the single-problem launch.  H = 1: dz = 0 and dgamma = 0 exactly."""
    from torchrl_amd import _C
    lib = _C.lib()
    for act in ("tanh", "relu"):
        case = group_case(G, M, H, act, seed=5)
        a_d, dy_d, g_d, b_d = ([dev(c[i]) for c in case] for i in (0, 1, 2, 3))
        _, sts = _C.layernorm_fwd_group(a_d, g_d, b_d)
        runs = []
        for fill in (0.0, 7.0):
            dgs = [torch.full((H,), fill, device=DEV) for _ in range(G)]
            dbs = [torch.full((H,), fill, device=DEV) for _ in range(G)]
            runs.append((_C.layernorm_bwd_group(dy_d, a_d, sts, g_d, ACTS[act], dgs, dbs), dgs, dbs))
        torch.cuda.synchronize()
        for p, q in zip(*runs):
            assert all(torch.equal(x, y) for x, y in zip(p, q))
        dzs, dgs, dbs = runs[0]
        Gc = min(G, 12)
        per = -(-M // (16 if H <= 64 else 4))
        assert lib.trl_layernorm_bwd_group_slabs(Gc, M, H) == per                  # one slab per workgroup, as alone
        assert lib.trl_layernorm_bwd_group_workspace(Gc, M, H) == Gc * per * 2 * H
        worst = 0.0
        for g, (a, dy, gamma, _) in enumerate(case):
            worst = max(worst, check_backward(dzs[g], dgs[g], dbs[g], a, dy, gamma, act))
            dg1, db1 = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
            dz1 = _C.layernorm_bwd(dy_d[g], a_d[g], sts[g], g_d[g], ACTS[act], dg1, db1)
            assert torch.equal(dzs[g], dz1) and torch.equal(dgs[g], dg1) and torch.equal(dbs[g], db1)
            if H == 1:
                assert bool((dzs[g] == 0).all()) and float(dgs[g][0]) == 0.0
        print("G=%d M=%d H=%d %s backward worst err / bound %.3f" % (G, M, H, act, worst))


@pytest.mark.parametrize("M,H", [(7, 64), (300, 256), (64, 24)])
def test_one_unaligned_problem_puts_the_launch_on_the_4_byte_route(M, H):
    """Problem 1's a, y, dy and dz sit 4 bytes past a 16-byte boundary beside two aligned problems: the whole launch moves
    single floats (a lane owns other columns there, so the row sums are added in another order -- the same bounds, not
    the same bits), and every problem, the aligned ones included, meets them."""
    from torchrl_amd import _C
    case = group_case(3, M, H, "tanh", seed=9)
    a_d, dy_d, g_d, b_d = ([dev(c[i]) for c in case] for i in (0, 1, 2, 3))
    a_d[1], dy_d[1] = offset_copy(a_d[1]), offset_copy(dy_d[1])
    ys = [torch.empty(M, H, device=DEV), offset_copy(torch.empty(M, H, device=DEV)), torch.empty(M, H, device=DEV)]
    assert [t.data_ptr() % 16 for t in a_d] == [0, 4, 0] and [t.data_ptr() % 16 for t in ys] == [0, 4, 0]
    ys, sts = _C.layernorm_fwd_group(a_d, g_d, b_d, ys=ys)
    dzs = [torch.empty(M, H, device=DEV), offset_copy(torch.empty(M, H, device=DEV)), torch.empty(M, H, device=DEV)]
    dgs, dbs = [torch.zeros(H, device=DEV) for _ in range(3)], [torch.zeros(H, device=DEV) for _ in range(3)]
    _C.layernorm_bwd_group(dy_d, a_d, sts, g_d, ACTS["tanh"], dgs, dbs, dzs=dzs)
    torch.cuda.synchronize()
    for g, (a, dy, gamma, beta) in enumerate(case):
        check_forward(ys[g], sts[g], a, gamma, beta)
        check_backward(dzs[g], dgs[g], dbs[g], a, dy, gamma, "tanh")
    # the aligned launch of the aligned problems alone takes the 16-byte route: same values within the bounds, and the
    # 4-byte launch above did not write past problem 1's rows (its neighbours in the buffer are intact)
    y_al, st_al = _C.layernorm_fwd_group([a_d[0], a_d[2]], [g_d[0], g_d[2]], [b_d[0], b_d[2]])
    for y, st, g in zip(y_al, st_al, (0, 2)):
        check_forward(y, st, case[g][0], case[g][2], case[g][3])
        np.testing.assert_allclose(st.cpu().numpy(), sts[g].cpu().numpy(), rtol=1e-5, atol=1e-6)


def test_problems_without_parameter_gradients():
    """dgamma[g] None for problems 1 and 3 of five: their dz is the dz of the full call, bit for bit, and right; their
    neighbours' dz, dgamma and dbeta are unchanged, bit for bit; their slabs of the workspace are not written; a group in
    which nobody wants parameter gradients runs the first launch alone."""
    from torchrl_amd import _C
    G, M, H = 5, 64, 100
    case = group_case(G, M, H, "relu", seed=3)
    a_d, dy_d, g_d, b_d = ([dev(c[i]) for c in case] for i in (0, 1, 2, 3))
    _, sts = _C.layernorm_fwd_group(a_d, g_d, b_d)
    mk = lambda: [torch.zeros(H, device=DEV) for _ in range(G)]
    dg_all, db_all = mk(), mk()
    dz_all = _C.layernorm_bwd_group(dy_d, a_d, sts, g_d, ACTS["relu"], dg_all, db_all)
    dg, db = mk(), mk()
    for g in (1, 3):
        dg[g] = db[g] = None
    need = _C.lib().trl_layernorm_bwd_group_workspace(G, M, H)
    ws = torch.full((need,), 123.0, device=DEV)
    dz = _C.layernorm_bwd_group(dy_d, a_d, sts, g_d, ACTS["relu"], dg, db, workspace=ws)
    torch.cuda.synchronize()
    per = need // G
    for g in range(G):
        assert torch.equal(dz[g], dz_all[g])
        check_backward(dz[g], dg[g], db[g], case[g][0], case[g][1], case[g][2], "relu")
        if g in (1, 3):
            assert bool((ws[g * per:(g + 1) * per] == 123.0).all())
        else:
            assert torch.equal(dg[g], dg_all[g]) and torch.equal(db[g], db_all[g])
            assert not bool((ws[g * per:(g + 1) * per] == 123.0).any())
    dz_none = _C.layernorm_bwd_group(dy_d, a_d, sts, g_d, ACTS["relu"], [None] * G, [None] * G)
    assert all(torch.equal(p, q) for p, q in zip(dz_none, dz_all))
    with pytest.raises(_C.TrlError, match="both None"):
        _C.layernorm_bwd_group(dy_d, a_d, sts, g_d, ACTS["relu"], [None] + dg_all[1:], db_all)


def test_one_gamma_under_two_problems():
    """One network on two inputs: problems 0 and 1 share gamma / beta (read-only) and have their own dgamma / dbeta."""
    from torchrl_amd import _C
    M, H = 64, 48
    case = group_case(2, M, H, "tanh", seed=7)
    case[1] = (case[1][0], case[1][1], case[0][2], case[0][3])
    a_d, dy_d = ([dev(c[i]) for c in case] for i in (0, 1))
    gamma, beta = dev(case[0][2]), dev(case[0][3])
    ys, sts = _C.layernorm_fwd_group(a_d, [gamma, gamma], [beta, beta])
    dgs, dbs = [torch.zeros(H, device=DEV) for _ in range(2)], [torch.zeros(H, device=DEV) for _ in range(2)]
    dzs = _C.layernorm_bwd_group(dy_d, a_d, sts, [gamma, gamma], ACTS["tanh"], dgs, dbs)
    torch.cuda.synchronize()
    for g, (a, dy, gm, bt) in enumerate(case):
        check_forward(ys[g], sts[g], a, gm, bt)
        check_backward(dzs[g], dgs[g], dbs[g], a, dy, gm, "tanh")
    assert not torch.equal(dgs[0], dgs[1])


def test_several_row_blocks_per_wave_and_the_slab_cap():
    """G = 2, M = 33000, H = 24: a problem alone would take 2063 workgroups of sixteen rows; the two share the backward's
    1024 (512 slabs each, some waves walk two row blocks) and the forward's 2048.  y and dz as everywhere; the column sums see
    2 + 16 + 32 + 16 additions in sequence, fewer than the single-problem case this bound was set for
    (tests/test_layernorm_gpu.py: abs 2e-5 x sum_rows |term|).  Two calls give the same bits."""
    from torchrl_amd import _C
    G, M, H = 2, 33000, 24
    case = group_case(G, M, H, "tanh", seed=11)
    a_d, dy_d, g_d, b_d = ([dev(c[i]) for c in case] for i in (0, 1, 2, 3))
    ys, sts = _C.layernorm_fwd_group(a_d, g_d, b_d)
    assert _C.lib().trl_layernorm_bwd_group_slabs(G, M, H) == 512
    assert _C.lib().trl_layernorm_bwd_group_workspace(G, M, H) == 1024 * 2 * H
    runs = []
    for _ in range(2):
        dgs, dbs = [torch.zeros(H, device=DEV) for _ in range(G)], [torch.zeros(H, device=DEV) for _ in range(G)]
        runs.append((_C.layernorm_bwd_group(dy_d, a_d, sts, g_d, ACTS["tanh"], dgs, dbs), dgs, dbs))
    torch.cuda.synchronize()
    for p, q in zip(*runs):
        assert all(torch.equal(x, y) for x, y in zip(p, q))
    for g, (a, dy, gamma, beta) in enumerate(case):
        check_forward(ys[g], sts[g], a, gamma, beta)
        w = check_backward(runs[0][0][g], runs[0][1][g], runs[0][2][g], a, dy, gamma, "tanh", sum_tol=2e-5)
        print("G=2 M=33000 H=24 problem %d worst err / bound %.3f" % (g, w))


def test_slabs_folded_by_a_fold_plan():
    """plan=: the first launch leaves the slabs in the plan's workspace and [dgamma | dbeta] (back to back, as in a flat
    gradient buffer) is one entry of the plan's fold -- nothing is written before `plan.run()`, the sums meet the bounds
    after it (another fixed order: not the bits of the two-launch form), and twice the same bits.  A problem whose dbeta does
    not follow its dgamma takes the fold launch of the grouped entry point instead."""
    from torchrl_amd import _C
    G, M, H = 3, 300, 100
    case = group_case(G, M, H, "tanh", seed=13)
    a_d, dy_d, g_d, b_d = ([dev(c[i]) for c in case] for i in (0, 1, 2, 3))
    _, sts = _C.layernorm_fwd_group(a_d, g_d, b_d)
    ws = torch.empty(_C.lib().trl_layernorm_bwd_group_workspace(G, M, H), device=DEV)
    outs = []
    for _ in range(2):
        flat = torch.full((G * 2 * H,), 5.0, device=DEV)
        dgs = [flat[2 * H * g:2 * H * g + H] for g in range(G)]
        dbs = [flat[2 * H * g + H:2 * H * (g + 1)] for g in range(G)]
        dgs[1] = dbs[1] = None
        plan = _C.FoldPlan(ws)
        dzs = _C.layernorm_bwd_group(dy_d, a_d, sts, g_d, ACTS["tanh"], dgs, dbs, plan=plan)
        assert len(plan.entries) == 2
        torch.cuda.synchronize()
        assert bool((flat == 5.0).all())
        plan.run()
        torch.cuda.synchronize()
        assert bool((flat[2 * H:4 * H] == 5.0).all())
        outs.append((dzs, flat))
        for g in (0, 2):
            check_backward(dzs[g], dgs[g], dbs[g], case[g][0], case[g][1], case[g][2], "tanh")
        check_backward(dzs[1], None, None, case[1][0], case[1][1], case[1][2], "tanh")
    assert torch.equal(outs[0][1], outs[1][1]) and all(torch.equal(p, q) for p, q in zip(outs[0][0], outs[1][0]))
    dgs, dbs = [torch.zeros(H, device=DEV) for _ in range(G)], [torch.zeros(H, device=DEV) for _ in range(G)]
    plan = _C.FoldPlan(ws)
    dzs = _C.layernorm_bwd_group(dy_d, a_d, sts, g_d, ACTS["tanh"], dgs, dbs, plan=plan)
    assert plan.entries == []
    for g in range(G):
        check_backward(dzs[g], dgs[g], dbs[g], case[g][0], case[g][1], case[g][2], "tanh")


# ---------------------------------------------------------------- the second activation
@pytest.mark.parametrize("n,offset", [(1, False), (5, False), (7000, False), (7000, True), (4096, False), (600000, False)])
@pytest.mark.parametrize("G", GS)
def test_second_tanh_group(G, n, offset):
    """t2 = tanh(t1) abs 3e-7 and dz rel 1e-6 + abs 1e-7 against float64 on the stored values, as for the single-problem
    kernels, and their bits (elementwise work: the route does not change a value); one problem 4 bytes past a 16-byte
    boundary puts the whole launch on the 4-byte route.  n = 600000 is past the 2048 / 12 workgroups a problem of twelve
    gets: threads walk several pieces.  A second ReLU is the identity."""
    from torchrl_amd import _C
    rs = np.random.RandomState(n + G)
    t1 = [np.tanh(rs.randn(n)).astype(np.float32) for _ in range(G)]
    d = [rs.randn(n).astype(np.float32) for _ in range(G)]
    t1_d, d_d = [dev(t) for t in t1], [dev(t) for t in d]
    outs = [torch.empty(n, device=DEV) for _ in range(G)]
    dz_outs = [torch.empty(n, device=DEV) for _ in range(G)]
    if offset:
        outs[G // 2], dz_outs[0] = offset_copy(outs[G // 2]), offset_copy(dz_outs[0])
    t2 = _C.act2_fwd_group(t1_d, ACTS["tanh"], outs=outs)
    dz = _C.act2_bwd_group(d_d, t1_d, t2, ACTS["tanh"], outs=dz_outs)
    torch.cuda.synchronize()
    for g in range(G):
        assert (np.abs(t2[g].cpu().numpy() - np.tanh(t1[g].astype(np.float64))) <= 3e-7).all()
        want = ref.act2_bwd(d[g].astype(np.float64), t1[g].astype(np.float64), t2[g].cpu().numpy().astype(np.float64), "tanh")
        assert (np.abs(dz[g].cpu().numpy() - want) <= 1e-7 + 1e-6 * np.abs(want)).all()
        assert torch.equal(t2[g], _C.act2_fwd(t1_d[g], ACTS["tanh"]))
        assert torch.equal(dz[g], _C.act2_bwd(d_d[g], t1_d[g], t2[g], ACTS["tanh"]))
    r1 = [dev(np.maximum(rs.randn(n), 0).astype(np.float32)) for _ in range(G)]
    for got, want in zip(_C.act2_fwd_group(r1, ACTS["relu"]), r1):
        assert torch.equal(got, want)
    for got, dd, r in zip(_C.act2_bwd_group(d_d, r1, r1, ACTS["relu"]), d_d, r1):
        assert torch.equal(got, dd * (r > 0))


# ---------------------------------------------------------------- what the entry points refuse
def test_group_entry_points_refuse_bad_sizes():
    from torchrl_amd import _C
    lib = _C.lib()
    assert lib.trl_layernorm_bwd_group_workspace(13, 4, 8) < 0 and lib.trl_layernorm_bwd_group_workspace(0, 4, 8) < 0
    assert lib.trl_layernorm_bwd_group_workspace(2, 4, 1025) < 0 and lib.trl_layernorm_bwd_group_slabs(2, 0, 8) < 0
    assert lib.trl_layernorm_bwd_group_workspace(12, 1, 24) == 12 * 2 * 24          # G = 12, M = 1: twelve workgroups
    a = torch.zeros(4, 8, device=DEV)
    v = torch.zeros(8, device=DEV)
    import ctypes as C
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    st = torch.zeros(4, 2, device=DEV)
    assert lib.trl_layernorm_fwd_group_f32(13, arr([a] * 13), arr([v] * 13), arr([v] * 13), arr([a] * 13), arr([st] * 13),
                                           4, 8, None) != 0
    assert "12 problems" in lib.trl_last_error().decode()
    with pytest.raises(_C.TrlError, match="1024"):
        _C.layernorm_fwd_group([torch.zeros(4, 1025, device=DEV)], [torch.zeros(1025, device=DEV)], [torch.zeros(1025, device=DEV)])
    with pytest.raises(_C.TrlError, match="one shape"):
        _C.layernorm_fwd_group([a, torch.zeros(5, 8, device=DEV)], [v, v], [v, v])
    with pytest.raises(_C.TrlError, match="one shape"):
        _C.act2_fwd_group([a, torch.zeros(5, 8, device=DEV)], ACTS["tanh"])
