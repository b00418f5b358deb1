"""The shared-std Gaussian PPO / A2C update kernels of torchrl_amd/csrc/k_ppo.hip called directly through _C, each against
the float64 restatement of tests/_ppo_update_ref.py on the inputs of tests/_ppo_update_cases.py:

  * ppo_grad_wave_kernel<..., HEAD_GAUSS> (trl_ppo_minibatch_grad_f32) + the fold: every gradient element within
    K u M_e + floor_e of float64 autograd (M: the element's running magnitude), every block within 1e-4 of its own largest
    entry, the 24-slot info row, NaN-filled workspaces, the clamp's exact zeros, the value loss's tie convention, shards,
    workgroup splits;
  * the fold alone on synthetic rows at the row counts where fold_rows_wave / fold_scalar_stats take another round;
  * clip_adam_kernel, its device-resident step state in both tick modes, device learning rates, max_norm <= 0, 1 to 4
    groups, an empty and an all-zero group; trl_clip_adam_polyak_f32's Polyak step and ring filing;
  * trl_ppo_reduce_adam_f32 with its workspace header over three chained updates.

The constants K come from the restatement's float32 run on the CPU (tests/test_ppo_update_kernels_cpu.py holds that run to
the same bounds at a quarter); profiles/NOTES_ppo_update_kernel_tests.md has err / bound per case."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_ref as gr                                                       # noqa: E402
import _ppo_update_cases as pc                                                # noqa: E402
import _ppo_update_ref as ref                                                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H = 64
NAN = float("nan")


def dev(x, dtype=None):
    t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


# ---------------------------------------------------------------- the gradient launch
class Launch:
    """Device copies of an input set and the descriptor of trl_ppo_minibatch_grad_f32 on them."""

    def __init__(self, x):
        from torchrl_amd import _C
        self.x = x
        # stored rows outside the minibatch are NaN in every buffer: nothing of them may reach a result (cell 0, which
        # lanes and tiles past the end of the minibatch read, is among them)
        out = torch.ones(x["rows"] + 3, dtype=torch.bool)
        out[torch.from_numpy(x["row_idx"])] = False
        assert bool(out[0])
        self.t = {}
        for k in ("obs", "acts", "advs", "rets", "old_values", "old_logp"):
            t = x[k].clone()
            t[out] = NAN
            self.t[k] = dev(t)
        self.row_idx = dev(x["row_idx"])
        self.raw = dev(x["adv_raw"], torch.float64)
        self.P_pf, self.P_vf = pc.p_sizes(x["D"], x["A"])
        self.flat0 = dev(ref.flat_params(x["pf"], x["logstd"], x["vf"]))
        assert self.flat0.numel() == self.P_pf + self.P_vf
        self.ps = _C.ppo_partial_stride(x["D"], H, x["A"])
        self.act = _C.ACT_TANH if x["act"] == "tanh" else _C.ACT_RELU

    def args(self, flat, loss_mode, clipv, n_wg, n_wg_pf, partial, scal):
        from torchrl_amd import _C
        x, g = self.x, _C.PpoBatchArgs()
        for k, v in self.t.items():
            setattr(g, k, v.data_ptr())
        if loss_mode == gr.LOSS_A2C:
            g.old_logp = None                                                # A2C never reads log pi_old
        if not clipv:
            g.old_values = None
        g.row_idx, g.rows_mb, g.N = self.row_idx.data_ptr(), x["rows"], x["N"]
        g.adv_raw, g.n_global = self.raw.data_ptr(), x["n_global"]
        g.pf_params, g.vf_params = flat.data_ptr(), flat.data_ptr() + 4 * self.P_pf
        g.D, g.H, g.A, g.act = x["D"], H, x["A"], self.act
        g.clip_para, g.entropy_coeff, g.clipped_value_loss, g.tanh_action = x["clip"], pc.C_ENT, int(clipv), int(x["tanh"])
        g.loss_mode = loss_mode
        g.partial, g.scal_partial, g.n_wg, g.n_wg_pf = partial.data_ptr(), scal.data_ptr(), n_wg, n_wg_pf
        return g

    def rows(self, n):
        # (NaN: every slot the fold reads has to be written by the launch)
        return (torch.full((n, self.ps), NAN, device=DEV), torch.full((n, 8), NAN, dtype=torch.float64, device=DEV))

    def grad_and_fold(self, loss_mode, clipv, n_wg, n_wg_pf, flat=None):
        """One gradient launch and its fold on NaN / sentinel-filled buffers -> (grads, info, partial, scal) on the host."""
        from torchrl_amd import _C
        flat = self.flat0 if flat is None else flat
        partial, scal = self.rows(n_wg)
        grads = torch.full((self.P_pf + self.P_vf,), NAN, device=DEV)
        info = torch.full((24,), ref.SENTINEL, dtype=torch.float64, device=DEV)
        _C.ppo_minibatch_grad(self.args(flat, loss_mode, clipv, n_wg, n_wg_pf, partial, scal), DEV)
        _C.ppo_reduce(partial, scal, n_wg, self.x["D"], H, self.x["A"], grads, info, pf_params=flat, n_wg_pf=n_wg_pf)
        return grads.cpu(), info.cpu().numpy(), partial.cpu(), scal.cpu()


_WANT = {}


def want_of(c, loss_mode, clipv):
    """The float64 restatement of a case (and its floors), computed once and shared."""
    key = (pc.case_id(c), loss_mode, clipv)
    if key not in _WANT:
        x = pc.grad_inputs(c)
        mb = pc.minibatch(x)
        w = ref.minibatch_grads(x["pf"], x["logstd"], x["vf"], mb, x["adv_raw"], x["n_global"], loss_mode, clipv, x["tanh"],
                                x["act"], torch.float64, x["clip"], pc.C_ENT)
        _WANT[key] = (x, w, ref.grad_floor(mb, x["pf"], x["vf"], x["act"], x["n_global"]))
    return _WANT[key]


def check_gradient(got, L, x, w, floors, label, errlog):
    """The element bound and the per-block contract -> the ratios."""
    D, A = x["D"], x["A"]
    assert bool(torch.isfinite(got).all()), label
    r = ref.grad_error_ratios(got[:L.P_pf], got[L.P_pf:], w, floors, pc.K_W, pc.K_LS, D, A)
    worst = max(r["blocks"], key=r["blocks"].get)
    print("%s: element err / bound %.3f, d_logstd %.3f; worst block %s at %.3f of 1e-4 max|block|"
          % (label, r["elem"], r["elem_ls"], worst, r["blocks"][worst]))
    errlog(label + "_elem_over_bound", r["elem"], 1.0)
    errlog(label + "_dlogstd_over_bound", r["elem_ls"], 1.0)
    errlog(label + "_worst_block_over_1e-4_max", r["blocks"][worst], 1.0)
    assert r["elem"] <= 1.0 and r["elem_ls"] <= 1.0, (label, r["elem"], r["elem_ls"])
    assert all(v <= 1.0 for v in r["blocks"].values()), (label, r["blocks"])
    return r


@pytest.mark.parametrize("c", pc.GRAD_CASES, ids=pc.case_id)
def test_gradient_and_info_vs_float64_restatement(c, errlog):
    for loss_mode, clipv in pc.LOSSES:
        x, w, floors = want_of(c, loss_mode, clipv)
        L = Launch(x)
        D, A, B = x["D"], x["A"], x["rows"] * x["N"]
        n_wg, n_wg_pf = x["n_wg"], x["n_wg_pf"]
        n_pf = n_wg_pf if n_wg_pf else n_wg // 2
        label = "mode%d_clipv%d" % (loss_mode, int(clipv))
        got, info, partial, scal = L.grad_and_fold(loss_mode, clipv, n_wg, n_wg_pf)
        # everything the fold reads was written, and is finite
        assert bool(torch.isfinite(partial[:n_pf, :L.P_pf]).all()) and bool(torch.isfinite(partial[n_pf:, :L.P_vf]).all())
        # (the value rows' ratio extrema, columns 4 and 5, are loaded by the fold and not used: they hold the -inf they start at)
        assert bool(torch.isfinite(scal[:n_pf, :7]).all()) and bool(torch.isfinite(scal[n_pf:, (0, 1, 2, 3, 6)]).all())
        assert not bool(torch.isnan(scal[:, :7]).any())
        check_gradient(got.double(), L, x, w, floors, label, errlog)
        # the info row: rel 1e-4, abs 1e-5 (times B on sums); 9 and 17 NaN exactly where A = 1; 20..23 keep the sentinel
        ratio = gr.info_error_ratio(info, w["info"], B)
        print("%s %s info %s\n want %s" % (pc.case_id(c), label, info, w["info"]))
        errlog(label + "_info_worst_over_bound", ratio, 1.0)
        assert ratio <= 1.0, (label, info, w["info"])
        assert [k for k in range(24) if np.isnan(info[k])] == ([9, 17] if A == 1 else [])
        assert (info[20:] == ref.SENTINEL).all()
        if x["kind"] == "clamp":
            hi, lo = pc.clamp_columns(A)
            d = got[L.P_pf - A:L.P_pf]
            assert float(d[hi]) == 0.0 and float(d[lo]) == 0.0, (label, d)
            assert all(float(d[k]) != 0.0 for k in range(A) if k not in (hi, lo))
            assert info[10] == 2.0 and info[11] == -20.0
        if x["kind"] == "tie" and clipv:
            # (db3 and dW3 of the value net are among the elements checked above: the 0.5 tie weight and the closed gate
            # interval show there; every term of the loss is on a binary grid)
            assert info[7] == pytest.approx(w["info"][7], rel=1e-6)
            sl = ref.block_slices(D, A, False)
            assert float(w["vf"][sl["b3"]].abs()) > 0 and bool((got[L.P_pf:][sl["W2"]] == 0).all())


def test_folded_gradient_does_not_depend_on_the_workgroup_split(errlog):
    loss_mode, clipv = pc.LOSSES[1]
    x, w, floors = want_of(pc.WG_CASE, loss_mode, clipv)
    L = Launch(x)
    outs = []
    for n_wg, n_wg_pf in pc.WG_SPLITS:
        got, info, _, _ = L.grad_and_fold(loss_mode, clipv, n_wg, n_wg_pf)
        check_gradient(got.double(), L, x, w, floors, "wg%d_pf%d" % (n_wg, n_wg_pf), errlog)
        assert gr.info_error_ratio(info, w["info"], x["rows"] * x["N"]) <= 1.0
        outs.append(got)
    assert not torch.equal(outs[0], outs[2])                                  # (another summation order, not the same launch)


# ---------------------------------------------------------------- the fold on synthetic rows
def adam_args(params, grads, m, v, sizes, lrs, max_norm, norms, step_count=1, grad_scale=1.0, device_state=0, step_state=None,
              device_lr=None):
    from torchrl_amd import _C
    a = _C.AdamArgs()
    a.params, a.grads, a.exp_avg, a.exp_avg_sq = params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr()
    a.n_groups = len(sizes)
    for k, n in enumerate(sizes):
        a.group_sizes[k], a.group_lr[k] = int(n), float(lrs[k])
    a.max_norm, a.beta1, a.beta2, a.eps, a.grad_scale = max_norm, 0.9, 0.999, 1e-5, grad_scale
    a.step_count, a.norms_out, a.device_state = step_count, (norms.data_ptr() if norms is not None else None), device_state
    a.step_state = step_state.data_ptr() if step_state is not None else None
    a.device_lr = device_lr.data_ptr() if device_lr is not None else None
    return a


@pytest.mark.parametrize("D,A", pc.FOLD_SHAPES)
@pytest.mark.parametrize("n_wg,n_pf", pc.FOLD_SPLITS)
def test_fold_on_synthetic_rows(D, A, n_wg, n_pf, errlog):
    from torchrl_amd import _C
    lib = _C.lib()
    ps = _C.ppo_partial_stride(D, H, A)
    p_pf, p_vf = pc.p_sizes(D, A)
    part, scal, logstd = pc.fold_case(D, A, n_wg, n_pf, ps, 100 * D + n_wg)
    params = torch.zeros(p_pf + p_vf)
    params[p_pf - A:p_pf] = logstd
    d_part, d_scal, d_params = dev(part), dev(scal), dev(params)
    grads = torch.full((p_pf + p_vf,), NAN, device=DEV)
    info = torch.full((24,), ref.SENTINEL, dtype=torch.float64, device=DEV)
    _C.ppo_reduce(d_part, d_scal, n_wg, D, H, A, grads, info, pf_params=d_params, n_wg_pf=n_pf)
    got, ginfo = grads.cpu().double(), info.cpu().numpy()
    worst = 0.0
    for rows, g in ((part[:n_pf, :p_pf], got[:p_pf]), (part[n_pf:n_wg, :p_vf], got[p_pf:])):
        want, S = ref.fold(rows)
        worst = max(worst, float(((g - want).abs() / ref.fold_bound(rows.shape[0], S)).max()))
    errlog("fold_err_over_bound", worst, 1.0)
    assert worst <= 1.0
    want = pc.fold_info(scal, n_wg, n_pf, logstd)
    for k in pc.FOLD_SUMS:
        assert ginfo[k] == pytest.approx(want[k], rel=1e-12), k              # doubles
    for k in pc.FOLD_EXACT:
        assert ginfo[k] == want[k], k
    for k in (8, 9, 10, 11, 16, 17, 18, 19):
        assert ginfo[k] == pytest.approx(want[k], rel=1e-12, abs=1e-15), k
    assert (ginfo[20:] == ref.SENTINEL).all()
    # pf_params = None: the log-std slots are left alone as well
    info2 = torch.full((24,), ref.SENTINEL, dtype=torch.float64, device=DEV)
    grads2 = torch.full((p_pf + p_vf,), NAN, device=DEV)
    _C.ppo_reduce(d_part, d_scal, n_wg, D, H, A, grads2, info2, pf_params=None, n_wg_pf=n_pf)
    i2 = info2.cpu().numpy()
    assert (i2[8:12] == ref.SENTINEL).all() and (i2[16:] == ref.SENTINEL).all()
    assert np.array_equal(i2[:8], ginfo[:8]) and np.array_equal(i2[12:16], ginfo[12:16]) and torch.equal(grads2, grads)
    # the fold inside trl_ppo_reduce_adam_f32: the same bits
    grads3 = torch.full((p_pf + p_vf,), NAN, device=DEV)
    info3 = torch.full((24,), ref.SENTINEL, dtype=torch.float64, device=DEV)
    ws = torch.zeros(lib.trl_ppo_reduce_adam_workspace(D, H, A), device=DEV)
    p3, m, v, norms = d_params.clone(), torch.zeros_like(d_params), torch.zeros_like(d_params), torch.zeros(2, device=DEV)
    a = adam_args(p3, grads3, m, v, (p_pf, p_vf), (3e-4, 1e-3), 0.5, norms)
    _C.check(lib.trl_ppo_reduce_adam_f32(d_part.data_ptr(), d_scal.data_ptr(), n_wg, n_pf, D, H, A, grads3.data_ptr(),
                                         info3.data_ptr(), C.byref(a), ws.data_ptr(), _C.stream_ptr(DEV)), "trl_ppo_reduce_adam_f32")
    torch.cuda.synchronize()
    assert int(ws[:1].view(torch.int32).item()) == 0                          # the norm rendezvous did not time out
    assert torch.equal(grads3, grads) and np.array_equal(info3.cpu().numpy(), ginfo)


# ---------------------------------------------------------------- clip + Adam
def run_adam(x, sizes, steps, state=None, use_device_lr=False, polyak=None):
    """The launches of `steps` = [(grads, lrs, max_norm, grad_scale, step_count or None)] -> (p, m, v, norms of every launch)."""
    from torchrl_amd import _C
    p, m, v = dev(x["p"]), dev(x["m"]), dev(x["v"])
    lr_dev = torch.zeros(4, device=DEV)
    out = []
    for grads, lrs, max_norm, gs, count in steps:
        g = dev(grads)
        norms = torch.full((5,), ref.SENTINEL, device=DEV)
        if use_device_lr:
            lr_dev[:len(sizes)].copy_(torch.tensor([float(l) for l in lrs]))
            lrs_host = [123.0] * len(sizes)                                   # (must not be read)
        else:
            lrs_host = lrs
        a = adam_args(p, g, m, v, sizes, lrs_host, max_norm, norms, count if count is not None else 0, gs,
                      step_state=state if count is None else None, device_lr=lr_dev if use_device_lr else None)
        if polyak is None:
            _C.clip_adam(a, DEV)
        else:
            polyak(a)
        out.append(norms.cpu().numpy())
    torch.cuda.synchronize()
    return p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), out


def check_adam(got, x, sizes, steps, label, errlog):
    p, m, v, norms = got
    opt, bound, r = ref.adam_chain(x, sizes, steps)
    ratios = ref.adam_error_ratios(p, m, v, opt, bound, pc.K_M, pc.K_V, pc.K_P, pc.K_R)
    print("%s: err / bound params %.3f, m %.3f, v %.3f" % (label, ratios["p"], ratios["m"], ratios["v"]))
    for k, val in ratios.items():
        errlog("%s_%s_over_bound" % (label, k), val, 1.0)
    assert max(ratios.values()) <= 1.0, (label, ratios)
    assert np.isfinite(p).all() and not np.array_equal(p, x["p"])
    max_norm = steps[-1][2]
    for k in range(len(sizes)):
        if max_norm <= 0.0:
            assert norms[-1][k] == 0.0, (label, k)                            # no clipping: the norm pass is skipped, 0 is written
        elif r["norms"][k] == 0.0:
            assert norms[-1][k] == 0.0, (label, k)                            # an empty or all-zero group
        else:
            assert norms[-1][k] == pytest.approx(r["norms"][k], rel=1e-5), (label, k)
    assert (norms[-1][len(sizes):] == np.float32(ref.SENTINEL)).all()         # nothing written behind the groups
    return opt


@pytest.mark.parametrize("sizes", pc.ADAM_LAYOUTS, ids=lambda s: "x".join(str(k) for k in s))
def test_clip_adam_vs_float64_restatement(sizes, errlog):
    for kind, max_norm, gs, count, zero in pc.adam_combos(sizes):
        x = pc.adam_case(sizes, kind, 17, zero)
        steps = [(x["g"], pc.ADAM_LRS, max_norm, gs, count)]
        label = "%s_mn%g_gs%g_t%d%s" % (kind, max_norm, gs, count, "" if zero is None else "_zero%d" % zero)
        check_adam(run_adam(x, sizes, steps), x, sizes, steps, label, errlog)


def fresh_state():
    return torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64, device=DEV)


def check_state(state, steps):
    s = state.cpu()
    assert float(s[0]) == float(steps)
    assert float(s[1]) == pytest.approx(ref.f32v(0.9) ** steps, rel=1e-15)
    assert float(s[2]) == pytest.approx(ref.f32v(0.999) ** steps, rel=1e-15)
    assert s[3:].view(torch.int32).tolist() == [0, 0]                         # the block counter is back at zero


@pytest.mark.parametrize("sizes", [(n,) for n in pc.TICK_SIZES] + [(255, 257), (4097, 3, 64, 8192)],
                         ids=lambda s: "x".join(str(k) for k in s))
def test_chain_of_launches_on_the_device_step_state(sizes, errlog):
    """5 launches on step_state with device_lr changed between them: 128 blocks (the last block ticks), 129 blocks (the
    one-thread tick launch), and two multi-group layouts."""
    n = int(sum(sizes))
    x = pc.adam_case(sizes, "big", 19)
    steps = pc.chain_steps(n, len(sizes))
    state = fresh_state()
    opt = check_adam(run_adam(x, sizes, steps, state=state, use_device_lr=True), x, sizes, steps, "chain", errlog)
    check_state(state, 5)
    assert opt.state[0] == 5.0


@pytest.mark.parametrize("n", pc.TICK_SIZES)
def test_clip_adam_polyak_ring_and_state_in_both_tick_modes(n, errlog):
    from torchrl_amd import _C
    sizes, slots, raw_bytes, tau = (n,), 3, 52, 0.005
    x = pc.adam_case(sizes, "big", 29)
    steps = pc.chain_steps(n, 1)
    state = fresh_state()
    rs = np.random.RandomState(n)
    n_t = pc.POLYAK_BIG if n == pc.TICK_SIZES[1] else 4099                    # the grid-stride loop once, a ragged small size once
    target = dev(rs.randn(n_t).astype(np.float32))
    ring = torch.full((slots, raw_bytes), 0xAB, dtype=torch.uint8, device=DEV)
    raws = [torch.from_numpy(rs.randint(0, 256, raw_bytes).astype(np.uint8)) for _ in steps]
    want_ring = ring.cpu().clone()
    u, worst = [0], [0.0]

    def polyak(a):
        k = u[0]
        source = rs.randn(n_t).astype(np.float32)
        t0 = target.cpu().numpy()
        _C.clip_adam_polyak(a, target, dev(source), tau, DEV, file=(dev(raws[k]), ring))
        torch.cuda.synchronize()
        want_ring[ref.ring_row(k, slots)] = raws[k]
        assert torch.equal(ring.cpu(), want_ring), k                          # row k % 3 holds update k's block, the others are untouched
        assert float(state[0].item()) == k + 1.0                              # advanced exactly once per update
        err = np.abs(target.cpu().numpy().astype(np.float64) - ref.polyak(t0, source, tau))
        worst[0] = max(worst[0], float((err / ref.polyak_bound(t0, source)).max()))
        u[0] += 1

    got = run_adam(x, sizes, steps, state=state, use_device_lr=True, polyak=polyak)
    check_adam(got, x, sizes, steps, "polyak_chain", errlog)
    check_state(state, 5)
    errlog("polyak_err_over_bound", worst[0], 1.0)
    assert 0.0 < worst[0] <= 1.0


# ---------------------------------------------------------------- gradient + fold-Adam, the workspace header
@pytest.mark.parametrize("c", pc.CHAIN_CASES, ids=pc.case_id)
def test_three_chained_updates_with_the_workspace_header(c, errlog):
    """trl_ppo_minibatch_grad_f32 + trl_ppo_reduce_adam_f32 with device_state = 1, three times: every launch's folded
    gradient against the restatement AT THE KERNEL'S CURRENT PARAMETERS (element bound), every Adam step against the float64
    step on the kernel's own folded gradient (running bounds), and the parameters at the end against three float64 updates on
    float64 gradients (the project's bound on post-step parameters, abs 1e-6)."""
    from torchrl_amd import _C
    lib = _C.lib()
    loss_mode, clipv = pc.LOSSES[1]
    x = pc.grad_inputs(c)
    mb = pc.minibatch(x)
    L = Launch(x)
    D, A, n_wg, n_wg_pf = x["D"], x["A"], x["n_wg"], x["n_wg_pf"]
    sizes, lrs = (L.P_pf, L.P_vf), (np.float32(3e-4), np.float32(1e-3))
    mv = pc.adam_case(sizes, "big", 31)
    flat, m, v = L.flat0.clone(), dev(mv["m"]), dev(mv["v"])
    grads = torch.zeros_like(flat)
    ws = torch.zeros(lib.trl_ppo_reduce_adam_workspace(D, H, A), device=DEV)
    ws[4:8].view(torch.float64).fill_(1.0)
    ws[2:4] = torch.tensor([float(l) for l in lrs])
    floors = ref.grad_floor(mb, x["pf"], x["vf"], x["act"], x["n_global"])
    own = ref.AdamRef(flat.cpu().numpy(), mv["m"], mv["v"], sizes)           # float64 Adam on the kernel's own gradients
    bound = ref.AdamBound(flat.numel())
    for k in range(3):
        p_now = flat.cpu().numpy()
        partial, scal = L.rows(n_wg)
        info = torch.full((24,), ref.SENTINEL, dtype=torch.float64, device=DEV)
        norms = torch.zeros(2, device=DEV)
        _C.ppo_minibatch_grad(L.args(flat, loss_mode, clipv, n_wg, n_wg_pf, partial, scal), DEV)
        a = adam_args(flat, grads, m, v, sizes, (77.0, 77.0), 0.5, norms, step_count=0, device_state=1)   # (lr, count: the header's)
        _C.check(lib.trl_ppo_reduce_adam_f32(partial.data_ptr(), scal.data_ptr(), n_wg, n_wg_pf, D, H, A, grads.data_ptr(),
                                             info.data_ptr(), C.byref(a), ws.data_ptr(), _C.stream_ptr(DEV)), "trl_ppo_reduce_adam_f32")
        torch.cuda.synchronize()
        w = ref.grads_at(p_now, x, mb, loss_mode, clipv, torch.float64, pc.C_ENT)
        check_gradient(grads.cpu().double(), L, x, w, floors, "update%d" % k, errlog)
        assert gr.info_error_ratio(info.cpu().numpy(), w["info"], x["rows"] * x["N"]) <= 1.0
        r = own.step(grads.cpu().numpy(), lrs, 0.5, 1.0, None)
        bound.add(r, own)
        assert norms.cpu().numpy() == pytest.approx(r["norms"], rel=1e-5)
    ratios = ref.adam_error_ratios(flat.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), own, bound, pc.K_M, pc.K_V, pc.K_P, pc.K_R)
    for name, val in ratios.items():
        errlog("adam_%s_over_bound" % name, val, 1.0)
    assert max(ratios.values()) <= 1.0, ratios
    head = ws[:8].cpu()
    assert head[:2].view(torch.int32).tolist() == [0, 3]                      # no time-out; three steps taken
    assert head[2:4].tolist() == [float(l) for l in lrs]
    pw = head[4:8].view(torch.float64).tolist()
    assert pw[0] == pytest.approx(ref.f32v(0.9) ** 3, rel=1e-15) and pw[1] == pytest.approx(ref.f32v(0.999) ** 3, rel=1e-15)
    want = ref.update_chain(x, mb, mv, lrs, 3, loss_mode, clipv, pc.C_ENT)
    err = float(np.abs(flat.cpu().numpy().astype(np.float64) - want.p).max())
    errlog("params_after_3_updates_abs", err, 1e-6)
    assert err <= 1e-6 and want.state[0] == 3.0
