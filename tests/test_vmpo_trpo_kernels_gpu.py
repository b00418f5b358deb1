"""The V-MPO and TRPO loss kernels (torchrl_amd/csrc/k_vmpo.hip, k_trpo.hip), each entry point called directly and
compared with the torch restatement in float64 (tests/_vmpo_trpo_ref.py) on identical float32 inputs: one partial wave,
exactly one block, one valid lane in the second block, two blocks with a ragged tail and four blocks; A = 1, 6 and 64; both
tanh_action values; the log_std clamp gate, small eta, the dual variables' floor, n = 1, repeatability and the refusals.
tests/test_vmpo_trpo_kernels_cpu.py checks the restatement and that the inputs make each comparison mean something.

The bounds are the project's (tests/test_gauss_sd_gpu.py::test_losses_vs_restatement_in_float64): d_mean rel 1e-4 and
abs 1e-4 / n, d_logstd rel 1e-4 and abs 1e-5 times the float64 sum over samples of the absolute per-sample term, logged
statistics rel 1e-4 / abs 1e-5, eta and alpha rel 2e-6 (tests/test_vmpo_gpu.py), Adam's moments rel 1e-4.  Every test
prints its worst err / bound (profiles/NOTES_vmpo_trpo_tests.md has them from one run)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _vmpo_trpo_ref as ref                                                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = lambda x: float(np.float32(x))
SENTINEL = 7.0
VMPO_KEYS = ("mean", "tmean", "logstd", "tlogstd", "acts", "adv")
TRPO_KEYS = ("mean", "logstd", "acts", "adv")


def dev(x):
    return x.to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def vmpo_cases():
    return {name: (c, tanh, eta) for name, c, tanh, eta in ref.vmpo_cases()}


@functools.lru_cache(maxsize=None)
def trpo_cases():
    return {name: (c, tanh) for name, c, tanh in ref.trpo_cases()}


MAIN_IDS = ["n%d-A%d-tanh%d" % (n, A, t) for n, A in ref.SHAPES for t in (0, 1)]


# ---------------------------------------------------------------- V-MPO
def run_vmpo(c, tanh, dual, eta_eps=0.02, alpha_eps=0.1, lr=1e-3, want=True):
    """-> (got, want): the kernel's outputs on the CPU and the float64 restatement on the same float32 values."""
    from torchrl_amd import _C
    n, A = c["mean"].shape
    dual32 = np.asarray(dual, dtype=np.float32)
    dual_d = torch.from_numpy(dual32.copy()).to(DEV)
    d_logstd = torch.full((A,), SENTINEL, device=DEV)
    info = torch.full((12,), SENTINEL, dtype=torch.float64, device=DEV)
    d_mean = _C.vmpo_losses(*[dev(c[k]) for k in VMPO_KEYS], dual_d, tanh, eta_eps, alpha_eps, lr, d_logstd, info)
    torch.cuda.synchronize()
    got = dict(d_mean=d_mean.cpu(), d_logstd=d_logstd.cpu(), info=info.cpu().numpy(), dual=dual_d.cpu().numpy())
    if not want:
        return got, None
    return got, ref.vmpo_losses(*[c[k].double() for k in VMPO_KEYS], dual32.astype(np.float64), tanh, F32(eta_eps),
                                F32(alpha_eps), F32(lr))


def check_vmpo(label, got, want, moments=True):
    n = want["d_mean"].shape[0]
    dm, dl = ref.grad_ratios(got, want)
    inf = ref.info_ratios(got["info"], want["info"], (2, 6) if n == 1 else ())
    du = ref.dual_ratios(got["dual"], want["dual"].numpy(), moments)
    print("RATIO vmpo %s: d_mean %.4f d_logstd %.4f info %.4f (slot %d) dual %.4f (slot %d)"
          % (label, dm, dl, max(inf), int(np.argmax(inf)), max(du), int(np.argmax(du))))
    assert torch.isfinite(got["d_mean"]).all() and torch.isfinite(got["d_logstd"]).all()
    assert dm <= 1.0, "d_mean"
    assert dl <= 1.0, "d_logstd"
    assert max(inf) <= 1.0, ("info", inf)
    assert max(du) <= 1.0, ("dual", du)


@pytest.mark.parametrize("case", MAIN_IDS)
def test_vmpo_losses_vs_restatement_in_float64(case):
    """d_mean, d_logstd, all 12 info slots and the dual state after the call, eta = 1, alpha = 0.1."""
    c, tanh, eta = vmpo_cases()[case]
    got, want = run_vmpo(c, tanh, ref.DUAL0)
    check_vmpo(case, got, want)
    assert got["dual"][6] == 1.0


def test_vmpo_three_chained_calls_carry_the_dual_state():
    """Fresh batches, the dual state handed from call to call: the same bounds after every call."""
    dual_got, dual_want = np.asarray(ref.DUAL0, dtype=np.float32), None
    for s in range(3):
        c = ref.policy_case(300, 6, True, 7700 + s)
        c["adv"] = ref.vmpo_adv(300, 60 + s)
        got, _ = run_vmpo(c, True, dual_got, want=False)
        # the restatement carries ITS state (float64) -- the comparison is of two whole chains, not of single steps
        want = ref.vmpo_losses(*[c[k].double() for k in VMPO_KEYS], ref.DUAL0 if dual_want is None else dual_want, True,
                               F32(0.02), F32(0.1), F32(1e-3))
        check_vmpo("chain call %d" % s, got, want)
        dual_got, dual_want = got["dual"], want["dual"]
    assert dual_got[6] == 3.0


@pytest.mark.parametrize("n", [300, 1000])
def test_vmpo_small_eta(n):
    """eta = 0.02: max(adv) / eta > 88, where a float32 exp overflows unless the maximum is subtracted first.  One call:
    a second step would depend on the last digits of eta's gradient, a difference of two terms of ~max(adv) / eta."""
    c, tanh, eta = vmpo_cases()["small-eta-n%d" % n]
    assert c["adv"].max().item() / eta > 88.73
    dual = list(ref.DUAL0)
    dual[0] = eta
    got, want = run_vmpo(c, tanh, dual)
    assert np.isfinite(got["info"]).all() and np.isfinite(got["dual"]).all()
    check_vmpo("small eta n=%d" % n, got, want, moments=False)
    assert got["dual"][6] == 1.0                                            # the step count does not depend on the gradient


@pytest.mark.parametrize("which", ["eta", "alpha"])
def test_vmpo_dual_floor(which):
    """dual_lr = 10 takes eta (eta_eps = 1: its gradient is positive) or alpha (alpha_eps = 10) below zero: the value
    afterwards is exactly 1e-8f, the other variable moved the other way, and the info slots are finite."""
    c, tanh, _ = vmpo_cases()["n300-A6-tanh1"]
    eta_eps, alpha_eps = (1.0, 0.0) if which == "eta" else (0.02, 10.0)
    got, want = run_vmpo(c, tanh, ref.DUAL0, eta_eps=eta_eps, alpha_eps=alpha_eps, lr=10.0)
    k = 0 if which == "eta" else 1
    print("RATIO vmpo floor %s: dual after the step %s" % (which, got["dual"][:2]))
    assert got["dual"][k] == np.float32(1e-8) and want["dual"][k].item() == 1e-8
    assert got["dual"][1 - k] > 5.0
    assert np.isfinite(got["info"]).all()
    assert got["info"][11 - k] == float(np.float32(1e-8))                   # slots 10 / 11: alpha / eta AFTER the step
    check_vmpo("floor " + which, got, want)


def test_vmpo_clamp_gate():
    """logstd[1] = -25, logstd[4] = 3, target_logstd[2] = 3, n = 300 (the gate is folded over two blocks): the closed
    entries get exactly 0, the others do not, everything is finite, and all outputs agree with the restatement, which
    clamps the same way (the clamped target log_std in the KL included)."""
    c, tanh, _ = vmpo_cases()["gate"]
    got, want = run_vmpo(c, tanh, ref.DUAL0)
    assert got["d_logstd"][1] == 0.0 and got["d_logstd"][4] == 0.0
    assert all(got["d_logstd"][o] != 0.0 for o in (0, 2, 3, 5))
    assert torch.isfinite(got["d_mean"]).all() and np.isfinite(got["info"]).all() and np.isfinite(got["dual"]).all()
    check_vmpo("gate", got, want)


def test_vmpo_single_sample():
    for t in (0, 1):
        c, tanh, _ = vmpo_cases()["n1-A6-tanh%d" % t]
        got, want = run_vmpo(c, tanh, ref.DUAL0)
        assert np.isnan(got["info"][2]) and np.isnan(got["info"][6])
        assert np.isfinite(np.delete(got["info"], (2, 6))).all()
        check_vmpo("n=1 tanh=%d" % t, got, want)


def test_vmpo_repeat_is_bit_identical():
    c, tanh, _ = vmpo_cases()["n1000-A6-tanh1"]
    a, _ = run_vmpo(c, tanh, ref.DUAL0, want=False)
    b, _ = run_vmpo(c, tanh, ref.DUAL0, want=False)
    assert torch.equal(a["d_mean"], b["d_mean"]) and torch.equal(a["d_logstd"], b["d_logstd"])
    assert np.array_equal(a["info"], b["info"]) and np.array_equal(a["dual"], b["dual"])


def _raw_vmpo(n, A, rows):
    """The entry point itself with buffers of `rows` rows: -> (return code, outputs, dual)."""
    from torchrl_amd import _C
    L, p = _C.lib(), _C.dev_ptr
    x = [torch.zeros(rows, A, device=DEV) for _ in range(3)]
    ls, adv = torch.zeros(A, device=DEV), torch.zeros(rows, device=DEV)
    dual = torch.tensor(ref.DUAL0, dtype=torch.float32, device=DEV)
    d_mean, d_ls = torch.full((rows, A), SENTINEL, device=DEV), torch.full((A,), SENTINEL, device=DEV)
    info = torch.full((12,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = torch.zeros(4 + 4 * (A + 9), dtype=torch.float64, device=DEV)
    code = L.trl_vmpo_losses_f32(p(x[0]), p(x[1]), p(ls), p(ls), p(x[2]), p(adv), p(dual), n, A, 1, 0.02, 0.1, 1e-3, p(d_mean),
                                 p(d_ls), p(info, torch.float64), p(ws, torch.float64), _C.stream_ptr(DEV))
    torch.cuda.synchronize()
    return code, (d_mean, d_ls, info), dual


def test_vmpo_refusals():
    from torchrl_amd import _C
    L = _C.lib()
    assert L.trl_vmpo_losses_workspace(300, 65) < 0 and L.trl_vmpo_losses_workspace(0, 6) < 0
    assert L.trl_vmpo_losses_workspace(300, 64) == 4 + 2 * (64 + 9)
    for n, A in ((300, 65), (0, 6)):
        code, outs, dual = _raw_vmpo(n, A, 300)
        assert code != 0
        assert all(bool((o == SENTINEL).all()) for o in outs)
        assert torch.equal(dual.cpu(), torch.tensor(ref.DUAL0, dtype=torch.float32))
    with pytest.raises(_C.TrlError):
        z = torch.zeros(8, 65, device=DEV)
        _C.vmpo_losses(z, z, z[0], z[0], z, z[:, 0].contiguous(), torch.tensor(ref.DUAL0, device=DEV), True, 0.02, 0.1, 1e-3,
                       torch.zeros(65, device=DEV), torch.zeros(12, dtype=torch.float64, device=DEV))


# ---------------------------------------------------------------- TRPO
def run_trpo(c, tanh, c_ent, want=True, **kw):
    from torchrl_amd import _C
    n, A = c["mean"].shape
    d_logstd = torch.full((A,), SENTINEL, device=DEV)
    info = torch.full((5,), SENTINEL, dtype=torch.float64, device=DEV)
    d_mean = _C.trpo_surrogate(*[dev(c[k]) for k in TRPO_KEYS], tanh, c_ent, d_logstd, info)
    torch.cuda.synchronize()
    got = dict(d_mean=d_mean.cpu(), d_logstd=d_logstd.cpu(), info=info.cpu().numpy())
    if not want:
        return got, None
    return got, ref.trpo_surrogate(*[c[k].double() for k in TRPO_KEYS], tanh, F32(c_ent), **kw)


def check_trpo(label, got, want):
    n = want["d_mean"].shape[0]
    dm, dl = ref.grad_ratios(got, want)
    inf = ref.info_ratios(got["info"], want["info"], (2,) if n == 1 else ())
    print("RATIO trpo %s: d_mean %.4f d_logstd %.4f info %.4f (slot %d)" % (label, dm, dl, max(inf), int(np.argmax(inf))))
    assert torch.isfinite(got["d_mean"]).all() and torch.isfinite(got["d_logstd"]).all()
    assert dm <= 1.0, "d_mean"
    assert dl <= 1.0, "d_logstd"
    assert max(inf) <= 1.0, ("info", inf)


@pytest.mark.parametrize("case", MAIN_IDS)
def test_trpo_surrogate_vs_restatement_in_float64(case):
    """d_mean, d_logstd and the 5 info slots at entropy_coeff 0 and 0.01; log pi is spread over [-22, -6], where the
    weight w = p / (p + 1e-8) moves between 0 and 1 (test_trpo_inputs_move_the_weight)."""
    c, tanh = trpo_cases()[case]
    for c_ent in (0.0, 0.01):
        got, want = run_trpo(c, tanh, c_ent)
        check_trpo("%s c_ent=%g" % (case, c_ent), got, want)


def test_trpo_wide_log_prob_pins_the_weight():
    """log pi over [-30, -8]: the kernel agrees with the restatement, and a kernel with w = 1 could not -- the float64
    gradients with and without the 1e-8 differ by more than ten times the bound on at least 20 % of the elements."""
    c, tanh = trpo_cases()["wide"]
    got, want = run_trpo(c, tanh, 0.01)
    w_one = ref.trpo_surrogate(*[c[k].double() for k in TRPO_KEYS], tanh, F32(0.01), prob_eps=0.0)
    n = c["mean"].shape[0]
    bound = 1e-4 / n + 1e-4 * want["d_mean"].abs()
    assert ((want["d_mean"] - w_one["d_mean"]).abs() > 10 * bound).double().mean() >= 0.2
    assert ref.grad_ratios(dict(d_mean=w_one["d_mean"], d_logstd=w_one["d_logstd"]), want)[0] > 10
    check_trpo("wide", got, want)


def test_trpo_clamp_gate():
    """As for V-MPO; the entropy term of d_logstd is gated too (with entropy_coeff = 0.01 an ungated entropy term alone
    would leave -0.01 there), and the entropy in info[0] uses the clamped values."""
    c, tanh = trpo_cases()["gate"]
    got, want = run_trpo(c, tanh, 0.01)
    assert got["d_logstd"][1] == 0.0 and got["d_logstd"][4] == 0.0
    assert all(got["d_logstd"][o] != 0.0 for o in (0, 2, 3, 5))
    assert torch.isfinite(got["d_mean"]).all() and np.isfinite(got["info"]).all()
    check_trpo("gate", got, want)
    got0, want0 = run_trpo(c, tanh, 0.0)
    ent = (0.5 + ref.HALF_LOG_2PI + c["logstd"].double().clamp(-20, 2)).sum().item()
    raw_ent = (0.5 + ref.HALF_LOG_2PI + c["logstd"].double()).sum().item()
    assert abs(ent - raw_ent) > 3.9
    assert got0["info"][0] - got["info"][0] == pytest.approx(F32(0.01) * ent, rel=1e-4, abs=1e-5)


def test_trpo_single_sample():
    for t in (0, 1):
        c, tanh = trpo_cases()["n1-A6-tanh%d" % t]
        got, want = run_trpo(c, tanh, 0.01)
        assert np.isnan(got["info"][2]) and np.isfinite(np.delete(got["info"], 2)).all()
        check_trpo("n=1 tanh=%d" % t, got, want)


def test_trpo_repeat_is_bit_identical():
    c, tanh = trpo_cases()["n1000-A6-tanh1"]
    a, _ = run_trpo(c, tanh, 0.01, want=False)
    b, _ = run_trpo(c, tanh, 0.01, want=False)
    assert torch.equal(a["d_mean"], b["d_mean"]) and torch.equal(a["d_logstd"], b["d_logstd"])
    assert np.array_equal(a["info"], b["info"])


def test_trpo_refusals():
    from torchrl_amd import _C
    L, p = _C.lib(), _C.dev_ptr
    assert L.trl_trpo_surrogate_workspace(300, 65) < 0 and L.trl_trpo_surrogate_workspace(0, 6) < 0
    assert L.trl_trpo_surrogate_workspace(300, 64) == 2 * (64 + 5)
    for n, A in ((300, 65), (0, 6)):
        x = [torch.zeros(300, A, device=DEV) for _ in range(2)]
        ls, adv = torch.zeros(A, device=DEV), torch.zeros(300, device=DEV)
        d_mean, d_ls = torch.full((300, A), SENTINEL, device=DEV), torch.full((A,), SENTINEL, device=DEV)
        info = torch.full((5,), SENTINEL, dtype=torch.float64, device=DEV)
        ws = torch.zeros(4 * (A + 5), dtype=torch.float64, device=DEV)
        code = L.trl_trpo_surrogate_f32(p(x[0]), p(ls), p(x[1]), p(adv), n, A, 0, 0.01, p(d_mean), p(d_ls), p(info, torch.float64),
                                        p(ws, torch.float64), _C.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert code != 0
        assert all(bool((o == SENTINEL).all()) for o in (d_mean, d_ls, info))
    with pytest.raises(_C.TrlError):
        z = torch.zeros(8, 65, device=DEV)
        _C.trpo_surrogate(z, z[0], z, z[:, 0].contiguous(), False, 0.01, torch.zeros(65, device=DEV),
                          torch.zeros(5, dtype=torch.float64, device=DEV))


# ---------------------------------------------------------------- the small kernels
def _f32(rs, *shape):
    return torch.from_numpy(rs.randn(*shape).astype(np.float32))


@pytest.mark.parametrize("eps", [1e-5, 1e-4])
@pytest.mark.parametrize("B", [2, 255, 256, 257, 5000])
def test_adv_normalize(B, eps):
    """n_global == B (one rank) and n_global == 2 B (the statistics come from twice as many values, of which the kernel
    sees half).  rel 1e-6 + abs 1e-6 against float64: the float32 mean is rounded once, and 6e-8 |mean| / std stays below
    the abs term at advantages of 2 N(0, 1) + 0.5."""
    from torchrl_amd import _C
    worst = 0.0
    for mult in (1, 2):
        allv = 2.0 * _f32(np.random.RandomState(300 + B + mult), mult * B) + 0.5
        a64 = allv.double()
        raw = torch.tensor([a64.sum(), (a64 ** 2).sum(), a64.max(), -a64.min()], dtype=torch.float64)
        got = _C.adv_normalize(dev(allv[:B]), dev(raw), float(mult * B), eps)
        torch.cuda.synchronize()
        want = ref.adv_normalize(a64[:B], a64, F32(eps))
        err = (got.cpu().double() - want).abs()
        worst = max(worst, (err / (1e-6 + 1e-6 * want.abs())).max().item())
    print("RATIO adv_normalize B=%d eps=%g: %.4f" % (B, eps, worst))
    assert worst <= 1.0


def test_adv_normalize_refuses_one_sample():
    from torchrl_amd import _C
    with pytest.raises(_C.TrlError):
        _C.adv_normalize(torch.zeros(1, device=DEV), torch.zeros(4, dtype=torch.float64, device=DEV), 1.0, 1e-5)


@pytest.mark.parametrize("B", [1, 255, 256, 257, 5000])
def test_mse_value_loss(B):
    """One block striding over B; d_v = 2 (v - R) / n_global and the local loss sum, rel 1e-6 each, n_global = B and 2 B
    (what TRPO passes)."""
    from torchrl_amd import _C
    rs = np.random.RandomState(400 + B)
    v, R = _f32(rs, B), _f32(rs, B)
    worst = 0.0
    for ng in (B, 2 * B):
        loss = torch.full((1,), SENTINEL, dtype=torch.float64, device=DEV)
        d_v = _C.mse_value_loss(dev(v), dev(R), float(ng), loss)
        torch.cuda.synchronize()
        want_dv, want_loss = ref.mse_value(v.double(), R.double(), float(ng))
        assert d_v.shape == (B, 1)
        err = (d_v.view(-1).cpu().double() - want_dv).abs()
        r = torch.where(want_dv == 0, (err != 0).double() * 2.0, err / (1e-6 * want_dv.abs()))    # v == R: exactly zero
        worst = max(worst, r.max().item(),
                    abs(loss.item() - want_loss.item()) / (1e-6 * want_loss.item()))
    print("RATIO mse_value_loss B=%d: %.4f" % (B, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("n", [1, 257, 5000])
def test_ratio_loss(n):
    """-mean(exp(lp_new - lp_old) adv), lp_new - lp_old uniform in [-2, 2].  The sum cancels, so the bound is on the
    terms: abs 1e-5 * mean |ratio adv| from float64."""
    from torchrl_amd import _C
    rs = np.random.RandomState(500 + n)
    lp_old = 3.0 * _f32(rs, n) - 10.0
    lp_new = lp_old + torch.from_numpy(rs.uniform(-2, 2, n).astype(np.float32))
    adv = _f32(rs, n)
    out = torch.full((1,), SENTINEL, dtype=torch.float64, device=DEV)
    _C.ratio_loss(dev(lp_new), dev(lp_old), dev(adv), out)
    torch.cuda.synchronize()
    want = ref.ratio_loss(lp_new.double(), lp_old.double(), adv.double()).item()
    bound = 1e-5 * (torch.exp(lp_new.double() - lp_old.double()) * adv.double()).abs().mean().item()
    print("RATIO ratio_loss n=%d: %.4f" % (n, abs(out.item() - want) / bound))
    assert abs(out.item() - want) <= bound


@pytest.mark.parametrize("act", ["none", "relu", "tanh"])
@pytest.mark.parametrize("n", [1, 255, 257, 70000])
def test_jvp_gate(n, act):
    """out = act'(h) (a + b) with b given or null and h given or null; h from ReLU holds exact zeros, where the gate is 0.
    Bound 1e-6 |want| + 2e-7 |a + b|: 1 - y y may be contracted to an fma, which moves the factor by one ulp of 1."""
    from torchrl_amd import _C
    code = {"none": _C.ACT_NONE, "relu": _C.ACT_RELU, "tanh": _C.ACT_TANH}[act]
    assert (_C.ACT_TANH, _C.ACT_RELU, _C.ACT_NONE) == (ref.ACT_TANH, ref.ACT_RELU, ref.ACT_NONE)
    rs = np.random.RandomState(600 + n)
    a, b, pre = _f32(rs, n), _f32(rs, n), _f32(rs, n)
    h = {"none": pre, "relu": torch.relu(pre), "tanh": torch.tanh(pre)}[act]
    if act == "relu" and n > 1:
        assert (h == 0).any() and (h > 0).any()
    worst = 0.0
    for bb in (b, None):
        for hh in (h, None):
            got = _C.jvp_gate(dev(a), None if bb is None else dev(bb), None if hh is None else dev(hh), code)
            torch.cuda.synchronize()
            want = ref.jvp_gate(a.double(), None if bb is None else bb.double(), None if hh is None else hh.double(), code)
            s = a.double() if bb is None else a.double() + bb.double()
            r = ((got.cpu().double() - want).abs() / (1e-6 * want.abs() + 2e-7 * s.abs())).max().item()
            worst = max(worst, r)
            if act == "relu" and hh is not None:
                assert bool((got.cpu()[h == 0] == 0).all())
    print("RATIO jvp_gate n=%d act=%s: %.4f" % (n, act, worst))
    assert worst <= 1.0


def test_jvp_gate_of_nothing_touches_nothing():
    from torchrl_amd import _C
    a, out = torch.ones(4, device=DEV), torch.full((4,), SENTINEL, device=DEV)
    code = _C.lib().trl_jvp_gate_f32(_C.dev_ptr(a), None, None, _C.ACT_TANH, 0, _C.dev_ptr(out), _C.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert code == 0 and bool((out == SENTINEL).all())


@pytest.mark.parametrize("n,A", [(1, 1), (300, 6), (257, 7), (100, 64)])
def test_fisher_scale(n, A):
    """out[b, o] = d_mu[b, o] exp(-2 clamp(logstd[o])) / n, rel 1e-5; the flat index e -> logstd[e % A] crosses block
    boundaries at A = 6 and 7, which do not divide 256.  One log_std is below -20 and one above 2 (A = 1: above 2)."""
    from torchrl_amd import _C
    rs = np.random.RandomState(700 + n + A)
    d_mu = _f32(rs, n, A)
    logstd = torch.from_numpy(rs.uniform(-1.5, 0.5, A).astype(np.float32))
    if A == 1:
        logstd[0] = 3.0
    else:
        logstd[1], logstd[4] = -25.0, 3.0
    got = _C.fisher_scale(dev(d_mu), dev(logstd))
    torch.cuda.synchronize()
    want = ref.fisher_scale(d_mu.double(), logstd.double())
    r = ((got.cpu().double() - want).abs() / (1e-5 * want.abs())).max().item()
    print("RATIO fisher_scale n=%d A=%d: %.4f" % (n, A, r))
    assert got.shape == (n, A) and r <= 1.0
