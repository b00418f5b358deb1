"""Checks of the oracle and of the inputs that tests/test_vmpo_trpo_kernels_gpu.py compares the V-MPO and TRPO loss
kernels with: the torch restatement (tests/_vmpo_trpo_ref.py) against torch.distributions and against the closed-form
gradients in the headers of k_vmpo.hip / k_trpo.hip, the conditions that keep a GPU comparison from comparing nothing,
and the float32 run of the restatement against its float64 run under the GPU test's bounds.  Needs no GPU and no library."""
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

KEYS = ("mean", "tmean", "logstd", "tlogstd", "acts", "adv")


@functools.lru_cache(maxsize=None)
def vmpo_cases():
    return ref.vmpo_cases()


@functools.lru_cache(maxsize=None)
def trpo_cases():
    return ref.trpo_cases()


def vmpo64(c, tanh, eta, dtype=torch.float64):
    dual = list(ref.DUAL0)
    dual[0] = float(np.float32(eta))
    return ref.vmpo_losses(*[c[k].to(dtype) for k in KEYS], dual, tanh, 0.02, 0.1, 1e-3)


def trpo64(c, tanh, c_ent=0.01, dtype=torch.float64, **kw):
    return ref.trpo_surrogate(*[c[k].to(dtype) for k in ("mean", "logstd", "acts", "adv")], tanh, c_ent, **kw)


def close(a, b):
    np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------- the oracle
def test_log_prob_and_kl_equal_torch_distributions():
    for name, c, tanh, _ in vmpo_cases():
        d = {k: v.double() for k, v in c.items()}
        ls, tls = d["logstd"].clamp(-20, 2), d["tlogstd"].clamp(-20, 2)
        pi = torch.distributions.Normal(d["mean"], torch.exp(ls).expand_as(d["mean"]))
        tgt = torch.distributions.Normal(d["tmean"], torch.exp(tls).expand_as(d["mean"]))
        pre, corr = d["acts"], torch.zeros_like(d["acts"])
        if tanh:
            pre = torch.log((1 + d["acts"]) / (1 - d["acts"])) / 2
            corr = torch.log(1 - d["acts"] * d["acts"] + 1e-6)
        close(ref.logp(d["mean"], d["logstd"], d["acts"], tanh), (pi.log_prob(pre) - corr).sum(-1))
        close(ref.kl_rows(d["mean"], ls, d["tmean"], tls), torch.distributions.kl_divergence(pi, tgt).sum(-1))


def _closed_form_parts(d, tanh):
    ls = d["logstd"].clamp(-20, 2)
    gate = ((d["logstd"] >= -20) & (d["logstd"] <= 2)).double()
    pre = torch.log((1 + d["acts"]) / (1 - d["acts"])) / 2 if tanh else d["acts"]
    return ls, gate, pre - d["mean"], torch.exp(2 * ls)


def test_vmpo_gradients_equal_the_closed_forms():
    """d_mean = g_lp zc / var + alpha / n dm / tvar, d_logstd = gate sum_b (g_lp (zc^2 / var - 1) + alpha / n (var / tvar - 1)),
    g_lp = -phi / n (header of k_vmpo.hip); the dual gradients eps + log mean exp(a / eta) - sum_b phi_b a_b / eta and
    eps - mean KL enter Adam's first step as lr g / (|g| + 1e-5)."""
    for name, c, tanh, eta in vmpo_cases():
        d = {k: v.double() for k, v in c.items()}
        r = vmpo64(c, tanh, eta)
        n = d["mean"].shape[0]
        ls, gate, zc, var = _closed_form_parts(d, tanh)
        tvar, dm = torch.exp(2 * d["tlogstd"].clamp(-20, 2)), d["mean"] - d["tmean"]
        g_lp = (-r["phi"] / n)[:, None]
        close(r["d_mean"], g_lp * zc / var + 0.1 / n * dm / tvar)
        close(r["d_logstd"], gate * (g_lp * (zc * zc / var - 1) + 0.1 / n * (var / tvar - 1)).sum(0))
        e = float(np.float32(eta))
        g_eta = 0.02 + torch.logsumexp(d["adv"] / e, 0) - np.log(n) - (r["phi"] * d["adv"]).sum() / e
        g_alpha = 0.1 - r["kl"].mean()
        for k, (g, before) in enumerate(((g_eta, e), (g_alpha, 0.1))):
            assert r["dual"][k].item() == pytest.approx(max(before - 1e-3 * g.item() / (abs(g.item()) + 1e-5), 1e-8), rel=1e-10), name
            assert r["dual"][2 + k].item() == pytest.approx(0.1 * g.item(), rel=1e-9, abs=1e-15)
        assert r["dual"][6].item() == 1.0
        assert r["info"][9] == pytest.approx(0.1 * 0.1 - 0.1 * r["kl"].mean().item(), rel=1e-12)      # alpha BEFORE the step
        assert r["info"][10] == r["dual"][1].item() and r["info"][11] == r["dual"][0].item()


def test_trpo_gradients_equal_the_closed_forms():
    """d_mean = -adv w / n zc / var, d_logstd = gate sum_b (-adv w / n (zc^2 / var - 1) - c_ent / n), w = p / (p + 1e-8)."""
    for name, c, tanh in trpo_cases():
        d = {k: v.double() for k, v in c.items()}
        n = d["mean"].shape[0]
        ls, gate, zc, var = _closed_form_parts(d, tanh)
        p = torch.exp(ref.logp(d["mean"], d["logstd"], d["acts"], tanh))
        for c_ent in (0.0, 0.01):
            r = trpo64(c, tanh, c_ent)
            close(r["w"], p / (p + 1e-8))
            g_lp = (-d["adv"] * r["w"] / n)[:, None]
            close(r["d_mean"], g_lp * zc / var)
            close(r["d_logstd"], gate * (g_lp * (zc * zc / var - 1) - c_ent / n).sum(0))
            ent = (0.5 + ref.HALF_LOG_2PI + ls).sum()
            assert r["info"][0] == pytest.approx((-(r["w"] * d["adv"]).mean() - c_ent * ent).item(), rel=1e-12, abs=1e-12)


def test_dual_state_carried_between_calls_equals_one_persistent_adam():
    """Three calls that hand the 7-value dual state on == one torch.optim.Adam(lr, eps=1e-5) stepping eta and alpha with
    the same three gradient pairs, each followed by clamp_(min=1e-8)."""
    eta, alpha = torch.tensor([1.0], dtype=torch.float64, requires_grad=True), torch.tensor([0.1], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([eta, alpha], lr=1e-3, eps=1e-5)
    dual = list(ref.DUAL0)
    for s in range(3):
        c = ref.vmpo_case(48, 6, True)
        c["adv"] = ref.vmpo_adv(48, 40 + s)
        d = {k: v.double() for k, v in c.items()}
        kl = ref.kl_rows(d["mean"], d["logstd"].clamp(-20, 2), d["tmean"], d["tlogstd"].clamp(-20, 2)).mean()
        loss = eta * 0.02 + eta * torch.log(torch.mean(torch.exp(d["adv"] / eta))) + alpha * 0.1 - alpha * kl   # v_mpo.py:89-96
        opt.zero_grad()
        loss.sum().backward()
        opt.step()
        with torch.no_grad():
            eta.clamp_(min=1e-8)
            alpha.clamp_(min=1e-8)
        dual = ref.vmpo_losses(*[d[k] for k in KEYS], dual, True, 0.02, 0.1, 1e-3)["dual"]
        assert dual[0].item() == pytest.approx(eta.item(), rel=1e-12) and dual[1].item() == pytest.approx(alpha.item(), rel=1e-12)
        assert dual[6].item() == s + 1


def test_small_restatements():
    rs = np.random.RandomState(0)
    v = torch.tensor(rs.randn(9), requires_grad=True)
    R = torch.tensor(rs.randn(9))
    d_v, loss_sum = ref.mse_value(v.detach(), R, 18.0)
    g, = torch.autograd.grad(((v - R) ** 2).sum() / 18.0, v)
    close(d_v, g)
    assert loss_sum.item() == pytest.approx(((v - R) ** 2).sum().item(), rel=1e-14)
    allv = torch.tensor(rs.randn(10))
    close(ref.adv_normalize(allv[:5], allv, 1e-4), (allv[:5] - allv.mean()) / (allv.std(unbiased=True) + 1e-4))
    a, b, h = (torch.tensor(rs.randn(7)) for _ in range(3))
    x = torch.tensor(rs.randn(7), requires_grad=True)
    for act, fn in ((ref.ACT_TANH, torch.tanh), (ref.ACT_RELU, torch.relu)):
        y = fn(x)
        g, = torch.autograd.grad(y, x, a + b)                                  # act'(x) (a + b), through the OUTPUT y
        close(ref.jvp_gate(a, b, y.detach(), act), g)
    close(ref.jvp_gate(a, None, h, ref.ACT_NONE), a)
    close(ref.jvp_gate(a, b, None, ref.ACT_TANH), a + b)
    d_mu, ls = torch.tensor(rs.randn(5, 3)), torch.tensor([-25.0, 0.3, 3.0], dtype=torch.float64)
    close(ref.fisher_scale(d_mu, ls), d_mu / torch.exp(ls.clamp(-20, 2)) ** 2 / 5)


# ---------------------------------------------------------------- the conditions on the inputs
def test_trpo_inputs_move_the_weight():
    """(a) In every TRPO case of at least 48 samples, 20 % of the samples have 0.01 < w < 0.99 in float64 and 20 % have
    w > 0.99: the first group tells the kernel from one with w = 1, the second from one with w = 0, and no case compares
    zeros.  A case of ONE sample can only have one of the two; the two n = 1 cases have one each (their seeds, set by
    _vmpo_trpo_ref.trpo_case, were kept because they fall that way: whoever changes the seeds re-checks this)."""
    single = []
    for name, c, tanh in trpo_cases():
        w = trpo64(c, tanh)["w"]
        mid, hi = ((w > 0.01) & (w < 0.99)).double().mean().item(), (w > 0.99).double().mean().item()
        print("%s: 0.01 < w < 0.99 on %.0f %%, w > 0.99 on %.0f %%" % (name, 100 * mid, 100 * hi))
        if c["mean"].shape[0] == 1:
            single.append((mid, hi))
            continue
        assert mid >= 0.2 and hi >= 0.2, name
        # ... and a kernel with w = 1 misses the bound by a factor of ten on at least 20 % of d_mean
        with_eps, without = trpo64(c, tanh), trpo64(c, tanh, prob_eps=0.0)
        bound = 1e-4 / c["mean"].shape[0] + 1e-4 * with_eps["d_mean"].abs()
        moved = ((with_eps["d_mean"] - without["d_mean"]).abs() > 10 * bound).double().mean().item()
        print("    w = 1 would move %.0f %% of d_mean by more than ten bounds" % (100 * moved))
        assert moved >= 0.2, name
    assert sorted(single) == [(0.0, 1.0), (1.0, 0.0)]


def test_trpo_wide_case_covers_the_range_and_tells_w_from_one():
    (c, tanh), = [(c, t) for name, c, t in trpo_cases() if name == "wide"]
    with_eps, without = trpo64(c, tanh), trpo64(c, tanh, prob_eps=0.0)
    assert with_eps["lp"].min() < -29 and with_eps["lp"].max() > -9
    n = c["mean"].shape[0]
    diff = (with_eps["d_mean"] - without["d_mean"]).abs()
    assert (diff > 10 * (1e-4 / n + 1e-4 * with_eps["d_mean"].abs())).double().mean() >= 0.2


def test_vmpo_small_eta_inputs():
    """(b) at least 3 samples carry phi > 1e-3, and a float32 softmax without the maximum subtracted overflows."""
    for name, c, tanh, eta in vmpo_cases():
        if eta != ref.SMALL_ETA:
            continue
        phi = vmpo64(c, tanh, eta)["phi"]
        assert (phi > 1e-3).sum() >= 3, name
        assert c["adv"].max().item() / eta > 88.73                              # log of the largest float32
        assert torch.isinf(torch.exp(c["adv"] / np.float32(eta))).any()
    assert sum(eta == ref.SMALL_ETA for _, _, _, eta in vmpo_cases()) == 2


def test_gated_inputs_are_away_from_the_clamp_boundaries():
    """(c) no log_std of a gated case lies within 1e-3 of -20 or 2, and the gate closes exactly the intended entries."""
    gated = [c for name, c, *_ in vmpo_cases() + trpo_cases() if name == "gate"]
    assert len(gated) == 2
    for c in gated:
        for k in ("logstd", "tlogstd"):
            assert ((c[k] + 20).abs() > 1e-3).all() and ((c[k] - 2).abs() > 1e-3).all()
        assert [i for i in range(6) if not -20 <= c["logstd"][i] <= 2] == [1, 4]
    assert gated[0]["tlogstd"][2] == 3.0 and -20 <= gated[0]["logstd"][2] <= 2


# ---------------------------------------------------------------- float32 against float64 under the GPU test's bounds
def test_float32_restatement_stays_within_the_kernel_bounds():
    worst = 0.0
    for name, c, tanh, eta in vmpo_cases():
        want, got = vmpo64(c, tanh, eta), vmpo64(c, tanh, eta, torch.float32)
        nan = (2, 6) if c["mean"].shape[0] == 1 else ()
        r = list(ref.grad_ratios(got, want)) + ref.info_ratios(got["info"], want["info"], nan) + ref.dual_ratios(got["dual"], want["dual"], moments=eta != ref.SMALL_ETA)
        print("vmpo %s: worst err / bound %.4f" % (name, max(r)))
        assert max(r) <= 1.0, name
        worst = max(worst, max(r))
    for name, c, tanh in trpo_cases():
        for c_ent in (0.0, 0.01):
            want, got = trpo64(c, tanh, c_ent), trpo64(c, tanh, c_ent, torch.float32)
            r = list(ref.grad_ratios(got, want)) + ref.info_ratios(got["info"], want["info"], (2,) if c["mean"].shape[0] == 1 else ())
            print("trpo %s c_ent %g: worst err / bound %.4f" % (name, c_ent, max(r)))
            assert max(r) <= 1.0, name
            worst = max(worst, max(r))
    print("worst float32 err / bound over all cases %.4f" % worst)     # ~0.1: room for the kernels' fast exp / log
