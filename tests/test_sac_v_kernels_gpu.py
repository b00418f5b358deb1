"""The two kernels of the value-network soft actor-critics (torchrl_amd/csrc/k_sac.hip: trl_sacv_samples_f32,
trl_sacv_losses_f32), called directly and compared with the float64 restatement (tests/_sac_v_ref.py) on identical
float32 inputs.

Losses: B in {1, 64, 65, 1023, 1025, 4096} -- the wave and block-stride boundaries of a one-workgroup kernel of 1024
threads that takes four rows per thread --, one and two critics, terminals all 0 / all 1 / mixed, planted exact ties
q1n == q2n, alpha read from the device, n = B and 2 B, the two riders on and off.  With u = 2^-24 the bounds count
roundings (six at most per output, contraction only removes some):
    |d dq| <= 8 u (|q| + |r| + gamma |tv|) 2 / n          |d dv| <= 8 u (|v| + |qn| + alpha |logp|) 2 / n
    dq_n n is exactly -1, -0.5 or 0
    each loss sum within sum_b(2 |diff_b| delta_b + delta_b^2 + 2 u diff_b^2), delta_b the bound above without its 2 / n
    the policy and reward sums within 4 u sum|terms|
and where every input is a multiple of 1/8 every fp32 operation is exact, so outputs and sums equal the restatement.
Every comparison prints its worst err / bound as a RATIO line (profiles/NOTES_sac_v.md has them from one run)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _sac_v_ref as R                                                        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = R.U
LOSS_B = (1, 64, 65, 1023, 1025, 4096, 4097, 8200)
KEYS = ("q1", "q2", "tv", "rew", "term", "v", "q1n", "q2n", "logp")


def loss_inputs(B, twin, term_mode, seed):
    """float32 CPU tensors; every third row an exact tie q1n == q2n."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(B, generator=gen)
    c = dict(q1=r() * 2, q2=r() * 2, tv=r() * 3, rew=r(), v=r() * 2, q1n=r() * 2, q2n=r() * 2, logp=r() * 3 - 4)
    c["term"] = {"zeros": torch.zeros(B), "ones": torch.ones(B),
                 "mixed": (torch.rand(B, generator=gen) < 0.3).float()}[term_mode]
    c["q2n"][::3] = c["q1n"][::3]
    if not twin:
        c["q2"] = c["q2n"] = None
    return c


def on_dev(c):
    return [None if c[k] is None else c[k].to(DEV) for k in KEYS]


def run_losses(c, alpha, gamma, n=None, **riders):
    from torchrl_amd import _C
    sums = torch.full((5,), 7.0, dtype=torch.float64, device=DEV)
    alpha_t = None if alpha is None else torch.tensor([alpha], dtype=torch.float32, device=DEV)
    outs = _C.sacv_losses(*on_dev(c), alpha_t, gamma, sums, n=n, **riders)
    torch.cuda.synchronize()
    got = dict(zip(("dq1", "dq2", "dv", "dq1n", "dq2n"), [None if o is None else o.cpu().numpy().reshape(-1) for o in outs]))
    got["sums"] = sums.cpu().numpy()
    return got


def restate(c, alpha, gamma, n):
    return R.losses_ref(*[None if c[k] is None else c[k].numpy() for k in KEYS], float(np.float32(alpha)),
                        float(np.float32(gamma)), n)


def ratios(got, ref, n, twin):
    """{name: worst err / bound}; the exact properties are asserted on the spot."""
    out = {}
    crit = [("dq1", "e1", 0)] + ([("dq2", "e2", 1)] if twin else [])
    for key, diff, i in crit:
        delta = 8 * U * ref["mag_q"][i]
        out[key] = float(np.max(np.abs(got[key].astype(np.float64) - ref[key]) / (delta * 2 / n)))
        bound = np.sum(2 * np.abs(ref[diff]) * delta + delta ** 2 + 2 * U * ref[diff] ** 2)
        out["sum_" + key] = float(abs(got["sums"][i] - ref["sums"][i]) / bound)
    delta = 8 * U * ref["mag_v"]
    out["dv"] = float(np.max(np.abs(got["dv"].astype(np.float64) - ref["dv"]) / (delta * 2 / n)))
    out["sum_dv"] = float(abs(got["sums"][2] - ref["sums"][2]) / np.sum(2 * np.abs(ref["ev"]) * delta + delta ** 2
                                                                         + 2 * U * ref["ev"] ** 2))
    pol_terms = np.abs(ref["pol"] + ref["qn"]) + np.abs(ref["qn"])               # |alpha logp| + |qn|
    out["sum_pol"] = float(abs(got["sums"][3] - ref["sums"][3]) / (4 * U * pol_terms.sum()))
    out["sum_rew"] = float(abs(got["sums"][4] - ref["sums"][4]) / (4 * U * ref["sum_abs_rew"]))
    # dq_n n is exactly -1, -0.5 or 0 (fp32 product), and the weights are the restatement's
    nf = np.float32(n)
    for key in ("dq1n", "dq2n") if twin else ("dq1n",):
        assert np.array_equal(got[key] * nf, (ref[key] * n).astype(np.float32)), key
        assert set(np.unique(got[key] * nf)) <= {-1.0, -0.5, 0.0}
    if not twin:
        assert got["dq2"] is None and got["dq2n"] is None and got["sums"][1] == 0.0
    return out


@pytest.mark.parametrize("twin", [True, False], ids=["twin", "single"])
@pytest.mark.parametrize("B", LOSS_B)
def test_losses_against_the_restatement(B, twin):
    worst = {}
    for term_mode in ("zeros", "ones", "mixed"):
        c = loss_inputs(B, twin, term_mode, seed=B + 7)
        for n in (B, 2 * B):
            got = run_losses(c, 0.37, 0.99, n=n)
            ref = restate(c, 0.37, 0.99, n)
            if twin and B >= 3:
                assert np.all(got["dq1n"][::3] * np.float32(n) == -0.5) and np.all(got["dq2n"][::3] * np.float32(n) == -0.5)
            for k, r in ratios(got, ref, n, twin).items():
                worst[k] = max(worst.get(k, 0.0), r)
    print("RATIO sacv_losses B=%d %s: %s" % (B, "twin" if twin else "single",
                                              " ".join("%s %.4f" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("twin", [True, False], ids=["twin", "single"])
@pytest.mark.parametrize("B", [64, 1024])
def test_losses_are_exact_where_fp32_is(B, twin):
    """Inputs that are multiples of 1/8 with |x| <= 4, gamma = 0.5, alpha = 0.25, n = B a power of two: no fp32 operation
    of the kernel rounds, so every output and all five sums equal the float64 restatement."""
    gen = torch.Generator().manual_seed(B)
    r = lambda: torch.randint(-32, 33, (B,), generator=gen).float() / 8
    c = dict(q1=r(), q2=r(), tv=r(), rew=r(), v=r(), q1n=r(), q2n=r(), logp=r(),
             term=torch.randint(0, 2, (B,), generator=gen).float())
    c["q2n"][::4] = c["q1n"][::4]
    if not twin:
        c["q2"] = c["q2n"] = None
    got, ref = run_losses(c, 0.25, 0.5), restate(c, 0.25, 0.5, B)
    for key in ("dq1", "dq2", "dv", "dq1n", "dq2n"):
        if ref[key] is None:
            assert got[key] is None
        else:
            assert np.array_equal(got[key].astype(np.float64), ref[key]), key
    assert np.array_equal(got["sums"], ref["sums"])
    print("RATIO sacv_losses exact B=%d %s: 0.0000" % (B, "twin" if twin else "single"))


@pytest.mark.parametrize("twin", [True, False], ids=["twin", "single"])
@pytest.mark.parametrize("B", LOSS_B)
def test_riders_equal_the_separate_launches(B, twin):
    """Temperature step and moment fold inside the loss launch against trl_sac_alpha_step_f32 and trl_moments_multi_f64
    as launches of their own on the same inputs: the temperature state, alpha and with them every output and loss sum
    bit for bit; the moments are summed in another order (per-wave partials), so to 1e-11."""
    from torchrl_amd import _C
    A, D = 6, 5
    gen = torch.Generator().manual_seed(3 * B + 1)
    r = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    head, eps, obs, acts = r(B, 2 * A), r(B, A), r(B, D), r(B, A)
    head[:, A:] *= 8.0
    mom_part = torch.zeros((B + 63) // 64, 12, dtype=torch.float64, device=DEV)
    _, logp, _, _ = _C.sacv_samples(head, eps, obs, acts, mom_part=mom_part)
    c = loss_inputs(B, twin, "mixed", seed=B)
    c["logp"] = logp.cpu()
    state0 = torch.tensor([0.1, 0.02, 0.003, 5.0], device=DEV)
    # separate launches
    state_a, out_a = state0.clone(), torch.zeros(2, device=DEV)
    _C.sac_alpha_step(logp, -6.0, 3e-4, state_a, out_a)
    mom_a = torch.zeros(3, 4, dtype=torch.float64, device=DEV)
    inf = float("inf")
    _C.moments_multi([(head, mom_a[0], 2 * A, A, A, -20.0, 2.0), (logp, mom_a[1], 1, 0, 1, -inf, inf),
                      (head, mom_a[2], 2 * A, 0, A, -inf, inf)])
    sums_a = torch.zeros(5, dtype=torch.float64, device=DEV)
    outs_a = _C.sacv_losses(*on_dev(c), out_a[0:1], 0.99, sums_a)
    # riding along
    state_b, out_b = state0.clone(), torch.zeros(2, device=DEV)
    mom_b = torch.zeros(3, 4, dtype=torch.float64, device=DEV)
    sums_b = torch.zeros(5, dtype=torch.float64, device=DEV)
    outs_b = _C.sacv_losses(*on_dev(c), None, 0.99, sums_b, alpha_step=(-6.0, 3e-4, state_b, out_b),
                            fold=(mom_part, A, mom_b))
    assert torch.equal(state_a, state_b) and torch.equal(out_a, out_b) and torch.equal(sums_a, sums_b)
    assert float(state_b[3]) == 6.0 and float(out_b[0]) != 0.0
    for x, y in zip(outs_a, outs_b):
        assert (x is None and y is None) or torch.equal(x, y)
    ma, mb = mom_a.cpu().numpy(), mom_b.cpu().numpy()                   # (B = 1: the std of one log_prob is NaN in all three)
    np.testing.assert_allclose(mb, ma, rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(mb, R.moments_ref(head.cpu().numpy(), logp.cpu().numpy(), A), rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("B,D,A", [(777, 17, 6), (64, 2, 1), (130, 32, 8), (4096, 23, 3), (65, 11, 3), (200, 33, 2)])
def test_sampling_launch_equals_the_separate_kernels(B, D, A):
    """trl_sacv_samples_f32 against rsample_fwd / concat2 / philox_normal bit for bit in both noise modes, its per-wave
    partial moments against float64 sums, and its numbers against the restatement."""
    from torchrl_amd import _C
    gen = torch.Generator().manual_seed(B + D)
    r = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    head, eps, obs, acts = r(B, 2 * A), r(B, A), r(B, D), r(B, A)
    head[:, A:] *= 8.0                                                    # some log_std outside [-20, 2]
    parts = (B + 63) // 64
    mom = torch.zeros(parts, 12, dtype=torch.float64, device=DEV)
    eps_in = eps.clone()
    new_a, logp, x_sa, x_new = _C.sacv_samples(head, eps, obs, acts, mom_part=mom)
    a1, l1 = _C.rsample_fwd(head, eps)
    assert torch.equal(eps, eps_in)                                       # read, not written
    assert torch.equal(new_a, a1) and torch.equal(logp, l1)
    assert torch.equal(x_sa, _C.concat2(obs, acts)) and torch.equal(x_new, _C.concat2(obs, a1))
    ls, mu, lp = head[:, A:].clamp(-20.0, 2.0).double(), head[:, :A].double(), l1.double().reshape(-1, 1)
    for p in range(parts):
        sl = slice(64 * p, min(B, 64 * p + 64))
        for j, t in enumerate((ls[sl], lp[sl], mu[sl])):
            want = torch.stack([t.sum(), (t * t).sum(), t.max(), (-t).max()])
            assert torch.allclose(mom[p, 4 * j:4 * j + 4], want, rtol=1e-12, atol=1e-12), (p, j)
    # ... and the numbers against the restatement, on a head with log_std around -1.  The reference's log-density takes
    # z - mean back out of z = mean + sd eps and the tanh correction takes log(1 - a^2 + 1e-6): both lose digits where sd is
    # small or |a| near 1, so a row's bound is made of these amplifications (8 u on each rounded quantity; tanh here is
    # 1 - 2 / (e^2z + 1), absolute error a few u)
    head_t = r(B, 2 * A)
    head_t[:, A:] = head_t[:, A:] * 0.5 - 1.0
    act_t, logp_t, _, _ = _C.sacv_samples(head_t, eps, obs, acts)
    hn, en = head_t.cpu().numpy().astype(np.float64), eps.cpu().numpy().astype(np.float64)
    ra, rl, _, _ = R.samples_ref(hn, en, obs.cpu().numpy(), acts.cpu().numpy())
    np.testing.assert_allclose(act_t.cpu().numpy(), ra, rtol=0, atol=8 * U)
    mean, ls = hn[:, :A], np.clip(hn[:, A:], -20.0, 2.0)
    sd = np.exp(ls)
    z, one_a2 = mean + sd * en, 1.0 - ra * ra + 1e-6
    bound = (8 * U * np.abs(en) * (np.abs(mean) + np.abs(z)) / sd + 8 * U * 2 * np.abs(ra) / one_a2
             + 8 * U * (0.5 * en * en + np.abs(ls) + 1.0 + np.abs(np.log(one_a2)))).sum(1)
    err = np.abs(logp_t.cpu().numpy().astype(np.float64) - rl)
    tame = bound < 1e-3                                                   # the rows where the comparison means something
    assert tame.sum() >= B // 2 and np.all(err[tame] <= bound[tame]), (tame.sum(), err[tame] / bound[tame])
    print("RATIO sacv_samples B=%d D=%d A=%d: logp %.4f over %d of %d rows" % (B, D, A, (err[tame] / bound[tame]).max(),
                                                                                tame.sum(), B))
    # device noise: update u draws (seed, u + 1) and leaves it in eps
    state = torch.tensor([3.0, 1.0, 1.0, 0.0], dtype=torch.float64, device=DEV)
    e1 = torch.zeros(B, A, device=DEV)
    outs = _C.sacv_samples(head, e1, obs, acts, philox=(state, 77))
    w1 = _C.philox_normal(torch.empty(B, A, device=DEV), 77, 4)
    assert torch.equal(e1, w1) and state.cpu().tolist() == [3.0, 1.0, 1.0, 0.0]
    b1, m1 = _C.rsample_fwd(head, w1)
    assert torch.equal(outs[0], b1) and torch.equal(outs[1], m1)
    assert torch.equal(outs[2], _C.concat2(obs, acts)) and torch.equal(outs[3], _C.concat2(obs, b1))
    # twice: equal bits
    again = _C.sacv_samples(head, eps, obs, acts, mom_part=torch.zeros_like(mom))
    assert all(torch.equal(x, y) for x, y in zip(again, (new_a, logp, x_sa, x_new)))


def test_two_runs_of_the_loss_launch_give_equal_bits():
    c = loss_inputs(4096, True, "mixed", seed=1)
    a, b = run_losses(c, 0.37, 0.99), run_losses(c, 0.37, 0.99)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_argument_errors_raise():
    from torchrl_amd import _C
    c = loss_inputs(8, True, "mixed", seed=2)
    sums = torch.zeros(5, dtype=torch.float64, device=DEV)
    alpha = torch.ones(1, device=DEV)
    args = on_dev(c)
    with pytest.raises(_C.TrlError, match="q2 and q2n come together"):
        _C.sacv_losses(*args[:7], None, args[8], alpha, 0.99, sums)
    with pytest.raises(_C.TrlError, match="empty batch"):
        _C.sacv_losses(*[None if t is None else t[:0] for t in args], alpha, 0.99, sums)
    with pytest.raises(_C.TrlError, match="global batch"):
        _C.sacv_losses(*args, alpha, 0.99, sums, n=4)
    with pytest.raises(_C.TrlError, match="alpha is None"):
        _C.sacv_losses(*args, None, 0.99, sums)
    with pytest.raises(_C.TrlError, match="in0 is None"):
        _C.sacv_losses(None, *args[1:], alpha, 0.99, sums)
    with pytest.raises(_C.TrlError, match="no CPU path"):
        _C.sacv_losses(args[0].cpu(), *args[1:], alpha, 0.99, sums)
    head, eps, obs, acts = (torch.zeros(8, w, device=DEV) for w in (18, 9, 4, 9))
    with pytest.raises(_C.TrlError, match="A <= 8"):
        _C.sacv_samples(head, eps, obs, acts)
    with pytest.raises(_C.TrlError, match="mom_part holds fewer"):
        _C.sacv_samples(head[:, :4], eps[:, :2], obs, acts[:, :2], mom_part=torch.zeros(0, 12, dtype=torch.float64, device=DEV))
    assert float(sums.abs().sum()) == 0.0                               # nothing was launched
