"""The restatements of tests/_offpolicy_ref.py without a GPU.

1. Against torch on the CPU in float64: the autograd of nn.MSELoss and torch.min (twin-Q SAC, DDPG, TD3, DQN),
   torch.optim.Adam over three temperature steps, torch.std and friends, and the quantile-Huber loss and gradient of
   tests/golden/dqn.npz.
2. Every bound tests/test_offpolicy_kernels_gpu.py holds a kernel to, on the restatement alone: the float32 run of the
   same formulas against the float64 run, same inputs, same `*_ratios` function, err / bound <= 1.
3. What the inputs guarantee: no QR-DQN or epsilon-greedy sample whose float32 greedy action may differ from the float64
   one, d = 0 and |d| = 1 among the Huber arguments with terms on both sides of both, a tie q1n == q2n on every third
   row, well-conditioned logged moments."""
import numpy as np
import pytest
import torch

import _offpolicy_ref as R

F32, F64, U = R.F32, R.F64, R.U


def t64(a, grad=False):
    return None if a is None else torch.tensor(np.asarray(a, dtype=F64), requires_grad=grad)


# ------------------------------------------------------------------ 1. restatements against torch
def test_sac_gradients_equal_autograd_of_mse_and_min():
    c = {k: v.astype(F64) for k, v in R.sac_loss_case(37, "mixed").items()}
    alpha, gamma, B = 0.3, 0.97, 37
    ref = R.sac_losses_ref(*[c[k] for k in R.SAC_KEYS], alpha, gamma)
    Q1, Q2, Q1n, Q2n = (t64(c[k], True) for k in ("q1", "q2", "q1n", "q2n"))
    tv = torch.min(t64(c["tq1"]), t64(c["tq2"])) - alpha * t64(c["logp_next"])
    qt = t64(c["rew"]) + (1.0 - t64(c["term"])) * gamma * tv
    mse = torch.nn.MSELoss()
    losses = [mse(Q1, qt), mse(Q2, qt), (alpha * t64(c["logp"]) - torch.min(Q1n, Q2n)).mean()]
    torch.stack(losses).sum().backward()
    for key, leaf in (("dq1", Q1), ("dq2", Q2), ("dq1n", Q1n), ("dq2n", Q2n)):
        np.testing.assert_allclose(ref[key], leaf.grad.numpy(), rtol=1e-13, atol=1e-16, err_msg=key)
    assert np.all(ref["dq1n"][::3] * B == -0.5) and np.all(ref["dq2n"][::3] * B == -0.5)
    assert np.all((ref["dq1n"] + ref["dq2n"]) * B == -1.0)
    np.testing.assert_allclose(ref["sums"], [l.item() * B for l in losses] + [c["rew"].sum()], rtol=1e-13)


@pytest.mark.parametrize("twin", [True, False])
@pytest.mark.parametrize("with_qn", [True, False])
def test_detac_gradients_equal_autograd(twin, with_qn):
    c = {k: v.astype(F64) for k, v in R.detac_case(41).items()}
    gamma, B = 0.98, 41
    q2, tq2 = (c["q2"], c["tq2"]) if twin else (None, None)
    qn = c["qn"] if with_qn else None
    ref = R.detac_losses_ref(c["q1"], q2, c["tq1"], tq2, c["rew"], c["term"], qn, gamma)
    Q1, Q2, Qn = t64(c["q1"], True), t64(q2, True), t64(qn, True)
    tv = torch.min(t64(c["tq1"]), t64(tq2)) if twin else t64(c["tq1"])
    qt = t64(c["rew"]) + (1.0 - t64(c["term"])) * gamma * tv
    mse = torch.nn.MSELoss()
    losses = [mse(Q1, qt)] + ([mse(Q2, qt)] if twin else []) + ([-Qn.mean()] if with_qn else [])
    torch.stack(losses).sum().backward()
    np.testing.assert_allclose(ref["dq1"], Q1.grad.numpy(), rtol=1e-13, atol=1e-16)
    want = [losses[0].item() * B, 0.0, 0.0, c["rew"].sum()]
    if twin:
        np.testing.assert_allclose(ref["dq2"], Q2.grad.numpy(), rtol=1e-13, atol=1e-16)
        want[1] = losses[1].item() * B
    else:
        assert ref["dq2"] is None
    if with_qn:
        np.testing.assert_allclose(ref["dqn"], Qn.grad.numpy(), rtol=1e-13)
        want[2] = losses[-1].item() * B
    else:
        assert ref["dqn"] is None
    np.testing.assert_allclose(ref["sums"], want, rtol=1e-13)


def test_three_temperature_steps_equal_torch_adam():
    la = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([la], lr=3e-4)
    state = np.zeros(4)
    for call in range(3):
        logp = R.alpha_logp_case(257, call).astype(F64)
        opt.zero_grad()
        loss = -(la * (t64(logp) + (-6.0))).mean()
        loss.backward()
        opt.step()
        state, alpha, ref_loss = R.alpha_step_ref(state, logp, -6.0, 3e-4)
        np.testing.assert_allclose(ref_loss, loss.item(), rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(state[0], la.item(), rtol=1e-12)
        st = opt.state[la]
        np.testing.assert_allclose(state[1:3], [st["exp_avg"].item(), st["exp_avg_sq"].item()], rtol=1e-12)
        assert state[3] == call + 1 and alpha == np.exp(state[0])
    assert abs(state[0]) > 5e-4                                           # three steps of lr in one direction


@pytest.mark.parametrize("rows,ld,off,width", R.MOMENT_CASES)
@pytest.mark.parametrize("lo,hi", R.MOMENT_CLAMPS)
def test_moments_equal_torch(rows, ld, off, width, lo, hi):
    x = R.moments_case(rows, ld)
    t = torch.tensor(x.astype(F64)).reshape(rows, ld)[:, off:off + width].clamp(lo, hi)
    want = [t.mean().item(), t.std().item() if t.numel() > 1 else np.nan, t.max().item(), t.min().item()]
    ref = R.moments_ref(x, ld, off, width, lo, hi)
    np.testing.assert_allclose(ref, want, rtol=1e-13, equal_nan=True)
    assert R.moments_ratio(R.moments_ref(x, ld, off, width, lo, hi, order="waves"), ref) <= 1.0
    assert max(R.moments_conditioning(x, ld, off, width, lo, hi)) * R.moments_chain(rows, width) * 2.0 ** -53 <= R.MOMENT_RTOL
    if (lo, hi) == (-20.0, 2.0) and t.numel() > 100:
        assert ref[2] == 2.0 and (x.reshape(rows, ld)[:, off:off + width] > 2.0).any()     # the clamp is hit


def test_policy_moments_are_the_three_logged_tensors():
    c = R.samples_case(65, 6)
    logp = R.samples_ref(c["head"], c["eps1"], c["obs"], c["acts"])[1]
    mom = R.policy_moments_ref(c["head"], logp, 6)
    head = torch.tensor(c["head"].astype(F64))
    for row, t in zip(mom, (head[:, 6:].clamp(-20.0, 2.0), torch.tensor(logp), head[:, :6])):
        np.testing.assert_allclose(row, [t.mean().item(), t.std().item(), t.max().item(), t.min().item()], rtol=1e-13)
    one = R.policy_moments_ref(c["head"][:1, [0, 6]], logp[:1], 1)         # B = 1, A = 1: no std anywhere
    assert np.isnan(one[:, 1]).all() and not np.isnan(one[:, [0, 2, 3]]).any()


def test_quantile_huber_restatement_reproduces_the_golden_loss_and_gradient(golden):
    g = golden("dqn")
    src, tgt = g["qr_src"], g["qr_tgt"]
    B, Q = src.shape
    ref = R.quantile_huber_ref(src, np.zeros(B, dtype=np.int64), tgt, np.zeros(B), np.zeros(B), 1.0, 1, Q)
    assert abs(ref["sums"][0] / (B * Q * Q) - float(g["qr_loss"])) < 1e-6
    np.testing.assert_allclose(ref["dq"], g["qr_grad"], atol=2e-9, rtol=1e-5)


def test_quantile_huber_restatement_equals_autograd():
    B, A, Q = 5, 3, 7
    c = R.qr_case(B, A, Q, True)
    ref = R.quantile_huber_ref(c["q"], c["acts"], c["qn"], c["rew"], c["term"], R.QR_GAMMA, A, Q)
    q = t64(c["q"], True)
    at = torch.tensor(R.clamp_action(c["acts"], A))
    nxt = t64(c["qn"]).reshape(B, A, Q)
    astar = nxt.mean(2).max(1)[1]                                         # torch.max: the first maximum
    assert np.array_equal(astar.numpy(), ref["astar"])
    T = t64(c["rew"])[:, None] + R.QR_GAMMA * (1.0 - t64(c["term"]))[:, None] * nxt[torch.arange(B), astar]
    theta = q.reshape(B, A, Q)[torch.arange(B), at]
    diff = T[:, :, None] - theta[:, None, :]                              # (b, i, j)
    hub = torch.where(diff.abs() <= 1.0, 0.5 * diff ** 2, diff.abs() - 0.5)
    tau = (2.0 * torch.arange(Q, dtype=torch.float64) + 1.0) / (2.0 * Q)
    loss = (hub * (tau[None, None, :] - (diff.detach() < 0).double()).abs()).mean()
    loss.backward()
    np.testing.assert_allclose(ref["sums"][0] / (B * Q * Q), loss.item(), rtol=1e-13)
    np.testing.assert_allclose(ref["dq"], q.grad.numpy(), rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(ref["sums"][1:], [theta.sum().item(), c["rew"].astype(F64).sum()], rtol=1e-13)


def test_stored_action_rule():
    assert R.clamp_action(np.array([-1, 0, 5, 6, 11], dtype=np.int64), 6).tolist() == [0, 0, 5, 5, 5]
    assert R.clamp_action(np.array([np.nan, -0.5, 2.7, 6.0, 11.0, 5.99, np.inf, -np.inf], dtype=F32), 6).tolist() == \
        [0, 0, 2, 5, 5, 5, 5, 0]
    assert R.clamp_action(np.array([2.7, np.nan], dtype=F32), 1).tolist() == [0, 0]


def test_dqn_td_restatement_equals_autograd():
    B, A, gamma = 23, 6, 0.97
    c = R.dqn_case(B, A, True)
    ref = R.dqn_td_ref(c["q"], c["acts"], c["qn"], c["rew"], c["term"], gamma)
    assert ref["at"][:5].tolist() == [A - 1, 0, A - 1, 0, 2]
    q = t64(c["q"], True)
    qsa = q.gather(1, torch.tensor(ref["at"])[:, None])[:, 0]
    tgt = t64(c["rew"]) + gamma * (1.0 - t64(c["term"])) * t64(c["qn"]).max(1)[0]
    loss = torch.nn.MSELoss()(qsa, tgt)
    loss.backward()
    np.testing.assert_allclose(ref["dq"], q.grad.numpy(), rtol=1e-13, atol=1e-18)
    np.testing.assert_allclose(ref["sums"], [loss.item() * B, qsa.sum().item(), c["rew"].astype(F64).sum()], rtol=1e-13)


def test_eps_greedy_restatement():
    q = np.array([[1, 3, 3, 2], [4, 4, 4, 4], [0, 1, 2, 5]], dtype=F32)
    assert R.eps_greedy_ref(q, 4, 1).tolist() == [1, 0, 3]                 # the first maximum
    u, ra = np.array([0.1, 0.25, 0.3], dtype=F32), np.array([2, 2, 2])
    assert R.eps_greedy_ref(q, 4, 1, u, ra, 0.25).tolist() == [2, 0, 3]    # strict: u == epsilon keeps the greedy action
    assert R.eps_greedy_ref(q, 2, 2).tolist() == [1, 0, 1]                 # means over pairs: (2, 2.5), (4, 4), (.5, 3.5)
    t = torch.tensor(q.astype(F64)).reshape(3, 2, 2).mean(2)
    assert R.eps_greedy_ref(q, 2, 2).tolist() == t.max(1)[1].tolist()


def test_noise_and_polyak_restatements_equal_torch():
    a, eps = R.stream_case(257)
    for sigma, clip, lo, hi in R.NOISE_ARGS:
        want = (t64(a) + (sigma * t64(eps)).clamp(-clip, clip)).clamp(lo, hi)
        assert np.array_equal(R.noisy_action_ref(a, eps, sigma, clip, lo, hi), want.numpy())
    for tau in R.POLYAK_TAU:
        tf = float(F32(tau))
        np.testing.assert_allclose(R.polyak_ref(a, eps, tau), a.astype(F64) * (1 - tf) + eps.astype(F64) * tf, rtol=1e-15)


# ------------------------------------------------------------------ 2. the float32 run within every bound of the GPU file
def worst(ratios):
    assert max(ratios.values()) <= 1.0, ratios
    return max(ratios.values())


@pytest.mark.parametrize("B", R.SAC_B)
def test_float32_sac_losses_within_the_bounds(B):
    for mode in R.TERM_MODES:
        c = R.sac_loss_case(B, mode)
        args = [c[k] for k in R.SAC_KEYS]
        for alpha in (0.37, float(R.alpha_step_ref(R.ALPHA_STATE0, c["logp"], *R.ALPHA_ARGS, dt=F32)[1])):
            a32, g32 = float(F32(alpha)), float(F32(0.99))
            worst(R.sac_ratios(R.sac_losses_ref(*args, a32, g32, dt=F32), R.sac_losses_ref(*args, a32, g32), B))


@pytest.mark.parametrize("B", R.SAC_EXACT_B)
def test_float32_is_exact_on_the_exact_sac_case(B):
    c = R.sac_exact_case(B)
    args = [c[k] for k in R.SAC_KEYS]
    lo, hi = R.sac_losses_ref(*args, 0.25, 0.5, dt=F32), R.sac_losses_ref(*args, 0.25, 0.5)
    for key in ("dq1", "dq2", "dq1n", "dq2n", "sums"):
        assert np.array_equal(lo[key].astype(F64), hi[key]), key


@pytest.mark.parametrize("k,B", list(enumerate(R.ALPHA_B)))
def test_float32_temperature_steps_within_the_bounds(k, B):
    s32 = s64 = np.array((R.ALPHA_LA0[k],) + R.ALPHA_STATE0[1:])
    for call in range(3):
        logp = R.alpha_logp_case(B, call)
        s32, alpha, loss = R.alpha_step_ref(s32, logp, *R.ALPHA_ARGS, dt=F32)
        s64, _, loss64 = R.alpha_step_ref(s64, logp, *R.ALPHA_ARGS)
        worst(R.alpha_ratios(s32, alpha, loss, s64, loss64))
        assert abs(s64[0]) <= 3.0


@pytest.mark.parametrize("A", R.FOLD_A)
@pytest.mark.parametrize("B", R.SAC_B)
def test_fold_inputs_are_well_conditioned(B, A):
    """The logged moments of the fold cases: summed per wave of 64 rows as the kernels do, within rel 1e-12 of the plain
    float64 value, and no mean or variance amplifies the sums' error beyond rel 1e-12."""
    c = R.samples_case(B, A)
    logp = R.samples_ref(c["head"], c["eps1"], c["obs"], c["acts"])[1]
    ref = R.policy_moments_ref(c["head"], logp, A)
    assert R.moments_ratio(R.policy_moments_ref(c["head"], logp, A, order="waves"), ref) <= 1.0
    assert np.isnan(ref[1, 1]) == (B == 1) and np.isnan(ref[0, 1]) == (B == 1 and A == 1)
    if B * A > 1:
        amp = [R.moments_conditioning(c["head"], 2 * A, A, A, -20.0, 2.0), R.moments_conditioning(c["head"], 2 * A, 0, A)]
        amp.append(R.moments_conditioning(logp, 1, 0, 1) if B > 1 else (1.0, 1.0))
        assert np.max(amp) * R.moments_chain(B, A) * 2.0 ** -53 <= R.MOMENT_RTOL, amp


@pytest.mark.parametrize("B", R.DETAC_B)
def test_float32_detac_losses_within_the_bounds(B):
    c = R.detac_case(B)
    g32 = float(F32(0.99))
    for twin in (True, False):
        for with_qn in (True, False):
            args = [c["q1"], c["q2"] if twin else None, c["tq1"], c["tq2"] if twin else None, c["rew"], c["term"],
                    c["qn"] if with_qn else None, g32]
            worst(R.detac_ratios(R.detac_losses_ref(*args, dt=F32), R.detac_losses_ref(*args), B))
    for Bx in R.DETAC_EXACT_B:
        cx = R.detac_exact_case(Bx)
        args = [cx[k] for k in ("q1", "q2", "tq1", "tq2", "rew", "term", "qn")] + [0.5]
        lo, hi = R.detac_losses_ref(*args, dt=F32), R.detac_losses_ref(*args)
        for key in ("dq1", "dq2", "dqn", "sums"):
            assert np.array_equal(lo[key].astype(F64), hi[key]), key


@pytest.mark.parametrize("n", R.STREAM_N)
def test_float32_noise_and_polyak_within_the_bounds(n):
    a, eps = R.stream_case(n)
    for sigma, clip, lo, hi in R.NOISE_ARGS:
        lo32 = R.noisy_action_ref(a, eps, sigma, clip, lo, hi, dt=F32)
        assert lo32.dtype == F32
        want = R.noisy_action_ref(a, eps, float(F32(sigma)), float(F32(clip)), lo, hi)
        assert np.all(np.abs(lo32 - want) <= 2 * U * (np.abs(a) + np.abs(eps)))
        if sigma == 0.0:
            assert np.array_equal(lo32, np.clip(a, F32(lo), F32(hi)))
    for tau in R.POLYAK_TAU:
        got = R.polyak_ref(a, eps, tau, dt=F32)
        assert R.polyak_ratio(got, a, eps, tau) <= 1.0
        assert tau != 1.0 or np.array_equal(got, eps)
        assert tau != 0.0 or np.array_equal(got.view(np.uint32), a.view(np.uint32))


@pytest.mark.parametrize("float_acts", [False, True])
@pytest.mark.parametrize("A", R.DQN_A)
@pytest.mark.parametrize("B", R.DQN_B)
def test_float32_dqn_td_within_the_bounds(B, A, float_acts):
    c = R.dqn_case(B, A, float_acts)
    args = [c[k] for k in ("q", "acts", "qn", "rew", "term")] + [float(F32(0.99))]
    ref = R.dqn_td_ref(*args)
    worst(R.dqn_ratios(R.dqn_td_ref(*args, dt=F32), ref, B))
    planted = [A - 1, 0, A - 1] + ([0, min(2, A - 1)] if float_acts else [])
    assert ref["at"][:len(planted)].tolist() == planted[:B]
    assert 0 < c["term"].sum() < B or B == 1


@pytest.mark.parametrize("float_acts", [False, True])
@pytest.mark.parametrize("B,A,Q", R.QR_CASES)
def test_float32_quantile_huber_within_the_bounds_and_input_guarantees(B, A, Q, float_acts):
    c = R.qr_case(B, A, Q, float_acts)
    args = [c[k] for k in ("q", "acts", "qn", "rew", "term")] + [R.QR_GAMMA, A, Q]
    ref = R.quantile_huber_ref(*args)
    worst(R.qr_ratios(R.quantile_huber_ref(*args, dt=F32), ref, B, A, Q))
    # greedy next action: no sample excluded, and the planted ties are ties at the top
    assert R.excluded_samples(c["qn"], A, Q) == 0
    gap = R.greedy_means(c["qn"], A, Q)[2]
    if A >= 2:
        assert np.all(gap[np.arange(B) % 3 != 2] == 0.0)
        want_first = np.where((np.arange(B) % 2 == 1) & (A >= 3), 1, 0)
        assert np.array_equal(ref["astar"][np.arange(B) % 3 != 2], want_first[np.arange(B) % 3 != 2])
    # the targets are exact in fp32, and so are the planted differences
    T32 = c["rew"][:, None] + (F32(R.QR_GAMMA) * (F32(1) - c["term"]))[:, None] * c["qn"].reshape(B, A, Q)[np.arange(B), ref["astar"]]
    assert T32.dtype == F32 and np.array_equal(T32.astype(F64), ref["T"])
    d = ref["T"][:, :, None] - ref["th"][:, None, :]
    if Q >= 3:
        assert np.all(d[:, 0, 0] == 0.0) and np.all(d[:, 0, 1] == -1.0) and np.all(d[:, 1, 2] == 1.0)
        ad = np.abs(d)
        assert (d < 0).any() and (d > 0).any() and ((ad > 0) & (ad < 1)).any() and (ad > 1).any()
    else:
        assert np.all(np.abs(d) == 1.0)                                   # (1, 1, 1): the one term there is
    assert (c["term"] == 1).sum() == len(range(1, B, 3))


@pytest.mark.parametrize("N,A,Q", R.EPS_CASES)
def test_eps_greedy_inputs_exclude_no_sample(N, A, Q):
    c = R.eps_case(N, A, Q)
    assert R.excluded_samples(c["q"], A, Q) == 0
    means, _, gap = R.greedy_means(c["q"], A, Q)
    if A >= 2:
        assert np.all(gap[::2] == 0.0)                                    # planted: the first of two equal rows wins
        assert np.array_equal(means.argmax(1)[::2], np.where((np.arange(0, N, 2) % 4 == 2) & (A >= 3), 1, 0))
    # a float32 mean summed in the kernel's order (lane-strided partial sums) picks the same action
    x = c["q"].reshape(N, A, Q)
    part = np.zeros((N, A, 64), dtype=F32)
    for i in range(Q):
        part[:, :, i % 64] += x[:, :, i]
    m32 = part.sum(2, dtype=F32) / F32(Q)
    assert np.array_equal(m32.argmax(1), R.eps_greedy_ref(c["q"], A, Q))
    got = R.eps_greedy_ref(c["q"], A, Q, c["u"], c["rand_act"], R.EPSILON)
    assert np.array_equal(got[::3], R.eps_greedy_ref(c["q"], A, Q)[::3])  # u == epsilon: greedy
    below = c["u"] < F32(R.EPSILON)
    assert np.array_equal(got[below], c["rand_act"][below]) and (N < 200 or (below.sum() > 10 and (~below).sum() > 10))


def test_twin_ties_sit_on_every_third_row():
    for B in R.SAC_B:
        c = R.sac_loss_case(B, "mixed")
        assert np.all(c["q1n"][::3] == c["q2n"][::3]) and np.all(c["tq1"][::3] == c["tq2"][::3])
        rest = np.ones(B, dtype=bool)
        rest[::3] = False
        assert np.all(c["q1n"][rest] != c["q2n"][rest])
        if B >= 64:
            assert 0 < c["term"].sum() < B


@pytest.mark.parametrize("B,A,tanh", R.RSAMPLE_CASES)
def test_sampler_cases_keep_four_fifths_of_their_rows_unsaturated(B, A, tanh):
    head, eps, _ = R.rsample_case(B, A)
    a = R.rsample(torch.tensor(head), torch.tensor(eps), tanh)[0]
    ok = (a.abs().max(dim=1).values < 0.999).numpy() if tanh else np.ones(B, dtype=bool)
    assert ok.mean() > 0.8
    raw = head[:, A:]
    assert (raw < -20.0).sum() == 1 and (raw > 2.0).sum() == (1 if B > 1 else 0)


def test_argument_checks_launch_nothing():
    """Empty batches, NULL pointers and both or neither of acts / acts_f come back as a negative code with a message
    before anything is launched (the pointers passed here are not device memory)."""
    from torchrl_amd import _C
    lib = _C.lib()
    p = 4096
    err = lambda: lib.trl_last_error().decode()
    for acts, acts_f in ((p, p), (None, None)):
        assert lib.trl_dqn_td_loss_f32(p, acts, acts_f, p, p, p, 0.99, 8, 6, p, p, None, 0, None, None) < 0
        assert "exactly one of acts" in err()
        assert lib.trl_quantile_huber_f32(p, acts, acts_f, p, p, p, 0.99, 8, 6, 5, p, p, p, None, 0, None, None) < 0
        assert "exactly one of acts" in err()
    assert lib.trl_dqn_td_loss_f32(p, p, None, p, p, p, 0.99, 0, 6, p, p, None, 0, None, None) < 0 and "bad sizes" in err()
    assert lib.trl_dqn_td_loss_f32(None, p, None, p, p, p, 0.99, 8, 6, p, p, None, 0, None, None) < 0 and "null pointer" in err()
    assert lib.trl_dqn_td_loss_f32(p, p, None, p, p, p, 0.99, 8, 6, p, p, p, 0, p, None) < 0 and "ring without slots" in err()
    assert lib.trl_quantile_huber_f32(p, p, None, p, p, p, 0.99, 0, 6, 5, p, p, p, None, 0, None, None) < 0 and "bad sizes" in err()
    assert lib.trl_quantile_huber_f32(p, p, None, p, p, p, 0.99, 8, 6, 5, p, None, p, None, 0, None, None) < 0 and "null pointer" in err()
    assert lib.trl_sac_losses_f32(*[p] * 11, 0.99, 0, p, p, p, p, p, None, None, 0.0, 0.0, 0.9, 0.999, 1e-8, None, 0, None, None) < 0
    assert "empty batch" in err()
    assert lib.trl_sac_losses_f32(None, *[p] * 10, 0.99, 8, p, p, p, p, p, None, None, 0.0, 0.0, 0.9, 0.999, 1e-8, None, 0, None, None) < 0
    assert "null input" in err()
    assert lib.trl_sac_losses_f32(*[p] * 10, None, 0.99, 8, p, p, p, p, p, None, None, 0.0, 0.0, 0.9, 0.999, 1e-8, None, 0, None, None) < 0
    assert "alpha" in err()
    assert lib.trl_sac_alpha_step_f32(p, 0, -6.0, 3e-4, 0.9, 0.999, 1e-8, p, p, None) < 0 and "empty batch" in err()
    assert lib.trl_detac_losses_f32(p, None, p, None, p, p, None, 0.99, 0, p, None, None, p, None) < 0 and "empty batch" in err()
    assert lib.trl_detac_losses_f32(p, p, p, p, p, p, None, 0.99, 8, p, None, None, p, None) < 0 and "come in pairs" in err()
    assert lib.trl_detac_losses_f32(None, None, p, None, p, p, None, 0.99, 8, p, None, None, p, None) < 0 and "null pointer" in err()
    assert lib.trl_eps_greedy_i64(None, 8, 6, 1, None, None, 0.1, p, None, 0, None) < 0 and "null pointer" in err()
    assert lib.trl_eps_greedy_i64(p, 8, 6, 1, None, None, 0.1, p, p, 0, None) < 0 and "bad sizes" in err()
    assert lib.trl_polyak_f32(None, p, 8, 0.005, None) < 0 and "null pointer" in err()
    assert lib.trl_noisy_action_f32(p, None, 0.1, 1.0, -1.0, 1.0, p, 8, None) < 0 and "null pointer" in err()
