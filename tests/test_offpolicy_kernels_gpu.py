"""The older off-policy kernels (torchrl_amd/csrc/k_sac.hip, k_dqn.hip) behind twin-Q SAC, DDPG, TD3, DQN and QR-DQN,
called directly through their `_C` wrappers and compared with the float64 restatements of tests/_offpolicy_ref.py on
identical float32 inputs.  The inputs, the bounds (`*_ratios`: worst err / bound) and the exact properties are those of
that module; tests/test_offpolicy_kernels_cpu.py holds the float32 run of the restatements to the same bounds and
asserts what the inputs guarantee.  With U = 2^-24:
    |d dq| <= 8 U mag 2 / B (mag: the magnitudes that enter the TD error)      dq_n B is exactly -1, -0.5 or 0
    a loss sum within sum_b(2 |e_b| delta_b + delta_b^2 + 2 U e_b^2), delta = 8 U mag; other sums within 4 U sum |terms|
    logged moments: mean and std rel 1e-12 (sums in double over exactly converted floats), max / min exact
    quantile Huber: a column of Q terms accumulated in fp32, (Q + 8) U sum |terms|
and where every input is a multiple of 1/8 no fp32 operation rounds, so outputs and sums equal the restatement.
Every comparison prints its worst err / bound as a RATIO line (profiles/NOTES_offpolicy_kernel_tests.md has one run)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _offpolicy_ref as R                                                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U, F32, F64 = R.U, R.F32, R.F64
INF = float("inf")
G32 = float(F32(0.99))                                                        # the discount the kernels are handed


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def report(name, ratios):
    print("RATIO %s: %s" % (name, " ".join("%s %.4f" % kv for kv in sorted(ratios.items()))))
    assert max(ratios.values()) <= 1.0, ratios


def merge(worst, ratios):
    for k, r in ratios.items():
        worst[k] = max(worst.get(k, 0.0), r)


def f64(n, fill=7.0):
    return torch.full((n,), fill, dtype=torch.float64, device=DEV)


# ------------------------------------------------------------------ trl_sac_losses_f32
def run_sac(c, alpha, gamma, **riders):
    from torchrl_amd import _C
    sums = f64(4)
    alpha_t = None if alpha is None else torch.tensor([alpha], dtype=torch.float32, device=DEV)
    outs = _C.sac_losses(*[dev(c[k]) for k in R.SAC_KEYS], alpha_t, gamma, sums, **riders)
    torch.cuda.synchronize()
    got = dict(zip(("dq1", "dq2", "dq1n", "dq2n"), [host(o).reshape(-1) for o in outs]))
    got["sums"] = host(sums)
    return got


def sac_ref(c, alpha, gamma):
    return R.sac_losses_ref(*[c[k] for k in R.SAC_KEYS], float(F32(alpha)), float(F32(gamma)))


@pytest.mark.parametrize("B", R.SAC_B)
def test_sac_losses_against_the_restatement(B):
    """Terminals all 0 / all 1 / mixed, a tie on every third row, alpha read from the device and alpha taken by the
    temperature step inside the launch (the restatement then uses the alpha the launch returned)."""
    worst = {}
    for mode in R.TERM_MODES:
        c = R.sac_loss_case(B, mode)
        got = run_sac(c, 0.37, 0.99)
        assert np.all(got["dq1n"][::3] * F32(B) == -0.5) and np.all(got["dq2n"][::3] * F32(B) == -0.5)
        merge(worst, R.sac_ratios(got, sac_ref(c, 0.37, 0.99), B))
        state, out = torch.tensor(R.ALPHA_STATE0, device=DEV), torch.zeros(2, device=DEV)
        got = run_sac(c, None, 0.99, alpha_step=(*R.ALPHA_ARGS, state, out))
        alpha = float(out[0])
        assert alpha > 1.0 and float(state[3]) == R.ALPHA_STATE0[3] + 1
        merge(worst, R.sac_ratios(got, sac_ref(c, alpha, 0.99), B))
    report("sac_losses B=%d" % B, worst)


@pytest.mark.parametrize("B", R.SAC_EXACT_B)
def test_sac_losses_are_exact_where_fp32_is(B):
    c = R.sac_exact_case(B)
    got, ref = run_sac(c, 0.25, 0.5), sac_ref(c, 0.25, 0.5)
    for key in ("dq1", "dq2", "dq1n", "dq2n"):
        assert np.array_equal(got[key].astype(F64), ref[key]), key
    assert np.array_equal(got["sums"], ref["sums"])
    print("RATIO sac_losses exact B=%d: 0.0000" % B)


def fold_setup(B, A):
    """The sampling launch's partial moments and log-probabilities, and a loss case that uses them."""
    from torchrl_amd import _C
    s = {k: dev(v) for k, v in R.samples_case(B, A).items()}
    mom_part = torch.zeros((B + 63) // 64, 12, dtype=torch.float64, device=DEV)
    logp = _C.sac_samples(s["head"], s["head2"], s["eps1"], s["eps2"], s["obs"], s["acts"], s["next_obs"], mom_part=mom_part)[1]
    c = R.sac_loss_case(B, "mixed", seed=1)
    c["logp"] = host(logp)
    return s["head"], logp, mom_part, c


@pytest.mark.parametrize("A", R.FOLD_A)
@pytest.mark.parametrize("B", R.SAC_B)
def test_sac_riders_equal_the_separate_launch_and_the_restatement(B, A):
    """With `alpha_step=` state, alpha and every output are bit-equal to trl_sac_alpha_step_f32 as a launch of its own on
    the same logp; with `fold=` the twelve logged moments are those of the float64 restatement: mean and std rel 1e-12,
    max / min exact, NaN std of logp at B = 1 and of all three at B = A = 1.  B = 4097 and 8200 have more than 64 partial
    rows."""
    from torchrl_amd import _C
    head, logp, mom_part, c = fold_setup(B, A)
    ins = [dev(c[k]) for k in R.SAC_KEYS]
    state_a, out_a = torch.tensor(R.ALPHA_STATE0, device=DEV), torch.zeros(2, device=DEV)
    _C.sac_alpha_step(logp, *R.ALPHA_ARGS, state_a, out_a)
    sums_a = f64(4)
    outs_a = _C.sac_losses(*ins, out_a[0:1], 0.99, sums_a)
    state_b, out_b, sums_b = torch.tensor(R.ALPHA_STATE0, device=DEV), torch.zeros(2, device=DEV), f64(4)
    mom_b = torch.zeros(3, 4, dtype=torch.float64, device=DEV)
    outs_b = _C.sac_losses(*ins, None, 0.99, sums_b, alpha_step=(*R.ALPHA_ARGS, state_b, out_b), fold=(mom_part, A, mom_b))
    assert torch.equal(state_a, state_b) and torch.equal(out_a, out_b) and torch.equal(sums_a, sums_b)
    assert float(state_b[3]) == R.ALPHA_STATE0[3] + 1 and float(out_b[0]) != 0.0
    assert all(torch.equal(x, y) for x, y in zip(outs_a, outs_b))
    ref = R.policy_moments_ref(host(head), host(logp), A)
    assert np.isnan(ref[1, 1]) == (B == 1) and np.isnan(ref[0, 1]) == np.isnan(ref[2, 1]) == (B == 1 and A == 1)
    report("sac_losses fold B=%d A=%d" % (B, A), {"moments": R.moments_ratio(host(mom_b), ref)})


@pytest.mark.parametrize("A", R.FOLD_A)
@pytest.mark.parametrize("B", R.SAC_B)
def test_sac_fold_equals_moments_multi_bit_for_bit(B, A):
    """The fold's twelve outputs against trl_moments_multi_f64 on the same head and logp, bit for bit: two launches that
    log the same statistic add the same doubles in the same order (moments_block follows the fold: one row per thread, 64
    rows per butterfly, partial p into slot p % 64 in ascending p, one butterfly over the slots)."""
    from torchrl_amd import _C
    head, logp, mom_part, c = fold_setup(B, A)
    mom_a, mom_b = (torch.zeros(3, 4, dtype=torch.float64, device=DEV) for _ in range(2))
    _C.moments_multi([(head, mom_a[0], 2 * A, A, A, -20.0, 2.0), (logp, mom_a[1], 1, 0, 1, -INF, INF),
                      (head, mom_a[2], 2 * A, 0, A, -INF, INF)])
    _C.sac_losses(*[dev(c[k]) for k in R.SAC_KEYS], torch.ones(1, device=DEV), 0.99, f64(4), fold=(mom_part, A, mom_b))
    ma, mb = host(mom_a), host(mom_b)
    keep = ~np.isnan(ma)
    assert np.array_equal(np.isnan(mb), ~keep)
    print("RATIO sac_losses fold vs moments_multi B=%d A=%d: worst relative difference %.3e" % (
        B, A, np.max(np.abs(mb[keep] - ma[keep]) / np.abs(ma[keep]))))
    assert np.array_equal(ma[:, 2:], mb[:, 2:])
    assert np.array_equal(ma[keep], mb[keep]), (ma, mb)


# ------------------------------------------------------------------ trl_sac_alpha_step_f32
@pytest.mark.parametrize("k,B", list(enumerate(R.ALPHA_B)))
def test_alpha_step_three_chained_calls(k, B):
    """log_alpha abs 1e-6, Adam's moments rel 1e-4, alpha_loss rel 1e-6 (the project's bounds) against the float64 chain.
    alpha against the float64 exp of the RETURNED log_alpha within (2 + |log_alpha|) 2^-23 relative: __expf(x) is
    exp2(x log2(e)) -- the product rounds once and log2(e) is a rounded constant, together |x log2(e)| 2^-23 in the
    exponent, i.e. |x| 2^-23 relative in the result -- and the hardware exp2 (v_exp_f32) is accurate to one ulp, at most
    2^-23 relative, as the ISA manual states; the microarchitecture notes of this project give no other figure.
    Hence (1 + |x|) 2^-23, one further 2^-23 of room.  |log_alpha| <= 3 (starts 0.1, -2.9, 2.9)."""
    from torchrl_amd import _C
    s0 = (R.ALPHA_LA0[k],) + R.ALPHA_STATE0[1:]
    state, out = torch.tensor(s0, dtype=torch.float32, device=DEV), torch.zeros(2, device=DEV)
    ref_state, worst = np.array(s0), {}
    for call in range(3):
        logp = R.alpha_logp_case(B, call)
        _C.sac_alpha_step(dev(logp), *R.ALPHA_ARGS, state, out)
        ref_state, _, ref_loss = R.alpha_step_ref(ref_state, logp, *R.ALPHA_ARGS)
        merge(worst, R.alpha_ratios(host(state), float(out[0]), float(out[1]), ref_state, ref_loss))
    assert float(state[3]) == s0[3] + 3 and abs(float(state[0])) <= 3.0
    report("sac_alpha_step B=%d" % B, worst)


# ------------------------------------------------------------------ trl_detac_losses_f32
def run_detac(c, twin, with_qn, gamma):
    from torchrl_amd import _C
    sums = f64(4)
    outs = _C.detac_losses(dev(c["q1"]), dev(c["q2"]) if twin else None, dev(c["tq1"]), dev(c["tq2"]) if twin else None,
                           dev(c["rew"]), dev(c["term"]), dev(c["qn"]) if with_qn else None, gamma, sums)
    torch.cuda.synchronize()
    got = dict(zip(("dq1", "dq2", "dqn"), [None if o is None else host(o).reshape(-1) for o in outs]))
    got["sums"] = host(sums)
    ref = R.detac_losses_ref(c["q1"], c["q2"] if twin else None, c["tq1"], c["tq2"] if twin else None, c["rew"], c["term"],
                             c["qn"] if with_qn else None, float(F32(gamma)))
    return got, ref


@pytest.mark.parametrize("B", R.DETAC_B)
def test_detac_losses_against_the_restatement(B):
    """One critic (DDPG) and two (TD3), with and without the policy loss: dq2 / dqn are None and their sums 0 when not
    asked for, dqn B is exactly -1."""
    worst = {}
    c = R.detac_case(B)
    for twin in (True, False):
        for with_qn in (True, False):
            got, ref = run_detac(c, twin, with_qn, 0.99)
            merge(worst, R.detac_ratios(got, ref, B))
    report("detac_losses B=%d" % B, worst)


@pytest.mark.parametrize("B", R.DETAC_EXACT_B)
def test_detac_losses_are_exact_where_fp32_is(B):
    got, ref = run_detac(R.detac_exact_case(B), True, True, 0.5)
    for key in ("dq1", "dq2", "dqn"):
        assert np.array_equal(got[key].astype(F64), ref[key]), key
    assert np.array_equal(got["sums"], ref["sums"])
    print("RATIO detac_losses exact B=%d: 0.0000" % B)


# ------------------------------------------------------------------ trl_noisy_action_f32, trl_polyak_f32
@pytest.mark.parametrize("n", R.STREAM_N)
def test_noisy_action_equals_the_float32_restatement(n):
    """No contraction is possible across the clamps: bit for bit the float32 numpy restatement (n = 262149 runs the
    grid-stride loop of a launch capped at 1024 blocks)."""
    from torchrl_amd import _C
    a, eps = R.stream_case(n)
    got = host(_C.noisy_action(dev(a), dev(eps), 0.3))                        # the default clips: none
    assert np.array_equal(got, R.noisy_action_ref(a, eps, 0.3, dt=F32))
    for sigma, clip, lo, hi in R.NOISE_ARGS:
        got = host(_C.noisy_action(dev(a), dev(eps), sigma, clip, lo, hi))
        assert np.array_equal(got, R.noisy_action_ref(a, eps, sigma, clip, lo, hi, dt=F32)), (sigma, clip, lo, hi)
        if sigma == 0.0:
            assert np.array_equal(got, np.clip(a, F32(lo), F32(hi)))
    print("RATIO noisy_action n=%d: 0.0000" % n)


@pytest.mark.parametrize("n", R.STREAM_N)
def test_polyak_against_the_restatement(n):
    from torchrl_amd import _C
    t, s = R.stream_case(n)
    worst = {}
    for tau in R.POLYAK_TAU:
        tgt = dev(t)
        _C.polyak(tgt, dev(s), tau)
        worst["tau=%g" % tau] = R.polyak_ratio(host(tgt), t, s, tau)
        if tau == 1.0:
            assert np.array_equal(host(tgt), s)                               # the source, exactly
        if tau == 0.0:
            assert np.array_equal(host(tgt).view(np.uint32), t.view(np.uint32))   # the target, bit for bit
    report("polyak n=%d" % n, worst)


# ------------------------------------------------------------------ trl_moments_multi_f64
@pytest.mark.parametrize("rows,ld,off,width", R.MOMENT_CASES)
def test_moments_against_the_restatement(rows, ld, off, width):
    """Widths that do not divide 4096, widths above 4096 (no whole row per stride), one element (NaN std); with and
    without the [-20, 2] clamp; as one launch of two statistics and as launches of their own."""
    from torchrl_amd import _C
    x = R.moments_case(rows, ld)
    xd = dev(x)
    out = torch.zeros(2, 4, dtype=torch.float64, device=DEV)
    _C.moments_multi([(xd, out[k], ld, off, width, lo, hi) for k, (lo, hi) in enumerate(R.MOMENT_CLAMPS)])
    worst = {}
    for k, (lo, hi) in enumerate(R.MOMENT_CLAMPS):
        ref = R.moments_ref(x, ld, off, width, lo, hi)
        assert np.isnan(ref[1]) == (rows * width == 1)
        worst["clamp" if k else "plain"] = R.moments_ratio(host(out[k]), ref)
        single = torch.zeros(4, dtype=torch.float64, device=DEV)
        _C.moments(xd, single, ld, off, width, lo, hi)
        assert np.array_equal(host(single), host(out[k]), equal_nan=True)
    report("moments rows=%d ld=%d off=%d width=%d" % (rows, ld, off, width), worst)


@pytest.mark.parametrize("count", [1, 3, 4])
def test_moments_ring_files_the_statistics_block(count):
    """Update counts 1, slots and slots + 1: slot (count - 1) % slots receives this launch's statistics and a verbatim
    copy of every other word of `raw`; the other slots keep their sentinel."""
    from torchrl_amd import _C
    slots = 3
    x1, x2 = R.moments_case(300, 12), R.moments_case(700, 9)
    raw = torch.zeros(96, dtype=torch.uint8, device=DEV)
    vals = raw.view(torch.float64)
    vals[4:8] = torch.tensor([1.5, -2.5, 3.25, 1e300], dtype=torch.float64)
    ring = torch.full((slots, 96), 0xAB, dtype=torch.uint8, device=DEV)
    counter = torch.tensor([float(count)], dtype=torch.float64, device=DEV)
    _C.moments_multi([(dev(x1), vals[0:4], 12, 6, 6, -20.0, 2.0), (dev(x2), vals[8:12], 9, 2, 7, -INF, INF)],
                     ring=(raw, ring, counter))
    got = host(vals)
    assert R.moments_ratio(got[0:4], R.moments_ref(x1, 12, 6, 6, -20.0, 2.0)) <= 1.0
    assert R.moments_ratio(got[8:12], R.moments_ref(x2, 9, 2, 7)) <= 1.0
    assert got[4:8].tolist() == [1.5, -2.5, 3.25, 1e300] and float(counter[0]) == count
    filed = (count - 1) % slots
    for k in range(slots):
        if k == filed:
            assert torch.equal(ring[k], raw)
        else:
            assert bool((ring[k] == 0xAB).all()), k


# ------------------------------------------------------------------ trl_dqn_td_loss_f32
def run_dqn(c, gamma, ring=None):
    from torchrl_amd import _C
    sums = f64(3)
    dq = _C.dqn_td_loss(dev(c["q"]), dev(c["acts"]), dev(c["qn"]), dev(c["rew"]), dev(c["term"]), gamma, sums, ring=ring)
    torch.cuda.synchronize()
    return dict(dq=host(dq), sums=host(sums))


@pytest.mark.parametrize("float_acts", [False, True], ids=["int64", "float"])
@pytest.mark.parametrize("A", R.DQN_A)
@pytest.mark.parametrize("B", R.DQN_B)
def test_dqn_td_loss_against_the_restatement(B, A, float_acts):
    """Stored actions -1, A, A + 5 and (floats) NaN and 2.7 on the first rows behave as the clamp rule says; dq is zero
    off the chosen column; terminals mixed."""
    c = R.dqn_case(B, A, float_acts)
    ref = R.dqn_td_ref(c["q"], c["acts"], c["qn"], c["rew"], c["term"], G32)
    report("dqn_td_loss B=%d A=%d %s" % (B, A, "float" if float_acts else "int64"), R.dqn_ratios(run_dqn(c, 0.99), ref, B))


@pytest.mark.parametrize("u", [0, 3, 4])
def test_dqn_td_loss_files_ring_row_u_mod_slots(u):
    slots = 4
    c = R.dqn_case(257, 6, True)
    ring = torch.full((slots, 3), -77.0, dtype=torch.float64, device=DEV)
    counter = torch.tensor([float(u)], dtype=torch.float64, device=DEV)
    got = run_dqn(c, 0.99, ring=(ring, counter))
    assert np.array_equal(got["sums"], run_dqn(c, 0.99)["sums"])
    rows = host(ring)
    for k in range(slots):
        assert np.array_equal(rows[k], got["sums"] if k == u % slots else np.full(3, -77.0)), k
    assert float(counter[0]) == u


# ------------------------------------------------------------------ trl_quantile_huber_f32
def run_quantile(c, A, Q, ring=None):
    """(dq, sums) through the wrapper, and the per-sample partial sums from a second call with a workspace of its own."""
    from torchrl_amd import _C
    ins = [dev(c[k]) for k in ("q", "acts", "qn", "rew", "term")]
    sums = f64(3)
    dq = _C.quantile_huber(*ins, R.QR_GAMMA, A, Q, sums, ring=ring)
    B = int(ins[0].shape[0])
    dq2, part, sums2 = torch.full_like(ins[0], 7.0), f64(2 * B), f64(3)
    ai, af = _C._acts_ptrs(ins[1])
    _C.check(_C.lib().trl_quantile_huber_f32(_C.dev_ptr(ins[0]), ai, af, _C.dev_ptr(ins[2]), _C.dev_ptr(ins[3]),
                                             _C.dev_ptr(ins[4]), R.QR_GAMMA, B, A, Q, _C.dev_ptr(dq2),
                                             _C.dev_ptr(part, torch.float64), _C.dev_ptr(sums2, torch.float64), None, 0, None,
                                             _C.stream_ptr(DEV)), "trl_quantile_huber_f32")
    torch.cuda.synchronize()
    assert torch.equal(dq, dq2) and torch.equal(sums, sums2)
    part = host(part).reshape(B, 2)
    return dict(dq=host(dq), sums=host(sums), loss_b=part[:, 0], theta_b=part[:, 1])


@pytest.mark.parametrize("float_acts", [False, True], ids=["int64", "float"])
@pytest.mark.parametrize("B,A,Q", R.QR_CASES)
def test_quantile_huber_against_the_restatement(B, A, Q, float_acts):
    """Q below 64, no multiple of 4, above 256; terminal rows; a* ties (first index); out-of-range stored actions; d = 0
    and |d| = 1 planted.  Per-sample loss, gradient and the three sums; dq zero off the taken action's quantiles."""
    c = R.qr_case(B, A, Q, float_acts)
    ref = R.quantile_huber_ref(c["q"], c["acts"], c["qn"], c["rew"], c["term"], R.QR_GAMMA, A, Q)
    got = run_quantile(c, A, Q)
    np.testing.assert_allclose(got["theta_b"], ref["th"].sum(1), rtol=1e-12, atol=1e-12)
    report("quantile_huber B=%d A=%d Q=%d %s" % (B, A, Q, "float" if float_acts else "int64"), R.qr_ratios(got, ref, B, A, Q))


def test_quantile_huber_files_ring_row_u_mod_slots():
    c = R.qr_case(3, 3, 5, False)
    ring = torch.full((2, 3), -77.0, dtype=torch.float64, device=DEV)
    got = run_quantile(c, 3, 5, ring=(ring, torch.tensor([5.0], dtype=torch.float64, device=DEV)))
    assert np.array_equal(host(ring), np.stack([np.full(3, -77.0), got["sums"]]))


# ------------------------------------------------------------------ trl_eps_greedy_i64
@pytest.mark.parametrize("N,A,Q", R.EPS_CASES)
def test_eps_greedy_equals_the_restatement(N, A, Q):
    """Q = 1: a thread per env; quantile nets: a wave per env, four envs per block.  Exact ties give the first index,
    u == epsilon keeps the greedy action, u / rand_act None is greedy."""
    from torchrl_amd import _C
    c = R.eps_case(N, A, Q)
    q, u, ra = dev(c["q"]), dev(c["u"]), dev(c["rand_act"])
    greedy = R.eps_greedy_ref(c["q"], A, Q)
    for kw in (dict(u=None, rand_act=None), dict(u=u, rand_act=None), dict(u=None, rand_act=ra)):
        assert np.array_equal(host(_C.eps_greedy(q, A, Q, kw["u"], kw["rand_act"], R.EPSILON)), greedy)
    got = host(_C.eps_greedy(q, A, Q, u, ra, R.EPSILON))
    assert np.array_equal(got, R.eps_greedy_ref(c["q"], A, Q, c["u"], c["rand_act"], R.EPSILON))
    assert np.array_equal(got[::3], greedy[::3])                              # u == epsilon there
    assert np.array_equal(host(_C.eps_greedy(q, A, Q, u, ra, 0.0)), greedy)
    assert np.array_equal(host(_C.eps_greedy(q, A, Q, u, ra, 1.5)), c["rand_act"])


@pytest.mark.parametrize("Q", [1, 5])
def test_eps_greedy_advances_the_ring_row(Q):
    from torchrl_amd import _C
    c = R.eps_case(5, 6, Q)
    row = torch.tensor([1], dtype=torch.int64, device=DEV)
    for want in (2, 0, 1):                                                   # n_rows = 3: 1 -> 2 -> 0 (wraps) -> 1
        act = _C.eps_greedy(dev(c["q"]), 6, Q, None, None, 0.0, ring_row=row, n_rows=3)
        assert int(row[0]) == want and np.array_equal(host(act), R.eps_greedy_ref(c["q"], 6, Q))


# ------------------------------------------------------------------ trl_tanh_gauss_rsample_fwd_f32 / _bwd_f32
@pytest.mark.parametrize("B,A,tanh", R.RSAMPLE_CASES)
def test_rsample_fwd_bwd_vs_autograd(B, A, tanh):
    """test_sac_gpu.py's comparison with autograd (same tolerances, same unsaturated-row rule and floor) at the block
    boundary of 64 rows, one row, one action dimension and without tanh; the elements whose log_std lies outside
    [-20, 2] have zero gradient."""
    from torchrl_amd import _C
    head, eps, d_act = (torch.tensor(t) for t in R.rsample_case(B, A))
    alpha, w_std, w_mean = 0.37, 1e-3, 2e-3
    hr = head.clone().requires_grad_(True)
    a, lp, mean, log_std = R.rsample(hr, eps, tanh)
    loss = (a * d_act).sum() + (alpha / B) * lp.sum() + w_std * (log_std ** 2).mean() + w_mean * (mean ** 2).mean()
    loss.backward()
    act, logp = _C.rsample_fwd(head.to(DEV), eps.to(DEV), tanh)
    np.testing.assert_allclose(act.cpu().numpy(), a.detach().numpy(), atol=1e-6)
    ok = (a.detach().abs().max(dim=1).values < 0.999).numpy() if tanh else np.ones(B, dtype=bool)
    assert ok.mean() > 0.8
    np.testing.assert_allclose(logp.cpu().numpy()[ok], lp.detach().numpy()[ok, 0], rtol=2e-5, atol=2e-4)
    d_head = _C.rsample_bwd(head.to(DEV), eps.to(DEV), act, d_act.to(DEV), torch.tensor([alpha], device=DEV), 1.0 / B,
                            w_std, w_mean, tanh)
    okr = torch.as_tensor(ok)
    err = (d_head.cpu() - hr.grad)[okr].abs().max().item()
    tol = 5e-5 * max(1.0, hr.grad[okr].abs().max().item())
    print("RATIO rsample B=%d A=%d tanh=%d: d_head %.4f" % (B, A, tanh, err / tol))
    assert err < tol, err
    outside = (head[:, A:] < -20.0) | (head[:, A:] > 2.0)
    assert int(outside.sum()) == (2 if B > 1 else 1)
    assert bool((d_head.cpu()[:, A:][outside] == 0.0).all()) and bool((hr.grad[:, A:][outside] == 0.0).all())


# ------------------------------------------------------------------ argument errors
def test_argument_errors_raise():
    from torchrl_amd import _C
    c = {k: dev(v) for k, v in R.sac_loss_case(8, "mixed").items()}
    ins = [c[k] for k in R.SAC_KEYS]
    alpha, sums = torch.ones(1, device=DEV), torch.zeros(4, dtype=torch.float64, device=DEV)
    with pytest.raises(_C.TrlError, match="empty batch"):
        _C.sac_losses(*[t[:0] for t in ins], alpha, 0.99, sums)
    with pytest.raises(_C.TrlError, match="in3 is None"):
        _C.sac_losses(*ins[:3], None, *ins[4:], alpha, 0.99, sums)
    with pytest.raises(_C.TrlError, match="alpha is None"):
        _C.sac_losses(*ins, None, 0.99, sums)
    with pytest.raises(_C.TrlError, match="empty batch"):
        _C.sac_alpha_step(c["logp"][:0], -6.0, 3e-4, torch.zeros(4, device=DEV), torch.zeros(2, device=DEV))
    with pytest.raises(_C.TrlError, match="empty batch"):
        _C.detac_losses(c["q1"][:0], None, c["tq1"][:0], None, c["rew"][:0], c["term"][:0], None, 0.99, sums)
    with pytest.raises(_C.TrlError, match="null pointer"):
        _C.detac_losses(c["q1"], None, None, None, c["rew"], c["term"], None, 0.99, sums)
    with pytest.raises(_C.TrlError, match="come in pairs"):
        _C.check(_C.lib().trl_detac_losses_f32(
            _C.dev_ptr(c["q1"]), _C.dev_ptr(c["q2"]), _C.dev_ptr(c["tq1"]), _C.dev_ptr(c["tq2"]), _C.dev_ptr(c["rew"]),
            _C.dev_ptr(c["term"]), None, 0.99, 8, _C.dev_ptr(c["q1"].clone()), None, None,
            _C.dev_ptr(sums, torch.float64), _C.stream_ptr(DEV)), "trl_detac_losses_f32")
    d = {k: dev(v) for k, v in R.dqn_case(8, 6, False).items()}
    sums3 = torch.zeros(3, dtype=torch.float64, device=DEV)
    with pytest.raises(_C.TrlError):
        _C.dqn_td_loss(d["q"][:0], d["acts"][:0], d["qn"][:0], d["rew"][:0], d["term"][:0], 0.99, sums3)
    with pytest.raises(_C.TrlError, match="q_next is None"):
        _C.dqn_td_loss(d["q"], d["acts"], None, d["rew"], d["term"], 0.99, sums3)
    with pytest.raises(_C.TrlError, match="has dtype"):
        _C.dqn_td_loss(d["q"], d["acts"].int(), d["qn"], d["rew"], d["term"], 0.99, sums3)
    with pytest.raises(_C.TrlError, match="q_next is None"):
        _C.quantile_huber(d["q"], d["acts"], None, d["rew"], d["term"], 0.99, 2, 3, sums3)
    ptr = _C.dev_ptr
    for ai, af in ((ptr(d["acts"], torch.int64), ptr(d["acts"].float())), (None, None)):     # both, neither
        with pytest.raises(_C.TrlError, match="exactly one of acts"):
            _C.check(_C.lib().trl_dqn_td_loss_f32(ptr(d["q"]), ai, af, ptr(d["qn"]), ptr(d["rew"]), ptr(d["term"]), 0.99, 8, 6,
                                                  ptr(torch.empty_like(d["q"])), ptr(sums3, torch.float64), None, 0, None,
                                                  _C.stream_ptr(DEV)), "trl_dqn_td_loss_f32")
        with pytest.raises(_C.TrlError, match="exactly one of acts"):
            _C.check(_C.lib().trl_quantile_huber_f32(ptr(d["q"]), ai, af, ptr(d["qn"]), ptr(d["rew"]), ptr(d["term"]), 0.99, 8,
                                                     2, 3, ptr(torch.empty_like(d["q"])), ptr(f64(16), torch.float64),
                                                     ptr(sums3, torch.float64), None, 0, None, _C.stream_ptr(DEV)),
                     "trl_quantile_huber_f32")
    with pytest.raises(_C.TrlError, match="no CPU path"):
        _C.eps_greedy(d["q"].cpu(), 6, 1, None, None, 0.1)
    with pytest.raises(_C.TrlError, match="source is None"):
        _C.polyak(c["q1"], None, 0.005)
    with pytest.raises(_C.TrlError, match="eps is None"):
        _C.noisy_action(c["q1"], None, 0.1)
    torch.cuda.synchronize()
    assert float(sums.abs().sum()) == 0.0 and float(sums3.abs().sum()) == 0.0    # nothing was launched
