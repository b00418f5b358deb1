"""Restatements of the older off-policy kernels (torchrl_amd/csrc/k_sac.hip, k_dqn.hip), written from the formulas of the
algorithms they serve -- twin_sac_q.py, ddpg.py, td3.py, dqn.py, qrdqn.py, discrete_policies.py -- and not from the kernel
code: Huber in its two-branch form, the quantile weight as |tau_j - 1[diff < 0]|, the gradient of torch.min as 1 / 0.5 / 0.

Every restatement takes `dt`: numpy float64 (the reference value) or numpy float32 (the same formulas with every operation
rounded to fp32, sums accumulated the way the kernels do -- in double over fp32 terms, except the quantile-Huber column
sums, which a thread keeps in fp32).  tests/test_offpolicy_kernels_cpu.py holds the float32 run to the bounds below, and
tests/test_offpolicy_kernels_gpu.py holds the kernels to the same bounds on the same inputs: the input builders and the
`*_ratios` functions (worst err / bound, 1.0 = at the bound) live here so that both files see the same cases.  numpy only
(the sampler's autograd restatement `rsample` is the oracle's torch function, re-exported)."""
import numpy as np

from _sac_v_ref import U, samples_ref                                    # noqa: F401  (U = 2^-24)
from oracle.sac import rsample                                           # noqa: F401  (head, eps) -> (a, logp, mean, log_std)

F32, F64 = np.float32, np.float64
INF = float("inf")


def _v(t, dt):
    return None if t is None else np.asarray(t).astype(dt).reshape(-1)


def _d(t):
    return np.asarray(t).astype(F64)


# ------------------------------------------------------------------ twin-Q SAC losses (twin_sac_q.py:125-155)
SAC_KEYS = ("q1", "q2", "tq1", "tq2", "logp_next", "rew", "term", "q1n", "q2n", "logp")
SAC_B = (1, 64, 65, 1023, 1025, 4096, 4097, 8200)                        # above 4096 a thread takes a second group of rows
SAC_EXACT_B = (64, 1024, 8192)
TERM_MODES = ("zeros", "ones", "mixed")
ALPHA_STATE0 = (0.1, 0.02, 0.003, 5.0)                                   # log_alpha, exp_avg, exp_avg_sq, step
ALPHA_ARGS = (-6.0, 3e-4)                                                # target entropy, learning rate


def _terminals(rs, B, mode):
    return {"zeros": np.zeros(B), "ones": np.ones(B), "mixed": (rs.rand(B) < 0.3)}[mode].astype(F32)


def sac_loss_case(B, term_mode, seed=0):
    """float32 inputs of trl_sac_losses_f32; every third row an exact tie q1n == q2n (and tq1 == tq2)."""
    rs = np.random.RandomState(1000 * seed + B)
    r = lambda s, o=0.0: (rs.randn(B) * s + o).astype(F32)
    c = dict(q1=r(2), q2=r(2), tq1=r(3), tq2=r(3), logp_next=r(3, -4), rew=r(1), q1n=r(2), q2n=r(2), logp=r(3, -4))
    c["term"] = _terminals(rs, B, term_mode)
    c["q2n"][::3] = c["q1n"][::3]
    c["tq2"][::3] = c["tq1"][::3]
    return c


def sac_exact_case(B):
    """Multiples of 1/8 with |x| <= 4: with gamma = 0.5, alpha = 0.25 and B a power of two no fp32 operation rounds."""
    rs = np.random.RandomState(B)
    c = {k: (rs.randint(-32, 33, B) / 8.0).astype(F32) for k in SAC_KEYS}
    c["term"] = rs.randint(0, 2, B).astype(F32)
    c["q2n"][::4] = c["q1n"][::4]
    return c


def sac_losses_ref(q1, q2, tq1, tq2, logp_next, rew, term, q1n, q2n, logp, alpha, gamma, dt=F64):
    """q_target = r + (1 - d) gamma (min(tq1, tq2) - alpha logp'); qf_i loss = mean((q_i - q_target)^2);
    policy loss = mean(alpha logp - min(q1n, q2n)).  dict(dq1, dq2, dq1n, dq2n, sums[4] = loss sums 1 and 2, policy sum,
    reward sum, and the magnitudes the bounds scale with)."""
    q1, q2, tq1, tq2, logp_next, rew, term, q1n, q2n, logp = (_v(t, dt) for t in (q1, q2, tq1, tq2, logp_next, rew, term,
                                                                                   q1n, q2n, logp))
    alpha, gamma, one, two, half, zero = dt(alpha), dt(gamma), dt(1), dt(2), dt(0.5), dt(0)
    inv_b = one / dt(q1.size)
    tmin = np.minimum(tq1, tq2)
    qt = rew + (one - term) * gamma * (tmin - alpha * logp_next)
    e1, e2 = q1 - qt, q2 - qt
    tie = q1n == q2n
    w1 = np.where(q1n < q2n, one, np.where(tie, half, zero))
    w2 = np.where(q2n < q1n, one, np.where(tie, half, zero))
    qn = np.minimum(q1n, q2n)
    pol = alpha * logp - qn
    out = dict(e1=_d(e1), e2=_d(e2), dq1=two * e1 * inv_b, dq2=two * e2 * inv_b, dq1n=-w1 * inv_b, dq2n=-w2 * inv_b,
               w1=_d(w1), w2=_d(w2), pol=_d(pol))
    out["sums"] = np.array([(_d(e1) ** 2).sum(), (_d(e2) ** 2).sum(), _d(pol).sum(), _d(rew).sum()])
    mag = _d(np.abs(rew)) + float(gamma) * (_d(np.abs(tmin)) + float(alpha) * _d(np.abs(logp_next)))
    out["mag_q"] = [_d(np.abs(q1)) + mag, _d(np.abs(q2)) + mag]
    out["pol_abs"] = float(alpha) * _d(np.abs(logp)) + _d(np.abs(qn))
    out["sum_abs_rew"] = float(_d(np.abs(rew)).sum())
    return out


def _td_ratios(out, got, ref, B, crit):
    """|d dq| <= 8 U mag 2 / B; a loss sum within sum(2 |e| delta + delta^2 + 2 U e^2), delta = 8 U mag."""
    for key, diff, mag, slot in crit:
        delta = 8 * U * mag
        out[key] = float(np.max(np.abs(_d(got[key]).reshape(-1) - _d(ref[key]).reshape(-1)) / (delta * 2 / B)))
        bound = np.sum(2 * np.abs(ref[diff]) * delta + delta ** 2 + 2 * U * ref[diff] ** 2)
        out["sum_" + key] = float(abs(got["sums"][slot] - ref["sums"][slot]) / bound)


def sac_ratios(got, ref, B):
    """{name: worst err / bound} of a trl_sac_losses_f32 result against the float64 restatement `ref`; the exact
    properties (dq_n B is -1, -0.5 or 0, and the restatement's) are asserted on the spot."""
    out = {}
    _td_ratios(out, got, ref, B, [("dq1", "e1", ref["mag_q"][0], 0), ("dq2", "e2", ref["mag_q"][1], 1)])
    out["sum_pol"] = float(abs(got["sums"][2] - ref["sums"][2]) / (4 * U * ref["pol_abs"].sum()))
    out["sum_rew"] = float(abs(got["sums"][3] - ref["sums"][3]) / (4 * U * ref["sum_abs_rew"]))
    for key, w in (("dq1n", "w1"), ("dq2n", "w2")):
        scaled = np.asarray(got[key], dtype=F32).reshape(-1) * F32(B)
        assert np.array_equal(scaled, -ref[w].astype(F32)), key
        assert set(np.unique(scaled)) <= {-1.0, -0.5, 0.0}, key
    return out


# ------------------------------------------------------------------ temperature step (twin_sac_q.py:111-120)
ALPHA_B = (1, 1023, 1025, 4097)
ALPHA_LA0 = (0.1, -2.9, 2.9, 0.1)                                        # the log_alpha each of them starts from


def alpha_logp_case(B, call):
    rs = np.random.RandomState(77 * B + call)
    return (rs.randn(B) * 3 - 4 - 2 * call).astype(F32)


def alpha_step_ref(state, logp, target_entropy, lr, beta1=0.9, beta2=0.999, eps=1e-8, dt=F64):
    """One Adam step on log_alpha with the gradient -(mean(logp) + H) of alpha_loss = -mean(log_alpha (logp + H)):
    (state' = [log_alpha, exp_avg, exp_avg_sq, step], alpha = exp(log_alpha'), alpha_loss at the old log_alpha)."""
    la, m, v, t = (dt(x) for x in state)
    b1, b2, one = dt(beta1), dt(beta2), dt(1)
    mean_term = dt(_d(logp).sum() / np.asarray(logp).size) + dt(target_entropy)     # (the mean itself is summed in double)
    loss, g, t = -la * mean_term, -mean_term, t + one
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * g * g
    bc1, bc2 = one - b1 ** t, one - b2 ** t
    la = la - (dt(lr) / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + dt(eps)))
    return np.array([la, m, v, t], dtype=dt), dt(np.exp(la)), dt(loss)


def alpha_ratios(state, alpha, loss, ref_state, ref_loss):
    """The project's bounds (test_twin_sac_q_update_matches_reference, the V-MPO dual state): log_alpha abs 1e-6, Adam's
    moments rel 1e-4, alpha_loss rel 1e-6; alpha against the float64 exp of the RETURNED log_alpha within
    (2 + |log_alpha|) 2^-23 relative."""
    state, ref_state = _d(state), _d(ref_state)
    assert state[3] == ref_state[3]
    return {"log_alpha": abs(state[0] - ref_state[0]) / 1e-6,
            "exp_avg": abs(state[1] - ref_state[1]) / (1e-4 * abs(ref_state[1])),
            "exp_avg_sq": abs(state[2] - ref_state[2]) / (1e-4 * abs(ref_state[2])),
            "alpha_loss": abs(float(loss) - float(ref_loss)) / (1e-6 * abs(float(ref_loss))),
            "alpha": abs(float(alpha) / np.exp(state[0]) - 1.0) / ((2 + abs(state[0])) * 2.0 ** -23)}


# ------------------------------------------------------------------ logged moments (twin_sac_q.py:190-207)
FOLD_A = (1, 6, 8)
FOLD_D = 5
MOMENT_RTOL = 1e-12
MOMENT_CASES = ((1, 1, 0, 1), (300, 12, 6, 6), (4097, 1, 0, 1), (700, 9, 2, 7), (4096, 2, 1, 1), (5, 5000, 0, 5000),
                (3, 4099, 2, 4097), (3000, 12, 6, 6))                    # (rows, ld, off, width); the last: five strides
MOMENT_CLAMPS = ((-INF, INF), (-20.0, 2.0))


def samples_case(B, A, seed=0):
    """float32 inputs of trl_sac_samples_f32: means around 0.7, raw log_std around -1 with a spread of 8 (many outside
    [-20, 2]) -- no logged mean is a cancelling sum."""
    rs = np.random.RandomState(31 * B + A + 7 * seed)
    r = lambda *s: rs.randn(*s).astype(F32)
    c = dict(head=r(B, 2 * A), head2=r(B, 2 * A), eps1=r(B, A), eps2=r(B, A), obs=r(B, FOLD_D), acts=r(B, A),
             next_obs=r(B, FOLD_D))
    for k in ("head", "head2"):
        c[k][:, :A] += F32(0.7)
        c[k][:, A:] = c[k][:, A:] * F32(8) - F32(1)
    return c


def moments_case(rows, ld, seed=0):
    rs = np.random.RandomState(rows + 3 * ld + seed)
    return (rs.randn(rows * ld) * 8 - 4.5).astype(F32)                       # (far enough from a cancelling sum, see below)


def moments_ref(x, ld, off, width, lo=-INF, hi=INF, order="plain"):
    """[mean, unbiased std (NaN for one element), max, min] over columns [off, off + width) of x seen as rows of ld,
    every value clamped to [lo, hi] first.  order = "waves": the same in double, summed as the kernels do -- sum and sum
    of squares per group of 64, groups added in turn, variance as (sum sq - sum mean) / (n - 1)."""
    t = np.clip(_d(x).reshape(-1, ld)[:, off:off + width], lo, hi).reshape(-1)
    if order == "plain":
        return np.array([t.mean(), t.std(ddof=1) if t.size > 1 else np.nan, t.max(), t.min()])
    s = sq = 0.0
    for k in range(0, t.size, 64):
        s += float(np.sum(t[k:k + 64]))
        sq += float(np.sum(t[k:k + 64] ** 2))
    mean = s / t.size
    sd = np.sqrt(max((sq - s * mean) / (t.size - 1), 0.0)) if t.size > 1 else np.nan
    return np.array([mean, sd, t.max(), t.min()])


def policy_moments_ref(head, logp, n_a, order="plain"):
    """(3, 4): the moments of the clamped log_std, of log_prob and of the mean."""
    head, logp = np.asarray(head), np.asarray(logp).reshape(-1)
    return np.stack([moments_ref(head, 2 * n_a, n_a, n_a, -20.0, 2.0, order), moments_ref(logp, 1, 0, 1, order=order),
                     moments_ref(head, 2 * n_a, 0, n_a, order=order)])


def moments_chain(rows, width):
    """The longest chain of additions behind a sum of the moment kernels: a row's columns in turn, a butterfly over 64 rows
    (6), the partials of a slot in turn (one in 64), a butterfly over the slots (6)."""
    return width + 6 + ((rows + 63) // 64 + 63) // 64 + 6


def moments_conditioning(x, ld, off, width, lo=-INF, hi=INF):
    """(sum |t| / |sum t|, (sum t^2 + 2 (sum t)^2 / n) / (2 sum (t - mean)^2)): how much a relative error of the two
    running sums is amplified in the mean and in the std (the variance is sum t^2 - (sum t)^2 / n; the root halves its
    relative error).  The kernels add exactly converted floats in double, so a sum carries at most chain * 2^-53 of
    sum |t| (sum t^2), chain = `moments_chain`; mean and std stay within rel 1e-12 while amplification * chain * 2^-53
    does -- asserted on every case's inputs: 5013 additions at width 5000 leave room for an amplification of 1.79 (the
    cases reach 1.63), 23 additions at 8 action dimensions for 390."""
    t = np.clip(_d(x).reshape(-1, ld)[:, off:off + width], lo, hi).reshape(-1)
    if t.size == 1:
        return 1.0, 1.0
    s, sq, var = t.sum(), (t ** 2).sum(), ((t - t.mean()) ** 2).sum()
    return float(np.abs(t).sum() / abs(s)), float((sq + 2 * s * s / t.size) / (2 * var))

def moments_ratio(got, ref):
    """Mean and std rel 1e-12, max / min exact, NaN std where the restatement's is."""
    got, ref = _d(got).reshape(-1, 4), _d(ref).reshape(-1, 4)
    assert np.array_equal(got[:, 2:], ref[:, 2:]), (got, ref)
    assert np.array_equal(np.isnan(got[:, :2]), np.isnan(ref[:, :2])), (got, ref)
    ok = ~np.isnan(ref[:, :2])
    return float(np.max(np.abs(got[:, :2][ok] - ref[:, :2][ok]) / (MOMENT_RTOL * np.abs(ref[:, :2][ok]))))


# ------------------------------------------------------------------ DDPG / TD3 (ddpg.py:59-73, td3.py:75-130)
DETAC_B = (1, 255, 256, 257, 1000)
DETAC_EXACT_B = (64, 512)


def detac_case(B, seed=0):
    rs = np.random.RandomState(500 * seed + B)
    r = lambda s: (rs.randn(B) * s).astype(F32)
    c = dict(q1=r(2), q2=r(2), tq1=r(3), tq2=r(3), rew=r(1), qn=r(2), term=_terminals(rs, B, "mixed"))
    c["tq2"][::3] = c["tq1"][::3]
    return c


def detac_exact_case(B):
    rs = np.random.RandomState(B + 1)
    c = {k: (rs.randint(-32, 33, B) / 8.0).astype(F32) for k in ("q1", "q2", "tq1", "tq2", "rew", "qn")}
    c["term"] = rs.randint(0, 2, B).astype(F32)
    return c


def detac_losses_ref(q1, q2, tq1, tq2, rew, term, qn, gamma, dt=F64):
    """q_target = r + (1 - d) gamma Q'(s', a'), Q' = tq1 (DDPG) or min(tq1, tq2) (TD3); MSE of one or two critics; with qn
    the policy loss -mean(Q(s, pi(s))), gradient -1 / B.  sums[4]: loss sums 1 and 2, sum(-qn), reward sum."""
    q1, q2, tq1, tq2, rew, term, qn = (_v(t, dt) for t in (q1, q2, tq1, tq2, rew, term, qn))
    gamma, one, two = dt(gamma), dt(1), dt(2)
    B = q1.size
    inv_b = one / dt(B)
    tv = tq1 if tq2 is None else np.minimum(tq1, tq2)
    qt = rew + (one - term) * gamma * tv
    mag = _d(np.abs(rew)) + float(gamma) * _d(np.abs(tv))
    e1 = q1 - qt
    out = dict(e1=_d(e1), dq1=two * e1 * inv_b, dq2=None, dqn=None, e2=None, mag_q=[_d(np.abs(q1)) + mag])
    sums = [(_d(e1) ** 2).sum(), 0.0, 0.0, _d(rew).sum()]
    if q2 is not None:
        e2 = q2 - qt
        out.update(e2=_d(e2), dq2=two * e2 * inv_b)
        out["mag_q"].append(_d(np.abs(q2)) + mag)
        sums[1] = (_d(e2) ** 2).sum()
    if qn is not None:
        out["dqn"] = np.full(B, -inv_b, dtype=dt)
        out["sum_abs_qn"] = float(_d(np.abs(qn)).sum())
        sums[2] = -_d(qn).sum()
    out["sums"], out["sum_abs_rew"] = np.array(sums), float(_d(np.abs(rew)).sum())
    return out


def detac_ratios(got, ref, B):
    out = {}
    crit = [("dq1", "e1", ref["mag_q"][0], 0)] + ([("dq2", "e2", ref["mag_q"][1], 1)] if ref["dq2"] is not None else [])
    _td_ratios(out, got, ref, B, crit)
    out["sum_rew"] = float(abs(got["sums"][3] - ref["sums"][3]) / (4 * U * ref["sum_abs_rew"]))
    if ref["dq2"] is None:
        assert got["dq2"] is None and got["sums"][1] == 0.0
    if ref["dqn"] is None:
        assert got["dqn"] is None and got["sums"][2] == 0.0
    else:
        assert np.all(np.asarray(got["dqn"], dtype=F32).reshape(-1) * F32(B) == -1.0)
        out["sum_qn"] = float(abs(got["sums"][2] - ref["sums"][2]) / (4 * U * ref["sum_abs_qn"]))
    return out


# ------------------------------------------------------------------ exploration noise, Polyak
STREAM_N = (1, 255, 257, 262144 + 5)                                     # the last: more than 1024 blocks of 256 threads
NOISE_ARGS = ((0.3, INF, -INF, INF), (0.2, 0.5, -1.0, 1.0), (0.0, 0.5, -1.0, 1.0))     # sigma, noise_clip, lo, hi
POLYAK_TAU = (0.005, 1.0, 0.0)


def stream_case(n, seed=0):
    rs = np.random.RandomState(n % 1000 + seed)
    return (rs.randn(n) * 1.5).astype(F32), rs.randn(n).astype(F32)


def noisy_action_ref(a, eps, sigma, noise_clip=INF, lo=-INF, hi=INF, dt=F64):
    """clamp(a + clamp(sigma eps, -c, c), lo, hi)   (continuous_policy.py:67-74, td3.py:75-82)"""
    a, eps = np.asarray(a).astype(dt), np.asarray(eps).astype(dt)
    noise = np.clip(dt(sigma) * eps, dt(-noise_clip), dt(noise_clip))
    return np.clip(a + noise, dt(lo), dt(hi))


def polyak_ref(target, source, tau, dt=F64):
    """(1 - tau) target + tau source   (algo/utils.py:16-20), tau the float32 the kernel is handed"""
    target, source, tau = np.asarray(target).astype(dt), np.asarray(source).astype(dt), dt(F32(tau))
    return target * (dt(1) - tau) + source * tau


def polyak_ratio(got, target, source, tau):
    """Three roundings (1 - tau, two products, one sum; contraction removes one): within 3 U (|t| + |s|)."""
    return float(np.max(np.abs(_d(got) - polyak_ref(target, source, tau)) / (3 * U * (np.abs(_d(target)) + np.abs(_d(source))))))


# ------------------------------------------------------------------ DQN (dqn.py:47-60)
DQN_B = (1, 255, 257, 1000)
DQN_A = (1, 2, 6, 18)


def clamp_action(acts, n_a):
    """The stored action as an index in [0, A): int64 clamped; floats NaN -> 0, negative -> 0, a >= A -> A - 1, and a
    fraction truncated (2.7 -> 2)."""
    acts = np.asarray(acts)
    if acts.dtype.kind in "iu":
        return np.clip(acts.astype(np.int64), 0, n_a - 1)
    a = _d(acts)
    a = np.where(np.isnan(a), 0.0, a)
    return np.trunc(np.clip(a, 0.0, float(n_a - 1))).astype(np.int64)


def stored_actions(rs, B, n_a, float_acts):
    """Random actions in range; the first rows hold -1, A, A + 5 and (floats) NaN and 2.7 where the batch has the rows."""
    acts = rs.randint(0, n_a, B)
    acts = acts.astype(F32) if float_acts else acts.astype(np.int64)
    planted = [n_a + 5, -1, n_a] + ([np.nan, 2.7] if float_acts else [])
    for k, val in enumerate(planted[:B]):
        acts[k] = val
    return acts


def dqn_case(B, n_a, float_acts, seed=0):
    rs = np.random.RandomState(100 * B + n_a + seed)
    return dict(q=(rs.randn(B, n_a) * 2).astype(F32), acts=stored_actions(rs, B, n_a, float_acts),
                qn=(rs.randn(B, n_a) * 2).astype(F32), rew=rs.randn(B).astype(F32), term=_terminals(rs, B, "mixed"))


def dqn_td_ref(q, acts, qn, rew, term, gamma, dt=F64):
    """q_s_a = Q(s)[a]; target = r + gamma (1 - d) max_a' Q'(s')[a']; loss = mean((q_s_a - target)^2); dq is
    2 (q_s_a - target) / B at the taken action and zero elsewhere.  sums[3]: loss sum, q_s_a sum, reward sum."""
    q, qn = np.asarray(q).astype(dt), np.asarray(qn).astype(dt)
    rew, term, gamma, one, two = _v(rew, dt), _v(term, dt), dt(gamma), dt(1), dt(2)
    B, n_a = q.shape
    at = clamp_action(acts, n_a)
    mx = qn.max(1)
    qsa = q[np.arange(B), at]
    e = qsa - (rew + gamma * (one - term) * mx)
    dq = np.zeros((B, n_a), dtype=dt)
    dq[np.arange(B), at] = two * e * (one / dt(B))
    return dict(at=at, e=_d(e), dq=dq, sums=np.array([(_d(e) ** 2).sum(), _d(qsa).sum(), _d(rew).sum()]),
                mag=_d(np.abs(qsa)) + _d(np.abs(rew)) + float(gamma) * _d(np.abs(mx)),
                sum_abs_q=float(_d(np.abs(qsa)).sum()), sum_abs_rew=float(_d(np.abs(rew)).sum()))


def dqn_ratios(got, ref, B):
    out = {}
    delta = 8 * U * ref["mag"]
    rows = np.arange(B)
    dq = _d(got["dq"])
    out["dq"] = float(np.max(np.abs(dq[rows, ref["at"]] - _d(ref["dq"])[rows, ref["at"]]) / (delta * 2 / B)))
    off = np.ones(dq.shape, dtype=bool)
    off[rows, ref["at"]] = False
    assert np.all(dq[off] == 0.0)                                        # zero off the chosen column
    out["sum_loss"] = float(abs(got["sums"][0] - ref["sums"][0]) / np.sum(2 * np.abs(ref["e"]) * delta + delta ** 2
                                                                           + 2 * U * ref["e"] ** 2))
    out["sum_q"] = float(abs(got["sums"][1] - ref["sums"][1]) / (4 * U * ref["sum_abs_q"]))
    out["sum_rew"] = float(abs(got["sums"][2] - ref["sums"][2]) / (4 * U * ref["sum_abs_rew"]))
    return out


# ------------------------------------------------------------------ QR-DQN (qrdqn.py:39-60, algo/utils.py:5-13)
QR_CASES = ((1, 1, 1), (3, 3, 5), (70, 6, 8), (5, 2, 51), (4, 6, 200), (2, 3, 257), (2, 2, 260))    # (B, A, Q)
QR_GAMMA = 0.5


def _grid(rs, *shape):
    return (rs.randint(-64, 65, shape) / 16.0).astype(F32)               # multiples of 1/16 in [-4, 4]


def greedy_means(x, n_a, n_q):
    """float64 per-action means of x (N, A * Q), the slack 2 Q U sum_i |x_i| / Q a float32 mean pair can be off by, and
    the top-two gap of every sample (0 where A = 1 has no second)."""
    x = _d(x).reshape(-1, n_a, n_q)
    means = x.mean(2)
    slack = (2 * n_q * U * np.abs(x).sum(2) / n_q).max(1)
    top = np.sort(means, 1)
    gap = top[:, -1] - top[:, -2] if n_a > 1 else np.full(len(x), INF)
    return means, slack, gap


def excluded_samples(x, n_a, n_q):
    """How many samples have a top-two gap that is neither exactly 0 nor above the float32 slack: there the greedy
    action of a float32 mean need not be the float64 one.  The cases are built so that this is 0."""
    _, slack, gap = greedy_means(x, n_a, n_q)
    return int(np.sum((gap != 0.0) & (gap <= slack)))


def qr_case(B, n_a, n_q, float_acts):
    """Next-state quantiles and rewards on a grid of 1/16 and gamma = 1/2: every target T_i is exact in fp32, so is every
    float32 sum over an action's quantiles, and d = T_i - theta_j rounds once, relative to d itself.  Planted: a* ties
    (two identical maximal rows, on two samples of three; actions 0 and 1, or 1 and 2 on odd samples where A >= 3), terminal rows
    (every third, from the second), theta_0 = T_0 (d = 0), theta_1 = T_0 + 1 (d = -1), theta_2 = T_1 - 1 (d = +1)."""
    rs = np.random.RandomState(97 * B + 13 * n_a + n_q + int(float_acts))
    qn = _grid(rs, B, n_a, n_q)
    for b in range(B):
        if n_a >= 2 and b % 3 != 2:
            lo = 1 if (b % 2 == 1 and n_a >= 3) else 0
            qn[b, lo] = np.abs(qn[b, lo]) / 2 + 4                        # in [4, 6]: the largest mean of the sample
            qn[b, lo + 1] = qn[b, lo]
    c = dict(qn=qn.reshape(B, n_a * n_q), rew=_grid(rs, B), term=(np.arange(B) % 3 == 1).astype(F32),
             acts=stored_actions(rs, B, n_a, float_acts))
    at = clamp_action(c["acts"], n_a)
    astar = greedy_means(c["qn"], n_a, n_q)[0].argmax(1)
    T = _d(c["rew"])[:, None] + QR_GAMMA * (1.0 - _d(c["term"]))[:, None] * _d(qn)[np.arange(B), astar]
    q = (rs.randn(B, n_a, n_q) * 1.5).astype(F32)
    for b in range(B):
        plant = [T[b, 0]] if n_q >= 3 else [T[b, 0] + 1.0]               # (one quantile: the lone term sits on |d| = 1)
        if n_q >= 3:
            plant += [T[b, 0] + 1.0, T[b, 1] - 1.0]
        q[b, at[b], :len(plant)] = plant
    c["q"] = q.reshape(B, n_a * n_q)
    return c


def huber(d, dt=F64):
    """d^2 / 2 inside |d| <= 1, |d| - 1/2 outside (algo/utils.py:5-8), and its derivative."""
    ad = np.abs(d)
    return np.where(ad <= dt(1), dt(0.5) * d * d, ad - dt(0.5)), np.clip(d, dt(-1), dt(1))


def quantile_huber_ref(q, acts, qn, rew, term, gamma, n_a, n_q, dt=F64):
    """theta = Q(s)[a]; a* = argmax_a mean_i Q'(s')[a][i] (first maximum); T_i = r + gamma (1 - d) Q'(s')[a*][i];
    diff_ij = T_i - theta_j; loss = mean_{b,i,j} huber(diff) |tau_j - 1[diff < 0]|, tau_j = (2 j + 1) / 2 Q.
    dict(loss_b: per-sample sums over (i, j), dq, sums[3] = loss sum, theta sum, reward sum, and the bounds' terms).
    float32: a column j is accumulated over i in fp32, as a thread does; the a* of float64 is used (see
    `excluded_samples`)."""
    B = np.asarray(q).shape[0]
    q3, n3 = np.asarray(q).astype(dt).reshape(B, n_a, n_q), np.asarray(qn).astype(dt).reshape(B, n_a, n_q)
    rew, term = _v(rew, dt), _v(term, dt)
    at = clamp_action(acts, n_a)
    astar = greedy_means(qn, n_a, n_q)[0].argmax(1)
    rows = np.arange(B)
    T = rew[:, None] + (dt(gamma) * (dt(1) - term))[:, None] * n3[rows, astar]          # (B, i)
    th = q3[rows, at]                                                                    # (B, j)
    tau = ((dt(2) * np.arange(n_q).astype(dt) + dt(1)) / (dt(2) * dt(n_q)))[None, :]
    l, g = np.zeros((B, n_q), dtype=dt), np.zeros((B, n_q), dtype=dt)
    abs_l, sum_w = np.zeros((B, n_q)), np.zeros((B, n_q))
    for i in range(n_q):
        d = T[:, i:i + 1] - th
        w = np.abs(tau - (d < 0).astype(dt))
        h, dh = huber(d, dt)
        l, g = l + h * w, g + dh * w
        abs_l, sum_w = abs_l + _d(h * w), sum_w + _d(w)
    norm = dt(1) / (dt(B) * dt(n_q) * dt(n_q))
    dq = np.zeros((B, n_a, n_q), dtype=dt)
    dq[rows, at] = -g * norm
    loss_b = _d(l).sum(1)
    return dict(at=at, astar=astar, loss_b=loss_b, dq=dq.reshape(B, n_a * n_q), abs_l=abs_l, sum_w=sum_w, T=_d(T), th=_d(th),
                sums=np.array([loss_b.sum(), _d(th).sum(), _d(rew).sum()]), sum_abs_th=float(_d(np.abs(th)).sum()),
                sum_abs_rew=float(_d(np.abs(rew)).sum()))


def qr_ratios(got, ref, B, n_a, n_q):
    """A thread accumulates Q terms in fp32: a column's loss within (Q + 8) U sum_i |term_ij|, its gradient within
    (Q + 8) U sum_i w_ij / (B Q^2); a sample's loss within the sum of its columns' bounds; the three sums in double."""
    k = (n_q + 8) * U
    rows = np.arange(B)
    dq = _d(got["dq"]).reshape(B, n_a, n_q)
    off = np.ones(dq.shape, dtype=bool)
    off[rows, ref["at"]] = False
    assert np.all(dq[off] == 0.0)                                        # zero off the taken action's quantiles
    want = _d(ref["dq"]).reshape(B, n_a, n_q)[rows, ref["at"]]
    out = {"dq": float(np.max(np.abs(dq[rows, ref["at"]] - want) / (k * ref["sum_w"] / (B * n_q * n_q))))}
    bound_b = k * ref["abs_l"].sum(1)
    if bound_b.min() > 0.0:
        out["loss_b"] = float(np.max(np.abs(_d(got["loss_b"]) - ref["loss_b"]) / bound_b))
    else:                                                                # (a sample whose every term is exactly zero)
        assert np.all(_d(got["loss_b"])[bound_b == 0.0] == 0.0)
    out["sum_loss"] = float(abs(got["sums"][0] - ref["sums"][0]) / max(bound_b.sum(), 1e-300))
    out["sum_theta"] = float(abs(got["sums"][1] - ref["sums"][1]) / (4 * U * ref["sum_abs_th"]))
    out["sum_rew"] = float(abs(got["sums"][2] - ref["sums"][2]) / (4 * U * max(ref["sum_abs_rew"], 1e-300)))
    return out


# ------------------------------------------------------------------ epsilon-greedy (discrete_policies.py:40-67)
EPS_CASES = tuple((n, a, 1) for n in (1, 255, 257) for a in DQN_A) + \
    tuple((n, a, nq) for nq in (5, 64, 200) for n in (1, 4, 5) for a in DQN_A)          # (N, A, Q)
EPSILON = 0.25


def eps_case(N, n_a, n_q):
    """Scores on the grid of 1/16 (float32 sums over an action's quantiles are exact; single values tie often); where
    A >= 2 every second env has its two best rows identical (an exact tie, first index wins; 0 and 1, or 1 and 2).
    u: uniform draws, every third exactly epsilon (as float32: the strict u < epsilon keeps the greedy action), the rest
    below or above; rand_act: the action a draw below epsilon selects."""
    rs = np.random.RandomState(11 * N + 5 * n_a + n_q)
    q = _grid(rs, N, n_a, n_q)
    for n in range(0, N, 2):
        if n_a >= 2:
            lo = 1 if (n % 4 == 2 and n_a >= 3) else 0
            q[n, lo] = np.abs(q[n, lo]) / 2 + 4
            q[n, lo + 1] = q[n, lo]
    u = rs.rand(N).astype(F32)
    u[::3] = F32(EPSILON)
    return dict(q=q.reshape(N, n_a * n_q), u=u, rand_act=rs.randint(0, n_a, N).astype(np.int64))


def eps_greedy_ref(q, n_a, n_q, u=None, rand_act=None, epsilon=0.0):
    """argmax_a of the score (Q values, or the mean over quantiles), first maximum; replaced by rand_act where
    u < epsilon (both as the float32 values the kernel is handed)."""
    best = greedy_means(q, n_a, n_q)[0].argmax(1).astype(np.int64)
    if u is None or rand_act is None:
        return best
    return np.where(np.asarray(u, dtype=F32) < F32(epsilon), np.asarray(rand_act, dtype=np.int64), best)


# ------------------------------------------------------------------ the sampler against autograd
RSAMPLE_CASES = tuple((B, A, t) for B in (1, 64, 65, 257) for A in (1, 8) for t in (True, False))


def rsample_case(B, A):
    """head with a moderate std (tanh rarely saturates), noise, and the gradient arriving at the action.  The clamp of
    log_std is hit at both ends where the batch has two rows: head[0, A] = 3 (above 2) and head[1, 2A - 1] = -25 (below
    -20); a batch of one row has the lower end only -- exp(2) times the noise would saturate its only row."""
    rs = np.random.RandomState(4 + B + A)
    head = rs.randn(B, 2 * A).astype(F32)
    head[:, A:] = head[:, A:] * F32(0.5) - F32(1.5)
    eps, d_act = rs.randn(B, A).astype(F32), rs.randn(B, A).astype(F32)
    if B > 1:
        head[0, A], head[1, 2 * A - 1] = 3.0, -25.0
        eps[0, 0] = 0.25                                                   # (a std of e^2: the action stays of order 1)
    else:
        head[0, 2 * A - 1] = -25.0
    return head, eps, d_act
