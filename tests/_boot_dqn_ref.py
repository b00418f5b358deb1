"""Restatements for Bootstrapped DQN (torchrl_amd/csrc/k_bootdqn.hip, algo/off_policy/bootstrapped_dqn.py), written from
the formulas of the reference's bootstrapped_dqn.py:73-90 and discrete_policies.py:92-121 and from the definitions in
include/trl_hip.h, not from the kernel code.

Kernel-level restatements take `dt`: numpy float64 (the reference value) or numpy float32 (the same formulas with every
operation rounded to fp32; sums accumulated in double over fp32 terms, as the kernels do).  tests/test_boot_dqn_cpu.py
holds the float32 run to the bounds below and tests/test_boot_dqn_kernels_gpu.py holds the kernels to the same bounds on
the same inputs.  The draws go through oracle.philox.  `Update` is the whole update in float64 with an explicit chain
rule (dense nets by hand, Adam and the target update of tests/_sac_v_ref.py)."""
import os

import numpy as np

from _offpolicy_ref import F32, F64, U, _d, _grid, _terminals, _v, clamp_action, stored_actions      # noqa: F401
from _sac_v_ref import Adam, flat, mlp_backward, mlp_forward, state_dict_of
from oracle import philox

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAG_HEAD, TAG_MASK = 0x42484541, 0x424D534B                              # trl_philox.h: "BHEA", "BMSK"
POLICY_SEED = 0xB007D                                                    # BootstrappedDQNDiscretePolicy.seed
CASES = ("lin", "hid", "hard")
BATCH_KEYS = ("obs", "next_obs", "acts", "rewards", "terminals", "masks")

ACT_N = (1, 255, 257, 1000)
KA = ((1, 1), (2, 2), (10, 6), (33, 18))                                 # (K, A); (64, 64) runs at one size only
KA_BIG, N_BIG = (64, 64), 257
TD_CAP = (4096, 33, 6)                                                   # (B, K, A): K B = 135 168 items, beyond 256 workgroups x 256


def ka_cases(sizes):
    return [(n, k, a) for n in sizes for k, a in KA] + [(N_BIG,) + KA_BIG]


# ------------------------------------------------------------------ the draws
def boot_words(seed, counter, g, tag):
    """The Philox word of (seed, counter, flat index g): element g & 3 of block g >> 2, counter words
    (lo32(counter), hi32(counter), block, tag), key (lo32(seed), hi32(seed))."""
    g = np.asarray(g, dtype=np.int64)
    ctr = np.stack([np.full_like(g, int(counter) & 0xFFFFFFFF), np.full_like(g, (int(counter) >> 32) & 0xFFFFFFFF),
                    (g >> 2) & 0xFFFFFFFF, np.full_like(g, tag)], axis=-1).astype(np.uint32)
    key = np.stack([np.full_like(g, int(seed) & 0xFFFFFFFF), np.full_like(g, (int(seed) >> 32) & 0xFFFFFFFF)],
                   axis=-1).astype(np.uint32)
    x = philox.philox4x32_10(ctr, key)
    return x[np.arange(g.size), (g & 3).astype(np.int64)] if g.ndim else x[int(g) & 3]


def heads_ref(head, K, seed, counter, env_offset=0, reset_mask=None):
    """head (N,) int64 after the draw: (uint64(x) K) >> 32 where the mask is set (everywhere when None)."""
    head = np.asarray(head, dtype=np.int64).copy()
    x = boot_words(seed, counter, env_offset + np.arange(head.size), TAG_HEAD).astype(np.uint64)
    new = ((x * np.uint64(K)) >> np.uint64(32)).astype(np.int64)
    sel = np.ones(head.size, dtype=bool) if reset_mask is None else np.asarray(reset_mask).reshape(-1) != 0
    head[sel] = new[sel]
    return head


def masks_ref(N, K, p, seed, counter, env_offset=0):
    """(N, K) float32: 1 where the uniform of flat index (env_offset + n) K + k lies below p (both as float32)."""
    i = (env_offset + np.arange(N, dtype=np.int64))[:, None] * K + np.arange(K, dtype=np.int64)[None, :]
    u = philox.u32_to_unit(boot_words(seed, counter, i.reshape(-1), TAG_MASK)).reshape(N, K)
    return (u < F32(p)).astype(F32)


# ------------------------------------------------------------------ actions
def act_case(N, K, A):
    """Q on the grid of 1/16 in [-4, 4] (fp32 sums over K <= 64 heads are exact).  Planted: inside every head of every
    second env the two best actions tie exactly (0 and 1, or 1 and 2); on every fourth env the ensemble SUMS of two
    actions tie while no single head does; heads -1, K and K + 5 on the first envs."""
    rs = np.random.RandomState(7 * N + 3 * K + A)
    q = _grid(rs, K, N, A)
    for n in range(0, N, 2):
        if A >= 2:
            lo = 1 if (n % 4 == 2 and A >= 3) else 0
            q[:, n, lo] = np.abs(q[:, n, lo]) / 2 + 4
            q[:, n, lo + 1] = q[:, n, lo]
    for n in range(1, N, 4):
        if A >= 2 and K >= 2:                                            # equal sums from different addends
            q[:, n, :] = -4.0
            q[0, n, A - 1], q[1, n, A - 1] = 1.0, 3.0
            q[0, n, A - 2], q[1, n, A - 2] = 3.0, 1.0
    head = rs.randint(0, K, N).astype(np.int64)
    for k, v in enumerate([-1, K, K + 5][:N]):
        head[k] = v
    return q, head


def boot_act_ref(q, head=None):
    """(action (N,), q_sel (N, A) float64, onehot (N, A)): arg-max under each env's (clamped) head, or of the ensemble
    vote sum_k q[k] (the sums are compared; q_sel is then the sum / K).  First maximum."""
    q = _d(q)
    K, N, A = q.shape
    if head is None:
        score = q.sum(0)
        q_sel = score / K
    else:
        h = np.clip(np.asarray(head, dtype=np.int64), 0, K - 1)
        score = q[h, np.arange(N)]
        q_sel = score
    act = score.argmax(1).astype(np.int64)
    onehot = np.zeros((N, A), dtype=F32)
    onehot[np.arange(N), act] = 1.0
    return act, q_sel, onehot


# ------------------------------------------------------------------ TD loss over K heads
GAMMA = 0.99


def td_case(B, K, A, float_acts, seed=0):
    """Random Q stacks, actions with the planted out-of-range values of `stored_actions`, mixed terminals, Bernoulli(0.5)
    masks with one all-zero column (the last head) and one all-zero row (the last sample) where the shape has room."""
    rs = np.random.RandomState(100 * B + 7 * K + A + seed)
    c = dict(q=(rs.randn(K, B, A) * 2).astype(F32), qn=(rs.randn(K, B, A) * 2).astype(F32),
             acts=stored_actions(rs, B, A, float_acts), rew=rs.randn(B).astype(F32), term=_terminals(rs, B, "mixed"),
             masks=(rs.rand(B, K) < 0.5).astype(F32))
    if K > 1:
        c["masks"][:, K - 1] = 0.0
    if B > 1:
        c["masks"][B - 1, :] = 0.0
    return c


def boot_td_ref(q, qn, acts, rew, term, masks, gamma, dt=F64):
    """e[k, b] = q[k, b, a_b] - (r_b + gamma (1 - d_b) max_a' qn[k, b, a']); dq = 2 masks[b, k] e / (K B) at the taken action,
    zero elsewhere; sums = (sum_b sum_k masks e^2 / K, sum masks, sum_b r_b)."""
    q, qn = np.asarray(q).astype(dt), np.asarray(qn).astype(dt)
    K, B, A = q.shape
    rew, term, gamma, one, two = _v(rew, dt), _v(term, dt), dt(gamma), dt(1), dt(2)
    m = np.asarray(masks).astype(dt).T                                   # (K, B)
    at = clamp_action(acts, A)
    rows = np.arange(B)
    mx = qn.max(2)
    qsa = q[:, rows, at]
    e = qsa - (rew[None, :] + (gamma * (one - term))[None, :] * mx)
    scale = two / (dt(K) * dt(B))
    dq = np.zeros((K, B, A), dtype=dt)
    dq[:, rows, at] = np.where(m != 0, scale * m * e, dt(0))
    sums = np.array([(_d(m) * _d(e) ** 2).sum() / K, _d(m).sum(), _d(rew).sum()])
    mag = _d(np.abs(qsa)) + _d(np.abs(rew))[None, :] + float(gamma) * _d(np.abs(mx))
    return dict(at=at, e=_d(e), m=_d(m), dq=dq, sums=sums, mag=mag, sum_abs_rew=float(_d(np.abs(rew)).sum()))


def boot_td_ratios(got, ref, K, B):
    """{name: worst err / bound} of a trl_boot_td_loss_f32 result against the float64 restatement, in units of U = 2^-24.

    e is three fp32 operations on values of size mag = |q_s_a| + |r| + gamma |max q'| (1 - d exact for d in {0, 1}; a
    product, a sum or an fma, a difference): |de| <= 3 U mag; `dqn_ratios` allows delta = 8 U mag for the same chain and
    so does this.  dq = (2 / (K B)) m e adds the rounding of the scale and of one product (m is 0 or 1): 2 U relative,
    inside the same delta -> |d dq| <= delta 2 / (K B).  The loss sum adds m e^2 exactly converted terms in double:
    sum m (2 |e| delta + delta^2 + 2 U e^2) / K.  The reward sum is exact conversions added in double: 4 U sum |r| as
    in `dqn_ratios`; the mask sum is a sum of 0s and 1s in double: exact.  Off the taken action and where the mask is 0
    dq is exactly 0 (asserted here)."""
    out = {}
    delta = 8 * U * ref["mag"]                                           # (K, B)
    rows = np.arange(B)
    dq = _d(got["dq"])
    off = np.ones(dq.shape, dtype=bool)
    off[:, rows, ref["at"]] = False
    assert np.all(dq[off] == 0.0)
    taken = dq[:, rows, ref["at"]]
    assert np.all(taken[ref["m"] == 0] == 0.0)
    live = ref["m"] != 0
    if live.any():
        want = _d(ref["dq"])[:, rows, ref["at"]]
        out["dq"] = float(np.max((np.abs(taken - want) / (delta * 2 / (K * B)))[live]))
    bound = np.sum(ref["m"] * (2 * np.abs(ref["e"]) * delta + delta ** 2 + 2 * U * ref["e"] ** 2)) / K
    if bound > 0:
        out["sum_loss"] = float(abs(got["sums"][0] - ref["sums"][0]) / bound)
    else:
        assert got["sums"][0] == 0.0
    assert got["sums"][1] == ref["sums"][1]
    out["sum_rew"] = float(abs(got["sums"][2] - ref["sums"][2]) / (4 * U * max(ref["sum_abs_rew"], 1e-300)))
    return out


def fold_ref(x, dt=F64):
    """Sum over the leading axis in ascending k."""
    x = np.asarray(x).astype(dt)
    s = x[0].copy()
    for k in range(1, x.shape[0]):
        s = s + x[k]
    return s


# ------------------------------------------------------------------ the whole update in float64
def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, "boot_dqn_update.npz"), allow_pickle=False))


def net_of(g, prefix, K):
    """(trunk [(W, b)], heads [[(W, b)] per head]) float64 of one stored BootstrappedNet."""
    sd = state_dict_of(g, prefix)
    pairs = lambda pre: [(sd[k].astype(F64), sd[k[:-6] + "bias"].astype(F64))
                         for k in sorted((k for k in sd if k.startswith(pre) and k.endswith(".weight")),
                                         key=lambda s: int(s.split(".")[-2]))]
    return pairs("base."), [pairs("head%d." % k) for k in range(K)]


def q_all(net, x):
    """(K, B, A) Q values of every head, and the tapes."""
    trunk, heads = net
    outs, tapes = [], []
    for h in heads:
        y, tape = mlp_forward(trunk + h, x)
        outs.append(y)
        tapes.append(tape)
    return np.stack(outs), tapes


class Update:
    """BootstrappedDQN.update (bootstrapped_dqn.py:56-104) in float64: one Adam over trunk and heads in module order, then
    the soft (Polyak) or hard (every `period` updates) target update of DQN."""

    def __init__(self, net, tnet, qlr, discount=0.99, tau=0.005, soft=True, period=1):
        self.net, self.tnet = net, tnet
        self.discount, self.tau, self.soft, self.period = discount, tau, soft, period
        self.params = flat(net[0]) + [t for h in net[1] for t in flat(h)]
        self.tparams = flat(tnet[0]) + [t for h in tnet[1] for t in flat(h)]
        self.opt = Adam(self.params, qlr)
        self.count = 0

    def update(self, batch):
        self.count += 1
        b = {k: np.asarray(batch[k], dtype=F64) for k in BATCH_KEYS}
        trunk, heads = self.net
        K, nt = len(heads), len(trunk)
        q, tapes = q_all(self.net, b["obs"])
        qn, _ = q_all(self.tnet, b["next_obs"])
        B = q.shape[1]
        td = boot_td_ref(q, qn, b["acts"].reshape(-1), b["rewards"], b["terminals"], b["masks"], self.discount)
        g_trunk, g_heads = None, []
        for k in range(K):
            grads, _ = mlp_backward(trunk + heads[k], tapes[k], td["dq"][k])
            g_trunk = grads[:2 * nt] if g_trunk is None else [a + c for a, c in zip(g_trunk, grads[:2 * nt])]
            g_heads += grads[2 * nt:]
        self.last_grads = [g.copy() for g in g_trunk + g_heads]           # (module order, as `params`)
        self.opt.step(self.params, g_trunk + g_heads)
        if self.soft:
            for t, p in zip(self.tparams, self.params):
                t *= 1.0 - self.tau
                t += self.tau * p
        elif self.count % self.period == 0:
            for t, p in zip(self.tparams, self.params):
                t[...] = p
        return {"Reward_Mean": td["sums"][2] / B, "Training/qf_loss": td["sums"][0] / B}


def update_from_fixture(g, tag):
    """(Update on the stored initial networks, K, number of stored updates)."""
    K, B, soft, period, steps = (int(v) for v in g[tag + "_args"][:5])
    qlr, tau = float(g[tag + "_args"][5]), float(g[tag + "_args"][6])
    up = Update(net_of(g, tag + "_qf0_", K), net_of(g, tag + "_tqf0_", K), qlr, tau=tau, soft=bool(soft), period=period)
    return up, K, steps
