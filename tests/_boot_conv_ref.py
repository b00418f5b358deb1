"""Restatements for Bootstrapped DQN over conv trunks (TRL_BOOT_CONV=1): the heads' input gradient at the conv feature
(trl_boot_head_dx_f32, include/trl_hip.h) and the whole update in float64 with an explicit chain rule, written from the
formulas of the reference's bootstrapped_dqn.py:73-90 / networks/base.py:59-107 and the header, not from the kernel code.
The dense heads, the TD loss and Adam are those of tests/_boot_dqn_ref.py / _sac_v_ref.py.

`head_dx_ref(case, dt)`: numpy float64 (the reference value, with every element's own sum of |terms|) or numpy float32 (the
same formulas with every operation rounded to fp32: per head one fp32 matrix product, the heads added in ascending k, then
the gate).  tests/test_boot_conv_cpu.py holds the float32 run to `K_HEAD_DX` and recomputes it;
tests/test_boot_conv_kernels_gpu.py holds the kernel (and the three launches it replaces) to the same bound on the same
inputs.

    bound per element = K_HEAD_DX * U * (|act'(y_top)| + t) * sum_k sum_j |dy_k[b][j]| (|act'(y_k[b][j])| + t) |W_k[j][f]|

i.e. relative to the element's own sum of |terms|, where t = TANH_ABS = 1 for Tanh and 0 for ReLU: act' = 1 - y y is a
product and a difference in fp32, rounded by at most U y y and U |1 - y y|, together at most U in ABSOLUTE terms
(y y + |1 - y y| <= 1), so a nearly saturated unit (1 - y y ~ 1e-3 for |y| = 0.9993) carries an error of up to U whatever
its own size -- a gate factor's error is U (|act'| + 1), not U |act'|, and the literal bound is out of reach of any fp32
evaluation there.  For ReLU (act' is exactly 0 or 1) the bound is K_HEAD_DX U sum|terms|.  `mag_plain` is the plain
|act'| sum|terms| (t = 0); the tests print the Tanh cells' ratio under it for information and hold nothing to it.

K_HEAD_DX is NOT fitted to the device: it is the largest err / (U sum|terms|) of the float32 numpy run over every case
below, times the margin 4 of tests/_optim_ref.py (MFMA accumulation order and fused multiply-adds move roundings), rounded up
to a power of two (the float32 run shows 3.59, in the ReLU cases of 70 rows).  An element all of whose terms are zero must be exactly zero."""
import os

import numpy as np

import _boot_dqn_ref as R
from _offpolicy_ref import F32, F64, U                                   # noqa: F401
from _sac_v_ref import Adam, flat, mlp_backward, mlp_forward, state_dict_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ACT_TANH, ACT_RELU, ACT_NONE = 0, 1, 2                                   # TRL_ACT_* of include/trl_hip.h
MARGIN = 4.0
TANH_ABS = 1.0                                                           # absolute roundings of 1 - y y (module docstring)
K_HEAD_DX = 16.0                                                         # 4 x 3.59 rounded up (test_boot_conv_cpu.py recomputes it)

# ------------------------------------------------------------------ trl_boot_head_dx_f32
HEAD_KS, HEAD_BS = (1, 3, 13), (1, 5, 70)                                # 13 heads: past one grouped launch (12)
HEAD_CP = ((16, 4), (16, 49), (64, 49))
HEAD_H1 = (3, 32)                                                        # 3 = A: heads without a hidden layer (dZ = dq)
HEAD_H1_BIG = 512                                                        # with the smallest B only
GATES = ((ACT_RELU, True), (ACT_RELU, False), (ACT_TANH, True), (ACT_TANH, False))       # (activation, gate_like_in)


def head_shapes():
    """(K, B, C, P, H1) of every kernel case; the last one has F = 21, no multiple of 4 (the 4-byte load path)."""
    out = [(k, b, c, p, h) for k in HEAD_KS for b in HEAD_BS for c, p in HEAD_CP for h in HEAD_H1]
    out += [(k, HEAD_BS[0], c, p, HEAD_H1_BIG) for k in HEAD_KS for c, p in HEAD_CP]
    return out + [(3, 5, 3, 7, 32)]


def dact(act, y):
    if act == ACT_TANH:
        return 1.0 - y * y
    if act == ACT_RELU:
        return (y > 0).astype(y.dtype)
    return np.ones_like(y)


_cases = {}


def head_case(K, B, C, P, H1, act):
    """float32 inputs of one case.  dz[k] (B, H1): for H1 = 3 one nonzero per row (dq of a head without a hidden layer,
    no gate), else dense with the activation outputs that gate it; a third of the (b, k) rows masked out (all zero), and
    every fourth sample masked out in EVERY head.  w[k] (H1, C P); y_top: the top conv layer's outputs in the feature's own
    (B, C, P) order (the caller transposes for the other layout)."""
    key = (K, B, C, P, H1, act)
    if key not in _cases:
        rs = np.random.RandomState(1000 * K + 37 * B + 11 * C + 3 * P + H1 + act)
        F = C * P
        dz = rs.randn(K, B, H1).astype(F32)
        if H1 == 3:
            keep = np.zeros((K, B, H1), dtype=bool)
            keep[np.arange(K)[:, None], np.arange(B)[None, :], rs.randint(0, H1, size=(K, B))] = True
            dz = np.where(keep, dz, F32(0))
            gates = None
        else:
            pre = rs.randn(K, B, H1).astype(F32)
            gates = np.maximum(pre, 0) if act == ACT_RELU else np.tanh(pre)
        off = rs.rand(K, B) < 1.0 / 3.0
        off[0, 0] = False                                                # (sample 0 stays live in head 0)
        dz[off] = 0.0
        dz[:, 3::4] = 0.0
        w = (rs.randn(K, H1, F) / np.sqrt(H1)).astype(F32)
        pre = rs.randn(B, C, P).astype(F32)
        y_top = (np.maximum(pre, 0) if act == ACT_RELU else np.tanh(pre)).astype(F32)
        _cases[key] = dict(dz=dz, gates=None if gates is None else gates.astype(F32), w=w, y_top=y_top, act=act,
                           K=K, B=B, C=C, P=P, H1=H1)
    return _cases[key]


def head_dx_ref(c, dt=F64):
    """{out (B, P, C), mag (B, P, C): |act'| sum |terms|} of one case in `dt`."""
    K, B, C, P = c["K"], c["B"], c["C"], c["P"]
    dz = c["dz"].astype(dt)
    if c["gates"] is not None:
        dz = dz * dact(c["act"], c["gates"].astype(dt))
    w = c["w"].astype(dt)
    acc = dz[0] @ w[0]
    for k in range(1, K):
        acc = acc + dz[k] @ w[k]
    g = dact(c["act"], c["y_top"].astype(dt)).reshape(B, C * P)
    out = (acc * g).reshape(B, C, P).transpose(0, 2, 1)
    t = TANH_ABS if c["act"] == ACT_TANH else 0.0
    dy = np.abs(c["dz"].astype(F64))
    dz_abs = dy if c["gates"] is None else dy * (np.abs(dact(c["act"], c["gates"].astype(F64))) + t)
    mag = np.zeros((B, C * P))
    for k in range(K):
        mag += dz_abs[k] @ np.abs(c["w"][k].astype(F64))
    mag = (mag * (np.abs(dact(c["act"], c["y_top"].astype(F64)).reshape(B, C * P)) + t)).reshape(B, C, P).transpose(0, 2, 1)
    plain = np.zeros((B, C * P))
    for k in range(K):
        plain += np.abs(dz[k].astype(F64)) @ np.abs(c["w"][k].astype(F64))
    plain = (plain * np.abs(g.astype(F64))).reshape(B, C, P).transpose(0, 2, 1)
    return dict(out=np.ascontiguousarray(out), mag=np.ascontiguousarray(mag), mag_plain=np.ascontiguousarray(plain))


def head_dx_ratio(got, ref):
    """worst err / (U mag) of a (B, P, C) result against the float64 restatement; elements whose terms are all zero
    (masked out in every head, or gated off) must be exactly zero (asserted here)."""
    got = np.asarray(got, dtype=F64).reshape(ref["out"].shape)
    zero = ref["mag"] == 0
    assert np.all(got[zero] == 0.0)
    if zero.all():
        return 0.0
    err = np.abs(got - ref["out"].astype(F64))
    return float((err[~zero] / (U * ref["mag"][~zero])).max())


def head_dx_plain_ratio(got, ref):
    """For information only: worst err / (U |act'| sum|terms|), the bound without the absolute term of a Tanh gate, over
    the elements where that is not zero."""
    got = np.asarray(got, dtype=F64).reshape(ref["out"].shape)
    live = ref["mag_plain"] > 0
    if not live.any():
        return 0.0
    return float((np.abs(got - ref["out"].astype(F64))[live] / (U * ref["mag_plain"][live])).max())


# ------------------------------------------------------------------ conv trunk in float64 (ReLU, no padding)
def im2col(x, kh, kw, sh, sw):
    """x (B, C, H, W) -> (B, Ho, Wo, C kh kw), the reduction in nn.Conv2d's (c, i, j) order."""
    win = np.lib.stride_tricks.sliding_window_view(x, (kh, kw), axis=(2, 3))[:, :, ::sh, ::sw]     # (B, C, Ho, Wo, kh, kw)
    B, C, Ho, Wo = win.shape[:4]
    return np.ascontiguousarray(win.transpose(0, 2, 3, 1, 4, 5)).reshape(B, Ho, Wo, C * kh * kw)


def conv_forward(convs, x):
    """convs: [(W (Co, Ci, kh, kw), b, (sh, sw))]; ReLU behind every layer.  Returns (feature (B, Co Ho Wo) in nn.Flatten's
    order, tape)."""
    tape, h = [], x
    for w, b, (sh, sw) in convs:
        cols = im2col(h, w.shape[2], w.shape[3], sh, sw)
        y = np.maximum(cols @ w.reshape(w.shape[0], -1).T + b, 0.0)      # (B, Ho, Wo, Co)
        tape.append((h.shape, cols, y))
        h = np.ascontiguousarray(y.transpose(0, 3, 1, 2))
    return h.reshape(h.shape[0], -1), tape


def conv_backward(convs, tape, d_feat):
    """[dW, db, ...] in layer order from the gradient at the flattened feature."""
    grads = []
    B = d_feat.shape[0]
    y_top = tape[-1][2]
    d = d_feat.reshape(B, y_top.shape[3], y_top.shape[1], y_top.shape[2]).transpose(0, 2, 3, 1)   # (B, Ho, Wo, Co)
    for k in range(len(convs) - 1, -1, -1):
        w, _b, (sh, sw) = convs[k]
        in_shape, cols, y = tape[k]
        dz = d * (y > 0.0)
        Co, Ci, kh, kw = w.shape
        dz2 = dz.reshape(-1, Co)
        grads = [(dz2.T @ cols.reshape(-1, cols.shape[-1])).reshape(w.shape), dz2.sum(0)] + grads
        if k == 0:
            break
        dcols = (dz2 @ w.reshape(Co, -1)).reshape(dz.shape[:3] + (Ci, kh, kw))
        dx = np.zeros(in_shape)
        Ho, Wo = dz.shape[1:3]
        for i in range(kh):
            for j in range(kw):
                dx[:, :, i:i + sh * Ho:sh, j:j + sw * Wo:sw] += dcols[:, :, :, :, i, j].transpose(0, 3, 1, 2)
        d = dx.transpose(0, 2, 3, 1)
    return grads


class RMSprop:
    """torch.optim.RMSprop without momentum / centering, in place on a flat list of arrays."""

    def __init__(self, params, lr, alpha, eps):
        self.lr, self.alpha, self.eps = lr, alpha, eps
        self.sq = [np.zeros_like(p) for p in params]

    def step(self, params, grads):
        for p, g, sq in zip(params, grads, self.sq):
            sq *= self.alpha
            sq += (1.0 - self.alpha) * g * g
            p -= self.lr * g / (np.sqrt(sq) + self.eps)


# ------------------------------------------------------------------ the whole update in float64
CASES = ("lin", "hid", "rms")
BATCH_KEYS = R.BATCH_KEYS
STRIDES = ((4, 4), (2, 2), (1, 1))                                       # of the fixture's conv stack


def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, "boot_dqn_conv_update.npz"), allow_pickle=False))


def frames_to_float(u8):
    """What the reference is fed: ScaledFloatFrame's u8 / 255 - 0.5."""
    return np.asarray(u8).astype(F64) / 255.0 - 0.5


def net_of(g, prefix, K):
    """(convs [(W, b, stride)], heads [[(W, b)] per head]) float64 of one stored BootstrappedNet over a CNNBase."""
    sd = state_dict_of(g, prefix)
    pairs = lambda pre: [(sd[k].astype(F64), sd[k[:-6] + "bias"].astype(F64))
                         for k in sorted((k for k in sd if k.startswith(pre) and k.endswith(".weight")),
                                         key=lambda s: int(s.split(".")[-2]))]
    convs = [(w, b, s) for (w, b), s in zip(pairs("base."), STRIDES)]
    return convs, [pairs("head%d." % k) for k in range(K)]


def params_of(net):
    return [t for w, b, _ in net[0] for t in (w, b)] + [t for h in net[1] for t in flat(h)]


def q_all(net, frames):
    """(K, B, A) Q values of every head on float frames, the conv tape, the feature and the heads' tapes."""
    convs, heads = net
    feat, ctape = conv_forward(convs, frames)
    outs, tapes = [], []
    for h in heads:
        y, tape = mlp_forward(h, feat)
        outs.append(y)
        tapes.append(tape)
    return np.stack(outs), ctape, feat, tapes


class Update:
    """BootstrappedDQN.update (bootstrapped_dqn.py:56-104) over a conv trunk in float64: one optimiser over trunk and heads
    in module order, then the soft (Polyak) or hard (every `period` updates) target update of DQN."""

    def __init__(self, net, tnet, qlr, opt=("adam",), discount=0.99, tau=0.005, soft=True, period=1):
        self.net, self.tnet = net, tnet
        self.discount, self.tau, self.soft, self.period = discount, tau, soft, period
        self.params, self.tparams = params_of(net), params_of(tnet)
        self.opt = Adam(self.params, qlr) if opt[0] == "adam" else RMSprop(self.params, qlr, opt[1], opt[2])
        self.count = 0

    def state(self):
        """{torch's state name: flat list of arrays in parameter order}."""
        if isinstance(self.opt, Adam):
            return {"exp_avg": self.opt.m, "exp_avg_sq": self.opt.v}
        return {"square_avg": self.opt.sq}

    def update(self, batch):
        self.count += 1
        b = {k: np.asarray(batch[k], dtype=F64) for k in BATCH_KEYS if k not in ("obs", "next_obs")}
        convs, heads = self.net
        K = len(heads)
        q, ctape, feat, tapes = q_all(self.net, frames_to_float(batch["obs"]))
        qn = q_all(self.tnet, frames_to_float(batch["next_obs"]))[0]
        B = q.shape[1]
        td = R.boot_td_ref(q, qn, b["acts"].reshape(-1), b["rewards"], b["terminals"], b["masks"], self.discount)
        g_heads, d_feat = [], np.zeros_like(feat)
        for k in range(K):
            grads, dx = mlp_backward(heads[k], tapes[k], td["dq"][k])
            g_heads += grads
            d_feat = d_feat + dx
        self.last_d_feat = d_feat
        g_all = conv_backward(convs, ctape, d_feat) + g_heads
        self.last_grads = [g.copy() for g in g_all]
        self.opt.step(self.params, g_all)
        if self.soft:
            for t, p in zip(self.tparams, self.params):
                t *= 1.0 - self.tau
                t += self.tau * p
        elif self.count % self.period == 0:
            for t, p in zip(self.tparams, self.params):
                t[...] = p
        return {"Reward_Mean": td["sums"][2] / B, "Training/qf_loss": td["sums"][0] / B}


def case_args(g, tag):
    """dict of a stored case's settings."""
    a = g[tag + "_args"]
    out = dict(K=int(a[0]), B=int(a[1]), soft=bool(a[2]), period=int(a[3]), steps=int(a[4]), qlr=float(a[5]), tau=float(a[6]),
               append=[int(v) for v in g[tag + "_append"]])
    o = g[tag + "_opt"]
    out["opt"] = ("adam",) if int(o[0]) == 0 else ("rmsprop", float(o[1]), float(o[2]))
    return out


def batch_of(g, s):
    return {k: g[f"batch_s{s}_{k}"] for k in BATCH_KEYS}


def update_from_fixture(g, tag):
    """(Update on the stored initial network -- the target starts as its copy --, settings)."""
    a = case_args(g, tag)
    up = Update(net_of(g, tag + "_qf0_", a["K"]), net_of(g, tag + "_qf0_", a["K"]), a["qlr"], opt=a["opt"], tau=a["tau"],
                soft=a["soft"], period=a["period"])
    return up, a
