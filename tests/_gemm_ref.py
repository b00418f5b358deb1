"""Float64 restatement of the dense-layer GEMM family (torchrl_amd/csrc/k_gemm.hip) with a per-element error bound, the
input builders and the case table shared by tests/test_gemm_ref_cpu.py and tests/test_gemm_routes_gpu.py.  Plain torch;
nothing is imported from torchrl_amd.

    forward      Y  = act(X W^T + b)               X (M, K), W (N, K), b (N)
    input grad   dX = dZ W                          dZ = dY * act'(Y), act' taken through the layer OUTPUT as the kernels do
    weight grad  dW = dZ^T X,  db = column sums of dZ                      (tanh: 1 - y^2, relu: y > 0, none: 1)

The bound follows tests/_rollout_ref.py: an fp32 sum of L products, in ANY order (so split and folded routes need no other
bound), is within (L + 2) U S of the exact value, U = 2^-24 and S the float64 sum of the terms' magnitudes, |bias| included.
A gated operand is rounded before it enters the sum: two more units on L.  (tanh gate: y y and 1 - y^2 are each rounded,
d = 1 - y^2 is off by at most U (y^2 + d), which is <= 2 U d as long as y^2 <= 1/2 -- `inputs` keeps tanh gates at
|y| <= 0.7 -- and the product dy d adds one more; the three fit the two units plus the spare one of L + 2, since a chain of
L fused steps and a bias rounds L + 1 times.  relu gate: the factor is exactly 0 or 1.)  A tanh epilogue adds trl_tanh's
2e-7 absolute (its slope is <= 1, so the pre-activation's error passes through unamplified); relu's slope is <= 1 too and
it adds nothing.
The relu gate is discontinuous at 0: gate tensors keep |y| >= 1e-3 apart from exact zeros (+0 and -0) planted to pin the
kernel's rule y > 0."""
import collections
import functools

import torch

U = 2.0 ** -24
TANH_ERR = 2e-7                       # trl_tanh's absolute error, as tests/_rollout_ref.py states it
ACTS = ("none", "relu", "tanh")


def _f64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def act_fn(z, act):
    return torch.tanh(z) if act == "tanh" else torch.relu(z) if act == "relu" else z


def dact_from_out(y, act):
    if act == "tanh":
        return 1.0 - y * y
    if act == "relu":
        return (y > 0).to(y.dtype)
    return torch.ones_like(y)


def fwd(x, w, b, act):
    """-> (y, bound), float64."""
    x, w, b = _f64(x), _f64(w), _f64(b)
    K = x.shape[1]
    z, S = x @ w.t(), x.abs() @ w.abs().t()
    if b is not None:
        z, S = z + b, S + b.abs()
    return act_fn(z, act), (K + 2) * U * S + (TANH_ERR if act == "tanh" else 0.0)


def _dz(dy, y, act):
    dy = _f64(dy)
    if act == "none" or y is None:
        return dy, 0
    return dy * dact_from_out(_f64(y), act), 2


def bwd_input(dy, y, act, w):
    """-> (dx, bound), float64."""
    dz, extra = _dz(dy, y, act)
    w = _f64(w)
    return dz @ w, (dz.shape[1] + extra + 2) * U * (dz.abs() @ w.abs())


def bwd_weight(dy, y, act, x):
    """-> (dw, db, bound_dw, bound_db), float64."""
    dz, extra = _dz(dy, y, act)
    x = _f64(x)
    L = dz.shape[0] + extra + 2
    return dz.t() @ x, dz.sum(0), L * U * (dz.abs().t() @ x.abs()), L * U * dz.abs().sum(0)


# ---- inputs ----
def _plant(t):
    """100 x larger values where a dropped, doubled or across-the-edge term would come from: the last row, the last column
    and the first index after every multiple of 32 (every panel depth, tile side and split granule is one), on both axes --
    at the crossings only, so that most outputs keep a bound of the unplanted size."""
    r = torch.arange(t.shape[0])
    c = torch.arange(t.shape[1])
    rm = (r % 32 == 0) | (r == t.shape[0] - 1)
    cm = (c % 32 == 0) | (c == t.shape[1] - 1)
    t[rm[:, None] & cm[None, :]] *= 100.0
    return t


def inputs(seed, M, K, N, act, planted=False):
    """Seeded fp32 Gaussian x (M, K), w (N, K) / sqrt(K), b (N), dy (M, N) and a gate tensor y (M, N) for `act` (None for
    "none"): independent of the forward, so the backward kernels are tested on their own inputs."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=gen)
    w = torch.randn(N, K, generator=gen) / K ** 0.5
    b = torch.randn(N, generator=gen)
    dy = torch.randn(M, N, generator=gen)
    g = torch.randn(M, N, generator=gen)
    if planted:
        x, w, dy = _plant(x), _plant(w), _plant(dy)
        b[-1] *= 100.0
    y = None
    if act == "tanh":
        y = 0.7 * torch.tanh(g)
    elif act == "relu":
        y = torch.where(g >= 0, g + 1e-3, g - 1e-3)
        y[0, 0], y[-1, -1], y[M // 2, N // 2] = 0.0, -0.0, 0.0
    return dict(x=x, w=w, b=b, dy=dy, y=y)


# ---- fp32 evaluations on the CPU: a correct fp32 implementation meets the bound ----
def fwd_f32(x, w, b, act, split_len=0):
    return act_fn(_sum_f32(x, w.t(), split_len) + b, act)


def bwd_input_f32(dy, y, act, w, split_len=0):
    dz = dy if y is None else dy * dact_from_out(y, act)
    return _sum_f32(dz, w, split_len)


def bwd_weight_f32(dy, y, act, x, split_len=0):
    dz = dy if y is None else dy * dact_from_out(y, act)
    if not split_len:
        return dz.t() @ x, dz.sum(0)
    db = torch.zeros(dz.shape[1])
    for lo in range(0, dz.shape[0], split_len):
        db = db + dz[lo:lo + split_len].sum(0)
    return _sum_f32(dz.t(), x, split_len), db


def _sum_f32(a, b, split_len):
    """a @ b in float32; split_len > 0: slices of the reduction multiplied on their own, partials folded in order."""
    if not split_len:
        return a @ b
    out = torch.zeros(a.shape[0], b.shape[1])
    for lo in range(0, a.shape[1], split_len):
        out = out + a[:, lo:lo + split_len] @ b[lo:lo + split_len]
    return out


# ---- the case table ----
# op: the entry point (a route-query op); G problems of (M, K, N); acts: epilogue / gate activations to run; route: the
# fields of the route query the case is there for (asserted, never assumed).
Case = collections.namedtuple("Case", "id op G M K N acts route")


def _c(id, op, G, M, K, N, acts=ACTS, **route):
    return Case(id, op, G, M, K, N, acts, route)


T64 = dict(tile_m=64, tile_n=64, panel=64, splits=1)
CASES = [
    # tile shapes on the 64-deep panel, single launches
    _c("t64", "fwd", 1, 130, 200, 70, **T64),
    _c("t64", "bwd_input", 1, 130, 70, 200, **T64),                       # dx (130, 70) behind a 200-long reduction
    _c("t64", "bwd_weight", 1, 200, 70, 130, **T64),                      # dw (130, 70), batch 200
    _c("t128x32", "fwd", 1, 300, 132, 32, tile_m=128, tile_n=32, panel=64, splits=1),
    _c("t128x32", "bwd_input", 1, 300, 32, 132, tile_m=128, tile_n=32, panel=64, splits=1),
    _c("t128x32", "bwd_weight", 1, 132, 32, 300, tile_m=128, tile_n=32, panel=64, splits=1),
    _c("t128x1", "fwd", 1, 129, 64, 1, tile_m=128, tile_n=32, panel=64, splits=1),
    _c("t128x1", "bwd_input", 1, 129, 1, 64, tile_m=128, tile_n=32, panel=64, splits=1),
    _c("t128x1", "bwd_weight", 1, 64, 1, 129, tile_m=128, tile_n=32, panel=64, splits=1),
    _c("t32x128", "fwd", 1, 32, 260, 130, tile_m=32, tile_n=128, panel=64, splits=1),
    _c("t32x128", "bwd_input", 1, 32, 130, 260, tile_m=32, tile_n=128, panel=64, splits=1),
    _c("t32x128", "bwd_weight", 1, 200, 130, 32, tile_m=32, tile_n=128, panel=64, splits=1),
    _c("t1x3", "fwd", 1, 1, 5, 3, tile_m=128, tile_n=32, panel=64, splits=1),       # N <= 32 wins over M <= 32
    _c("t1x3", "bwd_input", 1, 1, 5, 3, tile_m=128, tile_n=32, panel=64, splits=1),
    _c("t1x3", "bwd_weight", 1, 1, 5, 3, tile_m=128, tile_n=32, panel=64, splits=1),
    _c("t1x40", "fwd", 1, 1, 5, 40, tile_m=32, tile_n=128, panel=64, splits=1),
    # the 128 x 128 tile (32-deep panel, 2 x 2 blocks per wave)
    _c("t128_fwd", "fwd_splitk", 2, 130, 1100, 132, ("relu", "tanh"), tile_m=128, tile_n=128, panel=32, splits=5, split_len=256),
    _c("t128_bwd_input", "bwd_input", 12, 1200, 1160, 40, ("tanh",), tile_m=128, tile_n=128, panel=32, splits=1),
    _c("t128_bwd_weight", "bwd_weight", 12, 70, 1160, 1200, ("relu",), tile_m=128, tile_n=128, panel=32, splits=1),
    # the 32-deep panel on the 64 x 64 tile, alone
    _c("kp32", "fwd", 1, 2048, 72, 1536, ("tanh",), tile_m=64, tile_n=64, panel=32, splits=1),
    _c("kp32", "bwd_input", 1, 2048, 1536, 72, ("relu",), tile_m=64, tile_n=64, panel=32, splits=1),
    # split boundaries (found with the query; the comments give the selector's arithmetic)
    # forward, 4 tiles (<= 16): splits from K = 4 * 128 on; 511 stays whole
    _c("fsplit_lo", "fwd_splitk", 1, 100, 511, 70, ("tanh",), **T64),
    _c("fsplit_at", "fwd_splitk", 1, 100, 512, 70, ("tanh",), tile_m=64, tile_n=64, panel=64, splits=4, split_len=128, fold_waves=4),
    _c("fsplit_tail1", "fwd_splitk", 1, 100, 513, 70, ("relu",), tile_m=64, tile_n=64, panel=64, splits=5, split_len=128),
    # input gradient, 4 tiles (< 128): splits from N = 8 * 128 on
    _c("isplit_lo", "bwd_input_splitk", 1, 100, 70, 1023, ("tanh",), **T64),
    _c("isplit_at", "bwd_input_splitk", 1, 100, 70, 1024, ("tanh",), tile_m=64, tile_n=64, panel=64, splits=8, split_len=128, fold_waves=4),
    _c("isplit_tail1", "bwd_input_splitk", 1, 100, 70, 1025, ("relu",), tile_m=64, tile_n=64, panel=64, splits=5, split_len=256),
    # weight gradient: slices of 256 batch rows; two, two with a one-row tail, and 32 (the 16-wave fold) with a one-row tail
    _c("wsplit_2", "bwd_weight", 1, 512, 70, 130, ("tanh",), tile_m=64, tile_n=64, panel=64, splits=2, split_len=256, fold_waves=4),
    _c("wsplit_tail1", "bwd_weight", 1, 257, 70, 130, ("relu",), tile_m=64, tile_n=64, panel=64, splits=2, split_len=256, fold_waves=4),
    _c("wsplit_fold16", "bwd_weight", 1, 7937, 64, 64, ("tanh",), tile_m=64, tile_n=64, panel=64, splits=32, split_len=256, fold_waves=16),
]

# loader hand-over: interior tiles only (M, N multiples of the tile).  The reduction takes KP, KP + 1, 2 KP + 4, 3 KP + 63
# and KP - 1: the fast loop runs 1, 1, 2, 3 or 0 whole panels before the general loop's tail.  In the forward the reduction
# is the operands' leading dimension, so only lengths that are multiples of 4 keep the 16-byte loads (the others test the
# all-edge path); in the weight gradient it is the row index and every length hands over.
def _handover(kp):
    red = [kp, kp + 1, 2 * kp + 4, 3 * kp + 63, kp - 1]
    m, n = (128, 128) if kp == 64 else (2048, 1536)                        # kp 32: >= 768 workgroups of 64 x 64
    route = dict(tile_m=64, tile_n=64, panel=kp, splits=1)
    out = []
    for r in red:
        out.append(_c("handover%d_k%d" % (kp, r), "fwd", 1, m, r, n, ("none",), **route))
        out.append(_c("handover%d_k%d" % (kp, r), "bwd_weight", 1, r, n, m, ("tanh",), **route))
    return out


HANDOVER = _handover(64) + _handover(32)

# pointer misalignment: the 64 x 64 interior shape, every operand in turn 1 and 3 floats into a larger buffer
MISALIGNED = _c("misaligned", "fwd", 1, 128, 132, 128, ("none",), **T64)

# mixed-shape weight gradients (FoldPlan(defer_gemm=True)): (K, N, gated) per layer, one activation per launch
SKINNY_SETS = [(1, 64, True), (31, 256, False), (64, 1, True), (256, 31, False), (256, 32, True), (64, 32, False),
               (31, 64, True), (256, 1, False)]
SKINNY_BATCHES = (300, 50)            # 300: slices of 128, the last 44 rows (two 16-row rounds and a tail); 50: under one slice
# one non-skinny member (the hetero GEMM): at M = 1000 the grid is 10 tiles x 8 slices; (520, 40) has 9 tiles and 4 slices
HETERO_SET = [(17, 256, True), (600, 40, True), (520, 40, True)]
HETERO_BATCH = 1000


def case_seed(case, g=0):
    return 1000003 * (case.M * 31 + case.K * 17 + case.N) % (2 ** 31) + 101 * g + len(case.op)


def reference(case, act, planted, g=0):
    """(inputs, outputs) of problem g of a case: outputs maps a name to (float64 value, bound).  Computed once, shared."""
    return _reference(case.op.replace("_splitk", ""), case_seed(case, g), case.M, case.K, case.N, act, planted)


@functools.lru_cache(maxsize=None)
def _reference(op, seed, M, K, N, act, planted):
    inp = inputs(seed, M, K, N, act, planted)
    if op == "fwd":
        y, by = fwd(inp["x"], inp["w"], inp["b"], act)
        out = dict(y=(y, by))
    elif op == "bwd_input":
        dx, bx = bwd_input(inp["dy"], inp["y"], act, inp["w"])
        out = dict(dx=(dx, bx))
    else:
        dw, db, bw, bb = bwd_weight(inp["dy"], inp["y"], act, inp["x"])
        out = dict(dw=(dw, bw), db=(db, bb))
    return inp, out


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements (a zero bound admits only an exact match)."""
    err = (_f64(got) - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(ratio.max()) if ratio.numel() else 0.0
