"""The dense-layer GEMM family (torchrl_amd/csrc/k_gemm.hip) against the float64 restatement of tests/_gemm_ref.py, on every
route it can take.  Every case (1) asks the host-only route query and ASSERTS the route it is there for, (2) places each
output inside a NaN-filled buffer at a 16-byte-aligned offset with guard bands on both sides, (3) runs the entry point,
(4) checks |got - ref| <= bound element by element and (5) that no NaN is left in the output and the guards are untouched.
The worst error / bound of each case goes to the errlog table."""
import ctypes as C

import pytest
import torch

import _gemm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096                          # floats on either side of an output: longer than any output row of the table


def _code(act):
    from torchrl_amd import _C
    return {"tanh": _C.ACT_TANH, "relu": _C.ACT_RELU, "none": _C.ACT_NONE}[act]


class Guarded:
    """An output of `shape` in the middle of a NaN-filled buffer."""

    def __init__(self, *shape):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((2 * GUARD + n,), float("nan"), device=DEV)
        self.out = self.buf[GUARD:GUARD + n].view(*shape)
        assert self.out.data_ptr() % 16 == 0

    def check(self, what):
        assert not torch.isnan(self.out).any(), "%s: NaN left inside the output" % what
        assert torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all(), "%s: guard band written" % what
        return self.out


def _offset_view(t, off):
    """t's values as a contiguous view that starts `off` floats into a larger (aligned) buffer."""
    big = torch.empty(t.numel() + 8, device=DEV)
    v = big[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


def _assert_route(case):
    from torchrl_amd import _C
    got = _C.linear_route(case.op, case.M, case.K, case.N, G=case.G)
    assert {k: got[k] for k in case.route} == case.route, (case.id, case.op, got)
    return got


def _ws(n):
    return torch.empty((max(1, n),), device=DEV)


def _launch(case, act, ins, outs):
    """The entry point of `case` on G problems: ins a list of device-input dicts, outs a list of dicts of output tensors."""
    from torchrl_amd import _C
    lib, G, (M, K, N), code = _C.lib(), case.G, (case.M, case.K, case.N), _code(act)
    col = lambda d, k, none=False: _C._ptrs([i[k] for i in d], k, none)
    s = _C.stream_ptr(DEV)
    gate_code = code if ins[0]["y"] is not None else _C.ACT_NONE
    if case.op == "fwd":
        if G == 1:
            rc = lib.trl_linear_fwd_f32(_C.dev_ptr(ins[0]["x"]), _C.dev_ptr(ins[0]["w"]), _C.dev_ptr(ins[0]["b"]),
                                        _C.dev_ptr(outs[0]["y"]), M, K, N, code, s)
        else:
            rc = lib.trl_linear_fwd_group_f32(G, col(ins, "x"), col(ins, "w"), col(ins, "b"), col(outs, "y"), M, K, N, code, s)
    elif case.op == "fwd_splitk":
        ws = _ws(G * lib.trl_linear_fwd_workspace(M, K, N))
        if G == 1:
            rc = lib.trl_linear_fwd_splitk_f32(_C.dev_ptr(ins[0]["x"]), _C.dev_ptr(ins[0]["w"]), _C.dev_ptr(ins[0]["b"]),
                                               _C.dev_ptr(outs[0]["y"]), M, K, N, code, _C.dev_ptr(ws), s)
        else:
            rc = lib.trl_linear_fwd_splitk_group_f32(G, col(ins, "x"), col(ins, "w"), col(ins, "b"), col(outs, "y"), M, K, N,
                                                     code, _C.dev_ptr(ws), s)
    elif case.op == "bwd_input":
        if G == 1:
            rc = lib.trl_linear_bwd_input_f32(_C.dev_ptr(ins[0]["dy"]), _C.dev_ptr(ins[0]["y"], allow_none=True), gate_code,
                                              _C.dev_ptr(ins[0]["w"]), _C.dev_ptr(outs[0]["dx"]), M, K, N, s)
        else:
            rc = lib.trl_linear_bwd_input_group_f32(G, col(ins, "dy"), col(ins, "y", True), gate_code, col(ins, "w"),
                                                    col(outs, "dx"), M, K, N, s)
    elif case.op == "bwd_input_splitk":
        ws = _ws(lib.trl_linear_bwd_input_workspace(M, K, N))
        rc = lib.trl_linear_bwd_input_splitk_f32(_C.dev_ptr(ins[0]["dy"]), _C.dev_ptr(ins[0]["y"], allow_none=True), gate_code,
                                                 _C.dev_ptr(ins[0]["w"]), _C.dev_ptr(outs[0]["dx"]), _C.dev_ptr(ws), M, K, N, s)
    else:
        ws = _ws(G * lib.trl_linear_bwd_weight_workspace(M, K, N))
        if G == 1:
            rc = lib.trl_linear_bwd_weight_f32(_C.dev_ptr(ins[0]["dy"]), _C.dev_ptr(ins[0]["y"], allow_none=True), gate_code,
                                               _C.dev_ptr(ins[0]["x"]), _C.dev_ptr(outs[0]["dw"]), _C.dev_ptr(outs[0]["db"]),
                                               _C.dev_ptr(ws), M, K, N, s)
        else:
            rc = lib.trl_linear_bwd_weight_group_f32(G, col(ins, "dy"), col(ins, "y", True), gate_code, col(ins, "x"),
                                                     col(outs, "dw"), col(outs, "db"), _C.dev_ptr(ws), M, K, N, s)
    _C.check(rc, case.op)
    torch.cuda.synchronize()


OUT_SHAPES = {"fwd": lambda c: dict(y=(c.M, c.N)), "bwd_input": lambda c: dict(dx=(c.M, c.K)),
              "bwd_weight": lambda c: dict(dw=(c.N, c.K), db=(c.N,))}


def _run_case(case, act, planted, errlog, offsets=None):
    """Steps 2-5 for one activation and input variant; -> the outputs of problem 0 (on the device)."""
    refs = [R.reference(case, act, planted, g) for g in range(case.G)]
    ins = [{k: (None if v is None else v.to(DEV)) for k, v in inp.items()} for inp, _ in refs]
    for name, off in (offsets or {}).items():
        ins[0][name] = _offset_view(ins[0][name], off)
    shapes = OUT_SHAPES[case.op.replace("_splitk", "")](case)
    guards = [{k: Guarded(*shape) for k, shape in shapes.items()} for _ in range(case.G)]
    _launch(case, act, ins, [{k: g.out for k, g in gs.items()} for gs in guards])
    worst = 0.0
    for g, ((_, out), gs) in enumerate(zip(refs, guards)):
        for name, (want, bound) in out.items():
            what = "%s %s %s %s g%d %s" % (case.id, case.op, act, "planted" if planted else "gauss", g, name)
            got = gs[name].check(what)
            ratio = R.worst_ratio(got, want, bound)
            print("%s: worst error / bound %.3f" % (what, ratio))
            assert ratio <= 1.0, what
            worst = max(worst, ratio)
    errlog("%s-%s-%s-%s" % (case.id, case.op, act, "planted" if planted else "gauss"), worst, 1.0)
    return {k: g.out for k, g in guards[0].items()}


ids = lambda cases: ["%s-%s" % (c.id, c.op) for c in cases]


@pytest.mark.parametrize("case", R.CASES + R.HANDOVER, ids=ids(R.CASES + R.HANDOVER))
def test_route_against_float64(case, errlog):
    _assert_route(case)
    for act in case.acts:
        for planted in (False, True):
            _run_case(case, act, planted, errlog)
    R._reference.cache_clear()


@pytest.mark.parametrize("operand", ["x", "w"])
@pytest.mark.parametrize("off", [1, 3])
def test_misaligned_operand_pointer_forward(operand, off, errlog):
    """A base pointer that is not 16-byte aligned drops that operand to element-wise loads; the k order is unchanged, so the
    result meets the same bound and equals the aligned run bit for bit."""
    case = R.MISALIGNED
    _assert_route(case)
    want = _run_case(case, "none", True, errlog)["y"]
    got = _run_case(case, "none", True, errlog, offsets={operand: off})["y"]
    assert torch.equal(got, want)


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("off", [1, 3])
def test_misaligned_gate_pointer(act, off, errlog):
    """The gate of the input gradient and of the weight gradient at an unaligned base, on interior 64 x 64 tiles."""
    for case in (R._c("misaligned", "bwd_input", 1, 128, 128, 132, **R.T64), R._c("misaligned", "bwd_weight", 1, 132, 128, 128, **R.T64)):
        _assert_route(case)
        want = _run_case(case, act, True, errlog)
        got = _run_case(case, act, True, errlog, offsets={"y": off})
        for k in want:
            assert torch.equal(got[k], want[k]), (case.op, k)
        for name in ("dy", "w" if case.op == "bwd_input" else "x"):
            got = _run_case(case, act, True, errlog, offsets={name: off})
            for k in want:
                assert torch.equal(got[k], want[k]), (case.op, name, k)


# ---- mixed-shape weight gradients through FoldPlan(defer_gemm=True), against the reference ----
def _mixed(layers, M, act, want_route, errlog, tag):
    from torchrl_amd import _C
    routes = _C.linear_route("bwd_weight_multi", M, [K for K, _, _ in layers], [N for _, N, _ in layers])
    want_route(routes)
    need = sum(r["splits"] * (N * K + N) for r, (K, N, _) in zip(routes, layers))
    wsg = Guarded(need)
    plan = _C.FoldPlan(wsg.out, defer_gemm=True)
    jobs = []
    for j, (K, N, gated) in enumerate(layers):
        a = act if gated else "none"
        for planted in (False, True):
            inp = R.inputs(7000 + 13 * j + M + planted, M, K, N, a, planted)
            dw, db, bw, bb = R.bwd_weight(inp["dy"], inp["y"], a, inp["x"])
            jobs.append((j, K, N, a, planted, inp, dict(dw=(dw, bw), db=(db, bb))))
    worst = 0.0
    for planted in (False, True):                                        # one launch per variant: the plan's workspace is reused
        outs = {}
        for j, K, N, a, p, inp, ref in jobs:
            if p != planted:
                continue
            d = {k: (None if v is None else v.to(DEV)) for k, v in inp.items()}
            gw, gb = Guarded(N, K), Guarded(N)
            _C.linear_bwd_weight_partials_group([d["dy"]], [d["y"]], _code(a), [d["x"]], [gw.out], [gb.out], plan)
            outs[j] = (d, gw, gb, ref)
        assert len(plan.problems) == len(layers)
        plan.run()
        torch.cuda.synchronize()
        for j, (d, gw, gb, ref) in outs.items():
            for name, gd in (("dw", gw), ("db", gb)):
                what = "%s M%d layer%d %s %s %s" % (tag, M, j, layers[j], "planted" if planted else "gauss", name)
                ratio = R.worst_ratio(gd.check(what), *ref[name])
                print("%s: worst error / bound %.3f" % (what, ratio))
                assert ratio <= 1.0, what
                worst = max(worst, ratio)
        assert torch.isnan(wsg.buf[:GUARD]).all() and torch.isnan(wsg.buf[-GUARD:]).all(), "workspace guard band written"
    errlog("%s-M%d-%s" % (tag, M, act), worst, 1.0)


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("M", R.SKINNY_BATCHES)
def test_skinny_weight_gradients_against_float64(M, act, errlog):
    """All-skinny launches, gated and ungated layers mixed, both orientations, wide side 64 and 256, narrow side 1, 31, 32."""
    def want(routes):
        assert all(r["skinny"] == 1 and r["split_len"] == 128 for r in routes), routes
        assert all(r["splits"] == (M + 127) // 128 for r in routes)
    _mixed(R.SKINNY_SETS, M, act, want, errlog, "skinny")


@pytest.mark.parametrize("want_db_only_gated", [False, True])
def test_hetero_weight_gradients_against_float64(want_db_only_gated, errlog):
    """One non-skinny member sends the set through the hetero GEMM; the (520, 40) layer has fewer tiles AND fewer slices than
    the common grid, so whole workgroups of its grid column leave.  Tanh gates; the second variant mixes an ungated layer in."""
    layers = list(R.HETERO_SET)
    if want_db_only_gated:
        layers[2] = (520, 40, False)

    def want(routes):
        assert all(r["skinny"] == 0 and r["tile_m"] == 64 and r["tile_n"] == 64 for r in routes), routes
        tiles = [-(-N // 64) * -(-K // 64) for K, N, _ in layers]
        splits = [r["splits"] for r in routes]
        assert tiles[2] < max(tiles) and splits[2] < max(splits), (tiles, splits)
    _mixed(layers, R.HETERO_BATCH, "tanh", want, errlog, "hetero")


def test_hetero_weight_gradient_without_db(errlog):
    """want_db = 0 through the entry point itself (FoldPlan always asks for db): partials in a guarded workspace, folded on
    the host in float64 -- the fold's own roundings are then absent, the bound is unchanged."""
    from torchrl_amd import _C
    layers, M = R.HETERO_SET, R.HETERO_BATCH
    routes = _C.linear_route("bwd_weight_multi", M, [K for K, _, _ in layers], [N for _, N, _ in layers])
    assert all(r["skinny"] == 0 for r in routes)
    g = len(layers)
    ins = [R.inputs(9100 + j, M, K, N, "tanh", True) for j, (K, N, _) in enumerate(layers)]
    dev = [{k: v.to(DEV) for k, v in inp.items()} for inp in ins]
    parts = [Guarded(r["splits"], N * K) for r, (K, N, _) in zip(routes, layers)]
    arr = lambda ts: (C.c_void_p * g)(*[t.data_ptr() for t in ts])
    Ks, Ns = (C.c_int * g)(*[K for K, _, _ in layers]), (C.c_int * g)(*[N for _, N, _ in layers])
    _C.check(_C.lib().trl_linear_bwd_weight_partials_multi_f32(
        g, arr([d["dy"] for d in dev]), arr([d["y"] for d in dev]), _C.ACT_TANH, arr([d["x"] for d in dev]), Ks, Ns, 0,
        arr([p.out for p in parts]), M, _C.stream_ptr(DEV)), "trl_linear_bwd_weight_partials_multi_f32")
    torch.cuda.synchronize()
    worst = 0.0
    for j, ((K, N, _), inp, p) in enumerate(zip(layers, ins, parts)):
        dw, _, bw, _ = R.bwd_weight(inp["dy"], inp["y"], "tanh", inp["x"])
        got = p.check("layer %d" % j).double().sum(0).view(N, K)
        ratio = R.worst_ratio(got, dw, bw)
        assert ratio <= 1.0, (j, ratio)
        worst = max(worst, ratio)
    errlog("hetero-nodb", worst, 1.0)


def test_grouped_launch_limits():
    """12 problems are accepted (the t128 cases run them), 13 refused; a gated / ungated mixture is refused with the existing
    message; M = 0 returns without touching the outputs."""
    from torchrl_amd import _C
    lib, s = _C.lib(), _C.stream_ptr(DEV)
    M, K, N = 8, 8, 8
    t = lambda *shape: torch.randn(*shape, device=DEV)
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[0 if x is None else x.data_ptr() for x in ts])
    for G, ok in ((12, True), (13, False)):
        xs, ws, ys = [t(M, K) for _ in range(G)], [t(N, K) for _ in range(G)], [Guarded(M, N) for _ in range(G)]
        rc = lib.trl_linear_fwd_group_f32(G, ptrs(xs), ptrs(ws), None, ptrs([y.out for y in ys]), M, K, N, _C.ACT_NONE, s)
        torch.cuda.synchronize()
        assert (rc == 0) == ok
        if ok:
            for g in range(G):
                want, bound = R.fwd(xs[g], ws[g], None, "none")
                assert R.worst_ratio(ys[g].check("g%d" % g), want, bound) <= 1.0
        else:
            assert "12 problems" in lib.trl_last_error().decode()
            assert all(torch.isnan(y.buf).all() for y in ys)
    dys, gates, ws, dxs = [t(M, N), t(M, N)], [t(M, N), None], [t(N, K), t(N, K)], [Guarded(M, K), Guarded(M, K)]
    rc = lib.trl_linear_bwd_input_group_f32(2, ptrs(dys), ptrs(gates), _C.ACT_TANH, ptrs(ws), ptrs([d.out for d in dxs]), M, K, N, s)
    assert rc != 0 and "either every problem of a group is gated or none" in lib.trl_last_error().decode()
    xs, dws, dbs = [t(M, K), t(M, K)], [Guarded(N, K), Guarded(N, K)], [Guarded(N), Guarded(N)]
    wsp = _ws(2 * lib.trl_linear_bwd_weight_workspace(M, K, N))
    rc = lib.trl_linear_bwd_weight_group_f32(2, ptrs(dys), ptrs(gates), _C.ACT_TANH, ptrs(xs), ptrs([d.out for d in dws]),
                                             ptrs([d.out for d in dbs]), wsp.data_ptr(), M, K, N, s)
    assert rc != 0 and "either every problem of a group is gated or none" in lib.trl_last_error().decode()
    y, dx = Guarded(4, N), Guarded(4, K)
    assert lib.trl_linear_fwd_group_f32(2, ptrs(xs), ptrs(ws), None, ptrs([y.out, y.out]), 0, K, N, _C.ACT_NONE, s) == 0
    assert lib.trl_linear_bwd_input_group_f32(2, ptrs(dys), None, _C.ACT_NONE, ptrs(ws), ptrs([dx.out, dx.out]), 0, K, N, s) == 0
    torch.cuda.synchronize()
    for d in dxs + dws + dbs + [y, dx]:
        assert torch.isnan(d.buf).all()
