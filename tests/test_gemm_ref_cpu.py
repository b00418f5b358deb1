"""tests/_gemm_ref.py before a GPU sees it: the restatement equals float64 autograd of act(F.linear(...)), and a correct fp32
evaluation on the CPU -- torch.matmul in float32, and a split-and-fold one -- stays inside the per-element bound for every
case of the table the GPU file runs.  The table's routes are checked here too: the route query touches no device."""
import pytest
import torch

import _gemm_ref as R

ALL_CASES = R.CASES + R.HANDOVER + [R.MISALIGNED]
ids = lambda cases: ["%s-%s" % (c.id, c.op) for c in cases]


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("M,K,N", [(7, 5, 3), (33, 70, 9)])
def test_restatement_equals_float64_autograd(M, K, N, act):
    inp = R.inputs(M + K + N, M, K, N, act)
    x, w, b = (inp[k].double().requires_grad_(True) for k in ("x", "w", "b"))
    y = R.act_fn(torch.nn.functional.linear(x, w, b), act)
    dy = inp["dy"].double()
    y.backward(dy)
    got_y, _ = R.fwd(inp["x"], inp["w"], inp["b"], act)
    assert torch.allclose(got_y, y.detach(), rtol=1e-13, atol=1e-13)
    gate = None if act == "none" else y.detach()                          # the gate autograd uses: the layer's own output
    dx, _ = R.bwd_input(dy, gate, act, inp["w"])
    dw, db, _, _ = R.bwd_weight(dy, gate, act, inp["x"])
    for got, want in ((dx, x.grad), (dw, w.grad), (db, b.grad)):
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)


def test_relu_gate_rule_at_zero_and_gate_ranges():
    y = R.inputs(5, 40, 8, 24, "relu")["y"]
    assert (y == 0).sum() == 3 and ((y.abs() >= 1e-3) | (y == 0)).all()
    assert (R.dact_from_out(y, "relu")[y == 0] == 0).all()                # +0 and -0: y > 0 is false
    assert R.inputs(5, 40, 8, 24, "tanh")["y"].abs().max() <= 0.7
    p, q = R.inputs(5, 70, 40, 33, "none", planted=True), R.inputs(5, 70, 40, 33, "none")
    ratio = (p["x"].double() / q["x"].double()).round()                   # (the planted product is rounded to fp32)
    assert set(ratio.unique().tolist()) == {1.0, 100.0}
    for r, c in ((69, 39), (32, 32), (0, 39), (64, 0)):                   # last row / column, first index after a boundary
        assert ratio[r, c] == 100.0
    assert ratio[31, 31] == 1.0


def _f32_outputs(case, act, inp, split_len):
    op = case.op.replace("_splitk", "")
    if op == "fwd":
        return dict(y=R.fwd_f32(inp["x"], inp["w"], inp["b"], act, split_len))
    if op == "bwd_input":
        return dict(dx=R.bwd_input_f32(inp["dy"], inp["y"], act, inp["w"], split_len))
    dw, db = R.bwd_weight_f32(inp["dy"], inp["y"], act, inp["x"], split_len)
    return dict(dw=dw, db=db)


@pytest.mark.parametrize("case", ALL_CASES, ids=ids(ALL_CASES))
def test_fp32_cpu_evaluations_meet_the_bound(case):
    big = case.G * case.M * case.K * case.N > 2e8
    for act in (case.acts[:1] if big else case.acts):
        for planted in (False, True):
            for g in sorted({0, case.G - 1}):
                inp, out = R.reference(case, act, planted, g)
                for split_len in (0, 128):
                    got = _f32_outputs(case, act, inp, split_len)
                    for name, (want, bound) in out.items():
                        ratio = R.worst_ratio(got[name], want, bound)
                        assert ratio <= 1.0, (case.id, case.op, act, planted, g, split_len, name, ratio)
    R._reference.cache_clear()


def test_a_dropped_or_doubled_planted_term_breaks_the_bound_by_far():
    """What the planted variant is for: lose the last reduction index, or read it twice, and the result leaves the bound by
    orders of magnitude in the rows and columns that carry a planted value."""
    case = R.CASES[0]
    inp, out = R.reference(case, "none", True)
    want, bound = out["y"]
    x = inp["x"].clone()
    x[:, -1] = 0.0
    assert R.worst_ratio(R.fwd_f32(x, inp["w"], inp["b"], "none"), want, bound) > 1e3
    x[:, -1] = 2.0 * inp["x"][:, -1]
    assert R.worst_ratio(R.fwd_f32(x, inp["w"], inp["b"], "none"), want, bound) > 1e3


def _route(case):
    from torchrl_amd import _C
    return _C.linear_route(case.op, case.M, case.K, case.N, G=case.G)


@pytest.mark.parametrize("case", ALL_CASES, ids=ids(ALL_CASES))
def test_table_routes_match_the_query(case):
    got = _route(case)
    assert {k: got[k] for k in case.route} == case.route, got


def test_route_query_arguments():
    from torchrl_amd import _C
    lib = _C.lib()
    import ctypes as C
    one, out = (C.c_int * 1)(64), (C.c_int32 * 7)()
    assert lib.trl_linear_route_i32(9, 1, 64, one, one, out) != 0 and b"unknown op" in lib.trl_last_error()
    assert lib.trl_linear_route_i32(0, 13, 64, one, one, out) != 0 and b"12 problems" in lib.trl_last_error()
    assert lib.trl_linear_route_i32(0, 1, 64, None, one, out) != 0
    rows = _C.linear_route("bwd_weight_multi", 300, [17, 256], [256, 12])
    assert [r["skinny"] for r in rows] == [1, 1] and rows[0]["splits"] == lib.trl_linear_bwd_weight_multi_splits(300, 17, 256)
    rows = _C.linear_route("bwd_weight_multi", 300, [17, 70], [256, 33])
    assert [r["skinny"] for r in rows] == [0, 0] and rows[0]["tile_m"] == 64
    assert _C.linear_route("bwd_weight", 4096, 256, 256)["splits"] == lib.trl_linear_bwd_weight_splits(4096, 256, 256)
