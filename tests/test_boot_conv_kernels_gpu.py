"""trl_boot_head_dx_f32 (the K heads' input gradient at a conv feature, summed, gated and un-flattened by one launch)
element by element against the float64 restatement of tests/_boot_conv_ref.py, and the three launches it replaces
(grouped input gradient into a (K, B, F) stack, trl_boot_fold_f32, trl_transpose_bpc_gate_f32) to the same bound on the
same inputs.  The bound's constant comes from the float32 CPU run (tests/test_boot_conv_cpu.py), not from the device."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _boot_conv_ref as R                                                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _device_case(c, like_in):
    """The case's operands on the device: (dzs, gates or None, ws, y_top in the asked layout)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    K = c["K"]
    dzs = [t(c["dz"][k]) for k in range(K)]
    gates = None if c["gates"] is None else [t(c["gates"][k]) for k in range(K)]
    ws = [t(c["w"][k]) for k in range(K)]
    y_top = t(c["y_top"] if like_in else c["y_top"].transpose(0, 2, 1))   # (B, C, P) | (B, P, C)
    return dzs, gates, ws, y_top


def _three_launches(c, dzs, gates, ws, y_top, like_in):
    from torchrl_amd import _C
    K, B, C, P = c["K"], c["B"], c["C"], c["P"]
    stack = torch.empty((K, B, C * P), dtype=torch.float32, device=DEV)
    _C.linear_bwd_input_group(dzs, gates if gates is not None else [None] * K, c["act"] if gates is not None else _C.ACT_NONE,
                              ws, dxs=list(stack.unbind(0)))
    return _C.transpose_bpc(_C.boot_fold(stack).view(B, C, P), B, C, P, y_gate=y_top, gate_act=c["act"], gate_like_in=like_in)


@pytest.mark.parametrize("K,B,C,P,H1", R.head_shapes())
def test_head_dx_against_the_restatement(K, B, C, P, H1, errlog):
    from torchrl_amd import _C
    assert (_C.ACT_TANH, _C.ACT_RELU, _C.ACT_NONE) == (R.ACT_TANH, R.ACT_RELU, R.ACT_NONE)
    assert _C.boot_head_dx_supported(K, B, H1, C, P) and K <= 64 and (K <= _C.GROUP_MAX or K == 13)
    for act, like_in in R.GATES:
        c = R.head_case(K, B, C, P, H1, act)
        ref = R.head_dx_ref(c)
        dzs, gates, ws, y_top = _device_case(c, like_in)
        gate_act = act if gates is not None else _C.ACT_NONE
        out = _C.boot_head_dx(dzs, gates, gate_act, ws, y_top, act, C, P, like_in)
        again = _C.boot_head_dx(dzs, gates, gate_act, ws, y_top, act, C, P, like_in)
        old = _three_launches(c, dzs, gates, ws, y_top, like_in)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (B, P, C)
        got, got2, got_old = out.cpu().numpy(), again.cpu().numpy(), old.cpu().numpy().reshape(B, P, C)
        assert np.array_equal(got, got2)                                  # the same inputs, the same bits
        r_new, r_old = R.head_dx_ratio(got, ref), R.head_dx_ratio(got_old, ref)      # (exact zeros are asserted inside)
        name = "act%d like_in%d" % (act, like_in)
        print("head_dx K=%d B=%d C=%d P=%d H1=%d %s: new %.3f old %.3f (bound %g)" % (K, B, C, P, H1, name, r_new, r_old, R.K_HEAD_DX))
        if act == R.ACT_TANH:                                            # information only: without the gate's absolute term
            print("  ... under the plain |act'| sum|terms|: new %.1f old %.1f"
                  % (R.head_dx_plain_ratio(got, ref), R.head_dx_plain_ratio(got_old, ref)))
        errlog(name + " head_dx", r_new, R.K_HEAD_DX)
        errlog(name + " three launches", r_old, R.K_HEAD_DX)
        if B > 3:
            assert np.all(got[3::4] == 0.0)                              # samples masked out in every head
        assert r_new <= R.K_HEAD_DX, (name, r_new)
        assert r_old <= R.K_HEAD_DX, (name, r_old)


def test_head_dx_takes_per_head_gates_and_unaligned_weights():
    """Gates given for some heads only (the others' dz is dZ as it stands), and weights that are views at a 4-byte offset
    (the 4-byte load path at F % 4 == 0)."""
    from torchrl_amd import _C
    K, B, C, P, H1 = 3, 5, 16, 4, 32
    c = dict(R.head_case(K, B, C, P, H1, R.ACT_TANH))
    dzs, gates, ws, y_top = _device_case(c, True)
    pool = torch.zeros(K * H1 * C * P + 1, device=DEV)
    ws_off = []
    for k in range(K):
        v = pool[1 + k * H1 * C * P:1 + (k + 1) * H1 * C * P].view(H1, C * P)
        v.copy_(ws[k])
        ws_off.append(v)
    assert all(w.data_ptr() % 16 for w in ws_off)
    a = _C.boot_head_dx(dzs, gates, R.ACT_TANH, ws, y_top, R.ACT_TANH, C, P, True)
    b = _C.boot_head_dx(dzs, gates, R.ACT_TANH, ws_off, y_top, R.ACT_TANH, C, P, True)
    assert torch.equal(a, b)                                             # same reduction order on either load path
    pre = [dzs[0] * (1.0 - gates[0] * gates[0]), dzs[1], dzs[2]]
    mixed = _C.boot_head_dx(pre, [None, gates[1], gates[2]], R.ACT_TANH, ws, y_top, R.ACT_TANH, C, P, True)
    ref = R.head_dx_ref(c)
    assert R.head_dx_ratio(mixed.cpu().numpy(), ref) <= R.K_HEAD_DX


def test_head_dx_refusals():
    from torchrl_amd import _C
    assert not _C.boot_head_dx_supported(65, 4, 8, 4, 4) and not _C.boot_head_dx_supported(0, 4, 8, 4, 4)
    assert not _C.boot_head_dx_supported(3, 0, 8, 4, 4) and not _C.boot_head_dx_supported(3, 4, 0, 4, 4)
    assert _C.boot_head_dx_supported(64, 512, 512, 64, 49)
    z = lambda *s: torch.zeros(s, device=DEV)
    with pytest.raises(_C.TrlError, match="unsupported shape"):
        _C.boot_head_dx([z(2, 4)] * 65, None, _C.ACT_NONE, [z(4, 8)] * 65, z(2, 2, 4), _C.ACT_RELU, 2, 4, True)
    with pytest.raises(_C.TrlError, match="K gradients"):
        _C.boot_head_dx([z(2, 4)] * 2, None, _C.ACT_NONE, [z(4, 9)] * 2, z(2, 2, 4), _C.ACT_RELU, 2, 4, True)
    with pytest.raises(_C.TrlError, match="no CPU path"):
        _C.boot_head_dx([torch.zeros(2, 4)], None, _C.ACT_NONE, [torch.zeros(4, 8)], torch.zeros(2, 2, 4), _C.ACT_RELU, 2, 4, True)
