"""The Bootstrapped DQN kernels (torchrl_amd/csrc/k_bootdqn.hip) called directly through their `_C` wrappers and compared
with the restatements of tests/_boot_dqn_ref.py on identical inputs; tests/test_boot_dqn_cpu.py holds the float32 run of
the restatements to the same bounds.  With U = 2^-24 (derivation: `_boot_dqn_ref.boot_td_ratios`):
    actions, one-hot rows, head-mode Q rows, head and mask draws, the K-fold: EXACT
    |d dq| <= 8 U mag 2 / (K B) at the taken action of an unmasked (sample, head), exactly 0 everywhere else
    loss sum within sum m (2 |e| delta + delta^2 + 2 U e^2) / K, delta = 8 U mag; reward sum within 4 U sum |r|; mask sum exact
Every bounded comparison prints its worst err / bound as a RATIO line and files it through `errlog`."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _boot_dqn_ref as R                                                     # noqa: E402
from torchrl.algo import BootstrappedDQN                                      # noqa: E402,F401  (no test here runs without the feature)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U, F32, F64 = R.U, R.F32, R.F64
G32 = float(F32(R.GAMMA))                                                     # the discount the kernel is handed


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def report(name, ratios, errlog):
    print("RATIO %s: %s" % (name, " ".join("%s %.4f" % kv for kv in sorted(ratios.items()))))
    for k, r in ratios.items():
        errlog("%s %s" % (name, k), r, 1.0)
    assert max(ratios.values()) <= 1.0, ratios


# ------------------------------------------------------------------ trl_boot_act_i64
@pytest.mark.parametrize("N,K,A", R.ka_cases(R.ACT_N))
def test_actions_equal_the_restatement_exactly(N, K, A):
    from torchrl_amd import _C
    q, head = R.act_case(N, K, A)
    qd = dev(q)
    # each env under its head (planted: ties inside a head, heads -1, K and K + 5)
    onehot = torch.full((N, A), 7.0, device=DEV)
    act, q_sel = _C.boot_act(qd, dev(head), want_q=True, onehot=onehot)
    want, want_q, want_1h = R.boot_act_ref(q, head)
    assert act.dtype == torch.int64 and np.array_equal(host(act), want)
    assert np.array_equal(host(q_sel).astype(F64), want_q) and np.array_equal(host(onehot), want_1h)
    # the ensemble vote (planted: ties between sums of different addends), from the list of the stack's blocks as well
    onehot.fill_(7.0)
    act, q_sel = _C.boot_act(list(qd.unbind(0)), None, want_q=True, onehot=onehot)
    want, want_q, want_1h = R.boot_act_ref(q, None)
    assert np.array_equal(host(act), want) and np.array_equal(host(onehot), want_1h)
    # the sum is exact on this grid; times the float32 1 / K: one rounding of 1 / K and one of the product
    assert np.all(np.abs(host(q_sel).astype(F64) - want_q) <= 2 * U * np.abs(want_q))
    act2, none = _C.boot_act(qd, None)
    assert none is None and torch.equal(act2, act)


# ------------------------------------------------------------------ the draws
COUNTERS = (0, 7, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, -1)


@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("N", [1, 3, 4, 5, 1000])
def test_head_and_mask_draws_equal_the_restatement(N, K):
    from torchrl_amd import _C
    seed = R.POLICY_SEED
    for ctr in COUNTERS:
        head = torch.full((N,), -7, dtype=torch.int64, device=DEV)
        _C.boot_heads(head, K, seed, ctr)
        assert np.array_equal(host(head), R.heads_ref(np.full(N, -7), K, seed, ctr)), ctr
        for p in (0.5, 0.1):
            out = torch.full((N, K), 7.0, device=DEV)
            _C.boot_masks(out, p, seed, ctr)
            assert np.array_equal(host(out), R.masks_ref(N, K, p, seed, ctr)), (ctr, p)
    # an env offset: the matching slice of a larger draw
    big_h = torch.zeros(N + 9, dtype=torch.int64, device=DEV)
    _C.boot_heads(big_h, K, seed + (5 << 32), 3)
    part = torch.zeros(N, dtype=torch.int64, device=DEV)
    _C.boot_heads(part, K, seed + (5 << 32), 3, env_offset=9)
    assert torch.equal(part, big_h[9:]) and np.array_equal(host(part), R.heads_ref(np.zeros(N), K, seed + (5 << 32), 3, 9))
    big_m, part_m = torch.zeros(N + 9, K, device=DEV), torch.zeros(N, K, device=DEV)
    _C.boot_masks(big_m, 0.5, seed, 3)
    _C.boot_masks(part_m, 0.5, seed, 3, env_offset=9)
    assert torch.equal(part_m, big_m[9:])
    # p = 0 and p = 1
    assert float(_C.boot_masks(torch.full((N, K), 7.0, device=DEV), 0.0, seed, 1).abs().sum()) == 0.0
    assert float(_C.boot_masks(torch.full((N, K), 7.0, device=DEV), 1.0, seed, 1).sum()) == N * K


def test_masked_head_draw_leaves_the_other_envs_bit_identical():
    from torchrl_amd import _C
    N, K = 1000, 10
    rs = np.random.RandomState(2)
    before = rs.randint(-3, 100, N).astype(np.int64)                     # (values a draw could not produce, too)
    for mask in (np.eye(1, N, 700, dtype=np.uint8)[0], (rs.rand(N) < 0.3).astype(np.uint8) * 255, np.zeros(N, np.uint8)):
        head = dev(before)
        _C.boot_heads(head, K, R.POLICY_SEED, 12, reset_mask=dev(mask))
        want = R.heads_ref(before, K, R.POLICY_SEED, 12, reset_mask=mask)
        assert np.array_equal(host(head), want)
        assert np.array_equal(host(head)[mask == 0], before[mask == 0])
    assert (want == before).all()                                        # the empty mask draws nothing
    only = np.eye(1, N, 700, dtype=np.uint8)[0]                          # the one set byte lies beyond index 255
    head = dev(before)
    _C.boot_heads(head, K, R.POLICY_SEED, 12, reset_mask=dev(only))
    assert int((host(head) != before).sum()) <= 1 and 0 <= int(host(head)[700]) < K


# ------------------------------------------------------------------ trl_boot_td_loss_f32
def run_td(c, ring=None, workspace=None):
    from torchrl_amd import _C
    sums = torch.full((3,), 7.0, dtype=torch.float64, device=DEV)
    dq = _C.boot_td_loss(dev(c["q"]), dev(c["qn"]), dev(c["acts"]), dev(c["rew"]), dev(c["term"]), dev(c["masks"]), G32, sums,
                         ring=ring, workspace=workspace)
    torch.cuda.synchronize()
    return dict(dq=host(dq), sums=host(sums))


@pytest.mark.parametrize("B,K,A", R.ka_cases(R.ACT_N))
def test_td_loss_against_the_restatement(B, K, A, errlog):
    worst = {}
    for float_acts in (False, True):
        c = R.td_case(B, K, A, float_acts)
        got = run_td(c)
        ref = R.boot_td_ref(c["q"], c["qn"], c["acts"], c["rew"], c["term"], c["masks"], G32)
        for k, r in R.boot_td_ratios(got, ref, K, B).items():
            worst[k] = max(worst.get(k, 0.0), r)
        if K > 1:
            assert np.all(got["dq"][K - 1] == 0.0)                       # the all-zero mask column
        if B > 1:
            assert np.all(got["dq"][:, B - 1] == 0.0)                    # the all-zero mask row
    report("boot_td B=%d K=%d A=%d" % (B, K, A), worst, errlog)


def test_td_loss_is_deterministic_and_files_its_ring_row():
    from torchrl_amd import _C
    c = R.td_case(257, 10, 6, True)
    a, b = run_td(c), run_td(c)
    assert np.array_equal(a["dq"], b["dq"]) and np.array_equal(a["sums"], b["sums"])
    slots = 4
    for u in (0, 3, 4):
        ring = torch.full((slots, 3), -5.0, dtype=torch.float64, device=DEV)
        counter = torch.tensor([float(u), 1.0, 1.0, 0.0], dtype=torch.float64, device=DEV)
        got = run_td(c, ring=(ring, counter))
        rows = host(ring)
        assert np.array_equal(rows[u % slots], got["sums"]) and np.array_equal(got["sums"], a["sums"])
        assert np.all(np.delete(rows, u % slots, axis=0) == -5.0)
        assert float(counter[0]) == float(u)


def test_td_loss_at_the_grid_cap_with_a_kept_workspace(errlog):
    """K B = 135 168 items: the grid stops at 256 workgroups and a thread takes up to three items; three launches on ONE
    workspace (the arrival counter is back at zero after each) give the same bits, inside the bounds."""
    from torchrl_amd import _C
    B, K, A = R.TD_CAP
    c = R.td_case(B, K, A, True)
    ws = _C.boot_td_loss_workspace(DEV)
    runs = [run_td(c, workspace=ws) for _ in range(3)]
    assert int(ws[:16].to(torch.int64).sum()) == 0
    for other in runs[1:]:
        assert np.array_equal(runs[0]["dq"], other["dq"]) and np.array_equal(runs[0]["sums"], other["sums"])
    ref = R.boot_td_ref(c["q"], c["qn"], c["acts"], c["rew"], c["term"], c["masks"], G32)
    report("boot_td B=%d K=%d A=%d" % (B, K, A), R.boot_td_ratios(runs[0], ref, K, B), errlog)
    small = R.td_case(255, 2, 2, False)                                   # another grid on the same workspace
    ref_s = R.boot_td_ref(small["q"], small["qn"], small["acts"], small["rew"], small["term"], small["masks"], G32)
    report("boot_td after the cap", R.boot_td_ratios(run_td(small, workspace=ws), ref_s, 2, 255), errlog)
    assert np.array_equal(run_td(c, workspace=ws)["sums"], runs[0]["sums"])


def test_k_fold_is_the_ascending_float32_sum():
    from torchrl_amd import _C
    rs = np.random.RandomState(4)
    for K, B, F in ((1, 5, 3), (10, 257, 32), (10, 255, 33), (64, 7, 5), (3, 1000, 128)):
        x = rs.randn(K, B, F).astype(F32)
        got = _C.boot_fold(dev(x))
        assert got.shape == (B, F) and np.array_equal(host(got), R.fold_ref(x, F32))
    x = rs.randn(4, 9, 8).astype(F32)                                    # an unaligned view: the scalar route
    base = dev(np.concatenate([np.zeros(1, F32), x.reshape(-1)]))
    assert np.array_equal(host(_C.boot_fold(base[1:].view(4, 9, 8))), R.fold_ref(x, F32))


# ------------------------------------------------------------------ argument errors
def test_argument_errors_raise_and_launch_nothing():
    from torchrl_amd import _C
    c = {k: dev(v) for k, v in R.td_case(8, 3, 4, False).items()}
    sums = torch.zeros(3, dtype=torch.float64, device=DEV)
    td = lambda **kw: _C.boot_td_loss(*[kw.get(k, c[k]) for k in ("q", "qn", "acts", "rew", "term", "masks")], G32, sums)
    lib, sp = _C.lib(), _C.stream_ptr(DEV)
    p = lambda t, dt=torch.float32: _C.dev_ptr(t, dt)
    dq = torch.zeros(3, 8, 4, device=DEV)
    ws = _C.boot_td_loss_workspace(DEV)
    raw = lambda ai, af, K=3, B=8, A=4: lib.trl_boot_td_loss_f32(p(c["q"]), p(c["qn"]), ai, af, p(c["rew"]), p(c["term"]),
                                                                   p(c["masks"]), G32, K, B, A, p(dq),
                                                                   p(sums, torch.float64), None, 0, None,
                                                                   p(ws, torch.uint8), sp)
    acts_f = c["acts"].float()
    for code in (raw(p(c["acts"], torch.int64), p(acts_f)), raw(None, None),          # both / neither action pointer
                 raw(p(c["acts"], torch.int64), None, B=0),                           # an empty batch
                 raw(p(c["acts"], torch.int64), None, K=0), raw(p(c["acts"], torch.int64), None, K=65),
                 raw(p(c["acts"], torch.int64), None, A=0), raw(p(c["acts"], torch.int64), None, A=65)):
        assert code != 0
    with pytest.raises(_C.TrlError, match="exactly one of acts"):
        _C.check(raw(None, None), "trl_boot_td_loss_f32")
    with pytest.raises(_C.TrlError, match="non-empty batch"):
        _C.check(raw(p(c["acts"], torch.int64), None, B=0), "trl_boot_td_loss_f32")
    with pytest.raises(_C.TrlError):                                     # (empty tensors have no address: refused all the same)
        _C.boot_td_loss(c["q"][:, :0], c["qn"][:, :0], c["acts"][:0], c["rew"][:0], c["term"][:0], c["masks"][:0], G32, sums)
    with pytest.raises(_C.TrlError, match="no CPU path"):
        td(q=c["q"].cpu())
    with pytest.raises(_C.TrlError, match="masks"):
        td(masks=c["masks"].t().contiguous())
    big = torch.zeros(65, 2, 2, device=DEV)
    with pytest.raises(_C.TrlError, match="1 <= K <= 64"):
        _C.boot_act(big, None)
    with pytest.raises(_C.TrlError, match="1 <= A <= 64"):
        _C.boot_act(torch.zeros(2, 2, 65, device=DEV), None)
    with pytest.raises(_C.TrlError, match="1 <= K <= 64"):
        _C.boot_heads(torch.zeros(4, dtype=torch.int64, device=DEV), 65, 1, 1)
    with pytest.raises(_C.TrlError, match="1 <= K <= 64"):
        _C.boot_masks(torch.zeros(4, 65, device=DEV), 0.5, 1, 1)
    with pytest.raises(_C.TrlError, match="env offset"):
        _C.boot_heads(torch.zeros(4, dtype=torch.int64, device=DEV), 4, 1, 1, env_offset=-1)
    with pytest.raises(_C.TrlError, match="env offset"):
        _C.boot_masks(torch.zeros(4, 4, device=DEV), 0.5, 1, 1, env_offset=-1)
    with pytest.raises(_C.TrlError, match="no CPU path"):
        _C.boot_act(torch.zeros(2, 2, 2), None)
    with pytest.raises(_C.TrlError, match="consecutive slices"):
        _C.boot_act([torch.zeros(2, 2, device=DEV), torch.zeros(2, 2, device=DEV) + 1], None)
    with pytest.raises(_C.TrlError, match="1 <= K <= 64"):
        _C.boot_fold(torch.zeros(65, 4, device=DEV))
    with pytest.raises(_C.TrlError, match="workspace"):
        _C.boot_td_loss(*[c[k] for k in ("q", "qn", "acts", "rew", "term", "masks")], G32, sums, workspace=ws[:64])
    torch.cuda.synchronize()
    assert float(sums.abs().sum()) == 0.0 and float(dq.abs().sum()) == 0.0            # nothing was launched
    assert int(ws.to(torch.int64).sum()) == 0
