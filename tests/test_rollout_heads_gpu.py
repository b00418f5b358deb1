"""The categorical and the state-dependent-std head of the persistent rollout, each launched through torchrl_amd._C and
compared with the float64 restatements of tests/_rollout_ref.py, teacher-forced (every stored cell is restated from the launch's
own obs[t, n], the step's noise and -- for what follows the action -- the STORED action, so a borderline categorical draw leaves
nothing else uncompared):

    trl_rollout_synth_cat_f32    rollout_kernel<.., HEAD_CAT>    k_rollout.hip
    trl_rollout_synth_sd_f32     rollout_kernel<.., HEAD_SD>

The bounds are those tests/test_rollout_heads_cpu.py holds the float32 run of the restatements to, and shows a list of subtly
wrong heads to miss; every test prints its worst err / bound and hands it to `errlog`
(profiles/NOTES_rollout_kernel_tests.md has one run's)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _rollout_ref as R                                                      # noqa: E402
from _rollout_launch import DEV, Launcher, check                              # noqa: E402

pytestmark = pytest.mark.gpu
HEAD_CASES = R.head_cases()


def run_case(c, what, errlog, run=None):
    """One launch of case `c` against the restatement -> (run dict, ratios); a categorical run moves no more than
    BORDERLINE_CAP of its cells' worth of borderline draws."""
    o = (Launcher(c) if run is None else run).launch().read()
    res = R.verify(c, o)
    check(res, what, errlog)
    if R.head_of(c) == "cat":
        assert res["_share_borderline"] <= R.BORDERLINE_CAP, res["_share_borderline"]
    return o, res


@pytest.mark.parametrize("name,kw", HEAD_CASES, ids=[n for n, _ in HEAD_CASES])
def test_head_steps_against_the_restatement(name, kw, errlog):
    """Every instantiation of both heads at N = 40 x 12 steps, N around the 16-env tile x 1 / 5 steps, a ring that wraps inside
    the launch, envs out of step, guards around every ring tensor; det / host / device noise; a second rank's env offset and a
    step counter whose high word changes inside the launch; tied, peaked and exact-threshold categorical heads; log_std on both
    clamps; the bookkeeping variants.  Categorical: the stored index is the restated one (on a borderline cell: or the neighbour
    across the close prefix sum); both heads: next observation, reward, log pi_old at the stored action, V, boot values within
    their derived bounds; flags, counters, chain identities, episode log, publish copy exact."""
    c = R.rollout_case(**kw)
    o, res = run_case(c, name, errlog)
    rr = R.ring_rows(c)
    if name == "cat-tie-det":
        assert (o["acts"][rr] == 1.0).all(), "equal logits: the lowest index wins"
    if name == "cat-tie":
        # log pi of either index is the same float64 number, and both are held to it above; both are drawn
        k = o["acts"][rr].reshape(-1)
        assert (k == 1).mean() > 0.25 and (k == c["A"] - 1).mean() > 0.25 and ((k == 1) | (k == c["A"] - 1)).mean() > 0.9
    if name.startswith("cat-peaked"):
        # where the float64 sum is 1 to float32 precision the drawn index is the arg-max (on every cell that is not
        # borderline) and its log pi is within its bound of 0: `verify` held it to -log S, |log S| <= 2^-25
        M = c["T"] * c["N"]
        st = R.step_terms(c, o["obs"][rr].reshape(M, -1), o["obs"][rr].reshape(M, -1), c["eps"].reshape(M, -1), o["acts"][rr].reshape(M, 1))
        one = st["S"] - 1.0 <= 2.0 ** -25
        top = st["logits"].argmax(1)
        assert np.isfinite(o["old_logp"][rr]).all() and (name != "cat-peaked-S1" or one.all())
        assert (st["k_stored"] == top)[one & ~st["border"]].all()
        lp = o["old_logp"][rr].reshape(M)
        assert (np.abs(lp) <= st["b_logp"] + 2.0 ** -25)[one & (st["k_stored"] == top)].all()
    if name == "cat-exact-threshold":
        t, n = R.EXACT_CELL
        assert o["acts"][rr[t], n, 0] == 1.0, "u S == P_1: the threshold is reached"


@pytest.mark.parametrize("head", ["cat", "sd"])
def test_device_noise_continues_over_two_launches(head, errlog):
    """Device noise keyed noise_step0 + t with noise_step0 = 100; the second launch continues the key, the ring and the env
    state on the device."""
    c = R.two_launch_case(head)
    run = Launcher(c)
    o, _ = run_case(c, head + " launch 1", errlog, run)
    c2 = R.continue_case(c, o, T=7)
    for v in run.ring.values():
        v.fill_(R.SENT)
    run.ep_count.zero_()
    run.ep_log.fill_(R.SENT)
    run.c = c2
    run_case(c2, head + " launch 2", errlog, run)


def test_refusals_launch_nothing():
    """A host noise pointer with the categorical head; a normaliser with either head; A outside the head's range; more steps
    than ring rows: TrlError, the *_supported queries say 0, and nothing the launch could write was written."""
    import torch
    from torchrl_amd import _C
    lib = _C.lib()
    act = _C.ACT_TANH
    assert lib.trl_rollout_cat_supported(17, 64, 6, act) == 1 and lib.trl_rollout_sd_supported(17, 64, 6, act) == 1
    assert lib.trl_rollout_cat_supported(17, 64, 1, act) == 0 and lib.trl_rollout_cat_supported(17, 64, 9, act) == 0
    assert lib.trl_rollout_sd_supported(17, 64, 9, act) == 0
    dummy = torch.zeros(4096, dtype=torch.float64, device=DEV)

    def refused(c, edit):
        run = Launcher(c)
        a = run.args()
        edit(a)
        with pytest.raises(_C.TrlError):
            run.call(a)
        torch.cuda.synchronize()
        assert run.untouched()

    cat = R.rollout_case(17, 6, "tanh", False, 17, 5, 901, head="cat", noise="device")
    sd = R.rollout_case(17, 6, "tanh", True, 17, 5, 902, head="sd")
    refused(cat, lambda a: setattr(a, "noise", dummy.data_ptr()))

    def with_norm(a):
        a.norm_state, a.policy_obs, a.norm_workspace = dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr()
    refused(cat, with_norm)
    refused(sd, with_norm)
    refused(cat, lambda a: setattr(a, "A", 1))
    refused(cat, lambda a: setattr(a, "A", 9))
    refused(sd, lambda a: setattr(a, "A", 9))
    refused(cat, lambda a: setattr(a, "n_steps", cat["rows"] + 1))
    refused(sd, lambda a: setattr(a, "n_steps", sd["rows"] + 1))
