"""The shared-std Gaussian loss kernel, the per-step collection kernels and the observation normaliser, each called
through torchrl_amd._C and compared with the restatements of tests/_gauss_ref.py run in float64 (numpy for the integer
bookkeeping: exact equality):

    trl_ppo_generic_losses_f32                       k_ppo_generic.hip, trl_ppo_loss.h
    trl_gauss_explore_f32, trl_gauss_logp_f32        k_rollout.hip
    trl_onpolicy_bookkeep_f32, trl_select_on_flag_f32, trl_select_on_mask_f32     k_rollout.hip
    trl_collector_bookkeep_f32                       k_sac.hip
    trl_norm_update_filt_f32, trl_norm_batch_moments_f64, trl_norm_merge_f64, trl_norm_shard_moments_f64,
    trl_norm_shard_merge_f64, trl_norm_filt_f32      k_norm.hip

The bounds are those tests/test_gauss_collector_kernels_cpu.py holds the float32 run of the restatements to; every test
prints its worst err / bound and hands it to `errlog` (profiles/NOTES_gauss_collector_kernel_tests.md has one run's)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_ref as R                                                        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64 = torch.float64
GUARD = 64                                                                    # sentinel elements behind an output


def dev(x):
    return None if x is None else torch.as_tensor(np.asarray(x)).to(DEV).contiguous()


def host(t):
    return t.detach().cpu().double()


def guarded(n, value, dtype=torch.float32):
    """(view of the first n elements, whole buffer): the kernel gets the view, the test looks at the rest."""
    full = torch.full((n + GUARD,), value, dtype=dtype, device=DEV)
    return full[:n], full


def guard_intact(full, n, value):
    return bool((full[n:] == value).all())


# ================================================================== 1. trl_ppo_generic_losses_f32
def gpu_losses(c, tanh, loss_mode, clipv, clip=0.2, c_ent=0.01, workspace=None, garbage=1e30):
    """-> dict(d_mean, d_v, d_logstd (float64 on the host), info (numpy)); d_logstd and the info row are pre-filled."""
    from torchrl_amd import _C
    A = c["mean"].shape[1]
    old, v_old = R.loss_args(c, loss_mode, clipv)
    d_logstd = torch.full((A,), garbage, dtype=torch.float32, device=DEV)
    info = torch.full((24,), R.SENTINEL, dtype=F64, device=DEV)
    d_mean, d_v = _C.ppo_generic_losses(dev(c["mean"]), dev(c["logstd"]), dev(c["acts"]), dev(c["advs"]), dev(old), dev(c["v"]),
                                        dev(c["rets"]), dev(v_old), dev(c["adv_raw"]), c["n_global"], clip, c_ent, clipv, tanh,
                                        loss_mode, d_logstd, info, workspace=workspace)
    torch.cuda.synchronize()
    return dict(d_mean=host(d_mean), d_v=host(d_v).reshape(-1), d_logstd=host(d_logstd), info=info.cpu().numpy())


def loss_grid():
    for B in R.LOSS_B:
        for A in R.LOSS_A:
            for combo in R.COMBOS:
                yield (B, A) + combo
    for combo in R.CROSS:
        yield (300, 6) + combo


def seed_of(B, A, n_mult):
    return 1000 + 7 * A + B + 100000 * n_mult


@pytest.mark.parametrize("n_mult", [1, 3])
@pytest.mark.parametrize("B,A,tanh,loss_mode,clipv", list(loss_grid()))
def test_losses_against_the_restatement(B, A, tanh, loss_mode, clipv, n_mult, errlog):
    """d_mean, d_v, d_logstd and the 24 info slots; one block (B <= 256), the block edge, two and three blocks with a ragged
    tail (the fold of d_logstd and of the twelve scalars), A up to PG_MAX_A, n_global = B and 3 B.  Bounds:
    _gauss_ref.loss_error_ratios."""
    c = R.loss_case(B, A, tanh, seed_of(B, A, n_mult), n_mult)
    want = R.run_losses_ref(c, tanh, loss_mode, clipv, F64)
    got = gpu_losses(c, tanh, loss_mode, clipv)
    assert got["d_mean"].shape == (B, A) and all(bool(torch.isfinite(got[k]).all()) for k in ("d_mean", "d_v", "d_logstd"))
    r = R.loss_error_ratios(got, want, B, c["n_global"])
    print("B %d A %d n_global %d: worst err / bound %s" % (B, A, c["n_global"], {k: round(v, 3) for k, v in r.items()}))
    for k, v in r.items():
        errlog(k, v, 1.0)
    assert all(v <= 1.0 for v in r.values()), r
    assert all(got["info"][k] == R.SENTINEL for k in (20, 21, 22, 23))     # not written for a Gaussian head


def test_clamped_log_std_columns_get_no_gradient():
    """Raw log_std -25 and +3: the gate closes d_logstd there exactly (the entropy term included), the other columns are
    non-zero, the statistics see the clamped values, everything is finite."""
    B, A = 300, 6
    c = R.loss_case(B, A, False, 31)
    c["logstd"][1], c["logstd"][4] = -25.0, 3.0
    c["acts"] = R.explore(c["mean"], c["logstd"], torch.from_numpy(np.random.RandomState(5).randn(B, A).astype(np.float32)), False)[0]
    c["old"] = R.logp(c["mean"], c["logstd"], c["acts"], False) + 0.1
    got = gpu_losses(c, False, R.LOSS_PPO_CLIP, False)
    assert all(bool(torch.isfinite(got[k]).all()) for k in ("d_mean", "d_v", "d_logstd")) and np.isfinite(got["info"][:20]).all()
    assert got["d_logstd"][1] == 0.0 and got["d_logstd"][4] == 0.0
    assert all(got["d_logstd"][o] != 0.0 for o in (0, 2, 3, 5))
    assert got["info"][10] == 2.0 and got["info"][11] == -20.0
    assert got["info"][18] == pytest.approx(np.exp(2.0), rel=1e-12) and got["info"][19] == pytest.approx(np.exp(-20.0), rel=1e-12)
    want = R.run_losses_ref(c, False, R.LOSS_PPO_CLIP, False, F64)
    r = R.loss_error_ratios(got, want, B, c["n_global"])
    print("clamped columns: worst err / bound %s" % r)
    assert r["d_logstd"] <= 1.0 and r["d_v"] <= 1.0 and r["info"] <= 1.0


@pytest.mark.parametrize("loss_mode", [R.LOSS_PPO_CLIP, R.LOSS_A2C])
def test_one_action_dimension_has_nan_std_slots_and_nothing_else(loss_mode):
    c = R.loss_case(70, 1, True, 8)
    got = gpu_losses(c, True, loss_mode, True)
    nan = [k for k in range(24) if np.isnan(got["info"][k])]
    assert nan == [9, 17], nan
    assert all(bool(torch.isfinite(got[k]).all()) for k in ("d_mean", "d_v", "d_logstd"))


@pytest.mark.parametrize("B_pad", [0, 300])
def test_value_loss_ties_and_gates_are_exact(B_pad):
    """Exactly representable inputs (grid of 1/8, clip 0.25, n_global 16 / 512): v == v_old (weight 0.5 each), v - v_old ==
    +-clip (gate open), outside the clip with either term larger and with both equal (the tie weight 0.5 shows only there:
    elsewhere a tie has v as its clipped value).  d_v * n_global equals the restatement's, bit for bit;
    B_pad more rows repeat the planted ones into a second block."""
    t = R.value_tie_case()
    rep = 1 + B_pad // len(t["kind"])
    v, v_old, rets = (t[k].repeat(rep) for k in ("v", "v_old", "rets"))
    B = v.numel()
    ng = 16.0 if B_pad == 0 else 512.0
    c = R.loss_case(B, 2, False, 77)
    c.update(v=v, v_old=v_old, rets=rets, n_global=ng, adv_raw=R.adv_raw_of(torch.cat([c["advs"], torch.zeros(int(ng) - B)])))
    got = gpu_losses(c, False, R.LOSS_PPO_CLIP, True, clip=t["clip"])
    want = R.run_losses_ref(c, False, R.LOSS_PPO_CLIP, True, F64, clip=t["clip"])
    assert torch.equal(got["d_v"] * ng, want["d_v"].double() * ng)
    kinds = t["kind"] * rep
    dv = got["d_v"] * ng
    for i in range(len(t["kind"])):
        vv, vo, Rr = float(v[i]), float(v_old[i]), float(rets[i])
        expect = {"tie": vv - Rr, "gate+": vv - Rr, "gate-": vv - Rr, "out_l1": vv - Rr, "out_l2": 0.0,
                  "out_tie": 0.5 * (vv - Rr), "in": vv - Rr}[kinds[i]]
        assert float(dv[i]) == expect, (i, kinds[i])
    assert got["info"][7] == float(want["info"][7])                       # the value-loss sum: exact terms, added in double


@pytest.mark.parametrize("B,n_mult", [(256, 1), (512, 1), (256, 3)])
def test_constant_advantages(B, n_mult):
    """All advantages 0.3f: the normalised advantage is exactly 0, d_mean exactly 0, and d_logstd is the entropy term alone:
    B (a power of two: its float32 sums are exact) times fl(c_ent fl(1 / n_global)), c_ent as the float32 the kernel is
    given -- two roundings, within one ulp of -c_ent B / n_global."""
    A, c_ent = 6, 0.01
    c = R.loss_case(B, A, True, 12)
    c["advs"] = torch.full((B,), 0.3, dtype=torch.float32)
    c["n_global"] = float(n_mult * B)
    c["adv_raw"] = R.adv_raw_of(torch.full((n_mult * B,), 0.3, dtype=torch.float32))
    got = gpu_losses(c, True, R.LOSS_PPO_CLIP, False, c_ent=c_ent)
    assert bool((got["d_mean"] == 0).all()) and got["info"][0] == 0.0
    want = -float(np.float32(c_ent)) * B / c["n_global"]
    err = (got["d_logstd"] - want).abs().max().item()
    print("constant advantages: d_logstd %.9g want %.9g (err %.3e, one ulp %.3e)" % (got["d_logstd"][0], want, err, 2 ** -23 * abs(want)))
    assert err <= 2.0 ** -23 * abs(want)
    assert all(bool(torch.isfinite(got[k]).all()) for k in ("d_mean", "d_v", "d_logstd")) and np.isfinite(got["info"][:20]).all()


@pytest.mark.parametrize("tanh", [True, False])
@pytest.mark.parametrize("A", [1, 6, 64])
def test_ratio_is_exactly_one_against_the_log_prob_kernel(A, tanh):
    """trl_mlp.h's promise: log pi_old from trl_gauss_logp_f32 and log pi inside the loss kernel are the same bits on the
    same (mean, action, log_std), so ratio/max == ratio/min == 1.  A2C mode without old_logp reports 1 too."""
    from torchrl_amd import _C
    B = 300
    c = R.loss_case(B, A, tanh, 40 + A)
    c["old"] = _C.gauss_logp(dev(c["mean"]), dev(c["acts"]), dev(c["logstd"]), tanh).cpu()
    got = gpu_losses(c, tanh, R.LOSS_PPO_CLIP, False)
    assert got["info"][5] == 1.0 and got["info"][6] == -1.0
    got = gpu_losses(c, tanh, R.LOSS_A2C, False)
    assert got["info"][5] == 1.0 and got["info"][6] == -1.0


def test_outputs_are_overwritten_and_runs_are_bit_equal():
    """d_logstd and the info row are stores, not accumulations (two different garbage pre-fills give the same bits), two
    runs are bit-equal, and a workspace larger than needed changes nothing."""
    from torchrl_amd import _C
    B, A = 700, 33
    c = R.loss_case(B, A, True, 21)
    need = _C.lib().trl_ppo_generic_losses_workspace(B, A)
    assert need == 3 * (A + 12)
    runs = [gpu_losses(c, True, R.LOSS_PPO_CLIP, True, garbage=g, workspace=w)
            for g, w in ((1e30, None), (-3.5, None), (float("nan"), torch.full((need + 1000,), 1e300, dtype=F64, device=DEV)))]
    for r in runs[1:]:
        for k in ("d_mean", "d_v", "d_logstd"):
            assert torch.equal(r[k], runs[0][k]), k
        assert np.array_equal(r["info"], runs[0]["info"])


def test_loss_kernel_refusals():
    from torchrl_amd import _C
    c = R.loss_case(8, 2, True, 2)
    big = dict(c, mean=torch.zeros(8, 65), acts=torch.zeros(8, 65), logstd=torch.zeros(65))
    with pytest.raises(_C.TrlError):
        gpu_losses(big, True, R.LOSS_PPO_CLIP, False)
    with pytest.raises(_C.TrlError):
        gpu_losses(dict(c, n_global=1.0), True, R.LOSS_PPO_CLIP, False)
    with pytest.raises(_C.TrlError):
        gpu_losses(dict(c, old=None), True, R.LOSS_PPO_CLIP, False)
    with pytest.raises(_C.TrlError):
        gpu_losses(dict(c, v_old=None), True, R.LOSS_A2C, True)
    gpu_losses(c, True, R.LOSS_PPO_CLIP, True)                             # and the unbroken call goes through


# ================================================================== 2. trl_gauss_explore_f32 / trl_gauss_logp_f32
def check_logp(name, lp, mean, logstd, act, tanh, errlog, keep_all=False):
    """lp (device) against the float64 restatement at the float32 action `act`, on the rows `logp_keep` covers."""
    want = R.logp(mean.double(), logstd.double(), act.double(), tanh)
    keep = (torch.ones_like(want, dtype=torch.bool) if keep_all else R.logp_keep(act, tanh)) & torch.isfinite(want)
    got = host(lp)
    assert bool((torch.isfinite(got) == torch.isfinite(want)).all())
    assert int(keep.sum()) >= max(1, act.shape[0] // 4)
    bound = R.logp_bound(mean, logstd, act, tanh)[keep]
    r = float(((got - want).abs()[keep] / bound).max())
    print("%s: %d of %d rows, log pi err / bound %.3f (bound %.2e .. %.2e, |log pi| median %.1f)"
          % (name, int(keep.sum()), act.shape[0], r, float(bound.min()), float(bound.max()), float(want[keep].abs().median())))
    errlog(name, r, 1.0)
    assert float(bound.max()) <= 1e-3 * max(1.0, float(want[keep].abs().median()))          # the bound has teeth
    return r


@pytest.mark.parametrize("tanh", [True, False])
@pytest.mark.parametrize("A", R.EXPLORE_A)
@pytest.mark.parametrize("N", R.EXPLORE_N)
def test_explore_against_the_restatement(N, A, tanh, errlog):
    """act against float64 (`act_bound`: the std is that of the CLAMPED log_std -- the unclamped one is more than 100
    bounds away, tests/test_gauss_collector_kernels_cpu.py), log pi finite where float64 at the kernel's own action is,
    and bit-equal to trl_gauss_logp_f32 on (mean, that action); with and without eps.  Log pi against float64
    (`logp_bound`) under `logstd_lp`: for tanh actions a second call without the column clamped at -20, where log pi is
    float32 atanh noise over e^-40 and no bound says anything."""
    from torchrl_amd import _C
    c = R.explore_case(N, A, tanh, 50 + A + N)
    mean, ls = c["mean"], c["logstd"]
    for eps in (c["eps"], None):
        act_v, act_full = guarded(N * A, -9.0)
        lp_v, lp_full = guarded(N, -9.0)
        act, lp = _C.gauss_explore(dev(mean), dev(ls), dev(eps), tanh, act=act_v.view(N, A), logp=lp_v)
        torch.cuda.synchronize()
        assert guard_intact(act_full, N * A, -9.0) and guard_intact(lp_full, N, -9.0)
        want_act = R.explore(mean.double(), ls.double(), None if eps is None else eps.double(), tanh)[0]
        r_act = float(((host(act) - want_act).abs() / R.act_bound(mean, ls, eps, tanh)).max()) if (eps is not None or tanh) else 0.0
        if eps is None and not tanh:
            assert torch.equal(act.cpu(), mean)                               # fma(std, 0, mean)
        tag = "N%d_A%d_tanh%d_eps%d" % (N, A, tanh, eps is not None)
        print("%s: act err / bound %.3f" % (tag, r_act))
        errlog("act_" + tag, r_act, 1.0)
        lp2 = _C.gauss_logp(dev(mean), act.contiguous(), dev(ls), tanh)
        assert np.array_equal(lp2.cpu().numpy(), lp.cpu().numpy())           # every row, saturated ones included
        lsp = c["logstd_lp"]
        if not torch.equal(lsp, ls):
            want = R.logp(mean.double(), ls.double(), act.cpu().double(), tanh)
            assert bool((torch.isfinite(lp.cpu()) == torch.isfinite(want)).all())
            act, lp = _C.gauss_explore(dev(mean), dev(lsp), dev(eps), tanh)
            lp2 = _C.gauss_logp(dev(mean), act.contiguous(), dev(lsp), tanh)
            assert np.array_equal(lp2.cpu().numpy(), lp.cpu().numpy())
        r_lp = check_logp("logp_" + tag, lp, mean, lsp, act.cpu(), tanh, errlog)
        assert r_act <= 1.0 and r_lp <= 1.0


@pytest.mark.parametrize("tanh", [True, False])
@pytest.mark.parametrize("A", R.EXPLORE_A)
@pytest.mark.parametrize("N", R.EXPLORE_N)
def test_logp_alone_against_the_restatement(N, A, tanh, errlog):
    """trl_gauss_logp_f32 on seeded stored actions (drawn by the float32 restatement, tanh actions clamped to +-0.995),
    under `logstd_lp`."""
    from torchrl_amd import _C
    c = R.explore_case(N, A, tanh, 900 + A + N)
    c["logstd"] = c["logstd_lp"]
    acts = R.explore(c["mean"], c["logstd"], c["eps"], tanh)[0]
    if tanh:
        acts = acts.clamp(-0.995, 0.995)
    out_v, out_full = guarded(N, -9.0)
    lp = _C.gauss_logp(dev(c["mean"]), dev(acts), dev(c["logstd"]), tanh, out=out_v)
    torch.cuda.synchronize()
    assert guard_intact(out_full, N, -9.0)
    assert check_logp("N%d_A%d_tanh%d" % (N, A, tanh), lp, c["mean"], c["logstd"], acts, tanh, errlog, keep_all=True) <= 1.0


@pytest.mark.parametrize("A", [1, 6])
def test_pre_tanh_values_up_to_seven(A, errlog):
    """|z| in [3, 7] planted through the means: the action stays below 1, log pi is finite and inside `logp_bound` against
    float64 at that action (the atanh part of the bound is derived for |a| <= 0.995 only; the ratio printed here says how
    far it carries)."""
    from torchrl_amd import _C
    N = 300
    c = R.big_z_case(N, A, 70 + A)
    act, lp = _C.gauss_explore(dev(c["mean"]), dev(c["logstd"]), dev(c["eps"]), True)
    a = act.cpu()
    assert float(a.abs().max()) < 1.0 and float(a.abs().min()) > 0.99 and bool(torch.isfinite(lp).all())
    assert check_logp("A%d" % A, lp, c["mean"], c["logstd"], a, True, errlog, keep_all=True) <= 1.0


# ================================================================== 3. bookkeeping and select kernels
class Book:
    """Device buffers of one collector's bookkeeping; ep_log has `extra` sentinel rows behind the ep_cap the kernel is told."""

    def __init__(self, N, cur_step, ep_return, ep_cap, epoch0=100.0, any0=0, extra=4):
        self.N, self.cap = N, ep_cap
        self.cur_step, self.ep_return = dev(cur_step.copy()), dev(ep_return.copy())
        self.mask = torch.full((N,), 7, dtype=torch.uint8, device=DEV)
        self.terminals = torch.full((N,), -9.0, device=DEV)
        self.any_flag = torch.full((1,), any0, dtype=torch.int32, device=DEV)
        self.epoch = torch.full((1,), epoch0, dtype=F64, device=DEV)
        self.ep_count = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.log_full = torch.full((ep_cap + extra, 3), -5.0, device=DEV)
        self.ep_log = self.log_full[:ep_cap]

    def call(self, c, step, discount=None):
        from torchrl_amd import _C
        rew = dev(c["rew"].copy())
        if discount is None:
            _C.collector_bookkeep(rew, dev(c["done"]), self.cur_step, self.ep_return, c["max_frames"], self.mask, self.epoch,
                                  self.ep_count, self.ep_log, step)
        else:
            _C.onpolicy_bookkeep(rew, dev(c["done"]), dev(c["v_next"]), discount, self.terminals, self.cur_step, self.ep_return,
                                 c["max_frames"], self.mask, self.any_flag, self.epoch, self.ep_count, self.ep_log, step)
        torch.cuda.synchronize()
        return rew.cpu().numpy()

    def log_rows(self):
        rows = self.log_full.cpu().numpy()
        return rows[:self.cap], rows[self.cap:]


def as_sorted(rows):
    return sorted((float(s), float(n), float(r)) for s, n, r in rows)


@pytest.mark.parametrize("onpolicy", [True, False])
@pytest.mark.parametrize("N", R.BOOK_N)
def test_bookkeeping_equals_the_restatement(N, onpolicy):
    """Two chained calls (step 0 and 1) of trl_onpolicy_bookkeep_f32 / trl_collector_bookkeep_f32: cur_step, ep_return, the
    reset mask, terminals and the any-flag exactly; the epoch sum exactly (rewards on a grid of 1/8: any order of the atomics
    gives the same double); the episode log as a set; rewards bit-equal where no episode ran over its length, and there
    within the two float32 roundings of raw + discount * v_next (the product's and the sum's, each half an ulp)."""
    discount = 0.99 if onpolicy else None
    c = R.bookkeep_case(N, 90 + N)
    b = Book(N, c["cur_step"], c["ep_return"], ep_cap=2 * N)
    logs, epoch = [], 100.0
    for step in (0, 1):
        want = R.bookkeep(c, step, discount)
        rew = b.call(c, step, discount)
        assert np.array_equal(b.cur_step.cpu().numpy(), want["cur_step"])
        assert np.array_equal(b.ep_return.cpu().numpy(), want["ep_return"])
        assert np.array_equal(b.mask.cpu().numpy(), want["mask"])
        epoch += want["epoch"]
        assert float(b.epoch.item()) == epoch
        logs += want["log"]
        assert int(b.ep_count.item()) == len(logs)
        got_rows, behind = b.log_rows()
        assert as_sorted(got_rows[:len(logs)]) == sorted(logs) and np.all(got_rows[len(logs):] == -5.0) and np.all(behind == -5.0)
        if onpolicy:
            assert np.array_equal(b.terminals.cpu().numpy(), want["terminals"])
            assert int(b.any_flag.item()) == (1 if step == 1 else want["any"])   # an OR: the caller clears it
            sp = want["surpass"]
            assert np.array_equal(rew[~sp], c["rew"][~sp])
            dv = np.float64(np.float32(discount)) * c["v_next"].astype(np.float64)
            bound = 2.0 ** -24 * (np.abs(dv) + np.abs(want["rew64"]))
            assert np.all(np.abs(rew.astype(np.float64) - want["rew64"])[sp] <= bound[sp])
            assert sp.sum() >= (min(N, 6) // 2 if step == 0 else 2 * (N >= 6))
        else:
            assert np.array_equal(rew, c["rew"])                                # the off-policy kernel reads rewards only
        nxt = R.bookkeep_case(N, 190 + N)                                        # the next step's rewards / dones
        c = dict(nxt, cur_step=want["cur_step"], ep_return=want["ep_return"])
        if N >= 6:                                                               # keep over-length rows in the second step
            c["cur_step"] = c["cur_step"].copy()
            c["cur_step"][1:3] = [c["max_frames"] - 1, c["max_frames"] + 5]
            b.cur_step.copy_(dev(c["cur_step"]))


@pytest.mark.parametrize("onpolicy", [True, False])
def test_episode_log_overflow(onpolicy):
    """More finished episodes than ep_cap: the counter counts all of them, exactly ep_cap rows are written -- each the
    (step, env, return) of a different finished env -- and the rows behind keep their sentinel."""
    N, cap = 257, 5
    c = R.bookkeep_case(N, 7)
    c["done"][:] = 1.0
    c["done"][10] = 0.0
    b = Book(N, c["cur_step"], c["ep_return"], ep_cap=cap)
    want = R.bookkeep(c, 3, 0.99 if onpolicy else None)
    b.call(c, 3, 0.99 if onpolicy else None)
    assert int(b.ep_count.item()) == N - 1 == len(want["log"])
    rows, behind = b.log_rows()
    assert np.all(behind == -5.0)
    assert len({r[1] for r in as_sorted(rows)}) == cap and all(r in set(want["log"]) for r in as_sorted(rows))
    assert np.array_equal(b.ep_return.cpu().numpy(), want["ep_return"]) and np.array_equal(b.mask.cpu().numpy(), want["mask"])


@pytest.mark.parametrize("N,row", [(1, 0), (257, 256), (257, 70), (1000, 999)])
def test_any_flag_and_zero_rewards(N, row):
    """any_flag goes 0 -> 1 exactly when a row is flagged (here one row, in the last wave / another block); a 1 already there
    stays when no row is flagged.  All-zero rewards leave epoch_reward's bits alone (both kernels)."""
    c = R.bookkeep_case(N, 5)
    c["done"][:] = 0.0
    c["cur_step"][:] = 0
    c["rew"][:] = 0.0
    for any0, flagged in ((0, False), (1, False), (0, True)):
        cc = dict(c, done=c["done"].copy())
        if flagged:
            cc["done"][row] = 1.0
        b = Book(N, cc["cur_step"], cc["ep_return"], ep_cap=4, epoch0=0.1, any0=any0)
        b.call(cc, 0, 0.99)
        assert int(b.any_flag.item()) == (1 if (any0 or flagged) else 0)
        assert b.epoch.cpu().numpy().tobytes() == np.array([0.1]).tobytes()
        assert int(b.mask.sum().item()) == int(flagged) and int(b.ep_count.item()) == int(flagged)
        b2 = Book(N, cc["cur_step"], cc["ep_return"], ep_cap=4, epoch0=0.1)
        b2.call(cc, 0)
        assert b2.epoch.cpu().numpy().tobytes() == np.array([0.1]).tobytes() and int(b2.mask.sum().item()) == int(flagged)


def test_reward_shortcut_edges_of_the_on_policy_kernel():
    """rew = raw + discount * v_next * (over-length ? 1 : 0), float32, as the reference's numpy line: on rows that did not
    run over their length the product is a zero only when v_next is finite.  The kernel has the reference's behaviour at both
    observable edges: a reward of -0.0 takes the sign of the product's zero (+0.0 next to a positive v_next, -0.0 next to a
    negative one), and a non-finite v_next makes the reward NaN whether or not the episode ran over its length (the value
    network's output is the caller's to keep finite).  Bit for bit the float32 numpy line on every finite row.  Everything else -- counters,
    mask, returns, the epoch sum of the RAW rewards -- is what the restatement says."""
    N = 70
    c = R.bookkeep_case(N, 3)
    c["done"][:] = 0.0
    c["cur_step"][:] = 0
    c["cur_step"][5] = c["max_frames"] - 1                                     # one over-length row with a finite value
    c["rew"][0], c["rew"][1], c["rew"][2], c["rew"][65] = -0.0, 1.0, -0.0, 2.0
    c["v_next"][0], c["v_next"][2] = 1.0, -1.0
    c["v_next"][1], c["v_next"][65], c["v_next"][66] = np.inf, np.nan, -np.inf
    c["rew"][66] = 0.0
    b = Book(N, c["cur_step"], c["ep_return"], ep_cap=4)
    rew = b.call(c, 0, 0.99)
    with np.errstate(invalid="ignore"):
        want = c["rew"] + np.float32(0.99) * c["v_next"] * (c["cur_step"] + 1 >= c["max_frames"]).astype(np.float32)
    assert want.dtype == np.float32 and np.isnan(want[[1, 65, 66]]).all() and np.isfinite(np.delete(want, [1, 65, 66])).all()
    assert np.array_equal(np.isnan(rew), np.isnan(want))
    ok = ~np.isnan(want)
    ok[5] = False
    assert rew[ok].tobytes() == want[ok].tobytes() and np.array_equal(rew[ok], c["rew"][ok])
    assert np.signbit(c["rew"][[0, 2]]).all() and not np.signbit(rew[0]) and np.signbit(rew[2])
    assert abs(float(rew[5]) - float(want[5])) <= 2.0 ** -23 * abs(float(want[5]))
    o = R.bookkeep(c, 0, 0.99)
    assert np.array_equal(b.mask.cpu().numpy(), o["mask"]) and np.array_equal(b.cur_step.cpu().numpy(), o["cur_step"])
    assert np.array_equal(b.ep_return.cpu().numpy(), o["ep_return"]) and float(b.epoch.item()) == 100.0 + o["epoch"]


def test_bookkeeping_wrappers_want_an_epoch_reward():
    """The C entries take epoch_reward == NULL; the Python wrappers do not (every collector passes one)."""
    from torchrl_amd import _C
    c = R.bookkeep_case(4, 1)
    b = Book(4, c["cur_step"], c["ep_return"], ep_cap=4)
    b.epoch = None
    with pytest.raises(_C.TrlError):
        b.call(c, 0, 0.99)
    with pytest.raises(_C.TrlError):
        b.call(c, 0)


@pytest.mark.parametrize("flag", [0, 1, -7])
@pytest.mark.parametrize("n", [1, 257, 300000])
def test_select_on_flag(n, flag):
    """n = 300000 is past the grid cap of 1024 x 256: the stride loop takes a second trip."""
    from torchrl_amd import _C
    rs = np.random.RandomState(n)
    a, b = dev(rs.randn(n).astype(np.float32)), dev(rs.randn(n).astype(np.float32))
    out, full = guarded(n, -9.0)
    _C.select_on_flag(torch.tensor([flag], dtype=torch.int32, device=DEV), a, b, out)
    torch.cuda.synchronize()
    assert torch.equal(out, a if flag != 0 else b) and guard_intact(full, n, -9.0)


@pytest.mark.parametrize("L", [1, 255, 256, 257, 5000])
def test_select_on_mask(L):
    """The only set byte at index 0 or at the last index (beyond the first 256 for L > 256), value 1 or 0x80; n = 70000 is
    past the grid cap of 256 x 256."""
    from torchrl_amd import _C
    for n in (1, 257, 70000):
        rs = np.random.RandomState(n + L)
        a, b = dev(rs.randn(n).astype(np.float32)), dev(rs.randn(n).astype(np.float32))
        for where, value in ((None, 0), (0, 1), (0, 0x80), (L - 1, 1), (L - 1, 0x80)):
            mask = torch.zeros(L, dtype=torch.uint8, device=DEV)
            if where is not None:
                mask[where] = value
            out, full = guarded(n, -9.0)
            _C.select_on_mask(mask, a, b, out)
            torch.cuda.synchronize()
            assert torch.equal(out, a if where is not None else b), (n, where, value)
            assert guard_intact(full, n, -9.0)


# ================================================================== 4. the observation normaliser
def fresh_state(D):
    from torchrl_amd.env.base_wrapper import Normalizer
    return Normalizer((D,), device=DEV).state.clone()


def three_launches(x, state, sums, clip, shard=False):
    """moments + merge + filt as launches of their own; shard: the pair env shards all-reduce between."""
    from torchrl_amd import _C
    if shard:
        _C.norm_shard_moments(x, state, sums)
        _C.norm_shard_merge(state, sums, x.shape[1])
    else:
        _C.norm_batch_moments(x, sums)
        _C.norm_merge(state, sums, x.shape[1])
    return _C.norm_filt(x, state, torch.empty_like(x), clip)


@pytest.mark.parametrize("D", R.NORM_D)
@pytest.mark.parametrize("N", R.NORM_N)
def test_normaliser_against_the_restatement(D, N, errlog):
    """Three batches from the Normalizer's initial state.  D sets the thread layout (R = 1024 / D row lanes, 1024 - R D idle
    threads: 4 at D = 17, 1 at D = 33, none at 1 and 64), N = 1, 2 and 15 leave row lanes without a row.  The one-launch and
    the three-launch path leave bit-equal states and outputs; state rel 1e-11 and output rtol 2e-7 / atol 1e-7 against the
    float64 two-pass restatement (the tolerances of test_normalizer_matches_oracle_at_full_size), for them and for the
    shard pair (sums about the running mean, what several ranks all-reduce); inputs of +-1e6 come out as exactly +-clip."""
    from torchrl_amd import _C
    clip = 10.0
    one, split, shard = fresh_state(D), fresh_state(D), fresh_state(D)
    assert np.array_equal(one.cpu().numpy(), R.norm_state_vec(R.norm_init(D)))
    sums = torch.zeros(2 * D + 1, dtype=F64, device=DEV)
    want = R.norm_init(D)
    worst_s = worst_o = 0.0
    for x in R.norm_batches(D, N, 11 * D + N):
        xd = dev(x)
        out_v, out_full = guarded(N * D, -9.0)
        out = _C.norm_update_filt(xd, one, out_v.view(N, D), clip, True)
        out2 = three_launches(xd, split, sums, clip)
        assert float(sums[2 * D].item()) == N
        out3 = three_launches(xd, shard, sums, clip, shard=True)
        torch.cuda.synchronize()
        assert guard_intact(out_full, N * D, -9.0)
        assert torch.equal(one, split) and torch.equal(out, out2)
        assert float(sums[2 * D].item()) == N
        want = R.norm_update(want, x)
        ws, wo = R.norm_state_vec(want), R.norm_filt(want, x, clip)
        for st, o in ((one, out), (shard, out3)):
            worst_s = max(worst_s, float((np.abs(st.cpu().numpy() - ws) / (R.NORM_STATE_RTOL * np.abs(ws))).max()))
            worst_o = max(worst_o, float((np.abs(o.cpu().numpy() - wo) / (R.NORM_OUT_ATOL + R.NORM_OUT_RTOL * np.abs(wo))).max()))
    print("D %d N %d: state err / tol %.4f, output err / tol %.3f" % (D, N, worst_s, worst_o))
    errlog("state", worst_s, 1.0)
    errlog("out", worst_o, 1.0)
    assert worst_s <= 1.0 and worst_o <= 1.0
    # filter only: +-1e6 come out as +-clip exactly, the state stays; both filter entries
    big = R.norm_batches(D, N, 5)[0]
    big[0, 0], big[N - 1, D - 1] = 1e6, (-1e6 if N * D > 1 else 1e6)
    before = one.clone()
    o1 = _C.norm_update_filt(dev(big), one, torch.empty(N, D, device=DEV), clip, False)
    o2 = _C.norm_filt(dev(big), one, torch.empty(N, D, device=DEV), clip)
    assert torch.equal(one, before) and torch.equal(o1, o2)
    assert float(o1[0, 0]) == clip and float(o1[N - 1, D - 1]) == (-clip if N * D > 1 else clip)
    wo = R.norm_filt(want, big, clip)
    np.testing.assert_allclose(o1.cpu().numpy(), wo, rtol=R.NORM_OUT_RTOL, atol=R.NORM_OUT_ATOL)


@pytest.mark.parametrize("D,N", [(17, 1000), (3, 5000), (64, 5000)])
def test_normaliser_conditioning(D, N, errlog):
    """Observations 1000 + 0.01 N(0, 1) merged into a state that has seen one such batch (its float64 mean and variance,
    count N), and into the fresh state.  Sums about zero would have an amplification (mean^2 + var) / var of 1e10 -- bound
    amplification * chain * 2^-53 ~ 1e-4 on the batch variance, and from the warm state a filtered output several tolerances
    off (the CPU twin runs that order of additions).  The kernels add in two passes, about the batch mean: variance inside
    the grid's rel 1e-11, output inside the grid's rtol 2e-7 / atol 1e-7, from both states.  The shard pair adds about the
    running mean: the same from the warm state; from the fresh one its centre is 0 and the variance has the bound about
    zero, which count = 1e-4 hides from the output (it puts mean^2 1e-4 into the first variance)."""
    from torchrl_amd import _C
    clip = 10.0
    warm, x = R.norm_conditioning_batches(N, D, 3)
    amp0, chain, bound0 = R.norm_conditioning(x, N, D)
    for name, st in (("warm", R.norm_warm_state(warm)), ("fresh", R.norm_init(D))):
        one, split, shard = (dev(R.norm_state_vec(st)) for _ in range(3))
        sums = torch.zeros(2 * D + 1, dtype=F64, device=DEV)
        out = _C.norm_update_filt(dev(x), one, torch.empty(N, D, device=DEV), clip, True)
        out2 = three_launches(dev(x), split, sums, clip)
        out3 = three_launches(dev(x), shard, sums, clip, shard=True)
        assert torch.equal(one, split) and torch.equal(out, out2)
        want = R.norm_update(st, x)
        wo = R.norm_filt(want, x, clip)
        for path, state, o in (("two_pass", one, out), ("shard", shard, out3)):
            got = state.cpu().numpy()
            var_err = float((np.abs(got[D:2 * D] - want[1]) / want[1]).max())
            mean_err = float((np.abs(got[:D] - want[0]) / np.abs(want[0])).max())
            r_out = float((np.abs(o.cpu().numpy() - wo) / (R.NORM_OUT_ATOL + R.NORM_OUT_RTOL * np.abs(wo))).max())
            # the grid's state tolerance (the restatement itself rounds a batch mean of size 1000: 1e-13 of a delta of 3e-4);
            # the shard pair from the fresh state: centre 0, the bound about zero
            tol = bound0 if (path, name) == ("shard", "fresh") else R.NORM_STATE_RTOL
            print("D %d N %d %s state, %s: about zero amplification %.3e chain %d bound %.3e; variance rel err %.3e (tol "
                  "%.1e), mean rel err %.3e, output err / tol %.3f" % (D, N, name, path, amp0, chain, bound0, var_err, tol,
                                                                      mean_err, r_out))
            errlog("var_%s_%s" % (path, name), var_err, tol)
            errlog("out_%s_%s" % (path, name), r_out, 1.0)
            assert var_err <= tol and mean_err <= R.NORM_STATE_RTOL and r_out <= 1.0


def test_normaliser_no_op_paths_and_refusals():
    from torchrl_amd import _C
    D, N = 17, 15
    x = dev(R.norm_batches(D, N, 1)[1])
    state = fresh_state(D)
    before = state.clone()
    out = _C.norm_update_filt(x, state, torch.empty(N, D, device=DEV), 10.0, False)
    assert torch.equal(state, before)                                            # update=False: bit-unchanged
    np.testing.assert_allclose(out.cpu().numpy(), R.norm_filt(R.norm_init(D), x.cpu().numpy(), 10.0), rtol=2e-7, atol=1e-7)
    assert _C.norm_update_filt(x, state, None, 10.0, True) is None               # out=None: the state alone
    want = R.norm_state_vec(R.norm_update(R.norm_init(D), x.cpu().numpy()))
    np.testing.assert_allclose(state.cpu().numpy(), want, rtol=R.NORM_STATE_RTOL, atol=0)
    x65, s65 = torch.zeros(4, 65, device=DEV), torch.zeros(131, dtype=F64, device=DEV)
    x0 = torch.zeros(0, D, device=DEV)
    sums = torch.zeros(2 * D + 1, dtype=F64, device=DEV)
    for bad in (lambda: _C.norm_update_filt(x65, s65, torch.empty_like(x65), 10.0, True),
                lambda: _C.norm_batch_moments(x65, s65),
                lambda: _C.norm_shard_moments(x65, s65, s65),
                lambda: _C.norm_merge(s65, s65, 65),
                lambda: _C.norm_shard_merge(s65, s65, 65),
                lambda: _C.norm_filt(x65, s65, torch.empty_like(x65), 10.0),
                lambda: _C.norm_update_filt(x0, state, torch.empty_like(x0), 10.0, True),
                lambda: _C.norm_batch_moments(x0, sums),
                lambda: _C.norm_shard_moments(x0, state, sums)):
        with pytest.raises(_C.TrlError):
            bad()
    _C.norm_filt(x0, state, torch.empty_like(x0), 10.0)                          # N = 0 is a no-op there
