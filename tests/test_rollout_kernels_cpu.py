"""CPU twin of tests/test_rollout_kernels_gpu.py: pins the restatements of tests/_rollout_ref.py to the oracle
(oracle/collector.py + oracle/synth_env.py, oracle/replay.py), holds their float32 run to every bound the GPU file uses,
and asserts what the planted inputs are said to guarantee.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_ref as G                                                        # noqa: E402
import _rollout_ref as R                                                      # noqa: E402
from oracle import replay                                                     # noqa: E402
from oracle.collector import VecOnPolicyCollectorOracle                       # noqa: E402
from oracle.synth_env import SynthVecEnvCPU                                   # noqa: E402

STEP_CASES = R.step_cases()


def ratios_ok(res, what):
    shown = {k: round(v, 4) for k, v in res.items()}
    print("%s: worst err / bound %s" % (what, shown))
    bad = {k: v for k, v in res.items() if not k.startswith("_") and not v <= 1.0}
    assert not bad, (what, bad)


# ------------------------------------------------------------------ the restatement against the oracle
@pytest.mark.parametrize("D,A,act", [(17, 6, "tanh"), (5, 3, "relu")])
def test_chained_restatement_is_the_oracle_collector(D, A, act):
    """`emulate` from a freshly reset env, in float32 and in float64, against SynthVecEnvCPU + VecOnPolicyCollectorOracle on
    the same noise (float32 bounds of the whole-trajectory tests: 2e-5); and `verify` (step_terms, teacher-forced) finds the
    float64 chain at zero distance."""
    N, T, horizon, max_frames, seed = 20, 12, 5, 7, 4
    c = R.rollout_case(D, A, act, True, N, T, seed, counters=R.quiet_counters)
    env = SynthVecEnvCPU(N, horizon=horizon, obs_dim=D, act_dim=A)
    env.seed(seed)
    ring = replay.RingOracle(N * T, env_nums=N, time_limit_filter=True)
    col = VecOnPolicyCollectorOracle(env, ring, c["pf"], c["logstd"], c["vf"], epoch_frames=N * T, max_episode_frames=max_frames,
                                     discount=c["discount"], act=act)
    c.update(horizon=horizon, max_frames=max_frames, cur_obs=np.asarray(col.current_ob, np.float32), rows=T, top=0,
             episode_idx=np.zeros(N, np.int32), ep_return=np.zeros(N, np.float32), epoch_reward0=0.0, ep_cap=256)
    res = col.train_one_epoch(noise=torch.from_numpy(c["eps"]))
    for dtype in (np.float32, np.float64):
        o = R.emulate(c, dtype)
        for k in ("obs", "next_obs", "acts", "values", "rewards", "terminals", "time_limits"):
            err = np.abs(o[k] - np.asarray(ring.data[k], np.float64).reshape(o[k].shape)).max()
            assert err < 2e-5, (k, err)
        assert abs(o["epoch_reward"] - float(res["train_epoch_reward"])) < 1e-3
        assert o["ep_count"] == len(res["train_rewards"]) > 0
        np.testing.assert_allclose(o["ep_log"][:o["ep_count"], 2], np.asarray(res["train_rewards"], np.float64).reshape(-1), atol=1e-4)
        np.testing.assert_allclose(o["cur_obs"], col.current_ob, atol=2e-5)
    r64 = R.verify(c, o)
    # (the running returns are restated as float32 sums: a float64 chain sits inside their bound, not at zero)
    assert all(v < 2e-3 if k not in ("ep_return", "ep_log") else v <= 1.0 for k, v in r64.items()), r64


# ------------------------------------------------------------------ the float32 run inside every bound
@pytest.mark.parametrize("name,kw", STEP_CASES + R.VALUE_CASES, ids=[n for n, _ in STEP_CASES + R.VALUE_CASES])
def test_float32_run_meets_the_bounds(name, kw):
    c = R.rollout_case(**kw)
    ratios_ok(R.verify(c, R.emulate(c, np.float32)), name)


def test_float32_run_meets_the_bounds_with_clamped_log_std():
    for lower in (True, False):
        c = R.rollout_case(17, 6, "tanh", False, 40, 5, 81, logstd=R.clamp_logstd(6, lower))
        ratios_ok(R.verify(c, R.emulate(c, np.float32), lower_clamp_col=0 if lower else None), "clamp lower=%s" % lower)


def test_float32_run_meets_the_bounds_over_two_device_noise_launches():
    c = R.rollout_case(17, 6, "tanh", True, 40, 5, 82, noise="device", noise_step0=100, rows=15, top=8)
    o = R.emulate(c, np.float32)
    ratios_ok(R.verify(c, o), "launch 1")
    c2 = R.continue_case(c, o, T=7)
    assert c2["noise_step0"] == 105 and c2["top"] == 13 and not np.array_equal(c2["eps"][:5], c["eps"])
    ratios_ok(R.verify(c2, R.emulate(c2, np.float32)), "launch 2")


# ------------------------------------------------------------------ what the inputs guarantee
@pytest.mark.parametrize("name,kw", STEP_CASES, ids=[n for n, _ in STEP_CASES])
def test_planted_events_and_action_range(name, kw):
    """Envs out of step: each kind of event on single envs, in different steps and tiles; some value-pass tile with marker
    cells next to cells without one; every float64 |tanh z| <= 0.995."""
    c = R.rollout_case(**kw)
    e = R.event_counts(c)
    print(name, e)
    N, T = c["N"], c["T"]
    assert e["done"] >= min(1, N // 1) and e["done"] + e["over"] + e["both"] <= 3 * N
    if N >= 15:
        assert e["done"] >= 2 and e["over"] >= 2 and e["both"] >= 2 and e["quiet"] >= 2 * (N // 5)
        assert e["mixed_tiles"] >= 1
        if T > 1:
            assert e["steps"] >= min(T, 3)
    if N >= 17:
        assert e["tiles"] >= 2
    o = R.emulate(c, np.float64)
    if c["tanh"]:
        amax = float(np.abs(o["acts"][R.ring_rows(c)]).max())
        assert amax <= 0.995, amax


def test_clamp_shares_and_markers_of_the_special_cases():
    c = R.rollout_case(17, 6, "tanh", False, 40, 5, 81, logstd=R.clamp_logstd(6))
    ls = c["logstd"]
    assert int((ls > 2).sum()) == 1 and int((ls < -20).sum()) == 1        # one column on each clamp: 1 / 6 of the elements each
    # the unclamped +3 column would move the action by far more than its bound
    o = R.emulate(c, np.float64)
    M = c["T"] * c["N"]
    st = R.step_terms(c, o["obs"][R.ring_rows(c)].reshape(M, 17), o["obs"][R.ring_rows(c)].reshape(M, 17), c["eps"].reshape(M, 6))
    moved = np.abs((np.exp(3.0) - np.exp(2.0)) * c["eps"].reshape(M, 6)[:, 5])
    assert np.median(moved / st["b_act"][:, 5]) > 100
    # no marker at all in the quiet case; the large case has markers in both rounds of tiles and its boot row in the second
    assert R.event_counts(R.rollout_case(**dict(R.VALUE_CASES)["quiet"]))["over"] == 0
    big = R.rollout_case(**R.BIG)
    w = R.counters_walk(big)
    m = np.nonzero(w["over"].reshape(-1))[0]
    n_tiles = (big["T"] * big["N"] + 15) // 16
    assert n_tiles > R.VP_TILES_PER_ROUND and not w["done"].any()
    assert (m // 16 < R.VP_TILES_PER_ROUND).sum() >= 100 and (m // 16 >= R.VP_TILES_PER_ROUND).sum() >= 100
    assert ((big["T"] - 1) * big["N"]) // 16 >= R.VP_TILES_PER_ROUND


# ------------------------------------------------------------------ the normaliser: conditioning
@pytest.mark.parametrize("N", [64, 200])
def test_parent_arithmetic_fails_the_conditioning_case(N):
    """Four steps of the basin case in float64.  The arithmetic the kernel had (float32 16-env sums of x and x^2, widened,
    sum x^2 / n - mean^2) misses the state tolerance on the variance by more than ten times in every step; the sums about
    the running mean in double meet it, here and on the two ordinary levels."""
    for level in ("basin", "offset", "centred"):
        c = R.norm_case("tanh", N, 91, level)
        worst_parent, worst_fixed = 0.0, 0.0
        for step in range(4):
            st = R.step_terms(c, c["policy_obs"], c["cur_obs"], c["eps"][0])
            x = st["next_obs"].astype(np.float32)
            want = G.norm_update(c["state"], x)
            ep = R.state_errors(R.norm_update_parent(c["state"], x), want)
            ef = R.state_errors(R.norm_update_fixed(c["state"], x), want)
            worst_parent, worst_fixed = max(worst_parent, ep[1]), max(worst_fixed, max(ef))
            if level == "basin":
                assert ep[1] > 10 * G.NORM_STATE_RTOL, (step, ep)
                assert float(np.abs(x - 0.995).max()) < 3e-3 and float(x.std(0).max()) < 2e-3
            assert max(ef) <= G.NORM_STATE_RTOL, (level, step, ef)
            c = dict(c, state=want, cur_obs=x, policy_obs=G.norm_filt(want, x, c["norm_clip"]).astype(np.float32), salt=step + 1)
            c["eps"] = R.noise_block(c, 1)
        print("N %d %s: variance rel err, parent arithmetic %.3e, sums about the running mean %.3e (tolerance %.0e)"
              % (N, level, worst_parent, worst_fixed, G.NORM_STATE_RTOL))


def test_norm_clip_half_fires_on_a_stated_share():
    c = R.norm_case("tanh", 40, 92, "centred", clip=0.5)
    st = R.step_terms(c, c["policy_obs"], c["cur_obs"], c["eps"][0])
    new = G.norm_update(c["state"], st["next_obs"])
    share = float((np.abs(G.norm_filt(new, st["next_obs"], 0.5)) == 0.5).mean())
    print("share of clamped elements at clip 0.5: %.3f" % share)
    assert 0.3 <= share <= 0.9


# ------------------------------------------------------------------ GAE / discounted return
def test_gae_ref_is_replay_gae():
    g = R.gae_case(65, 9, 1, gamma=0.5, tau=0.25)                      # (float32 == float64 for these two)
    sh = lambda x: np.asarray(x, np.float64)[..., None]
    for filt in (0, 1):
        wa, wr = replay.gae(sh(g["r"]), sh(g["v"]), sh(g["d"]), sh(g["tl"]), sh(g["lv"]), 0.5, 0.25, bool(filt))
        a, r, _ = R.gae_ref(g, filt, False)
        assert np.array_equal(a, wa[..., 0]) and np.array_equal(r, wr[..., 0])
        wa, wr = replay.discounted_return(sh(g["r"]), sh(g["v"]), sh(g["d"]), sh(g["tl"]), sh(g["lv"]), 0.5, bool(filt))
        a, r, _ = R.discount_ref(g, filt, False)
        assert np.array_equal(a, wa[..., 0]) and np.array_equal(r, wr[..., 0])


@pytest.mark.parametrize("T,N", R.GAE_SHAPES)
def test_float32_scan_meets_the_bound_and_rows_are_planted(T, N):
    g = R.gae_case(T, N, 1000 + 7 * T + N)
    d, tl = g["d"], g["tl"]
    if N >= 7:
        assert d[T - 1, 0] == 1 and d[:, 4].sum() == 0 and d[:, 5].all() and g["lt"][6] == 1 and g["lt"][4] == 0
        assert (tl[:, 5].sum() > 0 or T == 0) and (T < 2 or tl[1, 5] == 0)
        if T >= 257:
            assert d[T - 256, 1] == 1 and d[T - 257, 2] == 1 and tl[T - 256, 1] == 1 and d[T - 256, 3] == 1 and tl[T - 256, 3] == 0
    assert ((tl == 1) <= (d == 1)).all()
    worst = 0.0
    for mode in ("gae", "disc"):
        for filt in (0, 1):
            for use_lt in (False, True):
                adv, ret = R.scan_f32(g, mode, filt, use_lt)
                worst = max(worst, *R.scan_ratios(g, mode, filt, use_lt, adv, ret))
    print("T %d N %d: float32 recurrence, worst err / bound %.3f" % (T, N, worst))
    assert worst <= 1.0


def test_float32_scan_growth_case_and_grid_case():
    g = R.gae_case(700, 9, 3, gamma=1.0, tau=1.0, plain=True)
    for mode in ("gae", "disc"):
        adv, ret = R.scan_f32(g, mode, 0, False)
        ra, rr = R.scan_ratios(g, mode, 0, False, adv, ret)
        _, _, b = (R.gae_ref if mode == "gae" else R.discount_ref)(g, 0, False)
        print("gamma = tau = 1, T 700, %s: err / bound %.3f %.3f; bound at t = 0 / t = T - 1: %.2e / %.2e"
              % (mode, ra, rr, b[0].max(), b[-1].max()))
        assert ra <= 1.0 and rr <= 1.0 and b[0].max() > 50 * b[-1].max()          # the bound follows the growing sum
    g = R.grid_case()
    for mode in ("gae", "disc"):
        for filt in (0, 1):
            adv, ret = R.scan_f32(g, mode, filt, True)
            wa, wr, _ = (R.gae_ref if mode == "gae" else R.discount_ref)(g, filt, True)
            assert np.array_equal(adv.astype(np.float64), wa) and np.array_equal(ret.astype(np.float64), wr)
