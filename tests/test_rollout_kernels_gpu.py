"""The kernels the benchmark collects with, each called through torchrl_amd._C and compared with the float64 restatements of
tests/_rollout_ref.py, teacher-forced (every stored cell is restated from the launch's own obs[t, n] and the step's noise):

    trl_rollout_synth_f32      rollout_kernel<17, 64, 6, ACT, NORM> and the runtime-dims Gaussian instantiations,
                               value_pass_kernel (boot_values, publish_*)                      k_rollout.hip
    trl_gae_f32, trl_discount_reward_f32                                                       k_gae.hip

The bounds are those tests/test_rollout_kernels_cpu.py holds the float32 run of the restatements to; every test prints its
worst err / bound and hands it to `errlog` (profiles/NOTES_rollout_kernel_tests.md has one run's)."""
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

from _rollout_launch import DEV, GUARD, RING, Launcher, check, dev           # noqa: E402

pytestmark = pytest.mark.gpu
STEP_CASES = R.step_cases()


# ================================================================== 1. teacher-forced steps, no normaliser
@pytest.mark.parametrize("name,kw", STEP_CASES, ids=[n for n, _ in STEP_CASES])
def test_rollout_steps_against_the_restatement(name, kw, errlog):
    """Every instantiation, N around the 16-env tile, 1 / 5 / 12 steps, a ring that wraps inside the launch, envs out of step
    (tests/_rollout_ref.py::plant_counters): action, next observation, reward (raw and bootstrapped), log pi_old, V, boot
    values within their derived bounds; flags, counters, markers, chain identities, episode log, publish copy exact."""
    c = R.rollout_case(**kw)
    check(R.verify(c, Launcher(c).launch().read()), name, errlog)


def test_rollout_with_both_log_std_clamps(errlog):
    """log_std = +3 in the last column and -25 in the first (plain actions).  The action is compared in every column; log pi
    with the -25 column present is held to what the clamp allows for that column (`verify`), and compared with float64 in
    full from a second launch without it."""
    for lower in (True, False):
        c = R.rollout_case(17, 6, "tanh", False, 40, 5, 81, logstd=R.clamp_logstd(6, lower))
        check(R.verify(c, Launcher(c).launch().read(), lower_clamp_col=0 if lower else None), "clamps, lower=%s" % lower, errlog)


def test_rollout_device_philox_continues_over_two_launches(errlog):
    """Device noise keyed noise_step0 + t with noise_step0 = 100 > 0; the second launch continues the key, the ring and the
    env state."""
    c = R.rollout_case(17, 6, "tanh", True, 40, 5, 82, noise="device", noise_step0=100, rows=15, top=8)
    run = Launcher(c).launch()
    o = run.read()
    check(R.verify(c, o), "launch 1", errlog)
    c2 = R.continue_case(c, o, T=7)
    # (the second launch continues ON THE DEVICE: the same tensors, a ring re-filled with the sentinel, a fresh log)
    for v in run.ring.values():
        v.fill_(R.SENT)
    run.ep_count.zero_()
    run.ep_log.fill_(R.SENT)
    run.c = c2
    check(R.verify(c2, run.launch().read()), "launch 2", errlog)


# ================================================================== 2. the value pass
@pytest.mark.parametrize("name,kw", R.VALUE_CASES, ids=[n for n, _ in R.VALUE_CASES])
def test_value_pass_against_the_restatement(name, kw, errlog):
    """M = n_steps N below one tile, tiles that straddle time rows, exact tiles, the wide tile; no marker at all (the rewards
    stay the rollout's bits: `verify` compares them with the restated raw reward and the epoch sum with their double sum);
    boot_values = NULL; 5000 publish words on a one-workgroup grid."""
    c = R.rollout_case(**kw)
    o = Launcher(c).launch().read()
    check(R.verify(c, o), name, errlog)
    if name == "quiet":
        # never a second forward: the stored rewards are the raw rewards, and their double sum is the epoch's
        raw = o["rewards"][R.ring_rows(c)].astype(np.float64).sum()
        assert abs(o["epoch_reward"] - c["epoch_reward0"] - raw) <= c["T"] * c["N"] * 2.0 ** -53 * (abs(raw) + 12.5) * 8


def test_value_pass_second_round_of_tiles(errlog):
    """1031 envs x 33 steps = 34 023 cells = 2127 tiles on 2048 waves: 79 waves take a second tile.  Over-length cells in
    step 2 (first round) and in the last step (second round), whose V(next_obs) is also the boot row."""
    c = R.rollout_case(**R.BIG)
    check(R.verify(c, Launcher(c).launch().read()), "big", errlog)


# ================================================================== 3. the cooperative NORM path
def norm_max_envs(act):
    from torchrl_amd import _C
    return _C.lib().trl_rollout_norm_max_envs(17, 64, 6, _C.ACT_TANH if act == "tanh" else _C.ACT_RELU)


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("N", [16, 40, 200])
def test_norm_single_steps(act, N, errlog):
    """n_steps = 1 launches from planted cur_obs, policy_obs and state: no env resets; one single env resets (every env's
    policy input is raw); the same with normalize_partial_reset (filtered, statistics as without); norm_update = 0 (state
    bit-unchanged, the filter still applies), also with a reset env (the flag is then its tile's own: the env starts from
    its reset observation, raw or filtered); norm_clip = 0.5."""
    cap = norm_max_envs(act)
    print("trl_rollout_norm_max_envs(17, 64, 6, %s) = %d" % (act, cap))
    assert cap >= 2048
    variants = [dict(), dict(reset_env=N - 1), dict(reset_env=N // 2, partial_reset=1), dict(update=0),
                dict(update=0, reset_env=0), dict(update=0, reset_env=N - 1, partial_reset=1), dict(clip=0.5)]
    states = {}
    for k, v in enumerate(variants):
        c = R.norm_case(act, N, 200 + N, "centred", **v)
        o = Launcher(c, norm=True).launch().read()
        res = R.verify_norm_step(c, o)
        share = res.pop("_share_clamped")
        check(res, "N %d %s %s (clamped share %.3f)" % (N, act, v, share), errlog)
        assert (0.3 <= share <= 0.9) if v.get("clip") else share < 0.01
        states[k] = o["state"]
    assert not np.array_equal(states[0], G.norm_state_vec(R.norm_case(act, N, 200 + N)["state"]))     # the update did update


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("N", [16, 40, 200])
def test_norm_one_launch_of_five_steps_is_five_launches_of_one(act, N):
    """Bit-equal ring, state, policy_obs and env state: both parities of the partial slots, the fixed-order fold, resets in
    different steps on different envs (horizon 4, envs start at t_env = n % 3: no env resets in steps 0 and 4, a third of
    them in each step between)."""
    base = R.norm_case(act, N, 300 + N)
    c = dict(base, T=5, rows=7, top=4, horizon=4, t_env=(np.arange(N) % 3).astype(np.int32), ep_cap=256)
    c["eps"] = R.noise_block(c, 5)
    one = Launcher(c, norm=True).launch().read()
    five = Launcher(c, norm=True)
    for t in range(5):
        five.launch(T=1, top=(4 + t) % 7, noise_step0=t, eps=c["eps"][t:t + 1])
    five = five.read()
    resets = R.counters_walk(c)["flag"].sum(1).tolist()
    assert resets[0] == 0 and resets[4] == 0 and all(0 < r < N for r in resets[1:4]), resets
    for k in [k for k, _ in RING] + ["state", "policy_obs", "cur_obs", "t_env", "cur_step", "episode_idx", "ep_return", "ep_count"]:
        assert np.array_equal(np.asarray(one[k]), np.asarray(five[k])), k
    assert not (one["state"] == G.norm_state_vec(c["state"])).all()


@pytest.mark.parametrize("level", ["basin", "offset", "centred"])
@pytest.mark.parametrize("N", [64, 200])
def test_norm_conditioning(level, N, errlog):
    """Four chained single steps.  basin: every observation +0.995 +- 1e-3 (env_A = 3 I, env_B = 0.05) and a state warmed on
    that distribution -- sums about zero in float32 leave the batch variance 16 % off there (the CPU twin runs that
    arithmetic); offset: 0.9 +- 1e-2; centred.  Held to the Normalizer kernels' tolerances: state rel 1e-11, filtered output
    rtol 2e-7 + atol 1e-7."""
    c = R.norm_case("tanh", N, 91, level)
    run = Launcher(c, norm=True)
    worst = {}
    for step in range(4):
        o = run.launch(noise_step0=c["noise_step0"]).read()
        res = R.verify_norm_step(c, o)
        res.pop("_share_clamped")
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in res.items()}
        c = R.continue_case(c, o)
        run.c = c
        for v in run.ring.values():
            v.fill_(R.SENT)
    check(worst, "%s N %d, four steps" % (level, N), errlog)


# ================================================================== 4. GAE and discounted return
def gpu_scan(g, mode, filt, use_lt):
    from torchrl_amd import _C
    T, N = g["T"], g["N"]
    full = [torch.full((T * N + GUARD,), R.SENT, device=DEV) for _ in range(2)]
    adv, ret = (f[:T * N].view(T, N) for f in full)
    args = (dev(g["r"]), dev(g["v"]), dev(g["d"]), dev(g["tl"]), dev(g["lv"]), adv, ret, g["gamma"])
    lt = dev(g["lt"]) if use_lt else None
    if mode == "gae":
        _C.gae(*args, g["tau"], filt, last_terminal=lt)
    else:
        _C.discount_reward(*args, filt, last_terminal=lt)
    torch.cuda.synchronize()
    assert all(bool((f[T * N:] == R.SENT).all()) for f in full), "guard overwritten"
    return adv.cpu().numpy(), ret.cpu().numpy()


def scan_worst(g):
    """-> {mode / filter: worst err / bound over adv, ret, with and without last_terminal}"""
    worst = {}
    for mode in ("gae", "disc"):
        for filt in (0, 1):
            for use_lt in (False, True):
                adv, ret = gpu_scan(g, mode, filt, use_lt)
                key = "%s%d" % (mode, filt)
                worst[key] = max(worst.get(key, 0.0), *R.scan_ratios(g, mode, filt, use_lt, adv, ret))
    return worst


@pytest.mark.parametrize("T,N", R.GAE_SHAPES)
def test_scan_against_the_restatement(T, N, errlog):
    """Both kernels, both filters, with and without last_terminal, per element within the bound recurrence
    (tests/_rollout_ref.py::_scan_bound).  T around the 64 lanes and the 256-step chunk, N giving 1, 2, 13 and 17 tiles (the
    last two: an uneven deal to the XCDs); planted terminals at T - 1, T - 256, T - 257, an env with none, an env with one
    at every step."""
    worst = scan_worst(R.gae_case(T, N, 1000 + 7 * T + N))
    print("T %d N %d: worst err / bound %s" % (T, N, {k: round(v, 3) for k, v in worst.items()}))
    for k, v in worst.items():
        errlog(k, v, 1.0)
    assert max(worst.values()) <= 1.0, worst


def test_scan_growth_and_grid_cases(errlog):
    """gamma = tau = 1 without terminals at T = 700: the sum grows linearly and the bound follows it.  On the grid of 1/8 at
    T = 8 float32 is exact: equality."""
    g = R.gae_case(700, 9, 3, gamma=1.0, tau=1.0, plain=True)
    for mode in ("gae", "disc"):
        adv, ret = gpu_scan(g, mode, 0, False)
        worst = max(R.scan_ratios(g, mode, 0, False, adv, ret))
        print("gamma = tau = 1, T 700, %s: worst err / bound %.3f, largest |y| %.1f" % (mode, worst, np.abs(adv).max()))
        errlog("growth_" + mode, worst, 1.0)
        assert worst <= 1.0
    g = R.grid_case()
    for mode in ("gae", "disc"):
        for filt in (0, 1):
            adv, ret = gpu_scan(g, mode, filt, True)
            wa, wr, _ = (R.gae_ref if mode == "gae" else R.discount_ref)(g, filt, True)
            assert np.array_equal(adv.astype(np.float64), wa) and np.array_equal(ret.astype(np.float64), wr), (mode, filt)
