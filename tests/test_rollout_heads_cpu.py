"""CPU twin of tests/test_rollout_heads_gpu.py: pins the categorical and state-dependent-std restatements of
tests/_rollout_ref.py to the independent CPU rollouts (tests/_categorical_rollout_ref.py, tests/_gauss_sd_rollout_ref.py),
holds their float32 run to every bound the GPU file uses, asserts what the planted inputs are said to guarantee, and shows that
each of a list of subtly wrong implementations fails those bounds on at least one GPU case.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _categorical_ref as CR                                                 # noqa: E402
import _categorical_rollout_ref as crr                                        # noqa: E402
import _gauss_sd_rollout_ref as gsr                                           # noqa: E402
import _rollout_ref as R                                                      # noqa: E402
from oracle.synth_env import SynthVecEnvCPU                                   # noqa: E402

HEAD_CASES = R.head_cases()
IDS = [n for n, _ in HEAD_CASES]
CAT_CASES = [(n, kw) for n, kw in HEAD_CASES if kw["head"] == "cat"]
SD_CASES = [(n, kw) for n, kw in HEAD_CASES if kw["head"] == "sd"]


def ratios_ok(res, what):
    print("%s: worst err / bound %s" % (what, {k: round(float(v), 4) for k, v in res.items()}))
    bad = {k: v for k, v in res.items() if not k.startswith("_") and not v <= 1.0}
    assert not bad, (what, bad)


def zero_distance(r64):
    """The float64 chain sits at the restatement.  (The running returns are restated as float32 sums of the stored rewards: a
    float64 chain, whose rewards are no float32 numbers, is one more rounding per step away -- within twice their bound.  The
    epoch reward's bound is itself that of a float64 sum.)"""
    lim = dict(ep_return=2.0, ep_log=2.0, epoch_reward=1.0)
    assert all(v <= lim.get(k, 2e-3) for k, v in r64.items() if not k.startswith("_")), r64


def fresh_env_case(D, A, act, tanh, N, T, horizon, max_frames, env_seed, head, pf, vf, **kw):
    """A case that starts where a freshly reset SynthVecEnvCPU starts, with the given torch networks."""
    env = SynthVecEnvCPU(N, horizon=horizon, obs_dim=D, act_dim=A)
    env.seed(env_seed)
    c = R.rollout_case(D, A, act, tanh, N, T, env_seed, head=head, counters=R.quiet_counters, **kw)
    c.update(pf=[p.detach() for p in crr.linear_params(pf)], vf=[p.detach() for p in crr.linear_params(vf)], horizon=horizon,
             max_frames=max_frames, cur_obs=np.asarray(env.reset(), np.float32), rows=T, top=0, episode_idx=np.zeros(N, np.int32),
             ep_return=np.zeros(N, np.float32), epoch_reward0=0.0, ep_cap=256)
    return c


# ------------------------------------------------------------------ the float64 chain against the independent rollouts
def test_categorical_chain_is_the_independent_cpu_rollout():
    """`emulate` in float64 from a freshly reset env against `_categorical_rollout_ref.cpu_rollout` (float32 networks, the
    collector's bookkeeping, SynthVecEnvCPU) on a run without a borderline row: the same indices, everything else within the
    whole-trajectory bound 2e-5; `verify` finds the float64 chain at zero distance."""
    cc = dict(crr.PAIR_CASES[0], max_frames=7)
    N, T, horizon = 20, 12, 5
    nets = crr.nets_of(cc["D"], cc["A"], cc["act"], cc["net_seed"])
    want = crr.cpu_rollout(cc, N, T, horizon, nets=nets)
    assert not want["borderline"].any()
    c = fresh_env_case(cc["D"], cc["A"], cc["act"], False, N, T, horizon, 7, cc["env_seed"], "cat", *nets, noise="device",
                       cat_seed=crr.NOISE_SEED)
    o = R.emulate(c, np.float64)
    assert np.array_equal(o["acts"], want["acts"].astype(np.float64))
    for k in ("obs", "next_obs", "values", "rewards", "terminals", "time_limits", "old_logp"):
        err = np.abs(o[k] - want[k].astype(np.float64)).max()
        assert err < 2e-5, (k, err)
    assert abs(o["epoch_reward"] - sum(want["epoch_reward"])) < 1e-3
    assert o["ep_count"] == len(want["episodes"]) > 0
    np.testing.assert_allclose(o["ep_log"][:o["ep_count"]], np.asarray(want["episodes"], np.float64) + [[c["step0"], 0, 0]], atol=1e-4)
    r64 = R.verify(c, o)
    assert r64["_share_borderline"] == 0.0 and r64["_moved"] == 0.0
    zero_distance(r64)


@pytest.mark.parametrize("tanh", [True, False])
def test_state_std_chain_is_the_independent_cpu_rollout(tanh):
    """`emulate` in float64 against `_gauss_sd_rollout_ref.cpu_rollout` in float64 on the same host noise: both are float64
    chains of the same step, 1e-9; `verify` finds the chain at zero distance."""
    cc = dict(gsr.PAIR_CASES[0], max_frames=7, tanh=tanh)
    N, T, horizon = 20, 12, 5
    nets = gsr.nets_of(cc)
    c = fresh_env_case(cc["D"], cc["A"], cc["act"], tanh, N, T, horizon, 7, cc["env_seed"], "sd", *nets, noise="host")
    want = gsr.cpu_rollout(cc, N, T, horizon, nets, torch.from_numpy(c["eps"]), dtype=torch.float64)
    o = R.emulate(c, np.float64)
    for k in ("obs", "next_obs", "acts", "values", "rewards", "terminals", "time_limits", "old_logp"):
        err = np.abs(o[k] - want[k]).max()
        assert err < 1e-9, (k, err)
    assert o["ep_count"] == len(want["episodes"]) > 0
    np.testing.assert_allclose(o["ep_log"][:o["ep_count"]], np.asarray(want["episodes"], np.float64) + [[c["step0"], 0, 0]], atol=1e-4)
    zero_distance(R.verify(c, o))


# ------------------------------------------------------------------ the float32 run inside every bound
@pytest.mark.parametrize("name,kw", HEAD_CASES, ids=IDS)
def test_float32_run_meets_the_bounds(name, kw):
    """A correct float32 implementation meets every bound of `verify`, and moves at most the borderline actions."""
    c = R.rollout_case(**kw)
    res = R.verify(c, R.emulate(c, np.float32))
    ratios_ok(res, name)
    if kw["head"] == "cat":
        assert res["_share_borderline"] <= R.BORDERLINE_CAP


@pytest.mark.parametrize("head", ["cat", "sd"])
def test_float32_run_meets_the_bounds_over_two_device_noise_launches(head):
    c = R.two_launch_case(head)
    o = R.emulate(c, np.float32)
    ratios_ok(R.verify(c, o), "launch 1")
    c2 = R.continue_case(c, o, T=7)
    assert c2["noise_step0"] == 105 and c2["top"] == 13 and not np.array_equal(c2["eps"][:5], c["eps"])
    ratios_ok(R.verify(c2, R.emulate(c2, np.float32)), "launch 2")


# ------------------------------------------------------------------ what the inputs guarantee
@pytest.mark.parametrize("name,kw", HEAD_CASES, ids=IDS)
def test_conditions_on_the_inputs(name, kw):
    """On the float64 restatement's own run: at most BORDERLINE_CAP of the categorical cells are borderline (and HEAD_SEED_BUMP
    skips only seeds for which that fails); the planted events hit single envs in different steps and tiles; the stress heads
    put the stated shares of log_std elements on each clamp; at least a quarter of the tanh rows are inside logp_keep
    (`verify` asserts it)."""
    c = R.rollout_case(**kw)
    res = R.verify(c, R.emulate(c, np.float64))
    e = R.event_counts(c)
    print(name, e, {k: v for k, v in res.items() if k.startswith("_")})
    N, T = c["N"], c["T"]
    assert e["done"] >= 1
    if N >= 15:
        assert e["done"] >= 2 and e["over"] >= 2 and e["both"] >= 2 and e["quiet"] >= 2 * (N // 5) and e["mixed_tiles"] >= 1
        assert T == 1 or e["steps"] >= min(T, 3)
    if N >= 17:
        assert e["tiles"] >= 2
    if kw["head"] == "cat":
        assert res["_share_borderline"] <= R.BORDERLINE_CAP
        for b in range(R.HEAD_SEED_BUMP.get(name, 0)):                        # a recorded bump skips only seeds that fail
            cb = R.rollout_case(**dict(kw, seed=kw["seed"] - 1 - b))
            assert R.verify(cb, R.emulate(cb, np.float64))["_share_borderline"] > R.BORDERLINE_CAP
    else:
        assert name not in R.HEAD_SEED_BUMP
        entry = R.sd_stress_of(kw)
        hi, lo = ((0.0, 0.0), (0.0, 0.0)) if entry is None else entry[1:]
        lo = (1.0 / c["A"], 1.0 / c["A"]) if lo is None else lo
        assert hi[0] <= res["_share_hi"] <= hi[1] and lo[0] - 1e-12 <= res["_share_lo"] <= lo[1] + 1e-12
        assert res["_share_keep"] >= 0.25
        if c["tanh"]:
            assert float(np.abs(R.emulate(c, np.float64)["acts"][R.ring_rows(c)]).max()) < 1.0


def test_conditions_of_the_tie_peak_and_exact_threshold_cases():
    cases = dict(HEAD_CASES)
    # ties: the two rows are one float row, dominant; under noise both indices are drawn
    for name in ("cat-tie-det", "cat-tie"):
        c = R.rollout_case(**cases[name])
        A = c["A"]
        assert torch.equal(c["pf"][4][1], c["pf"][4][A - 1]) and float(c["pf"][5][1]) == float(c["pf"][5][A - 1])
        o = R.emulate(c, np.float32)
        k = o["acts"][R.ring_rows(c)].reshape(-1)
        if name == "cat-tie-det":
            assert (k == 1).all()
        else:
            assert (k == 1).mean() > 0.25 and (k == A - 1).mean() > 0.25
    # the peaked heads: logits of magnitude 30; with the bias every other term of the sum vanishes in float32
    for name, all_one in (("cat-peaked", False), ("cat-peaked-S1", True)):
        c = R.rollout_case(**cases[name])
        o = R.emulate(c, np.float64)
        lg = R.mlp(c["pf"], o["obs"][R.ring_rows(c)].reshape(-1, c["D"]), c["act"])
        assert 10.0 <= np.abs(np.delete(lg, 2, axis=1)).max() <= 60.0
        S32 = np.exp((lg - lg.max(1, keepdims=True)).astype(np.float32)).astype(np.float32).sum(1, dtype=np.float32)
        print(name, "share of cells whose float32 S is 1: %.3f" % (S32 == 1).mean())
        assert (S32 == 1).all() if all_one else (S32 == 1).any()
    # the exact threshold: u = 1/2 in EXACT_CELL, P_1 = 1 and S = 2 exactly there, in float64 and in float32
    c = R.rollout_case(**cases["cat-exact-threshold"])
    t, n = R.EXACT_CELL
    assert float(c["eps"][t, n, 0]) == 0.5 and int((c["eps"] == 0.5).sum()) == 1
    for dtype in (np.float64, np.float32):
        o = R.emulate(c, dtype)
        lg = torch.from_numpy(R.mlp(c["pf"], o["obs"][R.ring_rows(c)[t], n][None], c["act"], dtype))
        _, _, pre, S = CR.cat_act(lg, c["eps"][t, n].astype(dtype))
        assert float(pre[0, 1]) == 1.0 and float(pre[0, c["A"] - 2]) == 1.0 and float(S[0]) == 2.0
        assert o["acts"][R.ring_rows(c)[t], n, 0] == 1.0


# ------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("perturb", R.PERTURBATIONS)
def test_a_subtly_wrong_head_fails_the_bounds(perturb):
    """The float32 emulation with ONE named fault: on at least one GPU case a ratio of `verify` exceeds 1 or one of its exact
    assertions fires.  (The unperturbed run passes every case: test_float32_run_meets_the_bounds.)"""
    caught = []
    for name, kw in (CAT_CASES if perturb.startswith("cat") else SD_CASES):
        c = R.rollout_case(**kw)
        try:
            res = R.verify(c, R.emulate(c, np.float32, perturb=perturb))
            bad = {k: round(float(v), 2) for k, v in res.items() if not k.startswith("_") and not v <= 1.0}
            if bad:
                caught.append((name, bad))
        except AssertionError as e:
            caught.append((name, "assert: " + str(e)[:90]))
        if len(caught) >= 2:
            break
    print("%s caught by %s" % (perturb, caught))
    assert caught, perturb + " passes every case"
