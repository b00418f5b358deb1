"""The fused state-dependent-std rollout without a GPU: the two new symbols and the argument checks of
trl_rollout_synth_sd_f32 (every case returns before anything is launched; fails on a build without the entry point), the
float32 restatement against the float64 one on the exact cases of the GPU tests and inside their bounds, and the share of
log_std elements the stress heads put on each clamp."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_sd_ref as ref                                                   # noqa: E402
import _gauss_sd_rollout_ref as rr                                            # noqa: E402


@pytest.fixture(scope="module")
def built_lib():
    from torchrl_amd import build
    return build.build(verbose=False)


# ---------------------------------------------------------------- entry point
def test_supported_shapes_at_the_edges(built_lib):
    from torchrl_amd import _C
    lib = _C.lib()
    assert _C.SIGNATURES["trl_rollout_synth_sd_f32"] == (C.c_int, [C.POINTER(_C.RolloutArgs), C.c_void_p])
    assert _C.SIGNATURES["trl_rollout_sd_supported"] == (C.c_int, [C.c_int] * 4)
    ok = lib.trl_rollout_sd_supported
    for act in (_C.ACT_TANH, _C.ACT_RELU):
        for A, want in ((0, 0), (1, 1), (8, 1), (9, 0)):
            assert ok(17, 64, A, act) == want, A
        for D, want in ((1, 0), (2, 1), (32, 1), (33, 0)):
            assert ok(D, 64, 6, act) == want, D
        assert ok(17, 63, 6, act) == 0 and ok(17, 64, 6, act) == 1
    assert ok(17, 64, 6, _C.ACT_NONE) == 0
    header = open(os.path.join(os.path.dirname(HERE), "include", "trl_hip.h")).read()
    assert "int trl_rollout_synth_sd_f32(const trl_rollout_t* args, void* stream);" in header
    assert "int trl_rollout_sd_supported(int D, int H, int A, int act);" in header


def _descriptor():
    """A descriptor whose pointers are never dereferenced: every call below returns from the host-side checks."""
    from torchrl_amd import _C
    a = _C.RolloutArgs()
    for k in ("pf_params", "vf_params", "env_A", "env_B", "cur_obs", "t_env", "cur_step", "episode_idx", "ep_return",
              "ep_count", "ep_log"):
        setattr(a, k, 0x1000)
    a.D, a.H, a.A, a.act = 17, 64, 6, _C.ACT_TANH
    a.N, a.n_steps, a.rows, a.top = 32, 0, 1, 0
    a.horizon, a.max_episode_frames, a.ep_cap = 5, 5, 8
    return a


def test_argument_checks_return_before_any_launch(built_lib):
    from torchrl_amd import _C
    lib = _C.lib()
    EINVAL, EUNSUPPORTED = -1, -2
    call = lambda a: lib.trl_rollout_synth_sd_f32(C.byref(a), None)
    assert call(_descriptor()) == 0                                          # n_steps == 0: nothing to do, nothing launched
    assert lib.trl_rollout_synth_sd_f32(None, None) == EINVAL
    assert b"null descriptor" in lib.trl_last_error()

    def bad(code, needle, **kw):
        a = _descriptor()
        a.n_steps = 4                                                         # (a good descriptor would launch from here on)
        for k, v in kw.items():
            setattr(a, k, v)
        assert call(a) == code, kw
        assert needle in lib.trl_last_error(), lib.trl_last_error()

    bad(EINVAL, b"null", pf_params=None)
    bad(EINVAL, b"ring", obs=0x1000)                                         # some ring tensors but not all
    bad(EINVAL, b"normaliser", norm_state=0x1000)
    bad(EINVAL, b"staged", stage_n=16)
    bad(EINVAL, b"staged", noise=0x1000, noise_flag=0x1000)
    for kw in (dict(A=9), dict(A=0), dict(D=33), dict(D=1), dict(H=63), dict(act=_C.ACT_NONE)):
        bad(EUNSUPPORTED, b"not instantiated", **kw)


# ---------------------------------------------------------------- the GPU tests' inputs stay inside their bounds
def _report(label, worst):
    for k, (ratio, err) in worst.items():
        print("%s %s: max abs err %.3e, worst err / bound %.4f" % (label, k, err, ratio))
    bad = {k: v for k, v in worst.items() if not v[0] <= 1.0}
    assert not bad, (label, bad)


TRAJECTORIES = [(c, m) for c in rr.PAIR_CASES for m in ("host", "device")] + [(rr.CPU_CASE, "host")] + \
    [(c, "device") for c in rr.WIDE_RELU_CASES]


@pytest.mark.parametrize("case,mode", TRAJECTORIES, ids=["%s-%s" % (rr.case_id(c), m) for c, m in TRAJECTORIES])
def test_float32_rollouts_stay_inside_the_trajectory_bounds(case, mode):
    N, steps, horizon = (rr.PAIR_N, rr.PAIR_T * rr.PAIR_EPOCHS, rr.PAIR_HORIZON)
    if case is rr.CPU_CASE:
        N, steps, horizon = rr.CPU_N, rr.CPU_T, rr.CPU_HORIZON
    if case in rr.WIDE_RELU_CASES:
        N, steps, horizon = rr.WIDE_RELU_N, rr.WIDE_RELU_T * rr.PAIR_EPOCHS, rr.WIDE_RELU_HORIZON
    nets = rr.nets_of(case)
    eps = rr.noise_of(mode, steps, N, case["A"], case["env_seed"])
    lo, hi = (rr.cpu_rollout(case, N, steps, horizon, nets, eps, dt) for dt in (torch.float32, torch.float64))
    _report("%s %s" % (rr.case_id(case), mode), {k: rr.worst_ratio(lo[k], hi[k], *tol) for k, tol in rr.TOL.items()})
    assert len(lo["episodes"]) == len(hi["episodes"]) and (len(hi["episodes"]) > 0) == (case["max_frames"] >= horizon)
    np.testing.assert_allclose([r for _, _, r in lo["episodes"]], [r for _, _, r in hi["episodes"]], rtol=0, atol=1e-5 * horizon)
    assert abs(sum(lo["epoch_reward"]) - sum(hi["epoch_reward"])) <= 1e-5 * steps * N
    assert hi["terminals"].sum() > 0
    if case["max_frames"] < horizon:
        assert hi["time_limits"].sum() == 0                                  # the over-length bootstrap fires, `done` never
    else:
        assert hi["time_limits"].sum() == hi["terminals"].sum()
    std = np.exp(np.clip(rr.forward(rr.params_of(nets[0], torch.float64), hi["obs"].reshape(steps * N, -1), case["act"],
                                    torch.float64).detach().numpy()[:, case["A"]:], -20, 2))
    assert 0.9 < std.min() and std.max() < 1.1                               # the default initialiser: std ~ 1


def _stress_steps(case, mode):
    """(obs (M, D), eps (M, A)) of the stress test: the float32 rollout's own observations, as a ring would hold them."""
    N, T = rr.STRESS_N, rr.STRESS_T
    nets = rr.nets_of(case)
    eps = rr.noise_of(mode, T, N, case["A"], case["env_seed"])
    out = rr.cpu_rollout(case, N, T, rr.STRESS_HORIZON, nets, eps, torch.float32)
    return nets, out["obs"].reshape(T * N, -1), eps.reshape(T * N, -1).numpy()


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("case", rr.STRESS_CASES, ids=rr.case_id)
def test_float32_steps_stay_inside_the_stress_bounds(case, mode):
    nets, obs, eps = _stress_steps(case, mode)
    want = rr.step_terms(case, rr.params_of(nets[0], torch.float64), obs, eps)
    got = rr.step_terms_f32(case, rr.params_of(nets[0], torch.float32), obs, eps)
    worst = {}
    for k, b in (("act", "b_act"), ("next_obs", "b_next"), ("reward", "b_rew")):
        err = np.abs(got[k].astype(np.float64) - want[k])
        worst[k] = (float((err / want[b]).max()), float(err.max()))
    keep = ~(want["raw"] <= -20.0).any(axis=1)                              # rows without an element on the lower clamp
    if keep.any():
        lp64 = ref.logp(torch.from_numpy(want["head"]), torch.from_numpy(got["act"]).double(), False)[0].numpy()
        worst["old_logp"] = rr.worst_ratio(got["old_logp"][keep], lp64[keep], 1e-4, 2e-3)
    _report("%s %s" % (rr.case_id(case), mode), worst)
    assert np.isfinite(got["old_logp"]).all() and np.isfinite(got["act"]).all()


# ---------------------------------------------------------------- the stress heads reach the clamps
@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("case", rr.STRESS_CASES, ids=rr.case_id)
def test_stress_heads_reach_the_clamps(case, mode):
    nets, obs, eps = _stress_steps(case, mode)
    raw = rr.step_terms(case, rr.params_of(nets[0], torch.float64), obs, eps)["raw"]
    hi, lo = float((raw >= 2.0).mean()), float((raw <= -20.0).mean())
    print("%s %s: %d elements, share at +2: %.4f, at -20: %.4f, raw in [%.2f, %.2f]"
          % (rr.case_id(case), mode, raw.size, hi, lo, raw.min(), raw.max()))
    assert case["share_hi"][0] <= hi <= case["share_hi"][1] and hi > 0
    assert case["share_lo"][0] - 1e-12 <= lo <= case["share_lo"][1] + 1e-12
    if case["stress"] == "pinned":
        A = case["A"]
        assert lo > 0 and (raw[:, A - 1] <= -20.0).all() and not (raw[:, :A - 1] <= -20.0).any()
        assert (raw[:, 0] >= 2.0).mean() > 0.5                               # b3 = +3: mostly on the upper clamp
    # no element is ill-conditioned without being exempt: off the lower clamp the std stays above e^-4
    assert raw[raw > -20.0].min() > -4.0
