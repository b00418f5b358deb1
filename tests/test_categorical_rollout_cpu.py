"""The fused categorical rollout without a GPU: the two new symbols and their ctypes signatures, the argument checks
of trl_rollout_synth_cat_f32 (every case returns before anything is launched), and the borderline share of the
GPU tests' cases on the CPU restatement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _categorical_rollout_ref as rr                                         # noqa: E402


@pytest.fixture(scope="module")
def built_lib():
    from torchrl_amd import build
    return build.build(verbose=False)


def test_new_symbols_and_signatures(built_lib):
    from torchrl_amd import _C
    lib = _C.lib()
    assert _C.SIGNATURES["trl_rollout_synth_cat_f32"] == (C.c_int, [C.POINTER(_C.RolloutArgs), C.c_int64, C.c_int64, C.c_void_p])
    assert _C.SIGNATURES["trl_rollout_cat_supported"] == (C.c_int, [C.c_int] * 4)
    for name in ("trl_rollout_synth_cat_f32", "trl_rollout_cat_supported"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _C.SIGNATURES[name][1]
    header = open(os.path.join(os.path.dirname(HERE), "include", "trl_hip.h")).read()
    assert "int trl_rollout_synth_cat_f32(const trl_rollout_t* args, int64_t noise_seed, int64_t env_offset, void* stream);" in header
    assert "int trl_rollout_cat_supported(int D, int H, int A, int act);" in header


def test_cat_supported_shapes(built_lib):
    from torchrl_amd import _C
    ok = _C.lib().trl_rollout_cat_supported
    for D, A in ((17, 6), (5, 3), (32, 8), (4, 2), (2, 2)):
        for act in (_C.ACT_TANH, _C.ACT_RELU):
            assert ok(D, 64, A, act) == 1
    for D, H, A, act in ((17, 64, 9, _C.ACT_TANH), (17, 64, 1, _C.ACT_TANH), (33, 64, 6, _C.ACT_TANH), (1, 64, 6, _C.ACT_TANH),
                         (17, 32, 6, _C.ACT_TANH), (17, 128, 6, _C.ACT_RELU), (17, 64, 6, _C.ACT_NONE)):
        assert ok(D, H, A, act) == 0


def _descriptor():
    """A descriptor whose pointers are never dereferenced: every call below returns from the host-side checks."""
    from torchrl_amd import _C
    a = _C.RolloutArgs()
    fake = 0x1000
    for k in ("pf_params", "vf_params", "env_A", "env_B", "cur_obs", "t_env", "cur_step", "episode_idx", "ep_return",
              "ep_count", "ep_log"):
        setattr(a, k, fake)
    a.D, a.H, a.A, a.act = 17, 64, 6, _C.ACT_TANH
    a.N, a.n_steps, a.rows, a.top = 32, 0, 1, 0
    a.horizon, a.max_episode_frames, a.ep_cap = 5, 5, 8
    return a


def test_argument_checks_return_before_any_launch(built_lib):
    from torchrl_amd import _C
    lib = _C.lib()
    EINVAL, EUNSUPPORTED = -1, -2
    call = lambda a, seed=1, off=0: lib.trl_rollout_synth_cat_f32(C.byref(a), seed, off, None)
    assert call(_descriptor()) == 0                                          # n_steps == 0: nothing to do, nothing launched
    assert lib.trl_rollout_synth_cat_f32(None, 1, 0, None) == EINVAL
    assert b"null descriptor" in lib.trl_last_error()

    def bad(code, needle=None, off=0, **kw):
        a = _descriptor()
        a.n_steps = 4                                                         # (a good descriptor would launch from here on)
        for k, v in kw.items():
            setattr(a, k, v)
        assert call(a, off=off) == code, kw
        assert lib.trl_last_error() and (needle is None or needle in lib.trl_last_error()), lib.trl_last_error()

    bad(EINVAL, b"null", pf_params=None)
    bad(EINVAL, b"null", env_B=None)
    bad(EINVAL, b"null", cur_obs=None)
    bad(EINVAL, b"null", ep_log=None)
    bad(EINVAL, b"ring", obs=0x1000)                                         # some ring tensors but not all
    bad(EINVAL, b"sizes", N=0)
    bad(EINVAL, b"sizes", rows=0)
    bad(EINVAL, b"top", top=3)
    bad(EINVAL, b"positive", horizon=0)
    bad(EINVAL, b"offset", off=-1)
    bad(EINVAL, b"Philox", noise=0x1000)
    bad(EINVAL, b"Philox", stage_n=16)
    bad(EINVAL, b"normaliser", norm_state=0x1000)
    bad(EUNSUPPORTED, b"not instantiated", A=9)
    bad(EUNSUPPORTED, b"not instantiated", A=1)
    bad(EUNSUPPORTED, b"not instantiated", D=33)
    bad(EUNSUPPORTED, b"not instantiated", H=32)
    bad(EUNSUPPORTED, b"not instantiated", act=_C.ACT_NONE)


@pytest.mark.parametrize("case", rr.PAIR_CASES + [rr.CPU_CASE, rr.WIDE_RELU_CASE], ids=rr.case_id)
def test_borderline_share_of_the_gpu_cases(case):
    """On the restatement alone: the rows of each case on which a kernel may legitimately draw the neighbouring action
    (threshold within 1e-5 * S of a prefix sum) stay within the cap the GPU tests allow -- with room: at most half of it."""
    N, steps, horizon = (rr.PAIR_N, rr.PAIR_T * rr.PAIR_EPOCHS, rr.PAIR_HORIZON)
    if case is rr.CPU_CASE:
        N, steps, horizon = rr.CPU_N, rr.CPU_T, rr.CPU_HORIZON
    if case is rr.WIDE_RELU_CASE:
        N, steps, horizon = rr.WIDE_RELU_N, rr.WIDE_RELU_T * rr.PAIR_EPOCHS, rr.WIDE_RELU_HORIZON
    out = rr.cpu_rollout(case, N, steps, horizon)
    share = float(out["borderline"].mean())
    acts = out["acts"].reshape(-1)
    counts = np.bincount(acts.astype(np.int64), minlength=case["A"])
    print("%s: borderline share %.5f, action counts %s, terminals %d" % (rr.case_id(case), share, counts.tolist(),
                                                                          int(out["terminals"].sum())))
    assert share <= 0.5 * rr.BORDERLINE_CAP
    assert (counts > 0).sum() >= 2                                           # the scaled head still explores
    assert out["terminals"].sum() > 0 and np.isfinite(out["rewards"]).all()
    if case["max_frames"] < horizon:
        assert out["time_limits"].sum() == 0                                 # the over-length bootstrap fires, `done` never
    else:
        assert out["time_limits"].sum() > 0 and len(out["episodes"]) > 0
