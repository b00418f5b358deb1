"""The fused state-dependent-std update without a GPU: the new symbols and their ctypes signatures, trl_ppo_sd_supported's
truth table, strides and workspace sizes against their formulas, the argument checks of the trl_ppo_sd_* entry points (every
case returns before anything is launched), and the conditions the GPU tests' random inputs are chosen to meet (on the
float64 restatement): no sample's ratio within 1e-4 of 1 +- clip_para, no raw log_std within 1e-3 of -20 or 2, and in the
clamp cases >= 10 % of the log_std elements well above 2 and one column of every row below -20."""
import ctypes as C
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_sd_update_cases as su                                           # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
NEW = ("trl_ppo_sd_supported", "trl_ppo_sd_partial_stride", "trl_ppo_sd_scalar_stride", "trl_ppo_sd_minibatch_grad_f32",
       "trl_ppo_sd_reduce_f32", "trl_ppo_sd_reduce_adam_workspace", "trl_ppo_sd_reduce_adam_f32",
       "trl_ppo_sd_reduce_adam_net_f32")


@pytest.fixture(scope="module")
def built_lib():
    from torchrl_amd import build
    return build.build(verbose=False)


def p_sizes(D, A):
    """[W1 b1 W2 b2 W3 b3] with 2A head rows and no logstd tail; the value net."""
    return 64 * D + 64 + 4096 + 64 + 64 * 2 * A + 2 * A, 64 * D + 64 + 4096 + 64 + 64 + 1


def test_new_symbols_and_signatures(built_lib):
    from torchrl_amd import _C
    lib = _C.lib()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _C.SIGNATURES[name][1]
    # the family mirrors the categorical one, argument list by argument list
    for name in NEW:
        if name != "trl_ppo_sd_scalar_stride":
            assert _C.SIGNATURES[name] == _C.SIGNATURES[name.replace("_sd_", "_cat_")], name
    header = open(os.path.join(os.path.dirname(HERE), "include", "trl_hip.h")).read()
    assert "int trl_ppo_sd_supported(int D, int H, int A, int act);" in header
    assert "int trl_ppo_sd_partial_stride(int D, int H, int A);" in header
    assert "int trl_ppo_sd_scalar_stride(void);" in header
    assert "int trl_ppo_sd_minibatch_grad_f32(const trl_ppo_batch_t* args, void* stream);" in header


def test_sd_supported_truth_table(built_lib):
    from torchrl_amd import _C
    ok = _C.lib().trl_ppo_sd_supported
    acts = {_C.ACT_TANH: 1, _C.ACT_RELU: 1, _C.ACT_NONE: 0, 7: 0, -1: 0}
    for D, d_ok in ((1, 0), (2, 1), (17, 1), (18, 1), (32, 1), (33, 0)):
        for A, a_ok in ((0, 0), (1, 1), (2, 1), (6, 1), (8, 1), (9, 0)):
            for Hh, h_ok in ((32, 0), (64, 1), (128, 0)):
                for act, act_ok in acts.items():
                    assert ok(D, Hh, A, act) == (d_ok & a_ok & h_ok & act_ok), (D, Hh, A, act)


def test_strides_and_workspace(built_lib):
    from torchrl_amd import _C
    lib = _C.lib()
    for D, A in ((2, 1), (17, 6), (17, 8), (32, 8), (27, 5), (18, 2)):
        p_pf, p_vf = p_sizes(D, A)
        ps = lib.trl_ppo_sd_partial_stride(D, 64, A)
        assert ps == (max(p_pf, p_vf) + 63) // 64 * 64 == _C.ppo_sd_partial_stride(D, 64, A)
        assert lib.trl_ppo_sd_reduce_adam_workspace(D, 64, A) == 16 + 4 * (ps // 64)
    assert lib.trl_ppo_sd_partial_stride(17, 64, 8) == 6400 and lib.trl_ppo_sd_partial_stride(32, 64, 8) == 7360
    # 8 doubles per workgroup as for every head, then 9 statistics of log_std / std padded to 16
    assert lib.trl_ppo_sd_scalar_stride() == _C.ppo_sd_scalar_stride() == 24
    for D, Hh, A in ((17, 64, 0), (17, 64, 9), (33, 64, 6), (1, 64, 6), (17, 32, 6)):
        assert lib.trl_ppo_sd_partial_stride(D, Hh, A) == EUNSUPPORTED
        assert b"not instantiated" in lib.trl_last_error()
        assert lib.trl_ppo_sd_reduce_adam_workspace(D, Hh, A) == EUNSUPPORTED


FAKE = 0x1000


def _batch():
    """A descriptor whose pointers are never dereferenced: every call below returns from the host-side checks."""
    from torchrl_amd import _C
    g = _C.PpoBatchArgs()
    for k in ("obs", "acts", "advs", "rets", "old_values", "old_logp", "adv_raw", "pf_params", "vf_params", "partial",
              "scal_partial"):
        setattr(g, k, FAKE)
    g.rows_mb, g.N, g.n_global = 4, 16, 64.0
    g.D, g.H, g.A, g.act = 17, 64, 6, _C.ACT_TANH
    g.clip_para, g.entropy_coeff, g.loss_mode = 0.2, 0.01, _C.LOSS_PPO_CLIP
    g.n_wg, g.n_wg_pf = 2, 0
    return g


def test_grad_argument_checks_return_before_any_launch(built_lib):
    from torchrl_amd import _C
    lib = _C.lib()
    assert lib.trl_ppo_sd_minibatch_grad_f32(None, None) == EINVAL
    assert b"null descriptor" in lib.trl_last_error()

    def bad(code, needle, **kw):
        g = _batch()
        for k, v in kw.items():
            setattr(g, k, v)
        assert lib.trl_ppo_sd_minibatch_grad_f32(C.byref(g), None) == code, kw
        assert needle in lib.trl_last_error(), lib.trl_last_error()

    bad(EUNSUPPORTED, b"not instantiated", A=0)
    bad(EUNSUPPORTED, b"not instantiated", A=9)
    bad(EUNSUPPORTED, b"not instantiated", D=33)
    bad(EUNSUPPORTED, b"not instantiated", D=1)
    bad(EUNSUPPORTED, b"not instantiated", H=32)
    bad(EUNSUPPORTED, b"not instantiated", act=_C.ACT_NONE)
    for k in ("obs", "acts", "advs", "rets", "adv_raw", "partial", "scal_partial", "pf_params", "vf_params"):
        bad(EINVAL, b"null", **{k: None})
    bad(EINVAL, b"old_logp", old_logp=None)                                   # the clip loss needs log pi_old ...
    bad(EINVAL, b"old_values", clipped_value_loss=1, old_values=None)
    bad(EINVAL, b"loss_mode", loss_mode=5)
    bad(EINVAL, b"empty", rows_mb=0)
    bad(EINVAL, b"empty", N=0)
    bad(EINVAL, b"n_wg", n_wg=1)
    bad(EINVAL, b"n_wg_pf", n_wg_pf=3)
    bad(EINVAL, b"n_wg_pf", n_wg_pf=-2)
    bad(EINVAL, b"n_global", n_global=1.0)
    bad(EINVAL, b"aligned", partial=FAKE + 4)
    bad(EINVAL, b"aligned", pf_params=FAKE + 2)


def _adam(p_pf, p_vf, grads=FAKE, **kw):
    from torchrl_amd import _C
    a = _C.AdamArgs()
    a.params, a.grads, a.exp_avg, a.exp_avg_sq = FAKE, grads, FAKE, FAKE
    a.n_groups = 2
    a.group_sizes[0], a.group_sizes[1] = p_pf, p_vf
    a.max_norm, a.beta1, a.beta2, a.eps, a.grad_scale, a.step_count = 0.5, 0.9, 0.999, 1e-5, 1.0, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_fold_argument_checks_return_before_any_launch(built_lib):
    from torchrl_amd import _C
    lib = _C.lib()
    D, A = 17, 6
    p_pf, p_vf = p_sizes(D, A)
    red = lambda *a: lib.trl_ppo_sd_reduce_f32(*a)
    assert red(None, FAKE, 2, 0, D, 64, A, None, FAKE, FAKE, None) == EINVAL and b"null" in lib.trl_last_error()
    assert red(FAKE, None, 2, 0, D, 64, A, None, FAKE, FAKE, None) == EINVAL
    assert red(FAKE, FAKE, 2, 0, D, 64, A, None, None, FAKE, None) == EINVAL
    assert red(FAKE, FAKE, 2, 0, D, 64, A, None, FAKE, None, None) == EINVAL
    assert red(FAKE, FAKE, 1, 0, D, 64, A, None, FAKE, FAKE, None) == EINVAL and b"n_wg" in lib.trl_last_error()
    assert red(FAKE, FAKE, 2, 2, D, 64, A, None, FAKE, FAKE, None) == EINVAL
    assert red(FAKE, FAKE, 2, 0, D, 64, 0, None, FAKE, FAKE, None) == EUNSUPPORTED
    assert red(FAKE, FAKE, 2, 0, D, 64, 9, None, FAKE, FAKE, None) == EUNSUPPORTED
    assert red(FAKE, FAKE, 2, 0, D, 32, A, None, FAKE, FAKE, None) == EUNSUPPORTED
    for fn, sel in ((lib.trl_ppo_sd_reduce_adam_f32, 0), (lib.trl_ppo_sd_reduce_adam_net_f32, 0)):
        good = _adam(p_pf, p_vf)
        call = lambda adam, part=FAKE, n_wg=2, A_=A, ws=FAKE, scal=FAKE, info=FAKE: fn(
            part, scal, n_wg, sel, D, 64, A_, FAKE, info, C.byref(adam) if adam is not None else None, ws, None)
        assert call(good, part=None) == EINVAL and b"null" in lib.trl_last_error()
        assert call(good, scal=None) == EINVAL
        assert call(good, info=None) == EINVAL
        assert call(good, ws=None) == EINVAL
        assert call(good, A_=0) == EUNSUPPORTED and b"not instantiated" in lib.trl_last_error()
        assert call(good, A_=9) == EUNSUPPORTED
        assert call(None) == EINVAL
        assert call(_adam(p_pf, p_vf, params=None)) == EINVAL
        assert call(_adam(p_pf, p_vf, n_groups=5)) == EINVAL
        assert call(_adam(p_pf - 64 * A, p_vf)) == EINVAL and b"groups" in lib.trl_last_error()   # the Gaussian block
        assert call(_adam(p_pf + A, p_vf)) == EINVAL and b"groups" in lib.trl_last_error()
        assert call(_adam(p_pf, p_vf, grads=FAKE + 64)) == EINVAL and b"grads" in lib.trl_last_error()
    assert lib.trl_ppo_sd_reduce_adam_f32(FAKE, FAKE, 1, 0, D, 64, A, FAKE, FAKE, C.byref(_adam(p_pf, p_vf)), FAKE, None) == EINVAL
    assert lib.trl_ppo_sd_reduce_adam_f32(FAKE, FAKE, 2, 2, D, 64, A, FAKE, FAKE, C.byref(_adam(p_pf, p_vf)), FAKE, None) == EINVAL
    assert lib.trl_ppo_sd_reduce_adam_net_f32(FAKE, FAKE, 0, 0, D, 64, A, FAKE, FAKE, C.byref(_adam(p_pf, p_vf)), FAKE, None) == EINVAL
    assert lib.trl_ppo_sd_reduce_adam_net_f32(FAKE, FAKE, 2, 2, D, 64, A, FAKE, FAKE, C.byref(_adam(p_pf, p_vf)), FAKE, None) == EINVAL
    assert b"net" in lib.trl_last_error()


@pytest.mark.parametrize("c", su.GRAD_CASES, ids=su.case_id)
def test_conditions_on_the_kernel_cases(c):
    """Conditions on the inputs, not tolerances on the kernel (float64 restatement, every stored sample of the case)."""
    import torch
    x = su.grad_inputs(c)
    A = x["A"]
    n_clip, raw = su.near_clip(x["lp"], x["old_logp"]), x["raw_ls"].reshape(-1, A)
    mb = su.minibatch(x)
    ratio = torch.exp(mb["lp"].double() - mb["old_logp"].double())
    print("%s: %d samples near a clip edge, %d log_std near a clamp edge; minibatch ratio in [%.3f, %.3f]; raw log_std in "
          "[%.3f, %.3f]" % (su.case_id(c), n_clip, su.near_clamp(raw), ratio.min(), ratio.max(), raw.min(), raw.max()))
    assert torch.isfinite(x["lp"]).all() and torch.isfinite(x["old_logp"]).all()
    assert n_clip == 0
    assert su.near_clamp(raw) == 0
    if x["rows"] * x["N"] >= 84:
        assert ratio.min() < 1.0 - su.CLIP and ratio.max() > 1.0 + su.CLIP
    if x["clamp"]:
        hi, lo = su.clamp_columns(A)
        assert float((raw > 2.0).double().mean()) >= 0.10 and bool((raw[raw > 2.0] >= 2.5).all())   # well beyond the clamp
        assert bool((raw[:, hi] == su.LS_HIGH).all())
        assert bool(((raw < -20.0).sum(dim=1) >= 1).all()) and bool((raw[:, lo] == su.LS_LOW).all())
        assert not x["tanh"]
    else:
        assert bool(((raw > -20.0) & (raw < 2.0)).all())


@pytest.mark.parametrize("c", su.ENGINE_CASES, ids=lambda c: "D%d_A%d" % c[:2])
def test_conditions_on_the_engine_cases(c):
    import torch
    x = su.engine_inputs(c)
    lp, old = su.engine_old_logp(x)
    assert su.near_clip(lp, old) == 0
    ratio = torch.exp(lp - old)
    assert ratio.min() > 1.0 - su.CLIP + 0.05 and ratio.max() < 1.0 + su.CLIP - 0.05   # far inside: a few Adam steps do not reach the edges
    pf, _ = su.nets_of(x["D"], x["A"], x["seed"])
    T, N = x["obs"].shape[:2]
    with torch.no_grad():
        head = su.forward([p.detach() for p in su.linear_params(pf)], x["obs"].reshape(T * N, -1), "tanh")
    assert su.near_clamp(head[:, x["A"]:]) == 0 and bool((head[:, x["A"]:].abs() < 1.5).all())
