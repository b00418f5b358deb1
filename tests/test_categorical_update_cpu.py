"""The fused categorical update without a GPU: the new symbols and their ctypes signatures, trl_ppo_cat_supported's truth
table, the argument checks of the trl_ppo_cat_* entry points (every case returns before anything is launched), and the
condition the GPU tests' random inputs are chosen to meet: no sample's ratio within 1e-4 of 1 +- clip_para."""
import ctypes as C
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _categorical_update_cases as cu                                        # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
NEW = ("trl_ppo_cat_supported", "trl_ppo_cat_partial_stride", "trl_ppo_cat_minibatch_grad_f32", "trl_ppo_cat_reduce_f32",
       "trl_ppo_cat_reduce_adam_workspace", "trl_ppo_cat_reduce_adam_f32", "trl_ppo_cat_reduce_adam_net_f32")


@pytest.fixture(scope="module")
def built_lib():
    from torchrl_amd import build
    return build.build(verbose=False)


def test_new_symbols_and_signatures(built_lib):
    from torchrl_amd import _C
    lib = _C.lib()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _C.SIGNATURES[name][1]
    # same argument lists as the Gaussian counterparts
    for cat, gauss in (("trl_ppo_cat_minibatch_grad_f32", "trl_ppo_minibatch_grad_f32"), ("trl_ppo_cat_reduce_f32", "trl_ppo_reduce_f32"),
                       ("trl_ppo_cat_reduce_adam_f32", "trl_ppo_reduce_adam_f32"),
                       ("trl_ppo_cat_reduce_adam_net_f32", "trl_ppo_reduce_adam_net_f32"),
                       ("trl_ppo_cat_reduce_adam_workspace", "trl_ppo_reduce_adam_workspace"),
                       ("trl_ppo_cat_partial_stride", "trl_ppo_partial_stride")):
        assert _C.SIGNATURES[cat] == _C.SIGNATURES[gauss]
    header = open(os.path.join(os.path.dirname(HERE), "include", "trl_hip.h")).read()
    assert "int trl_ppo_cat_supported(int D, int H, int A, int act);" in header
    assert "int trl_ppo_cat_partial_stride(int D, int H, int A);" in header
    assert "int trl_ppo_cat_minibatch_grad_f32(const trl_ppo_batch_t* args, void* stream);" in header


def test_cat_supported_truth_table(built_lib):
    from torchrl_amd import _C
    ok = _C.lib().trl_ppo_cat_supported
    acts = {_C.ACT_TANH: 1, _C.ACT_RELU: 1, _C.ACT_NONE: 0, 7: 0, -1: 0}
    for D, d_ok in ((1, 0), (2, 1), (17, 1), (18, 1), (32, 1), (33, 0)):
        for A, a_ok in ((1, 0), (2, 1), (6, 1), (8, 1), (9, 0)):
            for Hh, h_ok in ((32, 0), (64, 1), (128, 0)):
                for act, act_ok in acts.items():
                    assert ok(D, Hh, A, act) == (d_ok & a_ok & h_ok & act_ok), (D, Hh, A, act)


def test_strides_and_workspace(built_lib):
    from torchrl_amd import _C
    lib = _C.lib()
    for D, A in ((2, 2), (17, 6), (17, 8), (32, 8), (27, 5)):
        p_pf = 64 * D + 64 + 4096 + 64 + 64 * A + A                          # [W1 b1 W2 b2 W3 b3]: no logstd tail
        p_vf = 64 * D + 64 + 4096 + 64 + 64 + 1
        ps = lib.trl_ppo_cat_partial_stride(D, 64, A)
        assert ps == (max(p_pf, p_vf) + 63) // 64 * 64
        assert lib.trl_ppo_cat_reduce_adam_workspace(D, 64, A) == 16 + 4 * (ps // 64)
    for D, Hh, A in ((17, 64, 1), (17, 64, 9), (33, 64, 6), (1, 64, 6), (17, 32, 6)):
        assert lib.trl_ppo_cat_partial_stride(D, Hh, A) == EUNSUPPORTED
        assert b"not instantiated" in lib.trl_last_error()
        assert lib.trl_ppo_cat_reduce_adam_workspace(D, Hh, A) == EUNSUPPORTED


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
    assert lib.trl_ppo_cat_minibatch_grad_f32(None, None) == EINVAL
    assert b"null descriptor" in lib.trl_last_error()

    def bad(code, needle, **kw):
        g = _batch()
        for k, v in kw.items():
            setattr(g, k, v)
        assert lib.trl_ppo_cat_minibatch_grad_f32(C.byref(g), None) == code, kw
        assert needle in lib.trl_last_error(), lib.trl_last_error()

    bad(EUNSUPPORTED, b"not instantiated", A=1)
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
    bad(EINVAL, b"n_wg", n_wg=1)
    bad(EINVAL, b"n_wg_pf", n_wg_pf=3)
    bad(EINVAL, b"n_global", n_global=1.0)
    bad(EINVAL, b"aligned", partial=FAKE + 4)


def _adam(p_pf, p_vf, grads=FAKE):
    from torchrl_amd import _C
    a = _C.AdamArgs()
    a.params, a.grads, a.exp_avg, a.exp_avg_sq = FAKE, grads, FAKE, FAKE
    a.n_groups = 2
    a.group_sizes[0], a.group_sizes[1] = p_pf, p_vf
    a.max_norm, a.beta1, a.beta2, a.eps, a.grad_scale, a.step_count = 0.5, 0.9, 0.999, 1e-5, 1.0, 1
    return a


def test_fold_argument_checks_return_before_any_launch(built_lib):
    from torchrl_amd import _C
    lib = _C.lib()
    D, A = 17, 6
    p_pf, p_vf = 64 * D + 64 + 4096 + 64 + 64 * A + A, 64 * D + 64 + 4096 + 64 + 64 + 1
    red = lambda *a: lib.trl_ppo_cat_reduce_f32(*a)
    assert red(None, FAKE, 2, 0, D, 64, A, None, FAKE, FAKE, None) == EINVAL and b"null" in lib.trl_last_error()
    assert red(FAKE, FAKE, 2, 0, D, 64, A, None, None, FAKE, None) == EINVAL
    assert red(FAKE, FAKE, 1, 0, D, 64, A, None, FAKE, FAKE, None) == EINVAL and b"n_wg" in lib.trl_last_error()
    assert red(FAKE, FAKE, 2, 0, D, 64, 1, None, FAKE, FAKE, None) == EUNSUPPORTED
    assert red(FAKE, FAKE, 2, 0, D, 32, A, None, FAKE, FAKE, None) == EUNSUPPORTED
    for fn, sel in ((lib.trl_ppo_cat_reduce_adam_f32, 0), (lib.trl_ppo_cat_reduce_adam_net_f32, 0)):
        good = _adam(p_pf, p_vf)
        call = lambda adam, part=FAKE, n_wg=2, A_=A, ws=FAKE: fn(part, FAKE, n_wg, sel, D, 64, A_, FAKE, FAKE,
                                                                   C.byref(adam) if adam is not None else None, ws, None)
        assert call(good, part=None) == EINVAL and b"null" in lib.trl_last_error()
        assert call(good, ws=None) == EINVAL
        assert call(good, A_=1) == EUNSUPPORTED and b"not instantiated" in lib.trl_last_error()
        assert call(good, A_=9) == EUNSUPPORTED
        assert call(None) == EINVAL
        assert call(_adam(p_pf + A, p_vf)) == EINVAL and b"groups" in lib.trl_last_error()   # the Gaussian block (logstd tail)
        assert call(_adam(p_pf, p_vf, grads=FAKE + 64)) == EINVAL and b"grads" in lib.trl_last_error()
    assert lib.trl_ppo_cat_reduce_adam_f32(FAKE, FAKE, 1, 0, D, 64, A, FAKE, FAKE, C.byref(_adam(p_pf, p_vf)), FAKE, None) == EINVAL
    assert lib.trl_ppo_cat_reduce_adam_net_f32(FAKE, FAKE, 2, 2, D, 64, A, FAKE, FAKE, C.byref(_adam(p_pf, p_vf)), FAKE, None) == EINVAL
    assert b"net" in lib.trl_last_error()


@pytest.mark.parametrize("c", cu.GRAD_CASES, ids=cu.case_id)
def test_no_ratio_near_the_clip_edges_in_the_kernel_cases(c):
    """A condition on the inputs, not a tolerance on the kernel: on the restatement, no stored sample of the case (the
    minibatch's rows and the others) has its ratio within 1e-4 of 1 - clip or 1 + clip -- while both sides of the clip
    are populated, so the clipped branch is exercised."""
    import torch
    x = cu.grad_inputs(c)
    n = cu.near_clip(x["lp"], x["old_logp"])
    mb = cu.minibatch(x)
    ratio = torch.exp(mb["lp"] - mb["old_logp"])
    print("%s: %d samples near a clip edge; minibatch ratio in [%.3f, %.3f]" % (cu.case_id(c), n, ratio.min(), ratio.max()))
    assert n == 0
    if x["rows"] * x["N"] >= 84:
        assert ratio.min() < 1.0 - cu.CLIP and ratio.max() > 1.0 + cu.CLIP


@pytest.mark.parametrize("c", cu.ENGINE_CASES, ids=lambda c: "D%d_A%d" % c[:2])
def test_no_ratio_near_the_clip_edges_in_the_engine_cases(c):
    x = cu.engine_inputs(c)
    lp, old = cu.engine_old_logp(x)
    assert cu.near_clip(lp, old) == 0
    import torch
    ratio = torch.exp(lp - old)
    assert ratio.min() > 1.0 - cu.CLIP + 0.05 and ratio.max() < 1.0 + cu.CLIP - 0.05   # far inside: a few Adam steps do not reach the edges
