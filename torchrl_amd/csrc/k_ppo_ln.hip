// The fused PPO / A2C minibatch gradient for `add_ln=True` networks: the LN instantiations of ppo_wave_pass /
// ppo_grad_wave_kernel (trl_ppo_wave.h) and their entry points.  Policy and critic carry their LayerNorm independently
// (ln_mask bit 0 / bit 1): a kernel of this file pairs a normed pass with a plain one when only one of the nets is normed.
// All three heads, both input tiles (17 / 32 features), Tanh / ReLU, runtime dims only.
//
// This file is compiled without the packed-fp32 VALU forms (build.py::SOURCE_FLAGS: the project's rule for LayerNorm
// arithmetic), k_ppo.hip with them: the plain kernels keep the code they have, and none of them is instantiated here.
// The folds behind these launches are k_ppo.hip's kernels (trl_ppo_ln_reduce_*), which take the lengths from the launch.
#include "trl_ppo_wave.h"

static bool ppo_ln_args_ok(int head, int ln_mask) { return head >= HEAD_GAUSS && head <= HEAD_SD && ln_mask >= 1 && ln_mask <= 3; }

extern "C" int trl_ppo_ln_supported(int D, int H, int A, int act, int head, int ln_mask) {
  return ppo_ln_args_ok(head, ln_mask) ? head_supported(head, D, H, A, act) : 0;
}

// floats of a partial row: the larger of [W1 b1 (gamma beta) W2 b2 W3 b3 (logstd)] of the two nets, in whole 64s
extern "C" int trl_ppo_ln_partial_stride(int D, int H, int A, int head, int ln_mask) {
  if (!ppo_ln_args_ok(head, ln_mask) || !head_shape_ok(head, D, H, A)) {
    trl_set_error("trl_ppo_ln_partial_stride: head %d, ln_mask %d, D=%d H=%d A=%d outside what the LayerNorm instantiations carry "
                  "(H == 64, 2 <= D <= 32, A in the head's range, ln_mask 1..3)", head, ln_mask, D, H, A);
    return TRL_EUNSUPPORTED;
  }
  return ppo_ln_stride(D, H, A, head, ln_mask);
}

template <int LNM> static int ppo_ln_launch(const PpoDev& d, int D, int act, int head, hipStream_t s) {
  return with_head(head, [&](auto hd) {
    return with_tile_act(D, act, [&](auto tile, auto ac) {
      return launch_ppo<decltype(tile)::value, 64, 8, decltype(ac)::value, true, decltype(hd)::value, LNM>(d, s);
    });
  });
}

// trl_ppo_minibatch_grad_f32 (and its per-head siblings) for a pair of which at least one net is normed.  The normed net's
// block is [W1 b1 gamma beta W2 b2 W3 b3 (logstd)] (ops.plan_params), its gradients leave in that order; partial rows are
// trl_ppo_ln_partial_stride floats, the scalar rows the head's.  Every n_wg_pf mode of trl_ppo_batch_t works.
extern "C" int trl_ppo_ln_minibatch_grad_f32(const trl_ppo_batch_t* p, int head, int ln_mask, void* stream) {
  if (!p) { trl_set_error("ppo_ln_grad: null descriptor"); return TRL_EINVAL; }
  if (!trl_ppo_ln_supported(p->D, p->H, p->A, p->act, head, ln_mask)) {
    trl_set_error("ppo_ln_grad: head %d, ln_mask %d, shape D=%d H=%d A=%d act=%d not instantiated (H == 64, 2 <= D <= 32, A in the "
                  "head's range, Tanh / ReLU, ln_mask 1..3)", head, ln_mask, p->D, p->H, p->A, p->act);
    return TRL_EUNSUPPORTED;
  }
  PpoDev d;
  const int rc = ppo_dev_fill(p, head, false, d);
  if (rc != TRL_OK) return rc;
  d.p_stride = ppo_ln_stride(p->D, p->H, p->A, head, ln_mask);
  hipStream_t s = (hipStream_t)stream;
  if (ln_mask == 1) return ppo_ln_launch<1>(d, p->D, p->act, head, s);
  if (ln_mask == 2) return ppo_ln_launch<2>(d, p->D, p->act, head, s);
  return ppo_ln_launch<3>(d, p->D, p->act, head, s);
}
