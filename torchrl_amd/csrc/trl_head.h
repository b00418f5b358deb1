// The policy heads of the fused PPO / A2C kernels (k_ppo.hip) and of the persistent rollout (k_rollout.hip): their names
// as a template parameter, one host-side table of what differs between them, and the run-time -> compile-time dispatch.
#pragma once
#include <type_traits>
#include "trl_common.h"

// HEAD_GAUSS: diagonal Gaussian with a free logstd vector behind the flat policy block (GuassianContPolicyBasicBias)
// HEAD_CAT:   categorical, the A head outputs are logits (CategoricalDisPolicy)
// HEAD_SD:    state-dependent-std Gaussian, a head of 2A rows [mean | log_std] (GuassianContPolicy)
enum { HEAD_GAUSS = 0, HEAD_CAT = 1, HEAD_SD = 2 };

// SD: doubles per workgroup in the SECOND block of scalar rows (behind the n_wg x 8 block every head writes):
//   0 log_std sum  1 sum of squares  2 max  3 -min   4 std sum  5 sum of squares  6 max  7 -min   8 samples   9..15 zero
#define SD_SCAL 16

struct HeadDesc {
  const char* name;      // in error texts
  const char* tag;       // in entry-point names: trl_ppo_<tag>partial_stride
  int a_min, a_max;      // actions / action dims the 64-wide runtime-dims tiles carry
  int rows_per_a;        // head rows (of W3 / b3) = rows_per_a * A
  bool logstd_tail;      // the flat policy block ends in A logstd floats
  int scal_stride;       // doubles of scal_partial per workgroup
};
static const HeadDesc HEADS[3] = {
  {"Gaussian", "", 1, 8, 1, true, 8},
  {"categorical", "cat_", 2, 8, 1, false, 8},
  {"state-dependent-std", "sd_", 1, 8, 2, false, 8 + SD_SCAL},
};

// what the runtime-dims instantiations carry: any 64-wide two-layer pair with 2..32 inputs, Tanh or ReLU
static inline bool head_shape_ok(int head, int D, int H, int A) {
  return H == 64 && D >= 2 && D <= 32 && A >= HEADS[head].a_min && A <= HEADS[head].a_max;
}
static inline int head_supported(int head, int D, int H, int A, int act) {
  return (head_shape_ok(head, D, H, A) && (act == TRL_ACT_TANH || act == TRL_ACT_RELU)) ? 1 : 0;
}
// floats of the flat parameter blocks (MlpFlat order, trl_mlp.h): [W1 b1 W2 b2 W3 b3 (logstd)]
static inline int ppo_p_pf(int D, int H, int A, int head) {
  const int R = HEADS[head].rows_per_a * A;
  return H * D + H + H * H + H + R * H + R + (HEADS[head].logstd_tail ? A : 0);
}
static inline int ppo_p_vf(int D, int H) { return H * D + H + H * H + H + H + 1; }

template <int V> using head_ic = std::integral_constant<int, V>;
// f(tile, act) with the input tile (17 or 32 features) and the activation as integral constants; the caller has checked
// that act is Tanh or ReLU
template <class F> static int with_tile_act(int D, int act, F&& f) {
  if (D <= 17) return act == TRL_ACT_TANH ? f(head_ic<17>{}, head_ic<TRL_ACT_TANH>{}) : f(head_ic<17>{}, head_ic<TRL_ACT_RELU>{});
  return act == TRL_ACT_TANH ? f(head_ic<32>{}, head_ic<TRL_ACT_TANH>{}) : f(head_ic<32>{}, head_ic<TRL_ACT_RELU>{});
}
// f(head) with the head as an integral constant
template <class F> static int with_head(int head, F&& f) {
  return head == HEAD_SD ? f(head_ic<HEAD_SD>{}) : (head == HEAD_CAT ? f(head_ic<HEAD_CAT>{}) : f(head_ic<HEAD_GAUSS>{}));
}
