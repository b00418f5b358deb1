// The persistent rollout for 128- and 256-wide `add_ln=True` networks: the LN = true instantiations of rollout_wide_kernel and
// value_pass_wide_kernel (trl_rollout_wide.h) and their entry point.  Policy and critic carry their LayerNorm independently --
// the rollout kernel takes the policy's flag, the value pass the critic's -- so a launch pairs one of this file's kernels with
// a plain one of k_rollout_wide.hip (rollout_wide_policy / rollout_wide_value) when only one of the nets is normed.
//
// This file is compiled without the packed-fp32 VALU forms (build.py::SOURCE_FLAGS), like k_rollout_ln.hip; k_rollout_wide.hip
// with them: the plain instantiations keep the code they have, and none of them is instantiated here.
#include "trl_rollout_wide.h"

extern "C" int trl_rollout_wide_ln_supported(int head, int D, int H, int A, int act) {
  return ((head == HEAD_GAUSS || head == HEAD_CAT || head == HEAD_SD) && wide_shape_ok(head, D, H, A, act)) ? 1 : 0;
}

extern "C" int trl_rollout_synth_wide_ln_f32(const trl_rollout_t* p, int head, int pf_ln, int vf_ln, int64_t noise_seed,
                                             int64_t env_offset, void* stream) {
  TRL_REQUIRE(head == HEAD_GAUSS || head == HEAD_CAT || head == HEAD_SD, "unknown head");
  TRL_REQUIRE(p, "null descriptor");
  TRL_REQUIRE(!p->norm_state, "wide LayerNorm rollout: no running observation normaliser in the persistent rollout");
  TRL_REQUIRE(!p->noise_flag && !p->stage_n,
              "wide LayerNorm rollout: the noise block is stream-ordered in front of the launch (no noise gate, nothing staged)");
  TRL_REQUIRE(pf_ln || (vf_ln && p->vf_params),
              "wide LayerNorm rollout: neither network carries a LayerNorm (a plain pair is trl_rollout_synth_wide_f32's)");
  if (!trl_rollout_wide_ln_supported(head, p->D, p->H, p->A, p->act)) {
    trl_set_error("wide LayerNorm rollout: %s shape D=%d H=%d A=%d act=%d outside the head's range (H == 128 or 256, 2 <= D <= 32, "
                  "%d <= A <= %d, Tanh or ReLU)", HEADS[head].name, p->D, p->H, p->A, p->act, HEADS[head].a_min, HEADS[head].a_max);
    return TRL_EUNSUPPORTED;
  }
  RolloutDev d;
  int rc = rollout_synth(p, head, noise_seed, env_offset, d, /*shape_checked=*/true);
  if (rc != TRL_OK || p->n_steps == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (!pf_ln) {
    rc = rollout_wide_policy(d, head, p->H, p->act, s);
    if (rc != TRL_OK) return rc;
  } else {
    RolloutDev e = d;
    e.n_ro_wg = trl_ceil_div(d.N, RO_ENVS);
    with_head(head, [&](auto hd) {
      return with_width(p->H, [&](auto wd) {
        return with_tile_act(p->D, p->act, [&](auto tile, auto act) {
          hipLaunchKernelGGL((rollout_wide_kernel<decltype(tile)::value, decltype(wd)::value, decltype(act)::value, decltype(hd)::value, true>),
                             dim3(e.n_ro_wg), dim3(RW_THREADS), 0, s, e);
          return TRL_OK;
        });
      });
    });
    TRL_LAUNCH_CHECK();
  }
  if (!d.store) return TRL_OK;
  if (!d.vf_params) return rollout_zero_value(d, s);    // no critic (a ZeroNet): the zero-storing value pass
  rc = rollout_value_wait(s, (hipEvent_t)p->value_wait_event);
  if (rc != TRL_OK) return rc;
  if (!vf_ln) return rollout_wide_value(d, p->H, p->act, s);
  with_width(p->H, [&](auto wd) {
    return with_tile_act(p->D, p->act, [&](auto tile, auto act) {
      hipLaunchKernelGGL((value_pass_wide_kernel<decltype(tile)::value, decltype(wd)::value, decltype(act)::value, true>),
                         dim3(value_pass_wide_grid(d, p->H)), dim3(VW_THREADS), 0, s, value_dev(d));
      return TRL_OK;
    });
  });
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}
