// The persistent rollout for plain 128- and 256-wide two-layer networks: the LN = false instantiations of rollout_wide_kernel
// and value_pass_wide_kernel (trl_rollout_wide.h, where the design is described) and their entry point
// trl_rollout_synth_wide_f32.  The LayerNorm variants are k_rollout_wide_ln.hip's; the plain halves of its mixed pairs are
// launched from here (rollout_wide_policy / rollout_wide_value).
#include "trl_rollout_wide.h"

extern "C" int trl_rollout_wide_supported(int head, int D, int H, int A, int act) {
  return ((head == HEAD_GAUSS || head == HEAD_CAT || head == HEAD_SD) && wide_shape_ok(head, D, H, A, act)) ? 1 : 0;
}

int rollout_wide_policy(const RolloutDev& d, int head, int H, int act, hipStream_t s) {
  RolloutDev e = d;
  e.n_ro_wg = trl_ceil_div(d.N, RO_ENVS);
  with_head(head, [&](auto hd) {
    return with_width(H, [&](auto wd) {
      return with_tile_act(d.D, act, [&](auto tile, auto ac) {
        hipLaunchKernelGGL((rollout_wide_kernel<decltype(tile)::value, decltype(wd)::value, decltype(ac)::value, decltype(hd)::value>),
                           dim3(e.n_ro_wg), dim3(RW_THREADS), 0, s, e);
        return TRL_OK;
      });
    });
  });
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}
int rollout_wide_value(const RolloutDev& d, int H, int act, hipStream_t s) {
  with_width(H, [&](auto wd) {
    return with_tile_act(d.D, act, [&](auto tile, auto ac) {
      hipLaunchKernelGGL((value_pass_wide_kernel<decltype(tile)::value, decltype(wd)::value, decltype(ac)::value>),
                         dim3(value_pass_wide_grid(d, H)), dim3(VW_THREADS), 0, s, value_dev(d));
      return TRL_OK;
    });
  });
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

extern "C" int trl_rollout_synth_wide_f32(const trl_rollout_t* p, int head, int64_t noise_seed, int64_t env_offset, void* stream) {
  TRL_REQUIRE(head == HEAD_GAUSS || head == HEAD_CAT || head == HEAD_SD, "unknown head");
  TRL_REQUIRE(p, "null descriptor");
  TRL_REQUIRE(!p->norm_state, "wide rollout: no running observation normaliser in the persistent rollout");
  TRL_REQUIRE(!p->noise_flag && !p->stage_n,
              "wide rollout: the noise block is stream-ordered in front of the launch (no noise gate, nothing staged)");
  if (!trl_rollout_wide_supported(head, p->D, p->H, p->A, p->act)) {
    trl_set_error("wide rollout: %s shape D=%d H=%d A=%d act=%d outside the head's range (H == 128 or 256, 2 <= D <= 32, %d <= A <= %d, "
                  "Tanh or ReLU)", HEADS[head].name, p->D, p->H, p->A, p->act, HEADS[head].a_min, HEADS[head].a_max);
    return TRL_EUNSUPPORTED;
  }
  RolloutDev d;
  int rc = rollout_synth(p, head, noise_seed, env_offset, d, /*shape_checked=*/true);
  if (rc != TRL_OK || p->n_steps == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  rc = rollout_wide_policy(d, head, p->H, p->act, s);
  if (rc != TRL_OK) return rc;
  if (!d.store) return TRL_OK;
  if (!d.vf_params) return rollout_zero_value(d, s);    // no critic (a ZeroNet): the zero-storing value pass
  rc = rollout_value_wait(s, (hipEvent_t)p->value_wait_event);
  if (rc != TRL_OK) return rc;
  return rollout_wide_value(d, p->H, p->act, s);
}
