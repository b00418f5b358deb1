// The persistent rollout for `add_ln=True` networks: the LN = true instantiations of rollout_kernel and value_pass_kernel
// (trl_rollout.h) and their entry point.  Policy and critic carry their LayerNorm independently -- the rollout kernel takes
// the policy's flag, the value pass the critic's -- so a launch pairs one of this file's kernels with a plain one of
// k_rollout.hip (rollout_policy_rt / rollout_value_rt) when only one of the nets is normed.
//
// This file is compiled without the packed-fp32 VALU forms (build.py::SOURCE_FLAGS), k_rollout.hip with them: the plain
// instantiations keep the code they have, and none of them is instantiated here.
#include "trl_rollout.h"

extern "C" int trl_rollout_ln_supported(int head, int D, int H, int A, int act) {
  return (head == HEAD_GAUSS || head == HEAD_CAT || head == HEAD_SD) ? head_supported(head, D, H, A, act) : 0;
}

extern "C" int trl_rollout_synth_ln_f32(const trl_rollout_t* p, int head, int pf_ln, int vf_ln, int64_t noise_seed,
                                        int64_t env_offset, void* stream) {
  TRL_REQUIRE(head == HEAD_GAUSS || head == HEAD_CAT || head == HEAD_SD, "unknown head");
  TRL_REQUIRE(p, "null descriptor");
  TRL_REQUIRE(!p->norm_state, "LayerNorm rollout: no running observation normaliser in the persistent rollout");
  TRL_REQUIRE(!p->noise_flag && !p->stage_n,
              "LayerNorm rollout: the noise block is stream-ordered in front of the launch (no noise gate, nothing staged)");
  if (!trl_rollout_ln_supported(head, p->D, p->H, p->A, p->act)) {
    trl_set_error("LayerNorm rollout: %s shape D=%d H=%d A=%d act=%d outside the head's range (H == 64, 2 <= D <= 32, %d <= A <= %d, "
                  "Tanh or ReLU)", HEADS[head].name, p->D, p->H, p->A, p->act, HEADS[head].a_min, HEADS[head].a_max);
    return TRL_EUNSUPPORTED;
  }
  RolloutDev d;
  int rc = rollout_synth(p, head, noise_seed, env_offset, d);
  if (rc != TRL_OK || p->n_steps == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (!pf_ln) {
    rc = rollout_policy_rt(d, head, p->act, s);
    if (rc != TRL_OK) return rc;
  } else {
    RolloutDev e = d;
    e.n_ro_wg = trl_ceil_div(d.N, RO_ENVS);             // (no stagers: nothing is staged on this route)
    with_head(head, [&](auto hd) {
      return with_tile_act(p->D, p->act, [&](auto tile, auto act) {
        hipLaunchKernelGGL((rollout_kernel<decltype(tile)::value, 64, 8, decltype(act)::value, false, true, decltype(hd)::value, true>),
                           dim3(e.n_ro_wg), dim3(RO_THREADS), 0, s, e);
        return TRL_OK;
      });
    });
    TRL_LAUNCH_CHECK();
  }
  if (!d.store) return TRL_OK;
  if (!d.vf_params) return rollout_zero_value(d, s);    // no critic (a ZeroNet): the zero-storing value pass
  rc = rollout_value_wait(s, (hipEvent_t)p->value_wait_event);
  if (rc != TRL_OK) return rc;
  if (!vf_ln) return rollout_value_rt(d, p->act, s);
  with_tile_act(p->D, p->act, [&](auto tile, auto act) {
    hipLaunchKernelGGL((value_pass_kernel<decltype(tile)::value, 64, decltype(act)::value, true, true>), dim3(value_pass_grid(d)),
                       dim3(VP_THREADS), 0, s, value_dev(d));
    return TRL_OK;
  });
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}
