// K1 + K2 + K3 -- the whole vectorised on-policy rollout as two launches: a persistent
// policy / env kernel that walks all T steps, then one streaming value pass over the T x N cells.
//
// Replaces n_steps x VecOnPolicyCollector.take_actions
// (torchrl/collector/on_policy.py:90-155; loop base.py:108-122) on the
// synthetic env: environments are independent, the networks are shared and
// read-only during collection, so a workgroup can carry 16 envs through all T
// steps with no inter-workgroup communication -- the 2 host<->device round
// trips and the python env loop per step of the reference disappear, and so do
// per-step kernel launches.
//
// The rollout is a latency problem (T strictly sequential steps, only N/16 independent tiles), so
// the sequential kernel carries only what the recurrence needs -- the policy and the env:
//   * workgroup = 4 waves = 16 envs on v_mfma_f32_16x16x4_f32; wave mo computes 16 of the 64 hidden
//     features; its slices of W1, W2, W3 and the env matrices stay in registers for the whole
//     rollout -- the per-step critical path has no weight fetches;
//   * per step: L1 5 MFMA -> tanh -> LDS exchange -> L2 16 MFMA -> tanh -> head partial 4 MFMA -> LDS
//     exchange -> action = tanh(mean + std*eps) for the two action dims the lane feeds to the env GEMM ->
//     env step as a 14-MFMA GEMM [obs, act] x [A; B] (every wave: everyone owns next_obs in the
//     operand layout of the next L1) -> reward / done -> partial reset from the Philox reset stream ->
//     ring-buffer row store;
//   * exploration noise (Philox4x32-10 + Box-Muller, ~300 instructions per block) is produced 16 steps
//     at a time, one (step, env) per lane, and parked in LDS -- 1/8 block per lane-step instead of 1.
// The value network is not part of the recurrence: V(obs) for every stored cell, and the over-length
// bootstrap reward + discount * V(next_obs) (on_policy.py:135-143), are computed afterwards by
// `value_pass_kernel` at full-chip parallelism (each wave owns whole 16-sample tiles, all weights in
// registers, layer outputs chain as the next layer's B operand -- no LDS, no barriers).
//
// HBM traffic per env-step: 176 B algorithmic (obs 68 + next_obs 68 + act 24 +
// value/reward/terminal/time_limit 16; the obs read is only at launch) + 4 B
// old_logp (+24 B if host noise is supplied) + 76 B re-read / marker traffic of the value pass.
#include "trl_rollout.h"

// The value pass of a rollout WITHOUT a critic (trl_rollout_t.vf_params == NULL: REINFORCE's ZeroNet, V == 0): what remains of
// value_pass_kernel is its stores.  values of the n_steps x N stored cells (same ring addressing; the rollout left its
// over-length markers there) and boot[0 .. N) become 0.0f, the rewards stay as the rollout wrote them (the bootstrap
// would add discount * 0), and the header goes to the host first, as in the value pass: posted writes, issued before the
// cell stores.  Grid-stride over plain vector stores; nothing is read but the header words.
__global__ __launch_bounds__(256) void zero_value_pass_kernel(float* __restrict__ values, int rows, int top, int N, int n_steps,
                                                              float* __restrict__ boot, uint32_t* __restrict__ pub_dst,
                                                              const uint32_t* __restrict__ pub_src, int64_t pub_words) {
  const int64_t e0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  for (int64_t e = e0; e < pub_words; e += stride) pub_dst[e] = pub_src[e];
  const int64_t M = (int64_t)n_steps * N;
  for (int64_t m = e0; m < M; m += stride) {
    const int t = (int)(m / N), n = (int)(m - (int64_t)t * N);
    values[(size_t)((top + t) % rows) * N + n] = 0.0f;
  }
  if (boot)
    for (int64_t n = e0; n < N; n += stride) boot[n] = 0.0f;
}

// Envs the normalised (cooperative) rollout can carry: its workgroups rendezvous once per step, so all of them
// must be resident at the same time.
template <int D, int H, int A, int ACT>
static int rollout_norm_capacity() {
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, rollout_kernel<D, H, A, ACT, true>, RO_THREADS, 0) != hipSuccess)
    return 0;
  return cus * per_cu * RO_ENVS;
}

int rollout_zero_value(const RolloutDev& d, hipStream_t s) {
  const int64_t blocks = ((int64_t)d.n_steps * d.N + 255) / 256;
  hipLaunchKernelGGL(zero_value_pass_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks)), dim3(256), 0, s, d.values, d.rows,
                     d.top, d.N, d.n_steps, d.boot, d.pub_dst, d.pub_src, d.pub_words);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}
int rollout_value_wait(hipStream_t s, hipEvent_t value_wait) {
  if (value_wait) {                                 // the value function's parameters are still being stepped on another stream
    hipError_t e = hipStreamWaitEvent(s, value_wait, 0);
    if (e != hipSuccess) { trl_set_error("rollout: hipStreamWaitEvent(value_wait_event): %s", hipGetErrorString(e)); return (int)e; }
  }
  return TRL_OK;
}

template <int D, int H, int A, int ACT, bool RT = false, int HEAD = HEAD_GAUSS>
static int launch_rollout(const RolloutDev& d, hipStream_t s, hipEvent_t value_wait = nullptr) {
  const int n_wg = trl_ceil_div(d.N, RO_ENVS);
  if constexpr (RT) {
    if (d.norm_state) { trl_set_error("rollout: the normalised rollout is instantiated for the benchmark shape only"); return TRL_EUNSUPPORTED; }
    RolloutDev e = d;
    e.n_ro_wg = n_wg;
    hipLaunchKernelGGL((rollout_kernel<D, H, A, ACT, false, true, HEAD>), dim3(n_wg + (e.stg_n4 ? RO_STAGERS : 0)), dim3(RO_THREADS), 0, s, e);
  } else if (d.norm_state) {
    const int cap = rollout_norm_capacity<D, H, A, ACT>();
    if (d.norm_update && d.N > cap) {
      trl_set_error("rollout: %d envs with a running normaliser exceed the %d that can be co-resident", d.N, cap);
      return TRL_EUNSUPPORTED;
    }
    hipLaunchKernelGGL((rollout_kernel<D, H, A, ACT, true>), dim3(n_wg), dim3(RO_THREADS), 0, s, d);
  } else {
    RolloutDev e = d;
    e.n_ro_wg = n_wg;
    hipLaunchKernelGGL((rollout_kernel<D, H, A, ACT, false>), dim3(n_wg + (e.stg_n4 ? RO_STAGERS : 0)), dim3(RO_THREADS), 0, s, e);
  }
  TRL_LAUNCH_CHECK();
  if (d.store && !d.vf_params) return rollout_zero_value(d, s);   // no critic: nothing to wait for, nothing to forward
  if (d.store) {
    const int rc = rollout_value_wait(s, value_wait);
    if (rc != TRL_OK) return rc;
    hipLaunchKernelGGL((value_pass_kernel<D, H, ACT, RT>), dim3(value_pass_grid(d)), dim3(VP_THREADS), 0, s, value_dev(d));
    TRL_LAUNCH_CHECK();
  }
  return TRL_OK;
}

// ---- page-locked host block -> device buffer by a kernel, for a stream of its own ----
__global__ __launch_bounds__(256) void stage_h2d_kernel(const f32x4* __restrict__ src, unsigned long long* __restrict__ dst,
                                                        int64_t n4, uint32_t* __restrict__ state, uint32_t stamp) {
  stage_block(src, dst, n4, (int)blockIdx.x, (int)gridDim.x, 256, state, stamp, nullptr);
}
extern "C" int trl_stage_h2d_f32(const float* host_src, float* dev_dst, int64_t n, uint32_t* state, uint32_t stamp,
                                 void* stream) {
  TRL_REQUIRE(n >= 0 && (n & 3) == 0, "stage_h2d: n must be a multiple of 4");
  TRL_REQUIRE(state, "stage_h2d: null state");
  TRL_REQUIRE(!n || (host_src && dev_dst && ((reinterpret_cast<uintptr_t>(host_src) | reinterpret_cast<uintptr_t>(dev_dst)) & 15) == 0),
              "stage_h2d: null / misaligned pointer");
  // few workgroups: the transfer is paced by the host link (~50 GB/s), and they share the chip with the other stream's work
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(16, (n / 4 + 1023) / 1024));
  hipLaunchKernelGGL(stage_h2d_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const f32x4*>(host_src),
                     reinterpret_cast<unsigned long long*>(dev_dst), n / 4, state, stamp);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// Shapes the persistent rollout carries without a normaliser: the benchmark shape (compile-time instantiation, Gaussian
// head) and any 64-wide two-layer pair with 2..32 inputs and the head's range of actions (HEADS, trl_head.h; runtime-dims
// instantiations) -- what the fused update kernels carry (trl_ppo_partial_stride), so such a task is 1 rollout launch +
// 2 launches per minibatch.  A categorical head's outputs are the logits; a state-dependent-std head has 2 A <= 16 rows, one
// MFMA head tile.  Neither runs with a running observation normaliser.
extern "C" int trl_rollout_supported(int D, int H, int A, int act) { return head_supported(HEAD_GAUSS, D, H, A, act); }
extern "C" int trl_rollout_cat_supported(int D, int H, int A, int act) { return head_supported(HEAD_CAT, D, H, A, act); }
extern "C" int trl_rollout_sd_supported(int D, int H, int A, int act) { return head_supported(HEAD_SD, D, H, A, act); }

// head: which entry point (trl_rollout_synth_f32 / _cat_f32 / _sd_f32); cat_seed, cat_env0: the categorical draw's key and
// first global env index; p->A is the number of actions (HEAD_CAT) or of action dims.  Checks *p and fills the launch
// descriptor `d` (nothing is launched; with p->n_steps == 0 the caller has nothing to launch either).
int rollout_synth(const trl_rollout_t* p, int head, int64_t cat_seed, int64_t cat_env0, RolloutDev& d, bool shape_checked) {
  if (!p) { trl_set_error("rollout: null descriptor"); return TRL_EINVAL; }
  TRL_REQUIRE(p->pf_params && p->env_A && p->env_B, "null network / env pointer");   // (vf_params NULL: no critic)
  TRL_REQUIRE(p->cur_obs && p->t_env && p->cur_step && p->episode_idx && p->ep_return, "null env state pointer");
  const bool all_ring = p->obs && p->next_obs && p->acts && p->values && p->rewards && p->terminals && p->time_limits;
  const bool no_ring = !p->obs && !p->next_obs && !p->acts && !p->values && !p->rewards && !p->terminals && !p->time_limits;
  TRL_REQUIRE(all_ring || no_ring, "ring tensors must be all set or all NULL");
  TRL_REQUIRE(p->ep_count && p->ep_log && p->ep_cap >= 0, "null episode log");
  TRL_REQUIRE(p->N > 0 && p->n_steps >= 0 && p->rows > 0, "bad sizes");
  TRL_REQUIRE(p->top >= 0 && p->top < p->rows, "top outside ring");
  TRL_REQUIRE(no_ring || p->n_steps <= p->rows, "n_steps exceeds ring rows");
  TRL_REQUIRE(p->horizon > 0 && p->max_episode_frames > 0, "horizon / max_episode_frames must be positive");
  if (head == HEAD_CAT) {
    TRL_REQUIRE(cat_env0 >= 0, "categorical: negative env offset");
    TRL_REQUIRE(!p->noise && !p->noise_flag && !p->stage_n,
                "categorical: actions are drawn from the device Philox stream only (no host noise block, nothing staged)");
    TRL_REQUIRE(!p->norm_state, "categorical: no running observation normaliser in the persistent rollout");
  }
  if (head == HEAD_SD) {
    TRL_REQUIRE(!p->norm_state, "state-dependent std: no running observation normaliser in the persistent rollout");
    TRL_REQUIRE(!p->noise_flag && !p->stage_n,
                "state-dependent std: the noise block is stream-ordered in front of the launch (no noise gate, nothing staged)");
  }
  if (head != HEAD_GAUSS && !shape_checked && !head_supported(head, p->D, p->H, p->A, p->act)) {
    trl_set_error("rollout: %s shape D=%d H=%d A=%d act=%d not instantiated", HEADS[head].name, p->D, p->H, p->A, p->act);
    return TRL_EUNSUPPORTED;
  }
  if (p->n_steps == 0) return TRL_OK;
  d.pf_params = p->pf_params; d.vf_params = p->vf_params; d.env_A = p->env_A; d.env_B = p->env_B;
  d.reward_scale = p->reward_scale; d.horizon = p->horizon; d.env_seed_base = p->env_seed_base;
  d.cur_obs = p->cur_obs; d.t_env = p->t_env; d.cur_step = p->cur_step; d.episode_idx = p->episode_idx;
  d.ep_return = p->ep_return; d.noise = p->noise; d.noise_step0 = p->noise_step0;
  d.obs = p->obs; d.next_obs = p->next_obs; d.acts = p->acts; d.values = p->values; d.rewards = p->rewards;
  d.terminals = p->terminals; d.time_limits = p->time_limits; d.old_logp = p->old_logp;
  d.rows = p->rows; d.top = p->top; d.N = p->N; d.n_steps = p->n_steps;
  d.max_episode_frames = p->max_episode_frames; d.discount = p->discount;
  d.epoch_reward = p->epoch_reward; d.ep_count = p->ep_count; d.ep_log = p->ep_log; d.ep_cap = p->ep_cap;
  d.step0 = p->step0; d.tanh_action = p->tanh_action; d.deterministic = p->deterministic; d.store = all_ring ? 1 : 0;
  d.norm_state = p->norm_state; d.policy_obs = p->policy_obs; d.norm_ws = p->norm_workspace; d.norm_clip = p->norm_clip;
  d.norm_update = p->norm_update; d.norm_partial_reset = p->normalize_partial_reset;
  d.clear_hdr = p->clear_header; d.boot = all_ring ? p->boot_values : nullptr;
  TRL_REQUIRE(p->publish_words >= 0 && (!p->publish_words || (p->publish_dst && p->publish_src && all_ring)) &&
              ((reinterpret_cast<uintptr_t>(p->publish_dst) | reinterpret_cast<uintptr_t>(p->publish_src)) & 3) == 0,
              "publish: needs ring tensors, non-null 4-byte aligned pointers");
  d.pub_dst = (uint32_t*)p->publish_dst; d.pub_src = (const uint32_t*)p->publish_src; d.pub_words = p->publish_words;
  d.noise_flag = p->noise ? p->noise_flag : nullptr; d.noise_stamp = p->noise_stamp;
  d.n_ro_wg = 0; d.stg_n4 = 0;
  d.cat_seed = cat_seed; d.cat_env0 = cat_env0;
  if (p->stage_n) {
    TRL_REQUIRE(p->stage_n > 0 && (p->stage_n & 3) == 0 && p->stage_src && p->stage_dst && p->stage_ready && p->stage_state &&
                p->stage_ack && !p->norm_state, "stage: n % 4 == 0, non-null pointers, no observation normaliser");
    TRL_REQUIRE(((reinterpret_cast<uintptr_t>(p->stage_src) | reinterpret_cast<uintptr_t>(p->stage_dst)) & 15) == 0,
                "stage: 16-byte aligned blocks");
    d.stg_src = reinterpret_cast<const f32x4*>(p->stage_src); d.stg_dst = reinterpret_cast<unsigned long long*>(p->stage_dst);
    d.stg_n4 = p->stage_n / 4; d.stg_ready = p->stage_ready; d.stg_job = p->stage_job; d.stg_state = p->stage_state;
    d.stg_ack = p->stage_ack;
  }
  TRL_REQUIRE(!p->clear_header || (p->clear_header != p->epoch_reward && (void*)p->clear_header != (void*)p->ep_count),
              "clear_header must not be the header this launch accumulates into");
  TRL_REQUIRE(!p->norm_state || (p->policy_obs && p->norm_workspace), "normaliser needs policy_obs and its workspace");
  d.D = p->D; d.A = p->A;
  return TRL_OK;
}

static int rollout_plain(const trl_rollout_t* p, void* stream, int head, int64_t cat_seed = 0, int64_t cat_env0 = 0) {
  RolloutDev d;
  const int rc = rollout_synth(p, head, cat_seed, cat_env0, d);
  if (rc != TRL_OK || p->n_steps == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t vw = (hipEvent_t)p->value_wait_event;
  if (head == HEAD_GAUSS && p->D == 17 && p->H == 64 && p->A == 6) {               // the benchmark shape, with or without a normaliser
    if (p->act == TRL_ACT_TANH) return launch_rollout<17, 64, 6, TRL_ACT_TANH>(d, s, vw);
    if (p->act == TRL_ACT_RELU) return launch_rollout<17, 64, 6, TRL_ACT_RELU>(d, s, vw);
  }
  if (head_supported(head, p->D, p->H, p->A, p->act) && !p->norm_state)            // runtime-dims instantiations
    return with_head(head, [&](auto hd) {
      return with_tile_act(p->D, p->act, [&](auto tile, auto act) {
        return launch_rollout<decltype(tile)::value, 64, 8, decltype(act)::value, true, decltype(hd)::value>(d, s, vw);
      });
    });
  trl_set_error("rollout: shape D=%d H=%d A=%d act=%d not instantiated", p->D, p->H, p->A, p->act);
  return TRL_EUNSUPPORTED;
}

// The plain halves of a rollout whose other half carries a LayerNorm (k_rollout_ln.hip): the runtime-dims rollout_kernel of
// a head alone, and the runtime-dims value pass alone.  They are launched from this file so that every plain instantiation
// has ONE definition, the one the plain entry points launch.
int rollout_policy_rt(const RolloutDev& d, int head, int act, hipStream_t s) {
  RolloutDev e = d;
  e.n_ro_wg = trl_ceil_div(d.N, RO_ENVS);
  with_head(head, [&](auto hd) {
    return with_tile_act(d.D, act, [&](auto tile, auto ac) {
      hipLaunchKernelGGL((rollout_kernel<decltype(tile)::value, 64, 8, decltype(ac)::value, false, true, decltype(hd)::value>),
                         dim3(e.n_ro_wg), dim3(RO_THREADS), 0, s, e);
      return TRL_OK;
    });
  });
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}
int rollout_value_rt(const RolloutDev& d, int act, hipStream_t s) {
  with_tile_act(d.D, act, [&](auto tile, auto ac) {
    hipLaunchKernelGGL((value_pass_kernel<decltype(tile)::value, 64, decltype(ac)::value, true>), dim3(value_pass_grid(d)),
                       dim3(VP_THREADS), 0, s, value_dev(d));
    return TRL_OK;
  });
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

extern "C" int trl_rollout_synth_f32(const trl_rollout_t* p, void* stream) { return rollout_plain(p, stream, HEAD_GAUSS); }

extern "C" int trl_rollout_synth_cat_f32(const trl_rollout_t* p, int64_t noise_seed, int64_t env_offset, void* stream) {
  return rollout_plain(p, stream, HEAD_CAT, noise_seed, env_offset);
}

extern "C" int trl_rollout_synth_sd_f32(const trl_rollout_t* p, void* stream) { return rollout_plain(p, stream, HEAD_SD); }

extern "C" int trl_rollout_norm_workspace(int N) {
  if (N <= 0) { trl_set_error("trl_rollout_norm_workspace: N must be positive"); return TRL_EINVAL; }
  return 2 + 2 * trl_ceil_div(N, RO_ENVS) * NORM_SLOT;                 // doubles: header + two parities of partials
}
extern "C" int trl_rollout_norm_max_envs(int D, int H, int A, int act) {
  if (D == 17 && H == 64 && A == 6) {
    if (act == TRL_ACT_TANH) return rollout_norm_capacity<17, 64, 6, TRL_ACT_TANH>();
    if (act == TRL_ACT_RELU) return rollout_norm_capacity<17, 64, 6, TRL_ACT_RELU>();
  }
  trl_set_error("rollout: shape D=%d H=%d A=%d act=%d not instantiated", D, H, A, act);
  return TRL_EUNSUPPORTED;
}

// ---------------------------------------------------------------- env (re)start
__global__ __launch_bounds__(256) void synth_reset_kernel(float* __restrict__ cur_obs, int32_t* __restrict__ t_env,
                                                          int32_t* __restrict__ cur_step,
                                                          int32_t* __restrict__ episode_idx,
                                                          float* __restrict__ ep_return,
                                                          const uint8_t* __restrict__ mask, int N, int D,
                                                          int64_t seed_base) {
  const int nblk = (D + 3) / 4;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;     // one thread per (env, 4-feature block)
  const int n = e / nblk, b = e - n * nblk;
  if (n >= N || (mask && !mask[n])) return;
  const int ep = episode_idx[n] + 1;
  float z[4];
  philox_normals4((uint32_t)ep, 0u, (uint32_t)b, TRL_TAG_RESET, seed_base + n, z);
  for (int c = 0; c < 4; ++c) if (4 * b + c < D) cur_obs[(size_t)n * D + 4 * b + c] = z[c];
  if (b == 0) {
    t_env[n] = 0;
    if (!mask) { cur_step[n] = 0; ep_return[n] = 0.0f; }      // collector-side state: full reset only
  }
}
__global__ __launch_bounds__(256) void synth_bump_episode_kernel(int32_t* __restrict__ episode_idx,
                                                                 const uint8_t* __restrict__ mask, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < N && (!mask || mask[n])) episode_idx[n] += 1;
}

extern "C" int trl_synth_reset_f32(float* cur_obs, int32_t* t_env, int32_t* cur_step, int32_t* episode_idx,
                                   float* ep_return, const uint8_t* mask, int N, int D, int64_t env_seed_base,
                                   void* stream) {
  TRL_REQUIRE(cur_obs && t_env && cur_step && episode_idx && ep_return, "null pointer");
  TRL_REQUIRE(N >= 0 && D > 0, "bad sizes");
  if (N == 0) return TRL_OK;
  const int nblk = (D + 3) / 4;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(synth_reset_kernel, dim3(trl_ceil_div((int64_t)N * nblk, 256)), dim3(256), 0, s, cur_obs,
                     t_env, cur_step, episode_idx, ep_return, mask, N, D, env_seed_base);
  TRL_LAUNCH_CHECK();
  // episode_idx is bumped in a second launch: threads of one env may sit in different workgroups
  hipLaunchKernelGGL(synth_bump_episode_kernel, dim3(trl_ceil_div(N, 256)), dim3(256), 0, s, episode_idx, mask, N);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// ---------------------------------------------------------------- diagonal-Gaussian / TanhNormal log-prob
__global__ __launch_bounds__(256) void gauss_logp_kernel(const float* __restrict__ mean, const float* __restrict__ acts,
                                                         const float* __restrict__ logstd, float* __restrict__ out,
                                                         int B, int A, int tanh_action) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float lp = 0.0f;
  for (int o = 0; o < A; ++o) {
    const float ls = fminf(fmaxf(logstd[o], -20.0f), 2.0f);
    float zc;
    lp += gauss_logp_term(acts[(size_t)b * A + o], mean[(size_t)b * A + o], __expf(-2.0f * ls), ls, tanh_action, zc);
  }
  out[b] = lp;
}

extern "C" int trl_gauss_logp_f32(const float* mean, const float* acts, const float* logstd, float* out, int B,
                                  int A, int tanh_action, void* stream) {
  TRL_REQUIRE(B >= 0 && A > 0, "bad sizes");
  if (B == 0) return TRL_OK;
  TRL_REQUIRE(mean && acts && logstd && out, "null pointer");
  hipLaunchKernelGGL(gauss_logp_kernel, dim3(trl_ceil_div(B, 256)), dim3(256), 0, (hipStream_t)stream, mean, acts,
                     logstd, out, B, A, tanh_action);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// ---------------------------------------------------------------- per-step on-policy collection
// The pieces of VecOnPolicyCollector.take_actions (torchrl/collector/on_policy.py:90-155) as stand-alone
// kernels, for environments the persistent rollout kernel cannot carry: with a running observation
// normaliser (NormObs) every step needs batch statistics over ALL envs before the next policy forward.

// pf.explore + log-prob for a state-independent-std Gaussian policy (continuous_policy.py:123-129, 180-188)
__global__ __launch_bounds__(256) void gauss_explore_kernel(const float* __restrict__ mean, const float* __restrict__ logstd,
                                                            const float* __restrict__ eps, float* __restrict__ act,
                                                            float* __restrict__ logp, int N, int A, int tanh_action) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float lp = 0.0f;
  for (int o = 0; o < A; ++o) {
    const float ls = fminf(fmaxf(logstd[o], -20.0f), 2.0f);
    const float m = mean[(size_t)n * A + o];
    const float z = fmaf(__expf(ls), eps ? eps[(size_t)n * A + o] : 0.0f, m);
    const float a = tanh_action ? trl_tanh(z) : z;
    act[(size_t)n * A + o] = a;
    float zc;
    lp += gauss_logp_term(a, m, __expf(-2.0f * ls), ls, tanh_action, zc);
  }
  if (logp) logp[n] = lp;
}

extern "C" int trl_gauss_explore_f32(const float* mean, const float* logstd, const float* eps, float* act, float* logp,
                                     int N, int A, int tanh_action, void* stream) {
  TRL_REQUIRE(N >= 0 && A > 0, "bad sizes");
  if (N == 0) return TRL_OK;
  TRL_REQUIRE(mean && logstd && act, "null pointer");
  hipLaunchKernelGGL(gauss_explore_kernel, dim3(trl_ceil_div(N, 256)), dim3(256), 0, (hipStream_t)stream, mean, logstd,
                     eps, act, logp, N, A, tanh_action);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// bookkeeping after env.step (on_policy.py:124-148): epoch reward, running returns (logged and cleared on done),
// over-length bootstrap r += discount * V(next_obs) * surpass, terminals = done | surpass = reset mask, and a
// device-side "any env flagged" word for the caller's choice of the next policy input (partial_reset, :145-147)
__global__ __launch_bounds__(256) void onpolicy_bookkeep_kernel(float* __restrict__ rew, const float* __restrict__ done,
                                                                const float* __restrict__ v_next, float discount,
                                                                float* __restrict__ terminals, int32_t* __restrict__ cur_step,
                                                                float* __restrict__ ep_return, int max_frames,
                                                                uint8_t* __restrict__ mask, int32_t* __restrict__ any_flag,
                                                                double* __restrict__ epoch_reward, int32_t* __restrict__ ep_count,
                                                                float* __restrict__ ep_log, int ep_cap, int step, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  double r = 0.0;
  bool flag = false;
  if (n < N) {
    const float raw = rew[n];
    r = (double)raw;
    const bool d = done[n] != 0.0f;
    const int cs = cur_step[n] + 1;
    float er = ep_return[n] + raw;
    if (d) {
      const int slot = atomicAdd(ep_count, 1);
      if (slot < ep_cap) { ep_log[slot * 3 + 0] = (float)step; ep_log[slot * 3 + 1] = (float)n; ep_log[slot * 3 + 2] = er; }
      er = 0.0f;
    }
    const bool surpass = cs >= max_frames;
    flag = d || surpass;
    rew[n] = raw + discount * v_next[n] * (surpass ? 1.0f : 0.0f);
    terminals[n] = flag ? 1.0f : 0.0f;
    cur_step[n] = flag ? 0 : cs;
    ep_return[n] = er;
    mask[n] = flag ? 1 : 0;
  }
  const double tot = wave_sum(r);
  if ((threadIdx.x & 63) == 0 && epoch_reward && tot != 0.0) atomicAdd(epoch_reward, tot);
  if (__ballot(flag) != 0ull && (threadIdx.x & 63) == 0) atomicOr(any_flag, 1);
}

extern "C" int trl_onpolicy_bookkeep_f32(float* rewards, const float* dones, const float* v_next, float discount,
                                         float* terminals, int32_t* cur_step, float* ep_return, int max_episode_frames,
                                         uint8_t* reset_mask, int32_t* any_flag, double* epoch_reward, int32_t* ep_count,
                                         float* ep_log, int ep_cap, int step, int N, void* stream) {
  TRL_REQUIRE(N >= 0 && ep_cap >= 0, "bad sizes");
  if (N == 0) return TRL_OK;
  TRL_REQUIRE(rewards && dones && v_next && terminals && cur_step && ep_return && reset_mask && any_flag && ep_count && ep_log,
              "null pointer");
  hipLaunchKernelGGL(onpolicy_bookkeep_kernel, dim3(trl_ceil_div(N, 256)), dim3(256), 0, (hipStream_t)stream, rewards,
                     dones, v_next, discount, terminals, cur_step, ep_return, max_episode_frames, reset_mask, any_flag,
                     epoch_reward, ep_count, ep_log, ep_cap, step, N);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// out = (*flag != 0) ? a : b, elementwise -- the flag stays on the device (no host round trip per step)
__global__ __launch_bounds__(256) void select_on_flag_kernel(const int32_t* __restrict__ flag, const float* __restrict__ a,
                                                             const float* __restrict__ b, float* __restrict__ out, int64_t n) {
  const bool f = *flag != 0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) out[e] = f ? a[e] : b[e];
}

extern "C" int trl_select_on_flag_f32(const int32_t* flag, const float* a, const float* b, float* out, int64_t n,
                                      void* stream) {
  TRL_REQUIRE(n >= 0, "negative size");
  if (n == 0) return TRL_OK;
  TRL_REQUIRE(flag && a && b && out, "null pointer");
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(select_on_flag_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks)), dim3(256), 0,
                     (hipStream_t)stream, flag, a, b, out, n);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// out = any(mask[0..N)) ? a : b, elementwise -- the off-policy collector's form of the same whole-array return
// (torchrl/collector/base.py:220-224): every block scans the (few-KB) reset mask itself, no flag word, no host sync
__global__ __launch_bounds__(256) void select_on_mask_kernel(const uint8_t* __restrict__ mask, int N, const float* __restrict__ a,
                                                             const float* __restrict__ b, float* __restrict__ out, int64_t n) {
  int any = 0;
  for (int e = threadIdx.x; e < N; e += 256) any |= mask[e];
  const bool f = __syncthreads_or(any) != 0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) out[e] = f ? a[e] : b[e];
}

extern "C" int trl_select_on_mask_f32(const uint8_t* mask, int N, const float* a, const float* b, float* out, int64_t n,
                                      void* stream) {
  TRL_REQUIRE(n >= 0 && N >= 0, "negative size");
  if (n == 0) return TRL_OK;
  TRL_REQUIRE(mask && a && b && out, "null pointer");
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(select_on_mask_kernel, dim3((unsigned)(blocks > 256 ? 256 : blocks)), dim3(256), 0,
                     (hipStream_t)stream, mask, N, a, b, out, n);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}
