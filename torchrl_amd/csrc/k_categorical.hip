// Categorical (discrete-action) policy heads for the on-policy algorithms
// (reference: torchrl/policies/discrete_policies.py:124-168 CategoricalDisPolicy; torchrl/algo/on_policy/ppo.py:41-152,
// a2c.py:45-106 with that policy).
//
//   trl_cat_act_f32         one vector step's action half: logits (N, A) -> action (N, 1), log pi(a) (N), one-hot (N, A)
//                           -- the counterpart of trl_gauss_explore_f32
//   trl_philox_uniform_f32  the uniforms trl_cat_act_f32 would draw for steps counter0 .. counter0 + T - 1, (T, N)
//   trl_cat_losses_f32      the loss half of PPO.update / A2C.update -- the counterpart of trl_ppo_generic_losses_f32,
//                           same inputs, outputs and two-pass fold (trl_ppo_loss.h)
//
// Fixed arithmetic (tests/_categorical_ref.py restates it): m = max_k l_k, e_k = exp(l_k - m), S = sum_k e_k and its
// prefix sums in ascending k in fp32, p_k = e_k / S, log p_k = (l_k - m) - log S.
// One thread owns one row: A <= 64 logits are 256 bytes, re-read from L1 per pass instead of held in registers (A is a
// run-time value); the ascending-k sums the semantics fix are a per-thread loop anyway.
#include "trl_common.h"
#include "trl_cat.h"
#include "trl_philox.h"
#include "trl_ppo_loss.h"

#define CAT_THREADS 256

__global__ __launch_bounds__(CAT_THREADS) void cat_act_kernel(const float* __restrict__ logits, const float* __restrict__ u_in,
                                                              int64_t seed, int64_t ctr, int64_t env_offset,
                                                              int deterministic, float* __restrict__ act,
                                                              float* __restrict__ logp, float* __restrict__ onehot, int N,
                                                              int A) {
  const int n = blockIdx.x * CAT_THREADS + threadIdx.x;
  if (n >= N) return;
  const float* l = logits + (size_t)n * A;
  int a;
  const float m = cat_row_max(l, A, a);
  float S = 0.0f;
  for (int k = 0; k < A; ++k) S += expf(l[k] - m);
  if (!deterministic) {
    const float u = u_in ? u_in[n] : trl_cat_uniform(seed, ctr, env_offset + n);
    const float thr = u * S;
    float c = 0.0f;
    a = A - 1;
    for (int k = 0; k < A; ++k) {
      c += expf(l[k] - m);
      if (c >= thr) { a = k; break; }
    }
  }
  act[n] = (float)a;
  if (logp) logp[n] = (l[a] - m) - logf(S);
  if (onehot)
    for (int k = 0; k < A; ++k) onehot[(size_t)n * A + k] = k == a ? 1.0f : 0.0f;
}

extern "C" int trl_cat_act_f32(const float* logits, const float* u, int64_t seed, int64_t counter, int64_t env_offset,
                               int deterministic, float* act, float* logp, float* onehot, int N, int A, void* stream) {
  TRL_REQUIRE(N >= 0 && A >= 2 && A <= PG_MAX_A, "bad sizes (2 <= A <= 64)");
  TRL_REQUIRE(env_offset >= 0, "negative env offset");
  if (N == 0) return TRL_OK;
  TRL_REQUIRE(logits && act, "null pointer");
  hipLaunchKernelGGL(cat_act_kernel, dim3(trl_ceil_div(N, CAT_THREADS)), dim3(CAT_THREADS), 0, (hipStream_t)stream, logits, u,
                     seed, counter, env_offset, deterministic, act, logp, onehot, N, A);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

__global__ __launch_bounds__(CAT_THREADS) void philox_uniform_kernel(float* __restrict__ out, int64_t total, int N, int64_t seed,
                                                                     int64_t ctr0, int64_t env_offset) {
  const int64_t e = (int64_t)blockIdx.x * CAT_THREADS + threadIdx.x;
  if (e >= total) return;
  out[e] = trl_cat_uniform(seed, ctr0 + e / N, env_offset + e % N);
}

extern "C" int trl_philox_uniform_f32(float* out, int T, int N, int64_t seed, int64_t counter0, int64_t env_offset,
                                      void* stream) {
  TRL_REQUIRE(T >= 0 && N >= 0 && env_offset >= 0, "bad sizes");
  const int64_t total = (int64_t)T * N;
  if (total == 0) return TRL_OK;
  TRL_REQUIRE(out, "null pointer");
  hipLaunchKernelGGL(philox_uniform_kernel, dim3(trl_ceil_div(total, CAT_THREADS)), dim3(CAT_THREADS), 0, (hipStream_t)stream,
                     out, total, N, seed, counter0, env_offset);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// log pi(a) (B), the entropy (B) and the probabilities (B, A) of (logits, stored action) pairs: CategoricalDisPolicy.forward
// / .update without autograd; every output is optional
__global__ __launch_bounds__(CAT_THREADS) void cat_logp_kernel(const float* __restrict__ logits, const float* __restrict__ acts,
                                                               float* __restrict__ logp, float* __restrict__ ent,
                                                               float* __restrict__ probs, int B, int A) {
  const int b = blockIdx.x * CAT_THREADS + threadIdx.x;
  if (b >= B) return;
  const float* l = logits + (size_t)b * A;
  int arg;
  const float m = cat_row_max(l, A, arg);
  float S = 0.0f;
  for (int k = 0; k < A; ++k) S += expf(l[k] - m);
  const float logS = logf(S);
  if (logp) {
    const int a = min(max((int)acts[b], 0), A - 1);
    logp[b] = (l[a] - m) - logS;
  }
  if (ent || probs) {
    float H = 0.0f;
    for (int k = 0; k < A; ++k) {
      const float p = expf(l[k] - m) / S;
      H -= p * ((l[k] - m) - logS);
      if (probs) probs[(size_t)b * A + k] = p;
    }
    if (ent) ent[b] = H;
  }
}

extern "C" int trl_cat_logp_f32(const float* logits, const float* acts, float* logp, float* ent, float* probs, int B, int A,
                                void* stream) {
  TRL_REQUIRE(B >= 0 && A >= 2 && A <= PG_MAX_A, "bad sizes (2 <= A <= 64)");
  if (B == 0) return TRL_OK;
  TRL_REQUIRE(logits && (logp || ent || probs), "null pointer");
  TRL_REQUIRE(!logp || acts, "log pi needs the actions");
  hipLaunchKernelGGL(cat_logp_kernel, dim3(trl_ceil_div(B, CAT_THREADS)), dim3(CAT_THREADS), 0, (hipStream_t)stream, logits,
                     acts, logp, ent, probs, B, A);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

struct CatLossDev {
  const float* logits; const float* acts; const float* advs; const float* old_logp;
  const float* v; const float* rets; const float* v_old;
  const double* adv_raw;
  float* d_logits; float* d_v; double* partial;     // partial: [blocks][1 + PG_SCAL], entropy sum first
  int B, A;
  float clip_para, entropy_coeff;
  int clipped_value_loss, loss_mode;
  double n_global;
};

__global__ __launch_bounds__(PG_THREADS) void cat_losses_kernel(CatLossDev a) {
  __shared__ double smem[PG_THREADS / 64];
  const int b = blockIdx.x * PG_THREADS + threadIdx.x;
  const bool valid = b < a.B;
  const int A = a.A;
  const PgAdvNorm nrm = pg_adv_norm(a.adv_raw, a.n_global);
  const float inv_b = nrm.inv_b;

  // ---- policy: softmax, log pi, entropy, surrogate, d/d(logits) ----
  float lp = 0.0f, H = 0.0f, m = 0.0f, S = 1.0f, logS = 0.0f;
  int act = 0;
  const float* l = a.logits + (size_t)(valid ? b : 0) * A;
  if (valid) {
    int arg;
    m = cat_row_max(l, A, arg);
    S = 0.0f;
    for (int k = 0; k < A; ++k) S += expf(l[k] - m);
    logS = logf(S);
    act = min(max((int)a.acts[b], 0), A - 1);
    lp = (l[act] - m) - logS;
    for (int k = 0; k < A; ++k) {
      const float p = expf(l[k] - m) / S;
      H -= p * ((l[k] - m) - logS);
    }
  }
  const float advn = valid ? (a.advs[b] - nrm.mu) * nrm.rstd : 0.0f;
  float ratio, s1, s2, g_lp;
  pg_surrogate(valid, lp, a.old_logp, b, advn, a.loss_mode, a.clip_para, inv_b, ratio, s1, s2, g_lp);
  if (valid) {
    const float ce = a.entropy_coeff * inv_b;
    for (int k = 0; k < A; ++k) {
      const float lpk = (l[k] - m) - logS;
      const float p = expf(l[k] - m) / S;
      a.d_logits[(size_t)b * A + k] = g_lp * ((k == act ? 1.0f : 0.0f) - p) + ce * p * (lpk + H);
    }
  }
  // ---- value: loss and d/d(v) ----
  const bool critic = a.loss_mode != TRL_LOSS_REINFORCE;
  float vv = 0.0f, vl = 0.0f;
  if (valid && critic) {
    vv = a.v[b];
    float dv;
    pg_value_loss(vv, a.rets[b], a.v_old, b, a.clip_para, a.clipped_value_loss, inv_b, vl, dv);
    a.d_v[b] = dv;
  }
  // ---- block partials ----
  double* out = a.partial + (size_t)blockIdx.x * (1 + PG_SCAL);
  const double hs = pg_block_reduce((double)H, false, smem);
  if (threadIdx.x == 0) out[0] = hs;
  pg_write_scalars(out + 1, valid, lp, ratio, s1, s2, vl, vv, smem, critic);
}

extern "C" int trl_cat_losses_workspace(int B, int A) {
  if (B <= 0 || A < 2 || A > PG_MAX_A) return TRL_EINVAL;
  return trl_ceil_div(B, PG_THREADS) * (1 + PG_SCAL);            // doubles
}

extern "C" int trl_cat_losses_f32(const float* logits, const float* acts, const float* advs, const float* old_logp,
                                  const float* v, const float* rets, const float* v_old, const double* adv_raw,
                                  double n_global, int B, int A, float clip_para, float entropy_coeff,
                                  int clipped_value_loss, int loss_mode, float* d_logits, float* d_v, double* info,
                                  double* workspace, void* stream) {
  TRL_REQUIRE(B > 0 && A >= 2 && A <= PG_MAX_A, "bad sizes (2 <= A <= 64)");
  TRL_REQUIRE(logits && acts && advs && adv_raw && d_logits && info && workspace, "null pointer");
  PG_REQUIRE_MODE(loss_mode, old_logp, v, rets, v_old, d_v, clipped_value_loss);
  TRL_REQUIRE(n_global >= 2.0, "need at least two samples for the advantage statistics");
  CatLossDev a{};
  a.logits = logits; a.acts = acts; a.advs = advs; a.old_logp = old_logp; a.v = v; a.rets = rets; a.v_old = v_old;
  a.adv_raw = adv_raw; a.d_logits = d_logits; a.d_v = d_v; a.partial = workspace; a.B = B; a.A = A;
  a.clip_para = clip_para; a.entropy_coeff = entropy_coeff; a.clipped_value_loss = clipped_value_loss;
  a.loss_mode = loss_mode; a.n_global = n_global;
  const int blocks = trl_ceil_div(B, PG_THREADS);
  hipLaunchKernelGGL(cat_losses_kernel, dim3(blocks), dim3(PG_THREADS), 0, (hipStream_t)stream, a);
  TRL_LAUNCH_CHECK();
  return pg_launch_fold(workspace, blocks, 1, nullptr, nullptr, info, (hipStream_t)stream);
}
