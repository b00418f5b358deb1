// State-dependent-std Gaussian policy heads for the on-policy algorithms
// (reference: torchrl/policies/continuous_policy.py:134-170 GuassianContPolicy -- the head emits [mean | log_std],
// log_std clamped to [-20, 2] per sample; torchrl/algo/on_policy/ppo.py:41-152, a2c.py:45-106 with that policy).
//
//   trl_gauss_sd_explore_f32  one vector step's action half: head (N, 2A), eps (N, A) -> act (N, A), log pi(act) (N)
//                             -- the counterpart of trl_gauss_explore_f32
//   trl_gauss_sd_logp_f32     log pi (B) and the entropy (B) of stored (head, action) pairs
//   trl_gauss_sd_losses_f32   the loss half of PPO.update / A2C.update -- the counterpart of trl_ppo_generic_losses_f32,
//                             same inputs, outputs and two-pass fold (trl_ppo_loss.h)
//
// Per element: ls = clamp(head[A + o], -20, 2), log pi term = gauss_logp_term(act, head[o], exp(-2 ls), ls) (trl_mlp.h,
// the reference's atanh / log(1 - a^2 + 1e-6) form for tanh actions).  All three kernels sum the terms of a row through
// ONE helper in ascending o, so log pi and log pi_old of the same (head, action) are bit-identical (ratio == 1).
// One thread owns one row (A is a run-time value, the row is walked in a loop).  Neighbouring lanes therefore touch head /
// d_head at a stride of 2A floats -- 256 bytes at A = 32 -- so the first read and the writes are NOT coalesced; only the
// second pass over a row finds it in L1.  These launches are small next to the dense-layer GEMMs around them and the route
// is untimed (profiles/NOTES_state_std.md lists the access pattern among what is unmeasured).
#include "trl_common.h"
#include "trl_mlp.h"
#include "trl_ppo_loss.h"

#define SD_THREADS 256
#define SD_MAX_A 32         // 2A <= PG_MAX_A
// what a block adds in front of the PG_SCAL scalars: entropy sum | log_std sum, sum of squares | std sum, sum of squares |
// log_std max, -min | std max, -min
#define SD_VEC 9
#define SD_HALF_LOG_2PI_PLUS_HALF 1.4189385332046727f

__device__ __forceinline__ float sd_clamp(float raw) { return fminf(fmaxf(raw, -20.0f), 2.0f); }

// log pi of one row, and its entropy sum_o (1/2 + 1/2 log 2 pi + ls) (the reference's TanhNormal.entropy is the Normal's)
__device__ __forceinline__ float sd_row_logp(const float* head, const float* act, int A, int tanh_action, float& ent) {
  float lp = 0.0f, h = 0.0f;
  for (int o = 0; o < A; ++o) {
    const float ls = sd_clamp(head[A + o]);
    float zc;
    lp += gauss_logp_term(act[o], head[o], __expf(-2.0f * ls), ls, tanh_action, zc);
    h += SD_HALF_LOG_2PI_PLUS_HALF + ls;
  }
  ent = h;
  return lp;
}

// pf.explore + log-prob (continuous_policy.py:92-131, 156-170); eps NULL: the deterministic action [tanh](mean)
__global__ __launch_bounds__(SD_THREADS) void gauss_sd_explore_kernel(const float* __restrict__ head, const float* __restrict__ eps,
                                                                      float* act, float* __restrict__ logp, int N, int A,
                                                                      int tanh_action) {
  const int n = blockIdx.x * SD_THREADS + threadIdx.x;
  if (n >= N) return;
  const float* h = head + (size_t)n * 2 * A;
  float* a = act + (size_t)n * A;
  for (int o = 0; o < A; ++o) {
    const float ls = sd_clamp(h[A + o]);
    const float z = fmaf(__expf(ls), eps ? eps[(size_t)n * A + o] : 0.0f, h[o]);
    a[o] = tanh_action ? trl_tanh(z) : z;
  }
  if (logp) {
    float ent;
    logp[n] = sd_row_logp(h, a, A, tanh_action, ent);          // (reads back what this thread stored: the stored action)
  }
}

extern "C" int trl_gauss_sd_explore_f32(const float* head, const float* eps, float* act, float* logp, int N, int A,
                                        int tanh_action, void* stream) {
  TRL_REQUIRE(N >= 0 && A >= 1 && A <= SD_MAX_A, "bad sizes (1 <= A <= 32)");
  if (N == 0) return TRL_OK;
  TRL_REQUIRE(head && act, "null pointer");
  hipLaunchKernelGGL(gauss_sd_explore_kernel, dim3(trl_ceil_div(N, SD_THREADS)), dim3(SD_THREADS), 0, (hipStream_t)stream,
                     head, eps, act, logp, N, A, tanh_action);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// GuassianContPolicyBase.update without autograd (continuous_policy.py:134-153): log_prob.sum(-1) and ent.sum(-1)
__global__ __launch_bounds__(SD_THREADS) void gauss_sd_logp_kernel(const float* __restrict__ head, const float* __restrict__ acts,
                                                                   float* __restrict__ logp, float* __restrict__ ent, int B,
                                                                   int A, int tanh_action) {
  const int b = blockIdx.x * SD_THREADS + threadIdx.x;
  if (b >= B) return;
  float h;
  const float lp = sd_row_logp(head + (size_t)b * 2 * A, acts + (size_t)b * A, A, tanh_action, h);
  if (logp) logp[b] = lp;
  if (ent) ent[b] = h;
}

extern "C" int trl_gauss_sd_logp_f32(const float* head, const float* acts, float* logp, float* ent, int B, int A,
                                     int tanh_action, void* stream) {
  TRL_REQUIRE(B >= 0 && A >= 1 && A <= SD_MAX_A, "bad sizes (1 <= A <= 32)");
  if (B == 0) return TRL_OK;
  TRL_REQUIRE(head && acts && (logp || ent), "null pointer");
  hipLaunchKernelGGL(gauss_sd_logp_kernel, dim3(trl_ceil_div(B, SD_THREADS)), dim3(SD_THREADS), 0, (hipStream_t)stream, head,
                     acts, logp, ent, B, A, tanh_action);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

struct GaussSdLossDev {
  const float* head; const float* acts; const float* advs; const float* old_logp;
  const float* v; const float* rets; const float* v_old;
  const double* adv_raw;
  float* d_head; float* d_v; double* partial;       // partial: [blocks][SD_VEC + PG_SCAL]
  int B, A;
  float clip_para, entropy_coeff;
  int clipped_value_loss, tanh_action, loss_mode;
  double n_global;
};

__global__ __launch_bounds__(PG_THREADS) void gauss_sd_losses_kernel(GaussSdLossDev a) {
  __shared__ double smem[PG_THREADS / 64];
  const int b = blockIdx.x * PG_THREADS + threadIdx.x;
  const bool valid = b < a.B;
  const int A = a.A;
  const PgAdvNorm nrm = pg_adv_norm(a.adv_raw, a.n_global);
  const float inv_b = nrm.inv_b;
  const float* h = a.head + (size_t)(valid ? b : 0) * 2 * A;
  const float* act = a.acts + (size_t)(valid ? b : 0) * A;

  // ---- policy: log pi, entropy, surrogate, d/d(head) ----
  float lp = 0.0f, ent = 0.0f;
  if (valid) lp = sd_row_logp(h, act, A, a.tanh_action, ent);
  const float advn = valid ? (a.advs[b] - nrm.mu) * nrm.rstd : 0.0f;
  float ratio, s1, s2, g_lp;
  pg_surrogate(valid, lp, a.old_logp, b, advn, a.loss_mode, a.clip_para, inv_b, ratio, s1, s2, g_lp);
  const double ninf = -INFINITY;
  double ls_s = 0.0, ls_q = 0.0, sd_s = 0.0, sd_q = 0.0, ls_mx = ninf, ls_mn = ninf, sd_mx = ninf, sd_mn = ninf;
  if (valid) {
    float* d = a.d_head + (size_t)b * 2 * A;
    const float ce = a.entropy_coeff * inv_b;
    for (int o = 0; o < A; ++o) {
      const float raw = h[A + o];
      const float ls = sd_clamp(raw);
      const float gate = (raw >= -20.0f && raw <= 2.0f) ? 1.0f : 0.0f;   // d clamp / d raw, the `pass` of the logstd head
      const float ivv = __expf(-2.0f * ls);
      float zc;
      gauss_logp_term(act[o], h[o], ivv, ls, a.tanh_action, zc);
      d[o] = g_lp * zc * ivv;
      d[A + o] = gate * (g_lp * (zc * zc * ivv - 1.0f) - ce);
      const double x = (double)ls, ex = (double)expf(ls);               // ppo.py:83-86 log_std/*, a2c.py:96-101 std/*
      ls_s += x; ls_q += x * x; ls_mx = fmax(ls_mx, x); ls_mn = fmax(ls_mn, -x);
      sd_s += ex; sd_q += ex * ex; sd_mx = fmax(sd_mx, ex); sd_mn = fmax(sd_mn, -ex);
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
  double* out = a.partial + (size_t)blockIdx.x * (SD_VEC + PG_SCAL);
  const double vec[SD_VEC] = {(double)ent, ls_s, ls_q, sd_s, sd_q, ls_mx, ls_mn, sd_mx, sd_mn};
#pragma unroll
  for (int k = 0; k < SD_VEC; ++k) {
    const double r = pg_block_reduce(vec[k], k >= 5, smem);
    if (threadIdx.x == 0) out[k] = r;
  }
  pg_write_scalars(out + SD_VEC, valid, lp, ratio, s1, s2, vl, vv, smem, critic);
}

// one block: fold the block partials in order into the info row (trl_ppo_reduce_f32's layout); n_elem = B * A
__global__ __launch_bounds__(PG_THREADS) void gauss_sd_fold_kernel(const double* __restrict__ partial, int blocks, double n_elem,
                                                                   double* __restrict__ info) {
  __shared__ double s_out[SD_VEC + PG_SCAL];
  const int stride = SD_VEC + PG_SCAL;
  for (int e = threadIdx.x; e < stride; e += PG_THREADS) {
    const int k = e - SD_VEC;
    const bool is_max = k < 0 ? e >= 5 : (k == 2 || k == 3 || k == 4 || k == 5 || k == 10 || k == 11);
    double r = is_max ? -INFINITY : 0.0;
    for (int w = 0; w < blocks; ++w) {
      const double o = partial[(size_t)w * stride + e];
      r = is_max ? fmax(r, o) : r + o;
    }
    s_out[e] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double* s = s_out + SD_VEC;
    info[0] = s[6]; info[1] = s[0]; info[2] = s[1]; info[3] = s[2]; info[4] = s[3]; info[5] = s[4]; info[6] = s[5];
    info[7] = s[7]; info[12] = s[8]; info[13] = s[9]; info[14] = s[10]; info[15] = s[11];
    const double n = n_elem, lm = s_out[1] / n, em = s_out[3] / n;
    info[8] = lm; info[9] = n > 1.0 ? sqrt(fmax((s_out[2] - s_out[1] * lm) / (n - 1.0), 0.0)) : NAN;
    info[10] = s_out[5]; info[11] = -s_out[6];
    info[16] = em; info[17] = n > 1.0 ? sqrt(fmax((s_out[4] - s_out[3] * em) / (n - 1.0), 0.0)) : NAN;
    info[18] = s_out[7]; info[19] = -s_out[8];
    info[20] = s_out[0];
  }
}

extern "C" int trl_gauss_sd_losses_workspace(int B, int A) {
  if (B <= 0 || A < 1 || A > SD_MAX_A) return TRL_EINVAL;
  return trl_ceil_div(B, PG_THREADS) * (SD_VEC + PG_SCAL);       // doubles
}

extern "C" int trl_gauss_sd_losses_f32(const float* head, const float* acts, const float* advs, const float* old_logp,
                                       const float* v, const float* rets, const float* v_old, const double* adv_raw,
                                       double n_global, int B, int A, float clip_para, float entropy_coeff,
                                       int clipped_value_loss, int tanh_action, int loss_mode, float* d_head, float* d_v,
                                       double* info, double* workspace, void* stream) {
  TRL_REQUIRE(B > 0 && A >= 1 && A <= SD_MAX_A, "bad sizes (1 <= A <= 32)");
  TRL_REQUIRE(head && acts && advs && adv_raw && d_head && info && workspace, "null pointer");
  PG_REQUIRE_MODE(loss_mode, old_logp, v, rets, v_old, d_v, clipped_value_loss);
  TRL_REQUIRE(n_global >= 2.0, "need at least two samples for the advantage statistics");
  GaussSdLossDev a{};
  a.head = head; a.acts = acts; a.advs = advs; a.old_logp = old_logp; a.v = v; a.rets = rets; a.v_old = v_old;
  a.adv_raw = adv_raw; a.d_head = d_head; a.d_v = d_v; a.partial = workspace; a.B = B; a.A = A;
  a.clip_para = clip_para; a.entropy_coeff = entropy_coeff; a.clipped_value_loss = clipped_value_loss;
  a.tanh_action = tanh_action; a.loss_mode = loss_mode; a.n_global = n_global;
  const int blocks = trl_ceil_div(B, PG_THREADS);
  hipLaunchKernelGGL(gauss_sd_losses_kernel, dim3(blocks), dim3(PG_THREADS), 0, (hipStream_t)stream, a);
  TRL_LAUNCH_CHECK();
  hipLaunchKernelGGL(gauss_sd_fold_kernel, dim3(1), dim3(PG_THREADS), 0, (hipStream_t)stream, workspace, blocks,
                     (double)B * A, info);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}
