// What the stand-alone loss kernels of PPO.update / A2C.update share, whatever the policy head
// (k_ppo_generic.hip: diagonal Gaussian, k_categorical.hip: categorical): advantage normalisation, the surrogate with
// its clip / tie conventions, the value loss, and the two-pass deterministic fold of the per-block statistics.
// (reference: torchrl/algo/on_policy/ppo.py:41-152, a2c.py:29-106)
#pragma once
#include "trl_common.h"

#define PG_THREADS 256
#define PG_MAX_A 64
#define PG_SCAL 12          // lp sum, lp^2, max lp, -min lp, max ratio, -min ratio, surrogate sum | vloss, v sum, v^2, max v, -min v

__device__ __forceinline__ double pg_block_reduce(double v, bool is_max, double* smem) {
  v = is_max ? wave_max(v) : wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) smem[wave] = v;
  __syncthreads();
  double r = is_max ? -INFINITY : 0.0;
  for (int w = 0; w < PG_THREADS / 64; ++w) r = is_max ? fmax(r, smem[w]) : r + smem[w];
  return r;
}

// advantage normalisation constants (ppo.py:141-147): mean, 1 / (unbiased std + 1e-5), 1 / n
struct PgAdvNorm { float mu, rstd, inv_b; };
__device__ __forceinline__ PgAdvNorm pg_adv_norm(const double* __restrict__ adv_raw, double ng) {
  const double adv_mean = adv_raw[0] / ng;
  const double adv_var = (adv_raw[1] - adv_raw[0] * adv_raw[0] / ng) / (ng - 1.0);
  PgAdvNorm n;
  n.mu = (float)adv_mean;
  n.rstd = 1.0f / ((float)sqrt(fmax(adv_var, 0.0)) + 1e-5f);
  n.inv_b = (float)(1.0 / ng);
  return n;
}

// the policy objective of one sample given its log pi: ratio, both surrogates and g_lp = d(loss)/d(log pi)
__device__ __forceinline__ void pg_surrogate(bool valid, float lp, const float* __restrict__ old_logp, int b, float advn,
                                             int loss_mode, float clip_para, float inv_b, float& ratio, float& s1,
                                             float& s2, float& g_lp) {
  if (loss_mode == TRL_LOSS_A2C || loss_mode == TRL_LOSS_REINFORCE) {   // L = -mean(log pi * adv) (a2c.py:69-70, reinforce.py:59)
    ratio = 1.0f;
    s1 = s2 = lp * advn;
    g_lp = valid ? -advn * inv_b : 0.0f;
  } else {                                                       // clipped surrogate (ppo.py:58-66)
    ratio = valid ? __expf(lp - old_logp[b]) : 1.0f;
    s1 = ratio * advn;
    s2 = fminf(fmaxf(ratio, 1.0f - clip_para), 1.0f + clip_para) * advn;
    g_lp = (valid && s1 <= s2) ? -advn * ratio * inv_b : 0.0f;
  }
}

// value loss of one sample and d(value loss)/d(v)
__device__ __forceinline__ void pg_value_loss(float vv, float R, const float* __restrict__ v_old, int b, float clip_para,
                                              int clipped_value_loss, float inv_b, float& l, float& dv) {
  if (clipped_value_loss) {                                      // ppo.py:104-111
    const float vo = v_old[b];
    const float dc = vv - vo;
    const float vc = vo + fminf(fmaxf(dc, -clip_para), clip_para);
    const float l1 = (vv - R) * (vv - R), l2 = (vc - R) * (vc - R);
    const float wa = l1 > l2 ? 1.0f : (l1 == l2 ? 0.5f : 0.0f), wb = 1.0f - wa;
    const float pass = (dc >= -clip_para && dc <= clip_para) ? 1.0f : 0.0f;
    l = 0.5f * fmaxf(l1, l2);
    dv = inv_b * (wa * (vv - R) + wb * pass * (vc - R));
  } else {                                                       // nn.MSELoss, a2c.py:43
    l = (vv - R) * (vv - R);
    dv = 2.0f * (vv - R) * inv_b;
  }
}

// the PG_SCAL scalar statistics of a block into out[0 .. PG_SCAL) (every thread of the block calls this)
// critic false (TRL_LOSS_REINFORCE, block-uniform): the five value-side entries are stored as 0.0 without a reduction
__device__ __forceinline__ void pg_write_scalars(double* __restrict__ out, bool valid, float lp, float ratio, float s1,
                                                 float s2, float l, float vv, double* smem, bool critic = true) {
  const double ninf = -INFINITY;
  const double vals[PG_SCAL] = {valid ? (double)lp : 0.0, valid ? (double)lp * lp : 0.0, valid ? (double)lp : ninf,
                                valid ? -(double)lp : ninf, valid ? (double)ratio : ninf, valid ? -(double)ratio : ninf,
                                valid ? -(double)fminf(s1, s2) : 0.0, (double)l, (double)vv, (double)vv * vv,
                                valid ? (double)vv : ninf, valid ? -(double)vv : ninf};
  const bool is_max[PG_SCAL] = {false, false, true, true, true, true, false, false, false, false, true, true};
#pragma unroll
  for (int k = 0; k < PG_SCAL; ++k) {
    if (k >= 7 && !critic) {
      if (threadIdx.x == 0) out[k] = 0.0;
      continue;
    }
    const double r = pg_block_reduce(vals[k], is_max[k], smem);
    if (threadIdx.x == 0) out[k] = r;
  }
}

// what the three loss entry points check alike: TRL_LOSS_REINFORCE runs without v / rets / v_old / d_v / old_logp
#define PG_REQUIRE_MODE(loss_mode, old_logp, v, rets, v_old, d_v, clipped_value_loss)                                   \
  do {                                                                                                                  \
    TRL_REQUIRE((loss_mode) == TRL_LOSS_PPO_CLIP || (loss_mode) == TRL_LOSS_A2C || (loss_mode) == TRL_LOSS_REINFORCE,   \
                "unknown loss_mode");                                                                                   \
    TRL_REQUIRE((loss_mode) == TRL_LOSS_REINFORCE || ((v) && (rets) && (d_v)), "null pointer");                         \
    TRL_REQUIRE((loss_mode) != TRL_LOSS_REINFORCE || !(clipped_value_loss),                                             \
                "TRL_LOSS_REINFORCE has no value loss: clipped_value_loss must be 0");                                  \
    TRL_REQUIRE((loss_mode) != TRL_LOSS_PPO_CLIP || (old_logp), "the clipped surrogate needs old_logp");                \
    TRL_REQUIRE(!(clipped_value_loss) || (v_old), "the clipped value loss needs the old values");                       \
  } while (0)

// Second pass (one block, fixed order): partial is [blocks][n_vec + PG_SCAL]; the n_vec leading sums go to vec_out (as
// floats) and the scalars to the info row (trl_ppo_reduce_f32's layout).  logstd given (n_vec == A, Gaussian head): its
// statistics fill info[8..11] / [16..19]; logstd NULL (categorical head, n_vec == 1): those slots are written as zero and
// the leading sum -- the entropy sum of the local samples -- goes to info[20].  Defined in k_ppo_generic.hip.
int pg_launch_fold(const double* partial, int blocks, int n_vec, const float* logstd, float* vec_out, double* info,
                   hipStream_t stream);
