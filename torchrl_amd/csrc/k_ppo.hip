// K8 + K9 + K10 -- fused PPO minibatch gradient on fp32 MFMA, plus the partial
// reduction, the global-norm-clip + Adam step (K11) and MLP inference.
//
// Replaces the tensor work of PPO.update (torchrl/algo/on_policy/ppo.py:41-152)
// for one minibatch.  One launch covers both networks: workgroups [0, n_wg/2)
// run the policy, [n_wg/2, n_wg) the value function; a workgroup is 4 waves
// (one per SIMD), each wave walks 32-sample tiles with a grid stride.  Per tile
// and network (D=17, H=64):
//     forward  L1 18 + L2 64 MFMA,   dH1 64,   dW2 64,   dW1 32   (v_mfma_f32_32x32x2_f32)
// = 242 MFMA * 64 cycles; heads, losses, tanh and the tile transposes run on
// the VALU / LDS next to them.  Inputs are read straight from the time-major
// rollout tensors through the minibatch's row index (the gather of
// on_policy.py:84-88 is fused away): 104 B per sample (obs 68, act 24, adv 4,
// ret 4, V_old 4) + 4 B cached old log-prob.  Weight gradients accumulate in
// MFMA accumulators across all tiles of a wave, are folded across the 4 waves
// in a fixed order (deterministic) and written as one partial per workgroup.
//
// log pi_old is read from the rollout (`old_logp`, written by the collector
// kernel with the epoch-start parameters) instead of re-running target_pf on
// every minibatch (ppo.py:54-56) -- identical values, SURVEY.md section 8(d).
#include <cstdlib>
#include "trl_common.h"
#include "trl_mlp.h"
#include "trl_head.h"
#include "trl_comm.h"
#include "trl_ppo_wave.h"
#include "trl_ppo_wide.h"

// ---------------------------------------------------------------- partial reduce
// grads[p] = sum_w partial[w][p] in fixed order; info[] from the scalar partials:
//  0 policy surrogate sum (-min(s1,s2))   1 sum logp   2 sum logp^2   3 max logp   4 -min logp
//  5 max ratio   6 -min ratio   7 value-loss sum
#define RED_CHUNK 64
// waves per block of 64 parameters / partial rows a lane has in flight per round.  Measured on MI355X at 147 + 109 rows
// (rocprofv3 mean of the fused launch, round 3, after its argument struct stopped going through scratch memory):
// 4 x 16 -> 7.9 us, 8 x 16 -> 7.4 us, 8 x 32 -> 7.8 us, 16 x 16 -> 7.8 us (profiles/r03_grad_kernel_experiments.txt); the
// launch is bound by its rendezvous and launch latencies: without any partial-row load it still takes ~6 us.
#ifndef RED_WAVES
#define RED_WAVES 8
#endif
#ifndef RED_DEPTH
#define RED_DEPTH 16
#endif
// ---- pieces of the fold (8 waves per 64 parameters): the association order is part of the contract -- every launch
// that folds gives the same bits.  Rows of one network's partials are dealt to 8 "fold waves" (row r -> wave r % 8), each
// with RED_DEPTH independent chains (chain k takes rows w + 8 k + 128 round, in round order), chains folded pairwise (k with
// k + 8, 4, 2, 1), fold waves as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)).
__device__ __forceinline__ float fold_chain_tree(float (&acc)[RED_DEPTH]) {
#pragma unroll
  for (int st = RED_DEPTH / 2; st > 0; st >>= 1)
#pragma unroll
    for (int k = 0; k < st; ++k) acc[k] += acc[k + st];
  return acc[0];
}
// one fold wave: src = first row of the network + this lane's parameter
__device__ __forceinline__ float fold_rows_wave(const float* __restrict__ src, int nrow, int p_stride, int w, bool in_range) {
  // 16 independent loads in flight per lane and round: the fold is latency-, not bandwidth-bound
  float acc[RED_DEPTH];
#pragma unroll
  for (int k = 0; k < RED_DEPTH; ++k) acc[k] = 0.0f;
  if (in_range) {
    for (; w < nrow; w += RED_DEPTH * RED_WAVES) { // predicated: a ragged row count must not fall back to a serial tail
      float v[RED_DEPTH];
#pragma unroll
      for (int k = 0; k < RED_DEPTH; ++k) v[k] = (w + RED_WAVES * k < nrow) ? src[(size_t)(w + RED_WAVES * k) * p_stride] : 0.0f;
#pragma unroll
      for (int k = 0; k < RED_DEPTH; ++k) acc[k] += v[k];
    }
  }
  return fold_chain_tree(acc);
}
__device__ __forceinline__ float fold_waves_tree(const float (*s_acc)[RED_CHUNK], int lane) {
  float t4[RED_WAVES / 4];
#pragma unroll
  for (int q = 0; q < RED_WAVES / 4; ++q)
    t4[q] = (s_acc[4 * q][lane] + s_acc[4 * q + 1][lane]) + (s_acc[4 * q + 2][lane] + s_acc[4 * q + 3][lane]);
  float gval = t4[0];
#pragma unroll
  for (int q = 1; q < RED_WAVES / 4; ++q) gval += t4[q];
  return gval;
}
// one wave: a network's loss / log-prob / value statistics from the workgroups' scalar rows, every row requested at once
// (3 x 7 loads in flight per lane; the per-lane accumulation order is the one of the strided loop)
__device__ __noinline__ void fold_scalar_stats(const double* __restrict__ base, int nrow, int net, int lane,
                                                  double* __restrict__ info) {
  double v[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) v[k] = (k >= 2 && k <= 5) ? -INFINITY : 0.0;
  // (three rows per lane and round: up to 192 workgroups per network in ONE round trip with 42 doubles in flight -- the
  // function is out of line and the launches that call it are bounded to 128 registers, see ppo_reduce_adam_kernel; a lane
  // still adds its rows lane, lane + 64, lane + 128, ... in that order)
  for (int w0 = 0; w0 < nrow; w0 += 192) {
    double o[3][7];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int w = w0 + lane + 64 * q;
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        double x = (k >= 2 && k <= 5) ? -INFINITY : 0.0;
        if (w < nrow) x = base[(size_t)w * 8 + k];
        o[q][k] = x;
      }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int k = 0; k < 7; ++k) v[k] = (k >= 2 && k <= 5) ? fmax(v[k], o[q][k]) : v[k] + o[q][k];
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) v[k] = (k >= 2 && k <= 5) ? wave_max(v[k]) : wave_sum(v[k]);
  if (lane == 0) {
    if (net == 0) {
      info[0] = v[6]; info[1] = v[0]; info[2] = v[1]; info[3] = v[2]; info[4] = v[3]; info[5] = v[4]; info[6] = v[5];
    } else {
      info[7] = v[6];
      info[12] = v[0]; info[13] = v[1]; info[14] = v[2]; info[15] = v[3];   // v_pred: sum, sum of squares, max, -min
    }
  }
}
// one wave: log_std/{mean,std,max,min} (ppo.py:82-85) and the same four for std = exp(clamped logstd) (a2c.py:95-100),
// one action dimension per lane (raw = the lane's log_std as stored, lanes >= n_act: anything)
// (not inlined, like fold_scalar_stats: double-precision exp() and 14 doubles in flight would otherwise set the register
// count of every launch that CAN reach them -- ppo_reduce_adam_kernel went from 85 to 156 registers that way, see there)
__device__ __noinline__ void fold_logstd_stats_raw(float raw, int n_act, int lane, double* __restrict__ info) {
  const bool has = lane < n_act;
  const double x = has ? fmin(fmax((double)raw, -20.0), 2.0) : 0.0;
  const double e = has ? exp(x) : 0.0;
  const double sm = wave_sum(x), sq = wave_sum(x * x), es = wave_sum(e), eq = wave_sum(e * e);
  const double mx = wave_max(has ? x : -INFINITY), mn = -wave_max(has ? -x : -INFINITY);
  const double emx = wave_max(has ? e : -INFINITY), emn = -wave_max(has ? -e : -INFINITY);
  if (lane == 0) {
    const double mean = sm / n_act, em = es / n_act;
    info[8] = mean;
    info[9] = n_act > 1 ? sqrt(fmax((sq - sm * mean) / (n_act - 1), 0.0)) : NAN;
    info[10] = mx; info[11] = mn;
    info[16] = em;
    info[17] = n_act > 1 ? sqrt(fmax((eq - es * em) / (n_act - 1), 0.0)) : NAN;
    info[18] = emx; info[19] = emn;
  }
}
__device__ __forceinline__ void fold_logstd_stats(const float* __restrict__ logstd, int n_act, int lane, double* __restrict__ info) {
  fold_logstd_stats_raw(logstd[lane < n_act ? lane : 0], n_act, lane, info);
}

// one wave, categorical head: the entropy sum of the local samples (eighth column of the policy's scalar rows, a lane adds
// its rows lane, lane + 64, ... in that order) into info[20]; the log_std / std slots are written as zero --
// trl_cat_losses_f32's convention (trl_ppo_loss.h)
__device__ __noinline__ void fold_entropy_stats(const double* __restrict__ base, int nrow, int lane, double* __restrict__ info) {
  double v = 0.0;
  for (int w = lane; w < nrow; w += 64) v += base[(size_t)w * 8 + 7];
  v = wave_sum(v);
  if (lane == 0) {
    info[20] = v;
#pragma unroll
    for (int k = 0; k < 4; ++k) info[8 + k] = info[16 + k] = 0.0;
  }
}

// one wave, state-dependent-std head: the entropy sum (eighth column of the policy's scalar rows) into info[20], and
// log_std/{mean,std,max,min}, std/{...} over all samples x n_act elements from the second block of scalar rows (`sd`: SD_SCAL
// doubles per workgroup, see there) into info[8..11] / info[16..19] -- the row trl_gauss_sd_losses_f32 writes.  A lane adds
// its rows lane, lane + 64, ... in that order.  (out of line, like the others: see ppo_reduce_adam_kernel's register bound)
__device__ __noinline__ void fold_sd_stats(const double* __restrict__ base, const double* __restrict__ sd, int nrow, int n_act,
                                           int lane, double* __restrict__ info) {
  double v[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) v[k] = (k < 8 && (k & 2)) ? -INFINITY : 0.0;
  for (int w = lane; w < nrow; w += 64) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const double o = sd[(size_t)w * SD_SCAL + k];
      v[k] = (k < 8 && (k & 2)) ? fmax(v[k], o) : v[k] + o;
    }
    v[9] += base[(size_t)w * 8 + 7];
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) v[k] = (k < 8 && (k & 2)) ? wave_max(v[k]) : wave_sum(v[k]);
  if (lane == 0) {
    const double n = v[8] * (double)n_act, lm = v[0] / n, em = v[4] / n;
    info[8] = lm; info[9] = n > 1.0 ? sqrt(fmax((v[1] - v[0] * lm) / (n - 1.0), 0.0)) : NAN;
    info[10] = v[2]; info[11] = -v[3];
    info[16] = em; info[17] = n > 1.0 ? sqrt(fmax((v[5] - v[4] * em) / (n - 1.0), 0.0)) : NAN;
    info[18] = v[6]; info[19] = -v[7];
    info[20] = v[9];
  }
}

// returns (wave 0 lanes) the reduced gradient value of chunk `bx` (64 parameters) of network `net`, 0 outside the parameter
// range; `stats`: this call also takes the network's scalar statistics (waves 2 / 3)
// CAT: the policy block has no logstd tail (logstd is null) and wave 3 folds the entropy column instead
// SD: no logstd tail either; wave 3 folds the entropy column and the second block of scalar rows (behind the n_wg x 8)
template <int HEAD = HEAD_GAUSS>
__device__ __forceinline__ float ppo_reduce_block(const float* __restrict__ partial,
                                                  const double* __restrict__ scal, int n_wg, int n_pf,
                                                  int p_stride, int p_pf, int p_vf,
                                                  const float* __restrict__ logstd, int n_act,
                                                  float* __restrict__ grads, double* __restrict__ info,
                                                  int net, int bx, bool stats) {
  // block = 64 consecutive parameters x RED_WAVES waves; wave w folds partials w, w + RED_WAVES, ... with RED_DEPTH
  // independent accumulators (fixed order => deterministic), then the waves fold through LDS.
  __shared__ float s_acc[RED_WAVES][RED_CHUNK];
  const int row0 = net == 0 ? 0 : n_pf, nrow = net == 0 ? n_pf : n_wg - n_pf;   // this network's partial rows
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = bx * RED_CHUNK + lane;
  const int pn = net == 0 ? p_pf : p_vf;
  s_acc[wave][lane] = fold_rows_wave(partial + (size_t)row0 * p_stride + p, nrow, p_stride, wave, p < pn);
  __syncthreads();
  float gval = 0.0f;
  if (wave == 0 && p < pn) {
    gval = fold_waves_tree(s_acc, lane);
    grads[(net == 0 ? 0 : p_pf) + p] = gval;
  }
  // Scalar statistics.  They used to sit in block (0, 0) -- three dependent rounds of loads over the workgroup partials and
  // then the log_std / std statistics as a serial double-precision loop (six exp() in ONE lane): ~5 us that the whole
  // launch waited for, twice the time of the fold itself.  Now the LAST chunk of each network's row takes them, off the
  // path of the blocks whose 64 parameters matter: wave 2 its network's statistics, wave 3 of the policy's block log_std
  // and std.
  if (stats && wave == 2) fold_scalar_stats(scal + (size_t)row0 * 8, nrow, net, lane, info);
  if constexpr (HEAD == HEAD_SD) {
    if (stats && net == 0 && wave == 3)
      fold_sd_stats(scal + (size_t)row0 * 8, scal + (size_t)n_wg * 8 + (size_t)row0 * SD_SCAL, nrow, n_act, lane, info);
  } else if constexpr (HEAD == HEAD_CAT) {
    if (stats && net == 0 && wave == 3) fold_entropy_stats(scal + (size_t)row0 * 8, nrow, lane, info);
  } else {
    if (stats && net == 0 && wave == 3 && logstd) fold_logstd_stats(logstd, n_act, lane, info);
  }
  return gval;
}

template <int HEAD = HEAD_GAUSS>
__global__ __launch_bounds__(64 * RED_WAVES) void ppo_reduce_kernel(const float* __restrict__ partial,
                                                         const double* __restrict__ scal, int n_wg, int n_pf,
                                                         int p_stride, int p_pf, int p_vf,
                                                         const float* __restrict__ logstd, int n_act,
                                                         float* __restrict__ grads, double* __restrict__ info) {
  ppo_reduce_block<HEAD>(partial, scal, n_wg, n_pf, p_stride, p_pf, p_vf, logstd, n_act, grads, info, blockIdx.y, blockIdx.x,
                        blockIdx.x == gridDim.x - 1);
}

// ---------------------------------------------------------------- K11 clip + Adam
// Every block recomputes the (tiny) group norms itself, so one launch does
// clip_grad_norm_ (coef = max_norm / (norm + 1e-6), clamped to 1) and Adam.
struct AdamDev {
  float* params; const float* grads; float* m; float* v;
  int n_groups; int off[5]; float lr[4];
  float max_norm, beta1, beta2, eps, grad_scale, bc1, bc2_sqrt;
  float* norms_out;
  double* step_state;         // {steps taken, beta1^steps, beta2^steps, -} or null (then bc1 / bc2_sqrt)
  const float* device_lr;     // per-group learning rates on the device, or null (then lr[])
  int self_tick;              // small grids: the last block to have read step_state advances it (no tick launch)
};
__global__ __launch_bounds__(256) void clip_adam_kernel(AdamDev a) {
  __shared__ float s_part[4][4];
  __shared__ float s_coef[4];
  __shared__ float s_bc[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (a.step_state && tid == 0) {                              // device-resident step: nothing in the launch changes
    s_bc[0] = (float)(1.0 - a.step_state[1] * (double)a.beta1);   // between replays of a captured graph
    s_bc[1] = (float)sqrt(1.0 - a.step_state[2] * (double)a.beta2);
    if (a.self_tick) {
      // Every block counts itself in AFTER its reads (release); the block that completes the count has therefore
      // seen all reads done (acquire) and advances the state for the next launch.  The counter lives in the reserved
      // 4th double and is back at zero when the kernel ends.
      unsigned* cnt = reinterpret_cast<unsigned*>(a.step_state + 3);
      const unsigned before = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      if (before == gridDim.x - 1) {
        a.step_state[0] += 1.0; a.step_state[1] *= (double)a.beta1; a.step_state[2] *= (double)a.beta2;
        __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  const bool need_norm = a.max_norm > 0.0f;                    // no clipping requested: skip the norm pass
  for (int g = 0; g < a.n_groups; ++g) {
    if (!need_norm) { if (lane == 0) s_part[g][wave] = 0.0f; continue; }
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int e = a.off[g] + tid;
    for (; e + 7 * 256 < a.off[g + 1]; e += 8 * 256) {         // 8 loads in flight per lane and round
      float x[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) x[k] = a.grads[e + 256 * k];
      s0 = fmaf(x[0], x[0], s0); s1 = fmaf(x[1], x[1], s1); s2 = fmaf(x[2], x[2], s2); s3 = fmaf(x[3], x[3], s3);
      s0 = fmaf(x[4], x[4], s0); s1 = fmaf(x[5], x[5], s1); s2 = fmaf(x[6], x[6], s2); s3 = fmaf(x[7], x[7], s3);
    }
    for (; e < a.off[g + 1]; e += 256) { const float x = a.grads[e]; s0 = fmaf(x, x, s0); }
    float ss = wave_sum((s0 + s1) + (s2 + s3)) * a.grad_scale * a.grad_scale;
    if (lane == 0) s_part[g][wave] = ss;
  }
  __syncthreads();
  if (tid < a.n_groups) {
    const float norm = sqrtf(s_part[tid][0] + s_part[tid][1] + s_part[tid][2] + s_part[tid][3]);
    s_coef[tid] = (a.max_norm > 0.0f) ? fminf(a.max_norm / (norm + 1e-6f), 1.0f) : 1.0f;
    if (blockIdx.x == 0 && a.norms_out) a.norms_out[tid] = norm;
  }
  __syncthreads();
  const float bc1 = a.step_state ? s_bc[0] : a.bc1, bc2_sqrt = a.step_state ? s_bc[1] : a.bc2_sqrt;
  const int e = blockIdx.x * 256 + tid;
  if (e < a.off[a.n_groups]) {
    int g = 0;
    while (e >= a.off[g + 1]) ++g;
    const float gr = a.grads[e] * a.grad_scale * s_coef[g];
    const float m = a.beta1 * a.m[e] + (1.0f - a.beta1) * gr;
    const float v = a.beta2 * a.v[e] + (1.0f - a.beta2) * gr * gr;
    a.m[e] = m; a.v[e] = v;
    const float denom = sqrtf(v) / bc2_sqrt + a.eps;
    const float lr = a.device_lr ? a.device_lr[g] : a.lr[g];
    a.params[e] -= (lr / bc1) * (m / denom);
  }
}

// advances the device-resident step state after clip_adam_kernel has read it (stream order: every block is done)
__global__ void adam_tick_kernel(double* __restrict__ st, float beta1, float beta2) {
  st[0] += 1.0; st[1] *= (double)beta1; st[2] *= (double)beta2;
}

// Adam update of element e with the clip coefficient of its group
__device__ __forceinline__ void adam_element(const AdamDev& a, int e, float gr) {
  const float m = a.beta1 * a.m[e] + (1.0f - a.beta1) * gr;
  const float v = a.beta2 * a.v[e] + (1.0f - a.beta2) * gr * gr;
  a.m[e] = m; a.v[e] = v;
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  int g = 0;
  while (e >= a.off[g + 1]) ++g;
  a.params[e] -= (a.lr[g] / a.bc1) * (m / denom);
}

// Single-GPU path: partial reduce + clip_grad_norm_ + Adam in ONE launch.  The 2 x nb jobs (job j = the 64 parameters
// `j % nb` of network `j / nb`) are dealt to the blocks of a 1-D grid (block b: jobs b, b + grid, ...; the default grid is
// one block per job).  A block folds its jobs' parameters and publishes each one's sum of squares as ONE 64-bit
// agent-scope store {ss, epoch}; every block then polls the 2 x nb slots until all carry the epoch of this launch (the
// blocks are always co-resident: at most 180 small blocks on 256 CUs), derives the two group norms from them in the same
// fixed order (deterministic, identical in all blocks) and takes the Adam step for its own parameters -- straight from
// registers when it has one job.  No ticket, no reset: a slot is valid iff its epoch matches (epoch = Adam step count > 0;
// the workspace starts zeroed).  The poll is capped: a scheduling accident trips ws[0] instead of hanging.
// The GRID is the launch's resident footprint while it waits (for other ranks' gradients, with env shards on several
// ranks): blocks x 8 waves that stay on the device until every rank has delivered.  One rank per GPU: irrelevant.  Ranks
// sharing a device (tests): it must leave room for the other ranks' gradient kernels (trl_comm_set_wait_footprint).
// (at most 128 registers per wave: a block is 2 waves per SIMD, and two ranks sharing a device need TWO waiting launches'
// blocks -- 4 waves per SIMD -- resident beside each other.  With the statistics inlined into the job loop the kernel took
// 156 registers: the second rank's blocks found no room next to the first's, its norm rendezvous could not complete, and
// both ranks sat out their time-outs -- round 6, caught by tests/test_bench_multirank_gpu.py)
template <bool LOOP, int HEAD = HEAD_GAUSS>   // LOOP false: the grid has one block per job (no job loop: the common launch)
__global__ __launch_bounds__(64 * RED_WAVES, 4) void ppo_reduce_adam_kernel(const float* __restrict__ partial,
                                                              const double* __restrict__ scal, int n_wg, int n_pf,
                                                              int p_stride, int p_pf, int p_vf,
                                                              const float* __restrict__ logstd, int n_act,
                                                              float* __restrict__ grads, double* __restrict__ info,
                                                              AdamDev a, float* __restrict__ ws, unsigned epoch,
                                                              int device_state, int xrank, XrArgs xr, int only_net) {
  __shared__ float s_coef[2];
  __shared__ float s_hyper[4];                                    // bc1, bc2_sqrt, lr_pf, lr_vf
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // only_net >= 0: the rows are ONE network's (a single-network gradient launch); its nb jobs only, its norm, its group
  const int nb = (p_stride + RED_CHUNK - 1) / RED_CHUNK, grid = gridDim.x, job0 = only_net == 1 ? nb : 0;
  const int n_jobs = only_net >= 0 ? job0 + nb : 2 * nb, blk = job0 + (int)blockIdx.x;
  // Graph-replayable form: the Adam step count and the learning rates live in the workspace header
  // (ws[1] = steps taken so far as uint32, ws[2..3] = lr), so no launch argument changes between replays.
  // Every block reads the count BEFORE it publishes its slots; block 0 bumps it only after it has seen
  // all slots, i.e. after every block has read it.
  // (the count was written by the previous launch, so a plain uniform load -- a scalar load that flies under the
  // reduction's vector loads -- is enough; the bias corrections are computed by an otherwise idle wave)
  double* bpow = reinterpret_cast<double*>(ws + 4);              // beta1^steps, beta2^steps of the steps taken so far
  double b1p = 0.0, b2p = 0.0;
  float lr0 = 0.0f, lr1 = 0.0f;
  if (device_state) {
    epoch = reinterpret_cast<const unsigned*>(ws)[1] + 1u;
    if (tid == 64 * (RED_WAVES - 1)) { b1p = bpow[0]; b2p = bpow[1]; lr0 = ws[2]; lr1 = ws[3]; }   // issued now, used after the fold
  }
  unsigned long long* slots = reinterpret_cast<unsigned long long*>(ws + 16);    // [2 nets][nb] {ss bits, epoch}
  // env shards on several ranks: the epoch of the cross-rank exchange is the communicator's own count of completed
  // gradient exchanges (read by every block before it publishes anything, advanced by block 0 at the end)
  // (two counts, ctl[4] and ctl[6]: a single-network launch of the value function -- the second of two concurrent update
  // chains -- counts its exchanges in ctl[6] and touches only the value function's granules, one of the policy in ctl[4];
  // a joint launch, which touches all granules, takes the larger of the two and leaves both at its epoch: a granule's stamps
  // only ever grow, whichever route wrote them last)
  unsigned xepoch = 0u;
  if (xrank) {
    const unsigned e4 = __hip_atomic_load(xr.ctl + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned e6 = __hip_atomic_load(xr.ctl + 6, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    xepoch = (only_net == 0 ? e4 : only_net == 1 ? e6 : (e4 > e6 ? e4 : e6)) + 1u;
  }
  float gval0 = 0.0f;                                             // wave 0: the (summed) gradient of this block's FIRST job
  for (int j = blk; j < (LOOP ? n_jobs : blk + 1); j += LOOP ? grid : 1) {
    const int net = j / nb, bx = j - net * nb;
    if (j != blk) __syncthreads();                                // the fold's LDS image is read by wave 0 of the previous job
    float gval = ppo_reduce_block<HEAD>(partial, scal, n_wg, n_pf, p_stride, p_pf, p_vf, logstd, n_act, grads, info, net, bx, bx == nb - 1);
    if (wave == 0) {
      if (xrank) {
        // C1 of SURVEY.md 8(e) inside the launch: every rank pushes its 64 folded values into its slot on all ranks and
        // sums the slots in rank order (trl_comm.h) -- the gradient every rank clips and steps with is the same, bit for bit
        const int pe = bx * RED_CHUNK + lane;
        const bool act = pe < (net == 0 ? p_pf : p_vf);
        const int ge = (net == 0 ? 0 : p_pf) + pe;
        gval = xr_allsum_f32(xr, xepoch, act ? ge : 0, gval, act);
        if (act) grads[ge] = gval;
      }
      if (j == blk) gval0 = gval;
      const float ss = wave_sum(gval * gval);
      if (lane == 0)
        __hip_atomic_store(slots + net * nb + bx, ((unsigned long long)epoch << 32) | (unsigned long long)__float_as_uint(ss),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (device_state && tid == 64 * (RED_WAVES - 1)) {
    b1p *= (double)a.beta1; b2p *= (double)a.beta2;
    s_hyper[0] = (float)(1.0 - b1p);
    s_hyper[1] = (float)sqrt(1.0 - b2p);
    s_hyper[2] = lr0; s_hyper[3] = lr1;
  }
  if (LOOP && blk >= n_jobs) return;                              // (a grid larger than the job list)
  // the optimiser state of this block's first job is requested now and arrives while the norm slots are polled
  const int net_ = blk / nb, pe_ = (blk - net_ * nb) * RED_CHUNK + lane;
  const bool own_ = wave == 0 && pe_ < (net_ == 0 ? p_pf : p_vf);
  const int ge_ = (net_ == 0 ? 0 : p_pf) + pe_;
  float m_old = 0.0f, v_old = 0.0f, p_old = 0.0f;
  if (own_) { m_old = a.m[ge_]; v_old = a.v[ge_]; p_old = a.params[ge_]; }
  // ---- group norms (pf, vf): wave w polls net w's slots, then sums them in fixed order ----
  if (wave < 2 && (only_net < 0 || wave == only_net)) {
    float acc = 0.0f;
    for (int b = lane; b < nb; b += 64) {
      unsigned long long v;
      unsigned it = 0;
      unsigned long long t0 = 0;
      while ((unsigned)((v = __hip_atomic_load(slots + wave * nb + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) != epoch) {
        __builtin_amdgcn_s_sleep(1);
        if ((++it & 1023u) == 0) {                                // bounded by wall-clock time (100 MHz counter): ~2 s alone,
          const unsigned long long now = wall_clock64();          // ~25 s when other ranks' gradients are being waited for
          if (t0 == 0) t0 = now;
          if (now - t0 > (xrank ? xr.wait_ticks + xr.wait_ticks / 4 : 200000000ull)) {
            __hip_atomic_store(reinterpret_cast<unsigned*>(ws), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
          }
        }
      }
      acc += __uint_as_float((unsigned)v);
    }
    acc = wave_sum(acc) * a.grad_scale * a.grad_scale;
    if (lane == 0) {
      const float norm = sqrtf(acc);
      s_coef[wave] = (a.max_norm > 0.0f) ? fminf(a.max_norm / (norm + 1e-6f), 1.0f) : 1.0f;
      if (a.norms_out && blk == job0) a.norms_out[wave] = norm;
    }
  }
  __syncthreads();
  // (locals, not fields of `a`: writing into the by-value argument struct moves it to scratch memory and turns every access
  // through its pointers into a flat instruction)
  float bc1 = a.bc1, bc2_sqrt = a.bc2_sqrt, lr_pf = a.lr[0], lr_vf = a.lr[1];
  if (device_state) {
    bc1 = s_hyper[0]; bc2_sqrt = s_hyper[1]; lr_pf = s_hyper[2]; lr_vf = s_hyper[3];
    if (blk == job0) {                                           // every block has read the header by now (see above)
      if (tid == 0) __hip_atomic_store(reinterpret_cast<unsigned*>(ws) + 1, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (tid == 64 * (RED_WAVES - 1)) { bpow[0] = b1p; bpow[1] = b2p; }
    }
  }
  // (every block has passed its exchanges by the time block 0 has seen all norm slots)
  if (xrank && blk == job0 && tid == 0) {
    if (only_net != 1) __hip_atomic_store(xr.ctl + 4, xepoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (only_net != 0) __hip_atomic_store(xr.ctl + 6, xepoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // A cross-rank wait that timed out left a PARTIAL gradient sum: no parameter is written then (every block has finished
  // its exchanges before any block sees all norm slots, so the flag is final here and all blocks decide alike); the host
  // raises through trl_comm_error at its next check.
  const bool xfail = xrank && __hip_atomic_load(xr.ctl + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
  if (wave == 0 && !xfail) {                                       // adam_element, the first job on the prefetched state
    for (int j = blk; j < (LOOP ? n_jobs : blk + 1); j += LOOP ? grid : 1) {
      const int net = j / nb, pe = (j - net * nb) * RED_CHUNK + lane;
      if (pe >= (net == 0 ? p_pf : p_vf)) continue;
      const int ge = (net == 0 ? 0 : p_pf) + pe;
      const bool first = j == blk;
      const float g_ = first ? gval0 : grads[ge];                  // (later jobs: this lane's own store of the fold above)
      const float mo = first ? m_old : a.m[ge], vo = first ? v_old : a.v[ge], po = first ? p_old : a.params[ge];
      const float gr = g_ * a.grad_scale * s_coef[net];
      const float m = a.beta1 * mo + (1.0f - a.beta1) * gr;
      const float v = a.beta2 * vo + (1.0f - a.beta2) * gr * gr;
      a.m[ge] = m; a.v[ge] = v;
      const float denom = sqrtf(v) / bc2_sqrt + a.eps;
      a.params[ge] = po - ((net == 0 ? lr_pf : lr_vf) / bc1) * (m / denom);
    }
  }
}

// ---------------------------------------------------------------- MLP inference
template <int D, int H, int O, int ACT>
__global__ __launch_bounds__(256) void mlp2_forward_kernel(const float* __restrict__ params,
                                                           const float* __restrict__ x,
                                                           float* __restrict__ out, int M) {
  using L = MlpLds<D, H, O>;
  constexpr int NT = H / 32, KS = ksteps_for(D);
  __shared__ __attribute__((aligned(16))) float sp[L::SIZE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, hi = lane >> 5;
  L::load(sp, params, false, tid, 256);
  __syncthreads();
  const int n_tiles = (M + 31) / 32;
  for (int tile = blockIdx.x * 4 + wave; tile < n_tiles; tile += gridDim.x * 4) {
    const int s = tile * 32 + i;
    float xb[KS];
#pragma unroll
    for (int q = 0; q < KS; ++q) { const int k = rowmap(q, hi); xb[q] = (k < D && s < M) ? x[(size_t)s * D + k] : 0.0f; }
    f32x16 h1[NT], h2[NT];
#pragma unroll
    for (int mo = 0; mo < NT; ++mo)
      h1[mo] = act_tile<ACT>(layer1_tile<D, L::LD1, KS>(bias_tile(sp + L::B1 + 32 * mo, hi), sp + L::W1, mo, xb, i, hi));
#pragma unroll
    for (int mo = 0; mo < NT; ++mo)
      h2[mo] = act_tile<ACT>(layer_tile<NT, L::LD2>(bias_tile(sp + L::B2 + 32 * mo, hi), sp + L::W2, mo, h1, i, hi));
    float o[O];
    head_fwd<NT, H, O>(sp + L::W3, sp + L::B3, h2, hi, o);
    if (hi == 0 && s < M) {
#pragma unroll
      for (int c = 0; c < O; ++c) out[(size_t)s * O + c] = o[c];
    }
  }
}

// ================================================================ host side
#define SHAPE_IS(d, h, o) (D == (d) && H == (h) && A == (o))

// Shapes the fused minibatch kernels carry: the benchmark shape as a compile-time instantiation (Gaussian head only), and
// any D in [2, 32] at H = 64 with the head's range of A (HEADS, trl_head.h) through the runtime-dims instantiations
// (ppo_wave_pass<..., RT = true, HEAD>: the 17- and the 32-wide tile).  The flat policy block is [W1 b1 W2 b2 W3 b3] with
// the head's rows, and the Gaussian's logstd tail: up to 1040 head floats (SD, 2A rows) against the Gaussian's 528.
// ln_mask (trl_ppo_ln_*): bit 0 the policy, bit 1 the critic carries a LayerNorm -- 128 more floats in that net's block
// ln_mask == PPO_WIDE_MASK (trl_ppo_wide_*): a plain pair of width 128, the rows of k_ppo_wide.hip
static int ppo_stride_for(int D, int H, int A, int head, int ln_mask = 0) {
  if (ln_mask == PPO_WIDE_MASK) {
    if (ppo_wide_ok(head, D, H, A, TRL_ACT_TANH)) return ppo_ln_stride(D, H, A, head, 0);
    trl_set_error("trl_ppo_wide: head %d, shape D=%d H=%d A=%d outside what the wide instantiations carry (H == 128, 2 <= D <= 32, "
                  "A in the head's range)", head, D, H, A);
    return TRL_EUNSUPPORTED;
  }
  if (head == HEAD_GAUSS && SHAPE_IS(17, 64, 6) && !ln_mask) return PpoShape<17, 64, 6>::P_STRIDE;
  if (head_shape_ok(head, D, H, A)) return ppo_ln_stride(D, H, A, head, ln_mask);
  trl_set_error("trl_ppo_%spartial_stride: shape D=%d H=%d A=%d not instantiated (H == 64, 2 <= D <= 32, %d <= A <= %d)",
                HEADS[head].tag, D, H, A, HEADS[head].a_min, HEADS[head].a_max);
  return TRL_EUNSUPPORTED;
}
extern "C" int trl_ppo_partial_stride(int D, int H, int A) { return ppo_stride_for(D, H, A, HEAD_GAUSS); }
extern "C" int trl_ppo_cat_partial_stride(int D, int H, int A) { return ppo_stride_for(D, H, A, HEAD_CAT); }
extern "C" int trl_ppo_sd_partial_stride(int D, int H, int A) { return ppo_stride_for(D, H, A, HEAD_SD); }
extern "C" int trl_ppo_cat_supported(int D, int H, int A, int act) { return head_supported(HEAD_CAT, D, H, A, act); }
extern "C" int trl_ppo_sd_supported(int D, int H, int A, int act) { return head_supported(HEAD_SD, D, H, A, act); }
// doubles of scal_partial per workgroup: the n_wg x 8 block of every head, then n_wg x SD_SCAL (see SD_SCAL)
extern "C" int trl_ppo_sd_scalar_stride(void) { return HEADS[HEAD_SD].scal_stride; }
static_assert(WvShapeSD<17, 64, 8>::P_STRIDE == 6400 && WvShapeSD<32, 64, 8>::P_STRIDE == 7360, "SD image strides at A = 8");
static_assert(WvShapeSD<32, 64, 8>::LDS_FLOATS * sizeof(float) <= 160 * 1024, "the wide tile's exchange area fits the LDS");


// Policy / value split of the grid.  A policy tile costs more than a value tile (head, log-prob loss,
// dW3 on the matrix pipe: 16.7 k vs 12.1 k cycles measured at D=17, H=64, A=6), and every wave runs whole
// tiles, so the split that minimises the slower side's ceil(tiles / waves) * cost is searched directly.
extern "C" int trl_ppo_wg_split(int D, int H, int A, int n_tiles, int n_wg) {
  if (n_wg < 2 || n_tiles <= 0) { trl_set_error("trl_ppo_wg_split: need n_wg >= 2 and n_tiles > 0"); return TRL_EINVAL; }
  const double c_pf = 16.7, c_vf = 12.1;
  int best = n_wg / 2;
  double best_t = 1e300;
  for (int x = 1; x < n_wg; ++x) {
    const double t_pf = (double)((n_tiles + WV_WAVES * x - 1) / (WV_WAVES * x)) * c_pf;
    const double t_vf = (double)((n_tiles + WV_WAVES * (n_wg - x) - 1) / (WV_WAVES * (n_wg - x))) * c_vf;
    const double t = t_pf > t_vf ? t_pf : t_vf;
    if (t < best_t - 1e-9 || (t < best_t + 1e-9 && abs(2 * x - n_wg) < abs(2 * best - n_wg))) { best_t = t; best = x; }
  }
  (void)D; (void)H; (void)A;
  return best;
}

static int ppo_grad_launch(const trl_ppo_batch_t* p, void* stream, int head = HEAD_GAUSS) {
  if (!p) { trl_set_error("ppo_grad: null descriptor"); return TRL_EINVAL; }
  if (!head_supported(head, p->D, p->H, p->A, p->act)) {      // (the benchmark shape is inside the Gaussian's range)
    trl_set_error("ppo_%sgrad: shape D=%d H=%d A=%d act=%d not instantiated (H == 64, 2 <= D <= 32, %d <= A <= %d, Tanh / ReLU)",
                  HEADS[head].tag, p->D, p->H, p->A, p->act, HEADS[head].a_min, HEADS[head].a_max);
    return TRL_EUNSUPPORTED;
  }
  const int D = p->D, H = p->H, A = p->A;
  PpoDev d;
  const int rc = ppo_dev_fill(p, head, head == HEAD_GAUSS && SHAPE_IS(17, 64, 6), d);
  if (rc != TRL_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  d.p_stride = ppo_stride_for(D, H, A, head);
  if (head == HEAD_GAUSS && SHAPE_IS(17, 64, 6))      // the compile-time instantiation of the benchmark shape
    return p->act == TRL_ACT_TANH ? launch_ppo<17, 64, 6, TRL_ACT_TANH, false>(d, s) : launch_ppo<17, 64, 6, TRL_ACT_RELU, false>(d, s);
  // actual dims at run time inside the (17, 64, 8) tile, or with 18 .. 32 input features the (32, 64, 8) tile
  return with_head(head, [&](auto hd) {
    return with_tile_act(D, p->act, [&](auto tile, auto act) {
      return launch_ppo<decltype(tile)::value, 64, 8, decltype(act)::value, true, decltype(hd)::value>(d, s);
    });
  });
}

extern "C" int trl_ppo_minibatch_grad_f32(const trl_ppo_batch_t* p, void* stream) { return ppo_grad_launch(p, stream); }
// The same launch for a categorical policy (2 <= A <= 8 logits): acts is (rows, N, 1) -- the action index as a float --,
// pf_params is [W1 b1 W2 b2 W3 b3], tanh_action is ignored, partial rows are trl_ppo_cat_partial_stride floats and the
// policy workgroups' scalar rows carry the entropy sum in their eighth column (trl_ppo_cat_reduce_*_f32 fold it).
extern "C" int trl_ppo_cat_minibatch_grad_f32(const trl_ppo_batch_t* p, void* stream) { return ppo_grad_launch(p, stream, HEAD_CAT); }
// The same launch for a state-dependent-std Gaussian policy (1 <= A <= 8 action dimensions, a head of 2A rows
// [mean | log_std]): acts is (rows, N, A), pf_params is [W1 b1 W2 b2 W3 b3], partial rows are trl_ppo_sd_partial_stride
// floats and scal_partial holds n_wg x trl_ppo_sd_scalar_stride() doubles: the n_wg x 8 block (entropy sum in the policy
// rows' eighth column), then the policy workgroups' log_std / std statistics (trl_ppo_sd_reduce_*_f32 fold both).
extern "C" int trl_ppo_sd_minibatch_grad_f32(const trl_ppo_batch_t* p, void* stream) { return ppo_grad_launch(p, stream, HEAD_SD); }

// pf_params: the Gaussian's logstd tail is read from it (may be null: no log_std / std statistics); the other heads have
// none -- wave 3 folds the entropy column (and, SD, the second scalar block) instead
static int launch_reduce(const float* partial, const double* scal_partial, int n_wg, int n_wg_pf, int D, int H, int A,
                         const float* pf_params, float* grads, double* info, void* stream, int head, int ln_mask = 0) {
  TRL_REQUIRE(partial && scal_partial && grads && info, "null pointer");
  TRL_REQUIRE(n_wg >= 2 && n_wg_pf >= 0 && n_wg_pf < n_wg, "need n_wg >= 2 and n_wg_pf in [0, n_wg)");
  const int ps = ppo_stride_for(D, H, A, head, ln_mask);
  if (ps < 0) return ps;
  const int p_pf = ppo_ln_p_pf(D, H, A, head, ln_mask), p_vf = ppo_ln_p_vf(D, H, ln_mask);
  const float* logstd = (HEADS[head].logstd_tail && pf_params) ? pf_params + (p_pf - A) : nullptr;
  with_head(head, [&](auto hd) {
    hipLaunchKernelGGL(ppo_reduce_kernel<decltype(hd)::value>, dim3(trl_ceil_div(ps, RED_CHUNK), 2), dim3(64 * RED_WAVES), 0,
                       (hipStream_t)stream, partial, scal_partial, n_wg, resolve_pf_wgs(n_wg, n_wg_pf), ps, p_pf, p_vf,
                       logstd, A, grads, info);
    return 0;
  });
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}
extern "C" int trl_ppo_reduce_f32(const float* partial, const double* scal_partial, int n_wg, int n_wg_pf, int D,
                                  int H, int A, const float* pf_params, float* grads, double* info, void* stream) {
  return launch_reduce(partial, scal_partial, n_wg, n_wg_pf, D, H, A, pf_params, grads, info, stream, HEAD_GAUSS);
}
// categorical head: pf_params is accepted for symmetry and not read (there is no logstd); info[20] = entropy sum
extern "C" int trl_ppo_cat_reduce_f32(const float* partial, const double* scal_partial, int n_wg, int n_wg_pf, int D,
                                      int H, int A, const float* pf_params, float* grads, double* info, void* stream) {
  return launch_reduce(partial, scal_partial, n_wg, n_wg_pf, D, H, A, pf_params, grads, info, stream, HEAD_CAT);
}
// state-dependent-std head: pf_params is accepted for symmetry and not read; info[8..11] / info[16..19] = log_std / std
// statistics over all samples x A elements, info[20] = entropy sum (trl_gauss_sd_losses_f32's row)
extern "C" int trl_ppo_sd_reduce_f32(const float* partial, const double* scal_partial, int n_wg, int n_wg_pf, int D,
                                     int H, int A, const float* pf_params, float* grads, double* info, void* stream) {
  return launch_reduce(partial, scal_partial, n_wg, n_wg_pf, D, H, A, pf_params, grads, info, stream, HEAD_SD);
}

static int fill_adam(const trl_adam_t* p, AdamDev& d) {
  if (!p) { trl_set_error("clip_adam: null descriptor"); return TRL_EINVAL; }
  TRL_REQUIRE(p->params && p->grads && p->exp_avg && p->exp_avg_sq, "null pointer");
  TRL_REQUIRE(p->n_groups >= 1 && p->n_groups <= 4, "n_groups must be 1..4");
  TRL_REQUIRE(p->step_count >= 1 || p->device_state || p->step_state, "step_count starts at 1");
  d.params = p->params; d.grads = p->grads; d.m = p->exp_avg; d.v = p->exp_avg_sq;
  d.n_groups = p->n_groups; d.off[0] = 0;
  for (int g = 0; g < p->n_groups; ++g) {
    TRL_REQUIRE(p->group_sizes[g] >= 0, "negative group size");
    d.off[g + 1] = d.off[g] + p->group_sizes[g];
    d.lr[g] = p->group_lr[g];
  }
  for (int g = p->n_groups; g < 4; ++g) { d.off[g + 1] = d.off[g]; if (g < 4) d.lr[g] = 0.f; }
  d.max_norm = p->max_norm; d.beta1 = p->beta1; d.beta2 = p->beta2; d.eps = p->eps;
  d.grad_scale = p->grad_scale;
  d.bc1 = (float)(1.0 - pow((double)p->beta1, (double)p->step_count));
  d.bc2_sqrt = (float)sqrt(1.0 - pow((double)p->beta2, (double)p->step_count));
  d.norms_out = p->norms_out;
  d.step_state = p->step_state;
  d.device_lr = p->device_lr;
  d.self_tick = 0;
  return TRL_OK;
}

static int reduce_adam_workspace(int D, int H, int A, int head, int ln_mask = 0) {
  const int ps = ppo_stride_for(D, H, A, head, ln_mask);
  if (ps < 0) return ps;
  return 16 + 4 * trl_ceil_div(ps, RED_CHUNK);       // header + {ss, epoch} per block and network
}
extern "C" int trl_ppo_reduce_adam_workspace(int D, int H, int A) { return reduce_adam_workspace(D, H, A, HEAD_GAUSS); }
extern "C" int trl_ppo_cat_reduce_adam_workspace(int D, int H, int A) { return reduce_adam_workspace(D, H, A, HEAD_CAT); }
extern "C" int trl_ppo_sd_reduce_adam_workspace(int D, int H, int A) { return reduce_adam_workspace(D, H, A, HEAD_SD); }

static int launch_reduce_adam(const float* partial, const double* scal_partial, int n_wg, int n_wg_pf, int D, int H, int A,
                              float* grads, double* info, const trl_adam_t* adam, float* workspace, const XrArgs* xr,
                              int max_blocks, void* stream, int only_net = -1, int head = HEAD_GAUSS, int ln_mask = 0) {
  TRL_REQUIRE(partial && scal_partial && grads && info && workspace, "null pointer");
  TRL_REQUIRE(only_net >= 0 ? n_wg >= 1 : (n_wg >= 2 && n_wg_pf >= 0 && n_wg_pf < n_wg), "need n_wg >= 2 and n_wg_pf in [0, n_wg)");
  const int ps = ppo_stride_for(D, H, A, head, ln_mask);
  if (ps < 0) return ps;
  AdamDev d;
  int rc = fill_adam(adam, d);
  if (rc) return rc;
  const int p_pf = ppo_ln_p_pf(D, H, A, head, ln_mask), p_vf = ppo_ln_p_vf(D, H, ln_mask);
  // (a policy-only optimiser -- REINFORCE -- steps through the policy's `_net` fold with its single group)
  TRL_REQUIRE((adam->n_groups == 2 && adam->group_sizes[0] == p_pf && adam->group_sizes[1] == p_vf) ||
              (only_net == 0 && !xr && adam->n_groups == 1 && adam->group_sizes[0] == p_pf),
              "optimiser groups must be [policy | value] of this shape");
  TRL_REQUIRE(adam->grads == grads, "adam->grads must be the reduce output");
  TRL_REQUIRE(!xr || p_pf + p_vf <= TRL_XR_CAP_GRAD, "gradient exceeds the peer buffer");
  XrArgs none;
  none.rank = 0; none.world = 1; none.ctl = nullptr; none.wait_ticks = 0;
  for (int r = 0; r < TRL_MAX_RANKS; ++r) none.peer[r] = nullptr;
  int grid = (only_net >= 0 ? 1 : 2) * trl_ceil_div(ps, RED_CHUNK);   // one block per job, unless the caller bounds the footprint
  if (max_blocks > 0 && max_blocks < grid) grid = max_blocks;
  const int n_pf = only_net == 0 ? n_wg : (only_net == 1 ? 0 : resolve_pf_wgs(n_wg, n_wg_pf));
  const int jobs = (only_net >= 0 ? 1 : 2) * trl_ceil_div(ps, RED_CHUNK);
  // the Gaussian's logstd tail; the other heads have none: wave 3 folds the entropy column (SD: and the second scalar block)
  const float* logstd = HEADS[head].logstd_tail ? adam->params + (p_pf - A) : nullptr;
  const unsigned epoch = (unsigned)adam->step_count;
  with_head(head, [&](auto hd) {
    auto launch = [&](auto loop) {
      hipLaunchKernelGGL((ppo_reduce_adam_kernel<decltype(loop)::value, decltype(hd)::value>), dim3(grid), dim3(64 * RED_WAVES), 0,
                         (hipStream_t)stream, partial, scal_partial, n_wg, n_pf, ps, p_pf, p_vf, logstd, A, grads, info, d,
                         workspace, epoch, adam->device_state, xr ? 1 : 0, xr ? *xr : none, only_net);
    };
    if (grid == jobs) launch(std::false_type{}); else launch(std::true_type{});
    return 0;
  });
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

extern "C" int trl_ppo_reduce_adam_f32(const float* partial, const double* scal_partial, int n_wg, int n_wg_pf,
                                       int D, int H, int A, float* grads, double* info, const trl_adam_t* adam,
                                       float* workspace, void* stream) {
  return launch_reduce_adam(partial, scal_partial, n_wg, n_wg_pf, D, H, A, grads, info, adam, workspace, nullptr, 0, stream);
}

// ONE network's half of the step: `partial` / `scal_partial` hold the n_wg rows of a single-network gradient launch
// (trl_ppo_minibatch_grad_f32 with n_wg_pf = n_wg: net 0, the policy; n_wg_pf = -1: net 1, the value function); the fold,
// that group's clip and its Adam step.  PPO's critic and actor updates are independent (separate networks, optimisers
// and clips: ppo.py:93-122 / 41-91), so the two halves may run as separate launch sequences, concurrently, each with its
// own workspace (own Adam header: both count the same steps).  Same arithmetic and order as the joint launch: bit-identical.
extern "C" int trl_ppo_reduce_adam_net_f32(const float* partial, const double* scal_partial, int n_wg, int net,
                                           int D, int H, int A, float* grads, double* info, const trl_adam_t* adam,
                                           float* workspace, void* stream) {
  TRL_REQUIRE(net == 0 || net == 1, "net: 0 = policy, 1 = value function");
  return launch_reduce_adam(partial, scal_partial, n_wg, 0, D, H, A, grads, info, adam, workspace, nullptr, 0, stream, net);
}

// The categorical head's folds (rows of trl_ppo_cat_minibatch_grad_f32; same row fold order, norm rendezvous and Adam
// arithmetic; optimiser groups [policy without logstd | value]).  The cross-rank variants do not exist for this head.
extern "C" int trl_ppo_cat_reduce_adam_f32(const float* partial, const double* scal_partial, int n_wg, int n_wg_pf,
                                           int D, int H, int A, float* grads, double* info, const trl_adam_t* adam,
                                           float* workspace, void* stream) {
  return launch_reduce_adam(partial, scal_partial, n_wg, n_wg_pf, D, H, A, grads, info, adam, workspace, nullptr, 0, stream, -1, HEAD_CAT);
}
extern "C" int trl_ppo_cat_reduce_adam_net_f32(const float* partial, const double* scal_partial, int n_wg, int net,
                                               int D, int H, int A, float* grads, double* info, const trl_adam_t* adam,
                                               float* workspace, void* stream) {
  TRL_REQUIRE(net == 0 || net == 1, "net: 0 = policy, 1 = value function");
  return launch_reduce_adam(partial, scal_partial, n_wg, 0, D, H, A, grads, info, adam, workspace, nullptr, 0, stream, net, HEAD_CAT);
}

// The state-dependent-std head's folds (rows of trl_ppo_sd_minibatch_grad_f32; same row fold order, norm rendezvous and Adam
// arithmetic; optimiser groups [policy with 2A head rows, no logstd | value]).  The `_net` fold of a policy-only launch reads
// the second scalar block behind THAT launch's n_wg x 8.  The cross-rank variants do not exist for this head.
extern "C" int trl_ppo_sd_reduce_adam_f32(const float* partial, const double* scal_partial, int n_wg, int n_wg_pf,
                                          int D, int H, int A, float* grads, double* info, const trl_adam_t* adam,
                                          float* workspace, void* stream) {
  return launch_reduce_adam(partial, scal_partial, n_wg, n_wg_pf, D, H, A, grads, info, adam, workspace, nullptr, 0, stream, -1, HEAD_SD);
}
extern "C" int trl_ppo_sd_reduce_adam_net_f32(const float* partial, const double* scal_partial, int n_wg, int net,
                                              int D, int H, int A, float* grads, double* info, const trl_adam_t* adam,
                                              float* workspace, void* stream) {
  TRL_REQUIRE(net == 0 || net == 1, "net: 0 = policy, 1 = value function");
  return launch_reduce_adam(partial, scal_partial, n_wg, 0, D, H, A, grads, info, adam, workspace, nullptr, 0, stream, net, HEAD_SD);
}

// The folds behind trl_ppo_ln_minibatch_grad_f32 (k_ppo_ln.hip): the same kernels, launched with the block lengths, the
// partial stride and the logstd offset of a pair of which the policy (ln_mask bit 0) and / or the critic (bit 1) carries a
// LayerNorm -- gamma | beta (128 floats behind b1) are ordinary elements of the fold, of the clip norm and of Adam.  `head`:
// 0 Gaussian, 1 categorical, 2 state-dependent-std.  One rank: there is no cross-rank variant.
static bool ln_args_ok(int head, int ln_mask) { return head >= HEAD_GAUSS && head <= HEAD_SD && ln_mask >= 1 && ln_mask <= 3; }
extern "C" int trl_ppo_ln_reduce_f32(const float* partial, const double* scal_partial, int n_wg, int n_wg_pf, int D, int H, int A,
                                     int head, int ln_mask, const float* pf_params, float* grads, double* info, void* stream) {
  TRL_REQUIRE(ln_args_ok(head, ln_mask), "head must be 0..2 and ln_mask 1..3");
  return launch_reduce(partial, scal_partial, n_wg, n_wg_pf, D, H, A, pf_params, grads, info, stream, head, ln_mask);
}
extern "C" int trl_ppo_ln_reduce_adam_workspace(int D, int H, int A, int head, int ln_mask) {
  TRL_REQUIRE(ln_args_ok(head, ln_mask), "head must be 0..2 and ln_mask 1..3");
  return reduce_adam_workspace(D, H, A, head, ln_mask);
}
extern "C" int trl_ppo_ln_reduce_adam_f32(const float* partial, const double* scal_partial, int n_wg, int n_wg_pf, int D, int H,
                                          int A, int head, int ln_mask, float* grads, double* info, const trl_adam_t* adam,
                                          float* workspace, void* stream) {
  TRL_REQUIRE(ln_args_ok(head, ln_mask), "head must be 0..2 and ln_mask 1..3");
  return launch_reduce_adam(partial, scal_partial, n_wg, n_wg_pf, D, H, A, grads, info, adam, workspace, nullptr, 0, stream, -1, head, ln_mask);
}
extern "C" int trl_ppo_ln_reduce_adam_net_f32(const float* partial, const double* scal_partial, int n_wg, int net, int D, int H,
                                              int A, int head, int ln_mask, float* grads, double* info, const trl_adam_t* adam,
                                              float* workspace, void* stream) {
  TRL_REQUIRE(ln_args_ok(head, ln_mask), "head must be 0..2 and ln_mask 1..3");
  TRL_REQUIRE(net == 0 || net == 1, "net: 0 = policy, 1 = value function");
  return launch_reduce_adam(partial, scal_partial, n_wg, 0, D, H, A, grads, info, adam, workspace, nullptr, 0, stream, net, head, ln_mask);
}

// The folds behind trl_ppo_wide_minibatch_grad_f32 (k_ppo_wide.hip): the same kernels again, launched with the block lengths
// and the stride of a plain 128-wide pair.  A policy block is up to 22.8 k floats -- ~360 jobs of 64 parameters per network,
// against the 64-wide pair's ~100 -- so the fold / clip / Adam launch takes the job-loop form (LOOP = true) on a grid of
// PPO_WIDE_FOLD_BLOCKS blocks (half of it for one network's `_net` fold, two of which may wait beside each other): every
// block is resident while it polls, whatever the job count.  The kernel is untouched: its slot poll already strides over any
// number of slots, and the workspace query sizes the slots from the job count.  One rank: there is no cross-rank variant.
extern "C" int trl_ppo_wide_reduce_f32(const float* partial, const double* scal_partial, int n_wg, int n_wg_pf, int D, int H, int A,
                                       int head, const float* pf_params, float* grads, double* info, void* stream) {
  TRL_REQUIRE(head >= HEAD_GAUSS && head <= HEAD_SD, "head must be 0..2");
  return launch_reduce(partial, scal_partial, n_wg, n_wg_pf, D, H, A, pf_params, grads, info, stream, head, PPO_WIDE_MASK);
}
extern "C" int trl_ppo_wide_reduce_adam_workspace(int D, int H, int A, int head) {
  TRL_REQUIRE(head >= HEAD_GAUSS && head <= HEAD_SD, "head must be 0..2");
  return reduce_adam_workspace(D, H, A, head, PPO_WIDE_MASK);
}
extern "C" int trl_ppo_wide_reduce_adam_f32(const float* partial, const double* scal_partial, int n_wg, int n_wg_pf, int D, int H,
                                            int A, int head, float* grads, double* info, const trl_adam_t* adam,
                                            float* workspace, void* stream) {
  TRL_REQUIRE(head >= HEAD_GAUSS && head <= HEAD_SD, "head must be 0..2");
  return launch_reduce_adam(partial, scal_partial, n_wg, n_wg_pf, D, H, A, grads, info, adam, workspace, nullptr,
                            PPO_WIDE_FOLD_BLOCKS, stream, -1, head, PPO_WIDE_MASK);
}
extern "C" int trl_ppo_wide_reduce_adam_net_f32(const float* partial, const double* scal_partial, int n_wg, int net, int D, int H,
                                                int A, int head, float* grads, double* info, const trl_adam_t* adam,
                                                float* workspace, void* stream) {
  TRL_REQUIRE(head >= HEAD_GAUSS && head <= HEAD_SD, "head must be 0..2");
  TRL_REQUIRE(net == 0 || net == 1, "net: 0 = policy, 1 = value function");
  return launch_reduce_adam(partial, scal_partial, n_wg, 0, D, H, A, grads, info, adam, workspace, nullptr,
                            PPO_WIDE_FOLD_BLOCKS / 2, stream, net, head, PPO_WIDE_MASK);
}

// Env shards on several ranks: the same launch with the gradient SUM over ranks between the fold and the clip
// (torchrl/algo/on_policy/ppo.py:72-74, 117-119: clip_grad_norm_ sees the whole-minibatch gradient).  Needs a
// communicator whose peers are mapped (trl_comm_peer_open).
extern "C" int trl_ppo_reduce_adam_xrank_f32(const float* partial, const double* scal_partial, int n_wg, int n_wg_pf,
                                             int D, int H, int A, float* grads, double* info, const trl_adam_t* adam,
                                             float* workspace, trl_comm_t* comm, void* stream) {
  const XrArgs* xr = trl_comm_xr(comm);
  if (!xr) { trl_set_error("trl_ppo_reduce_adam_xrank_f32: communicator without mapped peers"); return TRL_EINVAL; }
  return launch_reduce_adam(partial, scal_partial, n_wg, n_wg_pf, D, H, A, grads, info, adam, workspace, xr,
                            trl_comm_wait_blocks(comm), stream);
}

// One network's half with the cross-rank SUM inside: the two update chains of a rank whose env shards sit on several
// ranks.  Each chain counts its own exchanges (ctl[4] / ctl[6] of the communicator) and owns its network's granules of the
// gradient region, so the two sequences of waiting launches never meet; a bounded wait footprint is shared between them.
extern "C" int trl_ppo_reduce_adam_xrank_net_f32(const float* partial, const double* scal_partial, int n_wg, int net,
                                                 int D, int H, int A, float* grads, double* info, const trl_adam_t* adam,
                                                 float* workspace, trl_comm_t* comm, void* stream) {
  TRL_REQUIRE(net == 0 || net == 1, "net: 0 = policy, 1 = value function");
  const XrArgs* xr = trl_comm_xr(comm);
  if (!xr) { trl_set_error("trl_ppo_reduce_adam_xrank_net_f32: communicator without mapped peers"); return TRL_EINVAL; }
  const int wb = trl_comm_wait_blocks(comm);
  return launch_reduce_adam(partial, scal_partial, n_wg, 0, D, H, A, grads, info, adam, workspace, xr,
                            wb > 0 ? (wb + 1) / 2 : 0, stream, net);
}

#define TICK_PENDING 0x70000001                    /* clip_adam_launch: the step state still has to be advanced */
static int clip_adam_launch(const trl_adam_t* p, void* stream, bool tick_here);
extern "C" int trl_clip_adam_f32(const trl_adam_t* p, void* stream) { return clip_adam_launch(p, stream, true); }

// clip + Adam followed by the Polyak step of the target networks (rl_algo.py:169-176 / utils.py:16-20), two launches:
// when the device-resident step state needs the one-thread tick kernel (large parameter blocks), the Polyak kernel's
// first thread advances it instead -- it runs behind the Adam kernel in stream order, i.e. after every block has read it.
// `file` (optional): block 0 also archives the update's statistics block into row (updates finished before this one) mod
// slots of a ring -- the last launch of the update, every statistic has been written by then.
struct FileRing { const uint32_t* raw; uint32_t* ring; const double* count; int words, slots, ticked; };
__global__ __launch_bounds__(256) void polyak_tick_kernel(float* __restrict__ tgt, const float* __restrict__ src, int64_t n,
                                                          float tau, double* __restrict__ st, float beta1, float beta2,
                                                          FileRing file) {
  if (file.ring && blockIdx.x == 0) {
    const int64_t u = (int64_t)file.count[0] - file.ticked;            // (read by every thread BEFORE thread 0 advances it)
    __syncthreads();
    uint32_t* row = file.ring + (int64_t)(((u % file.slots) + file.slots) % file.slots) * file.words;
    for (int w = threadIdx.x; w < file.words; w += 256) row[w] = file.raw[w];
  }
  if (st && blockIdx.x == 0 && threadIdx.x == 0) { st[0] += 1.0; st[1] *= (double)beta1; st[2] *= (double)beta2; }
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256)
    tgt[e] = tgt[e] * (1.0f - tau) + src[e] * tau;
}
// the launch itself (trl_common.h): behind clip_adam_kernel here and behind k_optim.hip's step kernel
int trl_polyak_file_launch(float* target, const float* source, int64_t n, float tau, double* tick_state, float beta1,
                           float beta2, const void* raw, int raw_bytes, void* ring, const double* count, int slots,
                           int ticked, void* stream) {
  int grid = trl_ceil_div(n, 256);
  if (grid > 1024) grid = 1024;
  FileRing file = {(const uint32_t*)raw, (uint32_t*)ring, count, raw_bytes / 4, slots, ticked};
  hipLaunchKernelGGL(polyak_tick_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, target, source, n, tau,
                     tick_state, beta1, beta2, file);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}
static int clip_adam_polyak(const trl_adam_t* p, float* target, const float* source, int64_t n, float tau,
                            const void* raw, int raw_bytes, void* ring, int slots, void* stream) {
  TRL_REQUIRE(n > 0 && target && source, "polyak: empty / null");
  int rc = clip_adam_launch(p, stream, false);
  if (rc != TRL_OK && rc != TICK_PENDING) return rc;
  return trl_polyak_file_launch(target, source, n, tau, rc == TICK_PENDING ? p->step_state : (double*)nullptr, p->beta1,
                                p->beta2, raw, raw_bytes, ring, p->step_state, slots, rc == TICK_PENDING ? 0 : 1, stream);
}
extern "C" int trl_clip_adam_polyak_f32(const trl_adam_t* p, float* target, const float* source, int64_t n, float tau,
                                        const void* raw, int raw_bytes, void* ring, int slots, void* stream) {
  if (!ring) return clip_adam_polyak(p, target, source, n, tau, nullptr, 0, nullptr, 0, stream);
  TRL_REQUIRE(raw && raw_bytes > 0 && raw_bytes % 4 == 0 && slots > 0, "clip_adam_polyak: bad ring");
  TRL_REQUIRE(p && p->step_state, "clip_adam_polyak: the ring row is picked by the device-resident step state");
  return clip_adam_polyak(p, target, source, n, tau, raw, raw_bytes, ring, slots, stream);
}

// ---------------------------------------------------------------- fold + clip + Adam + Polyak, ONE launch
// The tail of an off-policy update (twin_sac_q.py:162-220): fold of the split weight-gradient partials of every layer
// (trl_fold_partials_multi_f32's arithmetic and summation order), clip_grad_norm_ per network, the Adam steps, the Polyak
// step of the target networks (algo/utils.py:16-20), the filing of the update's statistics block -- three launches before
// (7 + 5 + 5 us for 217 k parameters at cfg 3, each latency-bound).  A grid of <= 256 always co-resident workgroups: a
// thread folds its parameters and leaves them in `grads`, the workgroup publishes its share of each group's sum of squares as
// {epoch, value} granules, every workgroup polls all of them (the rendezvous of ppo_reduce_adam_kernel: no ticket, no
// reset, device-scope relaxed accesses only), derives the clip coefficients in the same fixed order and steps its own
// parameters and their targets.  The step state is read by every workgroup BEFORE it publishes; workgroup 0 advances it
// after it has seen every granule.  A poll that does not complete (~1 s) trips workspace word 0 and leaves the parameters
// untouched.
#define FAP_THREADS 1024
#define FAP_MAX_WG 256
#define FAP_MAX_ENTRIES 32
struct FapDev {
  int count;
  int off[FAP_MAX_ENTRIES + 1];                    // entry k owns grads[off[k] .. off[k + 1])
  int splits[FAP_MAX_ENTRIES];
  const float* part[FAP_MAX_ENTRIES];              // [splits][n_k]
  float* target; int target_off, target_n; float tau;
  unsigned long long* slots;                       // [4 groups][FAP_MAX_WG] {epoch, ss bits}
  unsigned* err;
  float* grads_out;
};
__global__ __launch_bounds__(FAP_THREADS) void fold_adam_polyak_kernel(AdamDev a, FapDev f, FileRing file) {
  __shared__ float s_ss[4][FAP_THREADS / 64];
  __shared__ float s_coef[4];
  __shared__ float s_bc[2];
  __shared__ int s_fail;
  // (the entry table goes to LDS: a per-lane index into the argument struct would be a dependent load per element)
  __shared__ int s_off[FAP_MAX_ENTRIES + 1], s_splits[FAP_MAX_ENTRIES];
  __shared__ const float* s_part[FAP_MAX_ENTRIES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nb = gridDim.x;
  if (tid <= f.count) s_off[tid] = f.off[tid];
  if (tid < f.count) { s_splits[tid] = f.splits[tid]; s_part[tid] = f.part[tid]; }
  const int total = a.off[a.n_groups];
  const int per = (total + nb - 1) / nb, lo = blockIdx.x * per, hi = min(total, lo + per);
  // the step state and the ring row are read before anything is published (workgroup 0 advances the state at the end)
  const double steps = a.step_state[0];
  const unsigned epoch = (unsigned)(long long)steps + 1u;
  if (tid == 0) {
    s_bc[0] = (float)(1.0 - a.step_state[1] * (double)a.beta1);
    s_bc[1] = (float)sqrt(1.0 - a.step_state[2] * (double)a.beta2);
    s_fail = 0;
  }
  __syncthreads();
  // ---- fold (trl_fold_partials_multi_f32's order: four interleaved chains over the splits, then (0 + 1) + (2 + 3)) ----
  float ss[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int e = lo + tid; e < hi; e += FAP_THREADS) {
    int k = 0;
    while (k + 1 < f.count && e >= s_off[k + 1]) ++k;
    const int n = s_off[k + 1] - s_off[k], splits = s_splits[k];
    const float* p = s_part[k] + (e - s_off[k]);
    float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int s0 = 0;
    for (; s0 + 16 <= splits; s0 += 16) {          // 16 loads in flight: chain j takes splits j, j + 4, j + 8, ...
      float x[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) x[q] = p[(size_t)(s0 + q) * n];
#pragma unroll
      for (int q = 0; q < 16; ++q) c[q & 3] += x[q];
    }
    for (; s0 < splits; ++s0) c[s0 & 3] += p[(size_t)s0 * n];
    const float gsum = (c[0] + c[1]) + (c[2] + c[3]);
    f.grads_out[e] = gsum;
    int g = 0;
    while (e >= a.off[g + 1]) ++g;
    const float gs = gsum * a.grad_scale;
#pragma unroll
    for (int q = 0; q < 4; ++q) ss[q] = fmaf(q == g ? gs : 0.0f, gs, ss[q]);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float w = wave_sum(ss[q]);
    if (lane == 0) s_ss[q][wave] = w;
  }
  __syncthreads();
  if (tid < a.n_groups) {
    float t = 0.0f;
    for (int w = 0; w < FAP_THREADS / 64; ++w) t += s_ss[tid][w];
    __hip_atomic_store(f.slots + tid * FAP_MAX_WG + blockIdx.x, ((unsigned long long)epoch << 32) | __float_as_uint(t),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // ---- rendezvous: every workgroup's granules of this launch; group norms in workgroup order ----
  // wave w polls granules 64 r .. 64 r + 63 of group g (w = 4 g + r): all rounds of all groups fly together
  {
    const int g = wave >> 2, r = wave & 3, b = 64 * r + lane;
    float v = 0.0f;
    if (g < a.n_groups && b < nb) {
      const unsigned long long* slot = f.slots + g * FAP_MAX_WG + b;
      unsigned long long x = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned long long t0 = wall_clock64();
      while ((unsigned)(x >> 32) != epoch) {
        __builtin_amdgcn_s_sleep(1);
        x = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (wall_clock64() - t0 > 100000000ull) { s_fail = 1; break; }
      }
      v = __uint_as_float((unsigned)x);
    }
    v = wave_sum(v);                                   // a fixed tree over the round's 64 values
    if (lane == 0) s_ss[g & 3][r] = v;                 // (s_ss is free again: its sums were published above)
  }
  __syncthreads();
  if (tid < a.n_groups) {
    const float t = ((s_ss[tid][0] + s_ss[tid][1]) + s_ss[tid][2]) + s_ss[tid][3];      // rounds in order
    const float norm = sqrtf(t);
    s_coef[tid] = (a.max_norm > 0.0f) ? fminf(a.max_norm / (norm + 1e-6f), 1.0f) : 1.0f;
    if (blockIdx.x == 0 && a.norms_out) a.norms_out[tid] = norm;
  }
  __syncthreads();
  if (s_fail) { if (tid == 0) __hip_atomic_store(f.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
  // ---- Adam on the own parameters, Polyak on their targets ----
  const float bc1 = s_bc[0], bc2_sqrt = s_bc[1];
  for (int e = lo + tid; e < hi; e += FAP_THREADS) {
    int g = 0;
    while (e >= a.off[g + 1]) ++g;
    const float gr = f.grads_out[e] * a.grad_scale * s_coef[g];
    const float m = a.beta1 * a.m[e] + (1.0f - a.beta1) * gr;
    const float v = a.beta2 * a.v[e] + (1.0f - a.beta2) * gr * gr;
    a.m[e] = m; a.v[e] = v;
    const float denom = sqrtf(v) / bc2_sqrt + a.eps;
    const float lr = a.device_lr ? a.device_lr[g] : a.lr[g];
    const float pn = a.params[e] - (lr / bc1) * (m / denom);
    a.params[e] = pn;
    const int te = e - f.target_off;
    if (te >= 0 && te < f.target_n) f.target[te] = f.target[te] * (1.0f - f.tau) + pn * f.tau;
  }
  if (blockIdx.x == 0) {
    if (file.ring) {
      const int64_t u = (int64_t)steps;
      uint32_t* row = file.ring + (int64_t)(((u % file.slots) + file.slots) % file.slots) * file.words;
      for (int w = tid; w < file.words; w += FAP_THREADS) row[w] = file.raw[w];
    }
    if (tid == 0) { a.step_state[0] = steps + 1.0; a.step_state[1] *= (double)a.beta1; a.step_state[2] *= (double)a.beta2; }
  }
}
extern "C" int trl_fold_clip_adam_polyak_workspace(void) { return (int)(16 + 4 * FAP_MAX_WG * sizeof(unsigned long long)); }   // bytes, zeroed once
extern "C" int trl_fold_clip_adam_polyak_f32(int count, const float* const* part, const int* n, const int* splits,
                                             const trl_adam_t* adam, float* target, int64_t target_off, int64_t target_n,
                                             float tau, const void* raw, int raw_bytes, void* ring, int slots,
                                             void* workspace, void* stream) {
  TRL_REQUIRE(count >= 1 && count <= FAP_MAX_ENTRIES && part && n && splits, "fold_clip_adam_polyak: 1..32 fold entries");
  TRL_REQUIRE(adam && adam->step_state && workspace, "fold_clip_adam_polyak: needs the device-resident step state and a workspace");
  TRL_REQUIRE((!target_n) || (target && target_off >= 0), "fold_clip_adam_polyak: bad target range");
  TRL_REQUIRE(!ring || (raw && raw_bytes > 0 && raw_bytes % 4 == 0 && slots > 0), "fold_clip_adam_polyak: bad ring");
  AdamDev d;
  int rc = fill_adam(adam, d);
  if (rc) return rc;
  FapDev f{};
  f.count = count;
  for (int k = 0; k < count; ++k) {
    TRL_REQUIRE(part[k] && n[k] > 0 && splits[k] >= 1, "fold_clip_adam_polyak: bad entry");
    f.part[k] = part[k]; f.splits[k] = splits[k]; f.off[k + 1] = f.off[k] + n[k];
  }
  const int total = d.off[d.n_groups];
  TRL_REQUIRE(f.off[count] == total, "fold_clip_adam_polyak: the fold entries must cover the parameter block exactly, in order");
  TRL_REQUIRE(target_off + target_n <= total, "fold_clip_adam_polyak: target range outside the parameter block");
  f.target = target; f.target_off = (int)target_off; f.target_n = (int)target_n; f.tau = tau;
  f.err = (unsigned*)workspace;
  f.slots = (unsigned long long*)((char*)workspace + 16);
  f.grads_out = const_cast<float*>(adam->grads);
  FileRing file = {(const uint32_t*)raw, (uint32_t*)ring, adam->step_state, raw_bytes / 4, slots, 0};
  const int grid = std::max(1, std::min(FAP_MAX_WG, trl_ceil_div(total, FAP_THREADS)));
  hipLaunchKernelGGL(fold_adam_polyak_kernel, dim3(grid), dim3(FAP_THREADS), 0, (hipStream_t)stream, d, f, file);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

static int clip_adam_launch(const trl_adam_t* p, void* stream, bool tick_here) {
  AdamDev d;
  int rc = fill_adam(p, d);
  if (rc) return rc;
  TRL_REQUIRE(!p->device_state, "device_state is a feature of trl_ppo_reduce_adam_f32");
  const int total = d.off[p->n_groups];
  if (total == 0) return TRL_OK;
  // Up to 128 blocks count themselves through one atomic (a few hundred ns, hidden under the norm pass); larger
  // parameter blocks would serialise on it (860 blocks: 25 us measured), so they keep the one-thread tick launch.
  const int blocks = trl_ceil_div(total, 256);
  // (counting RETIRED blocks with a relaxed add at the end of each block instead was measured too: SAC cfg 3, 852 blocks,
  // 0.392 ms per update against 0.381 ms with the tick launch)
  d.self_tick = (d.step_state && blocks <= 128) ? 1 : 0;
  hipLaunchKernelGGL(clip_adam_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d);
  TRL_LAUNCH_CHECK();
  if (d.step_state && !d.self_tick) {
    if (!tick_here) return TICK_PENDING;             // the caller's next kernel advances the state
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, d.step_state, d.beta1, d.beta2);
    TRL_LAUNCH_CHECK();
  }
  return TRL_OK;
}

template <int D, int H, int O>
static int launch_fwd(const float* params, const float* x, float* out, int M, int act, hipStream_t s) {
  int grid = trl_ceil_div(M, 128);
  if (grid > 1024) grid = 1024;
  if (act == TRL_ACT_TANH)
    hipLaunchKernelGGL((mlp2_forward_kernel<D, H, O, TRL_ACT_TANH>), dim3(grid), dim3(256), 0, s, params, x, out, M);
  else
    hipLaunchKernelGGL((mlp2_forward_kernel<D, H, O, TRL_ACT_RELU>), dim3(grid), dim3(256), 0, s, params, x, out, M);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

extern "C" int trl_mlp2_forward_supported(int D, int H, int O) {
  return (D == 17 && H == 64 && (O == 6 || O == 1)) ? 1 : 0;     // keep in step with the dispatch below
}

extern "C" int trl_mlp2_forward_f32(const float* params, const float* x, float* out, int M, int D, int H,
                                    int O, int act, void* stream) {
  TRL_REQUIRE(M >= 0, "negative M");
  if (M == 0) return TRL_OK;
  TRL_REQUIRE(params && x && out, "null pointer");
  TRL_REQUIRE(act == TRL_ACT_TANH || act == TRL_ACT_RELU, "unknown activation");
  hipStream_t s = (hipStream_t)stream;
  if (D == 17 && H == 64 && O == 6) return launch_fwd<17, 64, 6>(params, x, out, M, act, s);
  if (D == 17 && H == 64 && O == 1) return launch_fwd<17, 64, 1>(params, x, out, M, act, s);
  trl_set_error("mlp2_forward: shape D=%d H=%d O=%d not instantiated", D, H, O);
  return TRL_EUNSUPPORTED;
}
