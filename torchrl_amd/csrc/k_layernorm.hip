// LayerNorm layers of `add_ln=True` MLPs (reference: torchrl/networks/base.py:29-41, nets.py:28-37 -- the module list
// [Linear, act, LayerNorm] * n, the norm applied AFTER the activation over the feature axis, biased variance, eps 1e-5,
// affine weight / bias) and the second activation that replaces the trunk's last norm.
//
//   trl_layernorm_fwd_f32   a (M, H) -> y = gamma * (a - mean) * rstd + beta, and the per-row (mean, rstd) (M, 2)
//   trl_layernorm_bwd_f32   dy, a, (mean, rstd), gamma -> dz = da * act'(a) (the gradient at the pre-activation of the layer
//                           that produced a, so the GEMMs below run ungated), dgamma, dbeta
//   trl_act2_fwd_f32        t2 = act(t1)               (Tanh only: relu(relu(x)) == relu(x), nothing is launched for ReLU)
//   trl_act2_bwd_f32        dz = d * act'(t2) * act'(t1), both through the stored outputs
//
// A sub-group of G lanes of a wave owns a row at a time and keeps it in registers: G = 64 for 64 < H <= 1024 (at most 16
// values per lane), G = 16 for H <= 64 (four rows per wave).  The statistics are two passes over registers -- mean first,
// then the sum of squared deviations -- summed across the sub-group by xor shuffles; nothing goes through LDS.  With
// H % 4 == 0 and 16-byte aligned row bases a lane moves float4 pieces (piece c = sl + G i covers columns 4c .. 4c + 3, sl the
// lane's index in its sub-group), otherwise single floats (column sl + G i).  gamma / beta are read once per wave with 4-byte
// loads (they are views of a flat parameter vector, at any offset) and stay in registers while the wave walks its row
// blocks gw, gw + W, gw + 2W, ... (row block b = rows b * 64 / G .. of the matrix).
//
// dgamma[j] = sum_rows dy xhat and dbeta[j] = sum_rows dy: a sub-group accumulates its rows in registers in ascending row
// order, the sub-groups of a workgroup are added in a fixed order through LDS into the workgroup's slab of the workspace, and
// a second small launch adds the slabs (sixteen interleaved runs in ascending order, then the runs in order).  No atomics:
// the same (M, H) gives the same bits every time.
//
// Grouped forms (trl_layernorm_{fwd,bwd}_group_f32, trl_act2_{fwd,bwd}_group_f32; the off-policy engines: twin critics,
// targets, one network on several inputs): up to 12 problems of one shape in one launch, the same device functions per
// row.  The grid covers the G * M rows with the same number of workgroups per problem -- what the problem would take
// alone, capped at an even share of the single launch's cap -- so a problem is walked in the order it is walked alone and
// carries those bits.  A problem that wants no dgamma / dbeta writes no slabs; the slabs of the others are folded by ONE
// second launch, or left to a fold the caller runs anyway (trl_layernorm_bwd_group_partials_f32).
#include "trl_common.h"
#include "trl_mlp.h"

#define LN_THREADS 256
#define LN_WAVES (LN_THREADS / 64)
#define LN_MAX_H 1024
#define LN_MAX_WG_FWD 2048     // workgroups of the forward pass at most (eight waves per SIMD)
#define LN_MAX_WG_BWD 1024     // workgroups = slabs of the backward pass at most
#define LN_EPS 1e-5f

template <int G> __device__ __forceinline__ float ln_group_sum(float v) {      // every lane of a sub-group gets its sum
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// column of register r of sub-group lane sl
template <bool VEC, int G> __device__ __forceinline__ int ln_col(int sl, int r) {
  return VEC ? 4 * (sl + G * (r >> 2)) + (r & 3) : sl + G * r;
}

// a row into registers; columns past H (and every column of a row that does not exist) read as 0
template <bool VEC, int G, int CH>
__device__ __forceinline__ void ln_load_row(const float* row, int H, int sl, bool valid, float (&v)[4 * CH]) {
  if (VEC) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = 4 * (sl + G * i);
      f32x4 q = {0.0f, 0.0f, 0.0f, 0.0f};
      if (valid && c < H) q = *reinterpret_cast<const f32x4*>(row + c);  // H % 4 == 0: a piece is inside the row or outside
#pragma unroll
      for (int k = 0; k < 4; ++k) v[4 * i + k] = q[k];
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4 * CH; ++r) {
      const int c = sl + G * r;
      v[r] = (valid && c < H) ? row[c] : 0.0f;
    }
  }
}

template <bool VEC, int G, int CH>
__device__ __forceinline__ void ln_store_row(float* row, int H, int sl, bool valid, const float (&v)[4 * CH]) {
  if (VEC) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = 4 * (sl + G * i);
      if (valid && c < H) {
        f32x4 q = {v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
        *reinterpret_cast<f32x4*>(row + c) = q;
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4 * CH; ++r) {
      const int c = sl + G * r;
      if (valid && c < H) row[c] = v[r];
    }
  }
}

// a per-column vector (gamma, beta) into the registers of its columns, 4-byte loads
template <bool VEC, int G, int CH> __device__ __forceinline__ void ln_load_cols(const float* p, int H, int sl, float (&v)[4 * CH]) {
#pragma unroll
  for (int r = 0; r < 4 * CH; ++r) {
    const int c = ln_col<VEC, G>(sl, r);
    v[r] = c < H ? p[c] : 0.0f;
  }
}

// the forward pass of one (M, H) problem by the W waves gw = 0 .. W - 1 that share it
template <bool VEC, int G, int CH>
__device__ __forceinline__ void ln_fwd_rows(const float* __restrict__ a, const float* __restrict__ gamma,
                                            const float* __restrict__ beta, float* __restrict__ y, float* __restrict__ stats,
                                            int M, int H, int gw, int W) {
  constexpr int R = 4 * CH, RPW = 64 / G;
  const int lane = threadIdx.x & 63, sl = lane & (G - 1), sg = lane / G;
  const int n_blocks = (M + RPW - 1) / RPW;
  float g[R], b[R], v[R];
  ln_load_cols<VEC, G, CH>(gamma, H, sl, g);
  ln_load_cols<VEC, G, CH>(beta, H, sl, b);
  const float inv_h = 1.0f / (float)H;
  for (int blk = gw; blk < n_blocks; blk += W) {                          // (wave-uniform: the shuffles below see all lanes)
    const int m = blk * RPW + sg;
    const bool valid = m < M;
    ln_load_row<VEC, G, CH>(a + (size_t)m * H, H, sl, valid, v);
    float s = 0.0f;
#pragma unroll
    for (int r = 0; r < R; ++r) s += v[r];                              // (columns past H hold 0)
    const float mean = ln_group_sum<G>(s) * inv_h;
    float q = 0.0f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float d = ln_col<VEC, G>(sl, r) < H ? v[r] - mean : 0.0f;
      q = fmaf(d, d, q);
    }
    const float rstd = 1.0f / sqrtf(ln_group_sum<G>(q) * inv_h + LN_EPS);
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = fmaf(g[r], (v[r] - mean) * rstd, b[r]);
    ln_store_row<VEC, G, CH>(y + (size_t)m * H, H, sl, valid, v);
    if (valid && sl == 0) { stats[2 * (size_t)m] = mean; stats[2 * (size_t)m + 1] = rstd; }
  }
}

template <bool VEC, int G, int CH>
__global__ __launch_bounds__(LN_THREADS) void layernorm_fwd_kernel(const float* __restrict__ a, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float* __restrict__ y,
                                                                   float* __restrict__ stats, int M, int H) {
  ln_fwd_rows<VEC, G, CH>(a, gamma, beta, y, stats, M, H, blockIdx.x * LN_WAVES + (threadIdx.x >> 6), gridDim.x * LN_WAVES);
}

// Grouped launches: P same-shaped problems (at most LN_MAX_GROUPS, the group limit of the grouped dense-layer launches) in
// one grid of P * wgs_per workgroups -- workgroup b works on problem b / wgs_per as that problem's workgroup b % wgs_per,
// so every problem has the same share of the grid and a problem's rows, slabs and summation order do not depend on its
// neighbours.  The pointer tables travel by value in the kernel arguments (a captured graph holds no host memory).
#define LN_MAX_GROUPS 12
struct LnFwdGroup { const float* a[LN_MAX_GROUPS]; const float* gamma[LN_MAX_GROUPS]; const float* beta[LN_MAX_GROUPS];
                    float* y[LN_MAX_GROUPS]; float* stats[LN_MAX_GROUPS]; };
template <bool VEC, int G, int CH>
__global__ __launch_bounds__(LN_THREADS) void layernorm_fwd_group_kernel(LnFwdGroup p, int wgs_per, int M, int H) {
  const int g = blockIdx.x / wgs_per, b = blockIdx.x - g * wgs_per;         // (workgroup-uniform: the tables are read by scalar loads)
  ln_fwd_rows<VEC, G, CH>(p.a[g], p.gamma[g], p.beta[g], p.y[g], p.stats[g], M, H, b * LN_WAVES + (threadIdx.x >> 6),
                          wgs_per * LN_WAVES);
}

__device__ __forceinline__ float ln_act_grad(float h, int act) {       // act'(.) through the activation's OUTPUT h (trl_mlp.h)
  if (act == TRL_ACT_TANH) return fmaf(-h, h, 1.0f);
  if (act == TRL_ACT_RELU) return h > 0.0f ? 1.0f : 0.0f;
  return 1.0f;
}

// the backward pass of one (M, H) problem by its workgroups wg = 0 .. n_wg - 1; slab: this workgroup's [dgamma | dbeta]
// partial sums, or NULL (workgroup-uniform) when nobody wants the parameter gradients
template <bool VEC, int G, int CH>
__device__ __forceinline__ void ln_bwd_rows(const float* dy, const float* __restrict__ a, const float* __restrict__ stats,
                                            const float* __restrict__ gamma, int act, float* dz, float* __restrict__ slab,
                                            int M, int H, int wg, int n_wg) {
  constexpr int R = 4 * CH, RPW = 64 / G, COLS = G * R;                   // COLS >= H
  __shared__ float s_acc[LN_WAVES * RPW][2][COLS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sl = lane & (G - 1), sg = lane / G;
  const int gw = wg * LN_WAVES + wave, W = n_wg * LN_WAVES;
  const int n_blocks = (M + RPW - 1) / RPW;
  float g[R], dg[R], db[R], x[R], d[R], gt[R];
  ln_load_cols<VEC, G, CH>(gamma, H, sl, g);                            // (columns past H: gamma == 0, dy == 0, a == 0)
#pragma unroll
  for (int r = 0; r < R; ++r) dg[r] = db[r] = 0.0f;
  const float inv_h = 1.0f / (float)H;
  for (int blk = gw; blk < n_blocks; blk += W) {
    const int m = blk * RPW + sg;
    const bool valid = m < M;
    ln_load_row<VEC, G, CH>(a + (size_t)m * H, H, sl, valid, x);
    ln_load_row<VEC, G, CH>(dy + (size_t)m * H, H, sl, valid, d);
    const float mean = valid ? stats[2 * (size_t)m] : 0.0f, rstd = valid ? stats[2 * (size_t)m + 1] : 0.0f;
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      gt[r] = ln_act_grad(x[r], act);
      const float xh = ln_col<VEC, G>(sl, r) < H ? (x[r] - mean) * rstd : 0.0f;
      const float gd = d[r] * g[r];
      s1 += gd;
      s2 = fmaf(gd, xh, s2);
      dg[r] = fmaf(d[r], xh, dg[r]);                                     // (a row that does not exist: d == 0)
      db[r] += d[r];
      x[r] = xh;
      d[r] = gd;
    }
    s1 = ln_group_sum<G>(s1) * inv_h;
    s2 = ln_group_sum<G>(s2) * inv_h;
#pragma unroll
    for (int r = 0; r < R; ++r) d[r] = rstd * (d[r] - s1 - x[r] * s2) * gt[r];
    ln_store_row<VEC, G, CH>(dz + (size_t)m * H, H, sl, valid, d);
  }
  if (slab == nullptr) return;
  // the workgroup's slab [dgamma (H) | dbeta (H)]: its sub-groups added in (wave, sub-group) order
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int c = ln_col<VEC, G>(sl, r);                                 // < COLS
    s_acc[wave * RPW + sg][0][c] = dg[r];
    s_acc[wave * RPW + sg][1][c] = db[r];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * H; e += LN_THREADS) {
    const int k = e >= H, c = e - k * H;
    float t = s_acc[0][k][c];
#pragma unroll
    for (int w = 1; w < LN_WAVES * RPW; ++w) t += s_acc[w][k][c];
    slab[e] = t;
  }
}

template <bool VEC, int G, int CH>
__global__ __launch_bounds__(LN_THREADS) void layernorm_bwd_kernel(const float* dy, const float* __restrict__ a,
                                                                   const float* __restrict__ stats, const float* __restrict__ gamma,
                                                                   int act, float* dz, float* __restrict__ slabs, int M, int H) {
  ln_bwd_rows<VEC, G, CH>(dy, a, stats, gamma, act, dz, slabs + (size_t)blockIdx.x * 2 * H, M, H, blockIdx.x, gridDim.x);
}

// slabs[g]: problem g's wgs_per slabs, or NULL for a problem that wants dz only
struct LnBwdGroup { const float* dy[LN_MAX_GROUPS]; const float* a[LN_MAX_GROUPS]; const float* stats[LN_MAX_GROUPS];
                    const float* gamma[LN_MAX_GROUPS]; float* dz[LN_MAX_GROUPS]; float* slabs[LN_MAX_GROUPS]; };
template <bool VEC, int G, int CH>
__global__ __launch_bounds__(LN_THREADS) void layernorm_bwd_group_kernel(LnBwdGroup p, int act, int wgs_per, int M, int H) {
  const int g = blockIdx.x / wgs_per, b = blockIdx.x - g * wgs_per;
  float* slabs = p.slabs[g];
  ln_bwd_rows<VEC, G, CH>(p.dy[g], p.a[g], p.stats[g], p.gamma[g], act, p.dz[g],
                          slabs ? slabs + (size_t)b * 2 * H : nullptr, M, H, b, wgs_per);
}

// dgamma / dbeta: entry e of [dgamma | dbeta] is the sum of the slabs' entries -- LN_FOLD_RUNS interleaved runs (slabs p,
// p + 16, ...), each in ascending order by one thread (eight loads in flight), then the runs added in order.  A workgroup
// owns 16 entries, so even H = 64 spreads the up to 1024 dependent additions per entry over 8 workgroups x 16 runs.
#define LN_FOLD_RUNS 16
#define LN_FOLD_COLS (LN_THREADS / LN_FOLD_RUNS)
__device__ __forceinline__ void ln_fold_entries(const float* __restrict__ slabs, int n_slabs, int H, float* __restrict__ dgamma,
                                                float* __restrict__ dbeta, int block) {
  __shared__ float s_run[LN_FOLD_RUNS][LN_FOLD_COLS];
  const int el = threadIdx.x % LN_FOLD_COLS, run = threadIdx.x / LN_FOLD_COLS;
  const int e = block * LN_FOLD_COLS + el;
  float t = 0.0f;
  if (e < 2 * H) {
#pragma unroll 8
    for (int s = run; s < n_slabs; s += LN_FOLD_RUNS) t += slabs[(size_t)s * 2 * H + e];
  }
  s_run[run][el] = t;
  __syncthreads();
  if (run == 0 && e < 2 * H) {
    t = s_run[0][el];
#pragma unroll
    for (int r = 1; r < LN_FOLD_RUNS; ++r) t += s_run[r][el];
    if (e < H) dgamma[e] = t; else dbeta[e - H] = t;
  }
}

__global__ __launch_bounds__(LN_THREADS) void layernorm_fold_kernel(const float* __restrict__ slabs, int n_slabs, int H,
                                                                    float* __restrict__ dgamma, float* __restrict__ dbeta) {
  ln_fold_entries(slabs, n_slabs, H, dgamma, dbeta, blockIdx.x);
}

// the folds of every problem of a grouped backward launch that wanted parameter gradients: problem blockIdx.y of the table
struct LnFoldGroup { const float* slabs[LN_MAX_GROUPS]; float* dgamma[LN_MAX_GROUPS]; float* dbeta[LN_MAX_GROUPS]; };
__global__ __launch_bounds__(LN_THREADS) void layernorm_fold_group_kernel(LnFoldGroup f, int n_slabs, int H) {
  const int g = blockIdx.y;
  ln_fold_entries(f.slabs[g], n_slabs, H, f.dgamma[g], f.dbeta[g], blockIdx.x);
}

// the second activation of a trunk's last hidden layer: t2 = act(t1); dz = d act'(t2) act'(t1)
__device__ __forceinline__ void act2_fwd_span(const float* __restrict__ t1, float* __restrict__ t2, int64_t n, int act, int vec,
                                              int block, int n_blocks) {
  const int64_t stride = (int64_t)n_blocks * LN_THREADS;
  int64_t i = (int64_t)block * LN_THREADS + threadIdx.x;
  const int64_t n4 = vec ? n >> 2 : 0;
  for (int64_t c = i; c < n4; c += stride) {
    f32x4 q = reinterpret_cast<const f32x4*>(t1)[c];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = act == TRL_ACT_TANH ? trl_tanh(q[k]) : fmaxf(q[k], 0.0f);
    reinterpret_cast<f32x4*>(t2)[c] = q;
  }
  for (int64_t e = 4 * n4 + i; e < n; e += stride) t2[e] = act == TRL_ACT_TANH ? trl_tanh(t1[e]) : fmaxf(t1[e], 0.0f);
}

__global__ __launch_bounds__(LN_THREADS) void act2_fwd_kernel(const float* __restrict__ t1, float* __restrict__ t2, int64_t n,
                                                              int act, int vec) {
  act2_fwd_span(t1, t2, n, act, vec, blockIdx.x, gridDim.x);
}

__device__ __forceinline__ void act2_bwd_span(const float* d, const float* __restrict__ t1, const float* __restrict__ t2, float* dz,
                                              int64_t n, int act, int vec, int block, int n_blocks) {
  const int64_t stride = (int64_t)n_blocks * LN_THREADS;
  int64_t i = (int64_t)block * LN_THREADS + threadIdx.x;
  const int64_t n4 = vec ? n >> 2 : 0;
  for (int64_t c = i; c < n4; c += stride) {
    f32x4 q = reinterpret_cast<const f32x4*>(d)[c];
    const f32x4 u = reinterpret_cast<const f32x4*>(t1)[c], w = reinterpret_cast<const f32x4*>(t2)[c];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = q[k] * ln_act_grad(w[k], act) * ln_act_grad(u[k], act);
    reinterpret_cast<f32x4*>(dz)[c] = q;
  }
  for (int64_t e = 4 * n4 + i; e < n; e += stride) dz[e] = d[e] * ln_act_grad(t2[e], act) * ln_act_grad(t1[e], act);
}

__global__ __launch_bounds__(LN_THREADS) void act2_bwd_kernel(const float* d, const float* __restrict__ t1,
                                                              const float* __restrict__ t2, float* dz, int64_t n, int act, int vec) {
  act2_bwd_span(d, t1, t2, dz, n, act, vec, blockIdx.x, gridDim.x);
}

struct Act2Group { const float* d[LN_MAX_GROUPS]; const float* t1[LN_MAX_GROUPS]; const float* t2[LN_MAX_GROUPS];
                   float* out[LN_MAX_GROUPS]; };
__global__ __launch_bounds__(LN_THREADS) void act2_fwd_group_kernel(Act2Group p, int wgs_per, int64_t n, int act, int vec) {
  const int g = blockIdx.x / wgs_per;
  act2_fwd_span(p.t1[g], p.out[g], n, act, vec, blockIdx.x - g * wgs_per, wgs_per);
}
__global__ __launch_bounds__(LN_THREADS) void act2_bwd_group_kernel(Act2Group p, int wgs_per, int64_t n, int act, int vec) {
  const int g = blockIdx.x / wgs_per;
  act2_bwd_span(p.d[g], p.t1[g], p.t2[g], p.out[g], n, act, vec, blockIdx.x - g * wgs_per, wgs_per);
}

static inline bool ln_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// rows a workgroup takes at a time: one per sub-group of G lanes (G = 16 for H <= 64, else 64)
static inline int ln_rows_per_wg(int H) { return H <= 64 ? LN_WAVES * 4 : LN_WAVES; }
static inline int ln_workgroups(int M, int H, int max_wg) {
  const int want = trl_ceil_div(M, ln_rows_per_wg(H));
  return want < max_wg ? want : max_wg;
}

extern "C" int trl_layernorm_supported(int H) { return H >= 1 && H <= LN_MAX_H; }

#define LN_LAUNCH(KERNEL, V, G, CH, ...) \
  hipLaunchKernelGGL((KERNEL<V, G, CH>), dim3(wgs), dim3(LN_THREADS), 0, (hipStream_t)stream, __VA_ARGS__)
#define LN_DISPATCH(KERNEL, ...)                                          \
  do {                                                                    \
    if (vec) {                                                            \
      if (H <= 64) LN_LAUNCH(KERNEL, true, 16, 1, __VA_ARGS__);           \
      else if (H <= 256) LN_LAUNCH(KERNEL, true, 64, 1, __VA_ARGS__);     \
      else if (H <= 512) LN_LAUNCH(KERNEL, true, 64, 2, __VA_ARGS__);     \
      else LN_LAUNCH(KERNEL, true, 64, 4, __VA_ARGS__);                   \
    } else {                                                              \
      if (H <= 64) LN_LAUNCH(KERNEL, false, 16, 1, __VA_ARGS__);          \
      else if (H <= 256) LN_LAUNCH(KERNEL, false, 64, 1, __VA_ARGS__);    \
      else if (H <= 512) LN_LAUNCH(KERNEL, false, 64, 2, __VA_ARGS__);    \
      else LN_LAUNCH(KERNEL, false, 64, 4, __VA_ARGS__);                  \
    }                                                                     \
  } while (0)

extern "C" int trl_layernorm_fwd_f32(const float* a, const float* gamma, const float* beta, float* y, float* stats, int M,
                                     int H, void* stream) {
  TRL_REQUIRE(M >= 0, "bad row count");
  TRL_REQUIRE(H >= 1 && H <= LN_MAX_H, "LayerNorm rows of 1 <= H <= 1024 features are carried");
  if (M == 0) return TRL_OK;
  TRL_REQUIRE(a && gamma && beta && y && stats, "null pointer");
  const bool vec = H % 4 == 0 && ln_aligned16(a) && ln_aligned16(y);
  const int wgs = ln_workgroups(M, H, LN_MAX_WG_FWD);
  LN_DISPATCH(layernorm_fwd_kernel, a, gamma, beta, y, stats, M, H);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

extern "C" int trl_layernorm_bwd_workspace(int M, int H) {
  if (M <= 0 || H < 1 || H > LN_MAX_H) return TRL_EINVAL;
  return ln_workgroups(M, H, LN_MAX_WG_BWD) * 2 * H;                     // floats
}

extern "C" int trl_layernorm_bwd_f32(const float* dy, const float* a, const float* stats, const float* gamma, int act,
                                     float* dz, float* dgamma, float* dbeta, float* workspace, int M, int H, void* stream) {
  TRL_REQUIRE(M > 0, "bad row count");
  TRL_REQUIRE(H >= 1 && H <= LN_MAX_H, "LayerNorm rows of 1 <= H <= 1024 features are carried");
  TRL_REQUIRE(act == TRL_ACT_TANH || act == TRL_ACT_RELU || act == TRL_ACT_NONE, "bad activation code");
  TRL_REQUIRE(dy && a && stats && gamma && dz && dgamma && dbeta && workspace, "null pointer");
  const bool vec = H % 4 == 0 && ln_aligned16(a) && ln_aligned16(dy) && ln_aligned16(dz);
  const int wgs = ln_workgroups(M, H, LN_MAX_WG_BWD);
  LN_DISPATCH(layernorm_bwd_kernel, dy, a, stats, gamma, act, dz, workspace, M, H);
  TRL_LAUNCH_CHECK();
  hipLaunchKernelGGL(layernorm_fold_kernel, dim3(trl_ceil_div(2 * H, LN_FOLD_COLS)), dim3(LN_THREADS), 0, (hipStream_t)stream,
                     workspace, wgs, H, dgamma, dbeta);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

static inline int act2_grid(int64_t n) {
  const int64_t want = (n / 4 + LN_THREADS - 1) / LN_THREADS + 1;
  return (int)(want < 2048 ? want : 2048);
}

extern "C" int trl_act2_fwd_f32(const float* t1, float* t2, int64_t n, int act, void* stream) {
  TRL_REQUIRE(n >= 0, "bad size");
  TRL_REQUIRE(act == TRL_ACT_TANH || act == TRL_ACT_RELU, "bad activation code");
  if (n == 0) return TRL_OK;
  TRL_REQUIRE(t1 && t2, "null pointer");
  const int vec = ln_aligned16(t1) && ln_aligned16(t2);
  hipLaunchKernelGGL(act2_fwd_kernel, dim3(act2_grid(n)), dim3(LN_THREADS), 0, (hipStream_t)stream, t1, t2, n, act, vec);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

extern "C" int trl_act2_bwd_f32(const float* d, const float* t1, const float* t2, float* dz, int64_t n, int act, void* stream) {
  TRL_REQUIRE(n >= 0, "bad size");
  TRL_REQUIRE(act == TRL_ACT_TANH || act == TRL_ACT_RELU, "bad activation code");
  if (n == 0) return TRL_OK;
  TRL_REQUIRE(d && t1 && t2 && dz, "null pointer");
  const int vec = ln_aligned16(d) && ln_aligned16(t1) && ln_aligned16(t2) && ln_aligned16(dz);
  hipLaunchKernelGGL(act2_bwd_kernel, dim3(act2_grid(n)), dim3(LN_THREADS), 0, (hipStream_t)stream, d, t1, t2, dz, n, act, vec);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// ---------------------------------------------------------------- grouped entry points
// workgroups per problem of a grouped launch: what the problem would take alone, the launch's cap shared evenly
static inline int ln_group_workgroups(int G, int M, int H, int max_wg) {
  const int cap = max_wg / G;                                             // G <= 12: >= 85
  const int want = trl_ceil_div(M, ln_rows_per_wg(H));
  return want < cap ? want : cap;
}
#define LN_GROUP_REQUIRE(G) TRL_REQUIRE((G) >= 1 && (G) <= LN_MAX_GROUPS, "1..12 problems per grouped launch")

extern "C" int trl_layernorm_fwd_group_f32(int G, const float* const* a, const float* const* gamma, const float* const* beta,
                                           float* const* y, float* const* stats, int M, int H, void* stream) {
  LN_GROUP_REQUIRE(G);
  TRL_REQUIRE(M >= 0, "bad row count");
  TRL_REQUIRE(H >= 1 && H <= LN_MAX_H, "LayerNorm rows of 1 <= H <= 1024 features are carried");
  if (M == 0) return TRL_OK;
  TRL_REQUIRE(a && gamma && beta && y && stats, "null pointer");
  LnFwdGroup p{};
  bool vec = H % 4 == 0;
  for (int g = 0; g < G; ++g) {
    TRL_REQUIRE(a[g] && gamma[g] && beta[g] && y[g] && stats[g], "null pointer");
    p.a[g] = a[g]; p.gamma[g] = gamma[g]; p.beta[g] = beta[g]; p.y[g] = y[g]; p.stats[g] = stats[g];
    vec = vec && ln_aligned16(a[g]) && ln_aligned16(y[g]);                // one route per launch: every problem must qualify
  }
  const int per = ln_group_workgroups(G, M, H, LN_MAX_WG_FWD), wgs = G * per;
  LN_DISPATCH(layernorm_fwd_group_kernel, p, per, M, H);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// slabs per problem of the grouped backward pass (the `splits` of a deferred fold)
extern "C" int trl_layernorm_bwd_group_slabs(int G, int M, int H) {
  if (G < 1 || G > LN_MAX_GROUPS || M <= 0 || H < 1 || H > LN_MAX_H) return TRL_EINVAL;
  return ln_group_workgroups(G, M, H, LN_MAX_WG_BWD);
}

extern "C" int trl_layernorm_bwd_group_workspace(int G, int M, int H) {
  const int per = trl_layernorm_bwd_group_slabs(G, M, H);
  return per < 0 ? per : G * per * 2 * H;                                 // floats: problem g's slabs at g * per * 2 H
}

// the first launch of the grouped backward pass: dz of every problem, and the slabs [slab][dgamma (H) | dbeta (H)] of the
// problems with want[g] != 0 at workspace + g * slabs * 2 H (want NULL: of all).  Their sums are somebody else's launch:
// layernorm_fold_group_kernel below, or a fold that the caller runs anyway (an entry of trl_fold_partials_multi_f32 /
// trl_fold_clip_adam_polyak_f32 with n = 2 H and splits = slabs, when dgamma and dbeta lie back to back).
extern "C" int trl_layernorm_bwd_group_partials_f32(int G, const float* const* dy, const float* const* a, const float* const* stats,
                                                    const float* const* gamma, int act, float* const* dz, const int* want,
                                                    float* workspace, int M, int H, void* stream) {
  LN_GROUP_REQUIRE(G);
  TRL_REQUIRE(M > 0, "bad row count");
  TRL_REQUIRE(H >= 1 && H <= LN_MAX_H, "LayerNorm rows of 1 <= H <= 1024 features are carried");
  TRL_REQUIRE(act == TRL_ACT_TANH || act == TRL_ACT_RELU || act == TRL_ACT_NONE, "bad activation code");
  TRL_REQUIRE(dy && a && stats && gamma && dz, "null pointer");
  const int per = ln_group_workgroups(G, M, H, LN_MAX_WG_BWD), wgs = G * per;
  LnBwdGroup p{};
  bool vec = H % 4 == 0;
  for (int g = 0; g < G; ++g) {
    TRL_REQUIRE(dy[g] && a[g] && stats[g] && gamma[g] && dz[g], "null pointer");
    p.dy[g] = dy[g]; p.a[g] = a[g]; p.stats[g] = stats[g]; p.gamma[g] = gamma[g]; p.dz[g] = dz[g];
    if (!want || want[g]) {
      TRL_REQUIRE(workspace, "null pointer");
      p.slabs[g] = workspace + (size_t)g * per * 2 * H;
    }
    vec = vec && ln_aligned16(a[g]) && ln_aligned16(dy[g]) && ln_aligned16(dz[g]);
  }
  LN_DISPATCH(layernorm_bwd_group_kernel, p, act, per, M, H);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

extern "C" int trl_layernorm_bwd_group_f32(int G, const float* const* dy, const float* const* a, const float* const* stats,
                                           const float* const* gamma, int act, float* const* dz, float* const* dgamma,
                                           float* const* dbeta, float* workspace, int M, int H, void* stream) {
  LN_GROUP_REQUIRE(G);
  TRL_REQUIRE(dgamma && dbeta, "null pointer");
  int want[LN_MAX_GROUPS];
  LnFoldGroup f{};
  int n = 0;
  for (int g = 0; g < G; ++g) {                                           // dgamma[g] == NULL: problem g wants dz only
    want[g] = dgamma[g] != nullptr;
    TRL_REQUIRE(!want[g] || dbeta[g], "dgamma without dbeta");
  }
  const int rc = trl_layernorm_bwd_group_partials_f32(G, dy, a, stats, gamma, act, dz, want, workspace, M, H, stream);
  if (rc != TRL_OK) return rc;
  const int per = ln_group_workgroups(G, M, H, LN_MAX_WG_BWD);
  for (int g = 0; g < G; ++g)
    if (want[g]) { f.slabs[n] = workspace + (size_t)g * per * 2 * H; f.dgamma[n] = dgamma[g]; f.dbeta[n] = dbeta[g]; ++n; }
  if (n == 0) return TRL_OK;
  hipLaunchKernelGGL(layernorm_fold_group_kernel, dim3(trl_ceil_div(2 * H, LN_FOLD_COLS), n), dim3(LN_THREADS), 0,
                     (hipStream_t)stream, f, per, H);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

static inline int act2_group_grid(int G, int64_t n) {
  const int want = act2_grid(n), cap = 2048 / G;
  return want < cap ? want : cap;
}

extern "C" int trl_act2_fwd_group_f32(int G, const float* const* t1, float* const* t2, int64_t n, int act, void* stream) {
  LN_GROUP_REQUIRE(G);
  TRL_REQUIRE(n >= 0, "bad size");
  TRL_REQUIRE(act == TRL_ACT_TANH || act == TRL_ACT_RELU, "bad activation code");
  if (n == 0) return TRL_OK;
  TRL_REQUIRE(t1 && t2, "null pointer");
  Act2Group p{};
  int vec = 1;
  for (int g = 0; g < G; ++g) {
    TRL_REQUIRE(t1[g] && t2[g], "null pointer");
    p.t1[g] = t1[g]; p.out[g] = t2[g];
    vec = vec && ln_aligned16(t1[g]) && ln_aligned16(t2[g]);
  }
  const int per = act2_group_grid(G, n);
  hipLaunchKernelGGL(act2_fwd_group_kernel, dim3(G * per), dim3(LN_THREADS), 0, (hipStream_t)stream, p, per, n, act, vec);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

extern "C" int trl_act2_bwd_group_f32(int G, const float* const* d, const float* const* t1, const float* const* t2,
                                      float* const* dz, int64_t n, int act, void* stream) {
  LN_GROUP_REQUIRE(G);
  TRL_REQUIRE(n >= 0, "bad size");
  TRL_REQUIRE(act == TRL_ACT_TANH || act == TRL_ACT_RELU, "bad activation code");
  if (n == 0) return TRL_OK;
  TRL_REQUIRE(d && t1 && t2 && dz, "null pointer");
  Act2Group p{};
  int vec = 1;
  for (int g = 0; g < G; ++g) {
    TRL_REQUIRE(d[g] && t1[g] && t2[g] && dz[g], "null pointer");
    p.d[g] = d[g]; p.t1[g] = t1[g]; p.t2[g] = t2[g]; p.out[g] = dz[g];
    vec = vec && ln_aligned16(d[g]) && ln_aligned16(t1[g]) && ln_aligned16(t2[g]) && ln_aligned16(dz[g]);
  }
  const int per = act2_group_grid(G, n);
  hipLaunchKernelGGL(act2_bwd_group_kernel, dim3(G * per), dim3(LN_THREADS), 0, (hipStream_t)stream, p, per, n, act, vec);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}
