// Device functions of the LayerNorm forward pass shared by k_layernorm.hip (rows from global memory) and the fused 256-wide
// forward of k_mlp3.hip (rows of its LDS tile).  A sub-group of G lanes owns a row; lane sl holds the row's columns
// ln_col(sl, r) in registers r = 0 .. 4 CH - 1.
#pragma once
#include "trl_common.h"

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

// a per-column vector (gamma, beta) into the registers of its columns, 4-byte loads
template <bool VEC, int G, int CH> __device__ __forceinline__ void ln_load_cols(const float* p, int H, int sl, float (&v)[4 * CH]) {
#pragma unroll
  for (int r = 0; r < 4 * CH; ++r) {
    const int c = ln_col<VEC, G>(sl, r);
    v[r] = c < H ? p[c] : 0.0f;
  }
}

struct LnRowStats { float mean, rstd; };

// The row arithmetic of ln_fwd_rows (k_layernorm.hip), statement for statement, for a caller that holds the row already:
// v (columns past H hold 0) -> gamma * (v - mean) * rstd + beta in place -- the lane's values summed in register order,
// the xor butterfly, the mean, the squared deviations by fmaf, rstd = 1 / sqrt(q / H + eps).  (ln_fwd_rows keeps its own
// spelling: calling this from its row loop reorders the instructions of that file's kernels.)
template <bool VEC, int G, int CH>
__device__ __forceinline__ LnRowStats ln_row_norm(float (&v)[4 * CH], const float (&g)[4 * CH], const float (&b)[4 * CH], int H,
                                                  float inv_h, int sl) {
  constexpr int R = 4 * CH;
  float s = 0.0f;
#pragma unroll
  for (int r = 0; r < R; ++r) s += v[r];
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
  return LnRowStats{mean, rstd};
}
