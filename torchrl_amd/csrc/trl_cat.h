// What the categorical kernels of more than one file share (k_categorical.hip, k_trpo.hip, k_vmpo.hip): the fixed
// arithmetic of a row of logits -- m = max_k l_k (the lowest index wins a tie), S = sum_k expf(l_k - m) in ascending k,
// log p_k = (l_k - m) - logf(S), p_k = expf(l_k - m) / S -- and the rule for a stored action outside [0, A).
#pragma once
#include "trl_common.h"

__device__ __forceinline__ float cat_row_max(const float* __restrict__ l, int A, int& arg) {
  float m = l[0];
  arg = 0;
  for (int k = 1; k < A; ++k) {
    const float x = l[k];
    if (x > m) { m = x; arg = k; }                                // strict: the lowest index wins a tie
  }
  return m;
}

// m and log S of a row: log p_k = (l_k - m) - logS
__device__ __forceinline__ float cat_row_norm(const float* __restrict__ l, int A, float& S) {
  int arg;
  const float m = cat_row_max(l, A, arg);
  S = 0.0f;
  for (int k = 0; k < A; ++k) S += expf(l[k] - m);
  return m;
}

// the stored action index as trl_cat_logp_f32 reads it: truncated, then clamped into [0, A)
__device__ __forceinline__ int cat_stored_action(float a, int A) { return min(max((int)a, 0), A - 1); }
