// The persistent rollout for 128- and 256-wide two-layer networks: rollout_wide_kernel and value_pass_wide_kernel, shared by
// k_rollout_wide.hip (the plain networks, entry point trl_rollout_synth_wide_f32) and k_rollout_wide_ln.hip (the LayerNorm
// variants, LN = true, entry point trl_rollout_synth_wide_ln_f32).  Same contract, same stored formats and same launch
// descriptor as the 64-wide kernels of trl_rollout.h (whose env step, heads, noise paths and bookkeeping are restated here so
// that the 64-wide instantiations keep the code they have); what is new is the trunk.
//
// The 64-wide kernel keeps a wave's 16 x 64 slice of W2 in 16 registers.  At H = 256 W2 is 256 KB: it does not fit a CU's LDS,
// only the register files of the CU.  Decision (both widths, one data path):
//   * rollout_wide_kernel: 4 waves (256 threads, ONE wave per SIMD, one workgroup per CU), a workgroup = 16 envs for all
//     n_steps, as before.  One wave per SIMD gives each wave the SIMD's whole file, 256 VGPRs + 256 AGPRs.  Wave w owns hidden
//     rows [w H / 4, (w + 1) H / 4) of BOTH layers: NT = H / 64 row tiles of 16 (2 at H = 128, 4 at H = 256); its rows of W1 (XK
//     floats per tile), W2 (H / 4 floats per tile: 2 x 32 = 64 at H = 128, 4 x 64 = 256 at H = 256) and W3 (4 per tile) are loaded
//     once and are MFMA A operands for the whole launch; at H = 256 the compiler parks W2 in the AGPR half of the file.
//     8 waves (two per SIMD, the issue's suggested split) were built first: each wave then has 256 registers in all, of which
//     W2 takes 128 at H = 256, and with W1, W3 and the env matrices moved to LDS the compiler still spilled 4 - 32 dwords of
//     step state to scratch.  The MFMA pipe is per SIMD, so one wave with twice the row tiles issues the same MFMAs in the
//     same time as two waves sharing it -- and the env step and head epilogue, which every wave repeats, run in 4 waves
//     instead of 8.  Registers over LDS for W2 at H = 128 too: 64 KB of LDS would fit, but every layer-2 MFMA would then wait
//     for a ds_read of its A operand;
//   * layer 1: NT tiles x XK MFMAs, activation, store_T into ONE [H][16] LDS tile, barrier; layer 2: every wave reads the whole
//     tile (H / 16 slices of 4 floats) as B operands -- each slice read once and used by the wave's NT tiles, two slices
//     requested ahead of the MFMAs that use them -- in 2 accumulation chains per tile (4 / 8 independent chains per wave:
//     16 / 32 dependent MFMAs per chain instead of 32 / 64);
//   * head: per-wave partial over the wave's own H / 4 rows into headp[4][HC][16], barrier, summed over the waves in ascending
//     order by every lane, as the 64-wide kernel sums its four;
//   * 2 barriers per step (+ 1 per 16 steps of device noise).  The env step is computed by all 4 waves (everyone owns next_obs
//     in the operand layout of the next layer 1); its matrices depend on the lane alone and sit in LDS ([q][lane], 5 KB); what
//     one wave is enough for is dealt out as in the 64-wide kernel: obs, next_obs, acts, the four scalars + log pi.
// Registers per lane (compiler's figures, gfx950; per instantiation in profiles/NOTES_wide_rollout.md): H = 128: 212 - 237 VGPRs
// + 16 AGPRs; H = 256: 256 VGPRs + 204 - 244 AGPRs; no scratch in any instantiation.  LDS: b1, b2 [H] | b3 [16] | logstd [8] |
// env matrices [2][10][64] | H1 [H][17] | headp [4][HC][16] | eps [16][8][16] = 25 / 27 KB (H = 128, HC = 8 / 16), 35 / 37 KB (256).
//
// value_pass_wide_kernel: 8 waves (two per SIMD), wave w owns rows [w H / 8, (w + 1) H / 8): W2 is 32 / 128 registers, and with
// no env step to carry 117 - 238 VGPRs are enough (no scratch).  A wave no longer holds all of W2, so the workgroup's waves
// exchange layer 1 through LDS; one barrier pair serves CT = 512 / H column tiles of 16 samples (4 at H = 128, 2 at H = 256:
// 34 KB of H1 tiles either way).  The 1-wide head is a per-lane dot over the wave's rows, two cross-lane adds, a per-wave
// partial in LDS and an ascending sum over the waves.  Whether a round needs the second forward (an over-length marker or the
// boot row among its samples) is read from the same global words by every wave, so the branch around its barriers is uniform
// without an exchange.
//
// LN: the reference's `add_ln` two-layer trunk Linear, act, LayerNorm(H), Linear, act, act, Linear; the parameter block is in
// plan order [W1 | b1 | gamma1 | beta1 | W2 | b2 | W3 | b3 (| logstd)].  An env's H activations are spread over the waves, so the
// row statistics are combined, not recomputed: every wave forms the mean of its own H / W rows and the sum of squared
// deviations M2 about THAT mean (lane tree + one ones x value MFMA each, ro_group_sum), lane group 0 puts (mean_w, M2_w) into
// stat[W][2][16] in front of the barrier that separates the layers anyway, and behind it every lane combines the W partials in
// ascending wave order, mean = sum mean_w / W, M2 = sum M2_w + (H / W) sum (mean_w - mean)^2 -- the exact equal-count pairwise
// combination, no E[x^2] - E[x]^2 -- so the barrier count stays 2 per step (one pair per round in the value pass).  The
// activations cross LDS un-normalised; (v - mean) * rstd is applied to the B operands where rw_layer2 loads them (a subtraction
// and a multiplication: one fma against -mean rstd would cancel under a large mean).  gamma and beta cost nothing in the step
// loop: the set-up folds beta into the bias, b2' = b2 + W2 beta (rw_fold_ln), and gamma into the W2 registers.  Layer 2
// applies the activation twice, as the reference's construction leaves it.  The value pass does the same with W = 8 and a
// stat[8][CT][2][16] block.
#pragma once
#include "trl_rollout.h"

#define RW_WAVES 4                                  // rollout_wide_kernel: one wave per SIMD
#define RW_THREADS (64 * RW_WAVES)
#define RW_NB 16                                    // steps of exploration noise per batch: one (step, env) per thread
#define RW_EK 10                                    // k steps of the env GEMM at the wide input tile (8 observation + 2 action)
#define VW_WAVES 8                                  // value_pass_wide_kernel: two waves per SIMD
#define VW_THREADS (64 * VW_WAVES)

template <int H, int HC_, bool LN = false> struct RwShape {
  static_assert(H == 128 || H == 256, "instantiated for H == 128 and H == 256");
  static_assert(HC_ == 8 || HC_ == 16, "the head exchange carries half or all of the 16-row head tile");
  static constexpr int HC = HC_, NT = H / (16 * RW_WAVES), NS = H / 16;
  // b1 [H] | b2 [H] | b3 [16] | logstd [8] | env matrices [2][RW_EK][64] | H1 [H][TL] | headp [4][HC][16] | eps [RW_NB][8][16]
  // (| LN: stat [4][2][16])
  static constexpr int O_B1 = 0, O_B2 = H, O_B3 = 2 * H, O_LS = O_B3 + 16, O_ENV = O_LS + 8, O_H1 = O_ENV + 2 * RW_EK * 64,
                       O_HP = O_H1 + H * TL, O_EPS = O_HP + RW_WAVES * HC * 16, O_ST = O_EPS + RW_NB * 8 * 16,
                       LDS_FLOATS = O_ST + (LN ? RW_WAVES * 2 * 16 : 0);
};

// The wave's rows of W1 and W2 as MFMA A operands: lane (i, g), tile tl <-> row 16 (NT wave + tl) + i; W1 k steps as in
// rollout_kernel (features 4g + q, then 16 + g (narrow tile) or 16 + 4g + q (wide tile)), W2 k index 16 sl + 4 g + r.
// LN: gamma1 | beta1 stand between b1 and W2.
template <int H, int NT, int XK, bool WIDE, bool LN = false>
__device__ __forceinline__ void rw_load_trunk(const float* __restrict__ gp, int Dr, int wave, int i, int g,
                                              float (&w1)[NT][XK], float (&w2)[NT][H / 16][4]) {
  constexpr int NS = H / 16;
  const int F_W2 = H * Dr + H + (LN ? 2 * H : 0);
#pragma unroll
  for (int tl = 0; tl < NT; ++tl) {
    const int row = 16 * (NT * wave + tl) + i;
#pragma unroll
    for (int q = 0; q < XK; ++q) {
      const int k = q < 4 ? 4 * g + q : WIDE ? 16 + 4 * g + (q - 4) : 16 + g;
      w1[tl][q] = k < Dr ? gp[row * Dr + (k < Dr ? k : 0)] : 0.0f;
    }
#pragma unroll
    for (int sl = 0; sl < NS; ++sl)
#pragma unroll
      for (int r = 0; r < 4; ++r) w2[tl][sl][r] = gp[F_W2 + row * H + 16 * sl + 4 * g + r];
  }
}

// LN set-up, once per launch, from gb = gamma [H] | beta [H] in LDS: beta goes into the bias, b2'[row] = b2[row] + sum_k
// W2[row][k] beta[k] -- the lane's quarter of k in ascending order, the four lane groups by two xor shuffles in fixed order,
// lane group 0 writes the wave's rows of the LDS bias block the layer-2 accumulators start from -- and then gamma into the
// W2 registers, w2[tl][sl][r] *= gamma[16 sl + 4 g + r]: the step loop sees neither.
template <int H, int NT>
__device__ __forceinline__ void rw_fold_ln(const float* gb, const float* __restrict__ b2, float* b2_lds, int wave, int i, int g,
                                           float (&w2)[NT][H / 16][4]) {
  constexpr int NS = H / 16;
#pragma unroll
  for (int tl = 0; tl < NT; ++tl) {
    float p = 0.0f;
#pragma unroll
    for (int sl = 0; sl < NS; ++sl)
#pragma unroll
      for (int r = 0; r < 4; ++r) p = fmaf(w2[tl][sl][r], gb[H + 16 * sl + 4 * g + r], p);
    p += __shfl_xor(p, 16, 64);
    p += __shfl_xor(p, 32, 64);
    const int row = 16 * (NT * wave + tl) + i;
    if (g == 0) b2_lds[row] = b2[row] + p;
  }
#pragma unroll
  for (int sl = 0; sl < NS; ++sl)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gm = gb[16 * sl + 4 * g + r];
#pragma unroll
      for (int tl = 0; tl < NT; ++tl) w2[tl][sl][r] *= gm;
    }
}

// LN, in front of the barrier between the layers: the wave's own 16 NT rows of env j (4 NT per lane, the env's four lane
// groups) -> their mean and the sum of squared deviations about THAT mean, to st[j] and st[16 + j].
template <int NT> __device__ __forceinline__ float rw_tree(const f32x4 (&v)[NT]) {
  static_assert(NT == 1 || NT == 2 || NT == 4, "1, 2 or 4 row tiles per wave");
  f32x4 s;
  if constexpr (NT == 1) s = v[0];
  else if constexpr (NT == 2) s = v[0] + v[1];
  else s = (v[0] + v[1]) + (v[2] + v[3]);
  return (s[0] + s[1]) + (s[2] + s[3]);
}
template <int NT> __device__ __forceinline__ void rw_ln_partial(const f32x4 (&h)[NT], float* st, int j, int g) {
  const float mean = ro_group_sum(rw_tree<NT>(h)) * (1.0f / (16 * NT));
  f32x4 q[NT];
#pragma unroll
  for (int tl = 0; tl < NT; ++tl)
#pragma unroll
    for (int r = 0; r < 4; ++r) { const float d = h[tl][r] - mean; q[tl][r] = d * d; }
  const float m2 = ro_group_sum(rw_tree<NT>(q));
  if (g == 0) { st[j] = mean; st[16 + j] = m2; }
}
// LN, behind that barrier: the W waves' partials (st + w stride) of env j in ascending wave order -> the row's mean and
// 1 / sqrt(var + eps).  Equal counts: mean = sum mean_w / W, M2 = sum M2_w + (H / W) sum (mean_w - mean)^2.
template <int H, int W> __device__ __forceinline__ void rw_ln_combine(const float* st, int stride, int j, float& mean, float& rstd) {
  float mw[W], m = 0.0f, m2 = 0.0f;
#pragma unroll
  for (int w = 0; w < W; ++w) { mw[w] = st[w * stride + j]; m += mw[w]; m2 += st[w * stride + 16 + j]; }
  mean = m * (1.0f / W);
  float d2 = 0.0f;
#pragma unroll
  for (int w = 0; w < W; ++w) { const float d = mw[w] - mean; d2 = fmaf(d, d, d2); }
  m2 = fmaf((float)(H / W), d2, m2);
  rstd = 1.0f / sqrtf(m2 * (1.0f / H) + LN_EPS);
}
__device__ __forceinline__ f32x4 rw_ln_apply(f32x4 v, float mean, float rstd) {
#pragma unroll
  for (int r = 0; r < 4; ++r) { v[r] -= mean; v[r] *= rstd; }
  return v;
}

// Layer 2 of the wave's NT row tiles over the [H][16] activation tile S: NCH chains per tile, chain 0 starts from b2; the sum
// of the chains is returned un-activated.  LN: S holds the un-normalised activations, the B operands are (v - mean) * rstd of
// the lane's env (gamma is in w2, beta in b2s: rw_fold_ln).
template <int H, int NT, bool LN = false>
__device__ __forceinline__ void rw_layer2(const float* __restrict__ S, const float* __restrict__ b2s, int j, int g,
                                          const float (&w2)[NT][H / 16][4], f32x4 (&out)[NT], float mean = 0.0f, float rstd = 1.0f) {
  constexpr int NS = H / 16, NCH = NT >= 4 ? 2 : 4 / NT;
  f32x4 acc[NT][NCH];
#pragma unroll
  for (int tl = 0; tl < NT; ++tl) {
    acc[tl][0] = *reinterpret_cast<const f32x4*>(b2s + 16 * tl);
#pragma unroll
    for (int c = 1; c < NCH; ++c) acc[tl][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // B operands two slices at a time, the next pair requested before the current pair's MFMAs; the fence keeps the scheduler
  // from hoisting all H / 4 LDS reads over the chains (which costs the registers W2 needs)
  f32x4 b0 = load_T(S, 0, j, g), b1 = load_T(S, 1, j, g);
  if constexpr (LN) { b0 = rw_ln_apply(b0, mean, rstd); b1 = rw_ln_apply(b1, mean, rstd); }
#pragma unroll
  for (int sl = 0; sl < NS; sl += 2) {
    f32x4 n0 = b0, n1 = b1;
    if (sl + 2 < NS) {
      n0 = load_T(S, sl + 2, j, g); n1 = load_T(S, sl + 3, j, g);
      if constexpr (LN) { n0 = rw_ln_apply(n0, mean, rstd); n1 = rw_ln_apply(n1, mean, rstd); }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int tl = 0; tl < NT; ++tl) {
        acc[tl][sl % NCH] = mfma16(w2[tl][sl][r], b0[r], acc[tl][sl % NCH]);
        acc[tl][(sl + 1) % NCH] = mfma16(w2[tl][sl + 1][r], b1[r], acc[tl][(sl + 1) % NCH]);
      }
    __builtin_amdgcn_sched_barrier(0);
    b0 = n0; b1 = n1;
  }
#pragma unroll
  for (int tl = 0; tl < NT; ++tl) {
    f32x4 s = acc[tl][0];
#pragma unroll
    for (int c = 1; c < NCH; ++c) s += acc[tl][c];
    out[tl] = s;
  }
}

// TILE: capacity of the input tile (17 or 32 features), the actual dims come with the launch (a.D, a.A), as in the runtime-dims
// instantiations of rollout_kernel; HEAD as there.  No normaliser, no staged noise, no noise gate (refused by the entry point).
template <int TILE, int H, int ACT, int HEAD, bool LN = false>
__global__ __launch_bounds__(RW_THREADS, 1) void rollout_wide_kernel(RolloutDev a) {
  static_assert(TILE == 17 || TILE == 32, "input tiles of 17 or 32 features");
  using S = RwShape<H, HEAD == HEAD_SD ? 16 : 8, LN>;
  constexpr bool WIDE = TILE > 17, CAT = HEAD == HEAD_CAT, SD = HEAD == HEAD_SD;
  constexpr int NT = S::NT;
  const int Dr = a.D, Ar = a.A;
  const int HW = SD ? 2 * Ar : Ar;                  // rows of W3 / b3
  const int F_B1 = H * Dr, F_G1 = F_B1 + H, F_W2 = F_B1 + H + (LN ? 2 * H : 0), F_B2 = F_W2 + H * H, F_W3 = F_B2 + H,
            F_B3 = F_W3 + HW * H, F_LS = F_B3 + HW;
  __shared__ __attribute__((aligned(16))) float lds[S::LDS_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int mo = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: branches on it stay scalar
  const int j = lane & 15, g = lane >> 4, i = j;
  const int n = blockIdx.x * RO_ENVS + j;
  const bool valid = n < a.N;
  const float* gp = a.pf_params;
  const bool has_lo = g < Ar, has_hi = 4 + g < Ar;          // the lane's two action dims: g and 4 + g
  const int o_lo = has_lo ? g : 0, o_hi = has_hi ? 4 + g : 0;
  if (blockIdx.x == 0 && tid == 0 && a.clear_hdr) { a.clear_hdr[0] = 0.0; a.clear_hdr[1] = 0.0; }   // the NEXT launch's header

  // ---- one-time setup: biases / logstd to LDS, this wave's weight rows to registers ----
  if constexpr (LN) {                                // b2 is written by the fold; gamma | beta wait for it in the (idle) H1 tile
    for (int e = tid; e < H; e += RW_THREADS) {
      lds[S::O_B1 + e] = gp[F_B1 + e]; lds[S::O_H1 + e] = gp[F_G1 + e]; lds[S::O_H1 + H + e] = gp[F_G1 + H + e];
    }
  } else {
    for (int e = tid; e < H; e += RW_THREADS) { lds[S::O_B1 + e] = gp[F_B1 + e]; lds[S::O_B2 + e] = gp[F_B2 + e]; }
  }
  if (tid < 16) lds[S::O_B3 + tid] = tid < HW ? gp[F_B3 + (tid < HW ? tid : 0)] : 0.0f;
  if (tid < 8) lds[S::O_LS + tid] = (HEAD == HEAD_GAUSS && tid < Ar) ? gp[F_LS + (tid < Ar ? tid : 0)] : 0.0f;
  bool fv[4], fv2[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { fv[q] = 4 * g + q < Dr; fv2[q] = WIDE && 16 + 4 * g + q < Dr; }
  const bool f16 = !WIDE && 16 + g < Dr;             // narrow tile: the 5th k step carries feature 16 + g
  const bool row_f = i < Dr, row_f2 = WIDE && 16 + i < Dr;   // env GEMM rows (next features i, 16 + i) that exist
  constexpr int XK = WIDE ? 8 : 5, EK = XK + 2;      // obs k steps of layer 1; k steps of the env GEMM (+ the two action steps)
  float w1r[NT][XK], w2r[NT][S::NS][4], w3a[NT][4];
  rw_load_trunk<H, NT, XK, WIDE, LN>(gp, Dr, mo, i, g, w1r, w2r);
  if constexpr (LN) {
    __syncthreads();                                 // gamma | beta are in LDS
    rw_fold_ln<H, NT>(lds + S::O_H1, gp + F_B2, lds + S::O_B2, mo, i, g, w2r);
  }
#pragma unroll
  for (int tl = 0; tl < NT; ++tl)
#pragma unroll
    for (int r = 0; r < 4; ++r) w3a[tl][r] = (i < HW) ? gp[F_W3 + (i < HW ? i : 0) * H + 16 * (NT * mo + tl) + 4 * g + r] : 0.0f;
  // env GEMM next^T[f][j] = sum_k M[f][k] [obs; act]^T[k][j]: features 0..15 (we0), wide tile 16..31 (we1); narrow tile:
  // feature 16 is a per-lane partial dot (w16) + a lane-group sum.  The operands depend on the lane alone, not on the wave,
  // and the registers are W2's: they sit in LDS, [q][lane] (conflict-free), and are read where a step uses them.
  float* envw0 = lds + S::O_ENV + lane;                    // we0[q] = envw0[64 q]
  float* envw1 = envw0 + RW_EK * 64;                       // we1[q] (wide tile) or w16[q] (narrow tile)
  if (mo == 0) {
    const bool has16 = !WIDE && Dr > 16;
#pragma unroll
    for (int q = 0; q < EK; ++q) {
      const float* mat = q < XK ? a.env_A : a.env_B;
      int k; bool kin;
      if (q < 4) { k = 4 * g + q; kin = k < Dr; }
      else if (q < XK) { k = WIDE ? 16 + 4 * g + (q - 4) : 16 + g; kin = k < Dr; }
      else { k = (q == XK) ? g : 4 + g; kin = k < Ar; }
      const int kc = kin ? k : 0;
      envw0[64 * q] = (kin && row_f) ? mat[kc * Dr + (row_f ? i : 0)] : 0.0f;
      if constexpr (WIDE) envw1[64 * q] = (kin && row_f2) ? mat[kc * Dr + (row_f2 ? 16 + i : 0)] : 0.0f;
      else envw1[64 * q] = (kin && has16) ? mat[kc * Dr + (has16 ? 16 : 0)] : 0.0f;
    }
  }
  __syncthreads();

  float* S_H1 = lds + S::O_H1;
  float* headp = lds + S::O_HP;
  float* S_EPS = lds + S::O_EPS;
  float* S_ST = lds + S::O_ST;                             // (LN only: the block has no floats otherwise)
  const float* b1s = lds + S::O_B1 + 16 * NT * mo + 4 * g;
  const float* b2s = lds + S::O_B2 + 16 * NT * mo + 4 * g;

  // the lane's two action dims (SD: the std is the env's own, from the head's rows Ar + o -- overwritten every step)
  float ls_lo = fminf(fmaxf(lds[S::O_LS + o_lo], -20.0f), 2.0f), ls_hi = fminf(fmaxf(lds[S::O_LS + o_hi], -20.0f), 2.0f);
  float std_lo = __expf(ls_lo), std_hi = __expf(ls_hi);
  float iv_lo = __expf(-2.0f * ls_lo), iv_hi = __expf(-2.0f * ls_hi);
  const float b3_lo = lds[S::O_B3 + o_lo], b3_hi = lds[S::O_B3 + o_hi];

  // ---- per-env state (replicated in all 4 waves and all 4 lane groups) ----
  float xb[XK];
#pragma unroll
  for (int r = 0; r < 4; ++r) xb[r] = (valid && fv[r]) ? a.cur_obs[(size_t)n * Dr + (fv[r] ? 4 * g + r : 0)] : 0.0f;
  if constexpr (WIDE) {
#pragma unroll
    for (int r = 0; r < 4; ++r) xb[4 + r] = (valid && fv2[r]) ? a.cur_obs[(size_t)n * Dr + (fv2[r] ? 16 + 4 * g + r : 0)] : 0.0f;
  } else {
    xb[4] = (valid && f16) ? a.cur_obs[(size_t)n * Dr + (f16 ? 16 + g : 0)] : 0.0f;
  }
  int t_env = valid ? a.t_env[n] : 0;
  int cur_step = valid ? a.cur_step[n] : 0;
  int ep_idx = valid ? a.episode_idx[n] : 0;
  float ep_ret = valid ? a.ep_return[n] : 0.0f;
  const int64_t env_seed = a.env_seed_base + n;
  double rew_sum = 0.0;
  const bool dev_noise = !a.deterministic && !a.noise;
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int t = 0; t < a.n_steps; ++t) {
    const int row = (a.top + t) % a.rows;
    const size_t cell = (size_t)row * a.N + n;

    // ---- exploration noise: host block or device Philox, RW_NB steps at a time: thread (wave mo, env j, g) draws step
    // t + 4 mo + g -- the values rollout_kernel / the per-step launches draw at that step ----
    if (dev_noise && (t % RW_NB) == 0) {
      const int ts = 4 * mo + g;
      const int64_t gs = a.noise_step0 + t + ts;
      if constexpr (CAT) {
        S_EPS[ts * 16 + j] = trl_cat_uniform(a.cat_seed, gs, a.cat_env0 + n);
      } else {
        float z0[4], z1[4];
        philox_normals4((uint32_t)(gs & 0xFFFFFFFFll), (uint32_t)((gs >> 32) & 0xFFFFFFFFll), 0u, TRL_TAG_NOISE, env_seed, z0);
        if (Ar > 4)
          philox_normals4((uint32_t)(gs & 0xFFFFFFFFll), (uint32_t)((gs >> 32) & 0xFFFFFFFFll), 1u, TRL_TAG_NOISE, env_seed, z1);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          S_EPS[(ts * 8 + c) * 16 + j] = z0[c];
          if (4 + c < Ar) S_EPS[(ts * 8 + 4 + c) * 16 + j] = z1[c];
        }
      }
      __syncthreads();   // readers of the previous batch finished before the barriers of the step that ended it
    }
    float cat_u = 0.0f, eps_lo = 0.0f, eps_hi = 0.0f;
    if constexpr (CAT) {
      if (dev_noise) cat_u = S_EPS[(t % RW_NB) * 16 + j];
    } else {
      if (dev_noise) {
        eps_lo = S_EPS[((t % RW_NB) * 8 + o_lo) * 16 + j];
        eps_hi = S_EPS[((t % RW_NB) * 8 + o_hi) * 16 + j];
      } else if (a.noise) {
        eps_lo = valid ? a.noise[((size_t)t * a.N + n) * Ar + o_lo] : 0.0f;
        eps_hi = valid ? a.noise[((size_t)t * a.N + n) * Ar + o_hi] : 0.0f;
      }
    }

    // ---- policy forward: layer 1 of the wave's rows ----
    if constexpr (LN) {
      auto layer1 = [&](int tl) {
        f32x4 h1 = *reinterpret_cast<const f32x4*>(b1s + 16 * tl);
#pragma unroll
        for (int q = 0; q < XK; ++q) h1 = mfma16(w1r[tl][q], xb[q], h1);
#pragma unroll
        for (int r = 0; r < 4; ++r) h1[r] = act_fn<ACT>(h1[r]);
        return h1;
      };
      // the wave's share of the row statistics rides on the same barrier
      if constexpr (NT == 4) {
        // H = 256 has no 16 registers to hold the wave's four tiles across both passes: the tiles go to LDS as they are
        // made, two at a time, and the pass about the mean reads the lane's OWN stores back (same lane, same addresses:
        // no barrier); the sums keep rw_ln_partial's tree, (t0 + t1) + (t2 + t3)
        f32x4 s2[2], q2[2];
#pragma unroll
        for (int tp = 0; tp < 2; ++tp) {
          const f32x4 ha = layer1(2 * tp), hb = layer1(2 * tp + 1);
          store_T(S_H1, NT * mo + 2 * tp, ha, j, g);
          store_T(S_H1, NT * mo + 2 * tp + 1, hb, j, g);
          s2[tp] = ha + hb;
        }
        const float mean_w = ro_group_sum(rw_tree<2>(s2)) * (1.0f / (16 * NT));
#pragma unroll
        for (int tp = 0; tp < 2; ++tp) {
          f32x4 da = load_T(S_H1, NT * mo + 2 * tp, j, g), db = load_T(S_H1, NT * mo + 2 * tp + 1, j, g);
#pragma unroll
          for (int r = 0; r < 4; ++r) { da[r] -= mean_w; db[r] -= mean_w; q2[tp][r] = da[r] * da[r] + db[r] * db[r]; }
        }
        const float m2_w = ro_group_sum(rw_tree<2>(q2));
        if (g == 0) { S_ST[32 * mo + j] = mean_w; S_ST[32 * mo + 16 + j] = m2_w; }
      } else {
        f32x4 h1[NT];
#pragma unroll
        for (int tl = 0; tl < NT; ++tl) h1[tl] = layer1(tl);
        rw_ln_partial<NT>(h1, S_ST + 32 * mo, j, g);
#pragma unroll
        for (int tl = 0; tl < NT; ++tl) store_T(S_H1, NT * mo + tl, h1[tl], j, g);
      }
    } else {
#pragma unroll
      for (int tl = 0; tl < NT; ++tl) {
        f32x4 h1 = *reinterpret_cast<const f32x4*>(b1s + 16 * tl);
#pragma unroll
        for (int q = 0; q < XK; ++q) h1 = mfma16(w1r[tl][q], xb[q], h1);
#pragma unroll
        for (int r = 0; r < 4; ++r) h1[r] = act_fn<ACT>(h1[r]);
        store_T(S_H1, NT * mo + tl, h1, j, g);
      }
    }
    // the observation part of the env step does not wait for the action: it runs in the shadow of the barriers
    f32x4 e0 = zero4, e1 = zero4;
    float p16 = 0.0f;
#pragma unroll
    for (int q = 0; q < XK; ++q) {
      e0 = mfma16(envw0[64 * q], xb[q], e0);
      if constexpr (WIDE) e1 = mfma16(envw1[64 * q], xb[q], e1);
      else p16 = fmaf(envw1[64 * q], xb[q], p16);
    }
    __syncthreads();
    f32x4 h2[NT];
    if constexpr (LN) {
      float ln_mean, ln_rstd;
      rw_ln_combine<H, RW_WAVES>(S_ST, 32, j, ln_mean, ln_rstd);
      rw_layer2<H, NT, true>(S_H1, b2s, j, g, w2r, h2, ln_mean, ln_rstd);
#pragma unroll
      for (int tl = 0; tl < NT; ++tl)
#pragma unroll
        for (int r = 0; r < 4; ++r) h2[tl][r] = act_fn<ACT>(h2[tl][r]);   // (the second application follows below)
    } else {
      rw_layer2<H, NT>(S_H1, b2s, j, g, w2r, h2);
    }
    f32x4 hp = zero4;                                      // partial head over the wave's own H / 8 features: D[o][env]
#pragma unroll
    for (int tl = 0; tl < NT; ++tl)
#pragma unroll
      for (int r = 0; r < 4; ++r) hp = mfma16(w3a[tl][r], act_fn<ACT>(h2[tl][r]), hp);
    if (SD || g < 2) {                                     // lane group g holds head rows 4g .. 4g + 3
#pragma unroll
      for (int r = 0; r < 4; ++r) headp[(mo * S::HC + 4 * g + r) * 16 + j] = hp[r];
    }
    __syncthreads();
    float mean_lo = b3_lo, mean_hi = b3_hi;
#pragma unroll
    for (int w = 0; w < RW_WAVES; ++w) { mean_lo += headp[(w * S::HC + o_lo) * 16 + j]; mean_hi += headp[(w * S::HC + o_hi) * 16 + j]; }
    if constexpr (SD) {
      // this step's std from the raw log_std rows Ar + o of the head (0 <= Ar + o < 2 Ar <= 16)
      float raw_lo = lds[S::O_B3 + Ar + o_lo], raw_hi = lds[S::O_B3 + Ar + o_hi];
#pragma unroll
      for (int w = 0; w < RW_WAVES; ++w) {
        raw_lo += headp[(w * S::HC + Ar + o_lo) * 16 + j];
        raw_hi += headp[(w * S::HC + Ar + o_hi) * 16 + j];
      }
      ls_lo = fminf(fmaxf(raw_lo, -20.0f), 2.0f); ls_hi = fminf(fmaxf(raw_hi, -20.0f), 2.0f);
      std_lo = __expf(ls_lo); std_hi = __expf(ls_hi);
      iv_lo = __expf(-2.0f * ls_lo); iv_hi = __expf(-2.0f * ls_hi);
    }

    // categorical head: cat_act_kernel's rule (k_categorical.hip) on the env's Ar logits, every lane for its own env
    int cat_k = 0;
    float cat_lsel = 0.0f, cat_m = 0.0f, cat_S = 1.0f;
    if constexpr (CAT) {
      float lg[8], ex[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float l = lds[S::O_B3 + k];
#pragma unroll
        for (int w = 0; w < RW_WAVES; ++w) l += headp[(w * 8 + k) * 16 + j];
        lg[k] = l;
      }
      cat_m = lg[0];
#pragma unroll
      for (int k = 1; k < 8; ++k)
        if (k < Ar && lg[k] > cat_m) { cat_m = lg[k]; cat_k = k; }    // strict: the lowest index wins a tie
      cat_S = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < Ar) { ex[k] = expf(lg[k] - cat_m); cat_S += ex[k]; }
      if (dev_noise) {
        const float thr = cat_u * cat_S;
        float c = 0.0f;
        bool hit = false;
        cat_k = Ar - 1;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < Ar) {
            c += ex[k];
            if (!hit && c >= thr) { cat_k = k; hit = true; }
          }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) cat_lsel = k == cat_k ? lg[k] : cat_lsel;
    }
    // action + log-prob under the collecting policy
    const float z_lo = fmaf(std_lo, eps_lo, mean_lo), z_hi = fmaf(std_hi, eps_hi, mean_hi);
    const float act_lo = CAT ? (g == cat_k ? 1.0f : 0.0f) : has_lo ? (a.tanh_action ? trl_tanh(z_lo) : z_lo) : 0.0f;
    const float act_hi = CAT ? (4 + g == cat_k ? 1.0f : 0.0f) : has_hi ? (a.tanh_action ? trl_tanh(z_hi) : z_hi) : 0.0f;
    // ---- env step, action part ----
    e0 = mfma16(envw0[64 * XK], act_lo, e0);
    e0 = mfma16(envw0[64 * (XK + 1)], act_hi, e0);
    if constexpr (WIDE) {
      e1 = mfma16(envw1[64 * XK], act_lo, e1);
      e1 = mfma16(envw1[64 * (XK + 1)], act_hi, e1);
    } else {
      p16 = fmaf(envw1[64 * XK], act_lo, p16);
      p16 = fmaf(envw1[64 * (XK + 1)], act_hi, p16);
    }
    // lane-group sums (same env, g = 0..3) as ones x value MFMAs: every lane gets the total
    const float e16 = WIDE ? 0.0f : mfma16(1.0f, p16, zero4)[0];
    const float act_sq = mfma16(1.0f, fmaf(act_lo, act_lo, act_hi * act_hi), zero4)[0];   // all action dims
    float logp = 0.0f;
    if (mo == 3) {                                          // only the wave that stores old_logp needs it
      if constexpr (CAT) {
        logp = (cat_lsel - cat_m) - logf(cat_S);
      } else {
        float zc, lp = 0.0f;
        if (has_lo) lp += gauss_logp_term(act_lo, mean_lo, iv_lo, ls_lo, a.tanh_action, zc);
        if (has_hi) lp += gauss_logp_term(act_hi, mean_hi, iv_hi, ls_hi, a.tanh_action, zc);
        logp = mfma16(1.0f, lp, zero4)[0];
      }
    }
    float nx[XK];
#pragma unroll
    for (int r = 0; r < 4; ++r) nx[r] = trl_tanh(e0[r]);     // features 4g + r (absent ones: tanh(0) = 0)
    if constexpr (WIDE) {
#pragma unroll
      for (int r = 0; r < 4; ++r) nx[4 + r] = trl_tanh(e1[r]);   // features 16 + 4g + r
    } else {
      nx[4] = (g == 0 && Dr > 16) ? trl_tanh(e16) : 0.0f;    // feature 16
    }
    // feature 0 lives in lane group 0 (r == 0): broadcast to the other groups with a selector MFMA
    const float nx0 = mfma16(1.0f, g == 0 ? nx[0] : 0.0f, zero4)[0];
    float raw_rew = a.reward_scale * (nx0 - 0.1f * act_sq);
    // the ring stores this ROUNDED product and an episode's return is the float32 sum of the stored rewards: keep the product
    // from being contracted into `ep_ret += raw_rew` as an fma of the unrounded one (see rollout_kernel)
    asm volatile("" : "+v"(raw_rew));
    t_env += 1; cur_step += 1;
    const bool done = t_env >= a.horizon;
    const bool surpass = cur_step >= a.max_episode_frames;
    ep_ret += raw_rew;
    if (mo == 0 && g == 0 && valid) {
      rew_sum += (double)raw_rew;
      if (done) {
        const int slot = atomicAdd(a.ep_count, 1);
        if (slot < a.ep_cap) { a.ep_log[slot * 3 + 0] = (float)(a.step0 + t); a.ep_log[slot * 3 + 1] = (float)n; a.ep_log[slot * 3 + 2] = ep_ret; }
      }
    }
    if (done) ep_ret = 0.0f;

    float xn[XK];
#pragma unroll
    for (int q = 0; q < XK; ++q) xn[q] = nx[q];
    if (done || surpass) {                                  // partial reset + counters
      ep_idx += 1; t_env = 0; cur_step = 0;
      float z[4];
      philox_normals4((uint32_t)ep_idx, 0u, (uint32_t)g, TRL_TAG_RESET, env_seed, z);     // features 4g..4g+3
#pragma unroll
      for (int c = 0; c < 4; ++c) xn[c] = fv[c] ? z[c] : 0.0f;
      if constexpr (WIDE) {
        philox_normals4((uint32_t)ep_idx, 0u, (uint32_t)(4 + g), TRL_TAG_RESET, env_seed, z);   // features 16 + 4g ..
#pragma unroll
        for (int c = 0; c < 4; ++c) xn[4 + c] = fv2[c] ? z[c] : 0.0f;
      } else {
        xn[4] = 0.0f;
        if (g == 0 && Dr > 16) {
          philox_normals4((uint32_t)ep_idx, 0u, 4u, TRL_TAG_RESET, env_seed, z);          // feature 16
          xn[4] = z[0];
        }
      }
    }

    // ---- ring-buffer row `row`, one key group per wave ----
    if (valid && a.store) {
      if (mo == 0 || mo == 1) {
        float* dst = (mo == 0 ? a.obs : a.next_obs) + cell * Dr;
#pragma unroll
        for (int r = 0; r < 4; ++r) if (fv[r]) dst[4 * g + r] = mo == 0 ? xb[r] : nx[r];
        if constexpr (WIDE) {
#pragma unroll
          for (int r = 0; r < 4; ++r) if (fv2[r]) dst[16 + 4 * g + r] = mo == 0 ? xb[4 + r] : nx[4 + r];
        } else {
          if (g == 0 && Dr > 16) dst[16] = mo == 0 ? xb[4] : nx[4];
        }
      } else if (mo == 2) {
        if constexpr (CAT) {
          if (g == 0) a.acts[cell] = (float)cat_k;          // (N, 1): the index
        } else {
          if (has_lo) a.acts[cell * Ar + g] = act_lo;
          if (has_hi) a.acts[cell * Ar + 4 + g] = act_hi;
        }
      } else {
        // lane group g writes key g; values[cell] carries the over-length marker to the value pass
        float* dst = g == 0 ? a.values : g == 1 ? a.rewards : g == 2 ? a.terminals : a.time_limits;
        const float val = g == 0 ? (surpass ? 1.0f : 0.0f) : g == 1 ? raw_rew
                        : g == 2 ? ((done || surpass) ? 1.0f : 0.0f) : (done ? 1.0f : 0.0f);
        dst[cell] = val;
        if (g == 0 && a.old_logp) a.old_logp[cell] = logp;
      }
    }
#pragma unroll
    for (int q = 0; q < XK; ++q) xb[q] = xn[q];
  }

  // ---- persist env / collector state ----
  if (mo == 0 && valid) {
    float* dst = a.cur_obs + (size_t)n * Dr;
#pragma unroll
    for (int r = 0; r < 4; ++r) if (fv[r]) dst[4 * g + r] = xb[r];
    if constexpr (WIDE) {
#pragma unroll
      for (int r = 0; r < 4; ++r) if (fv2[r]) dst[16 + 4 * g + r] = xb[4 + r];
    } else {
      if (g == 0 && Dr > 16) dst[16] = xb[4];
    }
  }
  if (mo == 1 && valid && g == 0) { a.t_env[n] = t_env; a.cur_step[n] = cur_step; a.episode_idx[n] = ep_idx; a.ep_return[n] = ep_ret; }
  if (mo == 0) {
    const double tot = wave_sum(rew_sum);
    if (lane == 0 && a.epoch_reward) atomicAdd(a.epoch_reward, tot);
  }
}

// ---------------------------------------------------------------- value pass over the stored cells
// value_pass_kernel's contract (trl_rollout.h): values[cell] = V(obs[cell]); rewards[cell] += discount * V(next_obs[cell])
// where the rollout left the over-length marker; boot[n] = V(next_obs) of the last step's row; the pub_* copy.  A round is
// CT column tiles of 16 samples; sample m = t N + n of column tile c sits in lane j = m % 16 of every wave.
template <int TILE, int H, int ACT, bool LN = false>
__global__ __launch_bounds__(VW_THREADS, 1) void value_pass_wide_kernel(ValueDev a) {
  static_assert(TILE == 17 || TILE == 32, "input tiles of 17 or 32 features");
  static_assert(H == 128 || H == 256, "instantiated for H == 128 and H == 256");
  constexpr bool WIDE = TILE > 17;
  constexpr int XK = WIDE ? 8 : 5, NT = H / (16 * VW_WAVES), NS = H / 16, CT = 512 / H;
  const int Dr = a.D;
  // MlpFlat<Dr, H, 1>; LN: gamma1 | beta1 between b1 and W2
  const int F_B1 = H * Dr, F_W2 = F_B1 + H + (LN ? 2 * H : 0), F_B2 = F_W2 + H * H, F_W3 = F_B2 + H, F_B3 = F_W3 + H;
  __shared__ __attribute__((aligned(16))) float sb[2 * H];
  __shared__ float S_H1[CT * H * TL];
  __shared__ float vp[VW_WAVES * CT * 16 + (LN ? VW_WAVES * CT * 32 : 0)];   // head partials (| LN: stat [8][CT][2][16])
  float* S_ST = vp + VW_WAVES * CT * 16;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4, i = j;
  const float* gp = a.vf_params;
  if constexpr (LN) {                                // b2 is written by the fold; gamma | beta wait for it in the (idle) H1 tiles
    for (int e = tid; e < H; e += VW_THREADS) { sb[e] = gp[F_B1 + e]; S_H1[e] = gp[F_B1 + H + e]; S_H1[H + e] = gp[F_B1 + 2 * H + e]; }
  } else {
    for (int e = tid; e < H; e += VW_THREADS) { sb[e] = gp[F_B1 + e]; sb[H + e] = gp[F_B2 + e]; }
  }
  bool fv[4], fv2[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { fv[q] = 4 * g + q < Dr; fv2[q] = WIDE && 16 + 4 * g + q < Dr; }
  const bool f16 = !WIDE && 16 + g < Dr;
  float w1[NT][XK], w2[NT][NS][4], w3[NT][4];
  rw_load_trunk<H, NT, XK, WIDE, LN>(gp, Dr, wave, i, g, w1, w2);
  if constexpr (LN) {
    __syncthreads();                                 // gamma | beta are in LDS
    rw_fold_ln<H, NT>(S_H1, gp + F_B2, sb + H, wave, i, g, w2);
  }
#pragma unroll
  for (int tl = 0; tl < NT; ++tl)
#pragma unroll
    for (int r = 0; r < 4; ++r) w3[tl][r] = gp[F_W3 + 16 * (NT * wave + tl) + 4 * g + r];
  const float b3 = gp[F_B3];
  const float* b1s = sb + 16 * NT * wave + 4 * g;
  const float* b2s = sb + H + 16 * NT * wave + 4 * g;
  __syncthreads();

  // (posted writes into host memory, issued before the tiles: they complete under the pass)
  for (int64_t e = (int64_t)blockIdx.x * VW_THREADS + tid; e < a.pub_words; e += (int64_t)gridDim.x * VW_THREADS)
    a.pub_dst[e] = a.pub_src[e];
  const int64_t M = (int64_t)a.n_steps * a.N;
  const int64_t n_tiles = (M + 15) / 16, n_rounds = (n_tiles + CT - 1) / CT;
  auto locate = [&](int64_t tile, bool& ok, int& t, int& n) -> size_t {
    const int64_t m = tile * 16 + j;
    ok = tile < n_tiles && m < M;
    t = ok ? (int)(m / a.N) : 0;
    n = ok ? (int)(m - (int64_t)t * a.N) : 0;
    return (size_t)((a.top + t) % a.rows) * a.N + n;
  };
  for (int64_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {   // (the same trip count in every wave)
    size_t cell[CT];
    bool ok[CT];
    int t_c[CT], n_c[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) cell[c] = locate(round * CT + c, ok[c], t_c[c], n_c[c]);
    // the lane's OWN sample: lane j of column tile g % CT -- its marker, and (wave 0, g < CT) its stores
    size_t cell_o = cell[0];
    bool ok_o = ok[0];
    int t_o = t_c[0], n_o = n_c[0];
#pragma unroll
    for (int c = 1; c < CT; ++c)
      if ((g & (CT - 1)) == c) { cell_o = cell[c]; ok_o = ok[c]; t_o = t_c[c]; n_o = n_c[c]; }
    const float marker = ok_o ? a.values[cell_o] : 0.0f;
    const bool last = ok_o && a.boot && t_o == a.n_steps - 1;          // the row the epoch's bootstrap value comes from
    // every wave reads the same words: the same answer in all eight, before anyone overwrites values[] (behind two barriers)
    const bool second = __ballot(marker != 0.0f || last) != 0ull;
    for (int ph = 0; ph < (second ? 2 : 1); ++ph) {
      const float* src = ph ? a.next_obs : a.obs;
      float x[CT][XK];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
#pragma unroll
        for (int r = 0; r < 4; ++r) x[c][r] = (ok[c] && fv[r]) ? src[cell[c] * Dr + (fv[r] ? 4 * g + r : 0)] : 0.0f;
        if constexpr (WIDE) {
#pragma unroll
          for (int r = 0; r < 4; ++r) x[c][4 + r] = (ok[c] && fv2[r]) ? src[cell[c] * Dr + (fv2[r] ? 16 + 4 * g + r : 0)] : 0.0f;
        } else {
          x[c][4] = (ok[c] && f16) ? src[cell[c] * Dr + (f16 ? 16 + g : 0)] : 0.0f;
        }
      }
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if constexpr (LN) {
          f32x4 h1[NT];
#pragma unroll
          for (int tl = 0; tl < NT; ++tl) {
            h1[tl] = *reinterpret_cast<const f32x4*>(b1s + 16 * tl);
#pragma unroll
            for (int q = 0; q < XK; ++q) h1[tl] = mfma16(w1[tl][q], x[c][q], h1[tl]);
#pragma unroll
            for (int r = 0; r < 4; ++r) h1[tl][r] = act_fn<ACT>(h1[tl][r]);
          }
          rw_ln_partial<NT>(h1, S_ST + (wave * CT + c) * 32, j, g);
#pragma unroll
          for (int tl = 0; tl < NT; ++tl) store_T(S_H1 + c * H * TL, NT * wave + tl, h1[tl], j, g);
        } else {
#pragma unroll
          for (int tl = 0; tl < NT; ++tl) {
            f32x4 h1 = *reinterpret_cast<const f32x4*>(b1s + 16 * tl);
#pragma unroll
            for (int q = 0; q < XK; ++q) h1 = mfma16(w1[tl][q], x[c][q], h1);
#pragma unroll
            for (int r = 0; r < 4; ++r) h1[r] = act_fn<ACT>(h1[r]);
            store_T(S_H1 + c * H * TL, NT * wave + tl, h1, j, g);
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        f32x4 h2[NT];
        if constexpr (LN) {
          float ln_mean, ln_rstd;
          rw_ln_combine<H, VW_WAVES>(S_ST + c * 32, CT * 32, j, ln_mean, ln_rstd);
          rw_layer2<H, NT, true>(S_H1 + c * H * TL, b2s, j, g, w2, h2, ln_mean, ln_rstd);
#pragma unroll
          for (int tl = 0; tl < NT; ++tl)
#pragma unroll
            for (int r = 0; r < 4; ++r) h2[tl][r] = act_fn<ACT>(h2[tl][r]);   // (the second application follows below)
        } else {
          rw_layer2<H, NT>(S_H1 + c * H * TL, b2s, j, g, w2, h2);
        }
        float v = 0.0f;
#pragma unroll
        for (int tl = 0; tl < NT; ++tl)
#pragma unroll
          for (int r = 0; r < 4; ++r) v = fmaf(w3[tl][r], act_fn<ACT>(h2[tl][r]), v);
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (g == 0) vp[(wave * CT + c) * 16 + j] = v;
      }
      __syncthreads();
      if (wave == 0 && g < CT) {                                       // (g < CT: the lane's own column tile is g)
        float v = b3;
#pragma unroll
        for (int w = 0; w < VW_WAVES; ++w) v += vp[(w * CT + g) * 16 + j];
        if (ph == 0) {
          if (ok_o) a.values[cell_o] = v;
        } else {
          if (ok_o && marker != 0.0f) a.rewards[cell_o] += a.discount * v;
          if (last) a.boot[n_o] = v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------- host side shared by the two translation units
static inline bool wide_shape_ok(int head, int D, int H, int A, int act) {
  return (H == 128 || H == 256) && D >= 2 && D <= 32 && A >= HEADS[head].a_min && A <= HEADS[head].a_max &&
         (act == TRL_ACT_TANH || act == TRL_ACT_RELU);
}
// f(H) with the width as an integral constant; the caller has checked that H is 128 or 256
template <class F> static int with_width(int H, F&& f) { return H == 128 ? f(head_ic<128>{}) : f(head_ic<256>{}); }
// one workgroup per CU is resident (two 256-register waves per SIMD): a grid of that many walks the rounds
static inline int value_pass_wide_grid(const RolloutDev& d, int H) {
  const int64_t n_tiles = ((int64_t)d.n_steps * d.N + 15) / 16;
  const int64_t rounds = (n_tiles + 512 / H - 1) / (512 / H);
  return (int)(rounds < 256 ? rounds : 256);
}
// defined in k_rollout_wide.hip: the plain rollout kernel of a head alone and the plain value pass alone -- the plain halves of
// a pair whose other net carries a LayerNorm (k_rollout_wide_ln.hip), launched from there so that every plain instantiation
// has ONE definition
int rollout_wide_policy(const RolloutDev& d, int head, int H, int act, hipStream_t s);
int rollout_wide_value(const RolloutDev& d, int H, int act, hipStream_t s);
