// The fused PPO / A2C / REINFORCE minibatch gradient for plain two-layer networks of width H = 128: ppo_grad_wide_kernel and
// its entry points (trl_ppo_wide_*).  Same contract as the 64-wide kernel of trl_ppo_wave.h -- the launch descriptor
// (trl_ppo_batch_t -> PpoDev), the fused gather through row_idx, one partial row per workgroup in the flat parameter order
// [W1 b1 W2 b2 W3 b3 (logstd)], the scalar rows of the head -- so that the folds of k_ppo.hip take its rows as they are
// (trl_ppo_wide_reduce_*).  What is new is how the work is split.
//
// The 64-wide kernel gives every wave a whole 16-sample tile and shares W2 / W2^T through LDS.  At H = 128 the three H x H
// objects of a pass (W2 as the forward operand, W2^T as the backward operand, the dW2 accumulators) are 192 KB: more than the
// LDS, less than the register files of a CU.  So the pass is WEIGHT-STATIONARY, split like rollout_wide_kernel:
//   * 4 waves, one per SIMD, one workgroup per CU (__launch_bounds__(256, 1): 512 registers per lane).  Wave w owns hidden
//     rows [32 w, 32 w + 32) of BOTH layers -- two row tiles of 16 -- for every sample the workgroup visits.  Loaded once per
//     launch, as MFMA A operands (v_mfma_f32_16x16x4_f32, Z^T = W X^T): its rows of W1 (10 / 16 registers), of W2 (64), its
//     columns of W2 as rows of W2^T (64), its columns of W3 twice (head and dH2: 8 + 8).  Resident across all tiles: the
//     accumulators of its rows of dW2 (64), dW1 (8 / 16), its columns of dW3 (8) and the per-lane bias partials.
//   * a workgroup walks tiles of S = 32 samples (two 16-sample column tiles per barrier phase).  Activations cross waves
//     through LDS as [128][S] tiles with rows of S + 4 floats: H1^T (B operand of layer 2 for every wave, B operand of dW2),
//     dZ2^T (B operand of dH1^T = W2^T dZ2^T for every wave, A operand of the owner's dW2); H2^T and dZ1^T are read by their
//     owner only (dW3 / dW1 operands: the transposes that put the sample index on the K axis).
//     S: a tile costs 5 barriers (4 in the value pass) whatever S is, so S = 64 halves the barriers per sample; but its four
//     tensors are 4 x 128 x 68 x 4 B = 139 KB, which with the head exchange (16 KB) does not fit 160 KB unless tensors alias,
//     and it doubles the per-tile register state (h1, h2, dz, inputs: 2 x 48) next to ~300 launch-resident registers.  S = 32:
//     74 KB + 8 KB, 5 barriers per 32 samples next to ~500 MFMAs (16 k cycles) per wave.
//   * per tile: (1) layer 1, act, store H1^T | barrier | (2) layer 2, act, store H2^T, head partial over the wave's 32 features
//     into headp[4][16][S] | barrier | (3) the loss half of column tile c in wave c -- head = b3 + the four partials in
//     ascending wave order, then the per-sample arithmetic of the 64-wide kernel for the same head, d head into dout^T[16][S],
//     statistics -- | barrier | (4) dZ2^T = (W3^T d head) act'(H2), dW3 | barrier | (5) dZ1^T = (W2^T dZ2^T) act'(H1), dW2 +=
//     dZ2^T H1, (6) dW1 += dZ1^T X | barrier.  The value pass has a 1-wide head: per-lane dot + two cross-lane adds, the
//     waves' partials summed in ascending order by everyone, loss per lane (no phase-3 barrier), dW3 as per-lane FMAs.
//   * LDS operand slices are read once for both row tiles of the wave and requested one slice pair ahead of the MFMAs that
//     use them; the first layer's operand of the NEXT tile is loaded mid-tile, the other cells of a tile at its top, two
//     barriers or more ahead of their use.
//   * epilogue: every gradient element lives in exactly one wave, so there is no cross-wave fold of the weight gradients --
//     each wave stores its rows of dW1 / dW2, its columns of dW3 and its bias sums (row_sum16) straight into the partial row;
//     only dlogstd (wave 0 + wave 1) is added through LDS.  Every float of [0, p_stride) is stored exactly once.
#include "trl_ppo_wave.h"
#include "trl_ppo_wide.h"

#define PW_WAVES 4
#define PW_THREADS (64 * PW_WAVES)
#define PW_NT 2                                     // row tiles of 16 per wave
#define PW_NS (PPO_WIDE_H / 16)                     // 16-feature slices of a layer
#define PW_CT (PPO_WIDE_S / 16)                     // column tiles of a sample tile
#define PW_LD (PPO_WIDE_S + 4)                      // row stride of the [128][S] tiles: lane groups 4 rows apart are 16 banks apart

struct PwShape {
  static constexpr int H = PPO_WIDE_H, T = H * PW_LD;
  // b1 | b2 | H1^T | H2^T | dZ2^T | dZ1^T | headp [4][16][S] | dout^T [16][LD] | dlogstd [2][16]
  static constexpr int O_B1 = 0, O_B2 = H, O_H1 = 2 * H, O_H2 = O_H1 + T, O_DZ2 = O_H2 + T, O_DZ1 = O_DZ2 + T, O_HP = O_DZ1 + T,
                       O_DO = O_HP + PW_WAVES * 16 * PPO_WIDE_S, O_XL = O_DO + 16 * PW_LD, LDS_FLOATS = O_XL + 32;
};
static_assert(PwShape::LDS_FLOATS * sizeof(float) <= 160 * 1024, "the tiles fit the LDS");

// out[tl] (+)= sum over the 128 rows k of T: w[tl][k] * T[k][16 c + j] -- the wave's two row tiles over column tile c of a
// [128][S] tile, as B operands (k index of step (sl, r) is row 16 sl + 4 g + r).  Two accumulation chains per row tile; a
// pair of slices is requested before the MFMAs of the previous pair (the fence keeps the reads from sinking to their use).
__device__ __forceinline__ f32x4 pw_ldb(const float* __restrict__ T, int sl, int c, int j, int g) {
  f32x4 t;
#pragma unroll
  for (int r = 0; r < 4; ++r) t[r] = T[(16 * sl + 4 * g + r) * PW_LD + 16 * c + j];
  return t;
}
__device__ __forceinline__ void pw_rows_gemm(const float* __restrict__ T, int c, int j, int g, const float (&w)[PW_NT][PW_NS][4],
                                             const f32x4 (&init)[PW_NT], f32x4 (&out)[PW_NT]) {
  f32x4 acc[PW_NT][2];
#pragma unroll
  for (int tl = 0; tl < PW_NT; ++tl) { acc[tl][0] = init[tl]; acc[tl][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  f32x4 b0 = pw_ldb(T, 0, c, j, g), b1 = pw_ldb(T, 1, c, j, g);
#pragma unroll
  for (int sl = 0; sl < PW_NS; sl += 2) {
    f32x4 n0 = b0, n1 = b1;
    if (sl + 2 < PW_NS) { n0 = pw_ldb(T, sl + 2, c, j, g); n1 = pw_ldb(T, sl + 3, c, j, g); }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int tl = 0; tl < PW_NT; ++tl) {
        acc[tl][0] = mfma16(w[tl][sl][r], b0[r], acc[tl][0]);
        acc[tl][1] = mfma16(w[tl][sl + 1][r], b1[r], acc[tl][1]);
      }
    __builtin_amdgcn_sched_barrier(0);
    b0 = n0; b1 = n1;
  }
#pragma unroll
  for (int tl = 0; tl < PW_NT; ++tl) out[tl] = acc[tl][0] + acc[tl][1];
}

// TILE: capacity of the input tile (17 or 32 features); the actual dims come with the launch (a.D, a.A).  One network pass
// of a workgroup: IS_PF the policy's with head HEAD, else the value function's.  Tiles wg_in_net, wg_in_net + n_wg_net, ...
template <int TILE, int HEAD, int ACT, bool IS_PF, bool CONTIG>
__device__ void ppo_wide_pass(const PpoDev& a, float* lds, int wg_in_net, int n_wg_net) {
  static_assert(TILE == 17 || TILE == 32, "input tiles of 17 or 32 features");
  using S = PwShape;
  constexpr int H = S::H, NT = PW_NT, NS = PW_NS, CT = PW_CT, LD = PW_LD, XK = TILE > 17 ? 8 : 5;
  constexpr bool WIDE = TILE > 17, CAT = IS_PF && HEAD == HEAD_CAT, SDP = IS_PF && HEAD == HEAD_SD, GAUSS = IS_PF && HEAD == HEAD_GAUSS;
  const int Dr = a.D, O = IS_PF ? a.A : 1, OH = SDP ? 2 * O : O;
  const int F_W1 = 0, F_B1 = H * Dr, F_W2 = F_B1 + H, F_B2 = F_W2 + H * H, F_W3 = F_B2 + H, F_B3 = F_W3 + OH * H, F_LS = F_B3 + OH,
            F_END = GAUSS ? F_LS + O : F_LS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4, i = j;
  const float* gp = IS_PF ? a.pf_params : a.vf_params;
  // tile row o of the head (lane (j, g) holds rows 4 g + r in the C layout): does it exist, and which row of W3 / b3 is it
  // (SD: rows 0..7 are the means, 8..15 the log_stds, whatever a.A is)
  auto has_row = [&](int o) -> bool { return SDP ? (o & 7) < O : o < O; };
  auto w3_row = [&](int o) -> int { return SDP ? (o < 8 ? o : O + (o - 8)) : o; };
  float* H1S = lds + S::O_H1;
  float* H2S = lds + S::O_H2;
  float* DZ2S = lds + S::O_DZ2;
  float* DZ1S = lds + S::O_DZ1;
  float* headp = lds + S::O_HP;
  float* DOS = lds + S::O_DO;

  const int B = a.rows_mb * a.N;
  const int n_tiles = (B + PPO_WIDE_S - 1) / PPO_WIDE_S;
  const int tpr = CONTIG ? a.N >> 4 : 1;            // CONTIG (N % 16 == 0): column tiles per time row
  // the ring cell of sample j of column tile T (16 T + j of the minibatch) and whether the sample exists; a missing sample
  // reads the minibatch's first cell (rows outside the minibatch are never touched) and is masked where it is consumed
  auto cell_of = [&](int T, bool& ok) -> int64_t {
    int r, e;
    if constexpr (CONTIG) {                          // wave-uniform row: a scalar load of the index
      const int Tu = __builtin_amdgcn_readfirstlane(T);
      r = Tu / tpr; e = 16 * (Tu - r * tpr) + j;
      ok = r < a.rows_mb;
    } else {
      const int s = 16 * T + j;
      ok = s < B;
      r = s / a.N; e = s - r * a.N;
    }
    if (!ok) { r = 0; e = 0; }
    const int64_t ridx = a.row_idx ? a.row_idx[r] : (int64_t)r;
    return ridx * a.N + e;
  };
  bool fv[4], fv2[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { fv[q] = 4 * g + q < Dr; fv2[q] = WIDE && 16 + 4 * g + q < Dr; }
  const bool f16 = !WIDE && Dr > 16, jv = i < Dr, jv2 = WIDE && 16 + i < Dr;
  // raw operand of layer 1 for column tile T: features 4 g + q, then 16 + 4 g + q (wide tile) or feature 16 (narrow tile)
  auto load_x = [&](int64_t cell, float (&x)[XK]) {
    const float* ob = a.obs + cell * Dr;
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = ob[fv[q] ? 4 * g + q : 0];
    if constexpr (WIDE) {
#pragma unroll
      for (int q = 0; q < 4; ++q) x[4 + q] = ob[fv2[q] ? 16 + 4 * g + q : 0];
    } else {
      x[4] = ob[f16 ? 16 : 0];
    }
  };

  // ---- the first tile's cells, then the set-up: biases to LDS, the wave's weight rows to registers ----
  int tile = wg_in_net;
  float xq[CT][XK];
  bool okq[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) load_x(cell_of(tile * CT + c, okq[c]), xq[c]);
  for (int e = tid; e < H; e += PW_THREADS) { lds[S::O_B1 + e] = gp[F_B1 + e]; lds[S::O_B2 + e] = gp[F_B2 + e]; }
  float w1[NT][XK], w2[NT][NS][4], w2t[NT][NS][4], w3a[NT][4], w3t[NT][4];
#pragma unroll
  for (int tl = 0; tl < NT; ++tl) {
    const int row = 16 * (NT * wave + tl) + i;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      w1[tl][q] = fv[q] ? gp[F_W1 + row * Dr + (fv[q] ? 4 * g + q : 0)] : 0.0f;
      if constexpr (WIDE) w1[tl][4 + q] = fv2[q] ? gp[F_W1 + row * Dr + (fv2[q] ? 16 + 4 * g + q : 0)] : 0.0f;
    }
    if constexpr (!WIDE) w1[tl][4] = (g == 0 && f16) ? gp[F_W1 + row * Dr + (f16 ? 16 : 0)] : 0.0f;
#pragma unroll
    for (int sl = 0; sl < NS; ++sl)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        w2[tl][sl][r] = gp[F_W2 + row * H + 16 * sl + 4 * g + r];              // forward: W2[own row][k]
        w2t[tl][sl][r] = gp[F_W2 + (16 * sl + 4 * g + r) * H + row];           // backward: W2[k][own column]
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = 4 * g + r;
      if constexpr (IS_PF) {
        w3a[tl][r] = has_row(i) ? gp[F_W3 + (has_row(i) ? w3_row(i) : 0) * H + 16 * (NT * wave + tl) + 4 * g + r] : 0.0f;   // head: W3[row i][k]
        w3t[tl][r] = has_row(o) ? gp[F_W3 + (has_row(o) ? w3_row(o) : 0) * H + row] : 0.0f;                               // dH2: W3[row o][own f]
      } else {
        w3a[tl][r] = gp[F_W3 + 16 * (NT * wave + tl) + 4 * g + r];            // the lane's own head weights (C layout)
        w3t[tl][r] = 0.0f;
      }
    }
  }
  // per-lane constants of the lane's 4 head rows o = 4 g + r (policy); the value head's bias
  float b3v[4], lsv[4], ivv[4], lspass[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int o = 4 * g + r;
    b3v[r] = (IS_PF && has_row(o)) ? gp[F_B3 + (has_row(o) ? w3_row(o) : 0)] : 0.0f;
    const float raw = (GAUSS && o < O) ? gp[F_LS + (o < O ? o : 0)] : 0.0f;
    lsv[r] = fminf(fmaxf(raw, -20.0f), 2.0f);                   // continuous_policy.py:8-9,185
    ivv[r] = __expf(-2.0f * lsv[r]);
    lspass[r] = (raw >= -20.0f && raw <= 2.0f) ? 1.0f : 0.0f;   // clamp passes gradient inside [-20, 2]
  }
  const float vb3 = IS_PF ? 0.0f : gp[F_B3];
  // advantage normalisation constants (ppo.py:141-147): mean, unbiased std
  const double adv_s1 = IS_PF ? a.adv_raw[0] : 0.0, adv_s2 = IS_PF ? a.adv_raw[1] : 0.0;
  const double ng = a.n_global;
  const double adv_var = (adv_s2 - adv_s1 * adv_s1 / ng) / (ng - 1.0);
  const float adv_mu = (float)(adv_s1 / ng);
  const float adv_rstd = 1.0f / ((float)sqrt(fmax(adv_var, 0.0)) + 1e-5f);
  const float inv_b = (float)(1.0 / ng);

  // ---- gradient accumulators: the wave's rows of dW2 / dW1, its columns of dW3, per-lane (own sample) bias partials ----
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 gW2[NT][NS], gW1[NT], gW1b[NT], gW3[NT], gb1[NT], gb2[NT], gW1c[NT];
#pragma unroll
  for (int tl = 0; tl < NT; ++tl) {
    gW1[tl] = gW1b[tl] = gW3[tl] = gb1[tl] = gb2[tl] = gW1c[tl] = zero4;
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) gW2[tl][sl] = zero4;
  }
  float db3[4] = {0.f, 0.f, 0.f, 0.f}, dls[4] = {0.f, 0.f, 0.f, 0.f}, stv[7], ent_sum = 0.0f, sd_cnt = 0.0f;
  float sdst[8] = {0.0f, 0.0f, -INFINITY, -INFINITY, 0.0f, 0.0f, -INFINITY, -INFINITY};
#pragma unroll
  for (int k = 0; k < 7; ++k) stv[k] = (k >= 2 && k <= 5) ? -INFINITY : 0.0f;
  const float* b1s = lds + S::O_B1 + 16 * NT * wave + 4 * g;
  const float* b2s = lds + S::O_B2 + 16 * NT * wave + 4 * g;
  __syncthreads();

  for (; tile < n_tiles; tile += n_wg_net) {
    // ---- this tile's cells: the prefetched layer-1 operand, and the loads whose use is two barriers or more away ----
    float xb[CT][XK], x16[CT], xt[CT][4], xt2[CT][4];
    bool ok[CT];
    float rets[CT], vold[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      ok[c] = okq[c];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        xb[c][q] = (ok[c] && fv[q]) ? xq[c][q] : 0.0f;
        if constexpr (WIDE) xb[c][4 + q] = (ok[c] && fv2[q]) ? xq[c][4 + q] : 0.0f;
      }
      x16[c] = 0.0f;
      if constexpr (!WIDE) { x16[c] = (ok[c] && f16) ? xq[c][4] : 0.0f; xb[c][4] = g == 0 ? x16[c] : 0.0f; }
      bool okc;
      const int64_t cell = cell_of(tile * CT + c, okc);
      // X[sample 4 g + q][feature j] (and 16 + j): B operand of the dW1 GEMM; the cell is sample lane 4 g + q's
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t pq = __shfl(cell, 4 * g + q, 64);
        const bool sv = CONTIG ? okc : (16 * (tile * CT + c) + 4 * g + q < B);
        const float v0 = a.obs[pq * Dr + (jv ? i : 0)];
        xt[c][q] = (sv && jv) ? v0 : 0.0f;
        xt2[c][q] = 0.0f;
        if constexpr (WIDE) { const float v1 = a.obs[pq * Dr + (jv2 ? 16 + i : 0)]; xt2[c][q] = (sv && jv2) ? v1 : 0.0f; }
      }
      rets[c] = vold[c] = 0.0f;
      if constexpr (!IS_PF) {
        rets[c] = a.rets[cell];
        vold[c] = a.clipped_value_loss ? a.old_values[cell] : 0.0f;
      }
    }
    // the loss inputs of column tile `wave` (policy; waves 0 .. CT - 1 run the loss half)
    float lin[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool lvalid = false;
    if constexpr (IS_PF) {
      if (wave < CT) {
        const int64_t cell = cell_of(tile * CT + wave, lvalid);
        if constexpr (CAT) lin[0] = a.acts[cell];
        else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = SDP ? 4 * (g & 1) + r : 4 * g + r;          // SD: lanes g, g ^ 2 hold the same action
            lin[r] = a.acts[cell * O + (o < O ? o : 0)];
          }
        }
        lin[4] = a.advs[cell];
        lin[5] = a.old_logp ? a.old_logp[cell] : 0.0f;
      }
    }

    // ---- (1) layer 1 of the wave's rows, both column tiles ----
    f32x4 h1[NT][CT], h2[NT][CT];
#pragma unroll
    for (int tl = 0; tl < NT; ++tl)
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        f32x4 z = lds4(b1s + 16 * tl);
#pragma unroll
        for (int q = 0; q < XK; ++q) z = mfma16(w1[tl][q], xb[c][q], z);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          h1[tl][c][r] = act_fn<ACT>(z[r]);
          H1S[(16 * (NT * wave + tl) + 4 * g + r) * LD + 16 * c + j] = h1[tl][c][r];
        }
      }
    __syncthreads();
    // ---- (2) layer 2, head partial over the wave's 32 features ----
    f32x4 b2i[NT];
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) b2i[tl] = lds4(b2s + 16 * tl);
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      f32x4 z[NT];
      pw_rows_gemm(H1S, c, j, g, w2, b2i, z);
#pragma unroll
      for (int tl = 0; tl < NT; ++tl)
#pragma unroll
        for (int r = 0; r < 4; ++r) h2[tl][c][r] = act_fn<ACT>(z[tl][r]);
      if constexpr (IS_PF) {
        f32x4 hp = zero4;
#pragma unroll
        for (int tl = 0; tl < NT; ++tl)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            hp = mfma16(w3a[tl][r], h2[tl][c][r], hp);
            H2S[(16 * (NT * wave + tl) + 4 * g + r) * LD + 16 * c + j] = h2[tl][c][r];      // H2^T[f][s] for the owner's dW3
          }
#pragma unroll
        for (int r = 0; r < 4; ++r) headp[(wave * 16 + 4 * g + r) * PPO_WIDE_S + 16 * c + j] = hp[r];
      } else {
        float v = 0.0f;
#pragma unroll
        for (int tl = 0; tl < NT; ++tl)
#pragma unroll
          for (int r = 0; r < 4; ++r) v = fmaf(w3a[tl][r], h2[tl][c][r], v);
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (g == 0) headp[wave * PPO_WIDE_S + 16 * c + j] = v;
      }
    }
    // the next tile's layer-1 operand (its use is four barriers away)
    {
      const int nt = tile + n_wg_net;
#pragma unroll
      for (int c = 0; c < CT; ++c) load_x(cell_of(nt < n_tiles ? nt * CT + c : tile * CT + c, okq[c]), xq[c]);
    }
    __syncthreads();

    f32x4 dz2[NT][CT];
    if constexpr (IS_PF) {
      // ---- (3) the loss half of column tile c in wave c: lane (j, g) owns head rows 4 g + r of sample j ----
      if (wave < CT) {
        const bool valid = lvalid;
        float ho[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ho[r] = b3v[r];
#pragma unroll
          for (int w = 0; w < PW_WAVES; ++w) ho[r] += headp[(w * 16 + 4 * g + r) * PPO_WIDE_S + 16 * wave + j];
        }
        float zc[4] = {0.f, 0.f, 0.f, 0.f}, lp = 0.0f;
        float pk[4], lpk[4], ent = 0.0f;                               // CAT: p_k, log p_k of the lane's logits; the sample's entropy
        int ai = 0;                                                    // CAT: the stored action
        if constexpr (CAT) {
          // the sample's (up to) 8 logits sit in lanes (j, 0) and (j, 1): max, exp, sum in ascending k (lane g = 1 continues
          // lane g = 0's partial sum), p_k = e_k / S, log p_k = (l_k - m) - log S -- cat_losses_kernel's arithmetic
          float ek[4], m = -INFINITY;
#pragma unroll
          for (int r = 0; r < 4; ++r) m = (4 * g + r < O) ? fmaxf(m, ho[r]) : m;
          m = fmaxf(m, __shfl_xor(m, 16, 64));
          m = g < 2 ? m : 0.0f;
#pragma unroll
          for (int r = 0; r < 4; ++r) ek[r] = (4 * g + r < O) ? expf(ho[r] - m) : 0.0f;
          const float c_own = ((ek[0] + ek[1]) + ek[2]) + ek[3];
          const float c_lo = __shfl_xor(c_own, 16, 64);
          float Ssum = g == 1 ? (((c_lo + ek[0]) + ek[1]) + ek[2]) + ek[3] : c_own;
          const float S_hi = __shfl_xor(Ssum, 16, 64);
          Ssum = g == 0 ? S_hi : (g == 1 ? Ssum : 1.0f);
          const float logS = logf(Ssum);
          ai = min(max((int)lin[0], 0), O - 1);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool has = 4 * g + r < O;
            lpk[r] = has ? (ho[r] - m) - logS : 0.0f;
            pk[r] = ek[r] / Ssum;
            lp += (has && 4 * g + r == ai) ? lpk[r] : 0.0f;
            ent -= pk[r] * lpk[r];
          }
          lp += __shfl_xor(lp, 16, 64);
          ent += __shfl_xor(ent, 16, 64);
        } else if constexpr (SDP) {
          // lane (j, g < 2) holds means 4 g + r, lane (j, g + 2) the raw log_std of the same outputs; after the exchange all
          // four lane groups run gauss_sd_losses_kernel's per-element arithmetic and each keeps its own half of d(head)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool has = 4 * (g & 1) + r < O;
            const float mine = ho[r], oth = __shfl_xor(mine, 32, 64);
            const float mean = g < 2 ? mine : oth, raw = g < 2 ? oth : mine;
            lsv[r] = fminf(fmaxf(raw, -20.0f), 2.0f);
            ivv[r] = __expf(-2.0f * lsv[r]);
            lspass[r] = (raw >= -20.0f && raw <= 2.0f) ? 1.0f : 0.0f;
            const float t = gauss_logp_term((valid && has) ? lin[r] : 0.0f, has ? mean : 0.0f, ivv[r], lsv[r], a.tanh_action, zc[r]);
            lp += has ? t : 0.0f;
            ent += has ? SD_HALF_LOG_2PI_PLUS_HALF + lsv[r] : 0.0f;
            zc[r] = has ? zc[r] : 0.0f;
          }
          lp += __shfl_xor(lp, 16, 64);
          ent += __shfl_xor(ent, 16, 64);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {                                // branch-free: lanes without an output compute on zeros
            const bool has = 4 * g + r < O;
            const float t = gauss_logp_term((valid && has) ? lin[r] : 0.0f, has ? ho[r] : 0.0f, ivv[r], lsv[r], a.tanh_action, zc[r]);
            lp += has ? t : 0.0f;
            zc[r] = has ? zc[r] : 0.0f;
          }
          lp += __shfl_xor(lp, 16, 64);                                // outputs 0..3 (g = 0) + 4..7 (g = 1)
        }
        const float advn = valid ? (lin[4] - adv_mu) * adv_rstd : 0.0f;
        float ratio, s1, s2, g_lp;
        if (a.loss_mode == TRL_LOSS_A2C) {                            // L = -mean(log pi * adv) (a2c.py:69-70)
          ratio = 1.0f;
          s1 = s2 = lp * advn;
          g_lp = (valid && (SDP || g < 2)) ? -advn * inv_b : 0.0f;
        } else {                                                     // clipped surrogate (ppo.py:58-66)
          ratio = __expf(lp - lin[5]);
          s1 = ratio * advn;
          s2 = fminf(fmaxf(ratio, 1.0f - a.clip_para), 1.0f + a.clip_para) * advn;
          g_lp = (valid && (SDP || g < 2) && s1 <= s2) ? -advn * ratio * inv_b : 0.0f;
        }
        const float ce = a.entropy_coeff * inv_b;
        float dout[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (CAT) {
            // dout_k = g_lp (1[k = a] - p_k) + (entropy_coeff / n) p_k (log p_k + H): the entropy bonus -c H in the loss
            const bool own = valid && g < 2 && 4 * g + r < O;
            dout[r] = own ? g_lp * ((4 * g + r == ai ? 1.0f : 0.0f) - pk[r]) + ce * pk[r] * (lpk[r] + ent) : 0.0f;
          } else if constexpr (SDP) {
            // tile rows 4 g + r: d(loss)/d(mean) in lanes g < 2, d(loss)/d(raw log_std) in lanes g >= 2
            const bool own = valid && 4 * (g & 1) + r < O;
            const float dm = g_lp * zc[r] * ivv[r], dr = lspass[r] * (g_lp * (zc[r] * zc[r] * ivv[r] - 1.0f) - ce);
            dout[r] = own ? (g < 2 ? dm : dr) : 0.0f;
            if (own && g < 2) {                                        // log_std/*, std/* over the elements (ppo.py:83-86, a2c.py:96-101)
              const float x = lsv[r], ex = expf(x);
              sdst[0] += x; sdst[1] = fmaf(x, x, sdst[1]); sdst[2] = fmaxf(sdst[2], x); sdst[3] = fmaxf(sdst[3], -x);
              sdst[4] += ex; sdst[5] = fmaf(ex, ex, sdst[5]); sdst[6] = fmaxf(sdst[6], ex); sdst[7] = fmaxf(sdst[7], -ex);
            }
          } else {
            const bool own = valid && g < 2 && 4 * g + r < O;
            dout[r] = own ? g_lp * zc[r] * ivv[r] : 0.0f;
            dls[r] += own ? lspass[r] * (g_lp * (zc[r] * zc[r] * ivv[r] - 1.0f) - ce) : 0.0f;
          }
          DOS[(4 * g + r) * LD + 16 * wave + j] = dout[r];             // dout^T[tile row][s]
        }
        if (valid && g == 0) {
          if constexpr (CAT || SDP) ent_sum += ent;
          if constexpr (SDP) sd_cnt += 1.0f;
          stv[0] += lp; stv[1] = fmaf(lp, lp, stv[1]); stv[6] -= fminf(s1, s2);
          stv[2] = fmaxf(stv[2], lp); stv[3] = fmaxf(stv[3], -lp);
          stv[4] = fmaxf(stv[4], ratio); stv[5] = fmaxf(stv[5], -ratio);
        }
      }
      __syncthreads();
      // ---- (4) dZ2^T = (W3^T d head) act'(H2) for the wave's rows; dW3[o][own f] += sum_s dout[s][o] H2[s][f] ----
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        f32x4 dC;                                                      // d head in the C layout: rows 4 g + r, sample j
#pragma unroll
        for (int r = 0; r < 4; ++r) dC[r] = DOS[(4 * g + r) * LD + 16 * c + j];
        const f32x4 dA = lds4(DOS + i * LD + 16 * c + 4 * g);          // as the A operand: row i, samples 4 g + q
        f32x4 hb[NT];
#pragma unroll
        for (int tl = 0; tl < NT; ++tl) hb[tl] = lds4(H2S + (16 * (NT * wave + tl) + j) * LD + 16 * c + 4 * g);
#pragma unroll
        for (int tl = 0; tl < NT; ++tl) {
          f32x4 d = zero4;
#pragma unroll
          for (int r = 0; r < 4; ++r) d = mfma16(w3t[tl][r], dC[r], d);
          dz2[tl][c] = d;
#pragma unroll
          for (int q = 0; q < 4; ++q) gW3[tl] = mfma16(dA[q], hb[tl][q], gW3[tl]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) db3[r] += dC[r];
      }
    } else {
      // ---- (3 + 4) the value head: v = b3 + the four partials in ascending order; loss per lane; dW3 as per-lane FMAs ----
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        float v = vb3;
#pragma unroll
        for (int w = 0; w < PW_WAVES; ++w) v += headp[w * PPO_WIDE_S + 16 * c + j];
        const float R = rets[c];
        float dv, l;
        if (a.clipped_value_loss) {                                  // ppo.py:104-111
          const float vo = vold[c];
          const float dc = v - vo;
          const float vc = vo + fminf(fmaxf(dc, -a.clip_para), a.clip_para);
          const float l1 = (v - R) * (v - R), l2 = (vc - R) * (vc - R);
          const float wa = l1 > l2 ? 1.0f : (l1 == l2 ? 0.5f : 0.0f), wb_ = 1.0f - wa;
          const float pass = (dc >= -a.clip_para && dc <= a.clip_para) ? 1.0f : 0.0f;
          l = 0.5f * fmaxf(l1, l2);
          dv = inv_b * (wa * (v - R) + wb_ * pass * (vc - R));
        } else {                                                     // nn.MSELoss, a2c.py:43
          l = (v - R) * (v - R);
          dv = 2.0f * (v - R) * inv_b;
        }
        dv = ok[c] ? dv : 0.0f;
        if (ok[c] && g == 0 && wave == 0) {
          stv[6] += l; db3[0] += dv;
          stv[0] += v; stv[1] = fmaf(v, v, stv[1]); stv[2] = fmaxf(stv[2], v); stv[3] = fmaxf(stv[3], -v);   // v_pred/*
        }
#pragma unroll
        for (int tl = 0; tl < NT; ++tl)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            dz2[tl][c][r] = dv * w3a[tl][r];
            gW3[tl][r] = fmaf(dv, h2[tl][c][r], gW3[tl][r]);           // per-lane dW3[f] partial (own sample)
          }
      }
    }
#pragma unroll
    for (int tl = 0; tl < NT; ++tl)
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          dz2[tl][c][r] *= act_grad<ACT>(h2[tl][c][r]);
          gb2[tl][r] += dz2[tl][c][r];
          DZ2S[(16 * (NT * wave + tl) + 4 * g + r) * LD + 16 * c + j] = dz2[tl][c][r];       // dZ2^T[f][s]
        }
    __syncthreads();
    // ---- (5) dZ1^T = (W2^T dZ2^T) act'(H1) for the wave's rows ----
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      f32x4 d[NT];
      const f32x4 zi[NT] = {zero4, zero4};
      pw_rows_gemm(DZ2S, c, j, g, w2t, zi, d);
#pragma unroll
      for (int tl = 0; tl < NT; ++tl)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float dz1 = d[tl][r] * act_grad<ACT>(h1[tl][c][r]);
          gb1[tl][r] += dz1;
          if constexpr (!WIDE) gW1c[tl][r] = fmaf(dz1, x16[c], gW1c[tl][r]);
          DZ1S[(16 * (NT * wave + tl) + 4 * g + r) * LD + 16 * c + j] = dz1;                 // dZ1^T[f][s] for the owner's dW1
        }
    }
    // ---- dW2[own f2][f1] += sum_s dZ2[s][f2] H1[s][f1]  (K step q is sample 16 c + 4 g + q; an H1 slice feeds both row tiles) ----
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      f32x4 za[NT];
#pragma unroll
      for (int tl = 0; tl < NT; ++tl) za[tl] = lds4(DZ2S + (16 * (NT * wave + tl) + i) * LD + 16 * c + 4 * g);
      f32x4 hb = lds4(H1S + j * LD + 16 * c + 4 * g);
#pragma unroll
      for (int sl = 0; sl < NS; ++sl) {
        const f32x4 hc = hb;
        if (sl + 1 < NS) hb = lds4(H1S + (16 * (sl + 1) + j) * LD + 16 * c + 4 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int tl = 0; tl < NT; ++tl) gW2[tl][sl] = mfma16(za[tl][q], hc[q], gW2[tl][sl]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // ---- (6) dW1[own f1][k] += sum_s dZ1[s][f1] X[s][k] ----
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int tl = 0; tl < NT; ++tl) {
        const f32x4 za = lds4(DZ1S + (16 * (NT * wave + tl) + i) * LD + 16 * c + 4 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          gW1[tl] = mfma16(za[q], xt[c][q], gW1[tl]);
          if constexpr (WIDE) gW1b[tl] = mfma16(za[q], xt2[c][q], gW1b[tl]);
        }
      }
    __syncthreads();                                                 // the next tile's stores into H1^T / headp / dout^T
  }

  // ---- epilogue: every wave stores what it owns; a workgroup without a tile stores its zeros ----
  float* prow = a.partial + (size_t)blockIdx.x * a.p_stride;
  float* xl = lds + S::O_XL;
#pragma unroll
  for (int tl = 0; tl < NT; ++tl)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = 16 * (NT * wave + tl) + 4 * g + r;                 // accumulator rows are the wave's features ...
#pragma unroll
      for (int sl = 0; sl < NS; ++sl) prow[F_W2 + f * H + 16 * sl + j] = gW2[tl][sl][r];
      if (jv) prow[F_W1 + f * Dr + j] = gW1[tl][r];
      if (jv2) prow[F_W1 + f * Dr + 16 + j] = gW1b[tl][r];
      const float s1 = row_sum16(gb1[tl][r]), s2 = row_sum16(gb2[tl][r]), sc = row_sum16(gW1c[tl][r]);
      const float s3 = IS_PF ? 0.0f : row_sum16(gW3[tl][r]);
      if (j == 0) {
        prow[F_B1 + f] = s1; prow[F_B2 + f] = s2;
        if (f16) prow[F_W1 + f * Dr + 16] = sc;
        if constexpr (!IS_PF) prow[F_W3 + f] = s3;
      }
      if constexpr (IS_PF) {                                           // ... those of dW3 are head rows, its columns the features
        const int o = 4 * g + r;
        if (has_row(o)) prow[F_W3 + w3_row(o) * H + 16 * (NT * wave + tl) + j] = gW3[tl][r];
      }
    }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int o = 4 * g + r;
    const float b3 = row_sum16(db3[r]), dl = row_sum16(dls[r]);
    if (wave == 0 && j == 0) {
      if constexpr (IS_PF) { if (has_row(o)) prow[F_B3 + w3_row(o)] = b3; }
      else if (o == 0) prow[F_B3] = b3;
    }
    if (GAUSS && wave < CT && j == 0) xl[16 * wave + o] = dl;
  }
  __syncthreads();
  if constexpr (GAUSS) {
    if (tid < O) {                                                     // dlogstd: wave 0's samples + wave 1's
      float acc = xl[tid];
#pragma unroll
      for (int w = 1; w < CT; ++w) acc += xl[16 * w + tid];
      prow[F_LS + tid] = acc;
    }
  }
  for (int e = F_END + tid; e < a.p_stride; e += PW_THREADS) prow[e] = 0.0f;   // the row's tail

  // ---- scalar statistics (the rows of the 64-wide kernel; waves without a loss half hold the identities) ----
  double* sred = reinterpret_cast<double*>(lds);
  const int wg = blockIdx.x;
  {
    const bool own = g == 0;
    const double v0 = wave_sum(own ? (double)stv[0] : 0.0), v1 = wave_sum(own ? (double)stv[1] : 0.0),
                 v6 = wave_sum(own ? (double)stv[6] : 0.0);
    const float v2 = wave_max(own ? stv[2] : -INFINITY), v3 = wave_max(own ? stv[3] : -INFINITY),
                v4 = wave_max(own ? stv[4] : -INFINITY), v5 = wave_max(own ? stv[5] : -INFINITY);
    double v7 = 0.0;                                   // CAT / SD: the entropy sum rides in the row's eighth column
    if constexpr (CAT || SDP) v7 = wave_sum(own ? (double)ent_sum : 0.0);
    if (lane == 0) {
      double* p = sred + wave * 8;
      p[0] = v0; p[1] = v1; p[2] = v2; p[3] = v3; p[4] = v4; p[5] = v5; p[6] = v6; p[7] = v7;
    }
    if constexpr (SDP) {
      double e[9];
#pragma unroll
      for (int k = 0; k < 8; ++k) e[k] = (k & 2) ? (double)wave_max(sdst[k]) : wave_sum((double)sdst[k]);
      e[8] = wave_sum((double)sd_cnt);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < SD_SCAL; ++k) sred[PW_WAVES * 8 + wave * SD_SCAL + k] = k < 9 ? e[k < 9 ? k : 0] : 0.0;
      }
    }
  }
  __syncthreads();
  if (tid < 8) {
    double r = sred[tid];
    for (int w = 1; w < PW_WAVES; ++w) {
      const double o = sred[w * 8 + tid];
      r = (tid >= 2 && tid <= 5) ? fmax(r, o) : r + o;
    }
    a.scal_partial[(size_t)wg * 8 + tid] = r;
  }
  if constexpr (SDP) {                                  // second block of scalar rows, behind the n_wg x 8 of every head
    if (tid >= 64 && tid < 64 + SD_SCAL) {
      const int k = tid - 64;
      double r = sred[PW_WAVES * 8 + k];
      for (int w = 1; w < PW_WAVES; ++w) {
        const double o = sred[PW_WAVES * 8 + w * SD_SCAL + k];
        r = (k < 8 && (k & 2)) ? fmax(r, o) : r + o;
      }
      a.scal_partial[(size_t)a.n_wg * 8 + (size_t)wg * SD_SCAL + k] = r;
    }
  }
}

// workgroups [0, n_pf) run the policy, [n_pf, n_wg) the value function (whose pass does not depend on the head)
template <int TILE_D, int HEAD, int ACT, bool CONTIG>
__global__ __launch_bounds__(PW_THREADS, 1) void ppo_grad_wide_kernel(PpoDev a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if ((int)blockIdx.x < a.n_pf) ppo_wide_pass<TILE_D, HEAD, ACT, true, CONTIG>(a, lds, blockIdx.x, a.n_pf);
  else                          ppo_wide_pass<TILE_D, HEAD_GAUSS, ACT, false, CONTIG>(a, lds, blockIdx.x - a.n_pf, a.n_wg - a.n_pf);
}

// ---------------------------------------------------------------- host side
template <int TILE_D, int HEAD, int ACT, bool CONTIG> static int launch_ppo_wide(const PpoDev& d, hipStream_t s) {
  const size_t lds = PwShape::LDS_FLOATS * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)ppo_grad_wide_kernel<TILE_D, HEAD, ACT, CONTIG>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { trl_set_error("ppo_wide_grad: hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
    attr_set = true;
  }
  hipLaunchKernelGGL((ppo_grad_wide_kernel<TILE_D, HEAD, ACT, CONTIG>), dim3(d.n_wg), dim3(PW_THREADS), lds, s, d);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

extern "C" int trl_ppo_wide_supported(int D, int H, int A, int act, int head) { return ppo_wide_ok(head, D, H, A, act) ? 1 : 0; }
extern "C" int trl_ppo_wide_tile(void) { return PPO_WIDE_S; }

extern "C" int trl_ppo_wide_partial_stride(int D, int H, int A, int head) {
  if (!ppo_wide_ok(head, D, H, A, TRL_ACT_TANH)) {
    trl_set_error("trl_ppo_wide_partial_stride: head %d, D=%d H=%d A=%d outside what the wide instantiations carry (H == 128, "
                  "2 <= D <= 32, A in the head's range)", head, D, H, A);
    return TRL_EUNSUPPORTED;
  }
  return ppo_ln_stride(D, H, A, head, 0);
}

// Policy / value split of a joint launch, in S-sample tiles: a workgroup runs whole tiles, a policy tile costs about 1.25
// value tiles (the head's 48 MFMAs of ~500, and the loss half in two of the four waves); the split that minimises the
// slower side's ceil(tiles / workgroups) * cost, ties to the more even one.
extern "C" int trl_ppo_wide_wg_split(int n_tiles, int n_wg) {
  if (n_wg < 2 || n_tiles <= 0) { trl_set_error("trl_ppo_wide_wg_split: need n_wg >= 2 and n_tiles > 0"); return TRL_EINVAL; }
  int best = n_wg / 2;
  double best_t = 1e300;
  for (int x = 1; x < n_wg; ++x) {
    const double t_pf = (double)((n_tiles + x - 1) / x) * 1.25, t_vf = (double)((n_tiles + (n_wg - x) - 1) / (n_wg - x));
    const double t = t_pf > t_vf ? t_pf : t_vf;
    if (t < best_t - 1e-9 || (t < best_t + 1e-9 && abs(2 * x - n_wg) < abs(2 * best - n_wg))) { best_t = t; best = x; }
  }
  return best;
}

// trl_ppo_minibatch_grad_f32 (and its per-head siblings) for a 128-wide pair.  Every n_wg_pf mode and every loss mode of
// trl_ppo_batch_t works; partial rows are trl_ppo_wide_partial_stride floats, the scalar rows the head's.
extern "C" int trl_ppo_wide_minibatch_grad_f32(const trl_ppo_batch_t* p, int head, void* stream) {
  if (!p) { trl_set_error("ppo_wide_grad: null descriptor"); return TRL_EINVAL; }
  if (!ppo_wide_ok(head, p->D, p->H, p->A, p->act)) {
    trl_set_error("ppo_wide_grad: head %d, shape D=%d H=%d A=%d act=%d not instantiated (H == 128, 2 <= D <= 32, A in the head's "
                  "range, Tanh / ReLU)", head, p->D, p->H, p->A, p->act);
    return TRL_EUNSUPPORTED;
  }
  PpoDev d;
  const int rc = ppo_dev_fill(p, head, false, d);
  if (rc != TRL_OK) return rc;
  d.p_stride = ppo_ln_stride(p->D, p->H, p->A, head, 0);
  hipStream_t s = (hipStream_t)stream;
  return with_head(head, [&](auto hd) {
    return with_tile_act(p->D, p->act, [&](auto tile, auto ac) {
      return (d.N % 16 == 0) ? launch_ppo_wide<decltype(tile)::value, decltype(hd)::value, decltype(ac)::value, true>(d, s)
                             : launch_ppo_wide<decltype(tile)::value, decltype(hd)::value, decltype(ac)::value, false>(d, s);
    });
  });
}
