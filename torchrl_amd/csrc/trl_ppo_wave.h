// The fused PPO / A2C minibatch gradient kernel (one wave per 16-sample tile, fp32 MFMA): ppo_wave_pass,
// ppo_grad_wave_kernel and their launch.  k_ppo.hip instantiates the plain networks, k_ppo_ln.hip the LN = true passes
// (a LayerNorm behind the first hidden layer, `add_ln` nets) -- see the notes at ppo_wave_pass.
#pragma once
#include <cstdlib>
#include "trl_common.h"
#include "trl_mlp.h"
#include "trl_head.h"
#include "trl_layernorm.h"

struct PpoDev {
  const float *obs, *acts, *advs, *rets, *old_values, *old_logp;
  const int64_t* row_idx;
  int rows_mb, N;
  const double* adv_raw;
  double n_global;
  const float *pf_params, *vf_params;
  float clip_para, entropy_coeff;
  int clipped_value_loss, tanh_action;
  int loss_mode;                              // TRL_LOSS_PPO_CLIP (ppo.py:41-91) or TRL_LOSS_A2C (a2c.py:45-75)
  float* partial;
  double* scal_partial;
  int n_wg, n_pf, p_stride;                  // workgroups [0, n_pf) run the policy, [n_pf, n_wg) the value net
  int D, A;                                  // actual input / action dims (runtime-dims instantiation of the kernel)
};

template <int D, int H, int A> struct PpoShape {
  static_assert(H == 64 && D > 16 && D <= 32 && A <= 8, "instantiated for 16 < D <= 32, H == 64, A <= 8");
  static constexpr int P_PF = MlpFlat<D, H, A>::P_PF, P_VF = MlpFlat<D, H, 1>::P_VF;
  static constexpr int P_STRIDE = ((P_PF > P_VF ? P_PF : P_VF) + 63) & ~63;   // floats per workgroup partial
};

// ================================================================ one wave = one tile
// Every wave walks whole 16-sample tiles on its own: all four 16-feature slices of a layer are
// independent accumulator chains in one instruction stream (the matrix pipe always has an MFMA that
// does not wait on the previous one), layer outputs chain as the next layer's B operand in
// registers, and the only LDS traffic is (a) the shared read-only W2 / W2^T operand copies and
// (b) the wave-private transposes that put the sample index on the K axis for the weight-gradient
// GEMMs.  No inter-wave synchronisation inside the tile loop.
//   per tile (policy):  L1 20 + L2 64 + head 16 + dH2 16 + dH1 64 + dW3 16 + dW2 64 + dW1 16 = 276 MFMA
//   per tile (value):   L1 20 + L2 64 +                      dH1 64 +          dW2 64 + dW1 16 = 228 MFMA
// (bias gradients, the 17th input column of dW1 and the 1-wide value head are per-lane FMAs).
#define WV_WAVES 4
// development aid (tools/time_grad.py): per-phase cycle totals of every wave 0 into the spare tail of `partial`
#ifdef TRL_EXP_CLK
#define WCLK_DECL long long clk_prev = clock64(); float clk_acc[24]; for (int q_ = 0; q_ < 24; ++q_) clk_acc[q_] = 0.f;
#define WCLK(ph) { __builtin_amdgcn_sched_barrier(0); const long long c_ = clock64(); clk_acc[ph] += (float)(c_ - clk_prev); clk_prev = c_; __builtin_amdgcn_sched_barrier(0); }
#else
#define WCLK_DECL
#define WCLK(ph)
#endif
#define WV_THREADS (64 * WV_WAVES)
#define LDT 20                                   // staging row stride: 16 samples + pad, rows 16-B aligned
#define LDW 68                                   // W2 operand copies: 64 + 4, ds_read_b128 rows

template <int D, int H, int A> struct WvShape {
  static_assert(H == 64 && (D == 17 || D == 32) && A <= 8, "instantiated for D == 17 / 32, H == 64, A <= 8");
  // shared: W2 (row-major) | W2^T | b1 | b2 ; per wave: H1^T | H2^T (later dZ1^T) | dZ2^T | dout^T[16]
  static constexpr int O_W2F = 0, O_W2B = H * LDW, O_B1 = 2 * H * LDW, O_B2 = O_B1 + H, O_SCR = O_B2 + H;
  static constexpr int O_H1 = 0, O_H2 = H * LDT, O_DZ2 = 2 * H * LDT, O_DO = 3 * H * LDT, WSCR = O_DO + 16 * LDT;
  static constexpr int P_STRIDE = PpoShape<D, H, A>::P_STRIDE;
  static constexpr int MAIN = O_SCR + WV_WAVES * WSCR;
  // epilogue exchange (re-uses the staging area): per wave its accumulator tiles as they sit in registers, [slot][lane] of
  // f32x4 -- dW2 16 slots, dW1 4 (+ 4 for the wide tile's second k group), dW3 4 (policy pass) -- then, behind all four
  // waves' tiles, per wave a block of row-summed scalars: db1 | db2 | dW1[:, 16] (64 each), policy db3 | dlogstd (16 each),
  // value dW3 (64) | db3 (16)
  static constexpr int XS_W2 = 0, XS_W1 = 16, XS_W1B = 20, XS_W3 = D > 17 ? 24 : 20, XS_PF = XS_W3 + 4, XS_VF = XS_W3;
  static constexpr int XSC_PF = 3 * H + 32, XSC_VF = 4 * H + 16;
  static constexpr int XCH_PF = WV_WAVES * (XS_PF * 256 + XSC_PF), XCH_VF = WV_WAVES * (XS_VF * 256 + XSC_VF);
  static constexpr int XCH = XCH_PF > XCH_VF ? XCH_PF : XCH_VF;
  // set-up image (a region of its own behind both): the flat parameter block without W2, [W1 | b1 | b2 | W3 | b3 | logstd]
  // at the actual dims, loaded with coalesced dword loads (element tid + 256 k) and read back per lane as register operands;
  // sized for the largest head (8 rows + b3 + logstd) and rounded to whole 256-float load rounds
  static constexpr int O_IMG = MAIN > XCH ? MAIN : XCH;
  static constexpr int IMG_HEAD = 8 * H + 16;
  static constexpr int IMG = (H * D + 2 * H + IMG_HEAD + WV_THREADS - 1) / WV_THREADS * WV_THREADS;
  static constexpr int LDS_FLOATS = O_IMG + IMG;
};

// State-dependent-std head (SD): up to 16 head rows [mean | log_std] and no logstd tail -- a partial row of its own
// stride (the Gaussian's assumes at most 8 head rows + 8 logstd floats).  The LDS layout, main loop and exchange, is
// WvShape's: the 16 head rows are the same four dW3 accumulator tiles.
template <int D, int H, int A> struct WvShapeSD : WvShape<D, H, A> {
  static constexpr int P_PF_SD = H * D + H + H * H + H + 2 * A * H + 2 * A, P_VF = MlpFlat<D, H, 1>::P_VF;
  static constexpr int P_STRIDE = ((P_PF_SD > P_VF ? P_PF_SD : P_VF) + 63) & ~63;
  static constexpr int IMG_HEAD = 16 * H + 16;      // 16 head rows + b3
  static constexpr int IMG = (H * D + 2 * H + IMG_HEAD + WV_THREADS - 1) / WV_THREADS * WV_THREADS;
  static constexpr int LDS_FLOATS = WvShape<D, H, A>::O_IMG + IMG;
};
template <int D, int H, int A, int HEAD> struct WvPick { using T = WvShape<D, H, A>; };
template <int D, int H, int A> struct WvPick<D, H, A, HEAD_SD> { using T = WvShapeSD<D, H, A>; };
// A normed first layer (LN): gamma | beta sit behind b1 in the flat block and in the set-up image (2 H more floats, a load
// round at the most), and dgamma | dbeta (H each) close the per-wave scalar block of the exchange area.  Main-loop layout,
// tile slots and the order of the older scalars are the base shape's.
template <class Base, int H> struct WvLN : Base {
  static constexpr int XSC_PF = Base::XSC_PF + 2 * H, XSC_VF = Base::XSC_VF + 2 * H;
  static constexpr int XCH_PF = WV_WAVES * (Base::XS_PF * 256 + XSC_PF), XCH_VF = WV_WAVES * (Base::XS_VF * 256 + XSC_VF);
  static constexpr int XCH = XCH_PF > XCH_VF ? XCH_PF : XCH_VF;
  static constexpr int O_IMG = Base::MAIN > XCH ? Base::MAIN : XCH;
  static constexpr int IMG = Base::IMG + WV_THREADS;
  static constexpr int LDS_FLOATS = O_IMG + IMG;
};
template <int D, int H, int A, int HEAD, bool LN> struct WvPickLN { using T = typename WvPick<D, H, A, HEAD>::T; };
template <int D, int H, int A, int HEAD> struct WvPickLN<D, H, A, HEAD, true> { using T = WvLN<typename WvPick<D, H, A, HEAD>::T, H>; };
// floats the flat block of a normed net has more than a plain one's (gamma | beta), and the partial-row stride of a pair
// of which the policy (ln_mask bit 0) and / or the critic (bit 1) is normed
#define PPO_LN_EXTRA 128
static inline int ppo_ln_p_pf(int D, int H, int A, int head, int ln_mask) { return ppo_p_pf(D, H, A, head) + ((ln_mask & 1) ? PPO_LN_EXTRA : 0); }
static inline int ppo_ln_p_vf(int D, int H, int ln_mask) { return ppo_p_vf(D, H) + ((ln_mask & 2) ? PPO_LN_EXTRA : 0); }
static inline int ppo_ln_stride(int D, int H, int A, int head, int ln_mask) {
  const int p_pf = ppo_ln_p_pf(D, H, A, head, ln_mask), p_vf = ppo_ln_p_vf(D, H, ln_mask);
  return ((p_pf > p_vf ? p_pf : p_vf) + 63) & ~63;
}
// sum over a sample's four lane groups (lanes j, j + 16, j + 32, j + 48) by ONE ones x value MFMA: D[i][j] = sum_g 1 * v[(j, g)],
// every lane of the sample gets the total (the persistent rollout's form, trl_rollout.h); the lane's 16 registers as a tree
__device__ __forceinline__ float wv_group_sum(float v) { return mfma16(1.0f, v, f32x4{0.f, 0.f, 0.f, 0.f})[0]; }
__device__ __forceinline__ float wv_tree16(const f32x4 (&v)[4]) {
  const f32x4 s = (v[0] + v[1]) + (v[2] + v[3]);
  return (s[0] + s[1]) + (s[2] + s[3]);
}
#define SD_HALF_LOG_2PI_PLUS_HALF 1.4189385332046727f   /* k_gauss_sd.hip's constant: entropy of a unit normal */

__device__ __forceinline__ f32x4 lds4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
// sum over the 16 lanes of a DPP row (same lane group g, all sample lanes j) with row rotations on the
// VALU (no LDS round trips); every lane ends with the total, callers read lane j == 0
__device__ __forceinline__ float row_sum16(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, false));  // row_ror:8
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xF, 0xF, false));  // row_ror:4
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xF, 0xF, false));  // row_ror:2
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xF, 0xF, false));  // row_ror:1
  return v;
}

// RT = false: the network dims are the template's (the benchmark shape, everything folds to constants).
// RT = true: D and A are UPPER BOUNDS (17, 8) and the actual dims come from the launch (a.D in [2, 17], a.A in [1, 8]):
// the same 16 + 1-feature tile with the missing input features and outputs masked to zero where they are loaded, the flat
// parameter offsets and row strides computed from the actual dims -- Hopper / Swimmer / Walker / Reacher-shaped tasks
// (torchrl/networks/base.py:8-44 is shape-generic) stay on the two-launch path.
// D = 32 (WIDE, RT only; a.D in [18, 32] -- Ant's 27 observations): input features 16..31 are a SECOND 16-wide k group of
// the first layer (four more MFMA steps forward, a second accumulator tile per slice for dW1) instead of the single
// 17th column that rides on the VALU.
// CAT (policy pass, RT only): a categorical head (policies.CategoricalDisPolicy; torchrl/policies/discrete_policies.py:124-168)
// instead of the diagonal Gaussian.  The A head outputs are logits, the stored action is ONE float per sample (the index:
// `acts` rows are (N, 1)), the flat policy block has no logstd tail ([W1 b1 W2 b2 W3 b3]) and the per-sample entropy sum
// leaves through the eighth column of the scalar row.  Only the block between the head MFMAs and `dout` differs: softmax,
// log pi and entropy in k_categorical.hip's fixed arithmetic, d(loss)/d(logits) as in cat_losses_kernel.
// SD (policy pass, RT only): a state-dependent-std Gaussian head (policies.GuassianContPolicy;
// torchrl/policies/continuous_policy.py:134-170).  The head has 2 a.A rows [mean | log_std] (MlpFlat order), the flat policy
// block has no logstd tail.  Tile row k < 8 is mean k, tile row 8 + k is log_std k, whatever a.A is: lanes (j, g) and
// (j, g ^ 2) hold a mean and its log_std, one xor-32 exchange apart.  The head row of tile row o -- o < 8 ? o : a.A + (o - 8)
// -- appears where W3 / b3 are loaded and where dW3 / db3 go to the partial row.  Per element the arithmetic is
// gauss_sd_losses_kernel's (k_gauss_sd.hip); the per-sample statistics of log_std and std leave through a second block of
// scalar rows (trl_ppo_sd_scalar_stride).
// LN (RT only; either pass on its own): the net is Linear(D, 64), act, LayerNorm(64, eps 1e-5, affine), Linear(64, 64), act,
// act, Linear(64, O) -- `Net.mlp2_ln_spec`, flat block [W1 b1 gamma beta W2 b2 W3 b3 (logstd)].  Forward: a1 = act(z1) stays
// in registers; mean and variance of the sample's 64 features in two passes (tree over the lane's 16, wv_group_sum over
// the four lane groups; the deviations about the mean are squared, never E[x^2] - E[x]^2); y = gamma xhat + beta goes to
// H1S and to the layer-2 MFMAs; layer 2 ends in act(act(z2)), t = act(z2) (Tanh keeps the gate).  Backward: dZ2 = dH2 act'(h2) act'(t);
// dH1 from the W2^T MFMAs is d y: dgamma += dH1 xhat, dbeta += dH1 (per-lane accumulators, row-summed in the epilogue like
// db1), dxhat = dH1 gamma, da1 = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)), dZ1 = da1 act'(a1).
template <int D, int H, int A, int ACT, bool IS_PF, bool CONTIG, bool RT, int HEAD = HEAD_GAUSS, bool LN = false>
__device__ void ppo_wave_pass(const PpoDev& a, float* lds, int wg_in_net, int n_wg_net) {
  using S = typename WvPickLN<D, H, A, HEAD, LN>::T;
  static_assert(!LN || RT, "the LayerNorm pass belongs to the runtime-dims kernels");
  constexpr bool WIDE = D > 17,                      // a second 16-feature group (features 16 .. 31) on the matrix pipe
                 CAT = HEAD == HEAD_CAT, SD = HEAD == HEAD_SD,
                 SDP = SD && IS_PF;                  // (SD's value pass differs in the stride of its partial row only)
  static_assert(!WIDE || RT, "the wide tile exists as a runtime-dims instantiation only");
  static_assert(!CAT || (IS_PF && RT), "the categorical head is a policy pass of the runtime-dims kernels");
  static_assert(!SD || RT, "the state-dependent-std head belongs to the runtime-dims kernels");
  constexpr int AS = CAT ? 1 : 0;                    // CAT: floats per stored action (0: the Gaussian's O)
  const int Dr = RT ? a.D : D;                       // input features = row stride of obs and of W1
  const int O = IS_PF ? (RT ? a.A : A) : 1;          // outputs
  // offsets inside the flat parameter block for the actual dims (MlpFlat, trl_mlp.h)
  const int OH = SDP ? 2 * O : O;                     // head rows (SD: [mean | log_std])
  const int F_W1 = 0, F_B1 = H * Dr, F_G = F_B1 + H /* LN: gamma | beta */, F_W2 = F_G + (LN ? 2 * H : 0), F_B2 = F_W2 + H * H,
            F_W3 = F_B2 + H, F_B3 = F_W3 + OH * H,
            F_LS = F_B3 + OH, F_END = (CAT || SDP) ? F_LS : F_LS + O;      // (no logstd tail behind a categorical / SD head)
  // SD: does tile row o exist, and which head row is it
  auto sd_has = [&](int o) -> bool { return (o & 7) < O; };
  auto sd_row = [&](int o) -> int { return o < 8 ? o : O + (o - 8); };
  const int PS = RT ? a.p_stride : S::P_STRIDE;      // floats of a partial row (the LDS images keep the template's stride)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, g = lane >> 4, i = j;
  const float* gp = IS_PF ? a.pf_params : a.vf_params;
  WCLK_DECL
  float* W2F = lds + S::O_W2F;
  float* W2B = lds + S::O_W2B;
  float* scr = lds + S::O_SCR + wave * S::WSCR;
  float* H1S = scr + S::O_H1;
  float* H2S = scr + S::O_H2;                       // H2^T until dW3 is done, then dZ1^T
  float* DZ2S = scr + S::O_DZ2;
  float* DOS = scr + S::O_DO;

  // The first tile's inputs sit behind a dependent pair of loads (row index -> cells): the index is requested before
  // anything else and the cells in front of the set-up's LDS stores, so that they travel while the weights are staged.
  // (behind the set-up's barrier these two loads were a memory round trip of their own -- a load cannot be hoisted
  // across a barrier by the compiler)
  const double adv_s1 = IS_PF ? a.adv_raw[0] : 0.0, adv_s2 = IS_PF ? a.adv_raw[1] : 0.0;
  const int B = a.rows_mb * a.N;
  const int n_tiles = (B + 15) / 16;
  const int tile_stride = n_wg_net * WV_WAVES;

  // Inputs are fetched ONE TILE AHEAD as raw values (masks are applied when they are consumed, so no wait
  // sits next to the loads) and the minibatch row index TWO tiles ahead (the dependent load behind it is
  // then off the critical path): x operand (5), X^T for dW1 (4), loss inputs (6 / 2).
  float xq[5], xtq[4], lq[6];
  float xq2[4], xtq2[4];                             // WIDE: features 16 + 4g + q of the x operand / feature 16 + j of X^T
  int tile = wg_in_net * WV_WAVES + wave;
  // ---- CONTIG (N % 16 == 0, hence B % 16 == 0: every tile is 16 consecutive envs of ONE time row, all samples valid) ----
  // The tile position (row, column tile) and the row's base addresses are wave-uniform: they live in scalar registers
  // and are advanced incrementally (no per-lane division, no 64-bit per-lane address arithmetic); each lane adds a
  // constant 32-bit byte offset, so a load is `global_load_dword v, v_off, s[base]` with nothing to compute in front.
  const int tpr = a.N >> 4;                                           // tiles per time row
  int p1r = 0, p1c = 0, p2r = 0, p2c = 0, st_r = 0, st_c = 0;         // positions of tile t+1 / t+2 (in strides), stride split
  int64_t ridx1 = 0, ridx2 = 0;
  // which of the tile's input features exist (RT): features 4g + q of the lane's x operand, feature 16, and feature j of
  // the lane's X^T operand; a missing feature is read from an in-range address and replaced by zero when it is consumed
  bool fv[4], fv2[4];
  const bool f16 = !WIDE && (!RT || Dr > 16), jv = !RT || i < Dr, jv2 = WIDE && 16 + i < Dr;
  const unsigned ox16 = (unsigned)(j * Dr + (f16 ? 16 : 0)) * 4u, os = (unsigned)j * 4u;
  unsigned oxq[4], oxt[4], oa_[4], oxq2[4], oxt2[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    fv[q] = !RT || 4 * g + q < Dr;
    fv2[q] = WIDE && 16 + 4 * g + q < Dr;
    oxq[q] = (unsigned)(j * Dr + (fv[q] ? 4 * g + q : 0)) * 4u;
    oxt[q] = (unsigned)((4 * g + q) * Dr + (jv ? i : 0)) * 4u;
    oxq2[q] = (unsigned)(j * Dr + (fv2[q] ? 16 + 4 * g + q : 0)) * 4u;
    oxt2[q] = (unsigned)((4 * g + q) * Dr + (jv2 ? 16 + i : 0)) * 4u;
    if constexpr (SDP) oa_[q] = (unsigned)(j * O + (4 * (g & 1) + q < O ? 4 * (g & 1) + q : 0)) * 4u;   // lanes g, g ^ 2: the same action
    else oa_[q] = CAT ? (unsigned)j * 4u : (unsigned)(j * O + (4 * g + q < O ? 4 * g + q : 0)) * 4u;
  }
  auto ldb = [](const float* base, unsigned byte_off) -> float {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
  };
  auto pos_advance = [&](int& r, int& c) { c += st_c; r += st_r; if (c >= tpr) { c -= tpr; ++r; } };
  auto load_ridx = [&](int r) -> int64_t {
    const int rr = r < a.rows_mb ? r : 0;                             // tiles past the end: any in-range row
    return a.row_idx ? a.row_idx[rr] : (int64_t)rr;
  };
  auto fetch_contig = [&](int64_t ridx, int r, int c) {
    const int64_t cell0 = (r < a.rows_mb) ? ridx * a.N + 16 * c : 0;  // wave-uniform
    const float* ob = a.obs + cell0 * Dr;
#pragma unroll
    for (int q = 0; q < 4; ++q) xq[q] = ldb(ob, oxq[q]);
    xq[4] = ldb(ob, ox16);
#pragma unroll
    for (int q = 0; q < 4; ++q) xtq[q] = ldb(ob, oxt[q]);           // X[sample 4g + q][feature j]: B operand of the dW1 GEMM
    if constexpr (WIDE) {
#pragma unroll
      for (int q = 0; q < 4; ++q) { xq2[q] = ldb(ob, oxq2[q]); xtq2[q] = ldb(ob, oxt2[q]); }
    }
    if constexpr (IS_PF) {
      const float* ab = a.acts + cell0 * (CAT ? AS : O);
      if constexpr (CAT) { lq[0] = ldb(ab, oa_[0]); lq[1] = lq[2] = lq[3] = 0.0f; }   // the action index of sample j
      else {
#pragma unroll
        for (int q = 0; q < 4; ++q) lq[q] = ldb(ab, oa_[q]);
      }
      lq[4] = ldb(a.advs + cell0, os);
      lq[5] = a.old_logp ? ldb(a.old_logp + cell0, os) : 0.0f;
    } else {
      lq[0] = lq[1] = lq[2] = lq[3] = 0.0f;
      lq[4] = ldb(a.rets + cell0, os);
      lq[5] = a.clipped_value_loss ? ldb(a.old_values + cell0, os) : 0.0f;
    }
  };
  // ---- generic path: any N, ragged last tile; per-lane cell indices ----
  auto row_of = [&](int smp, int& e) -> int { const int sm = smp < B ? smp : 0; const int r = sm / a.N; e = sm - r * a.N; return r; };
  auto fetch_inputs = [&](int64_t p, int s0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) xq[r] = a.obs[p * Dr + (fv[r] ? 4 * g + r : 0)];
    xq[4] = a.obs[p * Dr + (f16 ? 16 : 0)];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int sj = 4 * g + q;
      const int64_t pr = __shfl(p, sj, 64);
      xtq[q] = a.obs[(s0 + sj < B ? pr : 0) * Dr + (jv ? i : 0)];
      if constexpr (WIDE) {
        xq2[q] = a.obs[p * Dr + (fv2[q] ? 16 + 4 * g + q : 0)];
        xtq2[q] = a.obs[(s0 + sj < B ? pr : 0) * Dr + (jv2 ? 16 + i : 0)];
      }
    }
    if constexpr (IS_PF) {
      if constexpr (CAT) { lq[0] = a.acts[p]; lq[1] = lq[2] = lq[3] = 0.0f; }
      else if constexpr (SDP) {
#pragma unroll
        for (int r = 0; r < 4; ++r) lq[r] = a.acts[p * O + (4 * (g & 1) + r < O ? 4 * (g & 1) + r : 0)];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) lq[r] = a.acts[p * O + (4 * g + r < O ? 4 * g + r : 0)];
      }
      lq[4] = a.advs[p]; lq[5] = a.old_logp ? a.old_logp[p] : 0.0f;
    } else {
      lq[0] = lq[1] = lq[2] = lq[3] = 0.0f;
      lq[4] = a.rets[p]; lq[5] = a.clipped_value_loss ? a.old_values[p] : 0.0f;
    }
  };
  int e_nn = 0;
  int64_t ridx_nn = 0;
  auto fetch_row = [&](int t) {
    const int r = row_of(t * 16 + j, e_nn);
    ridx_nn = a.row_idx ? a.row_idx[r] : (int64_t)r;
  };
  // loads of tile `nt` (= current + stride) and the row index of the tile after it
  auto prefetch_next = [&](int nt) {
    if constexpr (CONTIG) {
      fetch_contig(ridx1, p1r, p1c);
      p1r = p2r; p1c = p2c; ridx1 = ridx2;
      pos_advance(p2r, p2c);
      ridx2 = load_ridx(p2r);
    } else {
      const int64_t pn = (nt * 16 + j < B) ? ridx_nn * a.N + e_nn : 0;
      fetch_inputs(pn, nt * 16);
      fetch_row(nt + tile_stride);
    }
  };
  // ---- one-time setup ----
  // Order of the set-up's loads: the first tile's row index, then everything that needs the kernel arguments only (W2
  // twice, the parameter image), and only then the first tile's cells, which wait for the index.  The cells' round trip
  // ends under the LDS stores, the barrier and the operand reads below.
  int r0 = 0, c0 = 0;
  int64_t ridx0 = 0;
  if constexpr (CONTIG) {
    const int t0 = __builtin_amdgcn_readfirstlane(tile);
    const int ts = __builtin_amdgcn_readfirstlane(tile_stride);
    st_r = ts / tpr; st_c = ts - st_r * tpr;
    r0 = t0 / tpr; c0 = t0 - (t0 / tpr) * tpr;
    ridx0 = load_ridx(r0);
  } else {
    fetch_row(tile);
  }
  __builtin_amdgcn_sched_barrier(0);
  constexpr int NV = H * H / (4 * WV_THREADS);    // all loads in flight before the first LDS store
  f32x4 wv[NV], wt[NV];
  const int tc = tid & 63, tq = tid >> 6;
  {
    // W2 is staged twice, row-major (forward A operand: W2[own row][k]) and transposed (backward A operand: W2[k][own
    // column]).  Both copies are written with 16-byte LDS stores: the transposed one from a second, column-wise read of
    // the 16 KB block (coalesced along the column index, served by L1 / L2) -- scattering the row-wise registers instead
    // took 64 four-byte stores per thread whose 16 lanes of a row hit two banks.
    static_assert(WV_THREADS == 256 && H == 64, "the transposed staging maps (column, 4 rows) onto 256 threads");
    // (runtime dims: the value block starts P_PF floats into the flat buffer, which is a multiple of 4 only for even A)
    const bool w2_al = !RT || ((reinterpret_cast<uintptr_t>(gp + F_W2) & 15) == 0);
#pragma unroll
    for (int t = 0; t < NV; ++t) {
      if (w2_al) wv[t] = *reinterpret_cast<const f32x4*>(gp + F_W2 + 4 * (tid + WV_THREADS * t));
      else {
#pragma unroll
        for (int x = 0; x < 4; ++x) wv[t][x] = gp[F_W2 + 4 * (tid + WV_THREADS * t) + x];
      }
    }
#pragma unroll
    for (int t = 0; t < NV; ++t)
#pragma unroll
      for (int x = 0; x < 4; ++x) wt[t][x] = gp[F_W2 + (4 * (tq + 4 * t) + x) * H + tc];       // W2[r4 + x][column tc]
  }
  // The parameter image: the two runs of the flat block on either side of W2, [0, F_W2) and [F_B2, F_END), as one
  // sequence of n_img floats; thread tid loads elements tid + 256 k with dword loads (the value block is 16-byte aligned
  // only for some A).  An element past the end re-reads the block's last float -- nothing outside [0, F_END) is touched --
  // and lands in the image's rounding tail, which no lane reads.
  constexpr int NI = S::IMG / WV_THREADS;
  const int n_img = F_W2 + (F_END - F_B2);
  float im[NI];
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const int e = tid + WV_THREADS * k, ec = e < n_img ? e : n_img - 1;
    im[k] = gp[ec < F_W2 ? ec : ec + H * H];
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (CONTIG) {
    fetch_contig(ridx0, r0, c0);                                      // tile t (dependent pair of loads, once per kernel)
    p1r = r0; p1c = c0;
    pos_advance(p1r, p1c);
    ridx1 = load_ridx(p1r);
    p2r = p1r; p2c = p1c;
    pos_advance(p2r, p2c);
    ridx2 = load_ridx(p2r);
  } else {
    const int64_t p0 = (tile * 16 + j < B) ? ridx_nn * a.N + e_nn : 0;
    fetch_inputs(p0, tile * 16);
    fetch_row(tile + tile_stride);
  }
#ifdef TRL_EXP_CLK
  // the set-up split: 22 = every global load issued, 23 = all of them returned (it includes the first tile's dependent
  // pair), 0 = the work behind them (LDS stores, barrier, operand reads from the image, f64 constants)
  WCLK(22)
  __builtin_amdgcn_s_waitcnt(0);
  WCLK(23)
#endif
  for (int e = lane; e < 16 * LDT; e += 64) DOS[e] = 0.0f;       // dout rows >= O stay zero
#pragma unroll
  for (int t = 0; t < NV; ++t) {
    const int e = 4 * (tid + WV_THREADS * t), r = e / H, c = e - r * H;
    *reinterpret_cast<f32x4*>(W2F + r * LDW + c) = wv[t];
    *reinterpret_cast<f32x4*>(W2B + tc * LDW + 4 * (tq + 4 * t)) = wt[t];
  }
  // the image, and from its registers b1 | b2 (adjacent in the image: elements [F_B1, F_B1 + 2H)) to their place
  float* img = lds + S::O_IMG;
  constexpr int KB_LO = H * (WIDE ? 18 : RT ? 2 : D) / WV_THREADS, KB_HI = (H * D + (LN ? 4 : 2) * H - 1) / WV_THREADS;
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const int e = tid + WV_THREADS * k;
    img[e] = im[k];
    if constexpr (LN) {                                  // (gamma | beta lie between the two: b2 is the image's F_W2 .. F_W2 + H)
      if (k >= KB_LO && k <= KB_HI && e >= F_B1 && e < F_B1 + H) lds[S::O_B1 + (e - F_B1)] = im[k];
      if (k >= KB_LO && k <= KB_HI && e >= F_W2 && e < F_W2 + H) lds[S::O_B2 + (e - F_W2)] = im[k];
    } else
    if (k >= KB_LO && k <= KB_HI && e >= F_B1 && e < F_B1 + 2 * H) lds[S::O_B1 + (e - F_B1)] = im[k];
  }
  static_assert(S::O_B2 == S::O_B1 + H, "b1 | b2 are stored as one run");
  __syncthreads();

  // register-resident A operands, lane (i, g): k index of MFMA step (slice sl, r) is feature 16 sl + 4 g + r.  Read from
  // the image at the flat block's offsets (behind W2: less its H * H floats).  Every read is issued before the first mask
  // is applied (one LDS round trip, not one per group of operands); a masked operand reads an in-range float and is an
  // exact zero.
  const int I_W3 = F_W3 - H * H, I_B3 = F_B3 - H * H, I_LS = F_LS - H * H;
  float w1[4][5], w3h[4][4], w3t[4][4];
  float w1b[4][4];                                   // WIDE: W1[row][16 + 4g + r]
  float b3v[4], lsraw[4];                            // per-lane constants of the lane's 4 outputs o = 4g + r (policy)
#pragma unroll
  for (int so = 0; so < 4; ++so) {
    const int row = 16 * so + i;
#pragma unroll
    for (int r = 0; r < 4; ++r) w1[so][r] = img[F_W1 + row * Dr + (fv[r] ? 4 * g + r : 0)];
    w1[so][4] = img[F_W1 + row * Dr + (f16 ? 16 : 0)];
    if constexpr (WIDE) {
#pragma unroll
      for (int r = 0; r < 4; ++r) w1b[so][r] = img[F_W1 + row * Dr + (fv2[r] ? 16 + 4 * g + r : 0)];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = 4 * g + r;
      if constexpr (SDP) {
        w3h[so][r] = img[I_W3 + (sd_has(i) ? sd_row(i) : 0) * H + 16 * so + 4 * g + r];        // head: W3[row of tile row i][k]
        w3t[so][r] = img[I_W3 + (sd_has(o) ? sd_row(o) : 0) * H + row];                        // dH2: W3[row of tile row o][own f]
      } else if constexpr (IS_PF) {
        w3h[so][r] = img[I_W3 + (i < O ? i : 0) * H + 16 * so + 4 * g + r];                    // head: W3[o = i][k]
        w3t[so][r] = img[I_W3 + (o < O ? o : 0) * H + row];                                    // dH2: W3[k = o][own f]
      } else {
        w3h[so][r] = img[I_W3 + 16 * so + 4 * g + r];                                          // per-lane head weights
        w3t[so][r] = 0.0f;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int o = 4 * g + r;
    if constexpr (IS_PF && !CAT && !SDP) lsraw[r] = img[I_LS + (o < O ? o : 0)];
    else lsraw[r] = 0.0f;
    if constexpr (SDP) b3v[r] = img[I_B3 + (sd_has(o) ? sd_row(o) : 0)];
    else b3v[r] = img[I_B3 + (o < O ? o : 0)];
  }
  const float vb3 = IS_PF ? 0.0f : img[I_B3];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int so = 0; so < 4; ++so) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = 4 * g + r;
      w1[so][r] = fv[r] ? w1[so][r] : 0.0f;
      if constexpr (WIDE) w1b[so][r] = fv2[r] ? w1b[so][r] : 0.0f;
      if constexpr (SDP) {
        w3h[so][r] = sd_has(i) ? w3h[so][r] : 0.0f;
        w3t[so][r] = sd_has(o) ? w3t[so][r] : 0.0f;
      } else if constexpr (IS_PF) {
        w3h[so][r] = (i < O) ? w3h[so][r] : 0.0f;
        w3t[so][r] = (o < O) ? w3t[so][r] : 0.0f;
      }
    }
    w1[so][4] = (g == 0 && f16) ? w1[so][4] : 0.0f;
  }
  float lsv[4], ivv[4], lspass[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int o = 4 * g + r;
    const float raw = (IS_PF && !CAT && !SDP && o < O) ? lsraw[r] : 0.0f;
    lsv[r] = fminf(fmaxf(raw, -20.0f), 2.0f);                   // continuous_policy.py:8-9,185
    ivv[r] = __expf(-2.0f * lsv[r]);
    lspass[r] = (raw >= -20.0f && raw <= 2.0f) ? 1.0f : 0.0f;   // clamp passes gradient inside [-20, 2]
    if constexpr (SDP) b3v[r] = sd_has(o) ? b3v[r] : 0.0f;      // (lsv / ivv are per tile, see the loop)
    else b3v[r] = (o < O) ? b3v[r] : 0.0f;
  }

  // advantage normalisation constants (ppo.py:141-147): mean, unbiased std
  const double ng = a.n_global;
  const double adv_mean = adv_s1 / ng;
  const double adv_var = (adv_s2 - adv_s1 * adv_s1 / ng) / (ng - 1.0);
  const float adv_mu = (float)adv_mean;
  const float adv_rstd = 1.0f / ((float)sqrt(fmax(adv_var, 0.0)) + 1e-5f);
  const float inv_b = (float)(1.0 / ng);

  // ---- gradient accumulators ----
  f32x4 gW2[4][4], gW1[4], gW3[4];                  // MFMA tiles: dW2[f2 slice][f1 slice], dW1[f1 slice][k < 16], dW3
  f32x4 gW1b[4];                                     // WIDE: dW1[f1 slice][16 <= k < 32]
  float gb1[4][4], gb2[4][4], gW1c[4][4];           // per-lane (own sample) partials: db1, db2, dW1[:, 16]
  float db3[4], dls[4], stv[7];
  float ent_sum = 0.0f;                              // CAT / SD: sum of the per-sample entropies (lanes g == 0)
  // SD: the lane's log_std / std elements (lanes g < 2 own outputs 4g + r): sum, sum of squares, max, -min of each; the
  // valid samples of lanes g == 0
  float sdst[8] = {0.0f, 0.0f, -INFINITY, -INFINITY, 0.0f, 0.0f, -INFINITY, -INFINITY}, sd_cnt = 0.0f;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    gW1[x] = gW3[x] = gW1b[x] = f32x4{0.f, 0.f, 0.f, 0.f};
    db3[x] = dls[x] = 0.0f;
#pragma unroll
    for (int y = 0; y < 4; ++y) { gW2[x][y] = f32x4{0.f, 0.f, 0.f, 0.f}; gb1[x][y] = gb2[x][y] = gW1c[x][y] = 0.0f; }
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) stv[k] = (k >= 2 && k <= 5) ? -INFINITY : 0.0f;
  f32x4 ggm[4], gbt[4];                              // LN: per-lane (own sample) partials of dgamma, dbeta
#pragma unroll
  for (int x = 0; x < 4; ++x) ggm[x] = gbt[x] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* lng = lds + S::O_IMG + F_G;          // LN: gamma | beta where the set-up image keeps them (H apart)

  WCLK(0)
  for (; tile < n_tiles; tile += tile_stride) {
    const int s = tile * 16 + j;
    const bool valid = CONTIG ? true : (s < B);
    float xb[5], xt[4], lin[6], xb2[4], xt2[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) xb[r] = (valid && fv[r]) ? xq[r] : 0.0f;
    xb[4] = (valid && f16) ? xq[4] : 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) xt[q] = (jv && (CONTIG || tile * 16 + 4 * g + q < B)) ? xtq[q] : 0.0f;
    if constexpr (WIDE) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        xb2[q] = (valid && fv2[q]) ? xq2[q] : 0.0f;
        xt2[q] = (jv2 && (CONTIG || tile * 16 + 4 * g + q < B)) ? xtq2[q] : 0.0f;
      }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) lin[q] = lq[q];
    const float x16 = xb[4];

    // LDS operand reads are issued one phase AHEAD of the MFMAs that consume them (PIN_DS keeps the compiler from
    // sinking them back next to their use): the ~130-cycle LDS round trip then runs under the previous phase's matrix
    // work instead of stalling the in-order wave in front of every 4-MFMA group.
#define PIN_DS() __builtin_amdgcn_sched_barrier(0x676)   /* VALU / SALU / VMEM / DS writes / transcendentals may cross; DS reads and MFMAs may not */
    // ---- forward layer 1: 4 independent slices ----
    f32x4 h1[4], h2[4];
    f32x4 t2[4];                                       // LN, Tanh: the gate of act(act(z2)), act'(h2) act'(tanh(z2))
    f32x4 wq[4], bq;                                  // W2 operand slices / b2 slice of the NEXT L2 output slice
#pragma unroll
    for (int so = 0; so < 4; ++so) h1[so] = lds4(lds + S::O_B1 + 16 * so + 4 * g);
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) wq[sl] = lds4(W2F + i * LDW + 16 * sl + 4 * g);
    bq = lds4(lds + S::O_B2 + 4 * g);
    PIN_DS();
    WCLK(9)
#pragma unroll
    for (int q = 0; q < (WIDE ? 4 : 5); ++q)
#pragma unroll
      for (int so = 0; so < 4; ++so) h1[so] = mfma16(w1[so][q], xb[q], h1[so]);
    if constexpr (WIDE) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int so = 0; so < 4; ++so) h1[so] = mfma16(w1b[so][q], xb2[q], h1[so]);
    }
    WCLK(10)
    f32x4 a1[4], xh[4];                                // LN: act(z1) and the normalised row; h1 then holds y = gamma xhat + beta
    float rstd = 0.0f;
    if constexpr (LN) {
#pragma unroll
      for (int so = 0; so < 4; ++so)
#pragma unroll
        for (int r = 0; r < 4; ++r) a1[so][r] = act_fn<ACT>(h1[so][r]);
      const float mean = wv_group_sum(wv_tree16(a1)) * (1.0f / 64.0f);
      f32x4 dq[4];
#pragma unroll
      for (int so = 0; so < 4; ++so)
#pragma unroll
        for (int r = 0; r < 4; ++r) { xh[so][r] = a1[so][r] - mean; dq[so][r] = xh[so][r] * xh[so][r]; }
      rstd = 1.0f / sqrtf(wv_group_sum(wv_tree16(dq)) * (1.0f / 64.0f) + LN_EPS);
#pragma unroll
      for (int so = 0; so < 4; ++so) {
        const f32x4 gm = lds4(lng + 16 * so + 4 * g), bt = lds4(lng + H + 16 * so + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          xh[so][r] *= rstd;
          h1[so][r] = fmaf(gm[r], xh[so][r], bt[r]);
          H1S[(16 * so + 4 * g + r) * LDT + j] = h1[so][r];      // y^T[f][s] for dW2
        }
      }
    } else {
#pragma unroll
    for (int so = 0; so < 4; ++so)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        h1[so][r] = act_fn<ACT>(h1[so][r]);
        H1S[(16 * so + 4 * g + r) * LDT + j] = h1[so][r];        // H1^T[f][s] for dW2
      }
    }
    WCLK(1)
    // ---- forward layer 2 ----
#pragma unroll
    for (int so = 0; so < 4; ++so) {
      f32x4 acc = bq;
      f32x4 wc[4];
#pragma unroll
      for (int sl = 0; sl < 4; ++sl) wc[sl] = wq[sl];
      if (so < 3) {
#pragma unroll
        for (int sl = 0; sl < 4; ++sl) wq[sl] = lds4(W2F + (16 * (so + 1) + i) * LDW + 16 * sl + 4 * g);
        bq = lds4(lds + S::O_B2 + 16 * (so + 1) + 4 * g);
        PIN_DS();
      }
#pragma unroll
      for (int sl = 0; sl < 4; ++sl)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = mfma16(wc[sl][r], h1[sl][r], acc);
      WCLK(11)
      if constexpr (LN && ACT == TRL_ACT_TANH) {        // act(act(z2)); for ReLU the second one changes nothing, gate included
#pragma unroll
        for (int r = 0; r < 4; ++r) {                    // (t2 ends as the gate act'(h2) act'(t): one live value, not two)
          const float t = act_fn<ACT>(acc[r]);
          h2[so][r] = act_fn<ACT>(t);
          t2[so][r] = act_grad<ACT>(h2[so][r]) * act_grad<ACT>(t);
        }
      } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) h2[so][r] = act_fn<ACT>(acc[r]);
      }
      WCLK(12)
    }

    // Next tile's loads are issued HERE, mid-tile: at the top of the loop every outstanding load is then
    // half a tile old, and no wait next to the first MFMAs can stall on a load that was just issued.
    prefetch_next(tile + tile_stride);            // loads of tile t+1 (addresses were resolved a tile ago), row index of tile t+2
    WCLK(2)
    // ---- head, loss, d(loss)/d(out), dZ2 ----
    f32x4 dz2[4];
    f32x4 wb[4];                                       // W2^T operand slices of the next dH1 k-slice
    if constexpr (IS_PF) {
#pragma unroll
      for (int so = 0; so < 4; ++so)
#pragma unroll
        for (int r = 0; r < 4; ++r) H2S[(16 * so + 4 * g + r) * LDT + j] = h2[so][r];            // H2^T[f][s] for dW3
      // out^T[o][s]: two interleaved accumulation chains over the 64 features
      f32x4 oa = f32x4{b3v[0], b3v[1], b3v[2], b3v[3]}, ob = f32x4{0.f, 0.f, 0.f, 0.f};
      // LN: the head's operands (W3[row of tile row i][k], W3[row of output o][own f]) are read from the set-up image every
      // tile instead of living in 32 registers -- with a1, xhat and the dgamma / dbeta partials resident the wide tile's
      // policy pass would otherwise go through scratch memory
      f32x4 wh[4], wt[4];
#define W3H(sl, r) (LN ? wh[sl][r] : w3h[sl][r])
#define W3T(so, r) (LN ? wt[so][r] : w3t[so][r])
      if constexpr (LN) {
        const bool hok = SDP ? sd_has(i) : i < O;
        const float* hp = img + I_W3 + (hok ? (SDP ? sd_row(i) : i) : 0) * H + 4 * g;
#pragma unroll
        for (int sl = 0; sl < 4; ++sl) {
          wh[sl] = lds4(hp + 16 * sl);
#pragma unroll
          for (int r = 0; r < 4; ++r) wh[sl][r] = hok ? wh[sl][r] : 0.0f;
        }
      }
#pragma unroll
      for (int sl = 0; sl < 4; sl += 2)
#pragma unroll
        for (int r = 0; r < 4; ++r) { oa = mfma16(W3H(sl, r), h2[sl][r], oa); ob = mfma16(W3H(sl + 1, r), h2[sl + 1][r], ob); }
      WCLK(14)
      // lane (j, g < 2) owns outputs o = 4g + r of sample j
      float zc[4], lp = 0.0f;
      float pk[4], lpk[4], ent = 0.0f;                               // CAT: p_k, log p_k of the lane's logits; the sample's entropy
      int ai = 0;                                                    // CAT: the stored action
      if constexpr (CAT) {
        // The sample's (up to) 8 logits sit in lanes (j, 0) and (j, 1).  m = max_k l_k; e_k = exp(l_k - m); S = sum_k e_k in
        // ascending k (lane g = 1 continues lane g = 0's partial sum: a missing logit adds an exact zero); p_k = e_k / S;
        // log p_k = (l_k - m) - log S -- the arithmetic of cat_losses_kernel.  Lanes g >= 2 run on zeros.
        float lg[4], ek[4], m = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          lg[r] = oa[r] + ob[r];
          m = (4 * g + r < O) ? fmaxf(m, lg[r]) : m;
        }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = g < 2 ? m : 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) ek[r] = (4 * g + r < O) ? expf(lg[r] - m) : 0.0f;
        const float c_own = ((ek[0] + ek[1]) + ek[2]) + ek[3];
        const float c_lo = __shfl_xor(c_own, 16, 64);                // lane g = 1: e_0 + .. + e_3
        float Ssum = g == 1 ? (((c_lo + ek[0]) + ek[1]) + ek[2]) + ek[3] : c_own;
        const float S_hi = __shfl_xor(Ssum, 16, 64);                 // lane g = 0: the whole sum
        Ssum = g == 0 ? S_hi : (g == 1 ? Ssum : 1.0f);
        const float logS = logf(Ssum);
        ai = min(max((int)lin[0], 0), O - 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool has = 4 * g + r < O;
          lpk[r] = has ? (lg[r] - m) - logS : 0.0f;
          pk[r] = ek[r] / Ssum;
          lp += (has && 4 * g + r == ai) ? lpk[r] : 0.0f;
          ent -= pk[r] * lpk[r];
        }
        lp += __shfl_xor(lp, 16, 64);                                // the action's lane holds log pi, the other an exact zero
        ent += __shfl_xor(ent, 16, 64);                              // H = -sum_k p_k log p_k (logits 0..3 + 4..7)
      } else if constexpr (SDP) {
        // Lane (j, g < 2) holds means 4g + r of sample j, lane (j, g + 2) the raw log_std of the same outputs.  After the
        // exchange ALL FOUR lane groups run the per-element arithmetic of gauss_sd_losses_kernel on (mean, raw) -- the same
        // instructions on the same values, so both halves hold the same log pi -- and each keeps its own half of d(head).
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool has = 4 * (g & 1) + r < O;
          const float mine = oa[r] + ob[r], oth = __shfl_xor(mine, 32, 64);
          const float mean = g < 2 ? mine : oth, raw = g < 2 ? oth : mine;
          lsv[r] = fminf(fmaxf(raw, -20.0f), 2.0f);
          ivv[r] = __expf(-2.0f * lsv[r]);
          lspass[r] = (raw >= -20.0f && raw <= 2.0f) ? 1.0f : 0.0f;   // d clamp / d raw
          const float t = gauss_logp_term((valid && has) ? lin[r] : 0.0f, has ? mean : 0.0f, ivv[r], lsv[r], a.tanh_action, zc[r]);
          lp += has ? t : 0.0f;
          ent += has ? SD_HALF_LOG_2PI_PLUS_HALF + lsv[r] : 0.0f;
          zc[r] = has ? zc[r] : 0.0f;
        }
        lp += __shfl_xor(lp, 16, 64);                                // outputs 0..3 + 4..7, in both halves
        ent += __shfl_xor(ent, 16, 64);
      } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {                                  // branch-free: lanes without an output compute on zeros
        const bool has = 4 * g + r < O;
        const float t = gauss_logp_term((valid && has) ? lin[r] : 0.0f, has ? oa[r] + ob[r] : 0.0f, ivv[r], lsv[r],
                                        a.tanh_action, zc[r]);
        lp += has ? t : 0.0f;
        zc[r] = has ? zc[r] : 0.0f;
      }
      WCLK(18)
      lp += __shfl_xor(lp, 16, 64);                                // outputs 0..3 (g = 0) + 4..7 (g = 1)
      }
      WCLK(19)
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
      WCLK(20)
      float dout[4];
      if constexpr (CAT) {
        // dout_k = g_lp (1[k = a] - p_k) + (entropy_coeff / n) p_k (log p_k + H): the entropy bonus -c H in the loss
        const float ce = a.entropy_coeff * inv_b;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool own = valid && g < 2 && 4 * g + r < O;
          dout[r] = own ? g_lp * ((4 * g + r == ai ? 1.0f : 0.0f) - pk[r]) + ce * pk[r] * (lpk[r] + ent) : 0.0f;
          db3[r] += dout[r];
          if (g < 2) DOS[(4 * g + r) * LDT + j] = dout[r];           // dout^T[o][s] for dW3
        }
        if (valid && g == 0) ent_sum += ent;
      } else if constexpr (SDP) {
        // tile rows 4g + r: d(loss)/d(mean) in lanes g < 2, d(loss)/d(raw log_std) in lanes g >= 2 (a clamped element: gate
        // 0, an exact zero); both halves go to the DOS rows of dW3 / dH2 and to db3
        const float ce = a.entropy_coeff * inv_b;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool own = valid && 4 * (g & 1) + r < O;
          const float dm = g_lp * zc[r] * ivv[r], dr = lspass[r] * (g_lp * (zc[r] * zc[r] * ivv[r] - 1.0f) - ce);
          dout[r] = own ? (g < 2 ? dm : dr) : 0.0f;
          db3[r] += dout[r];
          DOS[(4 * g + r) * LDT + j] = dout[r];                      // dout^T[tile row][s] for dW3
          if (own && g < 2) {                                        // log_std/*, std/* over the elements (ppo.py:83-86, a2c.py:96-101)
            const float x = lsv[r], ex = expf(x);
            sdst[0] += x; sdst[1] = fmaf(x, x, sdst[1]); sdst[2] = fmaxf(sdst[2], x); sdst[3] = fmaxf(sdst[3], -x);
            sdst[4] += ex; sdst[5] = fmaf(ex, ex, sdst[5]); sdst[6] = fmaxf(sdst[6], ex); sdst[7] = fmaxf(sdst[7], -ex);
          }
        }
        if (valid && g == 0) { ent_sum += ent; sd_cnt += 1.0f; }
      } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool own = valid && g < 2 && 4 * g + r < O;
        dout[r] = own ? g_lp * zc[r] * ivv[r] : 0.0f;
        db3[r] += dout[r];
        dls[r] += own ? lspass[r] * (g_lp * (zc[r] * zc[r] * ivv[r] - 1.0f) - a.entropy_coeff * inv_b) : 0.0f;
        if (g < 2) DOS[(4 * g + r) * LDT + j] = dout[r];           // dout^T[o][s] for dW3
      }
      }
      WCLK(21)
      if (valid && g == 0) {
        stv[0] += lp; stv[1] = fmaf(lp, lp, stv[1]); stv[6] -= fminf(s1, s2);
        stv[2] = fmaxf(stv[2], lp); stv[3] = fmaxf(stv[3], -lp);
        stv[4] = fmaxf(stv[4], ratio); stv[5] = fmaxf(stv[5], -ratio);
      }
      WCLK(15)
      // operands of dW3 (and of the first dH1 k-slice) are requested now and arrive under the dH2 MFMAs
      const f32x4 da = lds4(DOS + i * LDT + 4 * g);
      f32x4 hb3[4];
#pragma unroll
      for (int so = 0; so < 4; ++so) hb3[so] = lds4(H2S + (16 * so + j) * LDT + 4 * g);
#pragma unroll
      for (int so = 0; so < 4; ++so) wb[so] = lds4(W2B + (16 * so + i) * LDW + 4 * g);
      if constexpr (LN) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = 4 * g + r;
          const bool ook = SDP ? sd_has(o) : o < O;
          const float* tp = img + I_W3 + (ook ? (SDP ? sd_row(o) : o) : 0) * H + i;
#pragma unroll
          for (int so = 0; so < 4; ++so) { const float w = tp[16 * so]; wt[so][r] = ook ? w : 0.0f; }
        }
      }
      PIN_DS();
      // dH2^T[f][s] = sum_o W3[o][f] dout[o][s];  dZ2 = dH2 * act'(H2)
#pragma unroll
      for (int so = 0; so < 4; ++so) dz2[so] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int so = 0; so < 4; ++so) dz2[so] = mfma16(W3T(so, r), dout[r], dz2[so]);
#undef W3H
#undef W3T
      // dW3[o][f] += sum_s dout[s][o] H2[s][f]   (K step q is sample 4g + q)
#pragma unroll
      for (int so = 0; so < 4; ++so)
#pragma unroll
        for (int q = 0; q < 4; ++q) gW3[so] = mfma16(da[q], hb3[so][q], gW3[so]);
      WCLK(16)
    } else {
#pragma unroll
      for (int so = 0; so < 4; ++so) wb[so] = lds4(W2B + (16 * so + i) * LDW + 4 * g);
      PIN_DS();
      float v = 0.0f;
#pragma unroll
      for (int so = 0; so < 4; ++so)
#pragma unroll
        for (int r = 0; r < 4; ++r) v = fmaf(w3h[so][r], h2[so][r], v);
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      v += vb3;
      const float R = lin[4];
      float dv, l;
      if (a.clipped_value_loss) {                                  // ppo.py:104-111
        const float vo = lin[5];
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
      dv = valid ? dv : 0.0f;
      if (valid && g == 0) {
        stv[6] += l; db3[0] += dv;
        stv[0] += v; stv[1] = fmaf(v, v, stv[1]); stv[2] = fmaxf(stv[2], v); stv[3] = fmaxf(stv[3], -v);   // v_pred/*
      }
#pragma unroll
      for (int so = 0; so < 4; ++so)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          dz2[so][r] = dv * w3h[so][r];
          gW3[so][r] = fmaf(dv, h2[so][r], gW3[so][r]);             // per-lane dW3[f] partial (own sample)
        }
    }
#pragma unroll
    for (int so = 0; so < 4; ++so)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (LN && ACT == TRL_ACT_TANH) dz2[so][r] *= t2[so][r];
        else
        dz2[so][r] *= act_grad<ACT>(h2[so][r]);
        gb2[so][r] += dz2[so][r];
        DZ2S[(16 * so + 4 * g + r) * LDT + j] = dz2[so][r];        // dZ2^T[f][s] for dW2
      }

    WCLK(3)
    // ---- dH1^T (all slices) = W2^T dZ2^T ; dZ1 = dH1 * act'(H1) ----
    f32x4 dz1[4];
    f32x4 hb[4], za2;                                  // dW2 operands: H1 rows (all four slices), dZ2 rows of the next slice
#pragma unroll
    for (int so = 0; so < 4; ++so) dz1[so] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) {
      f32x4 w[4];
#pragma unroll
      for (int so = 0; so < 4; ++so) w[so] = wb[so];
      if (sl < 3) {
#pragma unroll
        for (int so = 0; so < 4; ++so) wb[so] = lds4(W2B + (16 * so + i) * LDW + 16 * (sl + 1) + 4 * g);
      } else {                                         // last k-slice: the dW2 operands are requested under it
#pragma unroll
        for (int c = 0; c < 4; ++c) hb[c] = lds4(H1S + (16 * c + j) * LDT + 4 * g);
        za2 = lds4(DZ2S + i * LDT + 4 * g);
      }
      PIN_DS();
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int so = 0; so < 4; ++so) dz1[so] = mfma16(w[so][r], dz2[sl][r], dz1[so]);
    }
    WCLK(17)
    if constexpr (LN) {
      // dz1 holds d y.  dgamma / dbeta partials, dxhat = d y gamma, then the norm's backward: two more per-sample means
      // (issued together), da1 = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat))
      f32x4 dp[4];
#pragma unroll
      for (int so = 0; so < 4; ++so) {
        const f32x4 gm = lds4(lng + 16 * so + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float dy = dz1[so][r];
          ggm[so][r] = fmaf(dy, xh[so][r], ggm[so][r]);
          gbt[so][r] += dy;
          dz1[so][r] = dy * gm[r];
          dp[so][r] = dz1[so][r] * xh[so][r];
        }
      }
      const float m1 = wv_group_sum(wv_tree16(dz1)) * (1.0f / 64.0f), m2 = wv_group_sum(wv_tree16(dp)) * (1.0f / 64.0f);
#pragma unroll
      for (int so = 0; so < 4; ++so)
#pragma unroll
        for (int r = 0; r < 4; ++r) dz1[so][r] = rstd * ((dz1[so][r] - m1) - xh[so][r] * m2);
    }
#pragma unroll
    for (int so = 0; so < 4; ++so)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dz1[so][r] *= act_grad<ACT>(LN ? a1[so][r] : h1[so][r]);
        gb1[so][r] += dz1[so][r];
        if constexpr (!WIDE) gW1c[so][r] = fmaf(dz1[so][r], x16, gW1c[so][r]);
        H2S[(16 * so + 4 * g + r) * LDT + j] = dz1[so][r];         // dZ1^T[f][s] for dW1 (H2^T is consumed)
      }
    // the dW1 operands (dZ1 rows) are requested now and arrive under the dW2 MFMAs
    f32x4 za1[4];
#pragma unroll
    for (int so = 0; so < 4; ++so) za1[so] = lds4(H2S + (16 * so + i) * LDT + 4 * g);
    PIN_DS();

    WCLK(4)
    // ---- dW2[f2][f1] += sum_s dZ2[s][f2] H1[s][f1]  (K step q is sample 4g + q) ----
#pragma unroll
    for (int so = 0; so < 4; ++so) {
      const f32x4 za = za2;
      if (so < 3) { za2 = lds4(DZ2S + (16 * (so + 1) + i) * LDT + 4 * g); PIN_DS(); }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) gW2[so][c] = mfma16(za[q], hb[c][q], gW2[so][c]);
    }
    WCLK(5)
    // ---- dW1[f1][k < 16] += sum_s dZ1[s][f1] X[s][k] ----
#pragma unroll
    for (int so = 0; so < 4; ++so)
#pragma unroll
      for (int q = 0; q < 4; ++q) gW1[so] = mfma16(za1[so][q], xt[q], gW1[so]);
    if constexpr (WIDE) {
#pragma unroll
      for (int so = 0; so < 4; ++so)
#pragma unroll
        for (int q = 0; q < 4; ++q) gW1b[so] = mfma16(za1[so][q], xt2[q], gW1b[so]);
    }
#undef PIN_DS
    WCLK(6)
  }

  __syncthreads();                                                 // staging / weight copies are dead from here
  const int wg = blockIdx.x;
  // ---- epilogue: the waves exchange their accumulators in register layout, every wave folds the slots it owns ----
  // Exchange: one 16-byte LDS store per accumulator tile at [wave][slot][lane] (consecutive lanes, consecutive 16 bytes),
  // and the wave's row-summed scalars.  A wave that ran no tile writes its zeros.
  {
    constexpr int NS = IS_PF ? S::XS_PF : S::XS_VF, SC = IS_PF ? S::XSC_PF : S::XSC_VF;
    f32x4* xch = reinterpret_cast<f32x4*>(lds);
    float* xsc = lds + WV_WAVES * NS * 256;
    f32x4* xw = xch + (wave * NS) * 64 + lane;
    float* sw = xsc + wave * SC;
    // The per-lane partials db1 | db2 | dW1[:, 16] (| the value net's dW3) are summed over the 16 sample lanes of a row
    // group.  Instead of a row_sum16 per value in all 64 lanes (four DPP adds each, 48 / 64 values), the wave first
    // transposes them through its own region: lane (j, g) stores the f32x4 of (kind, so) as entry j of task
    // tt = 16 kind + 4 so + g, lane tt reads the task's 16 entries back and adds them in row_sum16's tree --
    // ((x0 + x8) + (x4 + x12)) + ((x2 + x10) + (x6 + x14)), the same over the odd lanes, even + odd: lane j == 0's result
    // bit for bit (its partners' values are the same sums with the operands swapped).  A task is 17 entries apart from
    // the next, so the 16 lanes of a read hit 16 different 16-byte bank slots.  LDS operations of one wave execute in
    // order: no barrier between the stores, the reads and the tile stores that overwrite the region.
    {
      constexpr int NK = IS_PF ? 3 : 4, TS = 17;
      static_assert(NK * 16 <= 64 && NK * 16 * TS <= NS * 64, "one task per lane, inside the wave's own region");
      f32x4* tr = xch + (wave * NS) * 64;
#pragma unroll
      for (int so = 0; so < 4; ++so) {
        f32x4* te = tr + (4 * so + g) * TS + j;
        te[0] = f32x4{gb1[so][0], gb1[so][1], gb1[so][2], gb1[so][3]};
        te[16 * TS] = f32x4{gb2[so][0], gb2[so][1], gb2[so][2], gb2[so][3]};
        te[32 * TS] = f32x4{gW1c[so][0], gW1c[so][1], gW1c[so][2], gW1c[so][3]};
        if constexpr (!IS_PF) te[48 * TS] = gW3[so];
      }
      if (lane < NK * 16) {
        const f32x4* x = tr + lane * TS;
        const f32x4 even = ((x[0] + x[8]) + (x[4] + x[12])) + ((x[2] + x[10]) + (x[6] + x[14]));
        const f32x4 odd = ((x[1] + x[9]) + (x[5] + x[13])) + ((x[3] + x[11]) + (x[7] + x[15]));
        *reinterpret_cast<f32x4*>(sw + 4 * lane) = even + odd;      // kind | feature 16 so + 4 g + r: sw[64 kind + f]
      }
    }
#pragma unroll
    for (int so = 0; so < 4; ++so) {                               // (behind the reads of the region they overwrite)
#pragma unroll
      for (int c = 0; c < 4; ++c) xw[(S::XS_W2 + 4 * so + c) * 64] = gW2[so][c];
      xw[(S::XS_W1 + so) * 64] = gW1[so];
      if constexpr (WIDE) xw[(S::XS_W1B + so) * 64] = gW1b[so];
      if constexpr (IS_PF) xw[(S::XS_W3 + so) * 64] = gW3[so];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = 4 * g + r;
      const float b3 = row_sum16(db3[r]), dl = row_sum16(dls[r]);
      if (j == 0) {
        if constexpr (IS_PF) { sw[3 * H + o] = b3; sw[3 * H + 16 + o] = dl; }
        else sw[4 * H + o] = b3;
      }
    }
    if constexpr (LN) {                                            // dgamma | dbeta: the block's last 2 H floats
#pragma unroll
      for (int so = 0; so < 4; ++so)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float dg = row_sum16(ggm[so][r]), db = row_sum16(gbt[so][r]);
          if (j == 0) { sw[SC - 2 * H + 16 * so + 4 * g + r] = dg; sw[SC - H + 16 * so + 4 * g + r] = db; }
        }
    }
    WCLK(7)
    __syncthreads();
    // Fold by ownership: wave w owns the dW2 / dW1 / dW3 tiles of feature slice so == w, adds the four waves' values as
    // ((w0 + w1) + w2) + w3 and stores the sums straight into the partial row (64-byte runs per 16 lanes, the four dW2
    // tiles of a slice side by side: whole 256-byte rows).  Every float of [0, PS) is stored exactly once.
    float* prow = a.partial + (size_t)wg * a.p_stride;
    auto fold4 = [&](int slot) -> f32x4 {
      const f32x4* p = xch + slot * 64 + lane;
      f32x4 acc = p[0];
#pragma unroll
      for (int w = 1; w < WV_WAVES; ++w) acc += p[w * NS * 64];
      return acc;
    };
    {
      const int so = wave;
      f32x4 t2[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) t2[c] = fold4(S::XS_W2 + 4 * so + c);
      const f32x4 t1 = fold4(S::XS_W1 + so);
      f32x4 t1b = f32x4{0.f, 0.f, 0.f, 0.f}, t3 = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (WIDE) t1b = fold4(S::XS_W1B + so);
      if constexpr (IS_PF) t3 = fold4(S::XS_W3 + so);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * so + 4 * g + r;
#pragma unroll
        for (int c = 0; c < 4; ++c) prow[F_W2 + f * H + 16 * c + j] = t2[c][r];
        if (jv) prow[F_W1 + f * Dr + j] = t1[r];
        if (WIDE && jv2) prow[F_W1 + f * Dr + 16 + j] = t1b[r];
        if constexpr (IS_PF) {
          const int o = 4 * g + r;                                 // gW3 rows are outputs
          if constexpr (SDP) { if (sd_has(o)) prow[F_W3 + sd_row(o) * H + 16 * so + j] = t3[r]; }
          else if (o < O) prow[F_W3 + o * H + 16 * so + j] = t3[r];
        }
      }
    }
    for (int k = tid; k < SC; k += WV_THREADS) {
      float acc = xsc[k];
#pragma unroll
      for (int w = 1; w < WV_WAVES; ++w) acc += xsc[w * SC + k];
      const int q = k & (H - 1);
      int dst = -1;
      if (LN && k >= SC - 2 * H) dst = F_G + (k - (SC - 2 * H));    // gamma | beta: behind b1, in the plan's order
      else if (k < H) dst = F_B1 + q;
      else if (k < 2 * H) dst = F_B2 + q;
      else if (k < 3 * H) { if (f16) dst = F_W1 + q * Dr + 16; }
      else if constexpr (IS_PF) {
        const int o = q & 15;
        if (q < 16) { if constexpr (SDP) { if (sd_has(o)) dst = F_B3 + sd_row(o); } else if (o < O) dst = F_B3 + o; }
        else if (!CAT && !SDP && o < O) dst = F_LS + o;
      } else {
        if (k < 4 * H) dst = F_W3 + q;
        else if (q < O) dst = F_B3 + q;
      }
      if (dst >= 0) prow[dst] = acc;
    }
    // the row's tail: padding, and the logstd slot behind the value net's block
    for (int e = (IS_PF ? F_END : F_LS) + tid; e < PS; e += WV_THREADS) prow[e] = 0.0f;
  }
  WCLK(8)
#ifdef TRL_EXP_CLK
  __syncthreads();                                                 // (the stamps go where other threads stored padding)
  if (tid == 0) for (int ph = 0; ph < 24; ++ph) a.partial[(size_t)wg * a.p_stride + PS - 40 + ph] = clk_acc[ph];
#endif
  // ---- scalar statistics ----
  __syncthreads();
  double* sred = reinterpret_cast<double*>(lds);
  {
    const bool own = g == 0;
    const double v0 = wave_sum(own ? (double)stv[0] : 0.0), v1 = wave_sum(own ? (double)stv[1] : 0.0),
                 v6 = wave_sum(own ? (double)stv[6] : 0.0);
    const float v2 = wave_max(own ? stv[2] : -INFINITY), v3 = wave_max(own ? stv[3] : -INFINITY),
                v4 = wave_max(own ? stv[4] : -INFINITY), v5 = wave_max(own ? stv[5] : -INFINITY);
    double v7 = 0.0;                                   // CAT: the entropy sum rides in the row's free eighth column
    if constexpr (CAT || SDP) v7 = wave_sum(own ? (double)ent_sum : 0.0);
    if (lane == 0) {
      double* p = sred + wave * 8;
      p[0] = v0; p[1] = v1; p[2] = v2; p[3] = v3; p[4] = v4; p[5] = v5; p[6] = v6; p[7] = v7;
    }
    if constexpr (SDP) {                                // the wave's element statistics and its count of samples
      double e[SD_SCAL];
#pragma unroll
      for (int k = 0; k < 8; ++k) e[k] = (k & 2) ? (double)wave_max(sdst[k]) : wave_sum((double)sdst[k]);
      e[8] = wave_sum((double)sd_cnt);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < SD_SCAL; ++k) sred[WV_WAVES * 8 + wave * SD_SCAL + k] = k < 9 ? e[k] : 0.0;
      }
    }
  }
  __syncthreads();
  if (tid < 8) {
    double r = sred[tid];
    for (int w = 1; w < WV_WAVES; ++w) {
      const double o = sred[w * 8 + tid];
      r = (tid >= 2 && tid <= 5) ? fmax(r, o) : r + o;
    }
    a.scal_partial[(size_t)wg * 8 + tid] = r;
  }
  if constexpr (SDP) {                                  // second block of scalar rows, behind the n_wg x 8 of every head
    if (tid >= 64 && tid < 64 + SD_SCAL) {
      const int k = tid - 64;
      double r = sred[WV_WAVES * 8 + k];
      for (int w = 1; w < WV_WAVES; ++w) {
        const double o = sred[WV_WAVES * 8 + w * SD_SCAL + k];
        r = (k < 8 && (k & 2)) ? fmax(r, o) : r + o;
      }
      a.scal_partial[(size_t)a.n_wg * 8 + (size_t)wg * SD_SCAL + k] = r;
    }
  }
}

// ---------------------------------------------------------------- the gradient launch: one network pass per workgroup
// LNM: which of the two passes is normed (bit 0 the policy's, bit 1 the value function's; k_ppo_ln.hip)
template <int D, int H, int A, int ACT, bool CONTIG, bool RT, int HEAD = HEAD_GAUSS, int LNM = 0>
__global__ __launch_bounds__(WV_THREADS, 1) void ppo_grad_wave_kernel(PpoDev a) {
  static_assert(HEAD == HEAD_GAUSS || RT, "categorical / state-dependent-std head: runtime-dims tiles");
  constexpr int HEAD_VF = HEAD == HEAD_CAT ? HEAD_GAUSS : HEAD;   // the value pass of a categorical policy is the Gaussian's
  extern __shared__ __attribute__((aligned(16))) float lds[];
#ifdef TRL_CHAIN_CLK                                  /* tools/time_chains.py: when did this workgroup start and end (100 MHz) */
  const unsigned long long clk0 = wall_clock64();
#endif
  if ((int)blockIdx.x < a.n_pf) ppo_wave_pass<D, H, A, ACT, true, CONTIG, RT, HEAD, (LNM & 1) != 0>(a, lds, blockIdx.x, a.n_pf);
  else                          ppo_wave_pass<D, H, A, ACT, false, CONTIG, RT, HEAD_VF, (LNM & 2) != 0>(a, lds, blockIdx.x - a.n_pf, a.n_wg - a.n_pf);
#ifdef TRL_CHAIN_CLK
  __syncthreads();
  if (threadIdx.x == 0) {                             // the row's unused 8th scalar and the last three padding floats of the partial row
    a.scal_partial[(size_t)blockIdx.x * 8 + 7] = (double)wall_clock64();
    float* pad = a.partial + (size_t)blockIdx.x * a.p_stride + a.p_stride - 3;
    pad[0] = (float)(clk0 >> 40); pad[1] = (float)((clk0 >> 20) & 0xFFFFFull); pad[2] = (float)(clk0 & 0xFFFFFull);
  }
#endif
}

// Kernel generations that were built and measured on MI355X before this one (profiles/README.md): groups of
// 4 waves per tile with LDS rendezvous (85 us per 65 536-sample minibatch), this wave-per-tile kernel (64 us),
// and a PAIR of waves per tile with two waves per SIMD (75 us) -- on gfx950 the fp32 MFMA and the VALU do not
// overlap across the two waves of a SIMD (tools/ubench/mfma_valu.hip: an MFMA-only wave and a VALU-only wave
// on one SIMD take the SUM of their times), so a second wave only adds its duplicated loss / fetch work.
template <int D, int H, int A, int ACT, bool CONTIG, bool RT, int HEAD, int LNM = 0>
static int launch_ppo_v(const PpoDev& d, hipStream_t s) {
  using S = typename WvPickLN<D, H, A, HEAD, LNM != 0>::T;   // (a normed pass of either net: the larger layout)
  const size_t lds = S::LDS_FLOATS * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)ppo_grad_wave_kernel<D, H, A, ACT, CONTIG, RT, HEAD, LNM>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { trl_set_error("ppo_grad: hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
    attr_set = true;
  }
  hipLaunchKernelGGL((ppo_grad_wave_kernel<D, H, A, ACT, CONTIG, RT, HEAD, LNM>), dim3(d.n_wg), dim3(WV_THREADS), lds, s, d);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}
// N % 16 == 0 (every tile = 16 consecutive envs of one time row): scalar tile addressing; any other N: per-lane cells.
template <int D, int H, int A, int ACT, bool RT, int HEAD = HEAD_GAUSS, int LNM = 0>
static int launch_ppo(const PpoDev& d, hipStream_t s) {
  return (d.N % 16 == 0) ? launch_ppo_v<D, H, A, ACT, true, RT, HEAD, LNM>(d, s) : launch_ppo_v<D, H, A, ACT, false, RT, HEAD, LNM>(d, s);
}

// n_wg_pf: 0 = even split, [1, n_wg) = that many policy workgroups, n_wg = ALL workgroups run the policy, -1 = all run the
// value net (one network per launch: the two update chains of PPO are independent -- ppo.py:93-122 vs 41-91 -- and may run
// as separate, concurrent launch sequences)
static int resolve_pf_wgs(int n_wg, int n_wg_pf) { return n_wg_pf < 0 ? 0 : (n_wg_pf > 0 ? n_wg_pf : n_wg / 2); }

// The descriptor of a gradient launch, checked, as the kernels take it (p_stride is the caller's: by head, and by the norms).
// `aligned16`: the parameter blocks of the compile-time instantiation
static int ppo_dev_fill(const trl_ppo_batch_t* p, int head, bool aligned16, PpoDev& d) {
  // TRL_LOSS_REINFORCE: no critic anywhere -- an all-policy launch only, whose workgroups (ppo_wave_pass<IS_PF = true>) load
  // obs, acts, advs, adv_raw, pf_params and old_logp where it is set; rets / old_values / vf_params are the value pass's
  const bool reinforce = p->loss_mode == TRL_LOSS_REINFORCE;
  TRL_REQUIRE(p->obs && p->acts && p->advs && (p->rets || reinforce), "null rollout tensor");
  TRL_REQUIRE(p->loss_mode == TRL_LOSS_PPO_CLIP || p->loss_mode == TRL_LOSS_A2C || reinforce, "unknown loss_mode");
  TRL_REQUIRE(!reinforce || p->n_wg_pf == p->n_wg, "TRL_LOSS_REINFORCE runs in an all-policy launch only (n_wg_pf == n_wg)");
  TRL_REQUIRE(!reinforce || !p->clipped_value_loss, "TRL_LOSS_REINFORCE has no value loss: clipped_value_loss must be 0");
  TRL_REQUIRE(p->loss_mode != TRL_LOSS_PPO_CLIP || p->old_logp, "the clipped surrogate needs old_logp");
  TRL_REQUIRE(!p->clipped_value_loss || p->old_values, "the clipped value loss needs old_values");
  TRL_REQUIRE(p->adv_raw && (p->pf_params || p->vf_params) && p->partial && p->scal_partial, "null pointer");
  TRL_REQUIRE(p->rows_mb > 0 && p->N > 0, "empty minibatch");
  TRL_REQUIRE(p->n_wg >= 1 && (p->n_wg >= 2 || p->n_wg_pf == -1 || p->n_wg_pf == p->n_wg), "n_wg must be >= 2 (>= 1 for one network)");
  TRL_REQUIRE(p->n_wg_pf >= -1 && p->n_wg_pf <= p->n_wg, "n_wg_pf must be 0 (even split), in [1, n_wg], or -1 (value net only)");
  TRL_REQUIRE(p->n_wg_pf == p->n_wg || p->vf_params, "null value parameters");
  TRL_REQUIRE(p->n_wg_pf == -1 || p->pf_params, "null policy parameters");
  TRL_REQUIRE(p->n_global > 1.0, "n_global must exceed 1 (unbiased std)");
  const int D = p->D, H = p->H, A = p->A;
  TRL_REQUIRE(((uintptr_t)p->partial & 15) == 0 && (((uintptr_t)p->pf_params | (uintptr_t)p->vf_params) & 3) == 0,
              "partial rows must be 16-byte aligned, parameter blocks 4-byte aligned");
  TRL_REQUIRE(!aligned16 || (((uintptr_t)p->pf_params | (uintptr_t)p->vf_params) & 15) == 0,
              "parameter blocks of the benchmark shape must be 16-byte aligned");
  d.obs = p->obs; d.acts = p->acts; d.advs = p->advs; d.rets = p->rets; d.old_values = p->old_values;
  d.old_logp = p->old_logp; d.row_idx = p->row_idx; d.rows_mb = p->rows_mb; d.N = p->N;
  d.adv_raw = p->adv_raw; d.n_global = p->n_global; d.pf_params = p->pf_params; d.vf_params = p->vf_params;
  d.clip_para = p->clip_para; d.entropy_coeff = p->entropy_coeff;
  d.clipped_value_loss = p->clipped_value_loss; d.tanh_action = p->tanh_action;
  d.loss_mode = reinforce ? TRL_LOSS_A2C : p->loss_mode;       // (the policy pass of the two is one and the same)
  d.partial = p->partial; d.scal_partial = p->scal_partial; d.n_wg = p->n_wg;
  d.n_pf = resolve_pf_wgs(p->n_wg, p->n_wg_pf);
  d.D = D; d.A = A;
  if (head == HEAD_CAT) d.tanh_action = 0;            // acts is (rows, N, 1): the action index
  return TRL_OK;
}
