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
template <int D, int H, int A, int ACT, bool IS_PF, bool CONTIG, bool RT, int HEAD = HEAD_GAUSS>
__device__ void ppo_wave_pass(const PpoDev& a, float* lds, int wg_in_net, int n_wg_net) {
  using S = typename WvPick<D, H, A, HEAD>::T;
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
  const int F_W1 = 0, F_B1 = H * Dr, F_W2 = F_B1 + H, F_B2 = F_W2 + H * H, F_W3 = F_B2 + H, F_B3 = F_W3 + OH * H,
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
  constexpr int KB_LO = H * (WIDE ? 18 : RT ? 2 : D) / WV_THREADS, KB_HI = (H * D + 2 * H - 1) / WV_THREADS;
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const int e = tid + WV_THREADS * k;
    img[e] = im[k];
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
    f32x4 wq[4], bq;                                   // W2 operand slices / b2 slice of the NEXT L2 output slice
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
#pragma unroll
    for (int so = 0; so < 4; ++so)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        h1[so][r] = act_fn<ACT>(h1[so][r]);
        H1S[(16 * so + 4 * g + r) * LDT + j] = h1[so][r];        // H1^T[f][s] for dW2
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
#pragma unroll
      for (int r = 0; r < 4; ++r) h2[so][r] = act_fn<ACT>(acc[r]);
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
#pragma unroll
      for (int sl = 0; sl < 4; sl += 2)
#pragma unroll
        for (int r = 0; r < 4; ++r) { oa = mfma16(w3h[sl][r], h2[sl][r], oa); ob = mfma16(w3h[sl + 1][r], h2[sl + 1][r], ob); }
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
      PIN_DS();
      // dH2^T[f][s] = sum_o W3[o][f] dout[o][s];  dZ2 = dH2 * act'(H2)
#pragma unroll
      for (int so = 0; so < 4; ++so) dz2[so] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int so = 0; so < 4; ++so) dz2[so] = mfma16(w3t[so][r], dout[r], dz2[so]);
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
#pragma unroll
    for (int so = 0; so < 4; ++so)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dz1[so][r] *= act_grad<ACT>(h1[so][r]);
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
      if (k < H) dst = F_B1 + q;
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

// ---------------------------------------------------------------- the gradient launch: one network pass per workgroup
template <int D, int H, int A, int ACT, bool CONTIG, bool RT, int HEAD = HEAD_GAUSS>
__global__ __launch_bounds__(WV_THREADS, 1) void ppo_grad_wave_kernel(PpoDev a) {
  static_assert(HEAD == HEAD_GAUSS || RT, "categorical / state-dependent-std head: runtime-dims tiles");
  constexpr int HEAD_VF = HEAD == HEAD_CAT ? HEAD_GAUSS : HEAD;   // the value pass of a categorical policy is the Gaussian's
  extern __shared__ __attribute__((aligned(16))) float lds[];
#ifdef TRL_CHAIN_CLK                                  /* tools/time_chains.py: when did this workgroup start and end (100 MHz) */
  const unsigned long long clk0 = wall_clock64();
#endif
  if ((int)blockIdx.x < a.n_pf) ppo_wave_pass<D, H, A, ACT, true, CONTIG, RT, HEAD>(a, lds, blockIdx.x, a.n_pf);
  else                          ppo_wave_pass<D, H, A, ACT, false, CONTIG, RT, HEAD_VF>(a, lds, blockIdx.x - a.n_pf, a.n_wg - a.n_pf);
#ifdef TRL_CHAIN_CLK
  __syncthreads();
  if (threadIdx.x == 0) {                             // the row's unused 8th scalar and the last three padding floats of the partial row
    a.scal_partial[(size_t)blockIdx.x * 8 + 7] = (double)wall_clock64();
    float* pad = a.partial + (size_t)blockIdx.x * a.p_stride + a.p_stride - 3;
    pad[0] = (float)(clk0 >> 40); pad[1] = (float)((clk0 >> 20) & 0xFFFFFull); pad[2] = (float)(clk0 & 0xFFFFFull);
  }
#endif
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
static int ppo_stride_for(int D, int H, int A, int head) {
  if (head == HEAD_GAUSS && SHAPE_IS(17, 64, 6)) return PpoShape<17, 64, 6>::P_STRIDE;
  if (head_shape_ok(head, D, H, A)) {
    const int p_pf = ppo_p_pf(D, H, A, head), p_vf = ppo_p_vf(D, H);
    return ((p_pf > p_vf ? p_pf : p_vf) + 63) & ~63;
  }
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

// Kernel generations that were built and measured on MI355X before this one (profiles/README.md): groups of
// 4 waves per tile with LDS rendezvous (85 us per 65 536-sample minibatch), this wave-per-tile kernel (64 us),
// and a PAIR of waves per tile with two waves per SIMD (75 us) -- on gfx950 the fp32 MFMA and the VALU do not
// overlap across the two waves of a SIMD (tools/ubench/mfma_valu.hip: an MFMA-only wave and a VALU-only wave
// on one SIMD take the SUM of their times), so a second wave only adds its duplicated loss / fetch work.
template <int D, int H, int A, int ACT, bool CONTIG, bool RT, int HEAD>
static int launch_ppo_v(const PpoDev& d, hipStream_t s) {
  using S = typename WvPick<D, H, A, HEAD>::T;
  const size_t lds = S::LDS_FLOATS * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)ppo_grad_wave_kernel<D, H, A, ACT, CONTIG, RT, HEAD>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { trl_set_error("ppo_grad: hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
    attr_set = true;
  }
  hipLaunchKernelGGL((ppo_grad_wave_kernel<D, H, A, ACT, CONTIG, RT, HEAD>), dim3(d.n_wg), dim3(WV_THREADS), lds, s, d);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}
// N % 16 == 0 (every tile = 16 consecutive envs of one time row): scalar tile addressing; any other N: per-lane cells.
template <int D, int H, int A, int ACT, bool RT, int HEAD = HEAD_GAUSS>
static int launch_ppo(const PpoDev& d, hipStream_t s) {
  return (d.N % 16 == 0) ? launch_ppo_v<D, H, A, ACT, true, RT, HEAD>(d, s) : launch_ppo_v<D, H, A, ACT, false, RT, HEAD>(d, s);
}

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
// n_wg_pf: 0 = even split, [1, n_wg) = that many policy workgroups, n_wg = ALL workgroups run the policy, -1 = all run the
// value net (one network per launch: the two update chains of PPO are independent -- ppo.py:93-122 vs 41-91 -- and may run
// as separate, concurrent launch sequences)
static int resolve_pf_wgs(int n_wg, int n_wg_pf) { return n_wg_pf < 0 ? 0 : (n_wg_pf > 0 ? n_wg_pf : n_wg / 2); }

static int ppo_grad_launch(const trl_ppo_batch_t* p, void* stream, int head = HEAD_GAUSS) {
  if (!p) { trl_set_error("ppo_grad: null descriptor"); return TRL_EINVAL; }
  if (!head_supported(head, p->D, p->H, p->A, p->act)) {      // (the benchmark shape is inside the Gaussian's range)
    trl_set_error("ppo_%sgrad: shape D=%d H=%d A=%d act=%d not instantiated (H == 64, 2 <= D <= 32, %d <= A <= %d, Tanh / ReLU)",
                  HEADS[head].tag, p->D, p->H, p->A, p->act, HEADS[head].a_min, HEADS[head].a_max);
    return TRL_EUNSUPPORTED;
  }
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
  TRL_REQUIRE(head != HEAD_GAUSS || !SHAPE_IS(17, 64, 6) || (((uintptr_t)p->pf_params | (uintptr_t)p->vf_params) & 15) == 0,
              "parameter blocks of the benchmark shape must be 16-byte aligned");
  PpoDev d;
  d.obs = p->obs; d.acts = p->acts; d.advs = p->advs; d.rets = p->rets; d.old_values = p->old_values;
  d.old_logp = p->old_logp; d.row_idx = p->row_idx; d.rows_mb = p->rows_mb; d.N = p->N;
  d.adv_raw = p->adv_raw; d.n_global = p->n_global; d.pf_params = p->pf_params; d.vf_params = p->vf_params;
  d.clip_para = p->clip_para; d.entropy_coeff = p->entropy_coeff;
  d.clipped_value_loss = p->clipped_value_loss; d.tanh_action = p->tanh_action;
  d.loss_mode = reinforce ? TRL_LOSS_A2C : p->loss_mode;       // (the policy pass of the two is one and the same)
  d.partial = p->partial; d.scal_partial = p->scal_partial; d.n_wg = p->n_wg;
  d.n_pf = resolve_pf_wgs(p->n_wg, p->n_wg_pf);
  d.D = D; d.A = A;
  hipStream_t s = (hipStream_t)stream;
  d.p_stride = ppo_stride_for(D, H, A, head);
  if (head == HEAD_CAT) d.tanh_action = 0;            // acts is (rows, N, 1): the action index
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
                         const float* pf_params, float* grads, double* info, void* stream, int head) {
  TRL_REQUIRE(partial && scal_partial && grads && info, "null pointer");
  TRL_REQUIRE(n_wg >= 2 && n_wg_pf >= 0 && n_wg_pf < n_wg, "need n_wg >= 2 and n_wg_pf in [0, n_wg)");
  const int ps = ppo_stride_for(D, H, A, head);
  if (ps < 0) return ps;
  const int p_pf = ppo_p_pf(D, H, A, head), p_vf = ppo_p_vf(D, H);
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

static int reduce_adam_workspace(int D, int H, int A, int head) {
  const int ps = ppo_stride_for(D, H, A, head);
  if (ps < 0) return ps;
  return 16 + 4 * trl_ceil_div(ps, RED_CHUNK);       // header + {ss, epoch} per block and network
}
extern "C" int trl_ppo_reduce_adam_workspace(int D, int H, int A) { return reduce_adam_workspace(D, H, A, HEAD_GAUSS); }
extern "C" int trl_ppo_cat_reduce_adam_workspace(int D, int H, int A) { return reduce_adam_workspace(D, H, A, HEAD_CAT); }
extern "C" int trl_ppo_sd_reduce_adam_workspace(int D, int H, int A) { return reduce_adam_workspace(D, H, A, HEAD_SD); }

static int launch_reduce_adam(const float* partial, const double* scal_partial, int n_wg, int n_wg_pf, int D, int H, int A,
                              float* grads, double* info, const trl_adam_t* adam, float* workspace, const XrArgs* xr,
                              int max_blocks, void* stream, int only_net = -1, int head = HEAD_GAUSS) {
  TRL_REQUIRE(partial && scal_partial && grads && info && workspace, "null pointer");
  TRL_REQUIRE(only_net >= 0 ? n_wg >= 1 : (n_wg >= 2 && n_wg_pf >= 0 && n_wg_pf < n_wg), "need n_wg >= 2 and n_wg_pf in [0, n_wg)");
  const int ps = ppo_stride_for(D, H, A, head);
  if (ps < 0) return ps;
  AdamDev d;
  int rc = fill_adam(adam, d);
  if (rc) return rc;
  const int p_pf = ppo_p_pf(D, H, A, head), p_vf = ppo_p_vf(D, H);
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
