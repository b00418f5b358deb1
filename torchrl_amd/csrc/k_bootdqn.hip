// K19 -- Bootstrapped DQN (torchrl/algo/off_policy/bootstrapped_dqn.py:73-90, policies/discrete_policies.py:92-121):
// the K-head TD loss with a per-sample, per-head mask, per-env head selection / ensemble-vote actions, the head and mask
// draws, and the fold of the K heads' gradients at the trunk feature.
//
// Q values of all heads travel as one dense head-major stack (K, rows, A): head k's block is the (rows, A) output of a
// (grouped) dense-layer launch.  1 <= K <= 64 heads, 1 <= A <= 64 actions.  Streaming kernels: a thread per row, no float
// atomics, fixed row -> thread maps and fold orders (the same inputs give the same bits).
#include "trl_common.h"
#include "trl_philox.h"

#define BT_THREADS 256
#define BT_LOSS_THREADS 256
#define BT_MAX_K 64
#define BT_MAX_A 64

// one word of the Philox stream `tag` for (seed, counter, flat index g): element g & 3 of block g >> 2 (trl_cat_uniform's
// convention)
__device__ __forceinline__ uint32_t bt_word(int64_t seed, int64_t ctr, int64_t g, uint32_t tag) {
  uint32_t x[4];
  philox4x32_10((uint32_t)(ctr & 0xFFFFFFFFll), (uint32_t)((ctr >> 32) & 0xFFFFFFFFll), (uint32_t)((g >> 2) & 0xFFFFFFFFll),
                tag, (uint32_t)(seed & 0xFFFFFFFFll), (uint32_t)((seed >> 32) & 0xFFFFFFFFll), x);
  const int c = (int)(g & 3);
  return c == 0 ? x[0] : c == 1 ? x[1] : c == 2 ? x[2] : x[3];
}

// ---------------------------------------------------------------- actions
// head != NULL: action[n] = argmax_a q[head[n]][n][a] (a stored head outside [0, K) is clamped, never used as an index);
// head == NULL: argmax_a of the ensemble vote sum_k q[k][n][a], summed in ascending k in fp32 -- the SUMS are compared,
// not the means (a division by K can merge distinct sums); q_sel is that sum times 1 / K.  First maximum wins.
__global__ __launch_bounds__(BT_THREADS) void boot_act_kernel(const float* __restrict__ q, const int64_t* __restrict__ head,
                                                              int K, int N, int A, int64_t* __restrict__ action,
                                                              float* __restrict__ q_sel, float* __restrict__ onehot) {
  const int n = blockIdx.x * BT_THREADS + threadIdx.x;
  if (n >= N) return;
  int best = 0;
  float bv = -INFINITY;
  if (head) {
    const int64_t h64 = head[n];
    const int h = h64 < 0 ? 0 : (h64 >= K ? K - 1 : (int)h64);
    const float* row = q + ((size_t)h * N + n) * A;
    for (int a = 0; a < A; ++a) {
      const float s = row[a];
      if (q_sel) q_sel[(size_t)n * A + a] = s;
      if (s > bv) { bv = s; best = a; }
    }
  } else {
    const float inv_k = 1.0f / (float)K;
    for (int a = 0; a < A; ++a) {
      float s = 0.0f;
      for (int k = 0; k < K; ++k) s += q[((size_t)k * N + n) * A + a];
      if (q_sel) q_sel[(size_t)n * A + a] = s * inv_k;
      if (s > bv) { bv = s; best = a; }
    }
  }
  action[n] = best;
  if (onehot)
    for (int a = 0; a < A; ++a) onehot[(size_t)n * A + a] = (a == best) ? 1.0f : 0.0f;
}
extern "C" int trl_boot_act_i64(const float* q, const int64_t* head, int K, int N, int A, int64_t* action, float* q_sel,
                                float* onehot, void* stream) {
  TRL_REQUIRE(N >= 0 && K >= 1 && K <= BT_MAX_K && A >= 1 && A <= BT_MAX_A, "boot_act: 1 <= K <= 64 heads, 1 <= A <= 64 actions");
  if (N == 0) return TRL_OK;
  TRL_REQUIRE(q && action, "null pointer");
  hipLaunchKernelGGL(boot_act_kernel, dim3(trl_ceil_div(N, BT_THREADS)), dim3(BT_THREADS), 0, (hipStream_t)stream, q, head,
                     K, N, A, action, q_sel, onehot);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// ---------------------------------------------------------------- head draw
// head[n] = (uint64(x) * K) >> 32 where reset_mask[n] != 0 (everywhere when it is NULL); x: the word of
// (seed, counter, env_offset + n) under the head tag.  Other entries are not touched.
__global__ __launch_bounds__(BT_THREADS) void boot_heads_kernel(int64_t* __restrict__ head,
                                                                const uint8_t* __restrict__ reset_mask, int N, int K,
                                                                int64_t seed, int64_t ctr, int64_t env_offset) {
  const int n = blockIdx.x * BT_THREADS + threadIdx.x;
  if (n >= N) return;
  if (reset_mask && !reset_mask[n]) return;
  const uint32_t x = bt_word(seed, ctr, env_offset + n, TRL_TAG_BOOT_HEAD);
  head[n] = (int64_t)(((uint64_t)x * (uint64_t)K) >> 32);
}
extern "C" int trl_boot_heads_i64(int64_t* head, const uint8_t* reset_mask, int N, int K, int64_t seed, int64_t counter,
                                  int64_t env_offset, void* stream) {
  TRL_REQUIRE(N >= 0 && K >= 1 && K <= BT_MAX_K, "boot_heads: 1 <= K <= 64 heads");
  TRL_REQUIRE(env_offset >= 0, "boot_heads: the env offset is a global env index, not negative");
  if (N == 0) return TRL_OK;
  TRL_REQUIRE(head, "null pointer");
  hipLaunchKernelGGL(boot_heads_kernel, dim3(trl_ceil_div(N, BT_THREADS)), dim3(BT_THREADS), 0, (hipStream_t)stream, head,
                     reset_mask, N, K, seed, counter, env_offset);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// ---------------------------------------------------------------- mask draw
// out (N, K): out[n][k] = 1 if u01(x) < p else 0; x: the word of flat index (env_offset + n) K + k under the mask tag.
__global__ __launch_bounds__(BT_THREADS) void boot_masks_kernel(float* __restrict__ out, int64_t total, int64_t flat0,
                                                                float p, int64_t seed, int64_t ctr) {
  const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
  if (i >= total) return;
  out[i] = trl_u01(bt_word(seed, ctr, flat0 + i, TRL_TAG_BOOT_MASK)) < p ? 1.0f : 0.0f;
}
extern "C" int trl_boot_masks_f32(float* out, int N, int K, float p, int64_t seed, int64_t counter, int64_t env_offset,
                                  void* stream) {
  TRL_REQUIRE(N >= 0 && K >= 1 && K <= BT_MAX_K, "boot_masks: 1 <= K <= 64 heads");
  TRL_REQUIRE(env_offset >= 0, "boot_masks: the env offset is a global env index, not negative");
  if (N == 0) return TRL_OK;
  TRL_REQUIRE(out, "null pointer");
  const int64_t total = (int64_t)N * K;
  hipLaunchKernelGGL(boot_masks_kernel, dim3(trl_ceil_div(total, BT_THREADS)), dim3(BT_THREADS), 0, (hipStream_t)stream, out,
                     total, env_offset * (int64_t)K, p, seed, counter);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// ---------------------------------------------------------------- TD loss over K heads
// per (b, k): e = q[k][b][a_b] - (r_b + gamma (1 - d_b) max_a' q_next[k][b][a']);
// dq[k][b][a] = 2 masks[b][k] e / (K B) at a = a_b, exactly 0 elsewhere;
// sums: sum_b sum_k masks e^2 / K, sum masks, sum_b r_b -- also filed into ring row (update count mod slots), as K14 does.
//
// Up to 256 workgroups of 256 threads (the grid is a function of K B alone).  Item i = k B + b belongs to thread
// i mod (grid * 256): neighbouring threads read neighbouring rows of one head.  A thread adds its items in ascending i in
// double, then a wave butterfly, then the 4 waves in turn: the workgroup's three partial sums.  Nobody waits for anybody:
// thread 0 of a workgroup stores the partials (as 64-bit words, agent scope), then takes a ticket from an integer arrival
// counter with release / acquire ordering at agent scope; the workgroup that draws the LAST ticket -- every other
// workgroup's partials are visible to it by then -- reads all partials back, adds them in workgroup order, writes sums and
// the ring row, and sets the counter back to zero for the next launch (launches sharing a workspace are stream-ordered).
// The same inputs give the same bits whichever workgroup comes last.
struct BtRing { double* ring; const double* step; int slots; };
struct BtWork { unsigned int* arrive; unsigned long long* part; };      // part: (BT_LOSS_MAX_WGS, 3) doubles as bit patterns
#define BT_LOSS_MAX_WGS 256
#define BT_LOSS_WS_BYTES (16 + BT_LOSS_MAX_WGS * 3 * 8)
__device__ __forceinline__ double bt_block_sum(double v, double* smem) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) smem[wave] = v;
  __syncthreads();
  double r = 0.0;
  for (int w = 0; w < BT_LOSS_THREADS / 64; ++w) r += smem[w];
  return r;
}
__global__ __launch_bounds__(BT_LOSS_THREADS) void boot_td_kernel(const float* __restrict__ q, const float* __restrict__ qn,
                                                                  const int64_t* __restrict__ act,
                                                                  const float* __restrict__ act_f,
                                                                  const float* __restrict__ rew, const float* __restrict__ term,
                                                                  const float* __restrict__ masks, float gamma, int K, int B,
                                                                  int A, float* __restrict__ dq, double* __restrict__ sums,
                                                                  BtRing ring, BtWork work) {
  __shared__ double smem[BT_LOSS_THREADS / 64];
  __shared__ double s_part[3 * BT_LOSS_MAX_WGS];
  __shared__ int s_last;
  double sl = 0, sm = 0, sr = 0;
  const float scale = 2.0f / ((float)K * (float)B);
  const int64_t total = (int64_t)K * B;
  const int64_t stride = (int64_t)gridDim.x * BT_LOSS_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * BT_LOSS_THREADS + threadIdx.x; i < total; i += stride) {
    const int k = (int)(i / B), b = (int)(i - (int64_t)k * B);
    const size_t row = (size_t)i * A;                                  // (k B + b) A
    float mx = -INFINITY;
    for (int a = 0; a < A; ++a) mx = fmaxf(mx, qn[row + a]);
    int at;                                                            // K14's clamp: never an out-of-range index
    if (act) { const int64_t a = act[b]; at = a < 0 ? 0 : (a >= A ? A - 1 : (int)a); }
    else { const float a = act_f[b]; at = (a >= 0.0f) ? (a < (float)A ? (int)a : A - 1) : 0; }
    const float r = rew[b];
    const float e = q[row + at] - (r + gamma * (1.0f - term[b]) * mx);
    const float m = masks[(size_t)b * K + k];
    const float g = (m != 0.0f) ? scale * m * e : 0.0f;                // a masked-out entry is exactly zero (e may be inf)
    for (int a = 0; a < A; ++a) dq[row + a] = (a == at) ? g : 0.0f;
    if (m != 0.0f) sl += (double)m * ((double)e * (double)e);
    sm += (double)m;
    if (k == 0) sr += (double)r;
  }
  sl = bt_block_sum(sl, smem); sm = bt_block_sum(sm, smem); sr = bt_block_sum(sr, smem);
  const int n_wg = (int)gridDim.x;
  if (threadIdx.x == 0) {
    unsigned long long* mine = work.part + 3 * blockIdx.x;
    __hip_atomic_store(mine + 0, (unsigned long long)__double_as_longlong(sl), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + 1, (unsigned long long)__double_as_longlong(sm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + 2, (unsigned long long)__double_as_longlong(sr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // release: the three stores above come before the ticket; acquire: the reads below come after it
    const unsigned int ticket = __hip_atomic_fetch_add(work.arrive, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (ticket == (unsigned int)(n_wg - 1));
  }
  __syncthreads();
  if (!s_last) return;                                                 // (uniform over the workgroup)
  for (int j = threadIdx.x; j < 3 * n_wg; j += BT_LOSS_THREADS)
    s_part[j] = __longlong_as_double((long long)__hip_atomic_load(work.part + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  __syncthreads();
  if (threadIdx.x == 0) {
    double tl = 0, tm = 0, tr = 0;
    for (int w = 0; w < n_wg; ++w) { tl += s_part[3 * w]; tm += s_part[3 * w + 1]; tr += s_part[3 * w + 2]; }
    tl /= (double)K;
    sums[0] = tl; sums[1] = tm; sums[2] = tr;
    if (ring.ring) {
      const int64_t u = (int64_t)ring.step[0];
      double* rowp = ring.ring + 3 * (((u % ring.slots) + ring.slots) % ring.slots);
      rowp[0] = tl; rowp[1] = tm; rowp[2] = tr;
    }
    __hip_atomic_store(work.arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
  }
}
extern "C" int64_t trl_boot_td_loss_workspace(void) { return BT_LOSS_WS_BYTES; }
extern "C" int trl_boot_td_loss_f32(const float* q, const float* q_next, const int64_t* acts, const float* acts_f,
                                    const float* rewards, const float* terminals, const float* masks, float gamma, int K,
                                    int B, int A, float* dq, double* sums, double* ring, int slots,
                                    const double* update_count, void* workspace, void* stream) {
  TRL_REQUIRE(!acts != !acts_f, "boot_td_loss: exactly one of acts (int64) / acts_f (float)");
  TRL_REQUIRE(!ring || (slots > 0 && update_count), "boot_td_loss: ring without slots / counter");
  TRL_REQUIRE(B > 0 && K >= 1 && K <= BT_MAX_K && A >= 1 && A <= BT_MAX_A,
              "boot_td_loss: a non-empty batch, 1 <= K <= 64 heads, 1 <= A <= 64 actions");
  TRL_REQUIRE(q && q_next && rewards && terminals && masks && dq && sums && workspace, "null pointer");
  TRL_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "boot_td_loss: a 16-byte aligned workspace");
  const int64_t total = (int64_t)K * B;
  const int64_t want = (total + BT_LOSS_THREADS - 1) / BT_LOSS_THREADS;
  const int grid = (int)(want < BT_LOSS_MAX_WGS ? want : BT_LOSS_MAX_WGS);
  BtWork work{reinterpret_cast<unsigned int*>(workspace),
              reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + 16)};
  hipLaunchKernelGGL(boot_td_kernel, dim3(grid), dim3(BT_LOSS_THREADS), 0, (hipStream_t)stream, q, q_next, acts, acts_f, rewards,
                     terminals, masks, gamma, K, B, A, dq, sums, BtRing{ring, update_count, slots}, work);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// ---------------------------------------------------------------- fold of the K heads' gradients at the trunk feature
// dst[i] = src[0][i] + src[1][i] + ... + src[K - 1][i] over the n = B F elements of a (K, B, F) stack, ascending k, fp32.
__global__ __launch_bounds__(BT_THREADS) void boot_fold_kernel(const float* __restrict__ src, float* __restrict__ dst, int K,
                                                               int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
  if (i >= n) return;
  float s = src[i];
  for (int k = 1; k < K; ++k) s += src[(int64_t)k * n + i];
  dst[i] = s;
}
__global__ __launch_bounds__(BT_THREADS) void boot_fold4_kernel(const float4* __restrict__ src, float4* __restrict__ dst, int K,
                                                                int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
  if (i >= n4) return;
  float4 s = src[i];
  for (int k = 1; k < K; ++k) {
    const float4 t = src[(int64_t)k * n4 + i];
    s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
  }
  dst[i] = s;
}
extern "C" int trl_boot_fold_f32(const float* src, float* dst, int K, int64_t n, void* stream) {
  TRL_REQUIRE(n >= 0 && K >= 1 && K <= BT_MAX_K, "boot_fold: 1 <= K <= 64 heads");
  if (n == 0) return TRL_OK;
  TRL_REQUIRE(src && dst, "null pointer");
  TRL_REQUIRE(n <= (int64_t)BT_THREADS * 0x7FFFFFFF, "boot_fold: too many elements");
  if (n % 4 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
    hipLaunchKernelGGL(boot_fold4_kernel, dim3(trl_ceil_div(n / 4, BT_THREADS)), dim3(BT_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(src), reinterpret_cast<float4*>(dst), K, n / 4);
  } else {
    hipLaunchKernelGGL(boot_fold_kernel, dim3(trl_ceil_div(n, BT_THREADS)), dim3(BT_THREADS), 0, (hipStream_t)stream, src, dst,
                       K, n);
  }
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}

// ---------------------------------------------------------------- the heads' input gradient at a conv feature
// Over a conv trunk the K heads' first layers all read one flattened feature (B, F = C P).  Its gradient, summed over the
// heads and turned into the top conv layer's dZ, is ONE product with one long reduction:
//     out[b][p][c] = act'(y_top) * sum_k sum_j dZ_k[b][j] W_k[j][c P + p],      dZ_k = dy_k * gate_act'(y_k)  (y_k nullable)
// i.e. (B x K H1) . (K H1 x F) with the reduction index r = k H1 + j walking the heads back to back -- no (K, B, F) stack,
// no fold, no transposing launch.  H1 is the heads' first width, or A itself for heads without a hidden layer (dZ_k is
// then dq: one nonzero per row; nothing here depends on that).
//
// Exact fp32 on v_mfma_f32_32x32x2_f32, the tile code of k_gemm.hip in its plainest form: a workgroup of 4 waves owns a
// 64 x 128 tile of (b, f) (a wave: 32 rows x 2 blocks of 32 columns, every A value read from LDS feeds two MFMAs), the
// reduction walks panels of 32 through two LDS buffers with one barrier per panel: while the 32 MFMAs per wave of panel p
// run, panel p + 1 goes from registers to the other buffer (gated there) and the loads of panel p + 2 are issued.
// MFMA step (q, r) of lane half `hi` takes reduction index 8 q + 4 hi + r of the panel, as in k_gemm.hip.  No workgroup
// shares an output element with another: every element is one chain in ascending panel order, so the same inputs give the
// same bits.  All-zero rows of dZ give exact zeros (a sum of products with zero).  The epilogue applies act' of the top
// conv output -- laid out like the feature (b, c, p) when `gate_like_in`, like `out` (b, p, c) otherwise -- and stores in
// the (b, p, c) order the conv backward reads; those 4-byte stores are C floats apart, B F of them in all (the operand
// traffic is K H1 F floats per row tile).  Any B, H1, C, P >= 1, 1 <= K <= 64; W rows are read with 16-byte loads when
// F % 4 == 0 and every W_k is 16-byte aligned, else with predicated 4-byte loads.
#define BH_TM 64
#define BH_TN 128
#define BH_KP 32
#define BH_LDA (BH_KP + 4)
#define BH_LDB (BH_TN + 8)
struct BhPtrs { const float* dz[BT_MAX_K]; const float* gate[BT_MAX_K]; const float* w[BT_MAX_K]; };

__device__ __forceinline__ float bh_dact(int act, float y) {
  if (act == TRL_ACT_TANH) return 1.0f - y * y;
  if (act == TRL_ACT_RELU) return y > 0.0f ? 1.0f : 0.0f;
  return 1.0f;
}
__device__ __forceinline__ f32x16 bh_mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// GATE_MODE: 0 no head's dz is gated, 1 every head's is (with gate_act != NONE), 2 some are (general loop only)
template <int GATE_MODE>
__global__ __launch_bounds__(256) void boot_head_dx_kernel(BhPtrs ptrs, int K, int B, int H1, int C, int P, int gate_act,
                                                           const float* __restrict__ ytop, int top_act, int gate_like_in,
                                                           int vec_ok, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float As[2 * BH_TM * BH_LDA];
  __shared__ __attribute__((aligned(16))) float Bs[2 * BH_KP * BH_LDB];
  __shared__ const float* tab[3 * BT_MAX_K];                           // dz | gate | w of head k (one dynamic read of the arguments)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int F = C * P, R = K * H1;
  const int row_tiles = (B + BH_TM - 1) / BH_TM;
  // workgroups are dealt round-robin to the 8 XCDs: renumber so that the row tiles that share W's columns share an L2
  int bid = blockIdx.x;
  const int nb = gridDim.x;
  if ((nb & 7) == 0) bid = (bid & 7) * (nb >> 3) + (bid >> 3);
  const int ct = bid / row_tiles, rt = bid - ct * row_tiles;
  const int m0 = rt * BH_TM, n0 = ct * BH_TN;
  if (tid < 3 * BT_MAX_K) {
    const int which = tid / BT_MAX_K, k = tid - which * BT_MAX_K;
    const float* p = nullptr;
    if (k < K) p = which == 0 ? ptrs.dz[k] : (which == 1 ? ptrs.gate[k] : ptrs.w[k]);
    tab[tid] = p;
  }
  __syncthreads();

  // Registers of one panel in flight: the raw loads only -- the gate is applied when they are written to LDS, a whole
  // panel of MFMAs later, so nothing waits for memory between the issue of the loads and the MFMAs that cover them.
  float ra[8], rg[8];
  f32x4 rb[4];
  bool gated = false;
  const int a_k = tid & 31, a_m = tid >> 5;                            // A slot: reduction index a_k, rows a_m + 8 t
  const int b_n = n0 + 4 * (tid & 31), b_k = tid >> 5;                 // B slot: columns b_n .. + 3, reduction rows b_k + 8 t
  auto fetch = [&](int r0) {
    {
      const int r = r0 + a_k;
      const bool rok = r < R;
      const int kk = rok ? r / H1 : 0, j = rok ? r - kk * H1 : 0;
      const float* dzp = tab[kk];
      const float* gp = tab[BT_MAX_K + kk];
      gated = rok && gp != nullptr && gate_act != TRL_ACT_NONE;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int m = m0 + a_m + 8 * t;
        const bool ok = rok && m < B;
        const size_t idx = ok ? (size_t)m * H1 + j : 0;
        ra[t] = ok ? dzp[idx] : 0.0f;
        rg[t] = (ok && gated) ? gp[idx] : 1.0f;
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int r = r0 + b_k + 8 * t;
      const bool rok = r < R;
      const int kk = rok ? r / H1 : 0, j = rok ? r - kk * H1 : 0;
      const float* wp = tab[2 * BT_MAX_K + kk] + (size_t)j * F;
      if (rok && vec_ok && b_n + 3 < F) {
        rb[t] = *reinterpret_cast<const f32x4*>(wp + b_n);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool ok = rok && b_n + e < F;
          rb[t][e] = ok ? wp[ok ? b_n + e : 0] : 0.0f;
        }
      }
    }
  };
  auto stash = [&](int buf) {
    float* A_ = As + buf * (BH_TM * BH_LDA);
    float* B_ = Bs + buf * (BH_KP * BH_LDB);
#pragma unroll
    for (int t = 0; t < 8; ++t) A_[(a_m + 8 * t) * BH_LDA + a_k] = gated ? ra[t] * bh_dact(gate_act, rg[t]) : ra[t];
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(B_ + (b_k + 8 * t) * BH_LDB + 4 * (tid & 31)) = rb[t];
  };

  const int i = lane & 31, hi = lane >> 5, wm = wave & 1, wn = wave >> 1;
  f32x16 acc[2];
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc[0][e] = 0.0f; acc[1][e] = 0.0f; }
  auto group = [&](int buf, int q) {                                   // the 8 MFMAs of 8-k group q of the panel in `buf`
    const f32x4 av = *reinterpret_cast<const f32x4*>(As + buf * (BH_TM * BH_LDA) + (32 * wm + i) * BH_LDA + 8 * q + 4 * hi);
    const float* bp = Bs + buf * (BH_KP * BH_LDB) + (8 * q + 4 * hi) * BH_LDB + 64 * wn + i;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc[0] = bh_mfma(av[r], bp[r * BH_LDB], acc[0]);
      acc[1] = bh_mfma(av[r], bp[r * BH_LDB + 32], acc[1]);
    }
  };
  // two panel buffers, one barrier per panel: while the MFMAs of panel p run from buffer p & 1, the registers that hold
  // panel p + 1 (fetched one panel earlier) go to the other buffer and the loads of panel p + 2 are issued
  const int np = (R + BH_KP - 1) / BH_KP;
  // Interior tiles (all 64 rows and 128 columns in range, 16-byte loads legal, every head gated or none) walk their WHOLE
  // panels in a loop of their own that holds nothing but unconditional loads, LDS traffic and MFMAs: with the predicated
  // loads of the general loop in the same body the compiler waits for all outstanding loads right where they are issued
  // (k_gemm.hip has the same split).  Same panels, same k order: the same bits on either route.
  const bool whole = m0 + BH_TM <= B && n0 + BH_TN <= F && vec_ok != 0 && GATE_MODE != 2;
  const int nw = whole ? R / BH_KP : 0;
  if (nw > 0) {
    auto fetch_whole = [&](int r0) {
      {
        const int r = r0 + a_k;
        const int kk = r / H1, j = r - kk * H1;
        const size_t at = (size_t)(m0 + a_m) * H1 + j;
        const float* dzp = tab[kk] + at;
        const float* gp = GATE_MODE == 1 ? tab[BT_MAX_K + kk] + at : nullptr;     // (mode 0: the entries are NULL)
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          ra[t] = dzp[(size_t)(8 * t) * H1];
          if (GATE_MODE == 1) rg[t] = gp[(size_t)(8 * t) * H1];
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int r = r0 + b_k + 8 * t;
        const int kk = r / H1, j = r - kk * H1;
        rb[t] = *reinterpret_cast<const f32x4*>(tab[2 * BT_MAX_K + kk] + (size_t)j * F + b_n);
      }
    };
    auto stash_whole = [&](int buf) {
      float* A_ = As + buf * (BH_TM * BH_LDA);
      float* B_ = Bs + buf * (BH_KP * BH_LDB);
#pragma unroll
      for (int t = 0; t < 8; ++t)
        A_[(a_m + 8 * t) * BH_LDA + a_k] = GATE_MODE == 1 ? ra[t] * bh_dact(gate_act, rg[t]) : ra[t];
#pragma unroll
      for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(B_ + (b_k + 8 * t) * BH_LDB + 4 * (tid & 31)) = rb[t];
    };
    fetch_whole(0);
    stash_whole(0);
    if (nw > 1) fetch_whole(BH_KP);
    __syncthreads();
    for (int p = 0; p < nw; ++p) {
      const int cur = p & 1;
      group(cur, 0); group(cur, 1);
      if (p + 1 < nw) stash_whole(cur ^ 1);
      if (p + 2 < nw) fetch_whole((p + 2) * BH_KP);
      group(cur, 2); group(cur, 3);
      __syncthreads();
    }
  }
  if (nw < np) {                                                       // general loop: panels [nw, np), edge-capable loads
    fetch(nw * BH_KP);
    stash(nw & 1);
    if (nw + 1 < np) fetch((nw + 1) * BH_KP);
    __syncthreads();
    for (int p = nw; p < np; ++p) {
      const int cur = p & 1;
      group(cur, 0); group(cur, 1);
      if (p + 1 < np) stash(cur ^ 1);
      if (p + 2 < np) fetch((p + 2) * BH_KP);
      group(cur, 2); group(cur, 3);
      __syncthreads();
    }
  }
  // epilogue: lane (i, hi) owns column f of rows 4 hi + (e & 3) + 8 (e >> 2) of each of the wave's two blocks
#pragma unroll
  for (int bb = 0; bb < 2; ++bb) {
    const int f = n0 + 64 * wn + 32 * bb + i;
    if (f >= F) continue;
    const int c = f / P, pp = f - c * P;
    const size_t o_col = (size_t)pp * C + c;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int m = m0 + 32 * wm + 4 * hi + (e & 3) + 8 * (e >> 2);
      if (m < B) {
        const size_t o = (size_t)m * F + o_col;
        const float y = ytop[gate_like_in ? (size_t)m * F + f : o];
        out[o] = acc[bb][e] * bh_dact(top_act, y);
      }
    }
  }
}

extern "C" int trl_boot_head_dx_supported(int K, int B, int H1, int C, int P) {
  if (K < 1 || K > BT_MAX_K || B < 1 || H1 < 1 || C < 1 || P < 1) return 0;
  if ((int64_t)C * P > 0x3FFFFFFF || (int64_t)K * H1 > 0x3FFFFFFF) return 0;
  const int64_t tiles = (((int64_t)C * P + BH_TN - 1) / BH_TN) * (((int64_t)B + BH_TM - 1) / BH_TM);
  return tiles <= 0x7FFFFFFF ? 1 : 0;
}
extern "C" int trl_boot_head_dx_f32(int K, const float* const* dz, const float* const* dz_gate, int gate_act,
                                    const float* const* w, int B, int H1, int C, int P, const float* y_top, int top_act,
                                    int gate_like_in, float* out, void* stream) {
  TRL_REQUIRE(trl_boot_head_dx_supported(K, B, H1, C, P),
              "boot_head_dx: 1 <= K <= 64 heads, B, H1, C, P >= 1, C P and K H1 below 2^30");
  TRL_REQUIRE(dz && w && y_top && out, "null pointer");
  const auto known = [](int a) { return a == TRL_ACT_TANH || a == TRL_ACT_RELU || a == TRL_ACT_NONE; };
  TRL_REQUIRE(known(gate_act) && known(top_act), "unknown activation");
  BhPtrs ptrs;
  const int F = C * P;
  int vec_ok = (F % 4 == 0);
  for (int k = 0; k < BT_MAX_K; ++k) {
    ptrs.dz[k] = k < K ? dz[k] : nullptr;
    ptrs.gate[k] = (k < K && dz_gate) ? dz_gate[k] : nullptr;
    ptrs.w[k] = k < K ? w[k] : nullptr;
    if (k < K) {
      TRL_REQUIRE(dz[k] && w[k], "boot_head_dx: null head operand");
      if (reinterpret_cast<uintptr_t>(w[k]) & 15) vec_ok = 0;
    }
  }
  int n_gated = 0;
  for (int k = 0; k < K; ++k) n_gated += (ptrs.gate[k] != nullptr && gate_act != TRL_ACT_NONE);
  const int grid = trl_ceil_div(F, BH_TN) * trl_ceil_div(B, BH_TM);
  const int like_in = gate_like_in ? 1 : 0;
  if (n_gated == 0)
    hipLaunchKernelGGL(boot_head_dx_kernel<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, ptrs, K, B, H1, C, P, gate_act,
                       y_top, top_act, like_in, vec_ok, out);
  else if (n_gated == K)
    hipLaunchKernelGGL(boot_head_dx_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, ptrs, K, B, H1, C, P, gate_act,
                       y_top, top_act, like_in, vec_ok, out);
  else
    hipLaunchKernelGGL(boot_head_dx_kernel<2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, ptrs, K, B, H1, C, P, gate_act,
                       y_top, top_act, like_in, vec_ok, out);
  TRL_LAUNCH_CHECK();
  return TRL_OK;
}
