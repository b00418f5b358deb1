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
