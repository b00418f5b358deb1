// Global-norm clip + RMSprop / SGD step (include/trl_hip.h trl_clip_step_f32): the second optimiser launch behind the call
// sites of trl_clip_adam_f32.  clip_grad_norm_ exactly as clip_adam_kernel (k_ppo.hip) does it -- every block recomputes the
// group norms itself, same summation order, so norms_out carries the same bits -- followed by single-tensor
// torch.optim.RMSprop / torch.optim.SGD arithmetic, one thread per element.  No in-kernel wait of any kind.
#include "trl_common.h"

struct OptDev {
  float* params; const float* grads; float* s0; float* s1; float* s2;
  int n_groups; int off[5]; float lr[4];
  float max_norm, grad_scale;
  float* norms_out;
  double* step_state;         // {steps taken, -, -, block counter} or null; this launch advances slot 0 only
  const float* device_lr;     // per-group learning rates on the device, or null (then lr[])
  float alpha, eps, momentum, dampening, weight_decay;
  int nesterov, first_step;   // first_step: SGD's `buf = g` rule when there is no step state to read it from
  int self_tick;              // small grids: the last block to have read step_state advances it (no tick launch)
};

// KIND: TRL_OPT_RMSPROP / TRL_OPT_SGD.  MOM: a momentum buffer exists.  CENT: RMSprop's grad_avg exists.
template <int KIND, bool MOM, bool CENT>
__global__ __launch_bounds__(256) void clip_step_kernel(OptDev a) {
  __shared__ float s_part[4][4];
  __shared__ float s_coef[4];
  __shared__ int s_first;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    s_first = a.step_state ? (a.step_state[0] == 0.0 ? 1 : 0) : a.first_step;
    if (a.step_state && a.self_tick) {
      // clip_adam_kernel's rule: every block counts itself in AFTER its read of the state (release); the block that
      // completes the count has therefore seen all reads done (acquire) and advances the state for the next launch.  The
      // counter lives in the 4th double and is back at zero when the kernel ends.
      unsigned* cnt = reinterpret_cast<unsigned*>(a.step_state + 3);
      const unsigned before = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      if (before == gridDim.x - 1) {
        a.step_state[0] += 1.0;
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
  const int e = blockIdx.x * 256 + tid;
  if (e >= a.off[a.n_groups]) return;
  // every load of the element first, then the arithmetic
  const float g_raw = a.grads[e], p = a.params[e];
  float st0 = 0.f, st1 = 0.f, st2 = 0.f;
  if constexpr (KIND == TRL_OPT_RMSPROP) {
    st0 = a.s0[e];
    if constexpr (MOM) st1 = a.s1[e];
    if constexpr (CENT) st2 = a.s2[e];
  } else {
    if constexpr (MOM) st0 = a.s0[e];
  }
  int g = 0;
  while (e >= a.off[g + 1]) ++g;
  const float lr = a.device_lr ? a.device_lr[g] : a.lr[g];
  float gr = g_raw * a.grad_scale * s_coef[g];
  if (a.weight_decay != 0.0f) gr += a.weight_decay * p;
  if constexpr (KIND == TRL_OPT_RMSPROP) {
    const float sq = a.alpha * st0 + (1.0f - a.alpha) * gr * gr;
    a.s0[e] = sq;
    float avg;
    if constexpr (CENT) {
      const float ga = st2 + (gr - st2) * (1.0f - a.alpha);
      a.s2[e] = ga;
      avg = sqrtf(sq - ga * ga) + a.eps;
    } else {
      avg = sqrtf(sq) + a.eps;
    }
    if constexpr (MOM) {
      const float buf = a.momentum * st1 + gr / avg;
      a.s1[e] = buf;
      a.params[e] = p - lr * buf;
    } else {
      a.params[e] = p - lr * (gr / avg);
    }
  } else {
    if constexpr (MOM) {
      const float buf = s_first ? gr : a.momentum * st0 + (1.0f - a.dampening) * gr;
      a.s0[e] = buf;
      gr = a.nesterov ? gr + a.momentum * buf : buf;
    }
    a.params[e] = p - lr * gr;
  }
}

// advances the device-resident step count after clip_step_kernel has read it (stream order: every block is done)
__global__ void step_tick_kernel(double* __restrict__ st) { st[0] += 1.0; }

static int fill_opt(const trl_opt_t* p, OptDev& d) {
  if (!p) { trl_set_error("clip_step: null descriptor"); return TRL_EINVAL; }
  TRL_REQUIRE(p->kind == TRL_OPT_RMSPROP || p->kind == TRL_OPT_SGD, "kind must be TRL_OPT_RMSPROP or TRL_OPT_SGD");
  TRL_REQUIRE(p->params && p->grads, "null pointer");
  TRL_REQUIRE(p->n_groups >= 1 && p->n_groups <= 4, "n_groups must be 1..4");
  const bool mom = p->momentum != 0.0f;
  if (p->kind == TRL_OPT_RMSPROP) {
    TRL_REQUIRE(p->state0, "RMSprop needs state0 (square_avg)");
    TRL_REQUIRE(!mom || p->state1, "RMSprop with momentum needs state1 (momentum_buffer)");
    TRL_REQUIRE(!p->centered || p->state2, "centered RMSprop needs state2 (grad_avg)");
  } else {
    TRL_REQUIRE(!mom || p->state0, "SGD with momentum needs state0 (momentum_buffer)");
    TRL_REQUIRE(!p->nesterov || (p->momentum > 0.0f && p->dampening == 0.0f),
                "Nesterov momentum requires a momentum and zero dampening");
  }
  d.params = p->params; d.grads = p->grads; d.s0 = p->state0; d.s1 = p->state1; d.s2 = p->state2;
  d.n_groups = p->n_groups; d.off[0] = 0;
  for (int g = 0; g < p->n_groups; ++g) {
    TRL_REQUIRE(p->group_sizes[g] >= 0, "negative group size");
    TRL_REQUIRE((int64_t)d.off[g] + p->group_sizes[g] <= INT32_MAX, "more than 2^31 - 1 elements");
    d.off[g + 1] = d.off[g] + p->group_sizes[g];
    d.lr[g] = p->group_lr[g];
  }
  for (int g = p->n_groups; g < 4; ++g) { d.off[g + 1] = d.off[g]; d.lr[g] = 0.f; }
  d.max_norm = p->max_norm; d.grad_scale = p->grad_scale; d.norms_out = p->norms_out;
  d.step_state = p->step_state; d.device_lr = p->device_lr;
  d.alpha = p->alpha; d.eps = p->eps; d.momentum = p->momentum; d.dampening = p->dampening;
  d.weight_decay = p->weight_decay; d.nesterov = p->nesterov; d.first_step = p->first_step;
  d.self_tick = 0;
  return TRL_OK;
}

#define TICK_PENDING 0x70000001                    /* clip_step_launch: the step count still has to be advanced */
#define NOTHING_STEPPED 0x70000002                 /* clip_step_launch: no element, no launch, the step count stands */
static int clip_step_launch(const trl_opt_t* p, void* stream, bool tick_here) {
  OptDev d;
  int rc = fill_opt(p, d);
  if (rc) return rc;
  const int total = d.off[p->n_groups];
  if (total == 0) return NOTHING_STEPPED;
  const int blocks = trl_ceil_div(total, 256);
  d.self_tick = (d.step_state && blocks <= 128) ? 1 : 0;       // (clip_adam_launch's threshold and its reasons)
  const dim3 grid(blocks), block(256);
  hipStream_t s = (hipStream_t)stream;
  const bool mom = p->momentum != 0.0f;
  if (p->kind == TRL_OPT_RMSPROP) {
    if (mom && p->centered) hipLaunchKernelGGL((clip_step_kernel<TRL_OPT_RMSPROP, true, true>), grid, block, 0, s, d);
    else if (mom) hipLaunchKernelGGL((clip_step_kernel<TRL_OPT_RMSPROP, true, false>), grid, block, 0, s, d);
    else if (p->centered) hipLaunchKernelGGL((clip_step_kernel<TRL_OPT_RMSPROP, false, true>), grid, block, 0, s, d);
    else hipLaunchKernelGGL((clip_step_kernel<TRL_OPT_RMSPROP, false, false>), grid, block, 0, s, d);
  } else {
    if (mom) hipLaunchKernelGGL((clip_step_kernel<TRL_OPT_SGD, true, false>), grid, block, 0, s, d);
    else hipLaunchKernelGGL((clip_step_kernel<TRL_OPT_SGD, false, false>), grid, block, 0, s, d);
  }
  TRL_LAUNCH_CHECK();
  if (d.step_state && !d.self_tick) {
    if (!tick_here) return TICK_PENDING;             // the caller's next kernel advances the count
    hipLaunchKernelGGL(step_tick_kernel, dim3(1), dim3(1), 0, s, d.step_state);
    TRL_LAUNCH_CHECK();
  }
  return TRL_OK;
}

extern "C" int trl_clip_step_f32(const trl_opt_t* p, void* stream) {
  const int rc = clip_step_launch(p, stream, true);
  return rc == NOTHING_STEPPED ? TRL_OK : rc;
}

extern "C" int trl_clip_step_polyak_f32(const trl_opt_t* p, float* target, const float* source, int64_t n, float tau,
                                        const void* raw, int raw_bytes, void* ring, int slots, void* stream) {
  TRL_REQUIRE(n > 0 && target && source, "polyak: empty / null");
  if (ring) {
    TRL_REQUIRE(raw && raw_bytes > 0 && raw_bytes % 4 == 0 && slots > 0, "clip_step_polyak: bad ring");
    TRL_REQUIRE(p && p->step_state, "clip_step_polyak: the ring row is picked by the device-resident step state");
  }
  int rc = clip_step_launch(p, stream, false);
  if (rc != TRL_OK && rc != TICK_PENDING && rc != NOTHING_STEPPED) return rc;
  // trl_clip_adam_polyak_f32's own Polyak / filing kernel; beta 1 leaves the step state's Adam slots as they are.
  // `ticked`: 1 only where the step kernel has advanced the count already -- an empty parameter set launched nothing and
  // ticked nothing, so the ring row is the count's own.
  return trl_polyak_file_launch(target, source, n, tau, rc == TICK_PENDING ? p->step_state : (double*)nullptr, 1.0f, 1.0f,
                                ring ? raw : nullptr, ring ? raw_bytes : 0, ring, p->step_state, slots,
                                rc == TRL_OK ? 1 : 0, stream);
}
