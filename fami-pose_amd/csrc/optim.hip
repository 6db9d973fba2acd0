// The fused SGD step: torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov) over a flat fp32 parameter arena
// (posetimation/optimizer/optimizer.py:58-64 builds the reference's; defaults posetimation/config/defaults.py:137-140).
//
// One pass over the arena per step: read p, g (and the momentum buffer), write p (and the buffer) -- 5 x 4 bytes per
// element with momentum, 3 x 4 without.  16-byte loads / stores over the aligned body of [p, p + n), scalar head and
// tail elements around it, so an arena sub-range with unaligned bounds (the Trainer's in-backward split) still works.
// The step count, the learning rate and the skip decision live in a device vector, as Adam's do: a captured hipGraph
// keeps replaying across LR changes and across the first-step rule of the momentum buffer.
//
// Global-norm gradient clipping and dynamic loss scaling, device-resident (nothing here needs a host sync or a re-capture):
// the sum of squares of the gradient arena as a partial-slab reduction (sumsq_kernel: one fixed contiguous chunk and one
// plain store per workgroup, no float atomics, so the result is a pure function of (g, n, alignment) and bitwise equal run to
// run), alone or fused into the unscale-and-check pass; clip_coef_kernel turns the slab into {total_norm, coef}
// (torch.nn.utils.clip_grad_norm_, norm_type 2); the *_scaled optimizer entry points multiply the gradient by a device
// scalar on load instead of rewriting the arena; loss_scale_update_kernel is torch.amp.GradScaler's update rule.
//
// The exponential moving average of the parameter arena, device-resident: ema_prep_kernel keeps {updates, decay_t, 1 - decay_t,
// apply} in a device vector and reads the optimizer's "this step was applied" scalar, so a skipped step leaves the average alone
// without a host read-back and a captured hipGraph keeps replaying; ema_update_kernel is one pass over both arenas (12 bytes per
// element); swap_kernel exchanges two arenas in place (the averaged weights into the model and out again).
#include "common.h"

// state = {step, lr, apply}
// flag (optional): raised by fami_unscale_check_f32 on inf / NaN gradients.  The step is then SKIPPED exactly as
// adam_prep_kernel skips it: no step count, apply = 0 tells sgd_kernel to return, the flag is cleared and flag[1] counts it.
__global__ void sgd_prep_kernel(float* state, unsigned* flag) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (flag && *flag) {
      *flag = 0u;
      flag[1] += 1u;
      state[2] = 0.f;
      return;
    }
    state[0] += 1.f;
    state[2] = 1.f;
  }
}

// torch.optim.SGD's single-tensor rule for one element (maximize = False).  Every rounding is spelled out (fmaf where the
// compiler has always fused, separately rounded products elsewhere) instead of left to fp-contraction: the plain and the
// scaled kernels inline this into different surroundings, and their results must agree bit for bit at a multiplier of 1.
template <bool MOM>
__device__ __forceinline__ void sgd_elem(float& p, float g, float& b, float lr, float mom, float damp1, float wd,
                                         bool first, int nesterov) {
#pragma clang fp contract(off)
  float d = g;
  if (wd != 0.f) d = fmaf(wd, p, d);
  if (MOM) {
    b = first ? d : mom * b + damp1 * d;          // the first step clones d: undampened
    d = nesterov ? fmaf(mom, b, d) : b;
  }
  p = fmaf(-lr, d, p);
}

// head: the elements in front of the first 16-byte boundary of p (g and buf share p's alignment; head = n when they
// do not, and every element takes the scalar path)
// SCALED: the gradient is gmul[0] * g on load (the clip coefficient of fami_clip_coef_f32); the arena is not rewritten
template <bool MOM, bool SCALED>
__device__ __forceinline__ void sgd_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n,
                                         long head, const float* __restrict__ state, float mom, float dampening, float wd,
                                         int nesterov, const float* __restrict__ gmul) {
  if (state[2] == 0.f) return;   // skipped step (non-finite gradients, see sgd_prep_kernel)
  const float lr = state[1];
  const bool first = state[0] <= 1.f;
  const float damp1 = 1.f - dampening;
  const float gm = SCALED ? gmul[0] : 1.f;
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  const long n4 = (n - head) >> 2, tail = head + n4 * 4;
  for (long i = tid; i < n4; i += stride) {
    const long o = head + i * 4;
    f32x4 pv = ld4(p + o);
    const f32x4 gv = ld4(g + o);
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (MOM) bv = ld4(buf + o);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float pe = pv[t], be = bv[t];
      sgd_elem<MOM>(pe, SCALED ? mul_rn(gm, gv[t]) : gv[t], be, lr, mom, damp1, wd, first, nesterov);
      pv[t] = pe;
      bv[t] = be;
    }
    st4(p + o, pv);
    if (MOM) st4(buf + o, bv);
  }
  // the scalar rest: [0, head) and [tail, n)
  const long nrest = head + (n - tail);
  for (long j = tid; j < nrest; j += stride) {
    const long i = j < head ? j : tail + (j - head);
    float pe = p[i], be = MOM ? buf[i] : 0.f;
    sgd_elem<MOM>(pe, SCALED ? mul_rn(gm, g[i]) : g[i], be, lr, mom, damp1, wd, first, nesterov);
    p[i] = pe;
    if (MOM) buf[i] = be;
  }
}
template <bool MOM>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ buf, long n, long head,
                                                  const float* __restrict__ state, float mom, float dampening,
                                                  float wd, int nesterov) {
  sgd_body<MOM, false>(p, g, buf, n, head, state, mom, dampening, wd, nesterov, nullptr);
}
template <bool MOM>
__global__ __launch_bounds__(256) void sgd_scaled_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ buf, long n, long head,
                                                         const float* __restrict__ state, float mom, float dampening,
                                                         float wd, int nesterov, const float* __restrict__ gmul) {
  sgd_body<MOM, true>(p, g, buf, n, head, state, mom, dampening, wd, nesterov, gmul);
}

// ---- the sum of squares of a gradient arena ------------------------------------------------------------------------------
// SUMSQ_PARTS workgroups of 256 lanes, always all of them: workgroup b owns the contiguous run of ceil(n4 / SUMSQ_PARTS) 16-byte
// vectors [b * chunk, (b + 1) * chunk) of the aligned body and stores ONE float into partials[b] (0 when its run is empty);
// workgroup 0 also takes the scalar head / tail elements (at most 3 + 3), one per lane.  Per lane: one fp32 accumulator per
// vector component over ceil(chunk / 256) vectors in address order, the four components pairwise (2 additions) plus the
// scalar rest (1), wave_sum (6), the four waves through LDS pairwise (2).  The longest chain of fp32 additions is therefore
//   k = ceil(ceil(n4 / 2048) / 256) + 11      (42 at the 64 655 204 elements of the W48 arena)
// and the relative error of the sum of non-negative squares at most (k + 1) 2^-24.  No atomics: the slab is a pure function of
// (g, n, alignment).  SUMSQ_RW: the unscale-and-check pass in front of it -- g *= f * (fdev ? fdev[0] : 1), *flag raised on inf /
// NaN, exactly what unscale_check_kernel leaves in the arena -- with the squares taken from the unscaled values on their way
// back to memory (partials may then be null: no reduction).  SUMSQ_ACC: the pass that closes a gradient-accumulation window,
// g = rn(rn(acc + g) * mul) with the same check and the same squares -- the layout is g's alone, so the slab is what SUMSQ_READ
// gives on the arena this pass leaves; acc is only read, as 16-byte vectors where it shares g's alignment (AVEC) and as four
// scalar loads per vector where it does not.
constexpr int SUMSQ_PARTS = 2048;
enum { SUMSQ_READ = 0, SUMSQ_RW = 1, SUMSQ_ACC = 2 };

// rn(rn(a + g) * mul): an add feeding a multiply has no fused form, and none may appear -- both roundings spelled out
__device__ __forceinline__ float accum_elem(float a, float g, float mul) {
#pragma clang fp contract(off)
  const float s = a + g;
  return s * mul;
}

template <int MODE, bool AVEC>
__device__ __forceinline__ f32x4 sumsq_vec(float* __restrict__ a, const float* __restrict__ c, float mul, bool& bad) {
  f32x4 v = ld4(a);
  if (MODE != SUMSQ_READ) {
    if (MODE == SUMSQ_ACC) {
      f32x4 w;
      if (AVEC) {
        w = ld4(c);
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) w[t] = c[t];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = accum_elem(w[t], v[t], mul);
    } else {
      v = v * mul;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) bad |= !(fabsf(v[t]) <= 3.4028235e38f);
    st4(a, v);
  }
  return v;
}

template <int MODE, bool AVEC>
__global__ __launch_bounds__(256) void sumsq_kernel(float* __restrict__ g, const float* __restrict__ accum, long n, long head,
                                                    float f, const float* __restrict__ fdev, unsigned* __restrict__ flag,
                                                    float* __restrict__ partials) {
  const float mul = MODE != SUMSQ_READ ? (fdev ? f * fdev[0] : f) : 1.f;
  const long n4 = (n - head) >> 2, tail = head + n4 * 4;
  const long chunk = (n4 + gridDim.x - 1) / gridDim.x;
  const long lo = blockIdx.x * chunk, hi = lo + chunk < n4 ? lo + chunk : n4;
  float* __restrict__ body = g + head;
  const float* __restrict__ abody = MODE == SUMSQ_ACC ? accum + head : nullptr;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  bool bad = false;
  long i = lo + threadIdx.x;
  for (; i + 3 * 256 < hi; i += 4 * 256) {       // four 16-byte loads in flight per lane; summed in address order
    const f32x4 v0 = sumsq_vec<MODE, AVEC>(body + i * 4, abody + i * 4, mul, bad);
    const f32x4 v1 = sumsq_vec<MODE, AVEC>(body + (i + 256) * 4, abody + (i + 256) * 4, mul, bad);
    const f32x4 v2 = sumsq_vec<MODE, AVEC>(body + (i + 512) * 4, abody + (i + 512) * 4, mul, bad);
    const f32x4 v3 = sumsq_vec<MODE, AVEC>(body + (i + 768) * 4, abody + (i + 768) * 4, mul, bad);
    acc += v0 * v0;
    acc += v1 * v1;
    acc += v2 * v2;
    acc += v3 * v3;
  }
  for (; i < hi; i += 256) {
    const f32x4 v = sumsq_vec<MODE, AVEC>(body + i * 4, abody + i * 4, mul, bad);
    acc += v * v;
  }
  float rest = 0.f;
  const long nrest = head + (n - tail);          // <= 6: [0, head) and [tail, n), one element per lane of workgroup 0
  if (blockIdx.x == 0 && threadIdx.x < nrest) {
    const long j = threadIdx.x < head ? threadIdx.x : tail + (threadIdx.x - head);
    float v = g[j];
    if (MODE != SUMSQ_READ) {
      if (MODE == SUMSQ_ACC)
        v = accum_elem(accum[j], v, mul);
      else
        v *= mul;
      bad |= !(fabsf(v) <= 3.4028235e38f);
      g[j] = v;
    }
    rest = v * v;
  }
  if (MODE != SUMSQ_READ && flag && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
  if (!partials) return;
  float s = wave_sum(((acc[0] + acc[1]) + (acc[2] + acc[3])) + rest);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// clip = {total_norm, coef}: the slab summed in double in a fixed order (each lane a contiguous run of partials in index
// order, then wave_sum_d and the four waves pairwise), total_norm = sqrt(sum) rounded to fp32 once,
// coef = min(1, max_norm / (total_norm + 1e-6f)) -- clip_grad_norm_'s rule.  A non-finite norm raises flag[0] (coef = 0): the
// checked prep kernels then skip and count the step like an fp16 overflow.
__global__ __launch_bounds__(256) void clip_coef_kernel(const float* __restrict__ partials, int nparts,
                                                        const float* __restrict__ max_norm, float* __restrict__ clip,
                                                        unsigned* __restrict__ flag) {
  const int per = (nparts + 255) / 256;
  double s = 0.0;
  for (int j = 0; j < per; ++j) {
    const int i = threadIdx.x * per + j;
    if (i < nparts) s += (double)partials[i];
  }
  s = wave_sum_d(s);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt((red[0] + red[1]) + (red[2] + red[3]));
    float coef = fminf(1.f, max_norm[0] / (norm + 1e-6f));
    if (!(fabsf(norm) <= 3.4028235e38f)) {
      coef = 0.f;
      flag[0] = 1u;
    }
    clip[0] = norm;
    clip[1] = coef;
  }
}

// scaler = {scale, 1 / scale, growth tracker}: torch's _amp_update_scale_.  Reads flag[0] and leaves it alone (the checked
// prep of the optimizer clears it afterwards).
__global__ void loss_scale_update_kernel(float* __restrict__ scaler, const unsigned* __restrict__ flag, float growth,
                                         float backoff, int interval) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float scale = scaler[0];
    if (flag[0]) {
      scale *= backoff;
      scaler[2] = 0.f;
    } else {
      const float t = scaler[2] + 1.f;
      if (t >= (float)interval) {
        const float grown = scale * growth;
        if (fabsf(grown) <= 3.4028235e38f) scale = grown;     // growth that would reach inf is refused
        scaler[2] = 0.f;
      } else {
        scaler[2] = t;
      }
    }
    scaler[0] = scale;
    scaler[1] = 1.f / scale;
  }
}

// ---- the exponential moving average of a parameter arena -----------------------------------------------------------------
// st = {updates, decay_t, w = 1 - decay_t, apply}.  gate (optional): the scalar the optimizer's prep leaves -- state[2] of
// adam_prep_kernel (the first bias correction, 0 on a skipped step) and of sgd_prep_kernel (apply).  A skipped step only
// clears `apply`: the update count, and with it the warm-up schedule, does not advance.  warmup: the usual
// min(decay, (1 + t) / (10 + t)) ramp, t the update being made (1, 2, ...).
__global__ void ema_prep_kernel(float* st, const float* gate, float decay, int warmup) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
#pragma clang fp contract(off)
    if (gate && gate[0] == 0.f) {
      st[3] = 0.f;
      return;
    }
    const float t = st[0] + 1.f;
    const float d = warmup ? fminf(decay, (1.f + t) / (10.f + t)) : decay;
    st[0] = t;
    st[1] = d;
    st[2] = 1.f - d;
    st[3] = 1.f;
  }
}

// rn(e + rn(w * rn(p - e))): three roundings, no fused multiply-add -- three fp32 torch operations give the same bits
__device__ __forceinline__ float ema_elem(float e, float p, float w) {
#pragma clang fp contract(off)
  const float d = p - e;
  const float s = w * d;
  return e + s;
}

// the second array of a two-arena pass: 16-byte accesses where it shares the first one's alignment (BVEC), four scalar
// ones per vector where it does not (sumsq_vec's AVEC split).  NT: a non-temporal load, for an arena this pass reads once --
// measured on the W48 arenas, the update pass with cold caches: 165 -> 140 us (the store side gains nothing from the hint)
template <bool BVEC, bool NT>
__device__ __forceinline__ f32x4 ld4_as(const float* b) {
  if (BVEC) return NT ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(b)) : ld4(b);
  f32x4 v;
#pragma unroll
  for (int t = 0; t < 4; ++t) v[t] = NT ? __builtin_nontemporal_load(b + t) : b[t];
  return v;
}
template <bool BVEC>
__device__ __forceinline__ void st4_as(float* b, f32x4 v) {
  if (BVEC) {
    st4(b, v);
    return;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) b[t] = v[t];
}

// The work layout of both passes is the first array's.  head: its elements in front of the first 16-byte boundary (sumsq_head).
// The aligned body is cut into tiles of TWO_U x 256 consecutive vectors (16 KB of each arena); a chip-sized grid strides the
// tiles, every lane with TWO_U vectors of each arena in flight, 256 vectors apart.  (Measured against a plain grid-stride loop,
// against the same loop with four vectors a whole grid apart in flight, and against sumsq_kernel's one-chunk-per-workgroup layout:
// the tiles are the fastest, the vectors-a-grid-apart form the slowest, 12 % behind.)  The workgroup that meets the last, partial
// tile walks it one vector per lane; workgroup 0 takes the <= 3 + 3 scalar head / tail elements, one per lane.
constexpr int TWO_U = 4;
static inline int two_arena_grid(long n) { return fami_ew_grid((n / 4 + TWO_U - 1) / TWO_U); }

template <bool PVEC>
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, long head,
                                                         const float* __restrict__ st) {
  if (st[3] == 0.f) return;      // skipped step (see ema_prep_kernel)
  const float w = st[2];
  const long n4 = (n - head) >> 2, tail = head + n4 * 4;
  float* __restrict__ eb = ema + head;
  const float* __restrict__ pb = p + head;
  const long tile = (long)TWO_U * 256, stride = (long)gridDim.x * tile;
  long base = blockIdx.x * tile;
  for (; base + tile <= n4; base += stride) {
    const long i = base + threadIdx.x;
    f32x4 e[TWO_U], q[TWO_U];
#pragma unroll
    for (int u = 0; u < TWO_U; ++u) {
      e[u] = ld4(eb + (i + u * 256) * 4);
      q[u] = ld4_as<PVEC, true>(pb + (i + u * 256) * 4);
    }
#pragma unroll
    for (int u = 0; u < TWO_U; ++u) {
#pragma unroll
      for (int t = 0; t < 4; ++t) e[u][t] = ema_elem(e[u][t], q[u][t], w);
      st4(eb + (i + u * 256) * 4, e[u]);
    }
  }
  if (base < n4) {               // the last, partial tile: [base, n4)
    for (long i = base + threadIdx.x; i < n4; i += 256) {
      f32x4 e = ld4(eb + i * 4);
      const f32x4 q = ld4_as<PVEC, true>(pb + i * 4);
#pragma unroll
      for (int t = 0; t < 4; ++t) e[t] = ema_elem(e[t], q[t], w);
      st4(eb + i * 4, e);
    }
  }
  const long nrest = head + (n - tail);          // <= 6: [0, head) and [tail, n)
  if (blockIdx.x == 0 && threadIdx.x < nrest) {
    const long j = threadIdx.x < head ? threadIdx.x : tail + (threadIdx.x - head);
    ema[j] = ema_elem(ema[j], p[j], w);
  }
}

// a <-> b in one pass, no temporary: every lane holds what it is about to overwrite in registers
template <bool BVEC>
__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, long n, long head) {
  const long n4 = (n - head) >> 2, tail = head + n4 * 4;
  float* __restrict__ ab = a + head;
  float* __restrict__ bb = b + head;
  const long tile = (long)TWO_U * 256, stride = (long)gridDim.x * tile;
  long base = blockIdx.x * tile;
  for (; base + tile <= n4; base += stride) {
    const long i = base + threadIdx.x;
    f32x4 x[TWO_U], y[TWO_U];
#pragma unroll
    for (int u = 0; u < TWO_U; ++u) {
      x[u] = ld4(ab + (i + u * 256) * 4);
      y[u] = ld4_as<BVEC, false>(bb + (i + u * 256) * 4);
    }
#pragma unroll
    for (int u = 0; u < TWO_U; ++u) {
      st4(ab + (i + u * 256) * 4, y[u]);
      st4_as<BVEC>(bb + (i + u * 256) * 4, x[u]);
    }
  }
  if (base < n4) {
    for (long i = base + threadIdx.x; i < n4; i += 256) {
      const f32x4 x = ld4(ab + i * 4);
      const f32x4 y = ld4_as<BVEC, false>(bb + i * 4);
      st4(ab + i * 4, y);
      st4_as<BVEC>(bb + i * 4, x);
    }
  }
  const long nrest = head + (n - tail);
  if (blockIdx.x == 0 && threadIdx.x < nrest) {
    const long j = threadIdx.x < head ? threadIdx.x : tail + (threadIdx.x - head);
    const float x = a[j], y = b[j];
    a[j] = y;
    b[j] = x;
  }
}

extern "C" {

// state (device float[3]) = {step, lr, apply}; prep increments step
int fami_sgd_prep_f32(float* state, hipStream_t s) {
  FAMI_REQUIRE(state, "fami_sgd_prep_f32", "bad argument");
  hipLaunchKernelGGL(sgd_prep_kernel, dim3(1), dim3(64), 0, s, state, (unsigned*)nullptr);
  FAMI_CHECK_LAUNCH("fami_sgd_prep_f32");
  return FAMI_OK;
}
// the same, skipping the step when *flag != 0 (and clearing the flag): see fami_unscale_check_f32
int fami_sgd_prep_checked_f32(float* state, unsigned* flag, hipStream_t s) {
  FAMI_REQUIRE(state && flag, "fami_sgd_prep_checked_f32", "bad argument");
  hipLaunchKernelGGL(sgd_prep_kernel, dim3(1), dim3(64), 0, s, state, flag);
  FAMI_CHECK_LAUNCH("fami_sgd_prep_checked_f32");
  return FAMI_OK;
}
// head elements of the scalar path in front of the 16-byte aligned body (n: no common alignment, everything scalar)
static long sgd_head(const float* p, const float* g, const float* buf, long n, bool mom) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p) & 15;
  const bool same = (reinterpret_cast<uintptr_t>(g) & 15) == a && (!mom || (reinterpret_cast<uintptr_t>(buf) & 15) == a);
  long head = n;
  if (same && (a & 3) == 0) head = ((16 - (long)a) & 15) >> 2;
  return head > n ? n : head;
}
int fami_sgd_f32(float* p, const float* g, float* buf, long n, const float* state, float momentum, float dampening,
                 float weight_decay, int nesterov, hipStream_t s) {
  FAMI_REQUIRE(p && g && state && n > 0 && (momentum == 0.f || buf), "fami_sgd_f32", "bad argument");
  FAMI_REQUIRE(!nesterov || (momentum > 0.f && dampening == 0.f), "fami_sgd_f32",
               "nesterov needs a momentum and zero dampening");
  const bool mom = momentum != 0.f;
  const long head = sgd_head(p, g, buf, n, mom);
  const dim3 grid(fami_ew_grid(head == n ? n : (n + 3) / 4));     // a chip-sized grid (<= 2048 blocks) strides the rest
  if (mom)
    hipLaunchKernelGGL(sgd_kernel<true>, grid, dim3(256), 0, s, p, g, buf, n, head, state, momentum, dampening,
                       weight_decay, nesterov);
  else
    hipLaunchKernelGGL(sgd_kernel<false>, grid, dim3(256), 0, s, p, g, (float*)nullptr, n, head, state, momentum,
                       dampening, weight_decay, nesterov);
  FAMI_CHECK_LAUNCH("fami_sgd_f32");
  return FAMI_OK;
}
// the same update with the gradient gmul[0] * g (gmul: device float, e.g. the clip coefficient): bitwise fami_sgd_f32 at gmul[0] == 1
int fami_sgd_scaled_f32(float* p, const float* g, float* buf, long n, const float* state, float momentum, float dampening,
                        float weight_decay, int nesterov, const float* gmul, hipStream_t s) {
  FAMI_REQUIRE(p && g && state && gmul && n > 0 && (momentum == 0.f || buf), "fami_sgd_scaled_f32", "bad argument");
  FAMI_REQUIRE(!nesterov || (momentum > 0.f && dampening == 0.f), "fami_sgd_scaled_f32",
               "nesterov needs a momentum and zero dampening");
  const bool mom = momentum != 0.f;
  const long head = sgd_head(p, g, buf, n, mom);
  const dim3 grid(fami_ew_grid(head == n ? n : (n + 3) / 4));
  if (mom)
    hipLaunchKernelGGL(sgd_scaled_kernel<true>, grid, dim3(256), 0, s, p, g, buf, n, head, state, momentum, dampening,
                       weight_decay, nesterov, gmul);
  else
    hipLaunchKernelGGL(sgd_scaled_kernel<false>, grid, dim3(256), 0, s, p, g, (float*)nullptr, n, head, state, momentum,
                       dampening, weight_decay, nesterov, gmul);
  FAMI_CHECK_LAUNCH("fami_sgd_scaled_f32");
  return FAMI_OK;
}

// ---- gradient norm, clip coefficient, loss-scale update
int fami_sumsq_parts(void) { return SUMSQ_PARTS; }
// elements in front of the first 16-byte boundary of a 4-byte aligned g
static long sumsq_head(const float* g, long n) {
  const long head = ((16 - (long)(reinterpret_cast<uintptr_t>(g) & 15)) & 15) >> 2;
  return head > n ? n : head;
}
// partials (device float[fami_sumsq_parts()]): every slot is written; their sum is sum_i g[i]^2
int fami_sumsq_f32(const float* g, long n, float* partials, hipStream_t s) {
  FAMI_REQUIRE(g && partials && n > 0 && (reinterpret_cast<uintptr_t>(g) & 3) == 0, "fami_sumsq_f32", "bad argument");
  hipLaunchKernelGGL((sumsq_kernel<SUMSQ_READ, true>), dim3(SUMSQ_PARTS), dim3(256), 0, s, const_cast<float*>(g),
                     (const float*)nullptr, n, sumsq_head(g, n), 1.f, (const float*)nullptr, (unsigned*)nullptr, partials);
  FAMI_CHECK_LAUNCH("fami_sumsq_f32");
  return FAMI_OK;
}
// fami_unscale_check_f32 with an optional device factor (fdev) and the sum of squares of the unscaled values (partials; may be null)
int fami_unscale_check_sumsq_f32(float* g, long n, float f, const float* fdev, unsigned* flag, float* partials, hipStream_t s) {
  FAMI_REQUIRE(g && flag && n > 0 && (reinterpret_cast<uintptr_t>(g) & 3) == 0, "fami_unscale_check_sumsq_f32", "bad argument");
  hipLaunchKernelGGL((sumsq_kernel<SUMSQ_RW, true>), dim3(SUMSQ_PARTS), dim3(256), 0, s, g, (const float*)nullptr, n,
                     sumsq_head(g, n), f, fdev, flag, partials);
  FAMI_CHECK_LAUNCH("fami_unscale_check_sumsq_f32");
  return FAMI_OK;
}
// the closing pass of a gradient-accumulation window: g = (acc + g) * f * (fdev ? fdev[0] : 1), each operation rounded once;
// flag (may be null: no check) raised on inf / NaN in what was written, partials (may be null) = fami_sumsq_f32 of the result
int fami_accum_unscale_check_sumsq_f32(float* g, const float* acc, long n, float f, const float* fdev, unsigned* flag,
                                       float* partials, hipStream_t s) {
  FAMI_REQUIRE(g && acc && n > 0 && ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(acc)) & 3) == 0,
               "fami_accum_unscale_check_sumsq_f32", "bad argument");
  // the work layout is g's (the slab must be fami_sumsq_f32's on the result); acc is read as vectors only where it shares g's
  // alignment, which is sgd_head's decision
  const long head = sumsq_head(g, n);
  const bool avec = sgd_head(g, acc, nullptr, n, false) == head;
  if (avec)
    hipLaunchKernelGGL((sumsq_kernel<SUMSQ_ACC, true>), dim3(SUMSQ_PARTS), dim3(256), 0, s, g, acc, n, head, f, fdev, flag, partials);
  else
    hipLaunchKernelGGL((sumsq_kernel<SUMSQ_ACC, false>), dim3(SUMSQ_PARTS), dim3(256), 0, s, g, acc, n, head, f, fdev, flag, partials);
  FAMI_CHECK_LAUNCH("fami_accum_unscale_check_sumsq_f32");
  return FAMI_OK;
}
int fami_clip_coef_f32(const float* partials, int nparts, const float* max_norm_dev, float* clip, unsigned* flag, hipStream_t s) {
  FAMI_REQUIRE(partials && nparts > 0 && max_norm_dev && clip && flag, "fami_clip_coef_f32", "bad argument");
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, s, partials, nparts, max_norm_dev, clip, flag);
  FAMI_CHECK_LAUNCH("fami_clip_coef_f32");
  return FAMI_OK;
}
int fami_loss_scale_update_f32(float* scaler, const unsigned* flag, float growth, float backoff, int interval, hipStream_t s) {
  FAMI_REQUIRE(scaler && flag && growth >= 1.f && backoff > 0.f && backoff <= 1.f && interval > 0,
               "fami_loss_scale_update_f32", "bad argument");
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, s, scaler, flag, growth, backoff, interval);
  FAMI_CHECK_LAUNCH("fami_loss_scale_update_f32");
  return FAMI_OK;
}

// ---- exponential moving average of the parameters, arena swap
// st (device float[4]) = {updates, decay_t, 1 - decay_t, apply}; gate (device float, may be null): 0 = the optimizer skipped this step
int fami_ema_prep_f32(float* st, const float* gate, float decay, int warmup, hipStream_t s) {
  FAMI_REQUIRE(st && decay > 0.f && decay < 1.f, "fami_ema_prep_f32", "bad argument");
  hipLaunchKernelGGL(ema_prep_kernel, dim3(1), dim3(64), 0, s, st, gate, decay, warmup);
  FAMI_CHECK_LAUNCH("fami_ema_prep_f32");
  return FAMI_OK;
}
// two 4-byte aligned arrays of n floats that do not overlap; *bvec: the second shares the first one's 16-byte alignment
static bool two_arenas(const float* a, const float* b, long n, bool* bvec) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  if (!a || !b || n <= 0 || ((x | y) & 3) != 0) return false;
  if (!(x + (uintptr_t)n * 4 <= y || y + (uintptr_t)n * 4 <= x)) return false;
  *bvec = (x & 15) == (y & 15);
  return true;
}
// ema = ema + st[2] * (p - ema), each operation rounded once; nothing is written when st[3] == 0; p is only read
int fami_ema_update_f32(float* ema, const float* p, long n, const float* st, hipStream_t s) {
  bool pvec = false;
  FAMI_REQUIRE(st && two_arenas(ema, p, n, &pvec), "fami_ema_update_f32", "bad argument");
  const long head = sumsq_head(ema, n);
  const dim3 grid(two_arena_grid(n));     // a chip-sized grid (<= 2048 workgroups) strides the tiles
  if (pvec)
    hipLaunchKernelGGL(ema_update_kernel<true>, grid, dim3(256), 0, s, ema, p, n, head, st);
  else
    hipLaunchKernelGGL(ema_update_kernel<false>, grid, dim3(256), 0, s, ema, p, n, head, st);
  FAMI_CHECK_LAUNCH("fami_ema_update_f32");
  return FAMI_OK;
}
// a <-> b, bit for bit (no arithmetic touches the values), in place
int fami_swap_f32(float* a, float* b, long n, hipStream_t s) {
  bool bvec = false;
  FAMI_REQUIRE(two_arenas(a, b, n, &bvec), "fami_swap_f32", "bad argument");
  const long head = sumsq_head(a, n);
  const dim3 grid(two_arena_grid(n));
  if (bvec)
    hipLaunchKernelGGL(swap_kernel<true>, grid, dim3(256), 0, s, a, b, n, head);
  else
    hipLaunchKernelGGL(swap_kernel<false>, grid, dim3(256), 0, s, a, b, n, head);
  FAMI_CHECK_LAUNCH("fami_swap_f32");
  return FAMI_OK;
}

}  // extern "C"
