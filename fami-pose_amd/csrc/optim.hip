// The fused SGD step: torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov) over a flat fp32 parameter arena
// (posetimation/optimizer/optimizer.py:58-64 builds the reference's; defaults posetimation/config/defaults.py:137-140).
//
// One pass over the arena per step: read p, g (and the momentum buffer), write p (and the buffer) -- 5 x 4 bytes per
// element with momentum, 3 x 4 without.  16-byte loads / stores over the aligned body of [p, p + n), scalar head and
// tail elements around it, so an arena sub-range with unaligned bounds (the Trainer's in-backward split) still works.
// The step count, the learning rate and the skip decision live in a device vector, as Adam's do: a captured hipGraph
// keeps replaying across LR changes and across the first-step rule of the momentum buffer.
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

// torch.optim.SGD's single-tensor rule for one element (maximize = False)
template <bool MOM>
__device__ __forceinline__ void sgd_elem(float& p, float g, float& b, float lr, float mom, float damp1, float wd,
                                         bool first, int nesterov) {
  float d = g;
  if (wd != 0.f) d += wd * p;
  if (MOM) {
    b = first ? d : mom * b + damp1 * d;          // the first step clones d: undampened
    d = nesterov ? d + mom * b : b;
  }
  p -= lr * d;
}

// head: the elements in front of the first 16-byte boundary of p (g and buf share p's alignment; head = n when they
// do not, and every element takes the scalar path)
template <bool MOM>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ buf, long n, long head,
                                                  const float* __restrict__ state, float mom, float dampening,
                                                  float wd, int nesterov) {
  if (state[2] == 0.f) return;   // skipped step (non-finite gradients, see sgd_prep_kernel)
  const float lr = state[1];
  const bool first = state[0] <= 1.f;
  const float damp1 = 1.f - dampening;
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
      sgd_elem<MOM>(pe, gv[t], be, lr, mom, damp1, wd, first, nesterov);
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
    sgd_elem<MOM>(pe, g[i], be, lr, mom, damp1, wd, first, nesterov);
    p[i] = pe;
    if (MOM) buf[i] = be;
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
int fami_sgd_f32(float* p, const float* g, float* buf, long n, const float* state, float momentum, float dampening,
                 float weight_decay, int nesterov, hipStream_t s) {
  FAMI_REQUIRE(p && g && state && n > 0 && (momentum == 0.f || buf), "fami_sgd_f32", "bad argument");
  FAMI_REQUIRE(!nesterov || (momentum > 0.f && dampening == 0.f), "fami_sgd_f32",
               "nesterov needs a momentum and zero dampening");
  const bool mom = momentum != 0.f;
  const uintptr_t a = reinterpret_cast<uintptr_t>(p) & 15;
  const bool same = (reinterpret_cast<uintptr_t>(g) & 15) == a && (!mom || (reinterpret_cast<uintptr_t>(buf) & 15) == a);
  long head = n;
  if (same && (a & 3) == 0) head = ((16 - (long)a) & 15) >> 2;
  if (head > n) head = n;
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

}  // extern "C"
