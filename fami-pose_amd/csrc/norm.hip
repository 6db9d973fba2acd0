// BatchNorm (train-mode batch statistics + running-stat update, eval-mode
// apply) and its backward, fused with ReLU and the residual add, for NHWC fp32
// activations viewed as a [P = N*H*W][C] matrix.  HBM-bound streaming kernels:
// each thread owns one 4-channel vector column and strides over pixels, so a
// wave reads whole 16-byte-per-lane contiguous rows.
//
// Replaces nn.BatchNorm2d (+ nn.ReLU, `out += residual`) as used by
//   posetimation/layers/basic_model.py:25-63 (BasicBlock), :66-113 (Bottleneck),
//   posetimation/layers/basic_layer.py:25-26 (conv_bn_relu.bn),
//   posetimation/backbones/hrnet.py:99-143 (fuse layers), :724-762 (transitions)
// with momentum 0.1, eps 1e-5, biased variance for normalisation and unbiased
// variance for running_var (torch.nn.BatchNorm2d semantics).
#include "common.h"

#define BN_MAXG 512
#ifndef BN_U
#define BN_U 4  // rows per thread in flight in the statistics passes
#endif

struct ColMap {
  int cv, prow, rows, CV;
  bool active;
};
__device__ __forceinline__ ColMap col_map(int C) {
  ColMap m;
  m.CV = C >> 2;
  m.rows = 256 / m.CV;
  m.cv = threadIdx.x % m.CV;
  m.prow = threadIdx.x / m.CV;
  m.active = m.prow < m.rows;
  return m;
}

// sum of one double per thread over a 256-thread block (result valid in thread 0)
__device__ __forceinline__ double block_sum_d(double v, double* sm4) {
  v = wave_sum_d(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sm4[wave] = v;
  __syncthreads();
  return (sm4[0] + sm4[1]) + (sm4[2] + sm4[3]);
}

// ---- the pieces every generation of the kernels below shares (three-launch, two-launch slot, one-launch small forms)

// forward statistics walk: s = sum (x - K), q = sum (x - K)^2 over this thread's rows of its 4-channel column, with the pivot
// K[c] = x[0][c] (the first pixel): shifted sums keep E[d^2] - E[d]^2 free of the cancellation that the raw moments suffer
// when |mean| >> std.
template <typename T>
__device__ __forceinline__ void bn_fwd_sums(const T* __restrict__ x, const ColMap& m, long P, int C, f32x4& s, f32x4& q) {
  const f32x4 piv = ld4(x + m.cv * 4);
  // BN_U rows per thread in flight: with one load per thread and <= 512 workgroups the pass is bound by memory
  // latency (8 KB in flight per CU), not bandwidth.  The sums are taken in the same row order as a rolled loop.
  // Main loop + rolled tail, NOT the clamped re-read of the backward walk (bn_bwd_sums): that form measured +7 % here.
  const long step = (long)gridDim.x * m.rows;
  long p = (long)blockIdx.x * m.rows + m.prow;
  for (; p + (BN_U - 1) * step < P; p += BN_U * step) {
    f32x4 v[BN_U];
#pragma unroll
    for (int u = 0; u < BN_U; ++u) v[u] = ld4(x + (p + u * step) * C + m.cv * 4);
#pragma unroll
    for (int u = 0; u < BN_U; ++u) {
      const f32x4 d = v[u] - piv;
      s += d;
      q += d * d;
    }
  }
  for (; p < P; p += step) {
    const f32x4 v = ld4(x + p * C + m.cv * 4) - piv;
    s += v;
    q += v * v;
  }
}

// a thread's two sums into its row of the [rows][2][C] LDS stage
__device__ __forceinline__ void bn_stage_rows(float* sm, const ColMap& m, int C, f32x4 s, f32x4 q) {
  float* d = sm + (long)m.prow * 2 * C;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    d[m.cv * 4 + t] = s[t];
    d[C + m.cv * 4 + t] = q[t];
  }
}

// fold of the [rows][2][C] LDS stage over its rows, with the two endings: the workgroup's row of the partial array
// (three-launch forms: fixed order, run-to-run bitwise), or an fp64 atomic add into slot row blockIdx.x % NS (two-launch forms)
template <bool SLOTS>
__device__ __forceinline__ void bn_fold_rows(const float* sm, int rows, int C, float* __restrict__ partial,
                                             double* __restrict__ slots, int NS) {
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * C; e += 256) {
    float tot = 0.f;
    for (int r = 0; r < rows; ++r) tot += sm[(long)r * 2 * C + e];
    if (SLOTS) unsafeAtomicAdd(slots + (long)(blockIdx.x % NS) * 2 * C + e, (double)tot);
    else partial[(long)blockIdx.x * 2 * C + e] = tot;
  }
}

// s = sum_k slots[k][0][c], q = sum_k slots[k][1][c]
__device__ __forceinline__ void bn_fold_slots(const double* __restrict__ slots, int NS, int C, int c, double& s, double& q) {
  s = 0.0;
  q = 0.0;
  for (int k = 0; k < NS; ++k) {
    s += slots[(long)k * 2 * C + c];
    q += slots[(long)k * 2 * C + C + c];
  }
}

// mean and biased variance from dm = E[x - K], dq = E[(x - K)^2] and the pivot K, in fp64
struct BnMoments {
  double mu, var;
};
__device__ __forceinline__ float bn_invstd(double var, float eps) { return (float)(1.0 / sqrt(var + (double)eps)); }
__device__ __forceinline__ BnMoments bn_moments(double dm, double dq, double piv) {
  double var = dq - dm * dm;
  if (var < 0.0) var = 0.0;
  return BnMoments{piv + dm, var};
}
// The two arithmetic forms of the expectations stay apart (they round differently): by division in the three-launch and
// one-launch forms ...
__device__ __forceinline__ BnMoments bn_moments_div(double s, double q, long P, double piv) {
  return bn_moments(s / (double)P, q / (double)P, piv);
}
// ... and by one reciprocal in the slot forms (as conv_epi.h xbn_channel takes them)
__device__ __forceinline__ BnMoments bn_moments_rcp(double s, double q, long P, double piv) {
  const double invP = 1.0 / (double)P;
  return bn_moments(s * invP, q * invP, piv);
}
// biased variance back from a finalised invstd
__device__ __forceinline__ double bn_var_of_invstd(double is, float eps) {
  double var = 1.0 / (is * is) - (double)eps;
  if (var < 0.0) var = 0.0;
  return var;
}

// running statistics of channel c: momentum step towards the batch mean and the UNBIASED batch variance
__device__ __forceinline__ void bn_running_update(float* rm, float* rv, int c, double mu, double var, double P, float momentum) {
  const double unb = P > 1.0 ? var * P / (P - 1.0) : var;
  rm[c] = (float)((1.0 - momentum) * rm[c] + momentum * mu);
  rv[c] = (float)((1.0 - momentum) * rv[c] + momentum * unb);
}

// partial[g][0][c] = sum (x - K), partial[g][1][c] = sum (x - K)^2 over this block's pixels (bn_fwd_sums)
template <typename T>
__global__ __launch_bounds__(256) void bn_partial_kernel(const T* __restrict__ x, float* __restrict__ partial,
                                                         long P, int C) {
  extern __shared__ float sm[];  // [rows][2][C]
  const ColMap m = col_map(C);
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
  if (m.active) {
    bn_fwd_sums(x, m, P, C, s, q);
    bn_stage_rows(sm, m, C, s, q);
  }
  bn_fold_rows<false>(sm, m.rows, C, partial, nullptr, 0);
}

template <typename T>
__global__ void bn_finalize_kernel(const float* __restrict__ partial, const T* __restrict__ x, int G, long P,
                                   int C, float* mean, float* invstd, float* running_mean, float* running_var,
                                   float momentum, float eps) {
  __shared__ double sm4[4];
  const int c = blockIdx.x;  // one 256-thread block per channel: G <= 512 partials are two loads per thread
  double s = 0.0, q = 0.0;
  for (int g = threadIdx.x; g < G; g += 256) {
    s += (double)partial[(long)g * 2 * C + c];
    q += (double)partial[(long)g * 2 * C + C + c];
  }
  s = block_sum_d(s, sm4);
  q = block_sum_d(q, sm4);
  if (threadIdx.x != 0) return;
  const BnMoments mo = bn_moments_div(s, q, P, (double)ld1(x + c));
  mean[c] = (float)mo.mu;
  invstd[c] = bn_invstd(mo.var, eps);
  if (running_mean) bn_running_update(running_mean, running_var, c, mo.mu, mo.var, (double)P, momentum);
}

// mean / invstd (+ running statistics) from slot rows a convolution epilogue filled (fuse terms: the cross-resolution sum
// kernel applies the normalisation itself and only needs the two vectors)
__global__ void bn_finalize_slots_kernel(const double* __restrict__ slots, int NS, const float* __restrict__ pivot, long P,
                                         int C, float* mean, float* invstd, float* running_mean, float* running_var,
                                         float momentum, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s, q;
  bn_fold_slots(slots, NS, C, c, s, q);
  const BnMoments mo = bn_moments_rcp(s, q, P, (double)pivot[c]);
  mean[c] = (float)mo.mu;
  invstd[c] = bn_invstd(mo.var, eps);
  if (running_mean) bn_running_update(running_mean, running_var, c, mo.mu, mo.var, (double)P, momentum);
}

// running statistics from an already finalised (mean, invstd): lets BatchNorm calls that SHARE a module run concurrently
// on several streams without touching the running buffers, and applies their updates afterwards in call order
// (Alignment_V15.py:125-135 applies one regressor to every supporting frame, updating frame by frame).
__global__ void bn_running_update_kernel(float* running_mean, float* running_var, const float* __restrict__ mean,
                                         const float* __restrict__ invstd, int C, long P, float momentum, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  bn_running_update(running_mean, running_var, c, (double)mean[c], bn_var_of_invstd((double)invstd[c], eps), (double)P, momentum);
}

// Batched form: the deferred updates of a forked region (32 per step for the translation regressors) in ONE launch, in
// call order -- thread c walks the entries sequentially for its channel, so several updates of one module's buffers
// apply in the order the reference applies them (frame by frame).
#define FAMI_BNRU_BATCH 32
struct BnRunBatch { float* rm[FAMI_BNRU_BATCH]; float* rv[FAMI_BNRU_BATCH]; const float* mean[FAMI_BNRU_BATCH]; const float* invstd[FAMI_BNRU_BATCH];
                    int C[FAMI_BNRU_BATCH]; float P[FAMI_BNRU_BATCH], mom[FAMI_BNRU_BATCH], eps[FAMI_BNRU_BATCH]; int n; };
__global__ __launch_bounds__(256) void bn_running_update_batch_kernel(BnRunBatch b) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  for (int k = 0; k < b.n; ++k) {
    if (c >= b.C[k]) continue;
    bn_running_update(b.rm[k], b.rv[k], c, (double)b.mean[k][c], bn_var_of_invstd((double)b.invstd[k][c], b.eps[k]),
                      (double)b.P[k], b.mom[k]);
  }
}

__global__ void bn_eval_stats_kernel(const float* running_mean, const float* running_var, float* mean, float* invstd,
                                     int C, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  mean[c] = running_mean[c];
  invstd[c] = 1.0f / sqrtf(running_var[c] + eps);
}

// y = [relu]( (x-mean)*invstd*gamma + beta [+ residual] )
// NOT bn_scale_shift: here (and in bn_small_fwd_kernel) sf = beta - mean*sc and x*sc + sf are left to the compiler's contraction;
// the relu == 2 mask and the convolution-side XBN / bnin kernels are bit-matched to bn_apply2_kernel's explicit fmas only.
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ x, const float* __restrict__ mean,
                                                       const float* __restrict__ invstd,
                                                       const float* __restrict__ gamma,
                                                       const float* __restrict__ beta,
                                                       const T* __restrict__ residual, T* __restrict__ y,
                                                       long P, int C, int relu) {
  const ColMap m = col_map(C);
  if (!m.active) return;
  f32x4 sc, sf;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = m.cv * 4 + t;
    sc[t] = invstd[c] * gamma[c];
    sf[t] = beta[c] - mean[c] * sc[t];
  }
  for (long p = (long)blockIdx.x * m.rows + m.prow; p < P; p += (long)gridDim.x * m.rows) {
    const long o = p * C + m.cv * 4;
    f32x4 v = ld4(x + o) * sc + sf;
    if (residual) v += ld4(residual + o);
    if (relu) {
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
    }
    st4(y + o, v);
  }
}

// ReLU mask of a BatchNorm output from the stored output y: dz = dy*(y > 0)
__device__ __forceinline__ f32x4 bn_relu_mask(f32x4 g, f32x4 yy) {
#pragma unroll
  for (int t = 0; t < 4; ++t) g[t] = yy[t] > 0.f ? g[t] : 0.f;
  return g;
}
// relu 0 = none, 1 = from y, 2 = recomputed from x (only valid without a residual, and only against a forward that applied
// bn_scale_shift with explicit fused multiply-adds: bn_apply2_kernel)
__device__ __forceinline__ f32x4 bn_relu_mask(f32x4 g, int relu, f32x4 yy, f32x4 xv, f32x4 sc, f32x4 sf) {
  if (relu == 1) return bn_relu_mask(g, yy);
  if (relu == 2) {
#pragma unroll
    for (int t = 0; t < 4; ++t) g[t] = __builtin_fmaf(xv[t], sc[t], sf[t]) > 0.f ? g[t] : 0.f;
  }
  return g;
}

// mean / invstd of this thread's four channels
__device__ __forceinline__ void bn_load_stats(const float* __restrict__ mean, const float* __restrict__ invstd, int c0, f32x4& mu,
                                              f32x4& is) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    mu[t] = mean[c0 + t];
    is[t] = invstd[c0 + t];
  }
}

// backward statistics walk: s = sum dz, q = sum dz*xhat over this thread's rows; dz = bn_relu_mask(dy) (sc / sf: relu 2 only).
// The spelling of the two relu tests is the one that keeps both callers' register counts at or below what their own copies of
// this loop had (`relu == 1` on the y loads, or one three-way bn_relu_mask call: +1 SGPR on one, +4-6 VGPRs on the other).
template <typename T>
__device__ __forceinline__ void bn_bwd_sums(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ y,
                                            const ColMap& m, long P, int C, int relu, f32x4 mu, f32x4 is, f32x4 sc, f32x4 sf,
                                            f32x4& s, f32x4& q) {
  const long step = (long)gridDim.x * m.rows;
  // Rows past the end re-read row p (a cache hit) and contribute an exact 0: the 3-7 rows per thread of the
  // low-resolution branches then also go out BN_U at a time instead of through a rolled tail (backward statistics
  // of the 48x36 / 24x18 maps -3...-11 %; the same form measured +7 % on the forward statistics of the 96x72 map,
  // which keeps the main loop + rolled tail: bn_fwd_sums).
  for (long p = (long)blockIdx.x * m.rows + m.prow; p < P; p += BN_U * step) {
    f32x4 g[BN_U], yy[BN_U], xx[BN_U];
    long o[BN_U];
#pragma unroll
    for (int u = 0; u < BN_U; ++u) {
      const long pu = p + u * step;
      o[u] = (pu < P ? pu : p) * C + m.cv * 4;
      g[u] = ld4(dy + o[u]);
    }
    if (relu & 1) {  // relu 1 of {0, 1, 2}
#pragma unroll
      for (int u = 0; u < BN_U; ++u) yy[u] = ld4(y + o[u]);
    }
#pragma unroll
    for (int u = 0; u < BN_U; ++u) xx[u] = ld4(x + o[u]);
#pragma unroll
    for (int u = 0; u < BN_U; ++u) {
      if (relu == 1) g[u] = bn_relu_mask(g[u], yy[u]);
      if (relu == 2) g[u] = bn_relu_mask(g[u], relu, yy[u], xx[u], sc, sf);
      if (p + u * step >= P) g[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      const f32x4 xh = (xx[u] - mu) * is;
      s += g[u];
      q += g[u] * xh;
    }
  }
}

// backward pass 1: partial[g][0][c] = sum dz, partial[g][1][c] = sum dz*xhat ; dz = relu ? dy*(y>0) : dy
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const T* __restrict__ dy,
                                                             const T* __restrict__ x,
                                                             const T* __restrict__ y,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ invstd,
                                                             float* __restrict__ partial, long P, int C, int relu) {
  extern __shared__ float sm[];
  const ColMap m = col_map(C);
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
  if (m.active) {
    f32x4 mu, is;
    bn_load_stats(mean, invstd, m.cv * 4, mu, is);
    const f32x4 none = {0.f, 0.f, 0.f, 0.f};  // any non-zero relu is "mask from y" here: no recomputed mask, no scale / shift
    bn_bwd_sums(dy, x, y, m, P, C, relu ? 1 : 0, mu, is, none, none, s, q);
    bn_stage_rows(sm, m, C, s, q);
  }
  bn_fold_rows<false>(sm, m.rows, C, partial, nullptr, 0);
}

// coef[0][c] = mean(dz), coef[1][c] = mean(dz*xhat) (coef optional); dgamma/dbeta optional
__global__ void bn_bwd_finalize_kernel(const float* __restrict__ partial, int G, long P, int C, float* coef,
                                       float* dgamma, float* dbeta, int accumulate) {
  __shared__ double sm4[4];
  const int c = blockIdx.x;  // one 256-thread block per channel
  double s = 0.0, q = 0.0;
  for (int g = threadIdx.x; g < G; g += 256) {
    s += (double)partial[(long)g * 2 * C + c];
    q += (double)partial[(long)g * 2 * C + C + c];
  }
  s = block_sum_d(s, sm4);
  q = block_sum_d(q, sm4);
  if (threadIdx.x != 0) return;
  if (coef) {  // null: the frozen-statistics backward has no batch terms and wants the two parameter sums only
    coef[c] = (float)(s / (double)P);
    coef[C + c] = (float)(q / (double)P);
  }
  if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)q : (float)q;
  if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)s : (float)s;
}

// one 4-channel row of the train-mode backward: dx (=|+=) gamma*invstd*(dz - c1 - xhat*c2) ; dres (=|+=) dz
template <typename T>
__device__ __forceinline__ void bn_bwd_row(T* __restrict__ dx, T* __restrict__ dres, long o, f32x4 g, f32x4 xh, f32x4 gi, f32x4 c1,
                                           f32x4 c2, int acc_dx, int acc_dres) {
  f32x4 d = gi * (g - c1 - xh * c2);
  if (acc_dx) d += ld4(dx + o);
  st4(dx + o, d);
  if (dres) {
    f32x4 r = g;
    if (acc_dres) r += ld4(dres + o);
    st4(dres + o, r);
  }
}

// backward pass 2: dx = gamma*invstd*(dz - c1 - xhat*c2) ; dres (=|+=) dz
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                           const T* __restrict__ y,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ coef, T* __restrict__ dx,
                                                           T* __restrict__ dres, long P, int C, int relu,
                                                           int acc_dx, int acc_dres) {
  const ColMap m = col_map(C);
  if (!m.active) return;
  f32x4 mu, is, gi, c1, c2;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = m.cv * 4 + t;
    mu[t] = mean[c];
    is[t] = invstd[c];
    gi[t] = gamma[c] * invstd[c];
    c1[t] = coef[c];
    c2[t] = coef[C + c];
  }
  for (long p = (long)blockIdx.x * m.rows + m.prow; p < P; p += (long)gridDim.x * m.rows) {
    const long o = p * C + m.cv * 4;
    f32x4 g = ld4(dy + o);
    if (relu) g = bn_relu_mask(g, ld4(y + o));
    bn_bwd_row(dx, dres, o, g, (ld4(x + o) - mu) * is, gi, c1, c2, acc_dx, acc_dres);
  }
}

// ---- backward with FROZEN statistics (eval-mode BatchNorm, Engine.bn_batch_stats false): mean / invstd are constants, not
// functions of x, so the batch terms of the train-mode backward vanish and ONE pass does it:
//   dz = relu ? dy*(y>0) : dy ; dx (=|+=) dz*gamma*invstd ; dres (=|+=) dz
// The walk is bn_bwd_sums' with the dx / dres loads and stores woven into it, so it stays here (sharing it would make the
// shared walk branch on its caller); the mask, the LDS stage and the fold are the shared ones.
// SUMS: the workgroup also leaves partial[g][0][c] = sum dz, partial[g][1][c] = sum dz*xhat for bn_bwd_finalize_kernel
// (fixed order, fp64: run-to-run bitwise).  Without SUMS (gamma / beta frozen too) x and mean are never read: dy (+ y) in,
// dx out.  BN_U rows per thread in flight; rows past the end re-read row p (a cache hit), contribute an exact 0 to the sums
// and store nothing.
template <typename T, bool SUMS>
__global__ __launch_bounds__(256) void bn_eval_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                          const T* __restrict__ y, const float* __restrict__ mean,
                                                          const float* __restrict__ invstd,
                                                          const float* __restrict__ gamma, float* __restrict__ partial,
                                                          T* dx, T* dres, long P, int C, int relu, int acc_dx,
                                                          int acc_dres) {
  extern __shared__ float sm[];  // SUMS: [rows][2][C]
  const ColMap m = col_map(C);
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
  if (m.active) {
    f32x4 mu = {0.f, 0.f, 0.f, 0.f}, is, gi;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int c = m.cv * 4 + t;
      is[t] = invstd[c];
      gi[t] = gamma[c] * is[t];
      if (SUMS) mu[t] = mean[c];
    }
    const long step = (long)gridDim.x * m.rows;
    for (long p = (long)blockIdx.x * m.rows + m.prow; p < P; p += BN_U * step) {
      f32x4 g[BN_U], yy[BN_U], xx[BN_U], dd[BN_U], rr[BN_U];
      long o[BN_U];
#pragma unroll
      for (int u = 0; u < BN_U; ++u) {
        const long pu = p + u * step;
        o[u] = (pu < P ? pu : p) * C + m.cv * 4;
        g[u] = ld4(dy + o[u]);
      }
      if (relu) {
#pragma unroll
        for (int u = 0; u < BN_U; ++u) yy[u] = ld4(y + o[u]);
      }
      if (SUMS) {
#pragma unroll
        for (int u = 0; u < BN_U; ++u) xx[u] = ld4(x + o[u]);
      }
      if (acc_dx) {
#pragma unroll
        for (int u = 0; u < BN_U; ++u) dd[u] = ld4(dx + o[u]);
      }
      if (dres && acc_dres) {
#pragma unroll
        for (int u = 0; u < BN_U; ++u) rr[u] = ld4(dres + o[u]);
      }
#pragma unroll
      for (int u = 0; u < BN_U; ++u) {
        if (relu) g[u] = bn_relu_mask(g[u], yy[u]);
        const bool in = p + u * step < P;
        if (SUMS) {
          const f32x4 gz = in ? g[u] : f32x4{0.f, 0.f, 0.f, 0.f};
          s += gz;
          q += gz * ((xx[u] - mu) * is);
        }
        if (in) {
          f32x4 d = g[u] * gi;
          if (acc_dx) d += dd[u];
          st4(dx + o[u], d);
          if (dres) {
            f32x4 r = g[u];
            if (acc_dres) r += rr[u];
            st4(dres + o[u], r);
          }
        }
      }
    }
    if (SUMS) bn_stage_rows(sm, m, C, s, q);
  }
  if (SUMS) bn_fold_rows<false>(sm, m.rows, C, partial, nullptr, 0);
}

// ---- two-launch forms (fami_bn_train_fwd2 / fami_bn_bwd2): the statistics pass adds its per-workgroup partial sums into
// NS slot rows of fp64 (global_atomic_add_f64; slot = workgroup % NS, so an address sees grid/NS adds), and the apply
// pass folds the NS rows itself in its prologue -- the one-workgroup-per-channel finalize launch in between (4-6.6 us of
// pure dependent latency per BatchNorm, ~600 launches per training step) is gone.  The slots must be zero on entry
// (the caller hands out slices of an arena it clears once per step).  fp64 adds in arrival order: the sums are
// reproducible to ~1e-16 relative, i.e. the fp32 mean / invstd almost always bit for bit, but not guaranteed -- the
// three-launch forms above stay for the deterministic mode.
// (BN_NS_MAX, bn_slots, bn_slots_bytes, bn_slots_pivot live in common.h: the convolution epilogues fill the same rows)

template <typename T>
__global__ __launch_bounds__(256) void bn_partial2_kernel(const T* __restrict__ x, double* __restrict__ slots, int NS,
                                                          long P, int C) {
  extern __shared__ float sm[];  // [rows][2][C]
  const ColMap m = col_map(C);
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
  if (m.active) {
    bn_fwd_sums(x, m, P, C, s, q);
    bn_stage_rows(sm, m, C, s, q);
  }
  bn_fold_rows<true>(sm, m.rows, C, nullptr, slots, NS);
}

// y = [relu]( (x-mean)*invstd*gamma + beta [+ residual] ), mean / invstd folded from the slot rows by every workgroup
// (workgroup 0 also stores them and advances the running statistics)
template <typename T>
__global__ __launch_bounds__(256) void bn_apply2_kernel(const T* __restrict__ x, const double* __restrict__ slots, int NS,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const T* __restrict__ residual, T* __restrict__ y,
                                                        float* __restrict__ mean, float* __restrict__ invstd,
                                                        float* running_mean, float* running_var, long P, int C,
                                                        int relu, float momentum, float eps, const float* pivot) {
  // pivot: null = the sums were shifted by the first pixel x[0][c] (bn_partial2_kernel); else the [C] pivots the
  // convolution epilogue that filled the slots wrote behind them (conv.hip, EpiBN mode 1)
  extern __shared__ float sm[];  // [2][C]: scale, shift
  for (int c = threadIdx.x; c < C; c += 256) {
    double s, q;
    bn_fold_slots(slots, NS, C, c, s, q);
    const BnMoments mo = bn_moments_rcp(s, q, P, (double)(pivot ? pivot[c] : ld1(x + c)));
    const float muf = (float)mo.mu, isf = bn_invstd(mo.var, eps);
    if (blockIdx.x == 0) {
      mean[c] = muf;
      invstd[c] = isf;
      if (running_mean) bn_running_update(running_mean, running_var, c, mo.mu, mo.var, (double)P, momentum);
    }
    float sc, sf;
    bn_scale_shift(muf, isf, gamma[c], beta[c], sc, sf);
    sm[c] = sc;
    sm[C + c] = sf;
  }
  __syncthreads();
  const ColMap m = col_map(C);
  if (!m.active) return;
  const f32x4 sc = *reinterpret_cast<const f32x4*>(sm + m.cv * 4), sf = *reinterpret_cast<const f32x4*>(sm + C + m.cv * 4);
  for (long p = (long)blockIdx.x * m.rows + m.prow; p < P; p += (long)gridDim.x * m.rows) {
    const long o = p * C + m.cv * 4;
    const f32x4 xv = ld4(x + o);
    f32x4 v;
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = __builtin_fmaf(xv[t], sc[t], sf[t]);  // explicit: bn_relu_mask (relu 2) recomputes exactly this
    if (residual) v += ld4(residual + o);
    if (relu) {
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
    }
    st4(y + o, v);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_partial2_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                              const T* __restrict__ y, const float* __restrict__ mean,
                                                              const float* __restrict__ invstd,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta,
                                                              double* __restrict__ slots, int NS, long P, int C, int relu) {
  extern __shared__ float sm[];
  const ColMap m = col_map(C);
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
  if (m.active) {
    f32x4 mu, is, sc, sf;
    bn_load_stats(mean, invstd, m.cv * 4, mu, is);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float a, b;
      bn_scale_shift(mu[t], is[t], gamma[m.cv * 4 + t], beta[m.cv * 4 + t], a, b);
      sc[t] = a;
      sf[t] = b;
    }
    bn_bwd_sums(dy, x, y, m, P, C, relu, mu, is, sc, sf, s, q);
    bn_stage_rows(sm, m, C, s, q);
  }
  bn_fold_rows<true>(sm, m.rows, C, nullptr, slots, NS);
}

// dx = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)) ; dres (=|+=) dz ; the two means folded from the slot rows by
// every workgroup (workgroup 0 also stores dgamma / dbeta)
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply2_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                            const T* __restrict__ y, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            const double* __restrict__ slots, int NS, T* __restrict__ dx,
                                                            float* dgamma, float* dbeta, T* __restrict__ dres, long P,
                                                            int C, int relu, int acc_dx, int acc_param, int acc_dres) {
  extern __shared__ float sm[];  // [2][C]: mean(dz), mean(dz*xhat)
  for (int c = threadIdx.x; c < C; c += 256) {
    double s, q;
    bn_fold_slots(slots, NS, C, c, s, q);
    sm[c] = (float)(s / (double)P);
    sm[C + c] = (float)(q / (double)P);
    if (blockIdx.x == 0) {
      if (dgamma) dgamma[c] = acc_param ? dgamma[c] + (float)q : (float)q;
      if (dbeta) dbeta[c] = acc_param ? dbeta[c] + (float)s : (float)s;
    }
  }
  __syncthreads();
  const ColMap m = col_map(C);
  if (!m.active) return;
  f32x4 mu, is, gi, sc, sf;
  const f32x4 c1 = *reinterpret_cast<const f32x4*>(sm + m.cv * 4), c2 = *reinterpret_cast<const f32x4*>(sm + C + m.cv * 4);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = m.cv * 4 + t;
    mu[t] = mean[c];
    is[t] = invstd[c];
    gi[t] = gamma[c] * invstd[c];
    float a, b;
    bn_scale_shift(mu[t], is[t], gamma[c], beta[c], a, b);
    sc[t] = a;
    sf[t] = b;
  }
  for (long p = (long)blockIdx.x * m.rows + m.prow; p < P; p += (long)gridDim.x * m.rows) {
    const long o = p * C + m.cv * 4;
    f32x4 g = ld4(dy + o);
    const f32x4 xv = ld4(x + o);
    f32x4 yy = {0.f, 0.f, 0.f, 0.f};
    if (relu == 1) yy = ld4(y + o);
    g = bn_relu_mask(g, relu, yy, xv, sc, sf);
    bn_bwd_row(dx, dres, o, g, (xv - mu) * is, gi, c1, c2, acc_dx, acc_dres);
  }
}

// ---- small-tensor BatchNorm: statistics + apply (forward) / both reductions + apply (backward) in ONE launch.
// One workgroup per 4-channel column: the tensor of a low-resolution HRNet branch (P <= BN_SMALL_P pixels) is
// L2-resident, so the second pass re-reads it from cache and the three launches of the general path collapse
// into one (these layers are launch-latency bound, not bandwidth bound).  Same arithmetic: shifted moments,
// fp64 finalize, biased variance for normalisation / unbiased for running_var.
#define BN_SMALL_P 16384
// one workgroup per 4 channels is serial over pixels: measured slower than the three-launch path for everything but
// tiny tensors (the translation regressor's 16-channel maps below 24x18), where launch count is all that matters
// [fami_route_t] g_bn_small_elems (default 32768)  // fami_bn_tune_small: tensors up to this many elements take the one-launch kernels
static inline bool bn_small_ok(long P, int C) { return P * C <= g_bn_small_elems; }

__device__ __forceinline__ f32x4 block_sum4(f32x4 v, float* sm) {  // sm: 4 * 4 floats
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < 4; ++t) v[t] = wave_sum(v[t]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) sm[wave * 4 + t] = v[t];
  }
  __syncthreads();
  f32x4 r;
#pragma unroll
  for (int t = 0; t < 4; ++t) r[t] = (sm[t] + sm[4 + t]) + (sm[8 + t] + sm[12 + t]);
  return r;
}

template <typename T>
__global__ __launch_bounds__(256) void bn_small_fwd_kernel(const T* __restrict__ x, const T* __restrict__ residual,
                                                           T* __restrict__ y, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ mean,
                                                           float* __restrict__ invstd, float* running_mean,
                                                           float* running_var, long P, int C, int relu,
                                                           float momentum, float eps) {
  __shared__ float sm[16];
  const int c0 = blockIdx.x * 4;
  const f32x4 piv = ld4(x + c0);
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
  for (long p = threadIdx.x; p < P; p += 256) {
    const f32x4 v = ld4(x + p * C + c0) - piv;
    s += v;
    q += v * v;
  }
  s = block_sum4(s, sm);
  q = block_sum4(q, sm);
  f32x4 mu, is, sc, sf;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const BnMoments mo = bn_moments_div((double)s[t], (double)q[t], P, (double)piv[t]);
    mu[t] = (float)mo.mu;
    is[t] = bn_invstd(mo.var, eps);
    if (threadIdx.x == 0) {
      mean[c0 + t] = mu[t];
      invstd[c0 + t] = is[t];
      if (running_mean) bn_running_update(running_mean, running_var, c0 + t, mo.mu, mo.var, (double)P, momentum);
    }
    sc[t] = is[t] * gamma[c0 + t];
    sf[t] = beta[c0 + t] - mu[t] * sc[t];  // the compiler's contraction, as in bn_apply_kernel: not bn_scale_shift
  }
  for (long p = threadIdx.x; p < P; p += 256) {
    const long o = p * C + c0;
    f32x4 v = ld4(x + o) * sc + sf;
    if (residual) v += ld4(residual + o);
    if (relu) {
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
    }
    st4(y + o, v);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_small_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                           const T* __restrict__ y, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma, T* __restrict__ dx,
                                                           float* dgamma, float* dbeta, T* __restrict__ dres, long P,
                                                           int C, int relu, int acc_dx, int acc_param, int acc_dres) {
  __shared__ float sm[16];
  const int c0 = blockIdx.x * 4;
  f32x4 mu, is, gi;
  bn_load_stats(mean, invstd, c0, mu, is);
#pragma unroll
  for (int t = 0; t < 4; ++t) gi[t] = gamma[c0 + t] * is[t];
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
  for (long p = threadIdx.x; p < P; p += 256) {
    const long o = p * C + c0;
    f32x4 g = ld4(dy + o);
    if (relu) g = bn_relu_mask(g, ld4(y + o));
    s += g;
    q += g * ((ld4(x + o) - mu) * is);
  }
  s = block_sum4(s, sm);
  q = block_sum4(q, sm);
  f32x4 c1, c2;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    c1[t] = (float)((double)s[t] / (double)P);
    c2[t] = (float)((double)q[t] / (double)P);
    if (threadIdx.x == 0) {  // the float sums as they are: the other forms add (float) of an fp64 sum
      if (dgamma) dgamma[c0 + t] = acc_param ? dgamma[c0 + t] + q[t] : q[t];
      if (dbeta) dbeta[c0 + t] = acc_param ? dbeta[c0 + t] + s[t] : s[t];
    }
  }
  for (long p = threadIdx.x; p < P; p += 256) {
    const long o = p * C + c0;
    f32x4 g = ld4(dy + o);
    if (relu) g = bn_relu_mask(g, ld4(y + o));
    bn_bwd_row(dx, dres, o, g, (ld4(x + o) - mu) * is, gi, c1, c2, acc_dx, acc_dres);
  }
}

// per-channel sum over pixels (bias gradients): partial then finalize
template <typename T>
__global__ __launch_bounds__(256) void chan_sum_partial_kernel(const T* __restrict__ x,
                                                               float* __restrict__ partial, long P, int C) {
  // scalar-channel version: works for any C (17, 2, 288, ...); C > 256 walks the channels in strides of 256
  extern __shared__ float sm[];  // [rows][C]
  if (C > 256) {
    for (int c = threadIdx.x; c < C; c += 256) {
      float s = 0.f;
      for (long p = blockIdx.x; p < P; p += gridDim.x) s += ld1(x + p * C + c);
      partial[(long)blockIdx.x * C + c] = s;
    }
    return;
  }
  const int rows = max(1, 256 / C);
  const int c = threadIdx.x % C, prow = threadIdx.x / C;
  const bool active = prow < rows;
  float s = 0.f;
  if (active) {
    for (long p = (long)blockIdx.x * rows + prow; p < P; p += (long)gridDim.x * rows) s += ld1(x + p * C + c);
    sm[prow * C + c] = s;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < C; e += 256) {
    float tot = 0.f;
    for (int r = 0; r < rows; ++r) tot += sm[r * C + e];
    partial[(long)blockIdx.x * C + e] = tot;
  }
}
// four channels per thread, BN_U rows in flight (C % 4 == 0, C <= 1024): the bias gradients of the alignment head's 48-channel
// convolutions took 19 us per launch in the scalar form above (2-byte loads) against 3 us of HBM time
template <typename T>
__global__ __launch_bounds__(256) void chan_sum_partial4_kernel(const T* __restrict__ x, float* __restrict__ partial, long P,
                                                                int C) {
  extern __shared__ float sm[];  // [rows][C]
  const ColMap m = col_map(C);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (m.active) {
    const long step = (long)gridDim.x * m.rows;
    long p = (long)blockIdx.x * m.rows + m.prow;
    for (; p + (BN_U - 1) * step < P; p += BN_U * step) {
      f32x4 v[BN_U];
#pragma unroll
      for (int u = 0; u < BN_U; ++u) v[u] = ld4(x + (p + u * step) * C + m.cv * 4);
#pragma unroll
      for (int u = 0; u < BN_U; ++u) s += v[u];
    }
    for (; p < P; p += step) s += ld4(x + p * C + m.cv * 4);
    *reinterpret_cast<f32x4*>(sm + (long)m.prow * C + m.cv * 4) = s;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < C; e += 256) {
    float tot = 0.f;
    for (int r = 0; r < m.rows; ++r) tot += sm[r * C + e];
    partial[(long)blockIdx.x * C + e] = tot;
  }
}
__global__ void chan_sum_finalize_kernel(const float* __restrict__ partial, int G, int C, float* out,
                                         int accumulate) {
  __shared__ double sm4[4];
  const int c = blockIdx.x;  // one 256-thread block per channel
  double s = 0.0;
  for (int g = threadIdx.x; g < G; g += 256) s += (double)partial[(long)g * C + c];
  s = block_sum_d(s, sm4);
  if (threadIdx.x != 0) return;
  out[c] = accumulate ? out[c] + (float)s : (float)s;
}

static inline int bn_rows(int C) { return 256 / (C >> 2); }  // pixel rows a 256-thread workgroup covers at 4 channels per thread
// workgroups that give each `steps` row steps over P pixels, at most `cap` and at least one
static inline int bn_capped_grid(long P, int C, int steps, long cap) {
  const long per = (long)bn_rows(C) * steps;
  long g = (P + per - 1) / per;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}
// at least 2*BN_U row steps per workgroup: on the low-resolution branches (12x9x384: 1080 row groups) a grid of 512
// made the partial array as large as the tensor itself and the finalize pass, which walks it with a stride, the
// longer half of the chain
static inline int bn_grid(long P, int C) { return bn_capped_grid(P, C, 2 * BN_U, BN_MAXG); }
// the statistics passes of the two-launch forms write no partial array (fp64 slot atomics), so their grid is not tied to BN_MAXG:
// fami_bn_tune_small(-(1000 + n)) sets the cap (route field bn2_maxg)
// Measured inside the step (tools/ab_env.py, caps 512 / 1024 / 2048 / 4096): f32 storage 45.50 / 45.45 / 45.30 ms and 46.68 / - / 46.64 /
// 46.57 on a second box, config 4 (512x384, 8 frames) 116.8 / - / 116.5 / 116.2 ms; bf16 20.02 / 20.01 / 20.14 ms -- the f32 tensors of
// the stem stretch are twice the bytes and want more loads in flight: four times the cap in f32 storage.
static inline int bn_grid2(long P, int C, int esz) {
  return bn_capped_grid(P, C, 2 * BN_U, (long)g_bn2_maxg * (esz == 4 ? 4 : 1));
}
// apply passes, one row step at a time: the three-launch forms, and the two-launch forms whose every workgroup folds the slot
// rows in its prologue -- fewer, longer workgroups
static inline int bn_apply_grid(long P, int C) { return bn_capped_grid(P, C, 1, 2048); }
static inline int bn_apply_grid2(long P, int C) { return bn_capped_grid(P, C, 1, 1024); }
// FAMI_OK, or FAMI_ESHAPE with the error text set
static inline int bn_check_shape(long P, int C, const char* nm) {
  if (P > 0 && C >= 4 && (C % 4) == 0 && C <= 1024) return FAMI_OK;
  fami_set_error(nm, "C must be a multiple of 4, <= 1024");
  return FAMI_ESHAPE;
}

static inline size_t bn_stage_bytes(int C) { return (size_t)bn_rows(C) * 2 * C * sizeof(float); }  // the [rows][2][C] LDS stage

// ------------------------------------------------------------------ host side (templates over the storage type)
// the one-launch kernels, for both generations of the entry points
template <typename T>
static int bn_small_fwd_launch(const T* x, const T* residual, T* y, const float* gamma, const float* beta, float* mean,
                               float* invstd, float* running_mean, float* running_var, long P, int C, int relu,
                               float momentum, float eps, hipStream_t s, const char* nm) {
  hipLaunchKernelGGL(bn_small_fwd_kernel<T>, dim3(C / 4), dim3(256), 0, s, x, residual, y, gamma, beta, mean, invstd,
                     running_mean, running_var, P, C, relu, momentum, eps);
  FAMI_CHECK_LAUNCH(nm);
  return FAMI_OK;
}
template <typename T>
static int bn_small_bwd_launch(const T* dy, const T* x, const T* y, const float* mean, const float* invstd,
                               const float* gamma, T* dx, float* dgamma, float* dbeta, T* dres, long P, int C, int relu,
                               int acc_dx, int acc_param, int acc_dres, hipStream_t s, const char* nm) {
  hipLaunchKernelGGL(bn_small_bwd_kernel<T>, dim3(C / 4), dim3(256), 0, s, dy, x, y, mean, invstd, gamma, dx, dgamma,
                     dbeta, dres, P, C, relu, acc_dx, acc_param, acc_dres);
  FAMI_CHECK_LAUNCH(nm);
  return FAMI_OK;
}

template <typename T>
static int bn_stats_impl(const T* x, long P, int C, float* mean, float* invstd, float* running_mean,
                         float* running_var, float momentum, float eps, float* ws, hipStream_t s, const char* nm) {
  FAMI_REQUIRE(x && mean && invstd && ws, nm, "null pointer");
  if (const int rc = bn_check_shape(P, C, nm)) return rc;
  const int G = bn_grid(P, C);
  hipLaunchKernelGGL(bn_partial_kernel<T>, dim3(G), dim3(256), bn_stage_bytes(C), s, x, ws, P, C);
  FAMI_CHECK_LAUNCH(nm);
  hipLaunchKernelGGL(bn_finalize_kernel<T>, dim3(C), dim3(256), 0, s, ws, x, G, P, C, mean, invstd, running_mean,
                     running_var, momentum, eps);
  FAMI_CHECK_LAUNCH(nm);
  return FAMI_OK;
}

template <typename T>
static int bn_apply_impl(const T* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                         const T* residual, T* y, long P, int C, int relu, hipStream_t s, const char* nm) {
  FAMI_REQUIRE(x && mean && invstd && gamma && beta && y, nm, "null pointer");
  if (const int rc = bn_check_shape(P, C, nm)) return rc;
  hipLaunchKernelGGL(bn_apply_kernel<T>, dim3(bn_apply_grid(P, C)), dim3(256), 0, s, x, mean, invstd, gamma, beta, residual, y, P,
                     C, relu);
  FAMI_CHECK_LAUNCH(nm);
  return FAMI_OK;
}

template <typename T>
static int bn_bwd_impl(const T* dy, const T* x, const T* y, const float* mean, const float* invstd,
                       const float* gamma, T* dx, float* dgamma, float* dbeta, T* dres, long P, int C, int relu,
                       int acc_dx, int acc_param, int acc_dres, float* ws, hipStream_t s, const char* nm) {
  FAMI_REQUIRE(dy && x && mean && invstd && gamma && dx && ws, nm, "null pointer");
  FAMI_REQUIRE(!relu || y, nm, "relu needs y");
  if (const int rc = bn_check_shape(P, C, nm)) return rc;
  if (bn_small_ok(P, C))  // low-resolution branches: one launch (see bn_small_bwd_kernel)
    return bn_small_bwd_launch<T>(dy, x, y, mean, invstd, gamma, dx, dgamma, dbeta, dres, P, C, relu, acc_dx, acc_param, acc_dres, s, nm);
  const int G = bn_grid(P, C);
  float* coef = ws + (long)BN_MAXG * 2 * C - 2 * C;  // tail of the workspace (G < BN_MAXG leaves it free)
  const int Gp = G < BN_MAXG ? G : BN_MAXG - 1;
  hipLaunchKernelGGL(bn_bwd_partial_kernel<T>, dim3(Gp), dim3(256), bn_stage_bytes(C), s, dy, x, y, mean, invstd, ws, P,
                     C, relu);
  FAMI_CHECK_LAUNCH(nm);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(256), 0, s, ws, Gp, P, C, coef, dgamma, dbeta, acc_param);
  FAMI_CHECK_LAUNCH(nm);
  hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, dim3(bn_apply_grid(P, C)), dim3(256), 0, s, dy, x, y, mean, invstd, gamma, coef, dx,
                     dres, P, C, relu, acc_dx, acc_dres);
  FAMI_CHECK_LAUNCH(nm);
  return FAMI_OK;
}

// frozen-statistics backward: one data pass (+ a channel-sized finalize when dgamma / dbeta are wanted)
template <typename T>
static int bn_eval_bwd_impl(const T* dy, const T* x, const T* y, const float* mean, const float* invstd,
                            const float* gamma, T* dx, float* dgamma, float* dbeta, T* dres, long P, int C, int relu,
                            int acc_dx, int acc_param, int acc_dres, float* ws, hipStream_t s, const char* nm) {
  FAMI_REQUIRE(dy && invstd && gamma && dx, nm, "null pointer");
  FAMI_REQUIRE(!relu || y, nm, "relu needs y");
  if (const int rc = bn_check_shape(P, C, nm)) return rc;
  if (!dgamma && !dbeta) {  // gamma / beta frozen too: no sums, no workspace, no second launch; x and mean are not read
    hipLaunchKernelGGL((bn_eval_bwd_kernel<T, false>), dim3(bn_capped_grid(P, C, BN_U, 2048)), dim3(256), 0, s, dy, x, y, mean, invstd, gamma,
                       (float*)nullptr, dx, dres, P, C, relu, acc_dx, acc_dres);
    FAMI_CHECK_LAUNCH(nm);
    return FAMI_OK;
  }
  FAMI_REQUIRE(x && mean && ws, nm, "parameter sums need x, mean and ws");
  const int G = bn_grid(P, C);  // <= BN_MAXG partial rows: the whole of fami_bn_workspace(C)
  hipLaunchKernelGGL((bn_eval_bwd_kernel<T, true>), dim3(G), dim3(256), bn_stage_bytes(C), s, dy, x, y, mean, invstd,
                     gamma, ws, dx, dres, P, C, relu, acc_dx, acc_dres);
  FAMI_CHECK_LAUNCH(nm);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(256), 0, s, ws, G, P, C, (float*)nullptr, dgamma, dbeta,
                     acc_param);
  FAMI_CHECK_LAUNCH(nm);
  return FAMI_OK;
}

// train-mode BatchNorm forward in one call: statistics (+ running-stat update) and apply (+ residual, + ReLU).
// Small tensors take the single-launch kernel, large ones the three-launch path.
template <typename T>
static int bn_train_fwd_impl(const T* x, const T* residual, T* y, const float* gamma, const float* beta, float* mean,
                             float* invstd, float* running_mean, float* running_var, long P, int C, int relu,
                             float momentum, float eps, float* ws, hipStream_t s, const char* nm) {
  FAMI_REQUIRE(x && y && gamma && beta && mean && invstd && ws, nm, "null pointer");
  if (const int rc = bn_check_shape(P, C, nm)) return rc;
  if (bn_small_ok(P, C))
    return bn_small_fwd_launch<T>(x, residual, y, gamma, beta, mean, invstd, running_mean, running_var, P, C, relu, momentum, eps, s, nm);
  int rc = bn_stats_impl<T>(x, P, C, mean, invstd, running_mean, running_var, momentum, eps, ws, s, nm);
  if (rc != FAMI_OK) return rc;
  return bn_apply_impl<T>(x, mean, invstd, gamma, beta, residual, y, P, C, relu, s, nm);
}

// two-launch forms: `slots` = fami_bn_slots_bytes(C) bytes, ZERO on entry
template <typename T>
static int bn_train_fwd2_impl(const T* x, const T* residual, T* y, const float* gamma, const float* beta, float* mean,
                              float* invstd, float* running_mean, float* running_var, long P, int C, int relu,
                              float momentum, float eps, void* slots, int pre, hipStream_t s, const char* nm) {
  FAMI_REQUIRE(x && y && gamma && beta && mean && invstd && slots, nm, "null pointer");
  if (const int rc = bn_check_shape(P, C, nm)) return rc;
  if (bn_small_ok(P, C) && !pre)
    return bn_small_fwd_launch<T>(x, residual, y, gamma, beta, mean, invstd, running_mean, running_var, P, C, relu, momentum, eps, s, nm);
  const int G = bn_grid2(P, C, (int)sizeof(T)), NS = bn_slots(C);
  if (!pre) {   // pre: the producing convolution's epilogue has filled the slot rows and the pivots already
    hipLaunchKernelGGL(bn_partial2_kernel<T>, dim3(G), dim3(256), bn_stage_bytes(C), s, x, reinterpret_cast<double*>(slots), NS,
                       P, C);
    FAMI_CHECK_LAUNCH(nm);
  }
  hipLaunchKernelGGL(bn_apply2_kernel<T>, dim3(bn_apply_grid2(P, C)), dim3(256), (size_t)2 * C * sizeof(float), s, x,
                     reinterpret_cast<const double*>(slots), NS, gamma, beta, residual, y, mean, invstd, running_mean,
                     running_var, P, C, relu, momentum, eps, pre ? bn_slots_pivot(slots, C) : (const float*)nullptr);
  FAMI_CHECK_LAUNCH(nm);
  return FAMI_OK;
}

template <typename T>
static int bn_bwd2_impl(const T* dy, const T* x, const T* y, const float* mean, const float* invstd, const float* gamma,
                        const float* beta, T* dx, float* dgamma, float* dbeta, T* dres, long P, int C, int relu,
                        int acc_dx, int acc_param, int acc_dres, void* slots, int pre, hipStream_t s, const char* nm) {
  FAMI_REQUIRE(dy && x && mean && invstd && gamma && beta && dx && slots, nm, "null pointer");
  FAMI_REQUIRE(relu != 1 || y, nm, "relu = 1 needs y");
  FAMI_REQUIRE(relu >= 0 && relu <= 2, nm, "relu must be 0, 1 (mask from y) or 2 (mask recomputed from x)");
  if (const int rc = bn_check_shape(P, C, nm)) return rc;
  if (bn_small_ok(P, C) && !pre) {  // the one-launch kernel takes its mask from y
    FAMI_REQUIRE(relu != 2 || y, nm, "small tensors take the ReLU mask from y");
    return bn_small_bwd_launch<T>(dy, x, y, mean, invstd, gamma, dx, dgamma, dbeta, dres, P, C, relu ? 1 : 0, acc_dx, acc_param, acc_dres, s, nm);
  }
  const int G = bn_grid2(P, C, (int)sizeof(T)), NS = bn_slots(C);
  if (!pre) {   // pre: the input-gradient convolution that produced dy summed dz and dz*xhat in its epilogue
    hipLaunchKernelGGL(bn_bwd_partial2_kernel<T>, dim3(G), dim3(256), bn_stage_bytes(C), s, dy, x, y, mean, invstd, gamma, beta,
                       reinterpret_cast<double*>(slots), NS, P, C, relu);
    FAMI_CHECK_LAUNCH(nm);
  }
  hipLaunchKernelGGL(bn_bwd_apply2_kernel<T>, dim3(bn_apply_grid2(P, C)), dim3(256), (size_t)2 * C * sizeof(float), s, dy, x,
                     y, mean, invstd, gamma, beta, reinterpret_cast<const double*>(slots), NS, dx, dgamma, dbeta, dres, P,
                     C, relu, acc_dx, acc_param, acc_dres);
  FAMI_CHECK_LAUNCH(nm);
  return FAMI_OK;
}

template <typename T>
static int channel_sum_impl(const T* x, long P, int C, float* out, int accumulate, float* ws, hipStream_t s,
                            const char* nm) {
  FAMI_REQUIRE(x && out && ws && P > 0 && C > 0, nm, "bad argument");
  FAMI_REQUIRE(C <= 4096, nm, "C > 4096 unsupported");
  int rows = C > 256 ? 1 : 256 / C;
  const bool vec4 = C % 4 == 0 && C <= 1024 && P >= 4096;
  if (vec4) rows = bn_rows(C);
  long g = (P + rows - 1) / rows;
  if (vec4) g = (g + 2 * BN_U - 1) / (2 * BN_U);          // at least 2 BN_U row steps per workgroup
  if (g > BN_MAXG) g = BN_MAXG;
  if (g < 1) g = 1;
  if (vec4) hipLaunchKernelGGL(chan_sum_partial4_kernel<T>, dim3((int)g), dim3(256), (size_t)rows * C * sizeof(float), s, x, ws, P, C);
  else hipLaunchKernelGGL(chan_sum_partial_kernel<T>, dim3((int)g), dim3(256), C > 256 ? 0 : (size_t)rows * C * sizeof(float), s, x, ws, P, C);
  FAMI_CHECK_LAUNCH(nm);
  hipLaunchKernelGGL(chan_sum_finalize_kernel, dim3(C), dim3(256), 0, s, ws, (int)g, C, out, accumulate);
  FAMI_CHECK_LAUNCH(nm);
  return FAMI_OK;
}

extern "C" {

long fami_bn_workspace(int C) { return (long)BN_MAXG * 2 * C * (long)sizeof(float); }
long fami_bn_slots_bytes(int C) { return bn_slots_bytes(C); }
int fami_bn_tune_small(long elems) {
  if (elems <= -1000) { g_bn2_maxg = (int)(-elems - 1000); return FAMI_OK; }      // benchmarks: grid cap of the two-launch statistics passes
  if (elems < 0) { g_bn_small_elems = 32768; g_bn2_maxg = 512; return FAMI_OK; }
  g_bn_small_elems = elems;
  return FAMI_OK;
}
int fami_bn_is_small(long P, int C) { return bn_small_ok(P, C) ? 1 : 0; }
long fami_channel_sum_workspace(int C) { return (long)BN_MAXG * C * (long)sizeof(float); }

int fami_bn_eval_stats_f32(const float* running_mean, const float* running_var, float* mean, float* invstd, int C,
                           float eps, hipStream_t s) {
  FAMI_REQUIRE(running_mean && running_var && mean && invstd && C > 0, "fami_bn_eval_stats_f32", "bad argument");
  hipLaunchKernelGGL(bn_eval_stats_kernel, dim3(fami_cdiv(C, 64)), dim3(64), 0, s, running_mean, running_var, mean,
                     invstd, C, eps);
  FAMI_CHECK_LAUNCH("fami_bn_eval_stats_f32");
  return FAMI_OK;
}

int fami_bn_finalize_slots_f32(void* slots, long P, int C, float* mean, float* invstd, float* running_mean,
                               float* running_var, float momentum, float eps, hipStream_t s) {
  FAMI_REQUIRE(slots && mean && invstd && C > 0 && P > 0, "fami_bn_finalize_slots_f32", "bad argument");
  hipLaunchKernelGGL(bn_finalize_slots_kernel, dim3(fami_cdiv(C, 64)), dim3(64), 0, s, reinterpret_cast<const double*>(slots),
                     bn_slots(C), bn_slots_pivot(slots, C), P, C, mean, invstd, running_mean, running_var, momentum, eps);
  FAMI_CHECK_LAUNCH("fami_bn_finalize_slots_f32");
  return FAMI_OK;
}

int fami_bn_running_update_f32(float* running_mean, float* running_var, const float* mean, const float* invstd, int C,
                               long P, float momentum, float eps, hipStream_t s) {
  FAMI_REQUIRE(running_mean && running_var && mean && invstd && C > 0 && P > 0, "fami_bn_running_update_f32", "bad argument");
  hipLaunchKernelGGL(bn_running_update_kernel, dim3(fami_cdiv(C, 64)), dim3(64), 0, s, running_mean, running_var, mean,
                     invstd, C, P, momentum, eps);
  FAMI_CHECK_LAUNCH("fami_bn_running_update_f32");
  return FAMI_OK;
}


// n deferred running-statistics updates in call order: ptrs = host array of 4 n longs (running_mean, running_var, mean,
// invstd per entry), meta = host array of 4 n floats (C, P, momentum, eps per entry; C and P are exact in fp32 here).
int fami_bn_running_update_batch_f32(const long* ptrs, const float* meta, int n, hipStream_t s) {
  FAMI_REQUIRE(ptrs && meta && n > 0, "fami_bn_running_update_batch_f32", "bad argument");
  for (int i0 = 0; i0 < n; i0 += FAMI_BNRU_BATCH) {
    BnRunBatch b;
    b.n = n - i0 < FAMI_BNRU_BATCH ? n - i0 : FAMI_BNRU_BATCH;
    int maxc = 1;
    for (int i = 0; i < FAMI_BNRU_BATCH; ++i) {
      const int j = i < b.n ? i0 + i : i0;
      b.rm[i] = reinterpret_cast<float*>(ptrs[4 * j]);
      b.rv[i] = reinterpret_cast<float*>(ptrs[4 * j + 1]);
      b.mean[i] = reinterpret_cast<const float*>(ptrs[4 * j + 2]);
      b.invstd[i] = reinterpret_cast<const float*>(ptrs[4 * j + 3]);
      b.C[i] = (int)meta[4 * j];
      b.P[i] = meta[4 * j + 1];
      b.mom[i] = meta[4 * j + 2];
      b.eps[i] = meta[4 * j + 3];
      if (i < b.n && b.C[i] > maxc) maxc = b.C[i];
    }
    hipLaunchKernelGGL(bn_running_update_batch_kernel, dim3(fami_cdiv(maxc, 256)), dim3(256), 0, s, b);
    FAMI_CHECK_LAUNCH("fami_bn_running_update_batch_f32");
  }
  return FAMI_OK;
}

#define FAMI_BN_ABI(sfx, T)                                                                                            \
  /* train-mode statistics: mean/invstd out, running stats updated in place (may be null) */                          \
  int fami_bn_stats_##sfx(const T* x, long P, int C, float* mean, float* invstd, float* running_mean,                  \
                          float* running_var, float momentum, float eps, float* ws, hipStream_t s) {                   \
    return bn_stats_impl<T>(x, P, C, mean, invstd, running_mean, running_var, momentum, eps, ws, s, "fami_bn_stats_" #sfx); \
  }                                                                                                                    \
  int fami_bn_apply_##sfx(const T* x, const float* mean, const float* invstd, const float* gamma, const float* beta,   \
                          const T* residual, T* y, long P, int C, int relu, hipStream_t s) {                           \
    return bn_apply_impl<T>(x, mean, invstd, gamma, beta, residual, y, P, C, relu, s, "fami_bn_apply_" #sfx);          \
  }                                                                                                                    \
  /* dz = relu ? dy*(y>0) : dy ; dx (=|+=) BN-backward(dz) ; dgamma/dbeta (=|+=) ; dres (=|+=) dz */                   \
  int fami_bn_bwd_##sfx(const T* dy, const T* x, const T* y, const float* mean, const float* invstd,                   \
                        const float* gamma, T* dx, float* dgamma, float* dbeta, T* dres, long P, int C, int relu,      \
                        int acc_dx, int acc_param, int acc_dres, float* ws, hipStream_t s) {                           \
    return bn_bwd_impl<T>(dy, x, y, mean, invstd, gamma, dx, dgamma, dbeta, dres, P, C, relu, acc_dx, acc_param,       \
                          acc_dres, ws, s, "fami_bn_bwd_" #sfx);                                                       \
  }                                                                                                                    \
  /* the same with mean / invstd FROZEN (eval-mode statistics): dx (=|+=) dz*gamma*invstd, dgamma (=|+=) sum dz*xhat, */ \
  /* dbeta (=|+=) sum dz, in one data pass; dgamma and dbeta both null: no sums, ws / x / mean unused                 */ \
  int fami_bn_eval_bwd_##sfx(const T* dy, const T* x, const T* y, const float* mean, const float* invstd,              \
                             const float* gamma, T* dx, float* dgamma, float* dbeta, T* dres, long P, int C, int relu, \
                             int acc_dx, int acc_param, int acc_dres, float* ws, hipStream_t s) {                      \
    return bn_eval_bwd_impl<T>(dy, x, y, mean, invstd, gamma, dx, dgamma, dbeta, dres, P, C, relu, acc_dx, acc_param,  \
                               acc_dres, ws, s, "fami_bn_eval_bwd_" #sfx);                                             \
  }                                                                                                                    \
  /* train-mode forward, statistics + apply in one call (one launch for P <= 16384 pixels) */                         \
  int fami_bn_train_fwd_##sfx(const T* x, const T* residual, T* y, const float* gamma, const float* beta,              \
                              float* mean, float* invstd, float* running_mean, float* running_var, long P, int C,      \
                              int relu, float momentum, float eps, float* ws, hipStream_t s) {                         \
    return bn_train_fwd_impl<T>(x, residual, y, gamma, beta, mean, invstd, running_mean, running_var, P, C, relu,      \
                                momentum, eps, ws, s, "fami_bn_train_fwd_" #sfx);                                      \
  }                                                                                                                    \
  /* two-launch forms (statistics with fp64 slot atomics + apply that folds the slots itself): `slots` =           */ \
  /* fami_bn_slots_bytes(C) bytes, ZERO on entry.  relu (backward): 0 none, 1 mask from y, 2 mask recomputed from x   */ \
  /* (no residual; y may be null) -- valid against fami_bn_train_fwd2 only.                                           */ \
  int fami_bn_train_fwd2_##sfx(const T* x, const T* residual, T* y, const float* gamma, const float* beta,             \
                               float* mean, float* invstd, float* running_mean, float* running_var, long P, int C,     \
                               int relu, float momentum, float eps, void* slots, hipStream_t s) {                      \
    return bn_train_fwd2_impl<T>(x, residual, y, gamma, beta, mean, invstd, running_mean, running_var, P, C, relu,     \
                                 momentum, eps, slots, 0, s, "fami_bn_train_fwd2_" #sfx);                              \
  }                                                                                                                    \
  /* the same with the statistics pass already done: `slots` was filled by fami_conv2d_fwd_stats_* (sums + pivots) */  \
  int fami_bn_apply_slots_##sfx(const T* x, const T* residual, T* y, const float* gamma, const float* beta,            \
                                float* mean, float* invstd, float* running_mean, float* running_var, long P, int C,    \
                                int relu, float momentum, float eps, void* slots, hipStream_t s) {                     \
    return bn_train_fwd2_impl<T>(x, residual, y, gamma, beta, mean, invstd, running_mean, running_var, P, C, relu,     \
                                 momentum, eps, slots, 1, s, "fami_bn_apply_slots_" #sfx);                             \
  }                                                                                                                    \
  /* backward apply pass alone: `slots` was filled by fami_conv2d_dgrad_bnstats_* (sums of dz and dz*xhat); dy holds  */\
  /* dz (the ReLU mask is applied already), so no mask is taken here                                                  */\
  int fami_bn_bwd_apply_slots_##sfx(const T* dz, const T* x, const float* mean, const float* invstd,                   \
                                    const float* gamma, const float* beta, T* dx, float* dgamma, float* dbeta,         \
                                    T* dres, long P, int C, int acc_dx, int acc_param, int acc_dres, void* slots,      \
                                    hipStream_t s) {                                                                   \
    return bn_bwd2_impl<T>(dz, x, (const T*)nullptr, mean, invstd, gamma, beta, dx, dgamma, dbeta, dres, P, C, 0,      \
                           acc_dx, acc_param, acc_dres, slots, 1, s, "fami_bn_bwd_apply_slots_" #sfx);                 \
  }                                                                                                                    \
  int fami_bn_bwd2_##sfx(const T* dy, const T* x, const T* y, const float* mean, const float* invstd,                  \
                         const float* gamma, const float* beta, T* dx, float* dgamma, float* dbeta, T* dres, long P,   \
                         int C, int relu, int acc_dx, int acc_param, int acc_dres, void* slots, hipStream_t s) {       \
    return bn_bwd2_impl<T>(dy, x, y, mean, invstd, gamma, beta, dx, dgamma, dbeta, dres, P, C, relu, acc_dx,           \
                           acc_param, acc_dres, slots, 0, s, "fami_bn_bwd2_" #sfx);                                    \
  }                                                                                                                    \
  /* out[c] (=|+=) sum_p x[p][c] */                                                                      \
  int fami_channel_sum_##sfx(const T* x, long P, int C, float* out, int accumulate, float* ws, hipStream_t s) {        \
    return channel_sum_impl<T>(x, P, C, out, accumulate, ws, s, "fami_channel_sum_" #sfx);                             \
  }
FAMI_BN_ABI(f32, float)
FAMI_BN_ABI(bf16, bf16_t)
FAMI_BN_ABI(f16, f16_t)
#undef FAMI_BN_ABI

}  // extern "C"
