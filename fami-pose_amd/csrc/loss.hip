// On-device targets, losses and decode for the heatmap head.  All tensors here
// are at the NCHW boundary: rows are (b, joint) or (b, channel) with H*W
// contiguous, which is what every reduction below runs over.
//
// Replaces
//   datasets/process/heatmaps_process.py:146-203  generate_heatmaps (Gaussian targets, sigma 3)
//   posetimation/loss/mse_loss.py:21-40           JointMSELoss.forward
//   posetimation/zoo/Alignment/Alignment_V15.py:250-277  the two MI estimators
//       kl_div(input=softmax(A/T) (probabilities!), target=softmax(Bt/T), 'mean'), T = 0.05
//   datasets/process/heatmaps_process.py:16-44    get_max_preds (flat argmax, first max on ties)
#include "common.h"

// joints [B,J,2] (x,y in input-image pixels), vis [B,J] -> target [B,J,Hh,Wh], weight [B,J]
// joint_w (or null): per-joint factors of the stored weight (heatmaps_process.py:200-201); the "> 0.5" test that decides
// whether a map is drawn stays on the unmultiplied weight (:195-196).
// SUB: the Gaussian is centred at the real-valued joint position (DARK's encoding) inside the window of the rounded
// centre; (float)((double)x - joint / stride) is the integer x - mx whenever joint / stride is a non-negative integer, so
// such a joint gets the quantised map bit for bit.
template <bool SUB>
__global__ void gauss_target_kernel(const float* __restrict__ joints, const float* __restrict__ vis,
                                    const float* __restrict__ joint_w, float* __restrict__ target,
                                    float* __restrict__ weight, int B, int J, int Hh, int Wh, double stride_x,
                                    double stride_y, int sigma) {
  const long HW = (long)Hh * Wh;
  const long total = (long)B * J * HW;
  const int r = sigma * 3;
  const float inv = (float)(2 * sigma * sigma);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long bj = i / HW;
    const int hw = (int)(i - bj * HW);
    const int y = hw / Wh, x = hw - y * Wh;
    // int(v + 0.5) of the reference truncates toward zero, in double
    const double cx = (double)joints[bj * 2 + 0] / stride_x, cy = (double)joints[bj * 2 + 1] / stride_y;
    const int mx = (int)(cx + 0.5);
    const int my = (int)(cy + 0.5);
    const int x0 = mx - r, y0 = my - r, x1 = mx + r + 1, y1 = my + r + 1;
    float w = vis[bj];
    const bool outside = x0 >= Wh || y0 >= Hh || x1 < 0 || y1 < 0;
    if (outside) w = 0.f;
    float v = 0.f;
    if (!outside && w > 0.5f && x >= x0 && x < x1 && y >= y0 && y < y1) {
      if constexpr (SUB) {
        const float dx = (float)((double)x - cx), dy = (float)((double)y - cy);
        v = expf(-(dx * dx + dy * dy) / inv);
      } else {
        const int dx = x - mx, dy = y - my;
        v = expf(-((float)(dx * dx + dy * dy)) / inv);
      }
    }
    target[i] = v;
    if (hw == 0) weight[bj] = joint_w ? w * joint_w[bj % J] : w;
  }
}

__device__ __forceinline__ float block_sum(float v, float* sm) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  return sm[0] + sm[1] + sm[2] + sm[3];
}
__device__ __forceinline__ float block_max(float v, float* sm) {
  v = wave_max(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  return fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}

// rowsum[r] = sum_p (w_r * (pred - gt))^2
__global__ __launch_bounds__(256) void wmse_rows_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                        const float* __restrict__ w, float* __restrict__ rowsum,
                                                        int L) {
  __shared__ float sm[4];
  const long r = blockIdx.x;
  const float wr = w ? w[r] : 1.f;
  float s = 0.f;
  for (int l = threadIdx.x; l < L; l += 256) {
    const float d = pred[r * L + l] * wr - gt[r * L + l] * wr;
    s += d * d;
  }
  s = block_sum(s, sm);
  if (threadIdx.x == 0) rowsum[r] = s;
}
__global__ void scalar_sum_kernel(const float* __restrict__ rows, int R, double scale, float* out) {
  __shared__ double sm[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < R; i += 256) s += (double)rows[i];
  s = wave_sum_d(s);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sm[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (float)((sm[0] + sm[1] + sm[2] + sm[3]) * scale);
}
// Online hard keypoint mining: one workgroup walks the samples.  Per sample the J row sums go to LDS, joint j counts the
// joints ranked before it -- larger first, equal values by lower index, NaN above every number (torch.topk's order) -- and is
// selected when fewer than k are.  sel_w[b,j] = w[b,j] (1 without w) if selected else 0;
// loss[0] = scale * sum over the selected row sums, in fp64: per thread in (b, j) order, then lanes, then waves.
__global__ __launch_bounds__(256) void ohkm_select_kernel(const float* __restrict__ rows, const float* __restrict__ w,
                                                          float* __restrict__ sel_w, float* __restrict__ loss, int B,
                                                          int J, int k, double scale) {
  extern __shared__ float row[];      // J floats
  __shared__ double sm[4];
  double s = 0.0;
  for (int b = 0; b < B; ++b) {
    __syncthreads();
    for (int j = threadIdx.x; j < J; j += 256) row[j] = rows[(long)b * J + j];
    __syncthreads();
    for (int j = threadIdx.x; j < J; j += 256) {
      const float vj = row[j];
      const bool nj = vj != vj;
      int before = 0;
      for (int i = 0; i < J; ++i) {
        const float vi = row[i];
        const bool ni = vi != vi;
        const bool first = ni != nj ? ni : ((ni || vi == vj) ? i < j : vi > vj);
        before += first ? 1 : 0;
      }
      const bool sel = before < k;
      sel_w[(long)b * J + j] = sel ? (w ? w[(long)b * J + j] : 1.f) : 0.f;
      if (sel) s += (double)vj;
    }
  }
  s = wave_sum_d(s);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sm[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (float)((sm[0] + sm[1] + sm[2] + sm[3]) * scale);
}
// dpred = g * 2 w^2 (pred - gt) * scale
__global__ void wmse_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                const float* __restrict__ w, float* __restrict__ dpred, long n, int L, float scale,
                                const float* gdev, int accumulate) {
  const float g = gdev ? gdev[0] * scale : scale;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float wr = w ? w[i / L] : 1.f;
    const float v = 2.f * g * wr * (pred[i] * wr - gt[i] * wr);
    dpred[i] = accumulate ? dpred[i] + v : v;
  }
}

// per row: stats[r] = {max_a, sum_a, max_b, sum_b, S = sum_l t_l*(log t_l + 1 - a_l)}, rowval[r] = sum_l t(log t - a)
// REG > 0: the row lives in registers (REG values per thread, L <= 256 * REG): all loads are requested up front and the
// three passes run out of registers.  The streaming form below walked the row three times with one dependent load per
// thread in flight -- 31 us per call for 68-192 rows of 6912 floats, six calls on the head's serial chain (the MI terms).
template <int REG>
__global__ __launch_bounds__(256) void softmax_kl_rows_kernel(const float* __restrict__ A,
                                                              const float* __restrict__ Bt,
                                                              float* __restrict__ stats, float* __restrict__ rowval,
                                                              int L, float temperature) {
  __shared__ float sm[4];
  const long r = blockIdx.x;
  const float* a = A + r * L;
  const float* b = Bt + r * L;
  constexpr int NR = REG > 0 ? REG : 1;
  float av[NR], bv[NR];
  if constexpr (REG > 0) {
#pragma unroll
    for (int j = 0; j < REG; ++j) {
      const int l = threadIdx.x + j * 256;
      av[j] = l < L ? a[l] / temperature : -INFINITY;
      bv[j] = l < L ? b[l] / temperature : -INFINITY;
    }
  }
  float ma = -INFINITY, mb = -INFINITY;
  if constexpr (REG > 0) {
#pragma unroll
    for (int j = 0; j < REG; ++j) {
      ma = fmaxf(ma, av[j]);
      mb = fmaxf(mb, bv[j]);
    }
  } else {
    for (int l = threadIdx.x; l < L; l += 256) {
      ma = fmaxf(ma, a[l] / temperature);
      mb = fmaxf(mb, b[l] / temperature);
    }
  }
  ma = block_max(ma, sm);
  mb = block_max(mb, sm);
  float sa = 0.f, sb = 0.f;
  if constexpr (REG > 0) {
#pragma unroll
    for (int j = 0; j < REG; ++j) {
      if (threadIdx.x + j * 256 < L) {
        sa += expf(av[j] - ma);
        sb += expf(bv[j] - mb);
      }
    }
  } else {
    for (int l = threadIdx.x; l < L; l += 256) {
      sa += expf(a[l] / temperature - ma);
      sb += expf(b[l] / temperature - mb);
    }
  }
  sa = block_sum(sa, sm);
  sb = block_sum(sb, sm);
  float val = 0.f, S = 0.f;
  auto term = [&](float al, float bl) {
    const float pa = expf(al - ma) / sa;
    const float t = expf(bl - mb) / sb;
    if (t > 0.f) {
      const float lt = logf(t);
      val += t * lt - t * pa;
      S += t * (lt + 1.f - pa);
    }
  };
  if constexpr (REG > 0) {
#pragma unroll
    for (int j = 0; j < REG; ++j)
      if (threadIdx.x + j * 256 < L) term(av[j], bv[j]);
  } else {
    for (int l = threadIdx.x; l < L; l += 256) term(a[l] / temperature, b[l] / temperature);
  }
  val = block_sum(val, sm);
  S = block_sum(S, sm);
  if (threadIdx.x == 0) {
    stats[r * 5 + 0] = ma;
    stats[r * 5 + 1] = sa;
    stats[r * 5 + 2] = mb;
    stats[r * 5 + 3] = sb;
    stats[r * 5 + 4] = S;
    rowval[r] = val;
  }
}
// dBt[r,l] (=|+=) g/(R*L*T) * t_l * (log t_l + 1 - a_l - S_r)   (0 where t_l underflows to 0)
template <int REG>
__global__ __launch_bounds__(256) void softmax_kl_bwd_kernel(const float* __restrict__ A,
                                                             const float* __restrict__ Bt,
                                                             const float* __restrict__ stats,
                                                             float* __restrict__ dBt, int L, float temperature,
                                                             float scale, const float* gdev, int accumulate) {
  const long r = blockIdx.x;
  const float g = (gdev ? gdev[0] * scale : scale) / temperature;
  const float ma = stats[r * 5 + 0], sa = stats[r * 5 + 1], mb = stats[r * 5 + 2], sb = stats[r * 5 + 3],
              S = stats[r * 5 + 4];
  auto grad = [&](float al, float bl) {
    const float pa = expf(al / temperature - ma) / sa;
    const float t = expf(bl / temperature - mb) / sb;
    return t > 0.f ? g * t * (logf(t) + 1.f - pa - S) : 0.f;
  };
  if constexpr (REG > 0) {
    float av[REG], bv[REG], dv[REG];
#pragma unroll
    for (int j = 0; j < REG; ++j) {          // every load of the row in flight at once (see softmax_kl_rows_kernel)
      const int l = threadIdx.x + j * 256;
      av[j] = l < L ? A[r * L + l] : 0.f;
      bv[j] = l < L ? Bt[r * L + l] : 0.f;
      dv[j] = (accumulate && l < L) ? dBt[r * L + l] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < REG; ++j) {
      const int l = threadIdx.x + j * 256;
      if (l < L) dBt[r * L + l] = dv[j] + grad(av[j], bv[j]);
    }
  } else {
    for (int l = threadIdx.x; l < L; l += 256) {
      const float v = grad(A[r * L + l], Bt[r * L + l]);
      float* d = dBt + r * L + l;
      *d = accumulate ? *d + v : v;
    }
  }
}

// numpy's order of (value, index) candidates (np.argmax / np.amax, which the reference decodes with): a NaN is above every
// number, the larger value otherwise, and among equals -- two NaNs are equals here -- the lower index.  ohkm_select_kernel ranks
// NaN the same way.
__device__ __forceinline__ bool argmax_before(float ov, int oi, float bv, int bi) {
  const bool on = ov != ov, bn = bv != bv;
  if (on != bn) return on;
  return (on || ov == bv) ? oi < bi : ov > bv;
}
// flat argmax per row, first max on ties; a row that holds a NaN gives its first NaN and maxval NaN
__global__ __launch_bounds__(256) void argmax_rows_kernel(const float* __restrict__ hm, long long* __restrict__ idx,
                                                          float* __restrict__ maxval, int L) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const long r = blockIdx.x;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int l = threadIdx.x; l < L; l += 256) {
    const float v = hm[r * L + l];
    if (v > bv || (v != v && bv == bv)) {      // (l ascends: the first maximum, the first NaN)
      bv = v;
      bi = l;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (argmax_before(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sv[wave] = bv;
    si[wave] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k)
      if (argmax_before(sv[k], si[k], bv, bi)) {
        bv = sv[k];
        bi = si[k];
      }
    idx[r] = bi == 0x7fffffff ? 0 : bi;
    if (maxval) maxval[r] = bv;
  }
}

// transform_preds' inverse affine for rot = 0: heatmap (x, y) -> image coordinates.  The ONE copy: the integral decode returns
// a masked joint bit for bit as the standard decode does.
__device__ __forceinline__ void preds_affine(float x, float y, const float* __restrict__ c, float scale0,
                                             float* __restrict__ out, int H, int W) {
  const float s = scale0 * 200.f / (float)W;
  out[0] = c[0] + (x - 0.5f * (float)W) * s;
  out[1] = c[1] + (y - 0.5f * (float)H) * s;
}

// get_final_preds (datasets/process/heatmaps_process.py:47-73): per (b, j) the argmax coordinate (zeroed when the
// maximum is <= 0), the quarter-pixel shift toward the higher neighbour, and transform_preds' inverse affine for
// rot = 0 (affine_transform.py:13-43: uniform scale s = 200*scale[0]/W about (W/2, H/2) -> image centre).
__global__ void final_preds_kernel(const float* __restrict__ hm, const long long* __restrict__ idx,
                                   const float* __restrict__ maxval, const float* __restrict__ center,
                                   const float* __restrict__ scale, float* __restrict__ preds, int B, int J, int H,
                                   int W) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B * J) return;
  const int b = r / J;
  const int i = (int)idx[r];
  float x = (float)(i % W), y = floorf((float)i / (float)W);
  if (!(maxval[r] > 0.f)) x = y = 0.f;
  const int px = (int)floorf(x + 0.5f), py = (int)floorf(y + 0.5f);
  if (1 < px && px < W - 1 && 1 < py && py < H - 1) {
    const float* m = hm + (long)r * H * W;
    const float dx = m[py * W + px + 1] - m[py * W + px - 1];
    const float dy = m[(py + 1) * W + px] - m[(py - 1) * W + px];
    x += (dx > 0.f ? 0.25f : (dx < 0.f ? -0.25f : 0.f));
    y += (dy > 0.f ? 0.25f : (dy < 0.f ? -0.25f : 0.f));
  }
  preds_affine(x, y, center + b * 2, scale[b * 2], preds + r * 2, H, W);
}

// PCK on heatmap argmax (engine/core/utils/evaluate.py:13-75 `calc_dists` / `dist_acc` / `accuracy`): one workgroup.
// pidx/tidx, pmax/tmax: argmax rows of the prediction / target stacks [B*J].  get_max_preds zeroes coordinates whose
// maximum is <= 0; a target joint counts only if both of its coordinates are > 1; x is normalised by H/10 and y by
// W/10 (the reference multiplies (x, y) by [h, w]/10 in that order); distances in fp64 as numpy computes them.
// out[0] = mean of the per-joint accuracies that exist (0 if none), out[1..J] = per-joint accuracy or -1,
// out[J+1] = avg_acc (== out[0] when cnt > 0), out[J+2] = cnt.
__global__ __launch_bounds__(256) void pck_kernel(const long long* __restrict__ pidx, const float* __restrict__ pmax,
                                                  const long long* __restrict__ tidx, const float* __restrict__ tmax,
                                                  float* __restrict__ out, int B, int J, int H, int W, double thr) {
  __shared__ int hit[64], val[64];
  for (int j = threadIdx.x; j < J; j += blockDim.x) {
    const double nx = (double)H / 10.0, ny = (double)W / 10.0;
    int h = 0, v = 0;
    for (int b = 0; b < B; ++b) {
      const int r = b * J + j;
      const long long pi = pidx[r], ti = tidx[r];
      const float pm = pmax[r] > 0.f ? 1.f : 0.f, tm = tmax[r] > 0.f ? 1.f : 0.f;
      const float px = (float)(pi % W) * pm, py = (float)(pi / W) * pm;
      const float tx = (float)(ti % W) * tm, ty = (float)(ti / W) * tm;
      if (tx > 1.f && ty > 1.f) {
        const double dx = (double)px / nx - (double)tx / nx, dy = (double)py / ny - (double)ty / ny;
        ++v;
        if (sqrt(dx * dx + dy * dy) < thr) ++h;
      }
    }
    hit[j] = h;
    val[j] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double avg = 0.0;
    int cnt = 0;
    for (int j = 0; j < J; ++j) {
      const double a = val[j] > 0 ? (double)hit[j] * 1.0 / (double)val[j] : -1.0;
      out[1 + j] = (float)a;
      if (a >= 0.0) {
        avg += a;
        ++cnt;
      }
    }
    avg = cnt != 0 ? avg / cnt : 0.0;
    out[0] = cnt != 0 ? (float)avg : 0.f;
    out[J + 1] = (float)avg;
    out[J + 2] = (float)cnt;
  }
}

// ---- integral (soft-argmax) coordinates: forward, L1 loss, gradient, decode (definition: include/fami.h) ----
// One workgroup per map, the row in registers as in softmax_kl_rows_kernel (REG values per thread, L <= 256 * REG; REG = 0
// streams).  a_l = beta * h_l is rounded on its own (mul_rn), so the forward, the gradient and the decode see the same
// logits; fp32 sums: per thread in l order, then lanes, then waves.
// DECODE = false: coords[r] = {cx, cy}, stats[r] = {m, Z}.
// DECODE = true: the argmax of argmax_rows_kernel in the same walk (m = beta * max h: rounding is monotone, beta > 0),
// out = preds [R,2] image coordinates, out2 = maxvals [R]; a joint final_preds_kernel masks gets its (0, 0).
template <int REG, bool DECODE>
__global__ __launch_bounds__(256) void softargmax_rows_kernel(const float* __restrict__ hm, float* __restrict__ out,
                                                              float* __restrict__ out2,
                                                              const float* __restrict__ center,
                                                              const float* __restrict__ scale, int J, int H, int W,
                                                              float beta) {
  __shared__ float sm[4];
  __shared__ int si[4];
  const long r = blockIdx.x;
  const int L = H * W;
  const float* h = hm + r * L;
  constexpr int NR = REG > 0 ? REG : 1;
  float hv[NR];
  if constexpr (REG > 0) {
#pragma unroll
    for (int j = 0; j < REG; ++j) {        // every load of the row in flight at once
      const int l = threadIdx.x + j * 256;
      hv[j] = l < L ? h[l] : -INFINITY;
    }
  }
  float m, maxval = 0.f;
  if constexpr (DECODE) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    auto take = [&](float v, int l) {      // (l ascends: the first maximum, the first NaN)
      if (v > bv || (v != v && bv == bv)) {
        bv = v;
        bi = l;
      }
    };
    if constexpr (REG > 0) {
#pragma unroll
      for (int j = 0; j < REG; ++j)
        if (threadIdx.x + j * 256 < L) take(hv[j], threadIdx.x + j * 256);
    } else {
      for (int l = threadIdx.x; l < L; l += 256) take(h[l], l);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (argmax_before(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
      sm[wave] = bv;
      si[wave] = bi;
    }
    __syncthreads();
    bv = sm[0];
    bi = si[0];
    for (int k = 1; k < 4; ++k)
      if (argmax_before(sm[k], si[k], bv, bi)) {
        bv = sm[k];
        bi = si[k];
      }
    maxval = bv;
    m = mul_rn(beta, bv);
  } else {
    m = -INFINITY;
    if constexpr (REG > 0) {
#pragma unroll
      for (int j = 0; j < REG; ++j) m = fmaxf(m, mul_rn(beta, hv[j]));
    } else {
      for (int l = threadIdx.x; l < L; l += 256) m = fmaxf(m, mul_rn(beta, h[l]));
    }
    m = block_max(m, sm);
  }
  float z = 0.f, sx = 0.f, sy = 0.f;
  auto add = [&](float hl, int l) {
    const float e = expf(mul_rn(beta, hl) - m);
    const int y = l / W, x = l - y * W;
    z += e;
    sx += e * (float)x;
    sy += e * (float)y;
  };
  if constexpr (REG > 0) {
#pragma unroll
    for (int j = 0; j < REG; ++j)
      if (threadIdx.x + j * 256 < L) add(hv[j], threadIdx.x + j * 256);
  } else {
    for (int l = threadIdx.x; l < L; l += 256) add(h[l], l);
  }
  z = block_sum(z, sm);
  sx = block_sum(sx, sm);
  sy = block_sum(sy, sm);
  if (threadIdx.x == 0) {
    float cx = sx / z, cy = sy / z;
    if constexpr (DECODE) {
      if (!(maxval > 0.f)) cx = cy = 0.f;
      const int b = (int)(r / J);
      preds_affine(cx, cy, center + b * 2, scale[b * 2], out + r * 2, H, W);
      out2[r] = maxval;
    } else {
      out[r * 2 + 0] = cx;
      out[r * 2 + 1] = cy;
      out2[r * 2 + 0] = m;
      out2[r * 2 + 1] = z;
    }
  }
}
// joints [n,2] in input-image pixels -> heatmap pixels, the centre gauss_target_kernel<true> computes, rounded to fp32
__global__ void heatmap_xy_kernel(const float* __restrict__ joints, float* __restrict__ xy, int n, double stride_x,
                                  double stride_y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  xy[i * 2 + 0] = (float)((double)joints[i * 2 + 0] / stride_x);
  xy[i * 2 + 1] = (float)((double)joints[i * 2 + 1] / stride_y);
}
// rowval[r] = w_r (|cx - tx| / W + |cy - ty| / H)
__global__ void integral_l1_rows_kernel(const float* __restrict__ coords, const float* __restrict__ txy,
                                        const float* __restrict__ w, float* __restrict__ rowval, int R, float fw,
                                        float fh) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float wr = w ? w[r] : 1.f;
  rowval[r] = wr * (fabsf(coords[r * 2 + 0] - txy[r * 2 + 0]) / fw + fabsf(coords[r * 2 + 1] - txy[r * 2 + 1]) / fh);
}
__device__ __forceinline__ float sgnf(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }
// dhm[r,l] (=|+=) beta p_l (gx (x_l - cx) + gy (y_l - cy)), p_l = expf(beta h_l - m) / Z from stats.
// gcoords (soft-argmax alone): (gx, gy) = gcoords[r].  Otherwise the L1 term: (gx, gy) = g w_r (sgn(cx - tx) / W, sgn(cy - ty) / H).
template <int REG>
__global__ __launch_bounds__(256) void softargmax_bwd_kernel(const float* __restrict__ hm,
                                                             const float* __restrict__ coords,
                                                             const float* __restrict__ stats,
                                                             const float* __restrict__ gcoords,
                                                             const float* __restrict__ txy, const float* __restrict__ w,
                                                             float* __restrict__ dhm, int H, int W, float beta,
                                                             float scale, const float* gdev, int accumulate) {
  const long r = blockIdx.x;
  const int L = H * W;
  const float cx = coords[r * 2 + 0], cy = coords[r * 2 + 1], m = stats[r * 2 + 0], z = stats[r * 2 + 1];
  float gx, gy;
  if (gcoords) {
    gx = gcoords[r * 2 + 0] * beta;
    gy = gcoords[r * 2 + 1] * beta;
  } else {
    const float g = (gdev ? gdev[0] * scale : scale) * (w ? w[r] : 1.f) * beta;
    gx = g * (sgnf(cx - txy[r * 2 + 0]) / (float)W);
    gy = g * (sgnf(cy - txy[r * 2 + 1]) / (float)H);
  }
  auto grad = [&](float hl, int l) {
    const float p = expf(mul_rn(beta, hl) - m) / z;
    const int y = l / W, x = l - y * W;
    return p * (gx * ((float)x - cx) + gy * ((float)y - cy));
  };
  const float* h = hm + r * L;
  float* d = dhm + r * L;
  if constexpr (REG > 0) {
    float hv[REG], dv[REG];
#pragma unroll
    for (int j = 0; j < REG; ++j) {
      const int l = threadIdx.x + j * 256;
      hv[j] = l < L ? h[l] : 0.f;
      dv[j] = (accumulate && l < L) ? d[l] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < REG; ++j) {
      const int l = threadIdx.x + j * 256;
      if (l < L) {
        const float v = grad(hv[j], l);
        d[l] = accumulate ? dv[j] + v : v;
      }
    }
  } else {
    for (int l = threadIdx.x; l < L; l += 256) {
      const float v = grad(h[l], l);
      d[l] = accumulate ? d[l] + v : v;
    }
  }
}
// the instance by row length, as fami_softmax_kl_*: registers for L <= 4096 and L <= 8192, streaming beyond
template <bool DECODE>
static void launch_softargmax_rows(int R, hipStream_t s, const float* hm, float* out, float* out2, const float* center,
                                   const float* scale, int J, int H, int W, float beta) {
  const long L = (long)H * W;
  if (L <= 256 * 16) hipLaunchKernelGGL((softargmax_rows_kernel<16, DECODE>), dim3(R), dim3(256), 0, s, hm, out, out2, center, scale, J, H, W, beta);
  else if (L <= 256 * 32) hipLaunchKernelGGL((softargmax_rows_kernel<32, DECODE>), dim3(R), dim3(256), 0, s, hm, out, out2, center, scale, J, H, W, beta);
  else hipLaunchKernelGGL((softargmax_rows_kernel<0, DECODE>), dim3(R), dim3(256), 0, s, hm, out, out2, center, scale, J, H, W, beta);
}
static void launch_softargmax_bwd(int R, hipStream_t s, const float* hm, const float* coords, const float* stats,
                                  const float* gcoords, const float* txy, const float* w, float* dhm, int H, int W,
                                  float beta, float scale, const float* gdev, int accumulate) {
  const long L = (long)H * W;
  if (L <= 256 * 16) hipLaunchKernelGGL(softargmax_bwd_kernel<16>, dim3(R), dim3(256), 0, s, hm, coords, stats, gcoords, txy, w, dhm, H, W, beta, scale, gdev, accumulate);
  else if (L <= 256 * 32) hipLaunchKernelGGL(softargmax_bwd_kernel<32>, dim3(R), dim3(256), 0, s, hm, coords, stats, gcoords, txy, w, dhm, H, W, beta, scale, gdev, accumulate);
  else hipLaunchKernelGGL(softargmax_bwd_kernel<0>, dim3(R), dim3(256), 0, s, hm, coords, stats, gcoords, txy, w, dhm, H, W, beta, scale, gdev, accumulate);
}
// beta finite and > 0 (NaN fails both comparisons), positive sizes, a row index that fits an int
static bool softargmax_args_ok(long R, int H, int W, float beta) {
  return R > 0 && R <= 0x7fffffffL && H > 0 && W > 0 && (long)H * W <= 0x7fffffffL && beta > 0.f && beta <= 3.4028234e38f;
}

// ---- structure (limb-direction cosine) term: rows and coordinate gradient (definition: include/fami.h) ----
#define STRUCT_MAX 64      // limbs and joints of a sample: the backward holds both in the LDS of one wavefront
// One limb a -> b of one sample (c, t, w point at the sample's joint 0; w may be null) in fp64 on the fp32 operands, every
// operation rounded on its own.  -> valid; cosv, and with GRAD (dx, dy) = dcos/du; all 0 where not valid.
// An index outside 0..J-1 or a == b (the host refuses such a table before upload) reads nothing and is not valid.
template <bool GRAD>
__device__ __forceinline__ bool limb_cos(const float* __restrict__ c, const float* __restrict__ t,
                                         const float* __restrict__ w, int a, int b, int J, double min_len2, double eps,
                                         double& cosv, double& dx, double& dy) {
#pragma clang fp contract(off)
  cosv = dx = dy = 0.0;
  if ((unsigned)a >= (unsigned)J || (unsigned)b >= (unsigned)J || a == b) return false;
  if (w && !(w[a] > 0.f && w[b] > 0.f)) return false;
  const double tx = (double)t[b * 2 + 0] - (double)t[a * 2 + 0], ty = (double)t[b * 2 + 1] - (double)t[a * 2 + 1];
  const double tt = tx * tx + ty * ty;
  if (!(tt > min_len2)) return false;
  const double ux = (double)c[b * 2 + 0] - (double)c[a * 2 + 0], uy = (double)c[b * 2 + 1] - (double)c[a * 2 + 1];
  const double uu = ux * ux + uy * uy, ut = ux * tx + uy * ty;
  const double nu = sqrt(uu), nt = sqrt(tt);
  const bool clamp = nu <= eps;           // (a NaN length is not clamped: it reaches loss and gradient)
  const double mu = clamp ? eps : nu, mt = nt <= eps ? eps : nt;
  cosv = ut / (mu * mt);
  if constexpr (GRAD) {
    const double nn = mu * mt;
    dx = tx / nn;
    dy = ty / nn;
    if (!clamp) {
      const double n2 = nu * nu;
      dx = dx - (cosv * ux) / n2;
      dy = dy - (cosv * uy) / n2;
    }
  }
  return true;
}
// rowval[s,p] = valid ? 1 - cos : 0, rounded once
__global__ void structure_cos_rows_kernel(const float* __restrict__ coords, const float* __restrict__ txy,
                                          const float* __restrict__ w, const int* __restrict__ pairs,
                                          float* __restrict__ rowval, int n, int J, int P, double min_len2, double eps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = i / P, p = i - s * P;
  const long o = (long)s * J;
  double cosv, dx, dy;
  const bool valid = limb_cos<false>(coords + o * 2, txy + o * 2, w ? w + o : nullptr, pairs[p * 2], pairs[p * 2 + 1], J,
                                     min_len2, eps, cosv, dx, dy);
  rowval[i] = valid ? (float)(1.0 - cosv) : 0.f;
}
// One wavefront per sample.  Lanes over the limbs put dcos/du and the two joints (-1: not valid) into LDS; lanes over the
// joints then walk the limb list in order: gcoords[s,j] = g sum_p -dcos/du_p (+1 at b_p, -1 at a_p) in fp64, rounded once;
// a joint on no valid limb gets 0.  g = scale * (gdev ? gdev[0] : 1), the fp32 product of wmse_bwd_kernel.
__global__ __launch_bounds__(STRUCT_MAX) void structure_cos_bwd_kernel(const float* __restrict__ coords,
                                                                       const float* __restrict__ txy,
                                                                       const float* __restrict__ w,
                                                                       const int* __restrict__ pairs,
                                                                       float* __restrict__ gcoords, int J, int P,
                                                                       double min_len2, double eps, float scale,
                                                                       const float* gdev) {
  __shared__ double sdx[STRUCT_MAX], sdy[STRUCT_MAX];
  __shared__ int sa[STRUCT_MAX], sb[STRUCT_MAX];
  const long o = (long)blockIdx.x * J;
  const int t = threadIdx.x;
  if (t < P) {
    const int a = pairs[t * 2], b = pairs[t * 2 + 1];
    double cosv, dx, dy;
    const bool valid = limb_cos<true>(coords + o * 2, txy + o * 2, w ? w + o : nullptr, a, b, J, min_len2, eps, cosv, dx, dy);
    sdx[t] = dx;
    sdy[t] = dy;
    sa[t] = valid ? a : -1;
    sb[t] = valid ? b : -1;
  }
  __syncthreads();
  if (t < J) {
    const double g = (double)(gdev ? gdev[0] * scale : scale);
    double gx = 0.0, gy = 0.0;
    bool any = false;
    for (int p = 0; p < P; ++p) {
      if (sb[p] == t) {
        gx -= sdx[p];
        gy -= sdy[p];
        any = true;
      } else if (sa[p] == t) {
        gx += sdx[p];
        gy += sdy[p];
        any = true;
      }
    }
    gcoords[(o + t) * 2 + 0] = any ? (float)(g * gx) : 0.f;
    gcoords[(o + t) * 2 + 1] = any ? (float)(g * gy) : 0.f;
  }
}
// sizes within the caps (a row index that fits an int), min_len finite and >= 0, eps finite and > 0 (NaN fails the comparisons)
static bool structure_args_ok(int B, int J, int P, float min_len, float eps) {
  return B > 0 && B <= 0x7fffffff / STRUCT_MAX && J >= 2 && J <= STRUCT_MAX && P >= 1 && P <= STRUCT_MAX && min_len >= 0.f &&
         min_len <= 3.4028234e38f && eps > 0.f && eps <= 3.4028234e38f;
}

#define OHKM_MAX_J 15360      // 60 KiB of the 64 KiB a workgroup may ask for without an opt-in

extern "C" {

// joints [B,J,2] px, vis [B,J] -> target [B,J,Hh,Wh] (NCHW), weight [B,J]
int fami_gauss_target_f32(const float* joints, const float* vis, float* target, float* weight, int B, int J, int Hh,
                          int Wh, int img_h, int img_w, int sigma, hipStream_t s) {
  FAMI_REQUIRE(joints && vis && target && weight && B > 0 && J > 0 && Hh > 0 && Wh > 0 && sigma > 0,
               "fami_gauss_target_f32", "bad argument");
  hipLaunchKernelGGL(gauss_target_kernel<false>, dim3(fami_ew_grid((long)B * J * Hh * Wh)), dim3(256), 0, s, joints, vis,
                     (const float*)nullptr, target, weight, B, J, Hh, Wh, (double)img_w / (double)Wh,
                     (double)img_h / (double)Hh, sigma);
  FAMI_CHECK_LAUNCH("fami_gauss_target_f32");
  return FAMI_OK;
}
// ... with joint_w [J] (device, or null): weight[b,j] *= joint_w[j]; subpixel != 0: the Gaussian centred at the real-valued
// joint position, window and weight those of the rounded centre.  (null, 0) writes what fami_gauss_target_f32 writes.
int fami_gauss_target_ex_f32(const float* joints, const float* vis, const float* joint_w, float* target, float* weight,
                             int B, int J, int Hh, int Wh, int img_h, int img_w, int sigma, int subpixel,
                             hipStream_t s) {
  FAMI_REQUIRE(joints && vis && target && weight && B > 0 && J > 0 && Hh > 0 && Wh > 0 && sigma > 0,
               "fami_gauss_target_ex_f32", "bad argument");
  const dim3 grid(fami_ew_grid((long)B * J * Hh * Wh));
  const double sx = (double)img_w / (double)Wh, sy = (double)img_h / (double)Hh;
  if (subpixel) hipLaunchKernelGGL(gauss_target_kernel<true>, grid, dim3(256), 0, s, joints, vis, joint_w, target, weight, B, J, Hh, Wh, sx, sy, sigma);
  else hipLaunchKernelGGL(gauss_target_kernel<false>, grid, dim3(256), 0, s, joints, vis, joint_w, target, weight, B, J, Hh, Wh, sx, sy, sigma);
  FAMI_CHECK_LAUNCH("fami_gauss_target_ex_f32");
  return FAMI_OK;
}

// loss[0] = scale * sum_{r,l} (w_r (pred-gt))^2 ; pred/gt [R,L], w [R] or null; ws >= R floats
int fami_wmse_fwd_f32(const float* pred, const float* gt, const float* w, float* loss, int R, int L, double scale,
                      float* ws, hipStream_t s) {
  FAMI_REQUIRE(pred && gt && loss && ws && R > 0 && L > 0, "fami_wmse_fwd_f32", "bad argument");
  hipLaunchKernelGGL(wmse_rows_kernel, dim3(R), dim3(256), 0, s, pred, gt, w, ws, L);
  FAMI_CHECK_LAUNCH("fami_wmse_fwd_f32/rows");
  hipLaunchKernelGGL(scalar_sum_kernel, dim3(1), dim3(256), 0, s, ws, R, scale, loss);
  FAMI_CHECK_LAUNCH("fami_wmse_fwd_f32/sum");
  return FAMI_OK;
}
// dpred (=|+=) (gdev? gdev[0] : 1) * scale * 2 w^2 (pred - gt)
int fami_wmse_bwd_f32(const float* pred, const float* gt, const float* w, float* dpred, int R, int L, float scale,
                      const float* gdev, int accumulate, hipStream_t s) {
  FAMI_REQUIRE(pred && gt && dpred && R > 0 && L > 0, "fami_wmse_bwd_f32", "bad argument");
  hipLaunchKernelGGL(wmse_bwd_kernel, dim3(fami_ew_grid((long)R * L)), dim3(256), 0, s, pred, gt, w, dpred, (long)R * L, L, scale, gdev, accumulate);
  FAMI_CHECK_LAUNCH("fami_wmse_bwd_f32");
  return FAMI_OK;
}

// OHKM: per sample only the k joints with the largest row sums count.  pred/gt [B*J,L], w [B*J] or null ->
// sel_w [B*J] = w (1 without w) on the selected joints, 0 elsewhere; loss[0] = scale * sum of the selected row sums.
// ws >= B*J floats.  The gradient is fami_wmse_bwd_f32 with sel_w in place of w (the selection factor is 0 or 1).
int fami_ohkm_fwd_f32(const float* pred, const float* gt, const float* w, float* loss, float* sel_w, int B, int J, int L,
                      int k, double scale, float* ws, hipStream_t s) {
  FAMI_REQUIRE(pred && gt && loss && sel_w && ws && B > 0 && J > 0 && L > 0 && (long)B * J <= 0x7fffffffL,
               "fami_ohkm_fwd_f32", "bad argument");
  FAMI_REQUIRE(k >= 1 && k <= J, "fami_ohkm_fwd_f32", "bad argument (1 <= k <= J)");
  FAMI_REQUIRE(J <= OHKM_MAX_J, "fami_ohkm_fwd_f32", "bad argument (the J row sums of a sample live in LDS: J <= 15360)");
  hipLaunchKernelGGL(wmse_rows_kernel, dim3(B * J), dim3(256), 0, s, pred, gt, w, ws, L);
  FAMI_CHECK_LAUNCH("fami_ohkm_fwd_f32/rows");
  hipLaunchKernelGGL(ohkm_select_kernel, dim3(1), dim3(256), (size_t)J * sizeof(float), s, ws, w, sel_w, loss, B, J, k, scale);
  FAMI_CHECK_LAUNCH("fami_ohkm_fwd_f32/select");
  return FAMI_OK;
}
// value[0] = mean over R*L of t*(log t - a), a = softmax(A/T) rows, t = softmax(Bt/T) rows.
// stats [R,5] saved for the backward; ws >= R floats.
int fami_softmax_kl_fwd_f32(const float* A, const float* Bt, float* value, float* stats, int R, int L,
                            float temperature, float* ws, hipStream_t s) {
  FAMI_REQUIRE(A && Bt && value && stats && ws && R > 0 && L > 0 && temperature > 0.f, "fami_softmax_kl_fwd_f32", "bad argument");
  if (L <= 256 * 16) hipLaunchKernelGGL(softmax_kl_rows_kernel<16>, dim3(R), dim3(256), 0, s, A, Bt, stats, ws, L, temperature);
  else if (L <= 256 * 32) hipLaunchKernelGGL(softmax_kl_rows_kernel<32>, dim3(R), dim3(256), 0, s, A, Bt, stats, ws, L, temperature);
  else hipLaunchKernelGGL(softmax_kl_rows_kernel<0>, dim3(R), dim3(256), 0, s, A, Bt, stats, ws, L, temperature);
  FAMI_CHECK_LAUNCH("fami_softmax_kl_fwd_f32/rows");
  hipLaunchKernelGGL(scalar_sum_kernel, dim3(1), dim3(256), 0, s, ws, R, 1.0 / ((double)R * (double)L), value);
  FAMI_CHECK_LAUNCH("fami_softmax_kl_fwd_f32/sum");
  return FAMI_OK;
}
// dBt (=|+=) gscale * d value / d Bt (gradient flows through the target only, as in the reference)
int fami_softmax_kl_bwd_f32(const float* A, const float* Bt, const float* stats, float* dBt, int R, int L,
                            float temperature, float gscale, const float* gdev, int accumulate, hipStream_t s) {
  FAMI_REQUIRE(A && Bt && stats && dBt && R > 0 && L > 0, "fami_softmax_kl_bwd_f32", "bad argument");
  const float sc = (float)((double)gscale / ((double)R * (double)L));
  if (L <= 256 * 16) hipLaunchKernelGGL(softmax_kl_bwd_kernel<16>, dim3(R), dim3(256), 0, s, A, Bt, stats, dBt, L, temperature, sc, gdev, accumulate);
  else if (L <= 256 * 32) hipLaunchKernelGGL(softmax_kl_bwd_kernel<32>, dim3(R), dim3(256), 0, s, A, Bt, stats, dBt, L, temperature, sc, gdev, accumulate);
  else hipLaunchKernelGGL(softmax_kl_bwd_kernel<0>, dim3(R), dim3(256), 0, s, A, Bt, stats, dBt, L, temperature, sc, gdev, accumulate);
  FAMI_CHECK_LAUNCH("fami_softmax_kl_bwd_f32");
  return FAMI_OK;
}

// idx[r] = first flat argmax of row r, maxval[r] (optional); hm [R,L].  NaN as in numpy: the first NaN of the row, maxval NaN.
int fami_argmax2d_f32(const float* hm, long long* idx, float* maxval, int R, int L, hipStream_t s) {
  FAMI_REQUIRE(hm && idx && R > 0 && L > 0, "fami_argmax2d_f32", "bad argument");
  hipLaunchKernelGGL(argmax_rows_kernel, dim3(R), dim3(256), 0, s, hm, idx, maxval, L);
  FAMI_CHECK_LAUNCH("fami_argmax2d_f32");
  return FAMI_OK;
}

// hm [B,J,H,W] NCHW, center/scale [B,2] -> preds [B,J,2] image coordinates, maxvals [B,J]; idx_ws: B*J int64 scratch
int fami_final_preds_f32(const float* hm, const float* center, const float* scale, float* preds, float* maxvals,
                         long long* idx_ws, int B, int J, int H, int W, hipStream_t s) {
  FAMI_REQUIRE(hm && center && scale && preds && maxvals && idx_ws && B > 0 && J > 0 && H > 2 && W > 2,
               "fami_final_preds_f32", "bad argument");
  hipLaunchKernelGGL(argmax_rows_kernel, dim3(B * J), dim3(256), 0, s, hm, idx_ws, maxvals, H * W);
  FAMI_CHECK_LAUNCH("fami_final_preds_f32/argmax");
  hipLaunchKernelGGL(final_preds_kernel, dim3(fami_cdiv(B * J, 64)), dim3(64), 0, s, hm, idx_ws, maxvals, center, scale,
                     preds, B, J, H, W);
  FAMI_CHECK_LAUNCH("fami_final_preds_f32");
  return FAMI_OK;
}

// ---- integral (soft-argmax) coordinates ----
// hm [R,H,W] -> coords [R,2] = (cx, cy) in heatmap pixels, stats [R,2] = {m, Z}
int fami_softargmax_fwd_f32(const float* hm, float* coords, float* stats, int R, int H, int W, float beta, hipStream_t s) {
  FAMI_REQUIRE(hm && coords && stats && softargmax_args_ok(R, H, W, beta), "fami_softargmax_fwd_f32",
               "bad argument (beta finite and > 0, sizes positive)");
  launch_softargmax_rows<false>(R, s, hm, coords, stats, nullptr, nullptr, 1, H, W, beta);
  FAMI_CHECK_LAUNCH("fami_softargmax_fwd_f32");
  return FAMI_OK;
}
// dhm (=|+=) d/dhm of sum_r (gcoords[r,0] cx_r + gcoords[r,1] cy_r)
int fami_softargmax_bwd_f32(const float* hm, const float* coords, const float* stats, const float* gcoords, float* dhm,
                            int R, int H, int W, float beta, int accumulate, hipStream_t s) {
  FAMI_REQUIRE(hm && coords && stats && gcoords && dhm && softargmax_args_ok(R, H, W, beta), "fami_softargmax_bwd_f32",
               "bad argument (beta finite and > 0, sizes positive)");
  launch_softargmax_bwd(R, s, hm, coords, stats, gcoords, nullptr, nullptr, dhm, H, W, beta, 1.f, nullptr, accumulate);
  FAMI_CHECK_LAUNCH("fami_softargmax_bwd_f32");
  return FAMI_OK;
}
// joints [n,2] (input-image pixels) -> xy [n,2] heatmap pixels: the centre of fami_gauss_target_ex_f32(subpixel = 1)
int fami_heatmap_xy_f32(const float* joints, float* xy, int n, int Hh, int Wh, int img_h, int img_w, hipStream_t s) {
  FAMI_REQUIRE(joints && xy && n > 0 && Hh > 0 && Wh > 0 && img_h > 0 && img_w > 0, "fami_heatmap_xy_f32", "bad argument");
  hipLaunchKernelGGL(heatmap_xy_kernel, dim3(fami_cdiv(n, 256)), dim3(256), 0, s, joints, xy, n,
                     (double)img_w / (double)Wh, (double)img_h / (double)Hh);
  FAMI_CHECK_LAUNCH("fami_heatmap_xy_f32");
  return FAMI_OK;
}
// loss[0] = scale * sum_r w_r (|cx_r - tx_r| / W + |cy_r - ty_r| / H); w [R] or null; ws >= R floats
int fami_integral_l1_fwd_f32(const float* coords, const float* target_xy, const float* w, float* loss, int R, int H,
                             int W, double scale, float* ws, hipStream_t s) {
  FAMI_REQUIRE(coords && target_xy && loss && ws && R > 0 && H > 0 && W > 0, "fami_integral_l1_fwd_f32", "bad argument");
  hipLaunchKernelGGL(integral_l1_rows_kernel, dim3(fami_cdiv(R, 256)), dim3(256), 0, s, coords, target_xy, w, ws, R,
                     (float)W, (float)H);
  FAMI_CHECK_LAUNCH("fami_integral_l1_fwd_f32/rows");
  hipLaunchKernelGGL(scalar_sum_kernel, dim3(1), dim3(256), 0, s, ws, R, scale, loss);
  FAMI_CHECK_LAUNCH("fami_integral_l1_fwd_f32/sum");
  return FAMI_OK;
}
// dhm (=|+=) (gdev ? gdev[0] : 1) * scale * d/dhm of the sum above
int fami_integral_l1_bwd_f32(const float* hm, const float* coords, const float* stats, const float* target_xy,
                             const float* w, float* dhm, int R, int H, int W, float beta, float scale, const float* gdev,
                             int accumulate, hipStream_t s) {
  FAMI_REQUIRE(hm && coords && stats && target_xy && dhm && softargmax_args_ok(R, H, W, beta), "fami_integral_l1_bwd_f32",
               "bad argument (beta finite and > 0, sizes positive)");
  launch_softargmax_bwd(R, s, hm, coords, stats, nullptr, target_xy, w, dhm, H, W, beta, scale, gdev, accumulate);
  FAMI_CHECK_LAUNCH("fami_integral_l1_bwd_f32");
  return FAMI_OK;
}
// ---- structure (limb-direction cosine) term ----
// loss[0] = scale * sum_sp (valid ? 1 - cos(c[b_p] - c[a_p], t[b_p] - t[a_p]) : 0); w [B*J] or null; pairs [P,2] int32 on the
// device; ws >= B*P floats, the row values
int fami_structure_cos_fwd_f32(const float* coords, const float* target_xy, const float* w, const int* pairs, float* loss,
                               int B, int J, int P, float min_len, float eps, double scale, float* ws, hipStream_t s) {
  FAMI_REQUIRE(coords && target_xy && pairs && loss && ws && structure_args_ok(B, J, P, min_len, eps),
               "fami_structure_cos_fwd_f32", "bad argument (1 <= P <= 64, 2 <= J <= 64, min_len finite and >= 0, eps finite and > 0)");
  hipLaunchKernelGGL(structure_cos_rows_kernel, dim3(fami_cdiv((long)B * P, 256)), dim3(256), 0, s, coords, target_xy, w,
                     pairs, ws, B * P, J, P, (double)min_len * (double)min_len, (double)eps);
  FAMI_CHECK_LAUNCH("fami_structure_cos_fwd_f32/rows");
  hipLaunchKernelGGL(scalar_sum_kernel, dim3(1), dim3(256), 0, s, ws, B * P, scale, loss);
  FAMI_CHECK_LAUNCH("fami_structure_cos_fwd_f32/sum");
  return FAMI_OK;
}
// gcoords [B*J,2] = (gdev ? gdev[0] : 1) * scale * d/dcoords of the sum above (every entry written)
int fami_structure_cos_bwd_f32(const float* coords, const float* target_xy, const float* w, const int* pairs,
                               float* gcoords, int B, int J, int P, float min_len, float eps, float scale,
                               const float* gdev, hipStream_t s) {
  FAMI_REQUIRE(coords && target_xy && pairs && gcoords && structure_args_ok(B, J, P, min_len, eps),
               "fami_structure_cos_bwd_f32", "bad argument (1 <= P <= 64, 2 <= J <= 64, min_len finite and >= 0, eps finite and > 0)");
  hipLaunchKernelGGL(structure_cos_bwd_kernel, dim3(B), dim3(STRUCT_MAX), 0, s, coords, target_xy, w, pairs, gcoords, J, P,
                     (double)min_len * (double)min_len, (double)eps, scale, gdev);
  FAMI_CHECK_LAUNCH("fami_structure_cos_bwd_f32");
  return FAMI_OK;
}
// hm [B,J,H,W], center/scale [B,2] -> preds [B,J,2] image coordinates of the soft-argmax, maxvals [B,J]: one launch
int fami_softargmax_preds_f32(const float* hm, const float* center, const float* scale, float beta, float* preds,
                              float* maxvals, int B, int J, int H, int W, hipStream_t s) {
  FAMI_REQUIRE(hm && center && scale && preds && maxvals && B > 0 && J > 0 && softargmax_args_ok((long)B * J, H, W, beta),
               "fami_softargmax_preds_f32", "bad argument (beta finite and > 0, sizes positive)");
  launch_softargmax_rows<true>(B * J, s, hm, preds, maxvals, center, scale, J, H, W, beta);
  FAMI_CHECK_LAUNCH("fami_softargmax_preds_f32");
  return FAMI_OK;
}

// PCK accuracy of a heatmap stack against the target stack, entirely on the device (no host sync):
// out[J+3] as documented at pck_kernel; idx_ws: 2*B*J int64, max_ws: 2*B*J floats (scratch)
int fami_pck_accuracy_f32(const float* pred_hm, const float* target_hm, float* out, long long* idx_ws, float* max_ws,
                          int B, int J, int H, int W, float thr, hipStream_t s) {
  FAMI_REQUIRE(pred_hm && target_hm && out && idx_ws && max_ws && B > 0 && J > 0 && J <= 64 && H > 0 && W > 0,
               "fami_pck_accuracy_f32", "bad argument (J <= 64)");
  const int R = B * J;
  hipLaunchKernelGGL(argmax_rows_kernel, dim3(R), dim3(256), 0, s, pred_hm, idx_ws, max_ws, H * W);
  FAMI_CHECK_LAUNCH("fami_pck_accuracy_f32/argmax");
  hipLaunchKernelGGL(argmax_rows_kernel, dim3(R), dim3(256), 0, s, target_hm, idx_ws + R, max_ws + R, H * W);
  FAMI_CHECK_LAUNCH("fami_pck_accuracy_f32/argmax");
  hipLaunchKernelGGL(pck_kernel, dim3(1), dim3(256), 0, s, idx_ws, max_ws, idx_ws + R, max_ws + R, out, B, J, H, W, (double)thr);
  FAMI_CHECK_LAUNCH("fami_pck_accuracy_f32");
  return FAMI_OK;
}

}  // extern "C"
