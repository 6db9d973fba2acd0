// DARK sub-pixel heatmap decode on the device (dark_get_final_preds, datasets/process/heatmaps_process.py:84-143:
// "Distribution-Aware coordinate Representation of Keypoints", Zhang et al., CVPR 2020).  Per (b, j) map, in fp32:
//   1. get_max_preds on the UNBLURRED map: flat argmax (first maximum on ties), (x, y) zeroed where the maximum is <= 0
//   2. gaussian_blur: a k x k separable Gaussian with zero padding (what cv2.GaussianBlur of the zero-padded map leaves
//      after the crop), the blurred map rescaled by origin_max / max(blurred)
//   3. log(max(., 1e-10))
//   4. taylor: one Newton step from the 5-point gradient and Hessian at the integer peak, where 1 < px < W-2 and
//      1 < py < H-2 and the determinant is not 0
//   5. transform_preds for rot = 0, as final_preds_kernel (loss.hip)
// One launch, one workgroup of 1024 threads per map, everything in LDS:
//   raw [H][W + 2r]   the map with r = (k-1)/2 zero columns on either side   (argmax taken while it is staged)
//   tmp [H + 2r][W]   the row pass, with r zero rows above and below
// so neither pass has a bounds test and nothing outside the map is ever read.  The column pass keeps only its maximum
// (a workgroup reduction); the 13 stencil values at the peak are then recomputed from `tmp` by 13 threads with the same
// instruction sequence, so the blurred map never exists in memory.  Lanes walk both passes along x: consecutive LDS
// addresses, no bank conflicts.  A map whose peak lies outside the guard of step 4 skips the blur altogether.  Where the
// ratio of step 2 is not finite (blurred maximum exactly 0) the reference yields NaN coordinates; here the refinement is
// skipped.
// The grid is small (B*J workgroups, one per CU at most) and each workgroup is a chain of dependent phases -- stage,
// row pass, column pass, reduce, stencil, solve -- so the time is latency, not throughput: hence 16 waves per workgroup
// and several loads / blur outputs in flight per thread (DARK_LOADS, DARK_OUTS; measured in docs/HISTORY.md).
#include <stdio.h>

#include "common.h"

#define DARK_THREADS 1024  // 16 waves: a map owns a whole CU (one workgroup per CU by its LDS), so latency is hidden by waves
#define DARK_WAVES (DARK_THREADS / 64)
#define DARK_LOADS 8  // global loads a thread keeps in flight while the map is staged
#define DARK_OUTS 4   // blur outputs a thread computes per trip
#define DARK_LDS_MAX (160 * 1024 - 256)  // dynamic bytes: the CU's 160 KiB less the static reduction scratch below

// flat index e = tid, tid + DARK_THREADS, ... over [rows][Wd] as (y, x) without a division per element
struct DarkWalk {
  int y, x, dy, dx;
  __device__ __forceinline__ DarkWalk(int Wd) {
    y = (int)threadIdx.x / Wd;
    x = (int)threadIdx.x - y * Wd;
    dy = DARK_THREADS / Wd;
    dx = DARK_THREADS - dy * Wd;
  }
  __device__ __forceinline__ void next(int Wd) {
    y += dy;
    x += dx;
    if (x >= Wd) {
      x -= Wd;
      ++y;
    }
  }
};

// sum_i t[i] * p[i * stride] for symmetric taps (t[i] == t[K-1-i]; only t[0..R] are read): the centre, then the pairs
// from the inside out, each pair added before it is scaled.  The one statement of a blur pass: both uses of the column
// pass must agree bit for bit, hence the explicit fmaf; and since a + b == b + a the blur of a mirrored map is the
// mirrored blur bit for bit, so a symmetric peak gets a gradient of exactly 0.
template <int K>
__device__ __forceinline__ float dark_taps(const float* p, int stride, const float (&t)[(K + 1) / 2]) {
  constexpr int R = (K - 1) / 2;
  float acc = t[R] * p[R * stride];
#pragma unroll
  for (int i = R - 1; i >= 0; --i) acc = fmaf(t[i], p[i * stride] + p[(K - 1 - i) * stride], acc);
  return acc;
}

template <int K>
__global__ __launch_bounds__(DARK_THREADS) void dark_preds_kernel(const float* __restrict__ hm,
                                                                  const float* __restrict__ center,
                                                                  const float* __restrict__ scale,
                                                                  const float* __restrict__ taps,
                                                                  float* __restrict__ preds,
                                                                  float* __restrict__ maxvals, int J, int H, int W) {
  constexpr int R = (K - 1) / 2;
  extern __shared__ __attribute__((aligned(16))) float dark_lds[];
  __shared__ float sv[DARK_WAVES], sb[DARK_WAVES], st[13];
  __shared__ int si[DARK_WAVES];
  const int Wp = W + 2 * R;
  float* __restrict__ raw = dark_lds;           // [H][Wp]
  float* __restrict__ tmp = dark_lds + H * Wp;  // [H + 2R][W]
  const int r = blockIdx.x;
  const float* __restrict__ m = hm + (long)r * H * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  float t[R + 1];
#pragma unroll
  for (int i = 0; i <= R; ++i) t[i] = taps[i];

  // ---- stage the map with its zero columns; argmax with argmax_rows_kernel's tie rule (strictly greater in ascending
  //      index order per thread, lower index on equal values between threads)
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  const int HW = H * W;
  {
    DarkWalk w(W);
    for (int e0 = threadIdx.x; e0 < HW; e0 += DARK_THREADS * DARK_LOADS) {
      float v[DARK_LOADS];
#pragma unroll
      for (int u = 0; u < DARK_LOADS; ++u) v[u] = m[min(e0 + u * DARK_THREADS, HW - 1)];  // all in flight at once
#pragma unroll
      for (int u = 0; u < DARK_LOADS; ++u) {
        const int e = e0 + u * DARK_THREADS;
        if (e < HW) {
          raw[w.y * Wp + R + w.x] = v[u];
          if (v[u] > bv) {
            bv = v[u];
            bi = e;
          }
        }
        w.next(W);
      }
    }
  }
  for (int e = threadIdx.x; e < H * 2 * R; e += DARK_THREADS) {  // the zero columns left and right of every row
    const int y = e / (2 * R), c = e - y * (2 * R);
    raw[y * Wp + (c < R ? c : W + c)] = 0.f;
  }
  for (int e = threadIdx.x; e < R * W; e += DARK_THREADS) {  // the zero rows above and below the row pass
    tmp[e] = 0.f;
    tmp[(H + R) * W + e] = 0.f;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    sv[wave] = bv;
    si[wave] = bi;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < DARK_WAVES; ++k)
    if (sv[k] > bv || (sv[k] == bv && si[k] < bi)) {
      bv = sv[k];
      bi = si[k];
    }
  if (bi == 0x7fffffff) bi = 0;
  const float omax = bv;  // every thread holds the map's maximum and its first index
  const int px = omax > 0.f ? bi % W : 0, py = omax > 0.f ? bi / W : 0;
  const bool inner = 1 < px && px < W - 2 && 1 < py && py < H - 2;  // workgroup-uniform
  float cx = (float)px, cy = (float)py;

  if (inner) {
    // ---- row pass: raw -> tmp.  DARK_OUTS outputs per trip, their LDS reads issued before the first store (the compiler
    //      cannot move a read of `raw` above a store to `tmp`); a trip past the end recomputes the last row and drops it
    {
      DarkWalk w(W);
      for (int e0 = threadIdx.x; e0 < HW; e0 += DARK_THREADS * DARK_OUTS) {
        float acc[DARK_OUTS];
        int o[DARK_OUTS];
#pragma unroll
        for (int u = 0; u < DARK_OUTS; ++u) {
          const int y = min(w.y, H - 1);
          acc[u] = dark_taps<K>(raw + y * Wp + w.x, 1, t);
          o[u] = w.y < H ? (y + R) * W + w.x : -1;
          w.next(W);
        }
#pragma unroll
        for (int u = 0; u < DARK_OUTS; ++u)
          if (o[u] >= 0) tmp[o[u]] = acc[u];
      }
    }
    __syncthreads();
    // ---- column pass: only its maximum is kept
    float bm = -INFINITY;
    {
      DarkWalk w(W);
      for (int e0 = threadIdx.x; e0 < HW; e0 += DARK_THREADS * DARK_OUTS) {
#pragma unroll
        for (int u = 0; u < DARK_OUTS; ++u) {
          const float v = dark_taps<K>(tmp + min(w.y, H - 1) * W + w.x, W, t);
          bm = w.y < H ? fmaxf(bm, v) : bm;
          w.next(W);
        }
      }
    }
    bm = wave_max(bm);
    if (lane == 0) sb[wave] = bm;
    __syncthreads();
    bm = sb[0];
#pragma unroll
    for (int k = 1; k < DARK_WAVES; ++k) bm = fmaxf(bm, sb[k]);
    const float ratio = omax / bm;
    // ---- the 13 stencil values: (0,0) (+-1,0) (0,+-1) (+-2,0) (0,+-2) (+-1,+-1)
    if (threadIdx.x < 13) {
      const int k = threadIdx.x;
      const int ox = k == 1 ? 1 : k == 2 ? -1 : k == 5 ? 2 : k == 6 ? -2 : k >= 9 ? ((k & 1) ? 1 : -1) : 0;
      const int oy = k == 3 ? 1 : k == 4 ? -1 : k == 7 ? 2 : k == 8 ? -2 : k >= 9 ? (k < 11 ? 1 : -1) : 0;
      const float v = dark_taps<K>(tmp + (py + oy) * W + px + ox, W, t);
      st[k] = logf(fmaxf(mul_rn(v, ratio), 1e-10f));
    }
    __syncthreads();
    if (threadIdx.x == 0 && isfinite(ratio)) {
      // st: 0 c | 1 x+1 | 2 x-1 | 3 y+1 | 4 y-1 | 5 x+2 | 6 x-2 | 7 y+2 | 8 y-2 | 9 (+1,+1) | 10 (-1,+1) | 11 (+1,-1) | 12 (-1,-1)
      const float dx = 0.5f * (st[1] - st[2]);
      const float dy = 0.5f * (st[3] - st[4]);
      const float dxx = 0.25f * (st[5] - 2.f * st[0] + st[6]);
      const float dyy = 0.25f * (st[7] - 2.f * st[0] + st[8]);
      const float dxy = 0.25f * (st[9] - st[11] - st[10] + st[12]);
      const float det = dxx * dyy - dxy * dxy;
      if (det != 0.f) {  // coord -= H^-1 g, the 2x2 inverse written out
        cx -= (dyy * dx - dxy * dy) / det;
        cy -= (dxx * dy - dxy * dx) / det;
      }
    }
  }
  if (threadIdx.x == 0) {
    const int b = r / J;
    const float s = scale[b * 2] * 200.f / (float)W;
    preds[r * 2 + 0] = center[b * 2 + 0] + (cx - 0.5f * (float)W) * s;
    preds[r * 2 + 1] = center[b * 2 + 1] + (cy - 0.5f * (float)H) * s;
    maxvals[r] = omax;
  }
}

// dynamic LDS of one workgroup, or -1 where k is not an accepted kernel size or H / W are not positive
static long dark_lds_bytes(int H, int W, int k) {
  if (H <= 0 || W <= 0 || k < 9 || k > 17 || k % 2 == 0) return -1;
  const long r = (k - 1) / 2;
  return 4 * ((long)H * (W + 2 * r) + ((long)H + 2 * r) * W);
}

template <int K>
static void dark_launch(const float* hm, const float* center, const float* scale, const float* taps, float* preds,
                        float* maxvals, int B, int J, int H, int W, size_t lds, hipStream_t s) {
  fami_lds_limit<dark_preds_kernel<K>>(DARK_LDS_MAX);  // a dynamic allocation above 64 KiB needs the function attribute
  hipLaunchKernelGGL(dark_preds_kernel<K>, dim3(B * J), dim3(DARK_THREADS), lds, s, hm, center, scale, taps, preds,
                     maxvals, J, H, W);
}

extern "C" {

long fami_dark_preds_lds_bytes(int H, int W, int k) { return dark_lds_bytes(H, W, k); }
long fami_dark_preds_lds_limit(void) { return DARK_LDS_MAX; }

// hm [B,J,H,W] NCHW, center/scale [B,2], taps: device float[k] (the normalised Gaussian, odd 9 <= k <= 17)
// -> preds [B,J,2] image coordinates, maxvals [B,J]
int fami_dark_preds_f32(const float* hm, const float* center, const float* scale, const float* taps, int k, float* preds,
                        float* maxvals, int B, int J, int H, int W, hipStream_t s) {
  FAMI_REQUIRE(hm && center && scale && taps && preds && maxvals && B > 0 && J > 0 && H > 0 && W > 0,
               "fami_dark_preds_f32", "bad argument");
  FAMI_REQUIRE(k >= 9 && k <= 17 && k % 2 == 1, "fami_dark_preds_f32", "blur kernel size must be odd, 9 <= k <= 17");
  const long lds = dark_lds_bytes(H, W, k);
  if (lds > DARK_LDS_MAX || (long)B * J > 0x7fffffffL / 2) {
    char msg[160];
    snprintf(msg, sizeof(msg), "map too large: 4 * (H * (W + k - 1) + (H + k - 1) * W) = %ld bytes of LDS, limit %d", lds,
             DARK_LDS_MAX);
    fami_set_error("fami_dark_preds_f32", msg);
    return FAMI_ESHAPE;
  }
  switch (k) {
    case 9: dark_launch<9>(hm, center, scale, taps, preds, maxvals, B, J, H, W, (size_t)lds, s); break;
    case 11: dark_launch<11>(hm, center, scale, taps, preds, maxvals, B, J, H, W, (size_t)lds, s); break;
    case 13: dark_launch<13>(hm, center, scale, taps, preds, maxvals, B, J, H, W, (size_t)lds, s); break;
    case 15: dark_launch<15>(hm, center, scale, taps, preds, maxvals, B, J, H, W, (size_t)lds, s); break;
    default: dark_launch<17>(hm, center, scale, taps, preds, maxvals, B, J, H, W, (size_t)lds, s); break;
  }
  FAMI_CHECK_LAUNCH("fami_dark_preds_f32");
  return FAMI_OK;
}

}  // extern "C"
