// Input pipeline on the device: the per-clip affine crop + ToTensor + Normalize that the
// reference runs on DataLoader workers with cv2 / torchvision:
//   cv2.warpAffine(frame, trans, (W, H), flags=cv2.INTER_LINEAR)   datasets/zoo/posetrack/PoseTrack_Alignment.py:421-427
//     (one transform shared by the key frame and every supporting frame of the clip; optional horizontal flip of the
//      source, :409-413; optional BGR->RGB, :299-300)
//   transforms.ToTensor + transforms.Normalize(mean, std)           datasets/transforms/build.py:12-23
// One thread owns one output pixel of all F frames: the source coordinate is computed once in the fixed-point
// arithmetic of OpenCV's generic warpAffine (10 fractional bits rounded to 1/32 pixel, integer bilinear weights summing
// to 2^15), so the 8-bit crop is bit-identical to the CPU restatement in oracle/ops.py::cv2_warp_affine_u8; the float
// conversion follows torch's operation order ((v / 255) - mean) / std with IEEE fp32 division.
// Two kernels share that per-pixel body: one clip per launch (fami_warp_normalize_u8), and a whole batch per launch from
// a descriptor table in device memory (fami_warp_normalize_batch_u8; grid pixels x clips).  A third kernel
// (fami_warp_degrade_batch_u8) runs the batch with a per-frame degradation record -- line blur, colour, occluders, all
// on the 8-bit crop before it becomes a float -- and shares the sampling code below.
#include "common.h"

struct WarpArgs {
  const unsigned char* src;  // [F][Hs][Ws][3]
  float* out;                // [F][3][Hd][Wd]
  double m[6];               // inverse map (dst -> src), row-major 2x3
  long src_stride;           // bytes between source frames
  long out_stride;           // floats between output frames
  int F, Hs, Ws, Hd, Wd, flip, swap_rb;
  float mean[3], stdv[3];
};

// One bilinear sample of OpenCV's fixed-point walk: where it reads (sx, sy; the mirrored columns c0, c1 under flip), which
// of its four taps lie inside the image, and their integer weights (sum 2^15).  X, Y are in 1/32 source pixels.
struct WarpTap {
  int sy, c0, c1, w00, w01, w10, w11;
  bool y0, y1, x0, x1;
};

__device__ __forceinline__ WarpTap warp_tap(int X, int Y, int Hs, int Ws, int flip) {
  WarpTap t;
  const int sx = min(max(X >> 5, -32768), 32767);
  t.sy = min(max(Y >> 5, -32768), 32767);
  const int fx = X & 31, fy = Y & 31;
  t.w00 = (32 - fy) * (32 - fx) * 32, t.w01 = (32 - fy) * fx * 32, t.w10 = fy * (32 - fx) * 32, t.w11 = fy * fx * 32;
  t.y0 = (unsigned)t.sy < (unsigned)Hs, t.y1 = (unsigned)(t.sy + 1) < (unsigned)Hs;
  t.x0 = (unsigned)sx < (unsigned)Ws, t.x1 = (unsigned)(sx + 1) < (unsigned)Ws;
  // flip mirrors the source columns
  t.c0 = flip ? Ws - 1 - sx : sx, t.c1 = flip ? Ws - 2 - sx : sx + 1;
  return t;
}

// source channel cs of the sample: the 8-bit value cv2.warpAffine writes (zero border)
template <class Src>
__device__ __forceinline__ int warp_tap_value(Src s, const WarpTap& t, int Ws, int cs) {
  int acc = 1 << 14;
  if (t.y0 && t.x0) acc += t.w00 * s[((long)t.sy * Ws + t.c0) * 3 + cs];
  if (t.y0 && t.x1) acc += t.w01 * s[((long)t.sy * Ws + t.c1) * 3 + cs];
  if (t.y1 && t.x0) acc += t.w10 * s[((long)(t.sy + 1) * Ws + t.c0) * 3 + cs];
  if (t.y1 && t.x1) acc += t.w11 * s[((long)(t.sy + 1) * Ws + t.c1) * 3 + cs];
  return acc >> 15;
}

// (X0 + adelta, Y0 + bdelta) of output pixel (x, y), in 1/1024 source pixels
__device__ __forceinline__ void warp_origin(const double* m, int x, int y, int& PX, int& PY) {
  // saturate_cast<int>(M[0]*x*AB_SCALE) etc.: separate IEEE double operations (no contraction), round half to even
  const int adelta = __double2int_rn(__dmul_rn(__dmul_rn(m[0], (double)x), 1024.0));
  const int bdelta = __double2int_rn(__dmul_rn(__dmul_rn(m[3], (double)x), 1024.0));
  const int X0 = __double2int_rn(__dmul_rn(__dadd_rn(__dmul_rn(m[1], (double)y), m[2]), 1024.0)) + 16;
  const int Y0 = __double2int_rn(__dmul_rn(__dadd_rn(__dmul_rn(m[4], (double)y), m[5]), 1024.0)) + 16;
  PX = X0 + adelta, PY = Y0 + bdelta;
}

// torch's ToTensor + Normalize on one value: ((v / 255) - mean) / std, each operation rounded
__device__ __forceinline__ float warp_normalize_value(float v, float mean, float stdv) {
  return __fdiv_rn(__fsub_rn(__fdiv_rn(v, 255.0f), mean), stdv);
}

// The per-pixel body the two plain kernels share: output pixel i of the F frames of one clip.  m, Hs, Ws, flip are the
// clip's; src_of(f) / out_of(f) give frame f's source image and its [3][Hd][Wd] output planes.
template <class SrcOf, class OutOf>
__device__ __forceinline__ void warp_normalize_pixel(const double* m, int Hs, int Ws, int flip, int F, int Hd, int Wd,
                                                     int swap_rb, const float* mean, const float* stdv, int i,
                                                     SrcOf src_of, OutOf out_of) {
  const int y = i / Wd, x = i - y * Wd;
  int PX, PY;
  warp_origin(m, x, y, PX, PY);
  const WarpTap t = warp_tap(PX >> 5, PY >> 5, Hs, Ws, flip);
  for (int f = 0; f < F; ++f) {
    const auto s = src_of(f);
    float* o = out_of(f) + (long)y * Wd + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int cs = swap_rb ? 2 - c : c;  // output channel c reads source channel cs
      const float v = (float)warp_tap_value(s, t, Ws, cs);
      o[(long)c * Hd * Wd] = warp_normalize_value(v, mean[c], stdv[c]);
    }
  }
}

__global__ __launch_bounds__(256) void warp_normalize_kernel(WarpArgs p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.Hd * p.Wd) return;
  warp_normalize_pixel(
      p.m, p.Hs, p.Ws, p.flip, p.F, p.Hd, p.Wd, p.swap_rb, p.mean, p.stdv, i,
      [&](int f) { return p.src + f * p.src_stride; }, [&](int f) { return p.out + f * p.out_stride; });
}

// ---- a whole batch in one launch -----------------------------------------------------------------------------------
// Mirrors fami_warp_clip_t (include/fami.h): the table is B of these, then B*F frame pointers.
struct WarpClip {
  double m[6];
  int flip, Hs, Ws, reserved;
};
static_assert(sizeof(WarpClip) == 64 && sizeof(void*) == 8, "fami_warp_clip_t layout");

struct WarpBatchArgs {
  const WarpClip* clips;             // [B]
  const unsigned char* const* srcs;  // [B][F], key frame first
  float* key;                        // [B][3][Hd][Wd]
  float* sup;                        // [B][3 (F-1)][Hd][Wd]
  int F, Hd, Wd, swap_rb;
  float mean[3], stdv[3];
};

// A frame pointer read from the table is a generic pointer to the compiler; the frames are device global memory.
typedef const __attribute__((address_space(1))) unsigned char* GlobalBytes;

// grid (pixel blocks, clips): blockIdx.y selects the clip, so its descriptor and frame pointers are read through a
// workgroup-uniform index (scalar loads of read-only memory), once per workgroup and not per lane.
__global__ __launch_bounds__(256) void warp_normalize_batch_kernel(WarpBatchArgs p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  const WarpClip* __restrict__ cp = p.clips + b;
  const double m[6] = {cp->m[0], cp->m[1], cp->m[2], cp->m[3], cp->m[4], cp->m[5]};
  const int flip = cp->flip, Hs = cp->Hs, Ws = cp->Ws;
  if (i >= p.Hd * p.Wd) return;
  const unsigned char* const* __restrict__ srcs = p.srcs + (long)b * p.F;
  const long plane3 = 3L * p.Hd * p.Wd;
  warp_normalize_pixel(
      m, Hs, Ws, flip, p.F, p.Hd, p.Wd, p.swap_rb, p.mean, p.stdv, i, [&](int f) { return (GlobalBytes)srcs[f]; },
      [&](int f) { return f == 0 ? p.key + b * plane3 : p.sup + ((long)b * (p.F - 1) + (f - 1)) * plane3; });
}

// ---- the batched crop with degradation (occluders, line blur, colour): the stages of include/fami.h -------------------
// Mirrors fami_degrade_frame_t (include/fami.h): one record per (clip, frame).
struct DegradeRect {
  int x0, y0, x1, y1;
  unsigned fill_mode;  // fill[0], fill[1], fill[2], mode: one byte each, lowest first
};
struct DegradeFrame {
  unsigned flags;
  int taps, step_x, step_y;
  float alpha, delta, sat;
  unsigned seed;
  int n_rect, reserved[3];
  DegradeRect rect[4];
};
static_assert(sizeof(DegradeRect) == 20 && sizeof(DegradeFrame) == 128, "fami_degrade_frame_t layout");
enum { DEGRADE_BLUR = 1, DEGRADE_COLOUR = 2, DEGRADE_OCCLUDE = 4 };

__device__ __forceinline__ unsigned lowbias32(unsigned v) {
  v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;
  return v;
}

// Same grid and indexing as warp_normalize_batch_kernel.  Frames outside, taps inside: the record of frame f (flags,
// taps, steps, rectangles) is read through the workgroup-uniform index b*F + f, so every branch on it is taken by whole
// workgroups; a frame without blur reuses the clip's un-shifted sample, computed once per pixel as in the plain kernel.
// Per tap the twelve byte loads (four corners x three adjacent channel bytes) are the plain kernel's.
__global__ __launch_bounds__(256) void warp_degrade_batch_kernel(WarpBatchArgs p, const DegradeFrame* __restrict__ recs) {
#pragma clang fp contract(off)  // stage 2 is separately rounded operations: no fma from this function's own operators
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  const WarpClip* __restrict__ cp = p.clips + b;
  const double m[6] = {cp->m[0], cp->m[1], cp->m[2], cp->m[3], cp->m[4], cp->m[5]};
  const int flip = cp->flip, Hs = cp->Hs, Ws = cp->Ws;
  if (i >= p.Hd * p.Wd) return;
  const unsigned char* const* __restrict__ srcs = p.srcs + (long)b * p.F;
  const long plane = (long)p.Hd * p.Wd;
  const int y = i / p.Wd, x = i - y * p.Wd;
  int PX, PY;
  warp_origin(m, x, y, PX, PY);
  const WarpTap t0 = warp_tap(PX >> 5, PY >> 5, Hs, Ws, flip);
  for (int f = 0; f < p.F; ++f) {
    const DegradeFrame* __restrict__ r = recs + ((long)b * p.F + f);
    const GlobalBytes s = (GlobalBytes)srcs[f];
    float* o = (f == 0 ? p.key + b * 3 * plane : p.sup + ((long)b * (p.F - 1) + (f - 1)) * 3 * plane) + (long)y * p.Wd + x;
    const unsigned flags = r->flags;
    float v[3];
    if (flags & DEGRADE_BLUR) {  // stage 1
      const int taps = min(max(r->taps, 1), 15), h = (taps - 1) >> 1, step_x = r->step_x, step_y = r->step_y;
      int sum[3] = {0, 0, 0};
      for (int k = -h; k <= h; ++k) {
        const WarpTap t = warp_tap((PX + k * step_x) >> 5, (PY + k * step_y) >> 5, Hs, Ws, flip);
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] += warp_tap_value(s, t, Ws, p.swap_rb ? 2 - c : c);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = (float)((2u * (unsigned)sum[c] + (unsigned)taps) / (2u * (unsigned)taps));
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = (float)warp_tap_value(s, t0, Ws, p.swap_rb ? 2 - c : c);
    }
    if (flags & DEGRADE_COLOUR) {  // stage 2: every operation rounded on its own (plain operators under the pragma above:
                                   // the __fmul_rn / __fadd_rn wrappers of the HIP headers are contracted into fma)
      const float alpha = r->alpha, delta = r->delta, sat = r->sat;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float a = v[c] * alpha;
        v[c] = a + delta;
      }
      const float gr = 0.299f * v[0], gg = 0.587f * v[1], gb = 0.114f * v[2];
      const float grg = gr + gg;
      const float g = grg + gb;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float d = v[c] - g;
        const float sd = sat * d;
        v[c] = fminf(fmaxf(g + sd, 0.0f), 255.0f);
      }
    }
    if (flags & DEGRADE_OCCLUDE) {  // stage 3: the later rectangle wins
      const int n_rect = min(max(r->n_rect, 0), 4);
      const unsigned seed = r->seed;
      for (int q = 0; q < n_rect; ++q) {
        const DegradeRect* __restrict__ k = r->rect + q;
        const int x0 = k->x0, y0 = k->y0, x1 = k->x1, y1 = k->y1;
        const unsigned fm = k->fill_mode;  // read outside the per-lane branch: a uniform load
        if (x >= x0 && x < x1 && y >= y0 && y < y1) {
#pragma unroll
          for (int c = 0; c < 3; ++c)
            v[c] = (fm >> 24) ? (float)(lowbias32(((unsigned)(c * p.Hd + y) * (unsigned)p.Wd + (unsigned)x) ^ seed) >> 24)
                              : (float)((fm >> (8 * c)) & 255u);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = warp_normalize_value(v[c], p.mean[c], p.stdv[c]);  // stage 4
  }
}

extern "C" {

int fami_warp_normalize_u8(const unsigned char* src, float* out, int F, int Hs, int Ws, long src_stride, int Hd, int Wd,
                           long out_stride, double m00, double m01, double m02, double m10, double m11, double m12,
                           int flip, int swap_rb, float mean0, float mean1, float mean2, float std0, float std1,
                           float std2, hipStream_t s) {
  FAMI_REQUIRE(src && out && F > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0, "fami_warp_normalize_u8", "bad argument");
  FAMI_REQUIRE(Hs < 32768 && Ws < 32768 && (long)Hd * Wd < (1L << 31), "fami_warp_normalize_u8", "image too large");
  FAMI_REQUIRE(std0 != 0.f && std1 != 0.f && std2 != 0.f, "fami_warp_normalize_u8", "zero std");
  WarpArgs a;
  a.src = src; a.out = out;
  a.m[0] = m00; a.m[1] = m01; a.m[2] = m02; a.m[3] = m10; a.m[4] = m11; a.m[5] = m12;
  a.src_stride = src_stride; a.out_stride = out_stride;
  a.F = F; a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd; a.flip = flip; a.swap_rb = swap_rb;
  a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2;
  a.stdv[0] = std0; a.stdv[1] = std1; a.stdv[2] = std2;
  hipLaunchKernelGGL(warp_normalize_kernel, dim3(fami_cdiv((long)Hd * Wd, 256)), dim3(256), 0, s, a);
  FAMI_CHECK_LAUNCH("fami_warp_normalize_u8");
  return FAMI_OK;
}

long fami_warp_batch_table_bytes(int B, int F) {
  if (B <= 0 || F <= 0) return -1;
  return (long)B * (long)sizeof(WarpClip) + (long)B * F * (long)sizeof(void*);
}

int fami_warp_normalize_batch_u8(const void* table, float* key, float* sup, int B, int F, int Hd, int Wd, int swap_rb,
                                 float mean0, float mean1, float mean2, float std0, float std1, float std2,
                                 hipStream_t s) {
  FAMI_REQUIRE(table && key && B > 0 && F > 0 && Hd > 0 && Wd > 0, "fami_warp_normalize_batch_u8", "bad argument");
  FAMI_REQUIRE(sup || F == 1, "fami_warp_normalize_batch_u8", "null sup with supporting frames");
  FAMI_REQUIRE(B <= 65535 && (long)Hd * Wd < (1L << 31), "fami_warp_normalize_batch_u8", "batch or image too large");
  FAMI_REQUIRE(std0 != 0.f && std1 != 0.f && std2 != 0.f, "fami_warp_normalize_batch_u8", "zero std");
  WarpBatchArgs a;
  a.clips = (const WarpClip*)table;
  a.srcs = (const unsigned char* const*)(a.clips + B);
  a.key = key; a.sup = sup;
  a.F = F; a.Hd = Hd; a.Wd = Wd; a.swap_rb = swap_rb;
  a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2;
  a.stdv[0] = std0; a.stdv[1] = std1; a.stdv[2] = std2;
  hipLaunchKernelGGL(warp_normalize_batch_kernel, dim3(fami_cdiv((long)Hd * Wd, 256), B), dim3(256), 0, s, a);
  FAMI_CHECK_LAUNCH("fami_warp_normalize_batch_u8");
  return FAMI_OK;
}

long fami_degrade_table_bytes(int B, int F) {
  if (B <= 0 || F <= 0) return -1;
  return (long)B * F * (long)sizeof(DegradeFrame);
}

int fami_warp_degrade_batch_u8(const void* table, const void* degrade, float* key, float* sup, int B, int F, int Hd,
                               int Wd, int swap_rb, float mean0, float mean1, float mean2, float std0, float std1,
                               float std2, hipStream_t s) {
  FAMI_REQUIRE(table && degrade && key && B > 0 && F > 0 && Hd > 0 && Wd > 0, "fami_warp_degrade_batch_u8", "bad argument");
  FAMI_REQUIRE(((unsigned long)degrade & 7) == 0, "fami_warp_degrade_batch_u8", "degrade table not 8-byte aligned");
  FAMI_REQUIRE(sup || F == 1, "fami_warp_degrade_batch_u8", "null sup with supporting frames");
  FAMI_REQUIRE(B <= 65535 && (long)Hd * Wd < (1L << 31), "fami_warp_degrade_batch_u8", "batch or image too large");
  FAMI_REQUIRE(std0 != 0.f && std1 != 0.f && std2 != 0.f, "fami_warp_degrade_batch_u8", "zero std");
  WarpBatchArgs a;
  a.clips = (const WarpClip*)table;
  a.srcs = (const unsigned char* const*)(a.clips + B);
  a.key = key; a.sup = sup;
  a.F = F; a.Hd = Hd; a.Wd = Wd; a.swap_rb = swap_rb;
  a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2;
  a.stdv[0] = std0; a.stdv[1] = std1; a.stdv[2] = std2;
  hipLaunchKernelGGL(warp_degrade_batch_kernel, dim3(fami_cdiv((long)Hd * Wd, 256), B), dim3(256), 0, s, a,
                     (const DegradeFrame*)degrade);
  FAMI_CHECK_LAUNCH("fami_warp_degrade_batch_u8");
  return FAMI_OK;
}

}  // extern "C"
