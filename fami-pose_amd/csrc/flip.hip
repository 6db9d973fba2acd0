// Flip testing on the device (HRNet / DCPose evaluation protocol; the reference declares VAL.FLIP_VAL, TEST.FLIP_TEST and
// the two SHIFT_HEATMAP switches at posetimation/config/mppe_config.py:322-346 and ships flip_back,
// datasets/process/pose_process.py:29-42):
//   mirror_cat_kernel   x [rows][W] -> out [2 rows][W] = [x ; x mirrored along W]: the doubled batch of ONE forward
//   flip_merge_kernel   hm2 [2B][J][H][W] -> out [B][J][H][W] = (plain + flip_back(mirrored)) * 0.5, optionally with
//                       HRNet's one-column shift of the mirrored half
// Both are launch-sized copies (the merge moves 1.4 MB at W48, B = 4): one thread owns one 16-byte chunk, a chip-sized
// grid strides the rest, no LDS, no atomics.  A reversed chunk is the mirrored chunk with its four lanes swapped in
// registers.  The scalar forms take any W and any 4-byte aligned pointers.
// Index arithmetic: the grid has at most 2048 x 256 threads, so a thread's first element and the grid stride fit 32 bits
// and are split into (row, column) with one 32-bit division; later elements advance the pair by the split stride.
#include "common.h"

__device__ __forceinline__ u32x4 rev4(u32x4 v) { return u32x4{v.w, v.z, v.y, v.x}; }

// (row, column) of a grid-stride walk over [rows][W]
struct RowCol {
  long i, row;
  unsigned col, stride, drow, dcol;
  __device__ __forceinline__ RowCol(unsigned W) {
    const unsigned i0 = blockIdx.x * 256u + threadIdx.x;
    stride = gridDim.x * 256u;
    i = i0;
    row = i0 / W;
    col = i0 - (unsigned)row * W;
    drow = stride / W;
    dcol = stride - drow * W;
  }
  __device__ __forceinline__ void next(unsigned W) {
    i += stride;
    row += drow;
    col += dcol;
    if (col >= W) {
      col -= W;
      ++row;
    }
  }
};

// the values travel as 32-bit integers: no float instruction sees them, every bit pattern survives
__global__ __launch_bounds__(256) void mirror_cat_v4_kernel(const unsigned* __restrict__ x, unsigned* __restrict__ out,
                                                            long rows, int W4) {
  const long n4 = rows * W4;
  unsigned* __restrict__ mir = out + n4 * 4;
  for (RowCol t(W4); t.i < n4; t.next(W4)) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(x + t.i * 4);
    *reinterpret_cast<u32x4*>(out + t.i * 4) = v;
    *reinterpret_cast<u32x4*>(mir + (t.row * W4 + (W4 - 1 - t.col)) * 4) = rev4(v);
  }
}

__global__ __launch_bounds__(256) void mirror_cat_kernel(const unsigned* __restrict__ x, unsigned* __restrict__ out,
                                                         long rows, int W) {
  const long n = rows * W;
  unsigned* __restrict__ mir = out + n;
  for (RowCol t(W); t.i < n; t.next(W)) {
    const unsigned v = x[t.i];
    out[t.i] = v;
    mir[t.row * W + (W - 1 - t.col)] = v;
  }
}

// row of the mirrored half that output row (b, j, y) averages with: batch B + b, channel perm[j], same y
// (the host admits at most 2^31 - 1 rows in hm2)
__device__ __forceinline__ long flip_src_row(unsigned row, const int* __restrict__ perm, int B, int J, int H) {
  const unsigned bj = row / (unsigned)H, y = row - bj * H;
  const unsigned b = bj / (unsigned)J, j = bj - b * J;
  return ((long)(B + b) * J + perm[j]) * H + y;
}

// W = 4 W4, 16-byte aligned bases.  Output columns 4c..4c+3 read the mirrored row at W-1-4c .. W-4-4c: chunk W4-1-c
// reversed.  With the shift they read W-4c, W-1-4c, W-2-4c, W-3-4c (the first clamped to W-1 at c = 0): lanes 3, 2, 1 of
// the same chunk behind one scalar element.
template <bool SHIFT>
__global__ __launch_bounds__(256) void flip_merge_v4_kernel(const float* __restrict__ hm2, const int* __restrict__ perm,
                                                            float* __restrict__ out, int B, int J, int H, int W4) {
  const long n4 = (long)B * J * H * W4;
  const int W = W4 * 4;
  for (RowCol t(W4); t.i < n4; t.next(W4)) {
    const long i = t.i;
    const int c = (int)t.col;
    const float* __restrict__ src = hm2 + flip_src_row((unsigned)t.row, perm, B, J, H) * W;
    const f32x4 a = ld4(hm2 + i * 4);
    const f32x4 m = ld4(src + (W4 - 1 - c) * 4);
    f32x4 f;
    if (SHIFT)
      f = f32x4{src[c == 0 ? W - 1 : W - 4 * c], m.w, m.z, m.y};
    else
      f = f32x4{m.w, m.z, m.y, m.x};
    st4(out + i * 4, (a + f) * 0.5f);
  }
}

template <bool SHIFT>
__global__ __launch_bounds__(256) void flip_merge_kernel(const float* __restrict__ hm2, const int* __restrict__ perm,
                                                         float* __restrict__ out, int B, int J, int H, int W) {
  const long n = (long)B * J * H * W;
  for (RowCol t(W); t.i < n; t.next(W)) {
    const int x = (int)t.col;
    const int xs = SHIFT ? min(W - x, W - 1) : W - 1 - x;
    out[t.i] = (hm2[t.i] + hm2[flip_src_row((unsigned)t.row, perm, B, J, H) * W + xs]) * 0.5f;
  }
}

// two 4-byte aligned ranges of na / nb floats that do not overlap
static bool flip_disjoint(const void* a, long na, const void* b, long nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  if (((x | y) & 3) != 0) return false;
  return x + (uintptr_t)na * 4 <= y || y + (uintptr_t)nb * 4 <= x;
}
static bool flip_vec(const void* a, const void* b, int W) {
  return W % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

extern "C" {

// out[r, :] = x[r, :], out[rows + r, w] = x[r, W-1-w]: x [B,C,H,W] with rows = B*C*H -> [x ; mirror_W(x)]
int fami_mirror_cat_f32(const float* x, float* out, long long rows, int W, hipStream_t s) {
  FAMI_REQUIRE(x && out && rows > 0 && W > 0, "fami_mirror_cat_f32", "bad argument");
  FAMI_REQUIRE(rows <= (1LL << 60) / W, "fami_mirror_cat_f32", "too many elements");
  const long n = (long)rows * W;
  FAMI_REQUIRE(flip_disjoint(x, n, out, 2 * n), "fami_mirror_cat_f32", "x and out overlap or are not 4-byte aligned");
  const unsigned* xi = reinterpret_cast<const unsigned*>(x);
  unsigned* oi = reinterpret_cast<unsigned*>(out);
  if (flip_vec(x, out, W))
    hipLaunchKernelGGL(mirror_cat_v4_kernel, dim3(fami_ew_grid(n / 4)), dim3(256), 0, s, xi, oi, (long)rows, W / 4);
  else
    hipLaunchKernelGGL(mirror_cat_kernel, dim3(fami_ew_grid(n)), dim3(256), 0, s, xi, oi, (long)rows, W);
  FAMI_CHECK_LAUNCH("fami_mirror_cat_f32");
  return FAMI_OK;
}

// out[b,j,y,x] = (hm2[b,j,y,x] + hm2[B+b,perm[j],y,xs]) * 0.5f, xs = shift ? min(W-x, W-1) : W-1-x.
// perm: device int[J], every entry in [0, J) (the caller's contract: it is not read on the host).
int fami_flip_merge_f32(const float* hm2, const int* perm, float* out, int B, int J, int H, int W, int shift,
                        hipStream_t s) {
  FAMI_REQUIRE(hm2 && perm && out && B > 0 && J > 0 && H > 0 && W > 0, "fami_flip_merge_f32", "bad argument");
  if (2L * B * J * H > 0x7fffffffL) {
    fami_set_error("fami_flip_merge_f32", "more than 2^31 - 1 heatmap rows");
    return FAMI_ESHAPE;
  }
  const long n = (long)B * J * H * W;
  FAMI_REQUIRE(flip_disjoint(hm2, 2 * n, out, n), "fami_flip_merge_f32", "hm2 and out overlap or are not 4-byte aligned");
  FAMI_REQUIRE((reinterpret_cast<uintptr_t>(perm) & 3) == 0, "fami_flip_merge_f32", "perm is not 4-byte aligned");
  if (flip_vec(hm2, out, W)) {
    const dim3 grid(fami_ew_grid(n / 4));
    if (shift)
      hipLaunchKernelGGL(flip_merge_v4_kernel<true>, grid, dim3(256), 0, s, hm2, perm, out, B, J, H, W / 4);
    else
      hipLaunchKernelGGL(flip_merge_v4_kernel<false>, grid, dim3(256), 0, s, hm2, perm, out, B, J, H, W / 4);
  } else {
    const dim3 grid(fami_ew_grid(n));
    if (shift)
      hipLaunchKernelGGL(flip_merge_kernel<true>, grid, dim3(256), 0, s, hm2, perm, out, B, J, H, W);
    else
      hipLaunchKernelGGL(flip_merge_kernel<false>, grid, dim3(256), 0, s, hm2, perm, out, B, J, H, W);
  }
  FAMI_CHECK_LAUNCH("fami_flip_merge_f32");
  return FAMI_OK;
}

}  // extern "C"
