// Track refinement on the device: what follows the association of track.hip -- short gaps of a track filled by linear
// interpolation, a confidence-weighted Gaussian filter along the track, and the mean box score of a track.  The reference
// has no tracker and so no such step: the rule is this project's, stated in include/fami.h.  Pruning short tracks and the
// bookkeeping of the image lists are host work (evaluate.track_refine).
//
// All arithmetic is fp64 on fp32 inputs, every operation rounded on its own (contraction into fused multiply-adds is
// switched off in each kernel body: the float64 restatement in numpy rounds after every operation, and the outputs must
// EQUAL it), in the stated order, rounded to fp32 once.  Nothing transcendental: the Gaussian table comes from the host.
// No atomics, no workspace; every output word has exactly one writer, so two runs agree bit for bit.
//
// Shape.  The three kernels are gathers over host-built tables, one thread per output element:
//   * fill: thread = (new row, value), J * 3 + 6 values per row, two 4-byte reads and one write each;
//   * smooth: thread = (member, joint) over the members sorted by (track, frame).  The window is found by walking the
//     sorted frame numbers at most `radius` members to either side (frame numbers ascend strictly within a track), so a
//     thread makes at most 2 * 16 + 1 neighbour reads of 12 bytes, plain cached gathers: the J threads of a member read
//     one contiguous row of J * 12 bytes per neighbour, and neighbouring members of a track read the same rows again
//     from the cache.  Staging a block's rows through LDS was not needed, see the measurements in docs/HISTORY.md;
//   * score: thread = track, a sequential sum over its segment in frame order.
// Every index read from a table is checked against the array it addresses before use; a thread whose check fails writes
// 1 to the launch's flag word (every writer the same value) and nothing else.
#include <initializer_list>
#include "common.h"

#define REF_THREADS 256
#define REF_RMAX 16   // the largest smoothing radius: 33 neighbour reads per thread

// thread (g, c): value c of new row g.  c < J * 3: keypoint word (x, y interpolated, confidence min * fill_conf);
// c >= J * 3: box column c - J * 3 (0 .. 4 interpolated, 5 min * fill_conf)
__global__ __launch_bounds__(REF_THREADS) void track_fill_kernel(
    const float* __restrict__ kpts, const float* __restrict__ boxes, const int* __restrict__ fill,
    float* __restrict__ kpts_new, float* __restrict__ boxes_new, int* __restrict__ flag, int N, int J, int G,
    double fill_conf) {
#pragma clang fp contract(off)
  const int per = J * 3 + 6;
  const long gid = (long)blockIdx.x * REF_THREADS + threadIdx.x;
  if (gid >= (long)G * per) return;
  const int g = (int)(gid / per), c = (int)(gid - (long)g * per);
  const int* __restrict__ row = fill + (long)g * 5;
  const int a = row[0], b = row[1];
  const long f = row[2], fa = row[3], fb = row[4];
  if ((unsigned)a >= (unsigned)N || (unsigned)b >= (unsigned)N || !(fa < f && f < fb)) {
    *flag = 1;  // an end row outside [0, N), or a frame number that is not inside the gap
    return;
  }
  const bool kp = c < J * 3;
  const int col = kp ? c % 3 : c - J * 3;
  const float va = kp ? kpts[(long)a * J * 3 + c] : boxes[(long)a * 6 + col];
  const float vb = kp ? kpts[(long)b * J * 3 + c] : boxes[(long)b * 6 + col];
  double r;
  if (col == (kp ? 2 : 5)) {
    r = (double)(vb < va ? vb : va) * fill_conf;  // the minimum: a's value unless b's is smaller
  } else {
    const double t = (double)(f - fa) / (double)(fb - fa);
    r = (double)va + ((double)vb - (double)va) * t;
  }
  (kp ? kpts_new + (long)g * J * 3 : boxes_new + (long)g * 6)[kp ? c : col] = (float)r;
}

// thread (i, j): joint j of member i of the sorted member list
__global__ __launch_bounds__(REF_THREADS) void track_smooth_kernel(
    const float* __restrict__ kpts, const int* __restrict__ mrow, const int* __restrict__ mfr,
    const int* __restrict__ mtrk, const int* __restrict__ tseg, const double* __restrict__ gauss,
    float* __restrict__ out, int* __restrict__ flag, int R, int J, int Mm, int T, int radius, float conf_thre) {
#pragma clang fp contract(off)
  const long gid = (long)blockIdx.x * REF_THREADS + threadIdx.x;
  if (gid >= (long)Mm * J) return;
  const int i = (int)(gid / J), j = (int)(gid - (long)i * J);
  const int tr = mtrk[i], row = mrow[i];
  if ((unsigned)tr >= (unsigned)T || (unsigned)row >= (unsigned)R) {
    *flag = 1;
    return;
  }
  const int s = tseg[tr], e = tseg[tr + 1];
  if (s < 0 || e > Mm || i < s || i >= e) {  // not a segment of the member list that holds i
    *flag = 1;
    return;
  }
  const long fi = mfr[i];
  // the window: at most `radius` members to either side, inside the track's segment, within `radius` frame numbers
  int lo = i, hi = i;
  while (lo > s && i - lo < radius && fi - (long)mfr[lo - 1] <= radius && fi - (long)mfr[lo - 1] >= 0) --lo;
  while (hi + 1 < e && hi - i < radius && (long)mfr[hi + 1] - fi <= radius && (long)mfr[hi + 1] - fi >= 0) ++hi;
  for (int k = lo; k <= hi; ++k)
    if ((unsigned)mrow[k] >= (unsigned)R) {
      *flag = 1;  // checked for the whole window before anything is read through it
      return;
    }
  const float* __restrict__ own = kpts + ((long)row * J + j) * 3;
  const float x = own[0], y = own[1], c = own[2];
  float ox = x, oy = y;
  if (c > conf_thre) {
    double sw = 0.0, sx = 0.0, sy = 0.0;
    int others = 0;
    for (int k = lo; k <= hi; ++k) {
      const float* __restrict__ p = kpts + ((long)mrow[k] * J + j) * 3;
      const float ck = p[2];
      if (ck > conf_thre) {
        const long d = (long)mfr[k] - fi;
        const double w = gauss[d < 0 ? -d : d] * (double)ck;
        sw += w;
        sx += w * (double)p[0];
        sy += w * (double)p[1];
        others += k != i;
      }
    }
    if (others) {
      ox = (float)(sx / sw);
      oy = (float)(sy / sw);
    }
  }
  float* __restrict__ o = out + ((long)row * J + j) * 3;
  o[0] = ox;
  o[1] = oy;
  o[2] = c;
}

// thread t: the mean box score (column 5) of the members of track t, summed in the order of the member list
__global__ __launch_bounds__(REF_THREADS) void track_score_kernel(
    const float* __restrict__ boxes, const int* __restrict__ mrow, const int* __restrict__ tseg,
    float* __restrict__ score, int* __restrict__ flag, int R, int Mm, int T) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * REF_THREADS + threadIdx.x;
  if (t >= T) return;
  const int s = tseg[t], e = tseg[t + 1];
  if (s < 0 || e <= s || e > Mm) {  // no non-empty segment of the member list
    *flag = 1;
    return;
  }
  double sum = 0.0;
  for (int k = s; k < e; ++k) {
    const int row = mrow[k];
    if ((unsigned)row >= (unsigned)R) {
      *flag = 1;
      return;
    }
    sum += (double)boxes[(long)row * 6 + 5];
  }
  score[t] = (float)(sum / (double)(e - s));
}

static inline bool ref_aligned4(std::initializer_list<const void*> ps) {
  uintptr_t all = 0;
  for (const void* p : ps) all |= (uintptr_t)p;
  return (all & 3) == 0;
}

extern "C" {

// see include/fami.h
int fami_track_fill_f32(const float* kpts, const float* boxes, const int* fill, int N, int J, int G, double fill_conf,
                        float* kpts_new, float* boxes_new, int* flag, hipStream_t s) {
  FAMI_REQUIRE(kpts && boxes && fill && kpts_new && boxes_new && flag, "fami_track_fill_f32", "null argument");
  FAMI_REQUIRE(ref_aligned4({kpts, boxes, fill, kpts_new, boxes_new, flag}), "fami_track_fill_f32",
               "every pointer must be 4-byte aligned");
  FAMI_REQUIRE(J >= 1 && J <= 32, "fami_track_fill_f32", "J must be in 1 .. 32");
  FAMI_REQUIRE(N >= 1 && G >= 1 && ((long)N + G) * J * 3 <= 0x7fffffffL, "fami_track_fill_f32",
               "N and G must be >= 1 and (N + G) * J * 3 <= 2^31 - 1");
  FAMI_REQUIRE(fill_conf >= 0.0 && fill_conf <= 1.0, "fami_track_fill_f32", "fill_conf must be in [0, 1]");
  const long total = (long)G * (J * 3 + 6);
  hipLaunchKernelGGL(track_fill_kernel, dim3(fami_cdiv(total, REF_THREADS)), dim3(REF_THREADS), 0, s, kpts, boxes, fill,
                     kpts_new, boxes_new, flag, N, J, G, fill_conf);
  FAMI_CHECK_LAUNCH("fami_track_fill_f32");
  return FAMI_OK;
}

int fami_track_smooth_f32(const float* kpts, const int* mrow, const int* mfr, const int* mtrk, const int* tseg,
                          const double* gauss, int R, int J, int Mm, int T, int radius, float conf_thre, float* out,
                          int* flag, hipStream_t s) {
  FAMI_REQUIRE(kpts && mrow && mfr && mtrk && tseg && gauss && out && flag, "fami_track_smooth_f32", "null argument");
  FAMI_REQUIRE(ref_aligned4({kpts, mrow, mfr, mtrk, tseg, out, flag}) && ((uintptr_t)gauss & 7) == 0,
               "fami_track_smooth_f32", "every pointer must be 4-byte aligned, gauss 8-byte");
  FAMI_REQUIRE(J >= 1 && J <= 32, "fami_track_smooth_f32", "J must be in 1 .. 32");
  FAMI_REQUIRE(R >= 1 && (long)R * J * 3 <= 0x7fffffffL, "fami_track_smooth_f32", "R must be in 1 .. (2^31 - 1) / (3 J)");
  FAMI_REQUIRE(Mm >= 1 && Mm <= R && T >= 1 && T <= Mm, "fami_track_smooth_f32", "1 <= T <= Mm <= R");
  FAMI_REQUIRE(radius >= 1 && radius <= REF_RMAX, "fami_track_smooth_f32", "radius must be in 1 .. 16");
  FAMI_REQUIRE(conf_thre == conf_thre, "fami_track_smooth_f32", "conf_thre is NaN");
  FAMI_REQUIRE(out != kpts, "fami_track_smooth_f32", "out must not be kpts: neighbours read unsmoothed values");
  hipLaunchKernelGGL(track_smooth_kernel, dim3(fami_cdiv((long)Mm * J, REF_THREADS)), dim3(REF_THREADS), 0, s, kpts, mrow,
                     mfr, mtrk, tseg, gauss, out, flag, R, J, Mm, T, radius, conf_thre);
  FAMI_CHECK_LAUNCH("fami_track_smooth_f32");
  return FAMI_OK;
}

int fami_track_score_f32(const float* boxes, const int* mrow, const int* tseg, int R, int Mm, int T, float* score,
                         int* flag, hipStream_t s) {
  FAMI_REQUIRE(boxes && mrow && tseg && score && flag, "fami_track_score_f32", "null argument");
  FAMI_REQUIRE(ref_aligned4({boxes, mrow, tseg, score, flag}), "fami_track_score_f32",
               "every pointer must be 4-byte aligned");
  FAMI_REQUIRE(R >= 1 && R <= 0x7fffffff / 6 && Mm >= 1 && Mm <= R && T >= 1 && T <= Mm, "fami_track_score_f32",
               "1 <= T <= Mm <= R <= (2^31 - 1) / 6");
  hipLaunchKernelGGL(track_score_kernel, dim3(fami_cdiv(T, REF_THREADS)), dim3(REF_THREADS), 0, s, boxes, mrow, tseg,
                     score, flag, R, Mm, T);
  FAMI_CHECK_LAUNCH("fami_track_score_f32");
  return FAMI_OK;
}

}  // extern "C"
