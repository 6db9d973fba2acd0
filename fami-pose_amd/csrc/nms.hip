// Pose rescoring and OKS-NMS on the device: the third step of the HRNet-family evaluation protocol, after flip testing
// (flip.hip) and the DARK decode (decode.hip).  Restated from datasets/process/nms.py:51-192 (oks_iou, oks_nms,
// _rescore, soft_oks_nms) and the HRNet rescoring rule whose switches the reference declares (VAL/TEST.IN_VIS_THRE,
// OKS_THRE, SOFT_NMS, posetimation/config/mppe_config.py:325-330).  Per image, in fp64 on the fp32 inputs:
//   1. score = box_score * mean(conf_j over joints with conf_j > in_vis_thre), mean 0 when no joint passes, rounded to
//      fp32 once.  Everything below orders by that fp32 value.
//   2. repeat: pick the remaining detection with the largest working score (ties: lower position in the image's list),
//      keep it, then for every remaining detection d
//        OKS(p, d) = mean_j exp(-(dx^2 + dy^2) / (2 sigma_j)^2 / ((a_p + a_d) / 2 + 2^-52) / 2)
//      over the joints with conf_j(d) > vis_thre -- the visibility of the COMPARED detection only, as the reference's
//      `list(vg > t) and list(vd > t)` evaluates to its second operand; all joints without a vis_thre, 0 on an empty mask
//        hard: d is dropped where OKS > oks_thre       (oks_nms: picking the maximum of what is left IS its walk along
//                                                       the sorted order, so no sort is needed)
//        soft: working(d) *= exp(-OKS^2 / oks_thre)    (soft_oks_nms with the Gaussian _rescore), at most max_dets picks
// One workgroup of 256 threads per image, thread t owning the t-th detection of the image's list (at most 256), no
// atomics and no workspace: every output word has exactly one writer, so two runs agree bit for bit.
//
// Shape.  The pick loop is a chain of `kept` dependent rounds, each ending in the one barrier behind which the picked
// index becomes known, so the time of an image is rounds x (argmax + one OKS), and what matters is the latency of a
// round, not throughput:
//   * keypoints are LDS-resident ([J][256] (x, y) pairs, staged once).  A round reads the picked pose (one address for
//     the whole wave: a broadcast) and each lane's own pose (consecutive 8-byte words: conflict-free) at LDS latency;
//     re-reading them from global memory would put an L2 round trip -- several times the LDS latency, and behind a
//     gather through `index` -- on every link of the chain, to save an LDS footprint (1376 + 2048 J bytes: 36 KiB at
//     J = 17, four images per CU) that costs nothing at this grid shape.  The own pose stays in LDS rather than in 64
//     registers so that J is a run-time loop.
//   * the argmax is a 64-lane butterfly per wave and four LDS slots per workgroup, double-buffered by the parity of
//     the round, which leaves ONE barrier per round: the slots of round r are rewritten in round r + 2, and a thread
//     can only get there through the barrier of round r + 1, which every reader of round r has then reached.
//   * a wave none of whose detections remain skips the OKS of the round; it still meets the barrier.
//   * the OKS of a round is J chains of two fp64 divisions and an exp, each several hundred cycles of dependent
//     instructions; the joint loop runs four joints per trip without a branch (masked joints are computed and left out
//     of the sum), so that four chains overlap (oks.h, shared with track.hip).
// All LDS is dynamic and 16-byte aligned (nothing static in front of it); at J = 32 it exceeds 64 KiB, hence the function
// attribute.  The visibility mask and the working score live in registers.
#include "common.h"
#include "oks.h"

#define NMS_THREADS 256
#define NMS_WAVES (NMS_THREADS / 64)
#define NMS_CAP NMS_THREADS  // detections per image: one thread each
#define NMS_JMAX OKS_JMAX    // joints: one bit each in the visibility mask
#define NMS_NONE 0x7fffffff  // "no detection" in the argmax

// dynamic LDS: vars[32] f64 | argmax slots [2][4] f64 + [2][4] i32 | area[256] f32 | xy[J][256] float2
#define NMS_LDS_FIXED (NMS_JMAX * 8 + 2 * NMS_WAVES * 8 + 2 * NMS_WAVES * 4 + NMS_CAP * 4)
static_assert(NMS_WAVES == 4 && NMS_CAP == OKS_CAP && NMS_LDS_FIXED % 16 == 0, "the (x, y) array must start 16-byte aligned");
static inline size_t nms_lds_bytes(int J) { return NMS_LDS_FIXED + (size_t)J * NMS_CAP * 8; }

// step 1 for one detection: k = its [J][3] keypoints, bs = its box score
__device__ __forceinline__ float nms_rescore(const float* __restrict__ k, int J, double bs, double in_vis_thre) {
  double sum = 0.0;
  int cnt = 0;
  for (int j = 0; j < J; ++j) {
    const double c = (double)k[j * 3 + 2];
    if (c > in_vis_thre) {
      sum += c;
      ++cnt;
    }
  }
  const double mean = cnt ? sum / (double)cnt : 0.0;
  return (float)(bs * mean);
}

// (w, t) better than (bw, bt)?  A total order on what the kernel can hold (finite scores); NMS_NONE never wins.
__device__ __forceinline__ bool nms_better(double w, int t, double bw, int bt) {
  return t != NMS_NONE && (bt == NMS_NONE || w > bw || (w == bw && t < bt));
}

__global__ __launch_bounds__(NMS_THREADS) void pose_nms_kernel(
    const float* __restrict__ kpts, const float* __restrict__ area, const float* __restrict__ box_score,
    const float* __restrict__ sigmas, const int* __restrict__ index, const int* __restrict__ seg,
    float* __restrict__ score, int* __restrict__ rank, int* __restrict__ kept, int N, int J, double in_vis_thre,
    double oks_thre, int soft, int max_dets, double vis_thre, int use_vis) {
#pragma clang fp contract(off)  // the reference's operation order, one rounding per operation
  extern __shared__ __attribute__((aligned(16))) unsigned char nms_lds[];
  double* __restrict__ vars = reinterpret_cast<double*>(nms_lds);          // [NMS_JMAX]  (2 sigma_j)^2
  double* __restrict__ redw = vars + NMS_JMAX;                               // [2][NMS_WAVES]
  int* __restrict__ redt = reinterpret_cast<int*>(redw + 2 * NMS_WAVES);    // [2][NMS_WAVES]
  float* __restrict__ s_area = reinterpret_cast<float*>(redt + 2 * NMS_WAVES);  // [NMS_CAP]
  float2* __restrict__ xy = reinterpret_cast<float2*>(s_area + NMS_CAP);    // [J][NMS_CAP]
  const int m = blockIdx.x, t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int s = seg[m], e = seg[m + 1];
  // everything up to the first barrier is workgroup-uniform
  if (s < 0 || e < s || e > N) {  // not a segment of index[0 .. N): nothing of it can be addressed
    if (t == 0) kept[m] = -1;
    return;
  }
  const int n = e - s;
  if (n > NMS_CAP) {  // over the cap: rescored, and the whole image marked
    for (int i = t; i < n; i += NMS_THREADS) {
      const int g = index[s + i];
      if ((unsigned)g < (unsigned)N) {
        score[g] = nms_rescore(kpts + (long)g * J * 3, J, (double)box_score[g], in_vis_thre);
        rank[g] = -1;
      }
    }
    if (t == 0) kept[m] = -1;
    return;
  }

  int g = -1;
  if (t < n) {
    g = index[s + t];
    if ((unsigned)g >= (unsigned)N) g = -1;
  }
  const int bad = t < n && g < 0;
  if (t < J) vars[t] = oks_var(sigmas[t]);
  double w = 0.0;      // the working score
  unsigned mask = 0u;  // joints of THIS detection that count when it is compared against a picked one
  if (g >= 0) {
    const float* __restrict__ k = kpts + (long)g * J * 3;
    for (int j = 0; j < J; ++j) {
      xy[j * NMS_CAP + t] = make_float2(k[j * 3], k[j * 3 + 1]);
      if (!use_vis || (double)k[j * 3 + 2] > vis_thre) mask |= 1u << j;
    }
    const float sc = nms_rescore(k, J, (double)box_score[g], in_vis_thre);
    score[g] = sc;
    rank[g] = -1;
    s_area[t] = area[g];
    w = (double)sc;
  }
  // "any bad index" through the second set of argmax slots (first rewritten in round 1, behind the barrier of round 0);
  // this barrier also publishes vars, s_area and xy
  const bool wave_bad = __ballot(bad) != 0ull;
  if (lane == 0) redt[NMS_WAVES + wave] = wave_bad;
  __syncthreads();
  if (redt[NMS_WAVES] | redt[NMS_WAVES + 1] | redt[NMS_WAVES + 2] | redt[NMS_WAVES + 3]) {
    if (t == 0) kept[m] = -1;  // an index outside [0, N): the image is marked, the addressable ranks stay -1
    return;
  }
  bool remaining = g >= 0;
  const int nmask = __popc(mask);
  const int limit = soft ? min(n, max_dets) : n;
  int count = 0;
  for (int it = 0; it < limit; ++it) {
    double bw = w;
    int bt = remaining ? t : NMS_NONE;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ow = __shfl_xor(bw, o, 64);
      const int ot = __shfl_xor(bt, o, 64);
      if (nms_better(ow, ot, bw, bt)) {
        bw = ow;
        bt = ot;
      }
    }
    const int buf = (it & 1) * NMS_WAVES;
    if (lane == 0) {
      redw[buf + wave] = bw;
      redt[buf + wave] = bt;
    }
    __syncthreads();
    bw = redw[buf];
    bt = redt[buf];
#pragma unroll
    for (int k = 1; k < NMS_WAVES; ++k)
      if (nms_better(redw[buf + k], redt[buf + k], bw, bt)) {
        bw = redw[buf + k];
        bt = redt[buf + k];
      }
    const int p = bt;  // the same in every thread: all read the same four slots in the same order
    if (p == NMS_NONE) break;
    if (t == p) {
      rank[g] = count;
      remaining = false;
    }
    ++count;
    if (remaining) {
      const double oks = oks_pair(xy + p, xy + t, vars, s_area[p], s_area[t], mask, nmask, J);
      if (soft)
        w = w * exp(-(oks * oks) / oks_thre);
      else if (oks > oks_thre)
        remaining = false;
    }
  }
  if (t == 0) kept[m] = count;
}

extern "C" {

// kpts [N,J,3] (x, y, confidence; image pixels), area / box_score [N], sigmas [J], index [N] + seg [M+1]: the detections
// of image m are index[seg[m] .. seg[m+1]) -> score [N], rank [N], kept [M]; see include/fami.h
int fami_pose_nms_f32(const float* kpts, const float* area, const float* box_score, const float* sigmas, const int* index,
                      const int* seg, int N, int J, int M, double in_vis_thre, double oks_thre, int soft, int max_dets,
                      double vis_thre, int use_vis, float* score, int* rank, int* kept, hipStream_t s) {
  FAMI_REQUIRE(kpts && area && box_score && sigmas && index && seg && score && rank && kept, "fami_pose_nms_f32",
               "null argument");
  FAMI_REQUIRE(J >= 1 && J <= NMS_JMAX, "fami_pose_nms_f32", "J must be in 1 .. 32");
  FAMI_REQUIRE(N >= 1 && (long)N * J * 3 <= 0x7fffffffL, "fami_pose_nms_f32", "N must be in 1 .. (2^31 - 1) / (3 J)");
  FAMI_REQUIRE(M >= 1 && M <= 0x7ffffffe, "fami_pose_nms_f32", "M must be in 1 .. 2^31 - 2");
  FAMI_REQUIRE((((uintptr_t)kpts | (uintptr_t)area | (uintptr_t)box_score | (uintptr_t)sigmas | (uintptr_t)index |
                 (uintptr_t)seg | (uintptr_t)score | (uintptr_t)rank | (uintptr_t)kept) & 3) == 0,
               "fami_pose_nms_f32", "every pointer must be 4-byte aligned");
  FAMI_REQUIRE(in_vis_thre == in_vis_thre && oks_thre == oks_thre && (!use_vis || vis_thre == vis_thre),
               "fami_pose_nms_f32", "a threshold is NaN");
  FAMI_REQUIRE(!soft || (oks_thre > 0.0 && max_dets >= 1), "fami_pose_nms_f32",
               "soft mode needs oks_thre > 0 and max_dets >= 1");
  fami_lds_limit<pose_nms_kernel>((int)nms_lds_bytes(NMS_JMAX));  // a dynamic allocation above 64 KiB (J = 32) needs the function attribute
  hipLaunchKernelGGL(pose_nms_kernel, dim3(M), dim3(NMS_THREADS), nms_lds_bytes(J), s, kpts, area, box_score, sigmas,
                     index, seg, score, rank, kept, N, J, in_vis_thre, oks_thre, soft ? 1 : 0, max_dets, vis_thre,
                     use_vis ? 1 : 0);
  FAMI_CHECK_LAUNCH("fami_pose_nms_f32");
  return FAMI_OK;
}

}  // extern "C"
