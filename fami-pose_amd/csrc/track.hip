// Pose tracking by object-keypoint similarity on the device: person identities for the poses the evaluation wrote so far
// with a placeholder track_id.  The reference declares the intent (EVAL_TRACKING / TRACKING_THRESHOLD,
// posetimation/config/defaults.py:34-36; the eval_tracking argument of convert_data_to_annorect_struct) and has no rule;
// the rule is this project's, stated in include/fami.h.  The similarity is the reference's `oks_iou`
// (datasets/process/nms.py:51-86), the arithmetic of nms.hip (oks.h).  Per video, frames in ascending frame number:
//   1. every live track with frame - last_frame > max_gap is retired;
//   2. the detections of the frame are walked in list order: detection d takes the live track with the largest
//      OKS(track, d) among those not yet matched in this frame (ties: the lowest track id), if that OKS is > oks_thre --
//      it gets the track's id and the track takes d's pose, area and frame number -- and is new otherwise;
//   3. the new detections get ids next_id, next_id + 1, ... in list order and become live tracks.
// One workgroup of 256 threads per video, thread t owning track SLOT t (at most 256 live tracks), no atomics and no
// workspace: every output word has exactly one writer, so two runs agree bit for bit.
//
// Shape.  A video is a chain of one dependent round per detection, each ending in the one barrier behind which its
// outcome becomes known, so what matters is the latency of a round:
//   * the live tracks' poses and the frame's detections are LDS-resident (2 x [J][256] (x, y) pairs).  A round reads the
//     detection (one address for the whole wave: a broadcast) and each lane's own track (consecutive 8-byte words:
//     conflict-free).  A track's pose is read and rewritten by its own thread only, so it needs no barrier.
//   * only a track whose OKS exceeds the threshold enters the argmax (the largest OKS is taken only if it is > oks_thre,
//     so the others cannot change the outcome); the argmax is a 64-lane butterfly per wave over (OKS, id << 8 | slot) and
//     four LDS slots per workgroup, double-buffered by the parity of the round as in nms.hip: ONE barrier per round.
//     The outcome of a round is read from the same four slots by every thread, so it is workgroup-uniform, and with it
//     the count and the list of the frame's new detections.
//   * a wave none of whose tracks compete skips the OKS of the round; it still meets the barrier.
//   * per frame three more barriers: behind the staging of the detections (which also carries "an index is out of
//     range"), behind the per-wave counts of free slots (the k-th free slot takes the k-th new detection), and in front
//     of the next staging, which overwrites what the new tracks copy from.
// The segment tables are read by every thread alike (workgroup-uniform), so a malformed one ends the video without a
// vote.  All LDS is dynamic and 16-byte aligned; at J = 32 it is 132 KiB, hence the function attribute.
#include "common.h"
#include "oks.h"

#define TRK_THREADS 256
#define TRK_WAVES (TRK_THREADS / 64)
#define TRK_CAP TRK_THREADS          // live tracks, and detections per frame
#define TRK_NONE 0x7fffffffffffffffL  // "no track" in the argmax

// dynamic LDS: vars[32] f64 | argmax slots [2][4] f64 + [2][4] i64 | bad / free counts [2][4] i32 | area, mask, row, new list [256] each
//              | track xy[J][256] float2 | detection xy[J][256] float2
#define TRK_LDS_FIXED (OKS_JMAX * 8 + 2 * TRK_WAVES * 8 + 2 * TRK_WAVES * 8 + 2 * TRK_WAVES * 4 + 4 * TRK_CAP * 4)
static_assert(TRK_WAVES == 4 && TRK_CAP == OKS_CAP && TRK_LDS_FIXED % 16 == 0, "the (x, y) arrays must start 16-byte aligned");
static inline size_t trk_lds_bytes(int J) { return TRK_LDS_FIXED + (size_t)J * TRK_CAP * 16; }

// (w, k) better than (bw, bk)?  k = id << 8 | slot, unique per live track; TRK_NONE never wins.
__device__ __forceinline__ bool trk_better(double w, long k, double bw, long bk) {
  return k != TRK_NONE && (bk == TRK_NONE || w > bw || (w == bw && k < bk));
}

__global__ __launch_bounds__(TRK_THREADS) void pose_track_kernel(
    const float* __restrict__ kpts, const float* __restrict__ area, const float* __restrict__ sigmas,
    const int* __restrict__ index, const int* __restrict__ fseg, const int* __restrict__ fnum,
    const int* __restrict__ vseg, int* __restrict__ track, int* __restrict__ ntracks, int N, int J, int n, int M,
    double oks_thre, int max_gap, double vis_thre, int use_vis) {
  extern __shared__ __attribute__((aligned(16))) unsigned char trk_lds[];
  double* __restrict__ vars = reinterpret_cast<double*>(trk_lds);           // [OKS_JMAX]  (2 sigma_j)^2
  double* __restrict__ redw = vars + OKS_JMAX;                                // [2][TRK_WAVES]
  long* __restrict__ redk = reinterpret_cast<long*>(redw + 2 * TRK_WAVES);   // [2][TRK_WAVES]
  int* __restrict__ wbad = reinterpret_cast<int*>(redk + 2 * TRK_WAVES);     // [TRK_WAVES] a bad index in the wave's share
  int* __restrict__ wcnt = wbad + TRK_WAVES;                                 // [TRK_WAVES] free slots per wave
  float* __restrict__ d_area = reinterpret_cast<float*>(wcnt + TRK_WAVES);   // [TRK_CAP] the frame's detections: area,
  unsigned* __restrict__ d_mask = reinterpret_cast<unsigned*>(d_area + TRK_CAP);  // joints that count,
  int* __restrict__ d_row = reinterpret_cast<int*>(d_mask + TRK_CAP);        // row of kpts,
  int* __restrict__ newdet = d_row + TRK_CAP;                                // and the positions of the new ones, in list order
  float2* __restrict__ txy = reinterpret_cast<float2*>(newdet + TRK_CAP);    // [J][TRK_CAP] live tracks
  float2* __restrict__ dxy = txy + J * TRK_CAP;                              // [J][TRK_CAP] detections of the frame
  const int v = blockIdx.x, t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int vs = vseg[v], ve = vseg[v + 1];
  // everything read from vseg, fseg and fnum is workgroup-uniform
  if (vs < 0 || ve < vs || ve > M) {  // not a segment of the M frames: nothing of it can be addressed
    if (t == 0) ntracks[v] = -1;
    return;
  }
  if (t < J) vars[t] = oks_var(sigmas[t]);  // published by the first frame's staging barrier
  // the track of slot t
  bool live = false;
  int id = 0, last = 0;
  float t_area = 0.f;
  int next_id = 0;
  for (int fi = vs; fi < ve; ++fi) {
    const int s = fseg[fi], e = fseg[fi + 1], f = fnum[fi];
    if (s < 0 || e < s || e > n || e - s > TRK_CAP || (fi > vs && f <= fnum[fi - 1])) {
      if (t == 0) ntracks[v] = -1;  // no segment of index[0 .. n), over the cap, or frame numbers not ascending
      return;
    }
    const int nd = e - s;
    if (live && (long)f - (long)last > (long)max_gap) live = false;
    bool matched = false;
    // stage the detections: thread t holds the t-th of the frame's list
    int bad = 0;
    if (t < nd) {
      const int g = index[s + t];
      if ((unsigned)g < (unsigned)N) {
        const float* __restrict__ k = kpts + (long)g * J * 3;
        unsigned mask = 0u;
        for (int j = 0; j < J; ++j) {
          dxy[j * TRK_CAP + t] = make_float2(k[j * 3], k[j * 3 + 1]);
          if (!use_vis || (double)k[j * 3 + 2] > vis_thre) mask |= 1u << j;
        }
        d_area[t] = area[g];
        d_mask[t] = mask;
        d_row[t] = g;
      } else {
        bad = 1;
      }
    }
    const bool wave_bad = __ballot(bad) != 0ull;
    if (lane == 0) wbad[wave] = wave_bad;  // (slots of its own: a frame without detections has no barrier up to the counts)
    __syncthreads();
    if (wbad[0] | wbad[1] | wbad[2] | wbad[3]) {
      if (t == 0) ntracks[v] = -1;  // an index outside [0, N)
      return;
    }
    int nnew = 0;
    for (int d = 0; d < nd; ++d) {
      double bw = 0.0;
      long bk = TRK_NONE;
      if (live && !matched) {
        const unsigned mask = d_mask[d];
        const double oks = oks_pair(txy + t, dxy + d, vars, t_area, d_area[d], mask, __popc(mask), J);
        if (oks > oks_thre) {
          bw = oks;
          bk = ((long)id << 8) | t;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ow = __shfl_xor(bw, o, 64);
        const long ok = __shfl_xor(bk, o, 64);
        if (trk_better(ow, ok, bw, bk)) {
          bw = ow;
          bk = ok;
        }
      }
      const int buf = (d & 1) * TRK_WAVES;
      if (lane == 0) {
        redw[buf + wave] = bw;
        redk[buf + wave] = bk;
      }
      __syncthreads();
      bw = redw[buf];
      bk = redk[buf];
#pragma unroll
      for (int k = 1; k < TRK_WAVES; ++k)
        if (trk_better(redw[buf + k], redk[buf + k], bw, bk)) {
          bw = redw[buf + k];
          bk = redk[buf + k];
        }
      // the same in every thread: all read the same four slots in the same order
      if (bk == TRK_NONE) {
        if (t == 0) newdet[nnew] = d;
        ++nnew;
      } else if (t == (int)(bk & 255)) {  // this slot's track takes detection d
        matched = true;
        last = f;
        t_area = d_area[d];
        for (int j = 0; j < J; ++j) txy[j * TRK_CAP + t] = dxy[j * TRK_CAP + d];
        track[d_row[d]] = id;
      }
    }
    // the k-th free slot takes the k-th new detection
    const unsigned long long fb = __ballot(!live);
    if (lane == 0) wcnt[wave] = __popcll(fb);
    __syncthreads();  // publishes the counts and thread 0's newdet
    int before = 0, nfree = 0;
#pragma unroll
    for (int k = 0; k < TRK_WAVES; ++k) {
      if (k < wave) before += wcnt[k];
      nfree += wcnt[k];
    }
    if (nnew > nfree) {  // more than TRK_CAP live tracks
      if (t == 0) ntracks[v] = -1;
      return;
    }
    const int k = before + __popcll(fb & ((1ull << lane) - 1ull));
    if (!live && k < nnew) {
      const int d = newdet[k];
      live = true;
      id = next_id + k;
      last = f;
      t_area = d_area[d];
      for (int j = 0; j < J; ++j) txy[j * TRK_CAP + t] = dxy[j * TRK_CAP + d];
      track[d_row[d]] = id;
    }
    next_id += nnew;
    __syncthreads();  // the next frame's staging overwrites the detections
  }
  if (t == 0) ntracks[v] = next_id;
}

extern "C" {

// kpts [N,J,3], area [N], sigmas [J], index [n] + fseg [M+1] + fnum [M] + vseg [V+1]: the detections of frame m are
// index[fseg[m] .. fseg[m+1]), its number fnum[m], the frames of video v are vseg[v] .. vseg[v+1) -> track [N],
// ntracks [V]; see include/fami.h
int fami_pose_track_f32(const float* kpts, const float* area, const float* sigmas, const int* index, const int* fseg,
                        const int* fnum, const int* vseg, int N, int J, int n, int M, int V, double oks_thre, int max_gap,
                        double vis_thre, int use_vis, int* track, int* ntracks, hipStream_t s) {
  FAMI_REQUIRE(kpts && area && sigmas && index && fseg && fnum && vseg && track && ntracks, "fami_pose_track_f32",
               "null argument");
  FAMI_REQUIRE(J >= 1 && J <= OKS_JMAX, "fami_pose_track_f32", "J must be in 1 .. 32");
  FAMI_REQUIRE(N >= 1 && (long)N * J * 3 <= 0x7fffffffL, "fami_pose_track_f32", "N must be in 1 .. (2^31 - 1) / (3 J)");
  FAMI_REQUIRE(n >= 0 && M >= 1 && M <= 0x7ffffffe && V >= 1 && V <= 0x7ffffffe, "fami_pose_track_f32",
               "n must be >= 0, M and V in 1 .. 2^31 - 2");
  FAMI_REQUIRE((((uintptr_t)kpts | (uintptr_t)area | (uintptr_t)sigmas | (uintptr_t)index | (uintptr_t)fseg |
                 (uintptr_t)fnum | (uintptr_t)vseg | (uintptr_t)track | (uintptr_t)ntracks) & 3) == 0,
               "fami_pose_track_f32", "every pointer must be 4-byte aligned");
  FAMI_REQUIRE(oks_thre == oks_thre && (!use_vis || vis_thre == vis_thre), "fami_pose_track_f32", "a threshold is NaN");
  FAMI_REQUIRE(max_gap >= 1, "fami_pose_track_f32", "max_gap must be >= 1");
  fami_lds_limit<pose_track_kernel>((int)trk_lds_bytes(OKS_JMAX));  // a dynamic allocation above 64 KiB needs the function attribute
  hipLaunchKernelGGL(pose_track_kernel, dim3(V), dim3(TRK_THREADS), trk_lds_bytes(J), s, kpts, area, sigmas, index, fseg,
                     fnum, vseg, track, ntracks, N, J, n, M, oks_thre, max_gap, vis_thre, use_vis ? 1 : 0);
  FAMI_CHECK_LAUNCH("fami_pose_track_f32");
  return FAMI_OK;
}

}  // extern "C"
