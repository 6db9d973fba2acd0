// COCO keypoint AP / AR on the device: the fourth step of the HRNet-family evaluation protocol, after flip testing
// (flip.hip), the DARK / integral decode (decode.hip) and rescoring + OKS-NMS (nms.hip): COCOeval(gt, dt, 'keypoints').
// pycocotools is not part of the reference tree; the definition is restated in include/fami.h (computeOks, evaluateImg,
// accumulate of cocoeval.py with iouType = 'keypoints', one category) and that text is the contract.  Two entry points, all
// arithmetic fp64 on fp64 inputs (annotations are arbitrary JSON doubles, and `OKS < best` is a decision: rounding an
// input to fp32 would move it -- the argument of posetrack_ap.hip):
//
// fami_coco_kpt_match_f64 -- per image, with detections d and annotations g:
//   1. the detections are ranked by descending score, equal scores by list position, and the first max_dets are kept;
//   2. OKS(d, g) for every kept d and every g: the mean over the labelled joints of g (v > 0) of
//        exp(-((dx^2 + dy^2) / vars_j / (area_g + 2^-52) / 2)),  dx = xd - xg, dy = yd - yg;
//      a g without a labelled joint takes the mean over ALL joints of the distance to its doubled box
//        dx = max(0, x0 - xd) + max(0, xd - x1),  x0 = bx - bw, x1 = bx + 2 bw  (and likewise dy);
//      one rounding per operation, the sum in ascending j (NOT oks_pair of oks.h: that one averages two areas, reads fp32);
//   3. per area range a and threshold t one greedy walk: the detections in score order, each over the annotations with
//      the non-ignored ones (ignore flag clear and lo <= area <= hi) first, list order otherwise; see fami.h.
//   Outputs per image and kept slot: score, source row, one byte per (a, t) (bit 0 matched, bit 1 ignored); per (image, a)
//   the number of non-ignored annotations.
// fami_coco_kpt_curve_f64 -- per (a, t), on the bytes gathered into global descending-score order (the stable sort is the
//   caller's): tp_k / fp_k cumulative counts of matched & !ignored / !matched & !ignored, rc_k = tp_k / npig,
//   pr_k = tp_k / (fp_k + tp_k + 2^-52), the suffix maximum of pr, and for each recall threshold r the envelope at the
//   first k with rc_k >= r (0 when there is none); recall = rc_last.
//
// Shape of the match.  Images are independent and small, and a validation set has thousands of them: one workgroup of
// 256 threads per image, as in nms.hip / posetrack_assign_kernel.  Thread i ranks detection i (at most 256) against the
// scores in LDS -- a count of the detections in front of it, which IS the stable order and needs no sort.  The image's
// annotations (at most 128) are staged in LDS as [J][128] x and y planes, so the lanes of a wave, which hold consecutive
// annotations against one detection, read consecutive words; the detection's own joints come from global memory at one
// address per wave.  One thread handles one OKS pair (a loop of J chains of two divisions and an exp), the kept x 128
// matrix stays in LDS, and the A * T walks then run one lane each: a walk is serial (a detection can only take what
// the ones before it left) but reads nothing except that matrix and 128-bit masks (ignored in range a, crowd, and per kept
// detection the annotations at or above the lowest threshold, which are all it can ever take), and keeps its own 128
// matched bits in two registers.  The stable "non-ignored first" order is two passes over the candidates.  No atomics, no
// workspace, every output word has one writer: two runs agree bit for bit.
// LDS: 8.9 KiB static + 2 KiB per joint + 1 KiB per kept slot (63 KiB at J = 17, max_dets = 20; 137 KiB at 32 / 64, hence
// the function attribute).
//
// Shape of the curve.  A * T independent scans over up to a few hundred thousand bytes: one workgroup per (a, t).  The
// scheme of posetrack_curve_kernel with two bits per detection: a coalesced pass packs tp and fp into two bit planes in
// LDS (a 64-lane ballot per word; 56 KiB hold 229376 detections, the cap), thread u then owns a contiguous run of words:
// popcounts -> exclusive prefixes over the 256 runs -> a forward walk for the run's largest precision.  The look-ups turn
// the search around: recall moves only where tp does, so threshold r needs the smallest COUNT c with c / npig >= r (a
// bisection on integers, evaluated with the very quotient the curve holds), the run that contains the c-th true positive
// (the prefixes), and one walk through that run from there on; its envelope is the larger of that walk's maximum and the
// later runs' maxima.  Every value written is int -> double, one add, one add of 2^-52 and one divide, or a maximum of
// such values: there is no sum whose order could differ from numpy's.
#include "common.h"

#define CK_THREADS 256
#define CK_DCAP CK_THREADS  // detections per image before the cut: one thread each
#define CK_GCAP 128         // annotations per image: LDS-resident, one mask bit each in two 64-bit words
#define CK_KCAP 64          // kept detections per image (max_dets)
#define CK_JMAX 32          // joints: one visibility bit each
#define CK_TMAX 32          // OKS thresholds
#define CK_AMAX 8           // area ranges
#define CK_RMAX 256         // recall thresholds: one thread each
#define CK_EPS 2.220446049250313e-16  // np.spacing(1)
#define CK_CURVE_MAX (7 << 15)        // detections of the set: two bits each in 56 KiB of dynamic LDS

// the thresholds travel as kernel arguments: the entry points read them on the host (a NaN is refused before any launch)
struct CkMatchParams {
  double vars[CK_JMAX];
  double thr[CK_TMAX];
  double rng[CK_AMAX * 2];
};
struct CkRecThrs {
  double r[CK_RMAX];
};

static inline size_t ck_match_lds(int J, int K) { return (size_t)K * CK_GCAP * 8 + (size_t)J * CK_GCAP * 16; }

__device__ __forceinline__ int ck_bit(unsigned long long lo, unsigned long long hi, int g) {
  return (int)(((g < 64 ? lo : hi) >> (g & 63)) & 1ull);
}

__global__ __launch_bounds__(CK_THREADS) void coco_kpt_match_kernel(
    const double* __restrict__ gt_kpts, const double* __restrict__ gt_area, const double* __restrict__ gt_bbox,
    const int* __restrict__ gt_flags, const double* __restrict__ dt_kpts, const double* __restrict__ dt_score,
    const double* __restrict__ dt_area, const int* __restrict__ gt_seg, const int* __restrict__ dt_seg,
    const CkMatchParams prm, int G, int D, int J, int T, int A, int K, double* __restrict__ out_score, int* __restrict__ out_row,
    unsigned char* __restrict__ out_flags, int* __restrict__ npig) {
#pragma clang fp contract(off)  // the definition's operation order, one rounding per operation
  extern __shared__ __attribute__((aligned(16))) unsigned char ck_lds[];
  double* __restrict__ s_oks = reinterpret_cast<double*>(ck_lds);  // [K][CK_GCAP]
  double* __restrict__ s_gx = s_oks + (size_t)K * CK_GCAP;         // [J][CK_GCAP]
  double* __restrict__ s_gy = s_gx + (size_t)J * CK_GCAP;          // [J][CK_GCAP]
  __shared__ double s_sc[CK_DCAP];
  __shared__ double s_garea[CK_GCAP];
  __shared__ double s_gbox[CK_GCAP * 4];
  __shared__ unsigned s_gvis[CK_GCAP];
  __shared__ unsigned long long s_gig[CK_AMAX][2];  // bit g: annotation g is ignored in range a
  __shared__ unsigned long long s_crowd[2];
  __shared__ int s_keep[CK_KCAP];  // the detection (image-local) in kept slot k
  __shared__ unsigned long long s_cand[CK_KCAP][2];  // bit g: annotation g can be taken by kept detection k at some threshold
  const int m = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int gs = gt_seg[m], ge = gt_seg[m + 1], ds = dt_seg[m], de = dt_seg[m + 1];
  // workgroup-uniform: an image whose segments cannot be addressed, or that is over a cap, is marked and left alone
  if (gs < 0 || ge < gs || ge > G || ge - gs > CK_GCAP || ds < 0 || de < ds || de > D || de - ds > CK_DCAP) {
    if (t < A) npig[(long)m * A + t] = -1;
    return;
  }
  const int ng = ge - gs, nd = de - ds, nk = min(nd, K);
  // stage: scores, annotations
  if (t < nd) s_sc[t] = dt_score[ds + t];
  if (t < CK_KCAP) s_keep[t] = 0;  // scores that are no total order (NaN) leave slots unranked: they stay addressable
  for (int i = t; i < ng * J; i += CK_THREADS) {
    const int g = i / J, j = i - g * J;
    const double* __restrict__ k = gt_kpts + ((long)(gs + g) * J + j) * 3;
    s_gx[j * CK_GCAP + g] = k[0];
    s_gy[j * CK_GCAP + g] = k[1];
  }
  int ign = 0, crowd = 0;
  double ga = 0.0;
  if (t < ng) {
    const double* __restrict__ k = gt_kpts + (long)(gs + t) * J * 3;
    unsigned vis = 0u;
    for (int j = 0; j < J; ++j)
      if (k[j * 3 + 2] > 0.0) vis |= 1u << j;
    s_gvis[t] = vis;
    ga = gt_area[gs + t];
    s_garea[t] = ga;
    for (int c = 0; c < 4; ++c) s_gbox[t * 4 + c] = gt_bbox[(long)(gs + t) * 4 + c];
    const int fl = gt_flags[gs + t];
    ign = fl & 1;
    crowd = (fl >> 1) & 1;
  }
  if (t < CK_GCAP) {  // waves 0 and 1, whole: every lane meets the ballots
    for (int a = 0; a < A; ++a) {
      const double lo = prm.rng[2 * a], hi = prm.rng[2 * a + 1];
      const unsigned long long w = __ballot(t < ng && (ign || ga < lo || ga > hi));
      if (lane == 0) s_gig[a][wave] = w;
    }
    const unsigned long long c = __ballot(t < ng && crowd);
    if (lane == 0) s_crowd[wave] = c;
  }
  __syncthreads();
  // rank: the number of detections in front of this one in the stable descending order
  if (t < nd) {
    const double sc = s_sc[t];
    int rank = 0;
    for (int u = 0; u < nd; ++u) {
      const double o = s_sc[u];
      rank += (o > sc || (o == sc && u < t)) ? 1 : 0;
    }
    if (rank < nk) s_keep[rank] = t;
  }
  if (t < A) npig[(long)m * A + t] = ng - __popcll(s_gig[t][0]) - __popcll(s_gig[t][1]);
  __syncthreads();
  // the score and the source row of every slot (empty slots: 0 and -1)
  if (t < K) {
    const int d = t < nk ? s_keep[t] : -1;
    out_score[(long)m * K + t] = d >= 0 ? s_sc[d] : 0.0;
    out_row[(long)m * K + t] = d >= 0 ? ds + d : -1;
  }
  // OKS of every (kept, annotated) pair
  for (int p = t; p < nk * ng; p += CK_THREADS) {
    const int k = p / ng, g = p - k * ng;
    const double* __restrict__ dk = dt_kpts + (long)(ds + s_keep[k]) * J * 3;
    const unsigned vis = s_gvis[g];
    const int k1 = __popc(vis);
    const double area = s_garea[g] + CK_EPS;
    const double bx = s_gbox[g * 4], by = s_gbox[g * 4 + 1], bw = s_gbox[g * 4 + 2], bh = s_gbox[g * 4 + 3];
    const double x0 = bx - bw, x1 = bx + bw * 2.0, y0 = by - bh, y1 = by + bh * 2.0;
    double sum = 0.0;
    for (int j = 0; j < J; ++j) {
      const double xd = dk[j * 3], yd = dk[j * 3 + 1];
      double dx, dy;
      if (k1 > 0) {
        dx = xd - s_gx[j * CK_GCAP + g];
        dy = yd - s_gy[j * CK_GCAP + g];
      } else {
        dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1);
        dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
      }
      const double e = (dx * dx + dy * dy) / prm.vars[j] / area / 2.0;
      if (k1 == 0 || ((vis >> j) & 1u)) sum += exp(-e);
    }
    s_oks[k * CK_GCAP + g] = sum / (double)(k1 > 0 ? k1 : J);
  }
  __syncthreads();
  // the candidates of every kept detection: the annotations whose OKS is not below the lowest threshold.  A walk starts at
  // its own threshold and only raises it, so it can take nothing else; most pairs of an image are far apart, and the walks
  // below then visit a handful of annotations where the list has up to 128.  One wave per row, a ballot per 64 annotations.
  double tmin = fmin(prm.thr[0], 1.0 - 1e-10);
  for (int i = 1; i < T; ++i) tmin = fmin(tmin, fmin(prm.thr[i], 1.0 - 1e-10));
  for (int k = wave; k < nk; k += CK_THREADS / 64) {  // wave-uniform trip count: every lane meets the ballots
    const unsigned long long c0 = __ballot(lane < ng && !(s_oks[k * CK_GCAP + lane] < tmin));
    const unsigned long long c1 = __ballot(64 + lane < ng && !(s_oks[k * CK_GCAP + 64 + lane] < tmin));
    if (lane == 0) {
      s_cand[k][0] = c0;
      s_cand[k][1] = c1;
    }
  }
  __syncthreads();
  // the A * T greedy walks, one lane each
  for (int w = t; w < A * T; w += CK_THREADS) {
    const int a = w / T, it = w - a * T;
    const double thr = fmin(prm.thr[it], 1.0 - 1e-10), lo = prm.rng[2 * a], hi = prm.rng[2 * a + 1];
    const unsigned long long ig0 = s_gig[a][0], ig1 = s_gig[a][1], cr0 = s_crowd[0], cr1 = s_crowd[1];
    unsigned long long m0 = 0ull, m1 = 0ull;  // matched at this (a, t)
    for (int k = 0; k < K; ++k) {
      unsigned char fl = 0;
      if (k < nk) {
        double best = thr;
        int mt = -1;
        // the non-ignored annotations first, then (only while nothing is taken) the ignored ones: the stable order, and
        // the rule that a non-ignored match ends the walk at the first ignored annotation.  Within a pass: list order,
        // without the annotations already matched here unless they are crowd; `not below best` takes, so a tie goes to
        // the later one
        for (int pass = 0; pass < 2 && mt < 0; ++pass)
          for (int h = 0; h < 2; ++h) {
            const unsigned long long ig = h ? ig1 : ig0, mm = h ? m1 : m0, cr = h ? cr1 : cr0;
            unsigned long long c = s_cand[k][h] & (pass ? ig : ~ig) & ~(mm & ~cr);
            while (c) {
              const int g = h * 64 + __builtin_ctzll(c);
              c &= c - 1ull;
              const double v = s_oks[k * CK_GCAP + g];
              if (v < best) continue;
              best = v;
              mt = g;
            }
          }
        if (mt >= 0) {
          fl = (unsigned char)(1 | (ck_bit(ig0, ig1, mt) << 1));
          if (mt < 64)
            m0 |= 1ull << mt;
          else
            m1 |= 1ull << (mt - 64);
        } else {
          const double da = dt_area[ds + s_keep[k]];
          fl = (da < lo || da > hi) ? 2 : 0;
        }
      }
      out_flags[((long)m * K + k) * (A * T) + w] = fl;
    }
  }
}

// one workgroup per (a, t); flags [A * T][N] bytes in descending-score order, npig_img [M][A]
__global__ __launch_bounds__(CK_THREADS) void coco_kpt_curve_kernel(const unsigned char* __restrict__ flags,
                                                                    const int* __restrict__ npig_img,
                                                                    const CkRecThrs rec, int N, int M, int T, int A, int R,
                                                                    double* __restrict__ precision,
                                                                    double* __restrict__ recall) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned char ck_lds[];
  const int nw = (N + 63) >> 6;
  unsigned long long* __restrict__ tpb = reinterpret_cast<unsigned long long*>(ck_lds);  // [nw] matched & !ignored
  unsigned long long* __restrict__ fpb = tpb + nw;                                        // [nw] !matched & !ignored
  __shared__ double s_max[CK_THREADS];  // the largest precision of run u
  __shared__ int s_tp[CK_THREADS];      // true positives of run u
  __shared__ int s_fp[CK_THREADS];
  __shared__ int s_i[CK_THREADS];
  const int w = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const int a = w / T, it = w - a * T;
  // npig: the images' counts, integers, summed in a fixed tree
  int acc = 0;
  for (int f = t; f < M; f += CK_THREADS) acc += npig_img[(long)f * A + a];
  s_i[t] = acc;
  __syncthreads();
  for (int o = CK_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) s_i[t] += s_i[t + o];
    __syncthreads();
  }
  const int np = s_i[0];
  if (np <= 0) {  // workgroup-uniform: nothing to find in this range
    for (int r = t; r < R; r += CK_THREADS) precision[((long)it * R + r) * A + a] = -1.0;
    if (t == 0) recall[it * A + a] = -1.0;
    return;
  }
  // two bits per detection: word q holds k = 64 q .. 64 q + 63 (wave-uniform trip count: every lane meets the ballots)
  const unsigned char* __restrict__ row = flags + (long)w * N;
  for (int base = t - lane; base < N; base += CK_THREADS) {
    const int k = base + lane;
    const int f = k < N ? row[k] : 2;
    const unsigned long long wt = __ballot((f & 3) == 1), wf = __ballot((f & 3) == 0);
    if (lane == 0) {
      tpb[base >> 6] = wt;
      fpb[base >> 6] = wf;
    }
  }
  __syncthreads();
  const int wpt = (nw + CK_THREADS - 1) / CK_THREADS;
  const int w0 = min(t * wpt, nw), w1 = min(w0 + wpt, nw);
  int ct = 0, cf = 0;
  for (int q = w0; q < w1; ++q) {
    ct += __popcll(tpb[q]);
    cf += __popcll(fpb[q]);
  }
  s_tp[t] = ct;
  s_fp[t] = cf;
  __syncthreads();
  int tp = 0, fp = 0;  // in front of this thread's run
  for (int u = 0; u < t; ++u) {
    tp += s_tp[u];
    fp += s_fp[u];
  }
  double mx = 0.0;
  for (int q = w0; q < w1; ++q) {
    const unsigned long long bt = tpb[q], bf = fpb[q];
    const int kn = min(64, N - q * 64);
    for (int b = 0; b < kn; ++b) {
      tp += (int)((bt >> b) & 1ull);
      fp += (int)((bf >> b) & 1ull);
      const double pr = (double)tp / ((double)fp + (double)tp + CK_EPS);
      mx = pr > mx ? pr : mx;
    }
  }
  s_max[t] = mx;
  __syncthreads();
  int total = 0;
  for (int u = 0; u < CK_THREADS; ++u) total += s_tp[u];
  const double dnp = (double)np;
  if (t == 0) recall[it * A + a] = N > 0 ? (double)total / dnp : 0.0;
  // the look-ups, one thread per recall threshold
  for (int r = t; r < R; r += CK_THREADS) {
    const double thr = rec.r[r];
    double q = 0.0;
    if (N > 0 && (double)total / dnp >= thr) {
      // the smallest count c with c / npig >= thr: the quotient is monotone in c
      int lo = 0, hi = total;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((double)mid / dnp >= thr)
          hi = mid;
        else
          lo = mid + 1;
      }
      const int c = lo;
      // the run in which the count first reaches c (run 0 for c = 0), and the counts in front of it
      int u = 0, btp = 0, bfp = 0;
      while (u < CK_THREADS - 1 && btp + s_tp[u] < c) {
        btp += s_tp[u];
        bfp += s_fp[u];
        ++u;
      }
      const int u0 = min(u * wpt, nw), u1 = min(u0 + wpt, nw);
      for (int qw = u0; qw < u1; ++qw) {
        const unsigned long long bt = tpb[qw], bf = fpb[qw];
        const int kn = min(64, N - qw * 64);
        for (int b = 0; b < kn; ++b) {
          btp += (int)((bt >> b) & 1ull);
          bfp += (int)((bf >> b) & 1ull);
          if (btp >= c) {  // from the first k with rc_k >= thr on: the envelope
            const double pr = (double)btp / ((double)bfp + (double)btp + CK_EPS);
            q = pr > q ? pr : q;
          }
        }
      }
      for (int v = u + 1; v < CK_THREADS; ++v) q = s_max[v] > q ? s_max[v] : q;
    }
    precision[((long)it * R + r) * A + a] = q;
  }
}

static bool ck_has_nan(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (v[i] != v[i]) return true;
  return false;
}

extern "C" {

// see include/fami.h
int fami_coco_kpt_match_f64(const double* gt_kpts, const double* gt_area, const double* gt_bbox, const int* gt_flags,
                            const double* dt_kpts, const double* dt_score, const double* dt_area, const int* gt_seg,
                            const int* dt_seg, const double* vars, const double* iou_thrs, const double* area_rng, int G,
                            int D, int M, int J, int T, int A, int max_dets, double* out_score, int* out_row,
                            unsigned char* out_flags, int* npig, hipStream_t s) {
  const char* me = "fami_coco_kpt_match_f64";
  FAMI_REQUIRE(J >= 1 && J <= CK_JMAX, me, "J must be in 1 .. 32");
  FAMI_REQUIRE(T >= 1 && T <= CK_TMAX && A >= 1 && A <= CK_AMAX, me, "T must be in 1 .. 32 and A in 1 .. 8");
  FAMI_REQUIRE(max_dets >= 1 && max_dets <= CK_KCAP, me, "max_dets must be in 1 .. 64");
  FAMI_REQUIRE(G >= 0 && D >= 0 && (long)G * J * 3 <= 0x7fffffffL && (long)D * J * 3 <= 0x7fffffffL, me,
               "G and D must be >= 0 with G * J * 3 and D * J * 3 below 2^31");
  FAMI_REQUIRE(M >= 1 && (long)M * max_dets * A * T <= 0x7fffffffL, me, "M must be >= 1 with M * max_dets * A * T below 2^31");
  FAMI_REQUIRE(gt_seg && dt_seg && vars && iou_thrs && area_rng && out_score && out_row && out_flags && npig, me,
               "null argument");
  FAMI_REQUIRE(G == 0 || (gt_kpts && gt_area && gt_bbox && gt_flags), me, "null argument with G > 0");
  FAMI_REQUIRE(D == 0 || (dt_kpts && dt_score && dt_area), me, "null argument with D > 0");
  FAMI_REQUIRE((((uintptr_t)gt_kpts | (uintptr_t)gt_area | (uintptr_t)gt_bbox | (uintptr_t)dt_kpts | (uintptr_t)dt_score |
                 (uintptr_t)dt_area | (uintptr_t)vars | (uintptr_t)iou_thrs | (uintptr_t)area_rng | (uintptr_t)out_score) & 7) == 0,
               me, "every fp64 pointer must be 8-byte aligned");
  FAMI_REQUIRE((((uintptr_t)gt_flags | (uintptr_t)gt_seg | (uintptr_t)dt_seg | (uintptr_t)out_row | (uintptr_t)npig) & 3) == 0,
               me, "every int pointer must be 4-byte aligned");
  FAMI_REQUIRE(!ck_has_nan(vars, J) && !ck_has_nan(iou_thrs, T) && !ck_has_nan(area_rng, 2 * A), me, "a threshold is NaN");
  CkMatchParams prm = {};
  for (int j = 0; j < J; ++j) prm.vars[j] = vars[j];
  for (int i = 0; i < T; ++i) prm.thr[i] = iou_thrs[i];
  for (int i = 0; i < 2 * A; ++i) prm.rng[i] = area_rng[i];
  fami_lds_limit<coco_kpt_match_kernel>((int)ck_match_lds(CK_JMAX, CK_KCAP));  // above 64 KiB: needs the function attribute
  hipLaunchKernelGGL(coco_kpt_match_kernel, dim3(M), dim3(CK_THREADS), ck_match_lds(J, max_dets), s, gt_kpts, gt_area, gt_bbox,
                     gt_flags, dt_kpts, dt_score, dt_area, gt_seg, dt_seg, prm, G, D, J, T, A, max_dets, out_score, out_row,
                     out_flags, npig);
  FAMI_CHECK_LAUNCH(me);
  return FAMI_OK;
}

int fami_coco_kpt_curve_f64(const unsigned char* flags, const int* npig_img, const double* rec_thrs, int N, int M, int T,
                            int A, int R, double* precision, double* recall, hipStream_t s) {
  const char* me = "fami_coco_kpt_curve_f64";
  FAMI_REQUIRE(N >= 0 && N <= CK_CURVE_MAX, me, "N must be in 0 .. 229376");
  FAMI_REQUIRE(T >= 1 && T <= CK_TMAX && A >= 1 && A <= CK_AMAX && R >= 1 && R <= CK_RMAX, me,
               "T must be in 1 .. 32, A in 1 .. 8 and R in 1 .. 256");
  FAMI_REQUIRE(M >= 1 && M <= 0x7ffffffe / CK_AMAX, me, "M must be in 1 .. (2^31 - 2) / 8");
  FAMI_REQUIRE(npig_img && rec_thrs && precision && recall && (N == 0 || flags), me, "null argument");
  FAMI_REQUIRE((((uintptr_t)rec_thrs | (uintptr_t)precision | (uintptr_t)recall) & 7) == 0 && ((uintptr_t)npig_img & 3) == 0,
               me, "the fp64 pointers must be 8-byte, npig_img 4-byte aligned");
  FAMI_REQUIRE(!ck_has_nan(rec_thrs, R), me, "a threshold is NaN");
  CkRecThrs rec = {};
  for (int r = 0; r < R; ++r) rec.r[r] = rec_thrs[r];
  const size_t lds = (size_t)((N + 63) / 64) * 16;
  hipLaunchKernelGGL(coco_kpt_curve_kernel, dim3(A * T), dim3(CK_THREADS), lds, s, flags, npig_img, rec, N, M, T, A, R,
                     precision, recall);
  FAMI_CHECK_LAUNCH(me);
  return FAMI_OK;
}

}  // extern "C"
