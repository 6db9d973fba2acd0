// PoseTrack MOTA on the device: the tracking half of the PoseTrack evaluation tool the reference vendors, restated from
// datasets/zoo/posetrack/posetrack_utils/poseval/py/evaluateTracking.py:13-222 (computeMetrics), the `mot` part of
// eval_helpers.assignGTmulti (:594-612, 648-658), py-motmetrics/motmetrics/mot.py:90-229 (MOTAccumulator.update,
// _sanitize_dists) and the count definitions of motmetrics/metrics.py:196-218.  include/fami.h has the rule.
//
// Shape.  The dependence runs along the frames of one (sequence, joint): the map m (annotated track -> the predicted
// track it was last matched to) is carried from frame to frame.  The S x 15 chains are independent (750 for PoseTrack17
// val), so every chain gets ONE 64-lane wavefront (a workgroup of 64) that walks its frames in order; nothing is shared
// between chains, every output word has one writer, there are no atomics, and two runs agree bit for bit.
// Per frame the wave
//   * compacts the annotated poses that still have the joint (<= 64: object row r is lane r's) and the predicted ones
//     (<= 256: hypothesis column c = k * 64 + lane, k < 4, is lane (c & 63)'s) into LDS by ballot + popcount,
//   * takes the largest valid distance for INV = 2 max + 1 (mot.py:225-226),
//   * carries forward: lane r looks up m[track(r)] among the frame's hypotheses, and keeps it when the pair is valid and no
//     earlier row wants the same column (the earlier row takes it, mot.py:145-159),
//   * solves the assignment of the remaining rows and columns by shortest augmenting paths (Jonker-Volgenant / the
//     Hungarian method with duals u, v).  The reference solves the full INV-filled rectangle; with every row free to stay
//     unassigned at cost INV that is the same problem (a constant apart), and it needs no transposition when there are
//     more rows than columns: row r has a private column 256 + r of cost INV, a valid pair costs its distance, everything
//     else (invalid pairs, rows and columns taken by the carry-forward) is forbidden.  A lane owns the duals, the
//     shortest-path labels and the `used` bits of its 5 columns in registers; the column minimum of every step is a
//     cross-lane (value, index) reduction by shuffles, the smaller column index on ties.  Which of several equal-cost
//     optima comes out is therefore a function of the input alone; it is not specified.
// Costs are recomputed from the staged coordinates (the expression of posetrack_ap.hip, so MOTA and AP decide
// `dist <= dist_thresh` on the same bits): a 64 x 256 fp64 matrix would be 128 KiB of LDS.  12.3 KiB are used.
// Every loop is bounded by the caps: the frames of the sequence, rows, columns, and rows + 1 steps per augmentation (each
// step marks one more assigned column used, and every assigned column holds a distinct earlier row).
//
// The alternative, a 256-thread workgroup with one column per thread, would put a workgroup barrier and an LDS tree
// behind every one of those steps; with the handful of poses a PoseTrack frame has, the steps are few and the fixed
// cost per frame (staging, compaction) dominates, which four times the threads do not shorten.  Not measured against
// each other: only this form was built.
#include "common.h"

#define MOT_J 15
#define MOT_JMASK 0x7fff
#define MOT_HCAP 256   // hypotheses per frame (the AP's cap on predicted poses)
#define MOT_OCAP 64    // objects per frame (the AP's cap on annotated poses)
#define MOT_TCAP 256   // annotated tracks per sequence
#define MOT_COLS (MOT_HCAP + MOT_OCAP)
#define MOT_NC 5       // columns per lane: 4 hypotheses + the private column of row `lane`

__device__ __forceinline__ double mot_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ int mot_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// dist of posetrack_ap.hip: sqrt(dx^2 + dy^2) / headSize, one rounding per operation
__device__ __forceinline__ double mot_dist(double ox, double oy, double head, double hx, double hy) {
#pragma clang fp contract(off)
  const double dx = ox - hx, dy = oy - hy;
  return sqrt(dx * dx + dy * dy) / head;
}

__global__ __launch_bounds__(64) void posetrack_mot_kernel(
    const double* __restrict__ pr_xys, const int* __restrict__ pr_has, const double* __restrict__ gt_xy,
    const int* __restrict__ gt_has, const double* __restrict__ gt_head, const int* __restrict__ pr_seg,
    const int* __restrict__ gt_seg, const int* __restrict__ poly_seg, const int* __restrict__ pr_track,
    const int* __restrict__ gt_track, const int* __restrict__ seq_seg, int P, int G, int F, double dist_thresh,
    int* __restrict__ counts, double* __restrict__ sumd, int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ double s_ox[MOT_OCAP], s_oy[MOT_OCAP], s_oh[MOT_OCAP], s_u[MOT_OCAP];
  __shared__ double s_hx[MOT_HCAP], s_hy[MOT_HCAP];
  __shared__ int s_hid[MOT_HCAP], s_taken[MOT_HCAP];
  __shared__ int s_oid[MOT_OCAP], s_cand[MOT_OCAP], s_match[MOT_OCAP];
  __shared__ int s_m[MOT_TCAP];
  __shared__ int s_p[MOT_COLS], s_way[MOT_COLS];
  const int s = blockIdx.x / MOT_J, j = blockIdx.x - s * MOT_J, lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  const double INF = __builtin_huge_val();
  const int f0 = seq_seg[s], f1 = seq_seg[s + 1];
  bool bad = f0 < 0 || f1 < f0 || f1 > F;  // wave-uniform throughout
  for (int i = lane; i < MOT_TCAP; i += 64) s_m[i] = -1;
  __syncthreads();
  int objs = 0, hyps = 0;          // wave-uniform: objects and hypotheses seen (dummy frames: one each)
  int ndet = 0, nsw = 0;           // lane r: detections and switches of object row r
  double sd = 0.0;                 // lane r: the distances of row r's detections
  // the last kept frame of a sequence is not evaluated (evaluateTracking.py:71)
  for (int f = f0; !bad && f < f1 - 1; ++f) {
    const int ps = pr_seg[f], pe = pr_seg[f + 1], gs = gt_seg[f], ge = gt_seg[f + 1];
    if (ps < 0 || pe < ps || pe > P || pe - ps > MOT_HCAP || gs < 0 || ge < gs || ge > G || ge - gs > MOT_OCAP) {
      bad = true;
      break;
    }
    const int np = pe - ps, ng = ge - gs;
    const bool poly = poly_seg[f + 1] > poly_seg[f];
    // a rect that the ignore filter emptied is no rect (removeIgnoredPointsRects); without regions every rect stays
    int gh = 0, gid = 0;
    if (lane < ng) {
      gh = gt_has[gs + lane] & MOT_JMASK;
      gid = gt_track[gs + lane];
    }
    const int ngr = __popcll(__ballot(lane < ng && (!poly || gh != 0)));
    int ph[4], pid[4], npr = 0;
    bool idbad = lane < ng && (gid < 0 || gid >= MOT_TCAP);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = k * 64 + lane;
      ph[k] = 0;
      pid[k] = 0;
      if (i < np) {
        ph[k] = pr_has[ps + i] & MOT_JMASK;
        pid[k] = pr_track[ps + i];
        idbad |= pid[k] < 0;
      }
      npr += __popcll(__ballot(i < np && (!poly || ph[k] != 0)));
    }
    if (__ballot(idbad) != 0ull) {
      bad = true;
      break;
    }
    if (ngr == 0 || npr == 0) {  // the reference's dummy lists: one MISS, one FP, one object (eval_helpers.py:648-658)
      ++objs;
      ++hyps;
      continue;
    }
    // objects and hypotheses of joint j, in list order
    const bool isobj = (gh >> j) & 1;
    const unsigned long long omask = __ballot(isobj);
    const int no = __popcll(omask);
    __syncthreads();  // the previous frame's readers are done
    if (isobj) {
      const int r = __popcll(omask & below);
      const double* __restrict__ h = gt_head + (long)(gs + lane) * 4;
      const double dx = h[2] - h[0], dy = h[3] - h[1];
      s_ox[r] = gt_xy[((long)(gs + lane) * MOT_J + j) * 2];
      s_oy[r] = gt_xy[((long)(gs + lane) * MOT_J + j) * 2 + 1];
      s_oh[r] = 0.6 * sqrt(dx * dx + dy * dy);
      s_oid[r] = gid;
    }
    int nh = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ishyp = (ph[k] >> j) & 1;
      const unsigned long long hmask = __ballot(ishyp);
      if (ishyp) {
        const int c = nh + __popcll(hmask & below);
        const long i = ps + k * 64 + lane;
        s_hx[c] = pr_xys[(i * MOT_J + j) * 3];
        s_hy[c] = pr_xys[(i * MOT_J + j) * 3 + 1];
        s_hid[c] = pid[k];
      }
      nh += __popcll(hmask);
    }
    objs += no;
    hyps += nh;
    if (no == 0 || nh == 0) continue;  // all MISS or all FP: both follow from the totals
#pragma unroll
    for (int k = 0; k < 4; ++k) s_taken[k * 64 + lane] = 0;
    s_u[lane] = 0.0;
    s_match[lane] = -1;
#pragma unroll
    for (int k = 0; k < MOT_NC; ++k) s_p[k * 64 + lane] = -1;
    __syncthreads();
    // this lane's columns and row
    double cx[4], cy[4];
    bool avail[MOT_NC];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = k * 64 + lane;
      avail[k] = c < nh;
      cx[k] = avail[k] ? s_hx[c] : 0.0;
      cy[k] = avail[k] ? s_hy[c] : 0.0;
    }
    const bool isrow = lane < no;
    const double rx = isrow ? s_ox[lane] : 0.0, ry = isrow ? s_oy[lane] : 0.0, rh = isrow ? s_oh[lane] : 1.0;
    const int roid = isrow ? s_oid[lane] : 0;
    // INV = 2 * (largest valid distance) + 1
    double mx = -1.0;
    for (int o = 0; o < no; ++o) {
      const double ox = s_ox[o], oy = s_oy[o], oh = s_oh[o];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double d = mot_dist(ox, oy, oh, cx[k], cy[k]);
        if (avail[k] && d <= dist_thresh && d > mx) mx = d;
      }
    }
    mx = mot_wave_max(mx);
    if (mx < 0.0) continue;  // no valid pair: nothing matches, m stays
    const double inv = 2.0 * mx + 1.0;
    // 1. carry forward
    int cand = -1;
    double dcand = 0.0;
    if (isrow) {
      const int hprev = s_m[roid];
      if (hprev >= 0) {
        for (int c = 0; c < nh; ++c)
          if (s_hid[c] == hprev) {
            cand = c;
            break;
          }
        if (cand >= 0) {
          dcand = mot_dist(rx, ry, rh, s_hx[cand], s_hy[cand]);
          if (!(dcand <= dist_thresh)) cand = -1;
        }
      }
    }
    s_cand[lane] = cand;
    __syncthreads();
    if (cand >= 0) {
      for (int r = 0; r < lane; ++r)
        if (s_cand[r] == cand) {  // an earlier object took that hypothesis
          cand = -1;
          break;
        }
    }
    if (cand >= 0) {
      s_taken[cand] = 1;
      ++ndet;
      sd += dcand;
    }
    const unsigned long long rtaken = __ballot(cand >= 0);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) avail[k] = avail[k] && s_taken[k * 64 + lane] == 0;
    avail[4] = isrow && !((rtaken >> lane) & 1ull);
    // 2. minimum-cost assignment of what is left, one row at a time
    double v[MOT_NC];
#pragma unroll
    for (int k = 0; k < MOT_NC; ++k) v[k] = 0.0;
    for (int i = 0; i < no && !bad; ++i) {
      if ((rtaken >> i) & 1ull) continue;
      double minv[MOT_NC];
#pragma unroll
      for (int k = 0; k < MOT_NC; ++k) minv[k] = INF;
      int used = 0, i0 = i, j0 = -1, jend = -1;
      for (int step = 0; step <= no; ++step) {
        const double ox = s_ox[i0], oy = s_oy[i0], oh = s_oh[i0], ui = s_u[i0];
        double best = INF;
        int bj = -1;
#pragma unroll
        for (int k = 0; k < MOT_NC; ++k) {
          if (avail[k] && !((used >> k) & 1)) {
            double a;
            if (k < 4) {
              a = mot_dist(ox, oy, oh, cx[k], cy[k]);
              if (!(a <= dist_thresh)) a = INF;
            } else {
              a = lane == i0 ? inv : INF;
            }
            const double cur = a - ui - v[k];
            if (cur < minv[k]) {
              minv[k] = cur;
              s_way[k * 64 + lane] = j0;
            }
            if (minv[k] < best) {  // k ascends: the smaller column of equal ones
              best = minv[k];
              bj = k * 64 + lane;
            }
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const double ob = __shfl_xor(best, o, 64);
          const int oj = __shfl_xor(bj, o, 64);
          if (oj >= 0 && (bj < 0 || ob < best || (ob == best && oj < bj))) {
            best = ob;
            bj = oj;
          }
        }
        if (bj < 0 || !(best < INF)) {  // cannot happen: row i's private column is free and finite
          bad = true;
          break;
        }
        __syncthreads();  // every lane has read s_u[i0]
#pragma unroll
        for (int k = 0; k < MOT_NC; ++k) {
          if ((used >> k) & 1) {
            s_u[s_p[k * 64 + lane]] += best;  // used columns hold distinct rows
            v[k] -= best;
          } else {
            minv[k] -= best;
          }
        }
        if (lane == 0) s_u[i] += best;  // the row being added (distinct from every assigned row)
        if (lane == (bj & 63)) used |= 1 << (bj >> 6);
        __syncthreads();
        j0 = bj;
        const int pj = s_p[bj];
        if (pj < 0) {
          jend = bj;
          break;
        }
        i0 = pj;
      }
      if (jend < 0) {  // the step bound ran out: cannot happen
        bad = true;
        break;
      }
      // augment along the path: at most `no` + 1 columns
      int jc = jend;
      for (int step = 0; step <= no && jc >= 0; ++step) {
        const int jp = s_way[jc];
        const int row = jp < 0 ? i : s_p[jp];
        __syncthreads();
        if (lane == 0) s_p[jc] = row;
        __syncthreads();
        jc = jp;
      }
    }
    if (bad) break;
    // the pairs: SWITCH where the object remembers another hypothesis, else MATCH; then m[o] = h
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = s_p[k * 64 + lane];
      if (r >= 0) s_match[r] = k * 64 + lane;
    }
    __syncthreads();
    if (isrow) {
      const int c = s_match[lane];
      if (c >= 0) {
        const int h = s_hid[c], prev = s_m[roid];
        if (prev >= 0 && prev != h) ++nsw;
        ++ndet;
        sd += mot_dist(rx, ry, rh, s_hx[c], s_hy[c]);
        s_m[roid] = h;
      }
    }
  }
  // totals of the chain: integers, and the 64 row sums in a fixed butterfly
  const int det = mot_wave_sum(ndet), sw = mot_wave_sum(nsw);
  const double total = wave_sum_d(sd);
  if (lane == 0) {
    int* __restrict__ c = counts + ((long)s * MOT_J + j) * 5;
    if (bad) {
      for (int k = 0; k < 5; ++k) c[k] = -1;
      sumd[(long)s * MOT_J + j] = 0.0;
    } else {
      c[0] = objs - det;  // num_misses
      c[1] = sw;          // num_switches
      c[2] = hyps - det;  // num_false_positives
      c[3] = det;         // num_detections = MATCH + SWITCH
      c[4] = objs;        // num_objects = MATCH + SWITCH + MISS
      sumd[(long)s * MOT_J + j] = total;
    }
    if (j == 0) status[s] = bad ? 1 : 0;  // the checks do not depend on the joint: one writer per sequence
  }
}

// the sequences added in index order, then evaluateTracking.py:158-192.  One workgroup; thread j owns joint j.
__global__ __launch_bounds__(64) void posetrack_mot_final_kernel(const int* __restrict__ counts,
                                                                 const double* __restrict__ sumd,
                                                                 const int* __restrict__ status, int S,
                                                                 int* __restrict__ totals, double* __restrict__ sumd_tot,
                                                                 double* __restrict__ table) {
#pragma clang fp contract(off)
  const int j = threadIdx.x;
  const double nan = __builtin_nan("");
  if (j < MOT_J) {
    int c[5] = {0, 0, 0, 0, 0};
    double sd = 0.0;
    for (int s = 0; s < S; ++s) {
      if (status[s] != 0) continue;
      for (int k = 0; k < 5; ++k) c[k] += counts[((long)s * MOT_J + j) * 5 + k];
      sd += sumd[(long)s * MOT_J + j];
    }
    for (int k = 0; k < 5; ++k) totals[j * 5 + k] = c[k];
    sumd_tot[j] = sd;
    const double miss = c[0], sw = c[1], fp = c[2], det = c[3];
    const double obj = c[4] > 0 ? (double)c[4] : nan;
    const double tot = c[2] + c[3] > 0 ? fp + det : nan;
    table[0 * 16 + j] = 100.0 * (1.0 - (miss + sw + fp) / obj);
    table[1 * 16 + j] = c[3] == 0 ? 0.0 : 100.0 * (1.0 - sd / det);
    table[2 * 16 + j] = 100.0 * (det / tot);
    table[3 * 16 + j] = 100.0 * (det / obj);
  }
  __syncthreads();
  if (j < 4) {  // entry 15: the mean over the non-NaN joints, in joint order (NaN when there is none)
    double sum = 0.0;
    int n = 0;
    for (int k = 0; k < MOT_J; ++k) {
      const double x = table[j * 16 + k];
      if (x == x) {
        sum += x;
        ++n;
      }
    }
    table[j * 16 + MOT_J] = sum / (double)n;
  }
}

extern "C" {

// see include/fami.h
int fami_posetrack_mot_f64(const double* pr_xys, const int* pr_has, const double* gt_xy, const int* gt_has,
                           const double* gt_head, const int* pr_seg, const int* gt_seg, const int* poly_seg,
                           const int* pr_track, const int* gt_track, const int* seq_seg, int P, int G, int F, int S,
                           double dist_thresh, int* counts, double* sumd, int* status, hipStream_t s) {
  const char* me = "fami_posetrack_mot_f64";
  FAMI_REQUIRE(P >= 0 && G >= 0 && (long)P * MOT_J * 3 <= 0x7fffffffL && (long)G * MOT_J * 2 <= 0x7fffffffL, me,
               "P and G must be >= 0 with P * 45 and G * 30 below 2^31");
  FAMI_REQUIRE(F >= 1 && F <= 0x7ffffffe / MOT_HCAP, me, "F must be in 1 .. (2^31 - 2) / 256");
  FAMI_REQUIRE(S >= 1 && S <= 0x7ffffffe / (MOT_J * 5), me, "S must be in 1 .. (2^31 - 2) / 75");
  FAMI_REQUIRE(pr_seg && gt_seg && poly_seg && seq_seg && counts && sumd && status, me, "null argument");
  FAMI_REQUIRE(P == 0 || (pr_xys && pr_has && pr_track), me, "null argument with P > 0");
  FAMI_REQUIRE(G == 0 || (gt_xy && gt_has && gt_head && gt_track), me, "null argument with G > 0");
  FAMI_REQUIRE((((uintptr_t)pr_xys | (uintptr_t)gt_xy | (uintptr_t)gt_head | (uintptr_t)sumd) & 7) == 0, me,
               "every fp64 pointer must be 8-byte aligned");
  FAMI_REQUIRE((((uintptr_t)pr_has | (uintptr_t)gt_has | (uintptr_t)pr_seg | (uintptr_t)gt_seg | (uintptr_t)poly_seg |
                 (uintptr_t)pr_track | (uintptr_t)gt_track | (uintptr_t)seq_seg | (uintptr_t)counts |
                 (uintptr_t)status) & 3) == 0,
               me, "every int pointer must be 4-byte aligned");
  FAMI_REQUIRE(dist_thresh == dist_thresh, me, "dist_thresh is NaN");
  hipLaunchKernelGGL(posetrack_mot_kernel, dim3(S * MOT_J), dim3(64), 0, s, pr_xys, pr_has, gt_xy, gt_has, gt_head, pr_seg,
                     gt_seg, poly_seg, pr_track, gt_track, seq_seg, P, G, F, dist_thresh, counts, sumd, status);
  FAMI_CHECK_LAUNCH(me);
  return FAMI_OK;
}

int fami_posetrack_mot_final_f64(const int* counts, const double* sumd, const int* status, int S, int* totals,
                                 double* sumd_tot, double* table, hipStream_t s) {
  const char* me = "fami_posetrack_mot_final_f64";
  FAMI_REQUIRE(S >= 1 && S <= 0x7ffffffe / (MOT_J * 5), me, "S must be in 1 .. (2^31 - 2) / 75");
  FAMI_REQUIRE(counts && sumd && status && totals && sumd_tot && table, me, "null argument");
  FAMI_REQUIRE((((uintptr_t)sumd | (uintptr_t)sumd_tot | (uintptr_t)table) & 7) == 0 &&
                   (((uintptr_t)counts | (uintptr_t)status | (uintptr_t)totals) & 3) == 0,
               me, "fp64 pointers must be 8-byte, int pointers 4-byte aligned");
  hipLaunchKernelGGL(posetrack_mot_final_kernel, dim3(1), dim3(64), 0, s, counts, sumd, status, S, totals, sumd_tot, table);
  FAMI_CHECK_LAUNCH(me);
  return FAMI_OK;
}

}  // extern "C"
