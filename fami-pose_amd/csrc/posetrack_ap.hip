// PoseTrack AP on the device: the pose half of the PoseTrack evaluation tool the reference vendors, restated from
// datasets/zoo/posetrack/posetrack_utils/poseval/py/eval_helpers.py (removeIgnoredPoints :322-367, assignGTmulti :453-668,
// computeRPC / VOCap :192-228) and evaluateAP.py:8-47 (computeMetrics).  Two entry points, all arithmetic fp64 on fp64
// inputs (the ground truth is arbitrary JSON doubles; rounding it to fp32 would move `dist <= 0.5` decisions):
//
// fami_posetrack_assign_f64 -- per frame, with predicted poses p and annotated poses g (15 joints, one has-bit each):
//   1. the has-bit of every point (predicted and annotated) inside any ignore polygon of its OWN frame is cleared: the
//      even-odd crossing rule, for every edge (i, j = i - 1, closing edge included)
//        (y_i > y) != (y_j > y)  and  x < (x_j - x_i) * (y - y_i) / (y_j - y_i) + x_i   toggles `inside`
//      (a point exactly on an edge: unspecified).  The cleared masks are outputs.
//   2. headSize(g) = 0.6 * sqrt(dx^2 + dy^2) of the head rectangle; dist = sqrt(dx^2 + dy^2) / headSize(g) where both
//      joints exist; match = dist <= dist_thresh (headSize 0 gives inf or NaN: no match);
//      pck[p,g] = #match / nGTp[g] (undivided where nGTp[g] = 0).  Every p keeps its best g (first on ties); every g then
//      takes the p with the largest remaining pck (first on ties, none when that is 0).  label[p] = the match bits of a
//      taken p against its g, 0 for every other p; assigned[p] = that g (frame-local) or -1; ngt_frame[f,j] = the number
//      of annotated poses of the frame that still have joint j.
// fami_posetrack_curve_f64 -- per joint, on the labels in descending-score order (the stable sort is the caller's):
//   npos_k = positives among the first k + 1; precision_k = npos_k / (k + 1); recall_k = npos_k / nGT;
//   envelope_k = max(precision_k ..); AP = sum over the k where recall changes of (recall_k - recall_(k-1)) * envelope_k,
//   recall_(-1) = 0, plus the reference's closing term (1 - recall_last) * 0; ap / pre / rec = AP, the last precision,
//   the last recall, x 100; row 15 = the mean over the non-NaN joints.  nGT = 0 with predictions gives NaN (0 / 0) for ap
//   and rec as in the reference; no prediction gives 0.
//
// Shape of the assignment.  Frames are independent and small (a handful of poses), and there are tens of thousands of
// them: one workgroup of 256 threads per frame, thread t owning predicted pose t (cap 256), as in nms.hip.  A thread
// holds its own pose in registers (30 doubles, the joint loop is unrolled) and walks the frame's annotated poses, which
// sit in LDS ([64][15] (x, y) fp64 = 15 KiB, head size, mask, joint count: 19.3 KiB in all, so eight frames per CU): every
// lane reads the SAME annotated joint in a step -- one LDS address per wave, a broadcast -- where a global read would put
// an L2 round trip behind each of the G x 15 steps.  The "every g takes its best p" step is G independent arg-max walks
// over at most 256 LDS words, one thread per g: no atomics, every output word has one writer, two runs agree bit for bit.
// Three barriers per frame (staged ground truth; cleared masks and head sizes; every p's best g).
//
// Shape of the curve.  15 independent joints, each a scan over up to a few hundred thousand labels: one workgroup per
// joint.  The labels are packed to one bit each in LDS by a coalesced pass (a 64-lane ballot per word; 56 KiB hold
// 458752 labels, the cap), then thread t owns a contiguous run of 64-bit words: popcount -> exclusive prefix over the 256
// runs -> a forward walk for the run's largest precision -> suffix maximum over the runs -> a backward walk that carries
// the envelope and adds the run's AP terms in descending k.  The 256 partial sums are added in a fixed binary tree, so the
// result depends on the input alone.  Only the summation order of the AP differs from numpy's; the quotients are the
// reference's expressions (npos / (k + 1), npos / nGT, and a recall step as the difference of two quotients).
#include "common.h"

#define AP_THREADS 256
#define AP_PCAP AP_THREADS  // predicted poses per frame: one thread each
#define AP_GCAP 64          // annotated poses per frame: LDS-resident
#define AP_J 15             // PoseTrack joints: one bit each
#define AP_JMASK 0x7fff
#define AP_CURVE_MAX (7 << 16)  // labels per joint: one bit each in 56 KiB of dynamic LDS

// even-odd test of (x, y) against the polygons [ps, pe) of a frame; vert_seg ranges were checked by the caller
__device__ __forceinline__ bool ap_ignored(double x, double y, const int* __restrict__ vert_seg,
                                           const double* __restrict__ verts, int ps, int pe) {
#pragma clang fp contract(off)
  for (int q = ps; q < pe; ++q) {
    const int vs = vert_seg[q], n = vert_seg[q + 1] - vs;
    bool inside = false;
    for (int i = 0, j = n - 1; i < n; j = i++) {
      const double xi = verts[2 * (long)(vs + i)], yi = verts[2 * (long)(vs + i) + 1];
      const double xj = verts[2 * (long)(vs + j)], yj = verts[2 * (long)(vs + j) + 1];
      if ((yi > y) != (yj > y)) {
        const double xc = (xj - xi) * (y - yi) / (yj - yi) + xi;
        if (x < xc) inside = !inside;
      }
    }
    if (inside) return true;
  }
  return false;
}

__global__ __launch_bounds__(AP_THREADS) void posetrack_assign_kernel(
    const double* __restrict__ pr_xys, const int* __restrict__ pr_has, const double* __restrict__ gt_xy,
    const int* __restrict__ gt_has, const double* __restrict__ gt_head, const int* __restrict__ pr_seg,
    const int* __restrict__ gt_seg, const int* __restrict__ poly_seg, const int* __restrict__ vert_seg,
    const double* __restrict__ verts, int P, int G, int NP, int NV, double dist_thresh, int* __restrict__ pr_has_out,
    int* __restrict__ gt_has_out, int* __restrict__ label, int* __restrict__ assigned, int* __restrict__ ngt_frame) {
#pragma clang fp contract(off)  // the reference's operation order, one rounding per operation
  __shared__ double s_gxy[AP_GCAP * AP_J * 2];
  __shared__ double s_head[AP_GCAP];
  __shared__ double s_pck[AP_PCAP];  // pck of p against its best g
  __shared__ int s_best[AP_PCAP];    // that g
  __shared__ int s_ghas[AP_GCAP];
  __shared__ int s_gn[AP_GCAP];
  __shared__ int s_taker[AP_GCAP];
  const int f = blockIdx.x, t = threadIdx.x;
  const int ps0 = pr_seg[f], pe0 = pr_seg[f + 1], gs = gt_seg[f], ge = gt_seg[f + 1];
  const int qs = poly_seg[f], qe = poly_seg[f + 1];
  // workgroup-uniform up to the first barrier: a frame whose segments cannot be addressed, or that is over a cap, is marked
  bool bad = ps0 < 0 || pe0 < ps0 || pe0 > P || pe0 - ps0 > AP_PCAP || gs < 0 || ge < gs || ge > G || ge - gs > AP_GCAP ||
             qs < 0 || qe < qs || qe > NP;
  if (!bad)
    for (int q = qs; q < qe; ++q) {
      const int vs = vert_seg[q], ve = vert_seg[q + 1];
      bad |= vs < 0 || ve < vs || ve > NV;
    }
  if (bad) {
    if (t < AP_J) ngt_frame[(long)f * AP_J + t] = -1;
    return;
  }
  const int np = pe0 - ps0, ng = ge - gs;
  for (int i = t; i < ng * AP_J * 2; i += AP_THREADS) s_gxy[i] = gt_xy[(long)gs * AP_J * 2 + i];
  __syncthreads();

  // step 1 (and the head sizes): thread t clears predicted pose t and annotated pose t
  double px[AP_J], py[AP_J];
  int has = 0;
  if (t < np) {
    const double* __restrict__ k = pr_xys + (long)(ps0 + t) * AP_J * 3;
    has = pr_has[ps0 + t] & AP_JMASK;
#pragma unroll
    for (int j = 0; j < AP_J; ++j) {
      px[j] = k[j * 3];
      py[j] = k[j * 3 + 1];
      if (((has >> j) & 1) && qe > qs && ap_ignored(px[j], py[j], vert_seg, verts, qs, qe)) has &= ~(1 << j);
    }
    pr_has_out[ps0 + t] = has;
  }
  if (t < ng) {
    int gh = gt_has[gs + t] & AP_JMASK;
    if (qe > qs)
      for (int j = 0; j < AP_J; ++j)
        if (((gh >> j) & 1) && ap_ignored(s_gxy[(t * AP_J + j) * 2], s_gxy[(t * AP_J + j) * 2 + 1], vert_seg, verts, qs, qe))
          gh &= ~(1 << j);
    gt_has_out[gs + t] = gh;
    s_ghas[t] = gh;
    s_gn[t] = __popc(gh);
    const double* __restrict__ h = gt_head + (long)(gs + t) * 4;
    const double dx = h[2] - h[0], dy = h[3] - h[1];
    s_head[t] = 0.6 * sqrt(dx * dx + dy * dy);
  }
  __syncthreads();
  if (t < AP_J) {
    int c = 0;
    for (int g = 0; g < ng; ++g) c += (s_ghas[g] >> t) & 1;
    ngt_frame[(long)f * AP_J + t] = c;
  }

  // step 2: every p keeps its best g
  int bg = 0, bm = 0;
  double bv = 0.0;
  if (t < np) {
    for (int g = 0; g < ng; ++g) {
      const int hm = has & s_ghas[g];
      const double head = s_head[g];
      int m = 0;
#pragma unroll
      for (int j = 0; j < AP_J; ++j) {
        const double dx = s_gxy[(g * AP_J + j) * 2] - px[j], dy = s_gxy[(g * AP_J + j) * 2 + 1] - py[j];
        const double d = sqrt(dx * dx + dy * dy) / head;
        if (((hm >> j) & 1) && d <= dist_thresh) m |= 1 << j;
      }
      const int gn = s_gn[g];
      const double v = gn > 0 ? (double)__popc(m) / (double)gn : (double)__popc(m);
      if (g == 0 || v > bv) {
        bv = v;
        bg = g;
        bm = m;
      }
    }
    s_best[t] = bg;
    s_pck[t] = bv;
  }
  __syncthreads();
  // every g takes the p with the largest remaining pck
  if (t < ng) {
    int tk = -1;
    double tv = 0.0;
    for (int p = 0; p < np; ++p)
      if (s_best[p] == t && s_pck[p] > tv) {
        tv = s_pck[p];
        tk = p;
      }
    s_taker[t] = tk;
  }
  __syncthreads();
  if (t < np) {
    const bool taken = ng > 0 && s_taker[bg] == t;
    label[ps0 + t] = taken ? bm : 0;
    assigned[ps0 + t] = taken ? bg : -1;
  }
}

// one workgroup per joint; lab [15][P] bytes (non-zero: a true positive) in descending-score order, n[j] of them valid
__global__ __launch_bounds__(AP_THREADS) void posetrack_curve_kernel(const unsigned char* __restrict__ lab,
                                                                     const int* __restrict__ n_valid,
                                                                     const int* __restrict__ ngt_frame, int P, int F,
                                                                     double* __restrict__ out, int* __restrict__ ngt_out) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned char ap_lds[];
  unsigned long long* __restrict__ bits = reinterpret_cast<unsigned long long*>(ap_lds);
  __shared__ double s_d[AP_THREADS];
  __shared__ int s_i[AP_THREADS];
  const int j = blockIdx.x, t = threadIdx.x, lane = t & 63;
  int n = n_valid[j];
  n = n < 0 ? 0 : (n > P ? P : n);
  // nGT[j]: the frames' counts, integers, summed in a fixed tree
  int acc = 0;
  for (int f = t; f < F; f += AP_THREADS) acc += ngt_frame[(long)f * AP_J + j];
  s_i[t] = acc;
  __syncthreads();
  for (int o = AP_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) s_i[t] += s_i[t + o];
    __syncthreads();
  }
  const int ngt = s_i[0];
  __syncthreads();  // s_i is reused below
  // the labels, one bit each: word w holds k = 64 w .. 64 w + 63 (wave-uniform trip count: every lane meets the ballot)
  const unsigned char* __restrict__ row = lab + (long)j * P;
  for (int base = t - lane; base < n; base += AP_THREADS) {
    const int k = base + lane;
    const unsigned long long w = __ballot(k < n && row[k] != 0);
    if (lane == 0) bits[base >> 6] = w;
  }
  __syncthreads();
  const int nw = (n + 63) >> 6, wpt = (nw + AP_THREADS - 1) / AP_THREADS;
  const int w0 = min(t * wpt, nw), w1 = min(w0 + wpt, nw);
  int cnt = 0;
  for (int w = w0; w < w1; ++w) cnt += __popcll(bits[w]);
  s_i[t] = cnt;
  __syncthreads();
  int before = 0;  // positives in front of this thread's run
  for (int u = 0; u < t; ++u) before += s_i[u];
  // forward: the largest precision of the run
  double mx = 0.0;
  int npos = before;
  for (int w = w0; w < w1; ++w) {
    const unsigned long long word = bits[w];
    const int kn = min(64, n - w * 64);
    for (int b = 0; b < kn; ++b) {
      npos += (int)((word >> b) & 1ull);
      const double prec = (double)npos / (double)(w * 64 + b + 1);
      mx = prec > mx ? prec : mx;
    }
  }
  s_d[t] = mx;
  __syncthreads();
  double env = 0.0;  // the envelope right of the run; 0 is the reference's closing sentinel
  for (int u = AP_THREADS - 1; u > t; --u) env = s_d[u] > env ? s_d[u] : env;
  __syncthreads();  // s_d is reused below
  // backward: the envelope, and the AP terms of the run in descending k.  recall changes where the label is 1 (and
  // compares unequal everywhere when nGT = 0 makes it NaN)
  double sum = 0.0;
  const double dgt = (double)ngt;
  for (int w = w1 - 1; w >= w0; --w) {
    const unsigned long long word = bits[w];
    const int kn = min(64, n - w * 64);
    for (int b = kn - 1; b >= 0; --b) {
      const int k = w * 64 + b, bit = (int)((word >> b) & 1ull);
      const double prec = (double)npos / (double)(k + 1);
      env = prec > env ? prec : env;
      if (bit || ngt == 0) {
        const double rec = (double)npos / dgt, prev = k == 0 ? 0.0 : (double)(npos - bit) / dgt;
        if (rec != prev) sum += (rec - prev) * env;
      }
      npos -= bit;
    }
  }
  s_d[t] = sum;
  __syncthreads();
  for (int o = AP_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) s_d[t] += s_d[t + o];
    __syncthreads();
  }
  if (t == 0) {
    double ap = 0.0, pre = 0.0, rec = 0.0;
    if (n > 0) {
      int total = 0;
      for (int u = 0; u < AP_THREADS; ++u) total += s_i[u];
      const double last = (double)total / dgt;
      ap = s_d[0];
      if (last != 1.0) ap += (1.0 - last) * 0.0;  // the closing term: 0, or NaN / inf kept as the reference keeps them
      ap *= 100.0;
      pre = (double)total / (double)n * 100.0;
      rec = last * 100.0;
    }
    out[j] = ap;
    out[16 + j] = pre;
    out[32 + j] = rec;
    ngt_out[j] = ngt;
  }
}

// row 15 of ap / pre / rec: the mean over the non-NaN joints, summed in joint order (NaN when every joint is NaN)
__global__ void posetrack_mean_kernel(double* __restrict__ out) {
#pragma clang fp contract(off)
  const int r = threadIdx.x;
  if (r >= 3) return;
  double s = 0.0;
  int c = 0;
  for (int j = 0; j < AP_J; ++j) {
    const double v = out[r * 16 + j];
    if (v == v) {
      s += v;
      ++c;
    }
  }
  out[r * 16 + AP_J] = s / (double)c;
}

extern "C" {

// see include/fami.h
int fami_posetrack_assign_f64(const double* pr_xys, const int* pr_has, const double* gt_xy, const int* gt_has,
                              const double* gt_head, const int* pr_seg, const int* gt_seg, const int* poly_seg,
                              const int* vert_seg, const double* verts, int P, int G, int F, int NP, int NV,
                              double dist_thresh, int* pr_has_out, int* gt_has_out, int* label, int* assigned,
                              int* ngt_frame, hipStream_t s) {
  const char* me = "fami_posetrack_assign_f64";
  FAMI_REQUIRE(P >= 0 && G >= 0 && NP >= 0 && NV >= 0 && (long)P * AP_J * 3 <= 0x7fffffffL &&
                   (long)G * AP_J * 2 <= 0x7fffffffL && NV <= 0x3fffffff,
               me, "P, G, NP, NV must be >= 0 with P * 45, G * 30 and NV * 2 below 2^31");
  FAMI_REQUIRE(F >= 1 && F <= 0x7ffffffe / AP_J, me, "F must be in 1 .. (2^31 - 2) / 15");
  FAMI_REQUIRE(pr_seg && gt_seg && poly_seg && vert_seg && ngt_frame, me, "null argument");
  FAMI_REQUIRE(P == 0 || (pr_xys && pr_has && pr_has_out && label && assigned), me, "null argument with P > 0");
  FAMI_REQUIRE(G == 0 || (gt_xy && gt_has && gt_head && gt_has_out), me, "null argument with G > 0");
  FAMI_REQUIRE(NV == 0 || verts, me, "null verts with NV > 0");
  FAMI_REQUIRE((((uintptr_t)pr_xys | (uintptr_t)gt_xy | (uintptr_t)gt_head | (uintptr_t)verts) & 7) == 0, me,
               "every fp64 pointer must be 8-byte aligned");
  FAMI_REQUIRE((((uintptr_t)pr_has | (uintptr_t)gt_has | (uintptr_t)pr_seg | (uintptr_t)gt_seg | (uintptr_t)poly_seg |
                 (uintptr_t)vert_seg | (uintptr_t)pr_has_out | (uintptr_t)gt_has_out | (uintptr_t)label |
                 (uintptr_t)assigned | (uintptr_t)ngt_frame) & 3) == 0,
               me, "every int pointer must be 4-byte aligned");
  FAMI_REQUIRE(dist_thresh == dist_thresh, me, "dist_thresh is NaN");
  hipLaunchKernelGGL(posetrack_assign_kernel, dim3(F), dim3(AP_THREADS), 0, s, pr_xys, pr_has, gt_xy, gt_has, gt_head,
                     pr_seg, gt_seg, poly_seg, vert_seg, verts, P, G, NP, NV, dist_thresh, pr_has_out, gt_has_out, label,
                     assigned, ngt_frame);
  FAMI_CHECK_LAUNCH(me);
  return FAMI_OK;
}

int fami_posetrack_curve_f64(const unsigned char* lab, const int* n_valid, const int* ngt_frame, int P, int F, double* out,
                             int* ngt, hipStream_t s) {
  const char* me = "fami_posetrack_curve_f64";
  FAMI_REQUIRE(P >= 0 && P <= AP_CURVE_MAX, me, "P must be in 0 .. 458752");
  FAMI_REQUIRE(F >= 1 && F <= 0x7ffffffe / AP_J, me, "F must be in 1 .. (2^31 - 2) / 15");
  FAMI_REQUIRE(n_valid && ngt_frame && out && ngt && (P == 0 || lab), me, "null argument");
  FAMI_REQUIRE(((uintptr_t)out & 7) == 0 && (((uintptr_t)n_valid | (uintptr_t)ngt_frame | (uintptr_t)ngt) & 3) == 0, me,
               "out must be 8-byte, the int pointers 4-byte aligned");
  const size_t lds = (size_t)((P + 63) / 64) * 8;
  hipLaunchKernelGGL(posetrack_curve_kernel, dim3(AP_J), dim3(AP_THREADS), lds, s, lab, n_valid, ngt_frame, P, F, out, ngt);
  FAMI_CHECK_LAUNCH(me);
  hipLaunchKernelGGL(posetrack_mean_kernel, dim3(1), dim3(64), 0, s, out);
  FAMI_CHECK_LAUNCH(me);
  return FAMI_OK;
}

}  // extern "C"
