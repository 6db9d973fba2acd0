// The object-keypoint similarity of two poses held in LDS, shared by the pose NMS (nms.hip) and the pose tracker
// (track.hip): the reference's `oks_iou` (datasets/process/nms.py:51-86) in fp64 on fp32 inputs, one rounding per
// operation, the sum over the joints in ascending order.
#pragma once
#include "common.h"

#define OKS_CAP 256   // poses per LDS array: xy[j * OKS_CAP + i] is joint j of pose i
#define OKS_JMAX 32   // joints: one bit each in a visibility mask
#define OKS_UNROLL 4  // joints per trip of the loop
#define OKS_EPS 2.220446049250313e-16  // np.spacing(1), the reference's guard of the area term

// vars[j] = (2 sigma_j)^2 for one joint
__device__ __forceinline__ double oks_var(float sigma) {
#pragma clang fp contract(off)
  const double v = (double)sigma * 2.0;
  return v * v;
}

// OKS(q, d) = mean over the joints in `mask` (nmask = its population) of
//   exp(-(dx^2 + dy^2) / vars[j] / ((area_q + area_d) / 2 + 2^-52) / 2),  0 on an empty mask.
// q and d point at joint 0 of the two poses ((x, y) pairs, OKS_CAP apart per joint).  Each joint is a chain of two fp64
// divisions and an exp, several hundred cycles of dependent instructions; the loop runs OKS_UNROLL joints per trip without
// a branch (masked joints are computed and left out of the sum), so that as many chains overlap.
__device__ __forceinline__ double oks_pair(const float2* __restrict__ q, const float2* __restrict__ d,
                                           const double* __restrict__ vars, float area_q, float area_d, unsigned mask,
                                           int nmask, int J) {
#pragma clang fp contract(off)  // the reference's operation order, one rounding per operation
  const double a = ((double)area_q + (double)area_d) / 2.0 + OKS_EPS;
  double sum = 0.0;
  for (int j0 = 0; j0 < J; j0 += OKS_UNROLL) {
    double ex[OKS_UNROLL];
#pragma unroll
    for (int u = 0; u < OKS_UNROLL; ++u) {
      const int j = min(j0 + u, J - 1);
      const float2 pq = q[j * OKS_CAP], pd = d[j * OKS_CAP];
      const double dx = (double)pd.x - (double)pq.x, dy = (double)pd.y - (double)pq.y;
      ex[u] = exp(-((dx * dx + dy * dy) / vars[j] / a / 2.0));
    }
#pragma unroll
    for (int u = 0; u < OKS_UNROLL; ++u)  // summed in ascending j, masked joints (and the clamped tail) left out
      if (j0 + u < J && ((mask >> (j0 + u)) & 1u)) sum += ex[u];
  }
  return nmask ? sum / (double)nmask : 0.0;
}
