// The point, the squared distance and the row mapping of the geometry kernels
// (gnn_geometry.hip, gnn_cells.hip), defined once: every search, brute force or binned, and
// every pair-distance kernel computes d2 through this sq_dist, so their results agree bit for
// bit.
//
//   dx = p_i[0] - p_j[0], dy = p_i[1] - p_j[1], dz = p_i[2] - p_j[2]     each one fp32 subtract
//   d2 = fma(dz, dz, fma(dy, dy, dx * dx))                                explicit, no contraction
// with the terms of absent coordinates dropped (D = 2: fma(dy, dy, dx * dx); D = 1: dx * dx).
//
// Device code only; include after cgnn_common.h (xcd_remap).
#pragma once
#include "cgnn_common.h"

namespace cgnn {
namespace geo {

template <int D>
struct Point {
  float c[D];
};

template <int D>
__device__ __forceinline__ Point<D> load_point(const float* __restrict__ pos, int i, int ldp) {
  Point<D> p;
  const float* q = pos + (size_t)i * ldp;
#pragma unroll
  for (int c = 0; c < D; ++c) p.c[c] = q[c];
  return p;
}

template <int D>
__device__ __forceinline__ float sq_dist(const Point<D>& a, const Point<D>& b) {
  const float dx = __fsub_rn(a.c[0], b.c[0]);
  float d2 = __fmul_rn(dx, dx);
  if (D > 1) {
    const float dy = __fsub_rn(a.c[D > 1 ? 1 : 0], b.c[D > 1 ? 1 : 0]);
    d2 = __fmaf_rn(dy, dy, d2);
  }
  if (D > 2) {
    const float dz = __fsub_rn(a.c[D > 2 ? 2 : 0], b.c[D > 2 ? 2 : 0]);
    d2 = __fmaf_rn(dz, dz, d2);
  }
  return d2;
}

// the row of this sub-group and its lane in it
template <int L>
__device__ __forceinline__ long sub_row(int& sub, int& sl) {
  constexpr int RPW = 64 / L;
  const int lane = threadIdx.x & 63;
  sub = lane / L;
  sl = lane - sub * L;
  const unsigned blk = xcd_remap(blockIdx.x, gridDim.x);
  return ((long)blk * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + sub;
}

}  // namespace geo
}  // namespace cgnn
