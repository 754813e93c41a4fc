// GNN track (beyond the reference): softmax over each destination node's incoming edges
// (DGL's edge_softmax, PyG's softmax(src, index)) for MI355X, and its gradient.
//
//   edge_softmax_fwd_kernel  p[k,e]  = exp(scale (s[k,e] - m)) / sum_e' exp(scale (s[k,e'] - m))
//                            over the edges e of row i = [rowptr[i], rowptr[i+1]), m the
//                            row's maximum of head k, scale > 0
//   edge_softmax_bwd_kernel  ds[k,e] = scale p[k,e] (dp[k,e] - sum_e' p[k,e'] dp[k,e'])
//
// Layout.  Scores, probabilities and their gradients are fp32 and head-major, [K, ld]:
// head k's value of edge e is at k * ld + e (size_t), ld >= nnz.  One head is a contiguous
// [nnz] slice, which ops.sddmm writes and ops.wspmm reads in place.
//
// Mapping.  wave64; a sub-group of L lanes (8 / 16 / 32 / 64) owns one (row, head) and lane
// sl takes the edges e0 + sl, e0 + sl + L, ...: every load and store of a chunk is
// coalesced, and the sub-groups of a wave own consecutive rows, that is consecutive edge
// ranges.  A block of 256 threads serves 4 * (64 / L) consecutive rows of one head.  Rows
// of at most 4 L edges stay in registers (one read, one write per element); a longer row
// loops over its edges three times (the maximum; the exponentials, stored unnormalised;
// the scaling) with the same arithmetic.  The launcher picks L from nnz / n_rows (8 up to
// 16 edges per row on average, 16 up to 32, 32 up to 64, else 64), or takes it as `lanes`.
//
// Arithmetic of the forward, per element, c = fl(scale * log2 e) (rounded once, on the host):
//   d = s - m_;  t = d * c;  x = v_exp_f32(t);  l = sum x;  r = 1 / l;  p = x * r
// m_ = m, or 0 when m = -inf.  The backward is g = fma(p, dp, g) per lane, then
// ds = (scale * p) * (dp - g).
//
// Determinism.  No atomics.  A lane adds its elements in edge order starting from 0, then
// the L partial sums are combined by an xor butterfly (distances 1, 2, ... L / 2), in which
// both partners of a step compute the same commutative sum: every lane holds the same
// bits.  The order of a (row, head) depends only on its own length and on L -- not on the
// grid, the row's position, the other rows or the run, and not on which of the two paths
// (registers / loops) serves it, since both add the same values in the same order.
//
// Edge cases.  An empty row reads and writes nothing (rowptr alone is dereferenced for it:
// every other load sits behind an e < e1 test).  A row with one edge gives exactly 1.0f
// (d = 0, x = 1, l = 1).  A score of -inf gives exactly 0; a row whose scores are all -inf
// gives all 0 (l = 0 -> r = 0), not NaN.  A NaN or +inf score makes every output of its
// (row, head) NaN (the maximum drops a NaN, then d is NaN for that element; +inf gives
// d = inf - inf) and touches no other row or head.
//
// In place.  p may alias s and ds may alias dp: each element is read and written by one
// lane, and written after that lane's last read of it.  (ds must not alias p.)
// Nothing outside [k * ld, k * ld + nnz) of any head is written.
#include "cgnn_common.h"
#include "cgnn_api.h"
#include <cmath>

using namespace cgnn;

namespace {

constexpr int ES_REG = 4;                          // elements per lane of the in-register path

template <int L>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int d = 1; d < L; d <<= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  return v;
}

template <int L>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int d = 1; d < L; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// the (row, head) of this sub-group: its edge range and the offset of its head
struct Unit {
  int e0, e1, sl;
  size_t base;
};

template <int L>
__device__ __forceinline__ Unit unit_of(const int* __restrict__ rowptr, int n_rows, unsigned row_blocks, size_t ld) {
  constexpr int RPW = 64 / L;
  const int lane = threadIdx.x & 63;
  const int sub = lane / L;
  const unsigned blk = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned k = blk / row_blocks, rb = blk - k * row_blocks;
  const long row = ((long)rb * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + sub;
  const bool rv = row < n_rows;
  Unit u;
  u.sl = lane - sub * L;
  u.e0 = rv ? rowptr[row] : 0;
  u.e1 = rv ? rowptr[row + 1] : 0;
  u.base = (size_t)k * ld;
  return u;
}

}  // namespace

// S and P may be the same buffer: no __restrict__ on them
template <int L>
__global__ __launch_bounds__(256) void edge_softmax_fwd_kernel(const int* __restrict__ rowptr, const float* S, float* P,
                                                               int n_rows, unsigned row_blocks, size_t ld, float c) {
  const Unit u = unit_of<L>(rowptr, n_rows, row_blocks, ld);
  const float* s = S + u.base;
  float* p = P + u.base;
  const int e0 = u.e0, e1 = u.e1, sl = u.sl;
  const float ninf = -__builtin_inff();
  const bool reg = e1 - e0 <= ES_REG * L;         // uniform per sub-group; an empty row loads nothing
  float v[ES_REG];
  float m = ninf;
  if (reg) {
#pragma unroll
    for (int r = 0; r < ES_REG; ++r) {
      const int e = e0 + r * L + sl;
      v[r] = e < e1 ? s[e] : ninf;
      m = fmaxf(m, v[r]);
    }
  } else {
#pragma unroll 4
    for (int e = e0 + sl; e < e1; e += L) m = fmaxf(m, s[e]);
  }
  m = group_max<L>(m);
  const float ms = m == ninf ? 0.f : m;
  float l = 0.f;
  if (reg) {
#pragma unroll
    for (int r = 0; r < ES_REG; ++r) {
      v[r] = __builtin_amdgcn_exp2f((v[r] - ms) * c);
      l += v[r];
    }
  } else {
#pragma unroll 4
    for (int e = e0 + sl; e < e1; e += L) {
      const float x = __builtin_amdgcn_exp2f((s[e] - ms) * c);
      p[e] = x;
      l += x;
    }
  }
  l = group_sum<L>(l);
  const float rinv = l == 0.f ? 0.f : 1.f / l;    // a NaN sum stays NaN
  if (reg) {
#pragma unroll
    for (int r = 0; r < ES_REG; ++r) {
      const int e = e0 + r * L + sl;
      if (e < e1) p[e] = v[r] * rinv;
    }
  } else {
#pragma unroll 4
    for (int e = e0 + sl; e < e1; e += L) p[e] = p[e] * rinv;
  }
}

// DP and DS may be the same buffer
template <int L>
__global__ __launch_bounds__(256) void edge_softmax_bwd_kernel(const int* __restrict__ rowptr, const float* __restrict__ Pm,
                                                               const float* DP, float* DS, int n_rows,
                                                               unsigned row_blocks, size_t ld, float scale) {
  const Unit u = unit_of<L>(rowptr, n_rows, row_blocks, ld);
  const float* p = Pm + u.base;
  const float* dp = DP + u.base;
  float* ds = DS + u.base;
  const int e0 = u.e0, e1 = u.e1, sl = u.sl;
  const bool reg = e1 - e0 <= ES_REG * L;
  float pv[ES_REG], gv[ES_REG];
  float g = 0.f;
  if (reg) {
#pragma unroll
    for (int r = 0; r < ES_REG; ++r) {
      const int e = e0 + r * L + sl;
      const bool ok = e < e1;
      pv[r] = ok ? p[e] : 0.f;
      gv[r] = ok ? dp[e] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < ES_REG; ++r) g = fmaf(pv[r], gv[r], g);
  } else {
#pragma unroll 4
    for (int e = e0 + sl; e < e1; e += L) g = fmaf(p[e], dp[e], g);
  }
  g = group_sum<L>(g);
  if (reg) {
#pragma unroll
    for (int r = 0; r < ES_REG; ++r) {
      const int e = e0 + r * L + sl;
      if (e < e1) ds[e] = (scale * pv[r]) * (gv[r] - g);
    }
  } else {
#pragma unroll 4
    for (int e = e0 + sl; e < e1; e += L) ds[e] = (scale * p[e]) * (dp[e] - g);
  }
}

// ---------------------------------------------------------------- launchers
// the sub-group width for an average of nnz / n_rows edges per row: the average row takes at
// most two of the four register elements of a lane
static int es_auto_lanes(int n_rows, int nnz) {
  const long a = (long)nnz;
  if (a <= 16L * n_rows) return 8;
  if (a <= 32L * n_rows) return 16;
  if (a <= 64L * n_rows) return 32;
  return 64;
}

// the argument checks the two launchers share; 1: go on and launch
static int es_prepare(int n_rows, int nnz, int K, long ld, float scale, int lanes, int* L) {
  // (the forward multiplies by scale * log2 e: that product has to be finite too)
  if (K < 1 || nnz < 0 || ld < nnz || !(scale > 0.f) || !std::isfinite(scale * 1.5f)) return -3;
  if (lanes != 0 && lanes != 8 && lanes != 16 && lanes != 32 && lanes != 64) return -1;
  if (n_rows <= 0 || nnz == 0) return 0;
  *L = lanes ? lanes : es_auto_lanes(n_rows, nnz);
  return 1;
}

// blocks of the (row blocks x heads) grid, or 0 when it would overflow: the launch counts
// its threads in 32 bits
static unsigned es_grid(int n_rows, int K, int L, unsigned* row_blocks) {
  const int rpb = 4 * (64 / L);
  const long rb = ((long)n_rows + rpb - 1) / rpb;
  *row_blocks = (unsigned)rb;
  const long lim = (1L << 24) - 1;                 // * 256 threads < 2^32
  if (K > lim || rb > lim / K) return 0;
  return (unsigned)(rb * K);
}

// p [K, ld] = the softmax of s [K, ld] over each row's edges.  lanes: 0 = auto, or one of
// the compiled sub-group widths 8 / 16 / 32 / 64.  No allocation and no synchronisation:
// capturable into a hipGraph.  Return codes: see cgnn_api.h.
extern "C" int gnn_launch_edge_softmax_fwd(const int* rowptr, const float* s, float* p, int n_rows, int nnz, int K,
                                           long ld, float scale, int lanes, hipStream_t st) {
  int L = 0;
  const int rc = es_prepare(n_rows, nnz, K, ld, scale, lanes, &L);
  if (rc <= 0) return rc;
  if (!rowptr || !s || !p) return -3;
  unsigned rb = 0;
  const unsigned blocks = es_grid(n_rows, K, L, &rb);
  if (!blocks) return -4;
  const float c = (float)((double)scale * 1.4426950408889634);
  dim3 grid(blocks), block(256);
#define CGNN_ES(LL) \
  hipLaunchKernelGGL((edge_softmax_fwd_kernel<LL>), grid, block, 0, st, rowptr, s, p, n_rows, rb, (size_t)ld, c)
  if (L == 8) CGNN_ES(8);
  else if (L == 16) CGNN_ES(16);
  else if (L == 32) CGNN_ES(32);
  else CGNN_ES(64);
#undef CGNN_ES
  return (int)hipGetLastError();
}

// ds [K, ld] from the forward's output p and the incoming dp, all with the row stride ld
extern "C" int gnn_launch_edge_softmax_bwd(const int* rowptr, const float* p, const float* dp, float* ds, int n_rows,
                                           int nnz, int K, long ld, float scale, int lanes, hipStream_t st) {
  int L = 0;
  const int rc = es_prepare(n_rows, nnz, K, ld, scale, lanes, &L);
  if (rc <= 0) return rc;
  if (!rowptr || !p || !dp || !ds) return -3;
  unsigned rb = 0;
  const unsigned blocks = es_grid(n_rows, K, L, &rb);
  if (!blocks) return -4;
  dim3 grid(blocks), block(256);
#define CGNN_ES(LL) \
  hipLaunchKernelGGL((edge_softmax_bwd_kernel<LL>), grid, block, 0, st, rowptr, p, dp, ds, n_rows, rb, (size_t)ld, scale)
  if (L == 8) CGNN_ES(8);
  else if (L == 16) CGNN_ES(16);
  else if (L == 32) CGNN_ES(32);
  else CGNN_ES(64);
#undef CGNN_ES
  return (int)hipGetLastError();
}
