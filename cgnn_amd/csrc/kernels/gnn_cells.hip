// GNN track (beyond the reference): the cell-list (binned) radius search for large point
// clouds on MI355X -- the radius graph of gnn_geometry.hip in O(n) instead of O(n_g^2).
//
//   cells_part_kernel    per chunk of 1024 points: min / max of the finite points, per axis
//   cells_grid_kernel    per graph: lo[3], the bin scale per axis, n_a cells per axis
//   cells_bin_kernel     cell_id[i] = the global cell of point i, or the sentinel n + G
//   cells_search_kernel  FILL = false: deg[i]; FILL = true: the row of i in scan order into a
//                        scratch edge list (j, d2) at rowptr[i] ..
//   cells_rows_kernel    col / d2 = the scratch rows in ascending source id
// Between bin and search the points are put in cell order on the device by the caller
// (ops.cells_order: a stable sort by cell_id, the row pointer of the cells, a gathered copy of
// the positions padded to 16 bytes).
//
// Contract.  For the same pos, D, r, gptr, seg_id and loop the pipeline gives deg, rowptr,
// col and d2 equal, element for element, to radius_count_kernel / radius_fill_kernel of
// gnn_geometry.hip: rows in ascending source id, d2 <= r2 inclusive with r2 = r * r one fp32
// product made on the host, d2 from the one sq_dist of gnn_point.h, coincident points are
// neighbours, a point with a NaN or inf coordinate has no edge and is nobody's neighbour (the
// brute kernels get there through a NaN distance; here the point goes to the sentinel cell,
// which no row scans).  No atomics; ordinary vector stores; the CSR is the same for every
// sub-group width, grid and run, and a graph's rows, relative to gptr[g], do not depend on
// its place in the batch (the grid of a graph is a function of its own points and r).
// One deliberate limit: seg_id[i] must be the graph whose range [gptr[g], gptr[g + 1]) holds
// i, as in every GraphBatch, or lie outside [0, G).  A point whose seg_id is outside, or names
// another graph's range, goes to the sentinel cell: an empty row, and nobody's neighbour (in
// the brute kernels it would stay a candidate of the range it stands in).
//
// The grid of graph g, computed on the device from its finite points (all D coordinates
// finite) in [gptr[g], gptr[g + 1]) and r alone; fp32, each operation rounded once:
//   lo_a, hi_a   min / max of coordinate a                      (no finite point: one cell)
//   s0           = max(r * (1 + 2^-10), 2^-60)                  the least cell side
//   ext_a        = hi_a - lo_a
//   n_a          = min(1024, (int)(ext_a / s0)) when 2 s0 <= ext_a <= 2^100, else 1
//   reduction    while n_0 n_1 n_2 > max(1, n_g): n_a = (n_a + 1) / 2 for the largest n_a (the
//                lowest axis among equals)
//   scale_a      = n_a / ext_a when n_a >= 2, else 0
//   bin_a(x)     = min(n_a - 1, (int)((x - lo_a) * scale_a))    monotone in x: a monotone
//                  rounding of a subtraction, of a product with scale_a >= 0, a truncation
//                  of a value >= 0, a minimum
//   cell(p)      = gptr[g] + g + (bin_0 n_1 + bin_1) n_2 + bin_2   (absent axes: n_a = 1)
// An axis of extent zero, below two cell sides, overflowing (coordinates near +-FLT_MAX) or
// beyond 2^100 has one cell; a graph with one cell on every axis is exactly the brute-force
// search.  r = 0 is legal (s0 = 2^-60).  The cells of graph g number at most max(1, n_g), so
// they fit the id range [gptr[g] + g, gptr[g + 1] + g + 1), every table has the host-known
// size n + G + 1 (the sentinel is id n + G) and the grid needs no host read-back.
//
// Why a kept pair lies in adjacent cells (u = 2^-24).  Let the brute predicate keep (x, y):
// d2 <= r2.  Every fma of sq_dist adds a square to the sum so far and rounding is monotone, so
// d2 >= fl(dx_a^2) for every axis, dx_a = fl(x_a - y_a): fl(dx_a^2) <= r2 = fl(r r).  A product
// is rounded with a relative error u, or, when it underflows, an absolute one of at most
// 2^-150: dx_a^2 <= r^2 (1 + u)^2 + 2^-149, so |dx_a| <= r (1 + u) + 2^-74.5; the subtraction
// has a relative error u (and none when it underflows), so
//   |x_a - y_a| <= rho = r (1 + 2^-22) + 2^-74.
// s0 is itself a rounded product, s0 >= r (1 + 2^-10) (1 - u), and s0 >= 2^-60.  For
// r >= 2^-63 the absolute term is at most r 2^-11, so rho / s0 <= (1 + 2^-11 + 2^-22) /
// ((1 + 2^-10) (1 - u)) < 1 - 2^-11 + 2^-19; for a smaller r, rho < 2^-62 and rho / s0 < 1 / 4.
// Now let a = x_a - lo_a >= b = y_a - lo_a >= 0 and t(x) = fl(fl(a) scale_a), the value whose
// truncation is the bin.  scale_a = fl(n_a / ext_a) <= (1 + u) / side_a with the real cell
// side side_a = ext_a / n_a >= s0 (1 - u): the quotient fl(ext_a / s0) may have rounded up to
// the integer n_a, and halving n_a only lengthens the side.  The subtraction and the product
// have a relative error u each (an underflowing product an absolute 2^-150), so
//   t(x) - t(y) <= (a - b) scale_a + (2 u + u^2) (a + b) scale_a + 2^-149
//               <= rho / s0 (1 + 3 u) + 4 u n_a (1 + 3 u) + 2^-149
//               <  (1 - 2^-11 + 2^-18) + 2^-12 (1 + 3 u)  <  1
// with a scale_a <= n_a (1 + u) and the cap n_a <= 1024, which is what the second term needs:
// 4 u 1024 = 2^-12.  So t(x) < t(y) + 1, the truncations differ by at most one, and the
// minimum with n_a - 1 keeps that.  A side of r (1 + 2^-10) with n_a <= 1024 closes the
// argument with a margin of 2^-12; a larger cap on n_a would need a wider side.  ext_a <=
// 2^100 keeps scale_a >= 2^-99 a normal number, and 2 s0 <= ext_a keeps it below 2^70.
//
// Search.  gnn_launch.h's mapping: wave64, 256-thread blocks, a sub-group of L lanes (8 / 16 /
// 32 / 64) per destination row, xcd_remap.  Rows are launched in cell order (sub-group k owns
// sorted position k), so neighbouring sub-groups read the same candidates from L2; results
// are stored under the original row id perm[k].  The last present axis is the fastest digit
// of the cell id, so the up to three cells (b_F - 1 .. b_F + 1) of a neighbouring cell row are
// one contiguous range of the sorted points: a row walks 3^(D-1) ranges (1 / 3 / 9), clipped
// at the grid's edges, each read as 16-byte loads of the gathered positions.  Inside a range
// lanes take the candidates t, t + L, ..; the predicate goes through a wave ballot cut to the
// sub-group, a kept candidate's slot is base + popcount(bits below my lane): the scheme of
// radius_kernel.  The loop conditions are ballots (every lane of the wave runs every step)
// and the range loop has a compile-time trip count, so all ballots sit in uniform control
// flow.  The scan order -- range after range, inside a range cell after cell, inside a cell
// ascending id (the sort is stable) -- is a function of the inputs alone.
//
// Row order.  The ids of a row are distinct, so the final slot of an entry is
// rowptr[i] + #{j' in the row : j' < j}.  cells_rows_kernel ranks each entry of the scratch
// row against the whole row (lane sl takes the entries e0 + sl, e0 + sl + L, ..; every lane of
// a sub-group reads the same j' at a time: one broadcast load) and stores col / d2 at the
// ranked slot.  Chosen over a k-way merge inside the fill: rows of a radius graph are short
// (tens of entries), the quadratic rank is then a few hundred cached compares, it has no
// capacity and no second code path -- any row length works -- and the fill stays the count
// pass with stores.  The cost is one scratch copy of the edge list.
//
// Bounds.  Every index read from a table is cut to its table: cell ids to [0, n + G), cell
// pointers to [0, n], perm to [0, n), graph ranges to [0, n], n_a to >= 1 and the cells of a
// graph to its id range.  The fill writes no slot at or past rowptr[i + 1] or the capacity
// `cap` of the edge buffers; the row pass writes only inside [rowptr[i], min(rowptr[i + 1],
// cap)), whatever the scratch list holds.
#include "cgnn_common.h"
#include "cgnn_api.h"
#include "gnn_launch.h"
#include "gnn_point.h"
#include <algorithm>
#include <cmath>

using namespace cgnn;
using namespace cgnn::geo;
using namespace cgnn::launch;

namespace {

constexpr int kChunk = 1024;                        // points per block of the first level
constexpr int kNaMax = 1024;                        // cells per axis: see the header's argument
constexpr float kSideFactor = 1.0009765625f;        // 1 + 2^-10
constexpr float kSideMin = 8.67361737988403547e-19f;   // 2^-60
constexpr float kExtMax = 1.2676506002282294e30f;   // 2^100

template <int D>
__device__ __forceinline__ bool finite_point(const Point<D>& p) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < D; ++c) ok = ok && fabsf(p.c[c]) < INFINITY;       // false for NaN
  return ok;
}

// min / max over the 256 threads of a block; the result is valid in thread 0
template <int D>
__device__ __forceinline__ void block_minmax(float (&mn)[D], float (&mx)[D], float* lds) {
#pragma unroll
  for (int c = 0; c < D; ++c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      mn[c] = fminf(mn[c], __shfl_xor(mn[c], off, 64));
      mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], off, 64));
    }
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < D; ++c) {
      lds[w * 8 + c] = mn[c];
      lds[w * 8 + 4 + c] = mx[c];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < 4; ++v) {
#pragma unroll
      for (int c = 0; c < D; ++c) {
        mn[c] = fminf(mn[c], lds[v * 8 + c]);
        mx[c] = fmaxf(mx[c], lds[v * 8 + 4 + c]);
      }
    }
  }
}

template <int D>
__device__ __forceinline__ void take_point(const float* __restrict__ pos, int j, int ldp, float (&mn)[D],
                                           float (&mx)[D]) {
  const Point<D> p = load_point<D>(pos, j, ldp);
  if (finite_point<D>(p)) {
#pragma unroll
    for (int c = 0; c < D; ++c) {
      mn[c] = fminf(mn[c], p.c[c]);
      mx[c] = fmaxf(mx[c], p.c[c]);
    }
  }
}

}  // namespace

// part [ceil(n / 1024), 8]: min (0..2) and max (4..6) of the finite points of each chunk
template <int D>
__global__ __launch_bounds__(256) void cells_part_kernel(const float* __restrict__ pos, float* __restrict__ part, int n,
                                                         int ldp) {
  __shared__ float lds[32];
  float mn[D], mx[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    mn[c] = INFINITY;
    mx[c] = -INFINITY;
  }
  const long j0 = (long)blockIdx.x * kChunk;
  const long j1 = min(j0 + kChunk, (long)n);
  for (long j = j0 + threadIdx.x; j < j1; j += 256) take_point<D>(pos, (int)j, ldp, mn, mx);
  block_minmax<D>(mn, mx, lds);
  if (threadIdx.x == 0) {
    float* o = part + (size_t)blockIdx.x * 8;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      o[c] = mn[c];
      o[4 + c] = mx[c];
    }
  }
}

// glo [G, 8] = lo[3], scale[3], 0, 0; gn [G, 4] = n_0, n_1, n_2, their product.  One block per
// graph: the chunks that lie inside the graph come from part, the points before and after
// them from pos.
template <int D>
__global__ __launch_bounds__(256) void cells_grid_kernel(const float* __restrict__ pos, const int* __restrict__ gptr,
                                                         const float* __restrict__ part, float* __restrict__ glo,
                                                         int* __restrict__ gn, int n, int ldp, float s0) {
  __shared__ float lds[32];
  const int g = blockIdx.x;
  const int g0 = min(max(gptr[g], 0), n);
  const int g1 = min(max(gptr[g + 1], g0), n);
  float mn[D], mx[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    mn[c] = INFINITY;
    mx[c] = -INFINITY;
  }
  const int c0 = g0 / kChunk + (g0 % kChunk != 0), c1 = g1 / kChunk;  // whole chunks [c0, c1)
  if (c0 < c1) {
    for (int j = g0 + threadIdx.x; j < c0 * kChunk; j += 256) take_point<D>(pos, j, ldp, mn, mx);
    for (int j = c1 * kChunk + threadIdx.x; j < g1; j += 256) take_point<D>(pos, j, ldp, mn, mx);
    for (int c = c0 + threadIdx.x; c < c1; c += 256) {
      const float* q = part + (size_t)c * 8;
#pragma unroll
      for (int a = 0; a < D; ++a) {
        mn[a] = fminf(mn[a], q[a]);
        mx[a] = fmaxf(mx[a], q[4 + a]);
      }
    }
  } else {
    for (int j = g0 + threadIdx.x; j < g1; j += 256) take_point<D>(pos, j, ldp, mn, mx);
  }
  block_minmax<D>(mn, mx, lds);
  if (threadIdx.x != 0) return;
  float lo[3] = {0.f, 0.f, 0.f}, ext[3] = {0.f, 0.f, 0.f};
  int na[3] = {1, 1, 1};
#pragma unroll
  for (int a = 0; a < D; ++a) {
    if (mn[a] <= mx[a]) {                           // the graph has a finite point
      lo[a] = mn[a];
      ext[a] = __fsub_rn(mx[a], mn[a]);             // +inf when it overflows
      if (ext[a] > 0.f && ext[a] <= kExtMax) {
        const int q = (int)fminf(__fdiv_rn(ext[a], s0), (float)kNaMax);
        if (q >= 2) na[a] = q;
      }
    }
  }
  const long cap = max(g1 - g0, 1);
  while ((long)na[0] * na[1] * na[2] > cap) {
    int a = 0;
    if (na[1] > na[a]) a = 1;
    if (na[2] > na[a]) a = 2;
    na[a] = (na[a] + 1) >> 1;
  }
  float* o = glo + (size_t)g * 8;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o[a] = lo[a];
    o[3 + a] = na[a] >= 2 ? __fdiv_rn((float)na[a], ext[a]) : 0.f;
    gn[(size_t)g * 4 + a] = na[a];
  }
  o[6] = o[7] = 0.f;
  gn[(size_t)g * 4 + 3] = na[0] * na[1] * na[2];
}

// cell_id [n]: the global cell of each point, or the sentinel n + G (see the header)
template <int D>
__global__ __launch_bounds__(256) void cells_bin_kernel(const float* __restrict__ pos, const int* __restrict__ gptr,
                                                        const int* __restrict__ seg_id, const float* __restrict__ glo,
                                                        const int* __restrict__ gn, int* __restrict__ cell_id, int n,
                                                        int G, int ldp) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int i = (int)t;
  int cell = n + G;
  const int s = seg_id[i];
  if (s >= 0 && s < G) {
    const int g0 = min(max(gptr[s], 0), n);
    const int g1 = min(max(gptr[s + 1], g0), n);
    const Point<D> p = load_point<D>(pos, i, ldp);
    if (i >= g0 && i < g1 && finite_point<D>(p)) {
      const float* q = glo + (size_t)s * 8;
      int idx = 0;
#pragma unroll
      for (int a = 0; a < D; ++a) {
        const int na = min(max(gn[(size_t)s * 4 + a], 1), kNaMax);
        const float v = __fmul_rn(__fsub_rn(p.c[a], q[a]), q[3 + a]);
        const int b = min(max((int)fminf(v, (float)kNaMax), 0), na - 1);
        idx = idx * na + b;
      }
      cell = g0 + s + min(idx, g1 - g0 - 1);        // at most max(1, n_g) cells: inside the id range
    }
  }
  cell_id[i] = cell;
}

// spos [n, 4]: the positions in cell order; perm [n]: the point at each sorted position; scell
// [n]: its cell; cptr [n + G + 2]: the sorted positions of each cell.  FILL = false: out = deg
// [n].  FILL = true: out = the scratch ids and dout their d2, at rowptr[i] ... in scan order.
template <int L, int D, bool FILL>
__global__ __launch_bounds__(256) void cells_search_kernel(const float4* __restrict__ spos,
                                                           const int* __restrict__ perm,
                                                           const int* __restrict__ scell,
                                                           const int* __restrict__ cptr, const int* __restrict__ gptr,
                                                           const int* __restrict__ seg_id, const int* __restrict__ gn,
                                                           const int* __restrict__ rowptr, int* __restrict__ out,
                                                           float* __restrict__ dout, int n, int G, float r2, int loop,
                                                           int cap) {
  int sub, sl;
  const long row = sub_row<L>(sub, sl);
  const int k = row < n ? (int)row : 0;
  int i = row < n ? perm[k] : -1;
  if (i >= n) i = -1;
  const bool rv = i >= 0;                           // a row to answer for
  bool act = false;                                 // a row with cells to scan
  int cb = 0, b[3] = {0, 0, 0}, na[3] = {1, 1, 1};
  if (rv) {
    const int c = scell[k];
    const int s = seg_id[i];
    if (c >= 0 && c < n + G && s >= 0 && s < G) {
      cb = min(max(gptr[s], 0), n) + s;
#pragma unroll
      for (int a = 0; a < D; ++a) na[a] = min(max(gn[(size_t)s * 4 + a], 1), kNaMax);
      const long nc = (long)na[0] * na[1] * na[2];
      const int l = c - cb;
      if (l >= 0 && l < nc && cb + nc <= (long)n + G) {
        act = true;
        if (D == 1) {
          b[0] = l;
        } else if (D == 2) {
          b[0] = l / na[1];
          b[1] = l - b[0] * na[1];
        } else {
          const int t = l / na[2];
          b[2] = l - t * na[2];
          b[0] = t / na[1];
          b[1] = t - b[0] * na[1];
        }
      }
    }
  }
  Point<D> pi;
#pragma unroll
  for (int c = 0; c < D; ++c) pi.c[c] = 0.f;
  if (act) {
    const float4 v = spos[k];
    pi.c[0] = v.x;
    if (D > 1) pi.c[D > 1 ? 1 : 0] = v.y;
    if (D > 2) pi.c[D > 2 ? 2 : 0] = v.z;
  }
  int base = 0, end = 0;
  if (FILL && rv) {
    base = rowptr[i];
    end = min(rowptr[i + 1], cap);
  }
  constexpr unsigned long long kGroup = L == 64 ? ~0ull : (1ull << (L & 63)) - 1ull;
  constexpr int F = D - 1;                          // the fastest axis of the cell id
  constexpr int NQ = D == 3 ? 9 : D == 2 ? 3 : 1;   // neighbouring cell rows
  const int shift = sub * L;
  const int flo = max(b[F] - 1, 0), fhi = min(b[F] + 1, na[F] - 1);
#pragma unroll 1
  for (int q = 0; q < NQ; ++q) {
    int j0 = 0, j1 = 0;
    if (act) {
      const int d0 = D == 3 ? q / 3 - 1 : D == 2 ? q - 1 : 0;
      const int d1 = D == 3 ? q - (q / 3) * 3 - 1 : 0;
      const int a0 = b[0] + d0, a1 = b[1] + d1;     // the outer digits (D = 1: unused)
      bool ok = true;
      int R = 0;
      if (D == 2) {
        ok = a0 >= 0 && a0 < na[0];
        R = a0;
      } else if (D == 3) {
        ok = a0 >= 0 && a0 < na[0] && a1 >= 0 && a1 < na[1];
        R = a0 * na[1] + a1;
      }
      if (ok) {
        const int c = cb + R * na[F];
        j0 = min(max(cptr[c + flo], 0), n);
        j1 = min(max(cptr[c + fhi + 1], 0), n);
      }
    }
    // the condition is wave-uniform: all 64 lanes run every step, finished sub-groups idle
    for (; __builtin_amdgcn_ballot_w64(j0 < j1) != 0ull; j0 += L) {
      const int kk = j0 + sl;
      float d = 0.f;
      bool keep = false;
      if (kk < j1) {
        const float4 v = spos[kk];
        Point<D> pj;
        pj.c[0] = v.x;
        if (D > 1) pj.c[D > 1 ? 1 : 0] = v.y;
        if (D > 2) pj.c[D > 2 ? 2 : 0] = v.z;
        d = sq_dist<D>(pi, pj);
        keep = d <= r2 && (loop || kk != k);        // a NaN distance compares false
      }
      const unsigned long long m = (__builtin_amdgcn_ballot_w64(keep) >> shift) & kGroup;
      if (FILL) {
        const int slot = base + __popcll(m & ((1ull << sl) - 1ull));
        if (keep && slot < end) {
          out[slot] = perm[kk];
          dout[slot] = d;
        }
      }
      base += __popcll(m);
    }
  }
  if (!FILL && rv && sl == 0) out[i] = base;
}

// col (and d2, which may be null) [rowptr[i], rowptr[i + 1]) = the scratch row in ascending id
template <int L>
__global__ __launch_bounds__(256) void cells_rows_kernel(const int* __restrict__ rowptr, const int* __restrict__ sj,
                                                         const float* __restrict__ sd, int* __restrict__ col,
                                                         float* __restrict__ d2, int n, int cap) {
  int sub, sl;
  const long row = sub_row<L>(sub, sl);
  if (row >= n) return;                             // no cross-lane traffic below
  const int i = (int)row;
  const int e0 = max(rowptr[i], 0), e1 = min(rowptr[i + 1], cap);
  for (int e = e0 + sl; e < e1; e += L) {
    const int j = sj[e];
    int rank = 0;
#pragma unroll 4
    for (int f = e0; f < e1; ++f) rank += sj[f] < j ? 1 : 0;
    const int slot = e0 + min(rank, e1 - e0 - 1);
    col[slot] = j;
    if (d2) d2[slot] = sd[e];
  }
}

// ---------------------------------------------------------------- launchers

namespace {

template <class Fn>
int with_d(int D, Fn&& fn) {
  if (D == 1) return fn(Const<1>{});
  if (D == 2) return fn(Const<2>{});
  return fn(Const<3>{});
}

template <class Fn>
int with_l(int L, Fn&& fn) {
  if (L == 8) return fn(Const<8>{});
  if (L == 16) return fn(Const<16>{});
  if (L == 32) return fn(Const<32>{});
  return fn(Const<64>{});
}

bool cells_shape_ok(int D, int lanes) {
  return D >= 1 && D <= 3 && (lanes == 0 || lanes == 8 || lanes == 16 || lanes == 32 || lanes == 64);
}

// blocks of rpb rows for n rows, or 0 when the launch would count its threads past 32 bits
unsigned cells_blocks(long n, long rpb) {
  const long b = (n + rpb - 1) / rpb;
  return b > (1L << 24) - 1 ? 0u : (unsigned)b;
}

bool radius_ok(float r) { return r >= 0.f && std::isfinite(r); }

// The default sub-group width of the search: a row walks ranges of up to three cells, a few
// to a few tens of candidates each, whatever the size of the cloud (docs/PERF.md, "Cell
// lists").
constexpr int kSearchLanes = 8;

}  // namespace

// floats of the `part` scratch of gnn_launch_cells_grid for n points
extern "C" int gnn_cells_grid_floats(int n) { return n <= 0 ? 0 : (int)(8 * (((long)n + kChunk - 1) / kChunk)); }

// glo [G, 8] / gn [G, 4]: the grid of every graph (see the header) from pos [n, ldp], gptr
// [G + 1] and r; part: gnn_cells_grid_floats(n) floats of scratch.  Two launches, no
// allocation and no synchronisation.  With n <= 0 nothing is launched and glo / gn are left
// to the caller.  Return codes: see cgnn_api.h.
extern "C" int gnn_launch_cells_grid(const float* pos, const int* gptr, float* part, float* glo, int* gn, int n,
                                     int G, int D, int ldp, float r, hipStream_t st) {
  if (!cells_shape_ok(D, 0)) return -1;
  if (ldp < D || !radius_ok(r)) return -3;
  if (n <= 0) return 0;
  if (!pos || !gptr || !part || !glo || !gn || G < 1) return -3;
  if (G > (1 << 24) - 1) return -4;
  const unsigned chunks = (unsigned)(((long)n + kChunk - 1) / kChunk);
  const float s0 = std::max(r * kSideFactor, kSideMin);
  return with_d(D, [&](auto d) {
    constexpr int DD = decltype(d)::value;
    hipLaunchKernelGGL((cells_part_kernel<DD>), dim3(chunks), dim3(256), 0, st, pos, part, n, ldp);
    hipLaunchKernelGGL((cells_grid_kernel<DD>), dim3((unsigned)G), dim3(256), 0, st, pos, gptr, (const float*)part,
                       glo, gn, n, ldp, s0);
    return (int)hipGetLastError();
  });
}

// cell_id [n] from the grid tables of gnn_launch_cells_grid.  Capturable.
extern "C" int gnn_launch_cells_bin(const float* pos, const int* gptr, const int* seg_id, const float* glo,
                                    const int* gn, int* cell_id, int n, int G, int D, int ldp, hipStream_t st) {
  if (!cells_shape_ok(D, 0)) return -1;
  if (ldp < D) return -3;
  if (n <= 0) return 0;
  if (!pos || !gptr || !seg_id || !glo || !gn || !cell_id || G < 1) return -3;
  const unsigned grid = cells_blocks(n, 256);
  if (!grid) return -4;
  return with_d(D, [&](auto d) {
    hipLaunchKernelGGL((cells_bin_kernel<decltype(d)::value>), dim3(grid), dim3(256), 0, st, pos, gptr, seg_id, glo,
                       gn, cell_id, n, G, ldp);
    return (int)hipGetLastError();
  });
}

// deg [n] (under the original row ids) of the radius graph, from the points in cell order:
// spos [n, 4] (ldp must be 4: 16-byte loads), perm / scell [n], cptr [n + G + 2].  lanes: 0 =
// the default width, or one of 8 / 16 / 32 / 64.  Capturable.
extern "C" int gnn_launch_cells_count(const float* spos, const int* perm, const int* scell, const int* cptr,
                                      const int* gptr, const int* seg_id, const int* gn, int* deg, int n, int G,
                                      int D, int ldp, float r, int loop, int lanes, hipStream_t st) {
  if (!cells_shape_ok(D, lanes)) return -1;
  if (ldp != 4 || !radius_ok(r)) return -3;
  if (n <= 0) return 0;
  if (!spos || !perm || !scell || !cptr || !gptr || !seg_id || !gn || !deg || G < 1) return -3;
  const int L = lanes ? lanes : kSearchLanes;
  const unsigned grid = cells_blocks(n, 4 * (64 / L));
  if (!grid) return -4;
  const float r2 = r * r;
  return with_l(L, [&](auto l) {
    return with_d(D, [&](auto d) {
      hipLaunchKernelGGL((cells_search_kernel<decltype(l)::value, decltype(d)::value, false>), dim3(grid), dim3(256),
                         0, st, (const float4*)spos, perm, scell, cptr, gptr, seg_id, gn, (const int*)nullptr, deg,
                         (float*)nullptr, n, G, r2, loop, 0);
      return (int)hipGetLastError();
    });
  });
}

// the rows in scan order: sj / sd [cap] at rowptr[i] .. rowptr[i + 1], rowptr [n + 1] the
// exclusive sum of the count pass's deg; nothing is written at or past cap.  Capturable.
extern "C" int gnn_launch_cells_fill(const float* spos, const int* perm, const int* scell, const int* cptr,
                                     const int* gptr, const int* seg_id, const int* gn, const int* rowptr, int* sj,
                                     float* sd, int n, int G, int D, int ldp, float r, int loop, int lanes, int cap,
                                     hipStream_t st) {
  if (!cells_shape_ok(D, lanes)) return -1;
  if (ldp != 4 || !radius_ok(r) || cap < 0) return -3;
  if (n <= 0 || cap == 0) return 0;
  if (!spos || !perm || !scell || !cptr || !gptr || !seg_id || !gn || !rowptr || !sj || !sd || G < 1) return -3;
  const int L = lanes ? lanes : kSearchLanes;
  const unsigned grid = cells_blocks(n, 4 * (64 / L));
  if (!grid) return -4;
  const float r2 = r * r;
  return with_l(L, [&](auto l) {
    return with_d(D, [&](auto d) {
      hipLaunchKernelGGL((cells_search_kernel<decltype(l)::value, decltype(d)::value, true>), dim3(grid), dim3(256),
                         0, st, (const float4*)spos, perm, scell, cptr, gptr, seg_id, gn, rowptr, sj, sd, n, G, r2,
                         loop, cap);
      return (int)hipGetLastError();
    });
  });
}

// col (and d2, which may be null) [cap]: every row of the scratch list sj / sd in ascending
// source id.  lanes: 0 = from cap / n.  Capturable.
extern "C" int gnn_launch_cells_rows(const int* rowptr, const int* sj, const float* sd, int* col, float* d2, int n,
                                     int cap, int lanes, hipStream_t st) {
  if (!cells_shape_ok(1, lanes)) return -1;
  if (cap < 0) return -3;
  if (n <= 0 || cap == 0) return 0;
  if (!rowptr || !sj || !sd || !col) return -3;
  int L = lanes;
  if (!L) L = cap <= 16L * n ? 8 : cap <= 32L * n ? 16 : cap <= 64L * n ? 32 : 64;
  const unsigned grid = cells_blocks(n, 4 * (64 / L));
  if (!grid) return -4;
  return with_l(L, [&](auto l) {
    hipLaunchKernelGGL((cells_rows_kernel<decltype(l)::value>), dim3(grid), dim3(256), 0, st, rowptr, sj, sd, col, d2,
                       n, cap);
    return (int)hipGetLastError();
  });
}
