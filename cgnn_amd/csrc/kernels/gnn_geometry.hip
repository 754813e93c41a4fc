// GNN track (beyond the reference): graphs from positions for MI355X -- the radius-graph
// and k-nearest-neighbour searches over a batch of point sets, the squared pair distances of a
// CSR's edges and their gradient with respect to the positions.
//
//   radius_count_kernel  deg[i]  = #{ j in graph(i) : d2(i, j) <= r2, j != i unless loop }
//   radius_fill_kernel   col[rowptr[i] ..] = those j in ascending order, d2[..] their d2(i, j)
//   knn_select_kernel    deg[i]  = min(k, #candidates of i), (tau_d2, tau_j)[i] = the k-th key
//   knn_fill_kernel      col[rowptr[i] ..] = the candidates with key <= tau, ascending j, and d2
//   pair_d2_kernel       d2[e]   = d2(i, col[e])  for the edges e of row i of any CSR
//   pair_d2_bwd_kernel   dpos[i] = 2 ( sum_{e in in(i)}  g[e] (p_i - p_src(e))
//                                    + sum_{e in out(i)} g[e] (p_i - p_dst(e)) )
//   radius_pbc_kernel    the radius search over the lattice images of a periodic cell: deg, or
//                        col / shift / d2 in ascending (j, image)
//   pair_d2_pbc_kernel, pair_d2_pbc_bwd_kernel   pair_d2 / pair_d2_bwd with the image offsets
//
// Positions are fp32 [n, ldp] with D coordinates per point, 1 <= D <= 3, ldp >= D; the columns
// D <= c < ldp are never read.  graph(i) = [gptr[seg_id[i]], gptr[seg_id[i] + 1]) (gptr int32
// [G + 1], seg_id int32 [n]: GraphBatch.gptr / .batch).
//
// The squared distance, one definition for every kernel of this file and of gnn_cells.hip
// (sq_dist, gnn_point.h):
//   dx = p_i[0] - p_j[0], dy = p_i[1] - p_j[1], dz = p_i[2] - p_j[2]     each one fp32 subtract
//   d2 = fma(dz, dz, fma(dy, dy, dx * dx))                                explicit, no contraction
// with the terms of absent coordinates dropped (D = 2: fma(dy, dy, dx * dx); D = 1: dx * dx).
// i is the row (the destination), j the column (the source).
//
// Contract of the search.  r2 = r * r is one fp32 product, made on the host.  The boundary is
// inclusive (d2 <= r2); a NaN d2 is not an edge (the compare is false); coincident points are
// neighbours.  The search is brute force inside each graph, O(n_g^2): the algorithm for
// molecules and other graphs of up to a few thousand points.  Large point clouds: the
// cell-list search of gnn_cells.hip, which returns this file's CSR bit for bit (radius search
// only, no periodic cells, no k-NN or neighbour cap there).  No k-NN in
// feature space (D > 3); periodic cells: the radius search only ("Periodic cells" below), no
// k-NN or neighbour cap over images, no gradient with respect to the cell.
//
// Contract of the k-NN search (the neighbour cap of the radius search is the same thing).  The
// candidates of row i are the j of its graph with j != i unless loop, a finite d2(i, j) (not
// NaN, not inf) and d2(i, j) <= r2; r = +inf means no radius (r2 = +inf: only the finiteness
// test is left).  Row i keeps the min(k, #candidates) candidates with the smallest key
// (d2, j), lexicographic, d2 compared as fp32: equal distances go to the lower id.  Keys are
// distinct, so the kept set is a function of pos, gptr and seg_id alone.  The kept neighbours
// are stored in ascending source id, like the radius fill, not in distance order: a row of
// knn(k, r) is a subset of the row of radius(r) and bit-equal to it when that has at most k
// entries.  1 <= k <= 64.  The result is in general a directed graph.
//
// Mapping (gnn_launch.h's blocks): wave64, 256-thread blocks, a sub-group of L lanes (8 / 16 /
// 32 / 64) owns one destination i and loads p_i once.  Lane sl takes the candidates
// j = g0 + sl, g0 + sl + L, ...: coalesced loads.  The predicate goes through a wave ballot cut
// to the sub-group's L bits; a kept candidate's slot is base + popcount(bits below my lane),
// and base advances by the popcount of the sub-group's bits.  That is the ascending order, and
// the same code is both passes (FILL = false counts, FILL = true writes).  The loop condition
// is itself a ballot, so that every lane of the wave runs every step and the ballots sit in
// uniform control flow.  The CSR is therefore a function of the positions, gptr and seg_id
// alone: the same for every L, grid and run.  No atomics.  A graph's rows, written with ids
// relative to gptr[g], do not depend on where the graph stands in the batch.
//
// knn_select_kernel: the same stream of candidates.  The sub-group holds its best keys
// sorted, one per lane (k <= L; empty slots are (+inf, INT_MAX), which every candidate beats).
// After the distance step the lanes whose candidate beats the row's current worst (the key of
// lane k - 1) are pending; they are inserted one at a time, lowest lane first: the key is
// broadcast, its rank is the popcount of the ballot "held key < new key" cut to the
// sub-group, the lanes above the rank take their lower neighbour's key and the lane at the
// rank the new one.  Before each insertion the pending lanes are tested against the new
// worst, so after the first k candidates few remain: the distance pass plus about
// k ln(n_g / k) insertions per row.  Both loops run while a ballot over the whole wave says
// that some sub-group has work, so every ballot and shuffle sits in wave-uniform control
// flow.  Row i gets deg[i], and its threshold, the largest kept key: tau_d2[i] / tau_j[i], or
// (-1, -1) for a row that keeps nothing (no d2 is <= -1).  No LDS, no atomics.
//
// knn_fill_kernel: the loop of the radius fill with the predicate "key <= tau" (a NaN
// distance compares false, +inf is above every tau, a d2 beyond r2 is above it too) and the
// same ballot / popcount slots: ascending ids, nothing at or past rowptr[i + 1].  It takes no
// k and no r, and any sub-group width whatever width selected.
//
// Bounds.  A seg_id outside [0, G) makes its row empty; graph ranges are cut to [0, n]; the
// fill pass writes no slot at or past rowptr[i + 1], so a rowptr that does not come from the
// count pass loses edges but writes nothing out of its rows.
//
// pair_d2_kernel: a sub-group owns row i, lane sl the edges e0 + sl, e0 + sl + L, ...  On a
// radius graph it reproduces the fill pass's d2 bit for bit (the same sq_dist(p_i, p_j)).
//
// pair_d2_bwd_kernel: a sub-group owns node i.  In-edges come from the CSR row (rowptr, col),
// out-edges from the transposed CSR (rowptr_t, col_t, eperm_t: transposed edge t is CSR edge
// eperm_t[t], and col_t[t] is its destination).  Order of the sum, per coordinate, fp32:
// lane sl starts from 0 and takes acc = fma(g[e], p_i - p_other, acc) over the in-edges
// e0 + sl, e0 + sl + L, ... in that order, then over the out-edges t0 + sl, t0 + sl + L, ...
// in that order; the L lane sums are combined by an xor butterfly (distances 1, 2, ... L / 2;
// both partners of a step compute the same commutative sum); one product with 2 at the end.
// The tree is a fixed function of the two degrees and L.  A self loop appears in both lists
// and contributes 0 twice.  Columns D <= c < ldp of dpos are written 0; a node without edges
// gets 0.  No atomics.
//
// Periodic cells (radius_pbc_kernel, pair_d2_pbc_kernel, pair_d2_pbc_bwd_kernel): one contract
// for the kernels, the CPU branches of ops.py and the tests.
//   Inputs.  Graph g has a cell C_g: fp32, row-major [G, 9], row a = lattice vector a; only the
//   leading D x D block is read.  It has image ranges nimg_g: int32 [G, 3], each in
//   0 .. PBC_NIMG_MAX (= 7), 0 = the axis is not periodic.  The kernels clamp what they read
//   to that range, so a bad table cannot make the loops run away (the Python layer never
//   passes one).
//   Candidates.  The candidates of row i are the pairs (j, s): j over the graph of i, s over
//   the box -nimg[a] <= s_a <= nimg[a], a < D.  (j, s) is kept when d2(i, j, s) <= r2; without
//   loop (j, s) = (i, 0) is left out.  (i, s != 0) is a real edge: an atom sees its own images.
//   Distance, fp32, explicit, no contraction:
//     off[c] = fma(s2, C[2][c], fma(s1, C[1][c], s0 * C[0][c]))   terms of absent axes (a >= D)
//                                                                 dropped, s_a converted to float
//     q[c]   = p_j[c] + off[c]                                    one fp32 add
//     d2     = sq_dist(p_i, q)                                    as above
//   With s = 0 this gives off = 0 and q = p_j: with nimg all zero the result is the radius
//   graph's bit for bit (finite cells).
//   Order.  Row i is stored in ascending (j, m), m the index of the image in lexicographic
//   order of (s0, s1, s2), s2 fastest, each from -nimg to +nimg.  The CSR is a function of
//   pos, gptr, seg_id, cell and nimg alone: the same for every sub-group width, grid and run.
//   No atomics.  A NaN distance is no edge; the boundary is inclusive.
//   Output.  col, optionally d2, and shift: int32 [nnz], byte a = s_a as a two's-complement
//   int8, byte 3 = 0, so 0 is the home image.  Written with ordinary vector stores.
//   Symmetry.  For finite inputs (i, j, s) is an edge iff (j, i, -s) is.
// Mapping of the search: the radius kernel's, over the flattened candidates
// t = (j - g0) * M + m, M the number of images of the graph: lane sl takes t = sl, sl + L, ...,
// so a cell of 2 atoms and 343 images fills its lanes, and the ballot / popcount slots give
// the (j, m) order as they give the j order there.  t is never formed: a lane keeps its
// candidate as the digits (j - g0, s0 + nimg0, .., s_{D-1} + nimg_{D-1}) of a mixed-radix
// number and adds the digits of L with carries each step -- D compares and subtracts, no
// division in the loop; the digits of sl and L come from one small division per axis before
// it.  A lane whose j has passed the end of the graph stops advancing.  The loop condition is
// a wave ballot, as above.
// pair_d2_pbc_kernel: pair_d2_kernel with q = p_col[e] + off_e, off_e from shift[e] (any int8
// values) and the cell of seg_id[i] (zeros for a seg_id outside [0, G)): on a periodic radius
// graph the fill pass's d2 bit for bit.  pair_d2_pbc_bwd_kernel: pair_d2_bwd_kernel with
// acc = fma(g[e], p_i - (p_j + off_e), acc) over the in-edges and
// acc = fma(g[e], p_i - (p_k - off_e), acc) over the out-edges t, off_e of CSR edge
// e = eperm_t[t]; lane order, butterfly and the final product with 2 as there.  The gradient
// goes to the positions only.  Both loops take the cell of seg_id[i], the node the sub-group
// owns; an edge's offset is defined by the cell of its destination row, so the out-edge loop
// is right only when the two ends of every edge have the same seg_id: the CSR must be block
// diagonal over the graphs, as every GraphBatch is.  pair_d2_pbc_kernel has no such limit.
#include "cgnn_common.h"
#include "cgnn_api.h"
#include "gnn_launch.h"
#include "gnn_point.h"
#include <algorithm>
#include <climits>
#include <cmath>

using namespace cgnn;
using namespace cgnn::geo;
using namespace cgnn::launch;

namespace {

// Point, load_point, sq_dist, sub_row: gnn_point.h, shared with gnn_cells.hip

template <int L>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int d = 1; d < L; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// ---- periodic cells (see the header: "Periodic cells")

constexpr int kPbcNimgMax = 7;                      // ops.PBC_NIMG_MAX

template <int D>
struct Cell {
  float v[D][D];                                    // v[a]: lattice vector a
};

template <int D>
__device__ __forceinline__ Cell<D> zero_cell() {
  Cell<D> C;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int c = 0; c < D; ++c) C.v[a][c] = 0.f;
  return C;
}

// the leading D x D block of graph g's row-major 3 x 3 cell
template <int D>
__device__ __forceinline__ Cell<D> load_cell(const float* __restrict__ cell, int g) {
  Cell<D> C;
  const float* q = cell + (size_t)g * 9;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int c = 0; c < D; ++c) C.v[a][c] = q[a * 3 + c];
  return C;
}

// the cell of row i's graph, or zeros (every offset 0) for a seg_id outside [0, G)
template <int D>
__device__ __forceinline__ Cell<D> cell_of_row(const float* __restrict__ cell, const int* __restrict__ seg_id, int i,
                                               int G) {
  const int s = seg_id[i];
  return s >= 0 && s < G ? load_cell<D>(cell, s) : zero_cell<D>();
}

// off[c] = fma(s2, C[2][c], fma(s1, C[1][c], s0 * C[0][c])), the terms of absent axes dropped
template <int D>
__device__ __forceinline__ Point<D> image_offset(const Cell<D>& C, const int (&s)[D]) {
  Point<D> off;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    float o = __fmul_rn((float)s[0], C.v[0][c]);
    if constexpr (D > 1) o = __fmaf_rn((float)s[1], C.v[1][c], o);
    if constexpr (D > 2) o = __fmaf_rn((float)s[2], C.v[2][c], o);
    off.c[c] = o;
  }
  return off;
}

// q = p + off, one fp32 add per coordinate
template <int D>
__device__ __forceinline__ Point<D> image_point(const Point<D>& p, const Point<D>& off) {
  Point<D> q;
#pragma unroll
  for (int c = 0; c < D; ++c) q.c[c] = __fadd_rn(p.c[c], off.c[c]);
  return q;
}

// byte a = s[a] as a two's-complement int8, byte 3 (and the bytes of absent axes) 0
template <int D>
__device__ __forceinline__ int pack_shift(const int (&s)[D]) {
  unsigned w = 0u;
#pragma unroll
  for (int a = 0; a < D; ++a) w |= ((unsigned)s[a] & 0xffu) << (8 * a);
  return (int)w;
}

template <int D>
__device__ __forceinline__ void unpack_shift(int w, int (&s)[D]) {
#pragma unroll
  for (int a = 0; a < D; ++a) s[a] = (int)(signed char)(((unsigned)w >> (8 * a)) & 0xffu);
}

// x / d for 0 <= x <= 64 and 1 <= d <= 15 without an integer division: (x + 0.5) / d is at
// least 0.5 / 15 away from every integer, the fast quotient of a value below 65 within 2^-16
__device__ __forceinline__ int small_div(int x, int d) { return (int)__fdividef((float)x + 0.5f, (float)d); }

}  // namespace

// FILL = false: out = deg [n].  FILL = true: out = col, written at rowptr[i] ...; d2 may be null.
template <int L, int D, bool FILL>
__global__ __launch_bounds__(256) void radius_kernel(const float* __restrict__ pos, const int* __restrict__ gptr,
                                                     const int* __restrict__ seg_id, const int* __restrict__ rowptr,
                                                     int* __restrict__ out, float* __restrict__ d2out, int n, int G,
                                                     int ldp, float r2, int loop) {
  int sub, sl;
  const long row = sub_row<L>(sub, sl);
  const bool rv = row < n;
  const int i = rv ? (int)row : 0;
  int g0 = 0, g1 = 0;
  if (rv) {
    const int s = seg_id[i];
    if (s >= 0 && s < G) {
      g0 = max(gptr[s], 0);
      g1 = min(gptr[s + 1], n);
    }
  }
  Point<D> pi;
#pragma unroll
  for (int c = 0; c < D; ++c) pi.c[c] = 0.f;
  if (g0 < g1) pi = load_point<D>(pos, i, ldp);
  int base = 0, end = 0;
  if (FILL && rv) {
    base = rowptr[i];
    end = rowptr[i + 1];
  }
  constexpr unsigned long long kGroup = L == 64 ? ~0ull : (1ull << (L & 63)) - 1ull;
  const int shift = sub * L;
  // the condition is wave-uniform: all 64 lanes run every step, finished sub-groups idle
  for (int j0 = g0; __builtin_amdgcn_ballot_w64(j0 < g1) != 0ull; j0 += L) {
    const int j = j0 + sl;
    const bool ok = j < g1;
    float d = 0.f;
    bool keep = false;
    if (ok) {
      const Point<D> pj = load_point<D>(pos, j, ldp);
      d = sq_dist<D>(pi, pj);
      keep = d <= r2 && (loop || j != i);           // a NaN distance compares false
    }
    const unsigned long long m = (__builtin_amdgcn_ballot_w64(keep) >> shift) & kGroup;
    if (FILL) {
      const int slot = base + __popcll(m & ((1ull << sl) - 1ull));
      if (keep && slot < end) {
        out[slot] = j;
        if (d2out) d2out[slot] = d;
      }
    }
    base += __popcll(m);
  }
  if (!FILL && rv && sl == 0) out[i] = base;
}

// (d, j) < (e, l), lexicographic; false when a distance is NaN
__device__ __forceinline__ bool key_less(float d, int j, float e, int l) { return d < e || (d == e && j < l); }

// deg [n], tau_d2 [n], tau_j [n]: see the header.  1 <= k <= L.
template <int L, int D>
__global__ __launch_bounds__(256) void knn_select_kernel(const float* __restrict__ pos, const int* __restrict__ gptr,
                                                         const int* __restrict__ seg_id, int* __restrict__ deg,
                                                         float* __restrict__ tau_d2, int* __restrict__ tau_j, int n,
                                                         int G, int ldp, int k, float r2, int loop) {
  int sub, sl;
  const long row = sub_row<L>(sub, sl);
  const bool rv = row < n;
  const int i = rv ? (int)row : 0;
  int g0 = 0, g1 = 0;
  if (rv) {
    const int s = seg_id[i];
    if (s >= 0 && s < G) {
      g0 = max(gptr[s], 0);
      g1 = min(gptr[s + 1], n);
    }
  }
  Point<D> pi;
#pragma unroll
  for (int c = 0; c < D; ++c) pi.c[c] = 0.f;
  if (g0 < g1) pi = load_point<D>(pos, i, ldp);
  constexpr unsigned long long kGroup = L == 64 ? ~0ull : (1ull << (L & 63)) - 1ull;
  const int shift = sub * L;
  const int worst = shift + k - 1;                  // the lane of the sub-group's k-th key
  float hd = INFINITY;                              // held key of sorted position sl
  int hj = INT_MAX;
  int cnt = 0;                                      // candidates seen
  // both conditions are wave-uniform: all 64 lanes run every step, finished sub-groups idle
  for (int j0 = g0; __builtin_amdgcn_ballot_w64(j0 < g1) != 0ull; j0 += L) {
    const int j = j0 + sl;
    float d = 0.f;
    bool pend = false;
    if (j < g1) {
      const Point<D> pj = load_point<D>(pos, j, ldp);
      d = sq_dist<D>(pi, pj);
      pend = d < INFINITY && d <= r2 && (loop || j != i);     // a NaN distance compares false
    }
    cnt += __popcll((__builtin_amdgcn_ballot_w64(pend) >> shift) & kGroup);
    for (;;) {
      const float wd = __shfl(hd, worst, 64);       // outside the &&: every lane takes part
      const int wj = __shfl(hj, worst, 64);
      pend = pend && key_less(d, j, wd, wj);
      const unsigned long long all = __builtin_amdgcn_ballot_w64(pend);
      if (all == 0ull) break;
      const unsigned long long m = (all >> shift) & kGroup;
      const int src = m ? __builtin_ctzll(m) : 0;   // the sub-group's lowest pending lane
      const float nd = __shfl(d, shift + src, 64);
      const int nj = __shfl(j, shift + src, 64);
      const int rank = __popcll((__builtin_amdgcn_ballot_w64(key_less(hd, hj, nd, nj)) >> shift) & kGroup);
      const float ud = __shfl_up(hd, 1, 64);
      const int uj = __shfl_up(hj, 1, 64);
      if (m) {                                      // rank <= k - 1 < L: the new key beat the worst
        if (sl > rank) {
          hd = ud;
          hj = uj;
        } else if (sl == rank) {
          hd = nd;
          hj = nj;
        }
        if (sl == src) pend = false;
      }
    }
  }
  const int kept = min(cnt, k);
  const int last = shift + max(kept - 1, 0);
  const float td = __shfl(hd, last, 64);
  const int tj = __shfl(hj, last, 64);
  if (rv && sl == 0) {
    deg[i] = kept;
    tau_d2[i] = kept ? td : -1.f;
    tau_j[i] = kept ? tj : -1;
  }
}

// col (and d2, which may be null) of the rows selected by knn_select_kernel
template <int L, int D>
__global__ __launch_bounds__(256) void knn_fill_kernel(const float* __restrict__ pos, const int* __restrict__ gptr,
                                                       const int* __restrict__ seg_id, const int* __restrict__ rowptr,
                                                       const float* __restrict__ tau_d2, const int* __restrict__ tau_j,
                                                       int* __restrict__ out, float* __restrict__ d2out, int n, int G,
                                                       int ldp, int loop) {
  int sub, sl;
  const long row = sub_row<L>(sub, sl);
  const bool rv = row < n;
  const int i = rv ? (int)row : 0;
  int g0 = 0, g1 = 0;
  if (rv) {
    const int s = seg_id[i];
    if (s >= 0 && s < G) {
      g0 = max(gptr[s], 0);
      g1 = min(gptr[s + 1], n);
    }
  }
  Point<D> pi;
#pragma unroll
  for (int c = 0; c < D; ++c) pi.c[c] = 0.f;
  if (g0 < g1) pi = load_point<D>(pos, i, ldp);
  int base = 0, end = 0, tj = -1;
  float td = -1.f;
  if (rv) {
    base = rowptr[i];
    end = rowptr[i + 1];
    td = tau_d2[i];
    tj = tau_j[i];
  }
  constexpr unsigned long long kGroup = L == 64 ? ~0ull : (1ull << (L & 63)) - 1ull;
  const int shift = sub * L;
  // the condition is wave-uniform: all 64 lanes run every step, finished sub-groups idle
  for (int j0 = g0; __builtin_amdgcn_ballot_w64(j0 < g1) != 0ull; j0 += L) {
    const int j = j0 + sl;
    float d = 0.f;
    bool keep = false;
    if (j < g1) {
      const Point<D> pj = load_point<D>(pos, j, ldp);
      d = sq_dist<D>(pi, pj);
      keep = (d < td || (d == td && j <= tj)) && (loop || j != i);   // a NaN distance compares false
    }
    const unsigned long long m = (__builtin_amdgcn_ballot_w64(keep) >> shift) & kGroup;
    const int slot = base + __popcll(m & ((1ull << sl) - 1ull));
    if (keep && slot < end) {
      out[slot] = j;
      if (d2out) d2out[slot] = d;
    }
    base += __popcll(m);
  }
}

template <int L, int D>
__global__ __launch_bounds__(256) void pair_d2_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                      const float* __restrict__ pos, float* __restrict__ d2out,
                                                      int n, int ldp) {
  int sub, sl;
  const long row = sub_row<L>(sub, sl);
  if (row >= n) return;                             // no cross-lane traffic below
  const int i = (int)row;
  const int e0 = rowptr[i], e1 = rowptr[i + 1];
  if (e0 >= e1) return;
  const Point<D> pi = load_point<D>(pos, i, ldp);
#pragma unroll 2
  for (int e = e0 + sl; e < e1; e += L) d2out[e] = sq_dist<D>(pi, load_point<D>(pos, col[e], ldp));
}

template <int L, int D>
__global__ __launch_bounds__(256) void pair_d2_bwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                          const int* __restrict__ rowptr_t,
                                                          const int* __restrict__ col_t,
                                                          const int* __restrict__ eperm_t,
                                                          const float* __restrict__ pos, const float* __restrict__ g,
                                                          float* __restrict__ dpos, int n, int ldp) {
  int sub, sl;
  const long row = sub_row<L>(sub, sl);
  const bool rv = row < n;                          // the butterfly below needs every lane
  const int i = rv ? (int)row : 0;
  const int e0 = rv ? rowptr[i] : 0, e1 = rv ? rowptr[i + 1] : 0;
  const int t0 = rv ? rowptr_t[i] : 0, t1 = rv ? rowptr_t[i + 1] : 0;
  float acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = 0.f;
  if (e0 < e1 || t0 < t1) {
    const Point<D> pi = load_point<D>(pos, i, ldp);
    for (int e = e0 + sl; e < e1; e += L) {
      const Point<D> pj = load_point<D>(pos, col[e], ldp);
      const float ge = g[e];
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = __fmaf_rn(ge, __fsub_rn(pi.c[c], pj.c[c]), acc[c]);
    }
    for (int t = t0 + sl; t < t1; t += L) {
      const Point<D> pj = load_point<D>(pos, col_t[t], ldp);
      const float ge = g[eperm_t[t]];
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = __fmaf_rn(ge, __fsub_rn(pi.c[c], pj.c[c]), acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = group_sum<L>(acc[c]);
  if (!rv) return;
  for (int c = sl; c < ldp; c += L) {
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < D; ++q) v = c == q ? acc[q] : v;
    dpos[(size_t)i * ldp + c] = __fmul_rn(2.f, v);
  }
}

// The periodic radius search.  FILL = false: out = deg [n].  FILL = true: out = col, written at
// rowptr[i] ... with shiftout (required) and d2out (may be null) at the same slots.  The
// candidate of a lane is the number (j - g0, dig[0], .., dig[D - 1]) in the mixed radix
// (*, rad[0], .., rad[D - 1]), rad[a] = 2 nimg[a] + 1, s[a] = dig[a] - nimg[a]: lane sl starts
// at the digits of sl and every step adds the digits of L with carries, so consecutive lanes
// hold consecutive t = (j - g0) * M + m and the loop has no division.
template <int L, int D, bool FILL>
__global__ __launch_bounds__(256) void radius_pbc_kernel(const float* __restrict__ pos, const int* __restrict__ gptr,
                                                         const int* __restrict__ seg_id,
                                                         const float* __restrict__ cell,
                                                         const int* __restrict__ nimg, const int* __restrict__ rowptr,
                                                         int* __restrict__ out, float* __restrict__ d2out,
                                                         int* __restrict__ shiftout, int n, int G, int ldp, float r2,
                                                         int loop) {
  int sub, sl;
  const long row = sub_row<L>(sub, sl);
  const bool rv = row < n;
  const int i = rv ? (int)row : 0;
  int g0 = 0, g1 = 0, gs = 0;
  if (rv) {
    const int s = seg_id[i];
    if (s >= 0 && s < G) {
      g0 = max(gptr[s], 0);
      g1 = min(gptr[s + 1], n);
      gs = s;
    }
  }
  Point<D> pi;
#pragma unroll
  for (int c = 0; c < D; ++c) pi.c[c] = 0.f;
  Cell<D> C = zero_cell<D>();
  int ni[D];
#pragma unroll
  for (int a = 0; a < D; ++a) ni[a] = 0;
  if (g0 < g1) {
    pi = load_point<D>(pos, i, ldp);
    C = load_cell<D>(cell, gs);
#pragma unroll
    for (int a = 0; a < D; ++a) ni[a] = min(max(nimg[(size_t)gs * 3 + a], 0), kPbcNimgMax);
  }
  int rad[D], dig[D], stp[D];
  int x = sl, y = L;
#pragma unroll
  for (int a = D - 1; a >= 0; --a) {
    rad[a] = 2 * ni[a] + 1;
    const int qx = small_div(x, rad[a]), qy = small_div(y, rad[a]);
    dig[a] = x - qx * rad[a];
    stp[a] = y - qy * rad[a];
    x = qx;
    y = qy;
  }
  int j = g0 + x;                                   // x <= sl < L, y <= L
  const int jstp = y;
  int base = 0, end = 0;
  if (FILL && rv) {
    base = rowptr[i];
    end = rowptr[i + 1];
  }
  constexpr unsigned long long kGroup = L == 64 ? ~0ull : (1ull << (L & 63)) - 1ull;
  const int shift = sub * L;
  // the condition is wave-uniform: all 64 lanes run every step, finished sub-groups idle
  while (__builtin_amdgcn_ballot_w64(j < g1) != 0ull) {
    const int jc = j;                               // this step's candidate: j advances below
    const bool ok = jc < g1;
    float d = 0.f;
    bool keep = false;
    int s[D];
#pragma unroll
    for (int a = 0; a < D; ++a) s[a] = dig[a] - ni[a];
    if (ok) {
      const Point<D> q = image_point<D>(load_point<D>(pos, jc, ldp), image_offset<D>(C, s));
      d = sq_dist<D>(pi, q);
      bool home = jc == i;
#pragma unroll
      for (int a = 0; a < D; ++a) home = home && s[a] == 0;
      keep = d <= r2 && (loop || !home);            // a NaN distance compares false
      // the next candidate of this lane; a finished lane stays where it is (j >= g1 for good)
      int carry = 0;
#pragma unroll
      for (int a = D - 1; a >= 0; --a) {
        const int v = dig[a] + stp[a] + carry;      // < 2 rad[a]
        carry = v >= rad[a] ? 1 : 0;
        dig[a] = v - (carry ? rad[a] : 0);
      }
      j += jstp + carry;
    }
    const unsigned long long m = (__builtin_amdgcn_ballot_w64(keep) >> shift) & kGroup;
    if (FILL) {
      const int slot = base + __popcll(m & ((1ull << sl) - 1ull));
      if (keep && slot < end) {
        out[slot] = jc;
        shiftout[slot] = pack_shift<D>(s);
        if (d2out) d2out[slot] = d;
      }
    }
    base += __popcll(m);
  }
  if (!FILL && rv && sl == 0) out[i] = base;
}

// d2 [nnz] of a CSR with image shifts: sq_dist(p_i, p_col[e] + shift[e] . cell(graph of i))
template <int L, int D>
__global__ __launch_bounds__(256) void pair_d2_pbc_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                          const int* __restrict__ shift,
                                                          const float* __restrict__ pos,
                                                          const float* __restrict__ cell,
                                                          const int* __restrict__ seg_id, float* __restrict__ d2out,
                                                          int n, int G, int ldp) {
  int sub, sl;
  const long row = sub_row<L>(sub, sl);
  if (row >= n) return;                             // no cross-lane traffic below
  const int i = (int)row;
  const int e0 = rowptr[i], e1 = rowptr[i + 1];
  if (e0 >= e1) return;
  const Point<D> pi = load_point<D>(pos, i, ldp);
  const Cell<D> C = cell_of_row<D>(cell, seg_id, i, G);
#pragma unroll 2
  for (int e = e0 + sl; e < e1; e += L) {
    int s[D];
    unpack_shift<D>(shift[e], s);
    d2out[e] = sq_dist<D>(pi, image_point<D>(load_point<D>(pos, col[e], ldp), image_offset<D>(C, s)));
  }
}

// pair_d2_bwd_kernel with the shifted differences: p_i - (p_j + off_e) over the in-edges,
// p_i - (p_k - off_e) over the out-edges (off_e of CSR edge e = eperm_t[t])
template <int L, int D>
__global__ __launch_bounds__(256) void pair_d2_pbc_bwd_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const int* __restrict__ shift,
    const int* __restrict__ rowptr_t, const int* __restrict__ col_t, const int* __restrict__ eperm_t,
    const float* __restrict__ pos, const float* __restrict__ cell, const int* __restrict__ seg_id,
    const float* __restrict__ g, float* __restrict__ dpos, int n, int G, int ldp) {
  int sub, sl;
  const long row = sub_row<L>(sub, sl);
  const bool rv = row < n;                          // the butterfly below needs every lane
  const int i = rv ? (int)row : 0;
  const int e0 = rv ? rowptr[i] : 0, e1 = rv ? rowptr[i + 1] : 0;
  const int t0 = rv ? rowptr_t[i] : 0, t1 = rv ? rowptr_t[i + 1] : 0;
  float acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = 0.f;
  if (e0 < e1 || t0 < t1) {
    const Point<D> pi = load_point<D>(pos, i, ldp);
    const Cell<D> C = cell_of_row<D>(cell, seg_id, i, G);
    for (int e = e0 + sl; e < e1; e += L) {
      int s[D];
      unpack_shift<D>(shift[e], s);
      const Point<D> off = image_offset<D>(C, s);
      const Point<D> pj = load_point<D>(pos, col[e], ldp);
      const float ge = g[e];
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = __fmaf_rn(ge, __fsub_rn(pi.c[c], __fadd_rn(pj.c[c], off.c[c])), acc[c]);
    }
    for (int t = t0 + sl; t < t1; t += L) {
      const int e = eperm_t[t];
      int s[D];
      unpack_shift<D>(shift[e], s);
      const Point<D> off = image_offset<D>(C, s);
      const Point<D> pk = load_point<D>(pos, col_t[t], ldp);
      const float ge = g[e];
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = __fmaf_rn(ge, __fsub_rn(pi.c[c], __fsub_rn(pk.c[c], off.c[c])), acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = group_sum<L>(acc[c]);
  if (!rv) return;
  for (int c = sl; c < ldp; c += L) {
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < D; ++q) v = c == q ? acc[q] : v;
    dpos[(size_t)i * ldp + c] = __fmul_rn(2.f, v);
  }
}

// ---------------------------------------------------------------- launchers

namespace {

// fn(Const<L>, Const<D>) for a compiled sub-group width and dimension; the caller has
// checked both
template <class Fn>
int with_ld(int L, int D, Fn&& fn) {
  auto dim = [&](auto l) {
    if (D == 1) return fn(l, Const<1>{});
    if (D == 2) return fn(l, Const<2>{});
    return fn(l, Const<3>{});
  };
  if (L == 8) return dim(Const<8>{});
  if (L == 16) return dim(Const<16>{});
  if (L == 32) return dim(Const<32>{});
  return dim(Const<64>{});
}

// the sub-group width for `per_row` candidates (or edges) per row on average: the average
// row takes at most two steps of its sub-group
int geo_auto_lanes(long per_row_total, int n_rows) {
  if (per_row_total <= 16L * n_rows) return 8;
  if (per_row_total <= 32L * n_rows) return 16;
  if (per_row_total <= 64L * n_rows) return 32;
  return 64;
}

bool geo_shape_ok(int D, int lanes) {
  return D >= 1 && D <= 3 && (lanes == 0 || lanes == 8 || lanes == 16 || lanes == 32 || lanes == 64);
}

// blocks for n rows, or 0 when the launch would count its threads past 32 bits
unsigned geo_grid(int L, int n) {
  const long rpb = 4 * (64 / L);
  const long b = ((long)n + rpb - 1) / rpb;
  return b > (1L << 24) - 1 ? 0u : (unsigned)b;
}

// the checks the two passes of the search share, in the documented order; 1: go on
int radius_prepare(int n, int G, int D, int ldp, float r, int lanes, int* L) {
  if (!geo_shape_ok(D, lanes)) return -1;
  if (ldp < D || !(r >= 0.f) || !std::isfinite(r)) return -3;
  if (n <= 0) return 0;
  // lanes = 0: from the average graph length (a caller that knows the longest graph passes
  // its own choice: gnn/geometry.py)
  *L = lanes ? lanes : geo_auto_lanes(n, G > 0 ? G : 1);
  return 1;
}

}  // namespace

// deg [n] of the radius graph of pos [n, ldp] over the graphs gptr [G + 1] / seg_id [n].
// lanes: 0 = from n / G, or one of 8 / 16 / 32 / 64.  No allocation and no synchronisation:
// capturable into a hipGraph.  Return codes: see cgnn_api.h.
extern "C" int gnn_launch_radius_count(const float* pos, const int* gptr, const int* seg_id, int* deg, int n, int G,
                                       int D, int ldp, float r, int loop, int lanes, hipStream_t st) {
  int L = 0;
  const int rc = radius_prepare(n, G, D, ldp, r, lanes, &L);
  if (rc <= 0) return rc;
  if (!pos || !gptr || !seg_id || !deg || G < 1) return -3;
  const unsigned grid = geo_grid(L, n);
  if (!grid) return -4;
  const float r2 = r * r;
  return with_ld(L, D, [&](auto l, auto d) {
    hipLaunchKernelGGL((radius_kernel<decltype(l)::value, decltype(d)::value, false>), dim3(grid), dim3(256), 0, st,
                       pos, gptr, seg_id, (const int*)nullptr, deg, (float*)nullptr, n, G, ldp, r2, loop);
    return (int)hipGetLastError();
  });
}

// col (and d2, which may be null) at rowptr[i] .. rowptr[i + 1], rowptr [n + 1] the exclusive
// sum of the count pass's deg for the same arguments.  Capturable like the count.
extern "C" int gnn_launch_radius_fill(const float* pos, const int* gptr, const int* seg_id, const int* rowptr,
                                      int* col, float* d2, int n, int G, int D, int ldp, float r, int loop, int lanes,
                                      hipStream_t st) {
  int L = 0;
  const int rc = radius_prepare(n, G, D, ldp, r, lanes, &L);
  if (rc <= 0) return rc;
  if (!pos || !gptr || !seg_id || !rowptr || !col || G < 1) return -3;
  const unsigned grid = geo_grid(L, n);
  if (!grid) return -4;
  const float r2 = r * r;
  return with_ld(L, D, [&](auto l, auto d) {
    hipLaunchKernelGGL((radius_kernel<decltype(l)::value, decltype(d)::value, true>), dim3(grid), dim3(256), 0, st,
                       pos, gptr, seg_id, rowptr, col, d2, n, G, ldp, r2, loop);
    return (int)hipGetLastError();
  });
}

namespace {

// the smallest compiled sub-group width that holds k keys, one per lane
int knn_min_lanes(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }

}  // namespace

// deg / tau_d2 / tau_j [n] of the k nearest candidates of every point (see the header): pos
// [n, ldp] over the graphs gptr [G + 1] / seg_id [n], 1 <= k <= 64, r >= 0 or +inf for no
// radius.  lanes: 0 = the smallest compiled width that is >= k and at least the radius
// search's choice, or one of 8 / 16 / 32 / 64 that is >= k.  No allocation and no
// synchronisation: capturable into a hipGraph.  Return codes: see cgnn_api.h.
extern "C" int gnn_launch_knn_select(const float* pos, const int* gptr, const int* seg_id, int* deg, float* tau_d2,
                                     int* tau_j, int n, int G, int D, int ldp, int k, float r, int loop, int lanes,
                                     hipStream_t st) {
  if (!geo_shape_ok(D, lanes) || k < 1 || k > 64 || (lanes && lanes < k)) return -1;
  if (ldp < D || !(r >= 0.f)) return -3;
  if (n <= 0) return 0;
  if (!pos || !gptr || !seg_id || !deg || !tau_d2 || !tau_j || G < 1) return -3;
  const int L = lanes ? lanes : std::max(knn_min_lanes(k), geo_auto_lanes(n, G));
  const unsigned grid = geo_grid(L, n);
  if (!grid) return -4;
  const float r2 = r * r;
  return with_ld(L, D, [&](auto l, auto d) {
    hipLaunchKernelGGL((knn_select_kernel<decltype(l)::value, decltype(d)::value>), dim3(grid), dim3(256), 0, st, pos,
                       gptr, seg_id, deg, tau_d2, tau_j, n, G, ldp, k, r2, loop);
    return (int)hipGetLastError();
  });
}

// col (and d2, which may be null) at rowptr[i] .. rowptr[i + 1] for the thresholds of
// gnn_launch_knn_select, rowptr [n + 1] the exclusive sum of its deg.  lanes: 0 = from n / G,
// or any compiled width, whatever k and lanes selected.  Capturable like the select.
extern "C" int gnn_launch_knn_fill(const float* pos, const int* gptr, const int* seg_id, const int* rowptr,
                                   const float* tau_d2, const int* tau_j, int* col, float* d2, int n, int G, int D,
                                   int ldp, int loop, int lanes, hipStream_t st) {
  if (!geo_shape_ok(D, lanes)) return -1;
  if (ldp < D) return -3;
  if (n <= 0) return 0;
  if (!pos || !gptr || !seg_id || !rowptr || !tau_d2 || !tau_j || !col || G < 1) return -3;
  const int L = lanes ? lanes : geo_auto_lanes(n, G);
  const unsigned grid = geo_grid(L, n);
  if (!grid) return -4;
  return with_ld(L, D, [&](auto l, auto d) {
    hipLaunchKernelGGL((knn_fill_kernel<decltype(l)::value, decltype(d)::value>), dim3(grid), dim3(256), 0, st, pos,
                       gptr, seg_id, rowptr, tau_d2, tau_j, col, d2, n, G, ldp, loop);
    return (int)hipGetLastError();
  });
}

// d2 [nnz] of the edges of the CSR (rowptr [n + 1], col) over pos [*, ldp].  lanes: 0 = from
// nnz / n.  Capturable.
extern "C" int gnn_launch_pair_d2(const int* rowptr, const int* col, const float* pos, float* d2, int n, int nnz,
                                  int D, int ldp, int lanes, hipStream_t st) {
  if (!geo_shape_ok(D, lanes)) return -1;
  if (ldp < D || nnz < 0) return -3;
  if (n <= 0 || nnz == 0) return 0;
  if (!rowptr || !col || !pos || !d2) return -3;
  const int L = lanes ? lanes : geo_auto_lanes(nnz, n);
  const unsigned grid = geo_grid(L, n);
  if (!grid) return -4;
  return with_ld(L, D, [&](auto l, auto d) {
    hipLaunchKernelGGL((pair_d2_kernel<decltype(l)::value, decltype(d)::value>), dim3(grid), dim3(256), 0, st, rowptr,
                       col, pos, d2, n, ldp);
    return (int)hipGetLastError();
  });
}

// dpos [n, ldp] from g [nnz] = dL / d d2 over the CSR and its transpose (square: n rows, n
// columns).  lanes: 0 = from 2 nnz / n.  With nnz == 0 nothing is launched and dpos is left to
// the caller (ops.pair_d2_bwd zeroes it).  Capturable.
extern "C" int gnn_launch_pair_d2_bwd(const int* rowptr, const int* col, const int* rowptr_t, const int* col_t,
                                      const int* eperm_t, const float* pos, const float* g, float* dpos, int n,
                                      int nnz, int D, int ldp, int lanes, hipStream_t st) {
  if (!geo_shape_ok(D, lanes)) return -1;
  if (ldp < D || nnz < 0) return -3;
  if (n <= 0 || nnz == 0) return 0;
  if (!rowptr || !col || !rowptr_t || !col_t || !eperm_t || !pos || !g || !dpos) return -3;
  const int L = lanes ? lanes : geo_auto_lanes(2L * nnz, n);
  const unsigned grid = geo_grid(L, n);
  if (!grid) return -4;
  return with_ld(L, D, [&](auto l, auto d) {
    hipLaunchKernelGGL((pair_d2_bwd_kernel<decltype(l)::value, decltype(d)::value>), dim3(grid), dim3(256), 0, st,
                       rowptr, col, rowptr_t, col_t, eperm_t, pos, g, dpos, n, ldp);
    return (int)hipGetLastError();
  });
}

namespace {

// radius_prepare for the periodic search: lanes = 0 chooses from the candidates per row, the
// average graph length times max_images (the launcher cannot read nimg)
int radius_pbc_prepare(int n, int G, int D, int ldp, float r, int lanes, int max_images, int* L) {
  if (!geo_shape_ok(D, lanes)) return -1;
  if (ldp < D || !(r >= 0.f) || !std::isfinite(r)) return -3;
  if (n <= 0) return 0;
  const long M = std::min(std::max(max_images, 1), 15 * 15 * 15);
  *L = lanes ? lanes : geo_auto_lanes((long)n * M, G > 0 ? G : 1);
  return 1;
}

}  // namespace

// deg [n] of the periodic radius graph (see the header, "Periodic cells"): pos [n, ldp] over the
// graphs gptr [G + 1] / seg_id [n] with the cells cell [G, 9] and the image ranges nimg [G, 3].
// lanes: 0 = from n / G * max_images (max_images: the largest number of images of a graph, a
// hint that only chooses the width), or one of 8 / 16 / 32 / 64.  No allocation and no
// synchronisation: capturable into a hipGraph.  Return codes: see cgnn_api.h.
extern "C" int gnn_launch_radius_pbc_count(const float* pos, const int* gptr, const int* seg_id, const float* cell,
                                           const int* nimg, int* deg, int n, int G, int D, int ldp, float r, int loop,
                                           int lanes, int max_images, hipStream_t st) {
  int L = 0;
  const int rc = radius_pbc_prepare(n, G, D, ldp, r, lanes, max_images, &L);
  if (rc <= 0) return rc;
  if (!pos || !gptr || !seg_id || !cell || !nimg || !deg || G < 1) return -3;
  const unsigned grid = geo_grid(L, n);
  if (!grid) return -4;
  const float r2 = r * r;
  return with_ld(L, D, [&](auto l, auto d) {
    hipLaunchKernelGGL((radius_pbc_kernel<decltype(l)::value, decltype(d)::value, false>), dim3(grid), dim3(256), 0,
                       st, pos, gptr, seg_id, cell, nimg, (const int*)nullptr, deg, (float*)nullptr, (int*)nullptr, n,
                       G, ldp, r2, loop);
    return (int)hipGetLastError();
  });
}

// col and shift (and d2, which may be null) at rowptr[i] .. rowptr[i + 1], rowptr [n + 1] the
// exclusive sum of the count pass's deg for the same arguments.  Capturable like the count.
extern "C" int gnn_launch_radius_pbc_fill(const float* pos, const int* gptr, const int* seg_id, const float* cell,
                                          const int* nimg, const int* rowptr, int* col, int* shift, float* d2, int n,
                                          int G, int D, int ldp, float r, int loop, int lanes, int max_images,
                                          hipStream_t st) {
  int L = 0;
  const int rc = radius_pbc_prepare(n, G, D, ldp, r, lanes, max_images, &L);
  if (rc <= 0) return rc;
  if (!pos || !gptr || !seg_id || !cell || !nimg || !rowptr || !col || !shift || G < 1) return -3;
  const unsigned grid = geo_grid(L, n);
  if (!grid) return -4;
  const float r2 = r * r;
  return with_ld(L, D, [&](auto l, auto d) {
    hipLaunchKernelGGL((radius_pbc_kernel<decltype(l)::value, decltype(d)::value, true>), dim3(grid), dim3(256), 0,
                       st, pos, gptr, seg_id, cell, nimg, rowptr, col, d2, shift, n, G, ldp, r2, loop);
    return (int)hipGetLastError();
  });
}

// d2 [nnz] of the edges of the CSR (rowptr [n + 1], col, shift) over pos [*, ldp], the cell of
// row i being cell[seg_id[i]] (seg_id [n], cell [G, 9]).  lanes: 0 = from nnz / n.  Capturable.
extern "C" int gnn_launch_pair_d2_pbc(const int* rowptr, const int* col, const int* shift, const float* pos,
                                      const float* cell, const int* seg_id, float* d2, int n, int nnz, int G, int D,
                                      int ldp, int lanes, hipStream_t st) {
  if (!geo_shape_ok(D, lanes)) return -1;
  if (ldp < D || nnz < 0) return -3;
  if (n <= 0 || nnz == 0) return 0;
  if (!rowptr || !col || !shift || !pos || !cell || !seg_id || !d2 || G < 1) return -3;
  const int L = lanes ? lanes : geo_auto_lanes(nnz, n);
  const unsigned grid = geo_grid(L, n);
  if (!grid) return -4;
  return with_ld(L, D, [&](auto l, auto d) {
    hipLaunchKernelGGL((pair_d2_pbc_kernel<decltype(l)::value, decltype(d)::value>), dim3(grid), dim3(256), 0, st,
                       rowptr, col, shift, pos, cell, seg_id, d2, n, G, ldp);
    return (int)hipGetLastError();
  });
}

// dpos [n, ldp] from g [nnz] = dL / d d2 over the CSR with image shifts and its transpose.
// lanes: 0 = from 2 nnz / n.  With nnz == 0 nothing is launched and dpos is left to the caller
// (ops.pair_d2_pbc_bwd zeroes it).  Capturable.
extern "C" int gnn_launch_pair_d2_pbc_bwd(const int* rowptr, const int* col, const int* shift, const int* rowptr_t,
                                          const int* col_t, const int* eperm_t, const float* pos, const float* cell,
                                          const int* seg_id, const float* g, float* dpos, int n, int nnz, int G, int D,
                                          int ldp, int lanes, hipStream_t st) {
  if (!geo_shape_ok(D, lanes)) return -1;
  if (ldp < D || nnz < 0) return -3;
  if (n <= 0 || nnz == 0) return 0;
  if (!rowptr || !col || !shift || !rowptr_t || !col_t || !eperm_t || !pos || !cell || !seg_id || !g || !dpos || G < 1)
    return -3;
  const int L = lanes ? lanes : geo_auto_lanes(2L * nnz, n);
  const unsigned grid = geo_grid(L, n);
  if (!grid) return -4;
  return with_ld(L, D, [&](auto l, auto d) {
    hipLaunchKernelGGL((pair_d2_pbc_bwd_kernel<decltype(l)::value, decltype(d)::value>), dim3(grid), dim3(256), 0, st,
                       rowptr, col, shift, rowptr_t, col_t, eperm_t, pos, cell, seg_id, g, dpos, n, G, ldp);
    return (int)hipGetLastError();
  });
}
