// GNN track (beyond the reference): max / min neighbour pooling for MI355X.
//
//   pool_fwd_kernel  Y[i,f]   = max (or min) over e in row i of X[col[e], f]
//                    arg[i,f] = the edge index e (global, int32) that supplied Y[i,f]
//   pool_bwd_kernel  dX[j,f]  = sum over the transposed edges t of row j, with i = col_t[t]
//                    and e = eperm[t], of (arg[i,f] == e ? dY[i,f] : 0): the gradient, as a
//                    gather over the transposed CSR.  Edge indices are compared, not node
//                    ids, so a source id repeated in one row is counted once.
//
// Contract of the forward.  Edges are scanned in CSR order; a candidate replaces the running
// best only when it is strictly better (> for max, < for min) or when it is NaN and the best
// is not.  Ties go to the first edge of the row holding the value, a NaN propagates and arg
// is the first NaN edge (fmaxf / fminf drop NaNs: the rule is written as compares).  An
// empty row gives Y = 0, arg = -1, and so do the padding columns F <= f < ld.  The output
// has the input's storage type: the value is a copy of an input element (16-bit inputs are
// compared as fp32, an exact conversion both ways), so the result is exact in every type.
//
// Mapping (gnn_launch.h's): wave64, a sub-group of L lanes owns one row, each lane owns 8
// consecutive features (one 16-byte load per gathered bf16 / fp16 row, two for fp32), L =
// 8 / 16 / 32 / 64 for widths up to 64 / 128 / 256 / 512; wider rows run as 512-column
// slabs in the launchers.  The ids of a chunk of L edges come with one coalesced load per
// lane, requested one chunk ahead at an address clamped into the row, and are broadcast
// inside the sub-group; eight gathered rows are in flight per lane.
//
// Determinism: the forward accumulates nothing; the backward adds the selected entries in
// fp32 as ONE chain in transposed-edge order per (row, feature).  Neither depends on the
// grid, on the other rows of the launch or on the run.  No atomics.
//
// Empty inputs: a row with e0 == e1 dereferences none of col / eperm (every edge load sits
// behind the row's e1 > e0 test and is clamped into [e0, e1)), so a graph without edges
// may pass null pointers for them.
#include "cgnn_common.h"
#include "cgnn_api.h"
#include "gnn_gather.h"
#include "gnn_launch.h"

using namespace cgnn;
using namespace cgnn::gather;
using namespace cgnn::launch;

namespace {

// (Raw8, load_raw8, raw8_to_f32, sub_bcast, store8: gnn_gather.h, shared with gnn_wspmm.hip)

// 8 int32 at element offset `off` (two 16-byte loads)
struct Int8 {
  int4 a, b;
};

__device__ __forceinline__ Int8 load_int8(const int* A, size_t off) {
  const int4* p = reinterpret_cast<const int4*>(A + off);
  Int8 r;
  r.a = p[0];
  r.b = p[1];
  return r;
}

// the rows X[j[u]], u = 0..N-1 (edges e .. e + N - 1), offered to the running best in that
// order; the N rows are loaded before the first compare
template <int T, int N, bool MIN>
__device__ __forceinline__ void pool_step(const void* __restrict__ X, const int* j, int e, int ldx, int f0,
                                          float* best, int* bi) {
  Raw8<T> r[N];
#pragma unroll
  for (int u = 0; u < N; ++u) r[u] = load_raw8<T>(X, (size_t)j[u] * ldx + f0);
#pragma unroll
  for (int u = 0; u < N; ++u) {
    float c[8];
    raw8_to_f32<T>(r[u], c);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const bool take = (MIN ? c[q] < best[q] : c[q] > best[q]) | ((c[q] != c[q]) & (best[q] == best[q]));
      best[q] = take ? c[q] : best[q];
      bi[q] = take ? e + u : bi[q];
    }
  }
}

// acc[q] += arg[i[u], f0 + q] == e[u] ? dY[i[u], f0 + q] : 0 for u = 0..N-1 in that order,
// the N index and gradient rows loaded before the first add
template <int T, int N>
__device__ __forceinline__ void pool_bwd_step(const int* __restrict__ arg, const void* __restrict__ dY, const int* i,
                                              const int* e, int ldarg, int lddy, int f0, float* acc) {
  Int8 a[N];
  Raw8<T> r[N];
#pragma unroll
  for (int u = 0; u < N; ++u) {
    a[u] = load_int8(arg, (size_t)i[u] * ldarg + f0);
    r[u] = load_raw8<T>(dY, (size_t)i[u] * lddy + f0);
  }
#pragma unroll
  for (int u = 0; u < N; ++u) {
    float g[8];
    raw8_to_f32<T>(r[u], g);
    const int s[8] = {a[u].a.x, a[u].a.y, a[u].a.z, a[u].a.w, a[u].b.x, a[u].b.y, a[u].b.z, a[u].b.w};
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] += s[q] == e[u] ? g[q] : 0.f;
  }
}

}  // namespace

// wy / wa: the columns of Y / arg this launch writes from its base (the row stride for a
// whole-row launch, the slab width for a column-slab launch); columns [F, wy) of Y are
// written 0 and columns [F, wa) of arg -1.  arg may be null: no index is stored.
template <int L, int T, bool MIN>
__global__ __launch_bounds__(256) void pool_fwd_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const void* __restrict__ X, void* __restrict__ Y,
    int* __restrict__ arg, int n_rows, int F, int ldx, int ldy, int ldarg, int wy, int wa) {
  constexpr int RPW = 64 / L;
  const int lane = threadIdx.x & 63;
  const int sub = lane / L, sl = lane - sub * L, sub_base = sub * L;
  const unsigned blk = xcd_remap(blockIdx.x, gridDim.x);
  const int row = (blk * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + sub;
  const bool rv = row < n_rows;
  const int f0 = sl * 8;
  const bool fv = rv && f0 < F;
  // the identity of the reduction, index -1: a candidate equal to it never replaces it, so
  // an index still -1 after a non-empty row means every edge held that value, and the first
  // edge of the row is the answer
  const float ident = MIN ? __builtin_inff() : -__builtin_inff();
  float best[8];
  int bi[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    best[q] = ident;
    bi[q] = -1;
  }
  const int e0 = rv ? rowptr[row] : 0, e1 = rv ? rowptr[row + 1] : 0;
  if (e1 > e0) {                                  // uniform per sub-group
    // lane sl's edge of a chunk, from an address clamped into the row (an unconditional
    // load: a "load or 0" would branch and wait at the join)
    int nxj = col[min(e0 + sl, e1 - 1)];
    for (int e = e0; e < e1; e += L) {
      const int myj = nxj;
      nxj = col[min(e + L + sl, e1 - 1)];         // the next chunk, under this chunk's gathers
      const int cnt = min(L, e1 - e);
      int k = 0;
      for (; k + 8 <= cnt; k += 8) {
        int j[8];
        sub_bcast<L, 8>(myj, sub_base, k, j);
        if (fv) pool_step<T, 8, MIN>(X, j, e + k, ldx, f0, best, bi);
      }
      for (; k + 4 <= cnt; k += 4) {
        int j[4];
        sub_bcast<L, 4>(myj, sub_base, k, j);
        if (fv) pool_step<T, 4, MIN>(X, j, e + k, ldx, f0, best, bi);
      }
      for (; k < cnt; ++k) {
        int j[1];
        sub_bcast<L, 1>(myj, sub_base, k, j);
        if (fv) pool_step<T, 1, MIN>(X, j, e + k, ldx, f0, best, bi);
      }
    }
  }
  if (!rv) return;
  const bool any = e1 > e0;
  if (f0 < wy) {
    float y[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) y[q] = (any && f0 + q < F) ? best[q] : 0.f;
    store8<T>(Y, (size_t)row * ldy + f0, y);
  }
  if (arg && f0 < wa) {
    int a[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) a[q] = (any && f0 + q < F) ? (bi[q] < 0 ? e0 : bi[q]) : -1;
    int4* p = reinterpret_cast<int4*>(arg + (size_t)row * ldarg + f0);
    p[0] = make_int4(a[0], a[1], a[2], a[3]);
    p[1] = make_int4(a[4], a[5], a[6], a[7]);
  }
}

// Over the transposed CSR: row j is a source node, its edges t name the destination i =
// col_t[t] and the forward edge e = eperm[t].  wcols as in wspmm_kernel.
template <int L, int TDY, int TDX>
__global__ __launch_bounds__(256) void pool_bwd_kernel(
    const int* __restrict__ rowptr_t, const int* __restrict__ col_t, const int* __restrict__ eperm,
    const int* __restrict__ arg, const void* __restrict__ dY, void* __restrict__ dX, int n_src, int F, int ldarg,
    int lddy, int lddx, int wcols) {
  constexpr int RPW = 64 / L;
  const int lane = threadIdx.x & 63;
  const int sub = lane / L, sl = lane - sub * L, sub_base = sub * L;
  const unsigned blk = xcd_remap(blockIdx.x, gridDim.x);
  const int row = (blk * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + sub;
  const bool rv = row < n_src;
  const int f0 = sl * 8;
  const bool fv = rv && f0 < F;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int e0 = rv ? rowptr_t[row] : 0, e1 = rv ? rowptr_t[row + 1] : 0;
  if (e1 > e0) {                                  // uniform per sub-group
    auto edge = [&](int t, int& i, int& e) {
      const int tc = min(t, e1 - 1);
      i = col_t[tc];
      e = eperm[tc];
    };
    int nxi, nxe;
    edge(e0 + sl, nxi, nxe);
    for (int t = e0; t < e1; t += L) {
      const int myi = nxi, mye = nxe;
      edge(t + L + sl, nxi, nxe);                 // the next chunk, under this chunk's gathers
      const int cnt = min(L, e1 - t);
      int k = 0;
      for (; k + 8 <= cnt; k += 8) {
        int i[8], e[8];
        sub_bcast<L, 8>(myi, sub_base, k, i);
        sub_bcast<L, 8>(mye, sub_base, k, e);
        if (fv) pool_bwd_step<TDY, 8>(arg, dY, i, e, ldarg, lddy, f0, acc);
      }
      for (; k + 4 <= cnt; k += 4) {
        int i[4], e[4];
        sub_bcast<L, 4>(myi, sub_base, k, i);
        sub_bcast<L, 4>(mye, sub_base, k, e);
        if (fv) pool_bwd_step<TDY, 4>(arg, dY, i, e, ldarg, lddy, f0, acc);
      }
      for (; k < cnt; ++k) {
        int i[1], e[1];
        sub_bcast<L, 1>(myi, sub_base, k, i);
        sub_bcast<L, 1>(mye, sub_base, k, e);
        if (fv) pool_bwd_step<TDY, 1>(arg, dY, i, e, ldarg, lddy, f0, acc);
      }
    }
  }
  if (!rv || f0 >= wcols) return;
  float y[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) y[q] = f0 + q < F ? acc[q] : 0.f;
  store8<TDX>(dX, (size_t)row * lddx + f0, y);
}

// ---------------------------------------------------------------- launchers
// (lane dispatch, grid, type tables and the slab walk: gnn_launch.h)

// X and Y share the storage type t; arg (int32, row stride ldarg) may be null (inference).
// No allocation and no synchronisation: capturable into a hipGraph.  Return codes: see
// cgnn_api.h.
extern "C" int gnn_launch_pool_fwd(const int* rowptr, const int* col, const void* X, void* Y, int* arg, int n_rows,
                                   int F, int ldx, int ldy, int ldarg, int t, int is_min, hipStream_t st) {
  if (F < 0 || !stride_ok(ldx, F) || !stride_ok(ldy, F)) return -3;
  if (arg && !stride_ok(ldarg, F)) return -3;
  if (!type_ok(t)) return -5;
  if (n_rows <= 0) return 0;
  if (!rowptr || !X || !Y) return -3;
  // two written widths: the walk covers the wider, each slab writes [0, wy) of Y and
  // [0, wa) of arg from their bases
  const int lda = arg ? ldarg : 0;
  return for_slabs(F, std::max(ldy, lda), [&](int c0, int fc, int) {
    const int wy = std::max(0, std::min(kSlab, ldy - c0));
    const int wa = std::max(0, std::min(kSlab, lda - c0));
    const void* x = in_at(X, t, c0, fc);
    void* y = wy ? out_at(Y, t, c0) : Y;
    int* a = arg && wa ? arg + c0 : nullptr;
    return with_lanes(std::max({fc, wy, wa}), [&](auto l) {
      constexpr int L = decltype(l)::value;
      return with_type(t, [&](auto tt) {
        constexpr int T = decltype(tt)::value;
        hipLaunchKernelGGL((!is_min ? pool_fwd_kernel<L, T, false> : pool_fwd_kernel<L, T, true>),
                           dim3(blocks(L, n_rows)), dim3(256), 0, st, rowptr, col, x, y, a, n_rows, fc, ldx, ldy, ldarg,
                           wy, wa);
        return (int)hipGetLastError();
      });
    });
  });
}

// dX [n_src, lddx] from the forward's arg [n_dst, ldarg] and dY [n_dst, lddy]; padding
// columns of dX are written 0.  The (dY, dX) type pairs are gnn_launch_wspmm's.  Capturable
// like the forward.
extern "C" int gnn_launch_pool_bwd(const int* rowptr_t, const int* col_t, const int* eperm, const int* arg, int ldarg,
                                   const void* dY, int lddy, void* dX, int lddx, int n_src, int F, int tdy, int tdx,
                                   hipStream_t st) {
  if (F < 0 || !stride_ok(ldarg, F) || !stride_ok(lddy, F) || !stride_ok(lddx, F)) return -3;
  if (!pair_ok(tdy, tdx)) return -5;
  if (n_src <= 0) return 0;
  if (!rowptr_t || !arg || !dY || !dX) return -3;
  return for_slabs(F, lddx, [&](int c0, int fc, int wc) {
    const int* a = in_at(arg, c0, fc);
    const void* dy = in_at(dY, tdy, c0, fc);
    void* dx = out_at(dX, tdx, c0);
    return with_lanes(std::max(fc, wc), [&](auto l) {
      constexpr int L = decltype(l)::value;
      return with_pair(tdy, tdx, [&](auto ty, auto tx) {
        hipLaunchKernelGGL((pool_bwd_kernel<L, decltype(ty)::value, decltype(tx)::value>), dim3(blocks(L, n_src)),
                           dim3(256), 0, st, rowptr_t, col_t, eperm, a, dy, dx, n_src, fc, ldarg, lddy, lddx, wc);
        return (int)hipGetLastError();
      });
    });
  });
}
