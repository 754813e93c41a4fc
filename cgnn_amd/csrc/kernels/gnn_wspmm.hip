// GNN track (beyond the reference): edge-weighted message passing for MI355X.
//
//   wspmm_kernel  Y[i,:F] = act( rscale[i] * sum_{e in row i} val[p(e)] * cscale[col[e]] * X[col[e],:F] + bias )
//                 CSR aggregate with one caller-supplied fp32 value per edge; p(e) = eperm[e]
//                 when an edge permutation is given (the backward runs over the transposed
//                 CSR and reads the forward's value array in place), else e.
//   sddmm_kernel  out[e] = rscale[i] * cscale[j] * sum_{f<F} A[i,f] * B[j,f]  for every edge
//                 e = (i, j) of the CSR: the gradient of the weighted aggregate with respect
//                 to each edge value.
//
// Mapping (gnn_launch.h's): wave64, a sub-group of L lanes owns one row, each lane owns 8
// consecutive features (one 16-byte load per gathered bf16 / fp16 row), L = 8 / 16 / 32 / 64
// for widths up to 64 / 128 / 256 / 512; wider rows run as 512-column slabs in the
// launchers.  The ids and values of a chunk of L edges come with one coalesced load per
// lane, requested one chunk ahead, and are broadcast inside the sub-group; eight gathered
// rows are in flight per lane.  Accumulation is fp32.
//
// Determinism: per row and feature the multiply-adds are ONE chain of fmaf in edge order
// (wspmm), and per edge the products are one fmaf chain per lane followed by a fixed
// exchange tree over the L lanes (sddmm).  Neither depends on the grid, on the other rows
// of the launch or on the run: outputs are bit-identical from run to run, and a row's
// result is the same in any launch that holds it.  No atomics.
//
// Empty inputs: a row with e0 == e1 dereferences none of col / val / eperm / cscale (every
// edge load sits behind the row's e1 > e0 test and is clamped into [e0, e1)), so a graph
// without edges may pass null pointers for them.
#include "cgnn_common.h"
#include "cgnn_api.h"
#include "gnn_gather.h"
#include "gnn_launch.h"

using namespace cgnn;
using namespace cgnn::gather;
using namespace cgnn::launch;

namespace {

// (Raw8, load_raw8, raw8_to_f32, sub_bcast, store8: gnn_gather.h, shared with gnn_pool.hip)

// acc[q] = fmaf(w[u], X[j[u], f0 + q], acc[q]) for u = 0..N-1 in that order, the N rows
// loaded before the first multiply-add
template <int XT, int N>
__device__ __forceinline__ void wgather_step(const void* __restrict__ X, const int* j, const int* w, int ldx,
                                             int f0, float* acc) {
  Raw8<XT> r[N];
#pragma unroll
  for (int u = 0; u < N; ++u) r[u] = load_raw8<XT>(X, (size_t)j[u] * ldx + f0);
#pragma unroll
  for (int u = 0; u < N; ++u) {
    float a[8];
    raw8_to_f32<XT>(r[u], a);
    const float wu = __int_as_float(w[u]);
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = fmaf(wu, a[q], acc[q]);
  }
}

}  // namespace

// wcols: output columns this launch writes from its base (the row stride for a whole-row
// launch, the slab width for a column-slab launch); columns [F, wcols) are written 0
template <int L, int XT, int YT>
__global__ __launch_bounds__(256) void wspmm_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ val,
    const int* __restrict__ eperm, const void* __restrict__ X, void* __restrict__ Y,
    const float* __restrict__ rscale, const float* __restrict__ cscale, const float* __restrict__ bias,
    int n_rows, int F, int ldx, int ldy, int relu, int wcols) {
  constexpr int RPW = 64 / L;
  const int lane = threadIdx.x & 63;
  const int sub = lane / L, sl = lane - sub * L, sub_base = sub * L;
  const unsigned blk = xcd_remap(blockIdx.x, gridDim.x);
  const int row = (blk * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + sub;
  const bool rv = row < n_rows;
  const int f0 = sl * 8;
  const bool fv = rv && f0 < F;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int e0 = rv ? rowptr[row] : 0, e1 = rv ? rowptr[row + 1] : 0;
  if (e1 > e0) {                                  // uniform per sub-group
    // lane sl's edge of a chunk: its id and value, from an address clamped into the row
    // (an unconditional load: a "load or 0" would branch and wait at the join)
    auto edge = [&](int e, int& j, float& v) {
      const int ec = min(e, e1 - 1);
      j = col[ec];
      v = val[eperm ? eperm[ec] : ec];
    };
    int nxj;
    float nxv;
    edge(e0 + sl, nxj, nxv);
    for (int e = e0; e < e1; e += L) {
      const int myj = nxj;
      const float myv = nxv;
      edge(e + L + sl, nxj, nxv);                 // the next chunk, under this chunk's gathers
      // the edge's weight, rounded once: val * cscale
      const int myw = __float_as_int(cscale ? myv * cscale[myj] : myv);
      const int cnt = min(L, e1 - e);
      int k = 0;
      for (; k + 8 <= cnt; k += 8) {
        int j[8], w[8];
        sub_bcast<L, 8>(myj, sub_base, k, j);
        sub_bcast<L, 8>(myw, sub_base, k, w);
        if (fv) wgather_step<XT, 8>(X, j, w, ldx, f0, acc);
      }
      for (; k + 4 <= cnt; k += 4) {
        int j[4], w[4];
        sub_bcast<L, 4>(myj, sub_base, k, j);
        sub_bcast<L, 4>(myw, sub_base, k, w);
        if (fv) wgather_step<XT, 4>(X, j, w, ldx, f0, acc);
      }
      for (; k < cnt; ++k) {
        int j[1], w[1];
        sub_bcast<L, 1>(myj, sub_base, k, j);
        sub_bcast<L, 1>(myw, sub_base, k, w);
        if (fv) wgather_step<XT, 1>(X, j, w, ldx, f0, acc);
      }
    }
  }
  if (!rv || f0 >= wcols) return;
  const float rs = rscale ? rscale[row] : 1.f;
  float y[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int f = f0 + q;
    float v = acc[q] * rs + ((bias && f < F) ? bias[f] : 0.f);
    if (relu) v = fmaxf(v, 0.f);
    y[q] = f < F ? v : 0.f;
  }
  store8<YT>(Y, (size_t)row * ldy + f0, y);
}

// out[e] for the edges of row i.  Row i's slice of A stays in registers; each gathered row
// of B gives 8 products per lane (one fmaf chain in feature order).  Eight edges at a
// time: the 8 partial sums of a lane are combined with those of the lanes sl ^ 4, sl ^ 2,
// sl ^ 1 in an exchange tree that halves the values a lane keeps at every level (4 + 2 + 1
// exchanges instead of 8 x 3), then the remaining levels sl ^ 8 .. sl ^ L/2 add single
// values: the dot product of edge k + (sl & 7) is in every lane, and the lane whose index
// in the sub-group is that edge's index in the chunk keeps it.  A chunk of L results is
// stored with ONE coalesced write, out[e + sl].
// first / last: a width above 512 runs as launches over 512-column slabs in stream order;
// a launch that is not the first adds to the sum its predecessor left in out[e], and the
// last one applies the scales -- an ordered sum, never an unordered accumulation.
template <int L, int T>
__global__ __launch_bounds__(256) void sddmm_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const void* __restrict__ A,
    const void* __restrict__ B, float* __restrict__ out, const float* __restrict__ rscale,
    const float* __restrict__ cscale, int n_rows, int F, int lda, int ldb, int first, int last) {
  constexpr int RPW = 64 / L;
  const int lane = threadIdx.x & 63;
  const int sub = lane / L, sl = lane - sub * L, sub_base = sub * L;
  const unsigned blk = xcd_remap(blockIdx.x, gridDim.x);
  const int row = (blk * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + sub;
  if (row >= n_rows) return;                      // uniform per sub-group
  const int e0 = rowptr[row], e1 = rowptr[row + 1];
  if (e1 <= e0) return;                           // uniform per sub-group
  const int f0 = sl * 8;
  const bool fv = f0 < F;
  const int nq = F - f0;                          // this lane's valid features: min(8, nq)
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (fv) {
    raw8_to_f32<T>(load_raw8<T>(A, (size_t)row * lda + f0), a);
#pragma unroll
    for (int q = 0; q < 8; ++q) a[q] = q < nq ? a[q] : 0.f;
  }
  const float rs = (last && rscale) ? rscale[row] : 1.f;
  int nxj = col[min(e0 + sl, e1 - 1)];
  for (int e = e0; e < e1; e += L) {
    const int myj = nxj;
    nxj = col[min(e + L + sl, e1 - 1)];
    const int cnt = min(L, e1 - e);
    const bool mine = sl < cnt;
    // loaded beside the gathers, used at the store
    const float mycs = (last && cscale && mine) ? cscale[myj] : 1.f;
    const float prev = (!first && mine) ? out[e + sl] : 0.f;
    float res = 0.f;
    for (int k = 0; k < cnt; k += 8) {
      int j[8];
      sub_bcast<L, 8>(myj, sub_base, k, j);
      float p[8];
      if (fv) {
        Raw8<T> r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (k + u < cnt) r[u] = load_raw8<T>(B, (size_t)j[u] * ldb + f0);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          p[u] = 0.f;
          if (k + u < cnt) {
            float b[8];
            raw8_to_f32<T>(r[u], b);
            // (padding columns of B may hold anything: they are not multiplied)
#pragma unroll
            for (int q = 0; q < 8; ++q) p[u] = fmaf(a[q], q < nq ? b[q] : 0.f, p[u]);
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) p[u] = 0.f;
      }
      // exchange tree over the lanes sl ^ 4, sl ^ 2, sl ^ 1: edge (sl & 7) stays
      const bool b4 = sl & 4, b2 = sl & 2, b1 = sl & 1;
      float s4[4], s2[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float keep = b4 ? p[i + 4] : p[i], send = b4 ? p[i] : p[i + 4];
        s4[i] = keep + __shfl_xor(send, 4, 64);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float keep = b2 ? s4[i + 2] : s4[i], send = b2 ? s4[i] : s4[i + 2];
        s2[i] = keep + __shfl_xor(send, 2, 64);
      }
      float s = (b1 ? s2[1] : s2[0]) + __shfl_xor(b1 ? s2[0] : s2[1], 1, 64);
#pragma unroll
      for (int off = 8; off < L; off <<= 1) s += __shfl_xor(s, off, 64);
      if ((sl >> 3) == (k >> 3)) res = s;
    }
    if (mine) {
      const float v = prev + res;
      out[e + sl] = last ? (rs * mycs) * v : v;
    }
  }
}

// ---------------------------------------------------------------- launchers
// (lane dispatch, grid, type tables and the slab walk: gnn_launch.h)

// No allocation and no synchronisation: capturable into a hipGraph.  Return codes: see
// cgnn_api.h.
extern "C" int gnn_launch_wspmm(const int* rowptr, const int* col, const float* val, const int* eperm,
                                const void* X, void* Y, const float* rscale, const float* cscale,
                                const float* bias, int n_rows, int F, int ldx, int ldy, int xt, int yt, int relu,
                                hipStream_t st) {
  if (F < 0 || !stride_ok(ldx, F) || !stride_ok(ldy, F)) return -3;
  if (!pair_ok(xt, yt)) return -5;
  if (n_rows <= 0) return 0;
  // one launch writing the columns [0, wc) of y, fc features among them
  auto slab = [&](const void* x, void* y, const float* b, int fc, int wc) {
    return with_lanes(std::max(fc, wc), [&](auto l) {
      constexpr int L = decltype(l)::value;
      return with_pair(xt, yt, [&](auto tx, auto ty) {
        hipLaunchKernelGGL((wspmm_kernel<L, decltype(tx)::value, decltype(ty)::value>), dim3(blocks(L, n_rows)),
                           dim3(256), 0, st, rowptr, col, val, eperm, x, y, rscale, cscale, b, n_rows, fc, ldx, ldy,
                           relu, wc);
        return (int)hipGetLastError();
      });
    });
  };
  // a row within one slab, apart from the walk: with F == 0 it keeps the caller's bias
  // pointer, which the walk's padding-only rule would turn into null
  if (ldy <= kSlab) return slab(X, Y, bias, F, ldy);
  return for_slabs(F, ldy, [&](int c0, int fc, int wc) {
    return slab(in_at(X, xt, c0, fc), out_at(Y, yt, c0), in_or_null(bias, c0, fc), fc, wc);
  });
}

// A and B share the storage type t.  The feature slabs run in stream order; the kernel's
// first / last turn them into one ordered sum per edge.
extern "C" int gnn_launch_sddmm(const int* rowptr, const int* col, const void* A, const void* B, float* out,
                                const float* rscale, const float* cscale, int n_rows, int F, int lda, int ldb,
                                int t, hipStream_t st) {
  if (F <= 0 || !stride_ok(lda, F) || !stride_ok(ldb, F)) return -3;
  if (!type_ok(t)) return -5;
  if (n_rows <= 0) return 0;
  return for_slabs(F, F, [&](int c0, int fc, int) {
    const void* a = in_at(A, t, c0, fc);
    const void* b = in_at(B, t, c0, fc);
    const int first = c0 == 0, last = c0 + kSlab >= F;
    return with_lanes(fc, [&](auto l) {
      constexpr int L = decltype(l)::value;
      return with_type(t, [&](auto tt) {
        hipLaunchKernelGGL((sddmm_kernel<L, decltype(tt)::value>), dim3(blocks(L, n_rows)), dim3(256), 0, st, rowptr,
                           col, a, b, out, rscale, cscale, n_rows, fc, lda, ldb, first, last);
        return (int)hipGetLastError();
      });
    });
  });
}
