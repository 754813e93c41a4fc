// GNN track (beyond the reference): message passing with a feature vector per edge.
//
//   espmm_kernel  Y[i,:F] = sum_{e in row i} w_e * m_e, with p(e) = eperm ? eperm[e] : e,
//                 w_e = val ? val[p(e)] : 1 and
//                   add:  m_e = X[col[e],:F] + E[p(e),:F]   (max(., 0) with relu)
//                   mul:  m_e = X[col[e],:F] * E[p(e),:F]
//                   X == nullptr:  m_e = E[p(e),:F], the sum of edge rows per destination.
//                 CSR aggregate that streams one edge row beside every gathered node row.
//                 Over the transposed CSR with its edge permutation it is the gradient
//                 with respect to the node rows.
//   egrad_kernel  over the forward CSR, row i's g = dY[i,:F] in registers; per edge e = (i, j):
//                   dE[e,:F] = w_e * g * d,  d = 1 (add), 1[X[j] + E[e] > 0] (add + relu),
//                                            X[j] (mul)
//                   dval[e]  = <g, m_e>      (m_e as in the forward, after the ReLU)
//                 the gradient with respect to the edge rows and the edge values.
//
// Mapping (gnn_launch.h's): wave64, a sub-group of L lanes owns one row, each lane owns 8
// consecutive features (one 16-byte load per bf16 / fp16 row), L = 8 / 16 / 32 / 64 for
// widths up to 64 / 128 / 256 / 512; wider rows run as 512-column slabs in the launchers.
// The ids and values of a chunk of L edges come with one coalesced load per lane,
// requested one chunk ahead at a clamped address, and are broadcast inside the sub-group.
// X, E, Y, dY, dE share one storage type; val / dval and the accumulation are fp32.  The
// offset of an edge row is computed in 64 bits (nnz * lde passes 2^31 on large graphs).
//
// Determinism: per row and feature the forward is ONE chain of fmaf(w, m, acc) in edge
// order; dE[e] is a product of three numbers; dval[e] is one fmaf chain per lane in feature
// order followed by a fixed exchange tree over the L lanes, and across column slabs an
// ordered sum in stream order.  None depends on the grid, on the other rows of the launch
// or on the run.  No atomics.
//
// Empty inputs: a row with e0 == e1 dereferences none of col / val / eperm / E (every edge
// load sits behind the row's e1 > e0 test and is clamped into [e0, e1)).
#include "cgnn_common.h"
#include "cgnn_api.h"
#include "gnn_gather.h"
#include "gnn_launch.h"

using namespace cgnn;
using namespace cgnn::gather;
using namespace cgnn::launch;

namespace {

// MODE of both kernels
constexpr int kAdd = 0, kMul = 1, kEdgeOnly = 2;

// rows in flight per lane and operand: fp32 rows take two registers quads each
template <int T, int MODE>
constexpr int step_rows() {
  return (T == 0 && MODE != kEdgeOnly) ? 4 : 8;
}

// acc[q] = fmaf(w[u], m_u[q], acc[q]) for u = 0..N-1 in that order, the rows of all N edges
// loaded before the first multiply-add.  pe: the edge rows' indices
template <int T, int MODE, int N>
__device__ __forceinline__ void egather_step(const void* __restrict__ X, const void* __restrict__ E, const int* j,
                                             const int* pe, const int* w, int ldx, int lde, int f0, bool relu,
                                             float* acc) {
  Raw8<T> rx[N], re[N];
  if (MODE != kEdgeOnly) {
#pragma unroll
    for (int u = 0; u < N; ++u) rx[u] = load_raw8<T>(X, (size_t)j[u] * ldx + f0);
  }
#pragma unroll
  for (int u = 0; u < N; ++u) re[u] = load_raw8<T>(E, (size_t)pe[u] * lde + f0);
#pragma unroll
  for (int u = 0; u < N; ++u) {
    float m[8];
    raw8_to_f32<T>(re[u], m);
    if (MODE != kEdgeOnly) {
      float x[8];
      raw8_to_f32<T>(rx[u], x);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (MODE == kMul) m[q] = x[q] * m[q];
        else m[q] = relu ? fmaxf(x[q] + m[q], 0.f) : x[q] + m[q];
      }
    }
    const float wu = __int_as_float(w[u]);
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = fmaf(wu, m[q], acc[q]);
  }
}

}  // namespace

// wcols: output columns this launch writes from its base (the row stride for a whole-row
// launch, the slab width for a column-slab launch); columns [F, wcols) are written 0
template <int L, int T, int MODE>
__global__ __launch_bounds__(256) void espmm_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ val,
    const int* __restrict__ eperm, const void* __restrict__ X, const void* __restrict__ E, void* __restrict__ Y,
    int n_rows, int F, int ldx, int lde, int ldy, int relu, int wcols) {
  constexpr int RPW = 64 / L;
  constexpr int NS = step_rows<T, MODE>();
  const int lane = threadIdx.x & 63;
  const int sub = lane / L, sl = lane - sub * L, sub_base = sub * L;
  const unsigned blk = xcd_remap(blockIdx.x, gridDim.x);
  const int row = (blk * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + sub;
  const bool rv = row < n_rows;
  const int f0 = sl * 8;
  const bool fv = rv && f0 < F;
  const bool rl = relu != 0;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int e0 = rv ? rowptr[row] : 0, e1 = rv ? rowptr[row + 1] : 0;
  if (e1 > e0) {                                  // uniform per sub-group
    // lane sl's edge of a chunk: its source id, edge-row index and weight, from addresses
    // clamped into the row (unconditional loads: a "load or 0" would branch and wait)
    auto edge = [&](int e, int& j, int& p, float& v) {
      const int ec = min(e, e1 - 1);
      j = MODE != kEdgeOnly ? col[ec] : 0;
      p = eperm ? eperm[ec] : ec;
      v = val ? val[p] : 1.f;
    };
    int nxj, nxp;
    float nxv;
    edge(e0 + sl, nxj, nxp, nxv);
    for (int e = e0; e < e1; e += L) {
      const int myj = nxj, myp = nxp;
      const int myw = __float_as_int(nxv);
      edge(e + L + sl, nxj, nxp, nxv);            // the next chunk, under this chunk's gathers
      const int cnt = min(L, e1 - e);
      int k = 0;
      for (; k + NS <= cnt; k += NS) {
        int j[NS], p[NS], w[NS];
        if (MODE != kEdgeOnly) sub_bcast<L, NS>(myj, sub_base, k, j);
        sub_bcast<L, NS>(myp, sub_base, k, p);
        sub_bcast<L, NS>(myw, sub_base, k, w);
        if (fv) egather_step<T, MODE, NS>(X, E, j, p, w, ldx, lde, f0, rl, acc);
      }
      if (NS == 8) {
        for (; k + 4 <= cnt; k += 4) {
          int j[4], p[4], w[4];
          if (MODE != kEdgeOnly) sub_bcast<L, 4>(myj, sub_base, k, j);
          sub_bcast<L, 4>(myp, sub_base, k, p);
          sub_bcast<L, 4>(myw, sub_base, k, w);
          if (fv) egather_step<T, MODE, 4>(X, E, j, p, w, ldx, lde, f0, rl, acc);
        }
      }
      for (; k < cnt; ++k) {
        int j[1], p[1], w[1];
        if (MODE != kEdgeOnly) sub_bcast<L, 1>(myj, sub_base, k, j);
        sub_bcast<L, 1>(myp, sub_base, k, p);
        sub_bcast<L, 1>(myw, sub_base, k, w);
        if (fv) egather_step<T, MODE, 1>(X, E, j, p, w, ldx, lde, f0, rl, acc);
      }
    }
  }
  if (!rv || f0 >= wcols) return;
  float y[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) y[q] = f0 + q < F ? acc[q] : 0.f;
  store8<T>(Y, (size_t)row * ldy + f0, y);
}

// dE rows and dval for the edges of row i.  Row i's slice of dY stays in registers (zero
// past F).  Eight edges at a time: their X and E rows are loaded (only those the requested
// outputs need), each edge's dE row is stored whole by the sub-group (lane sl's 16 bytes at
// column f0: one coalesced row), and the 8 partial dot products of a lane go through
// sddmm_kernel's exchange tree: lanes sl ^ 4, sl ^ 2, sl ^ 1 halve the values a lane keeps
// at every level, the levels sl ^ 8 .. sl ^ L/2 add single values, and the lane whose index
// in the sub-group is the edge's index in the chunk keeps the result.  A chunk of L dval
// results is stored with ONE coalesced write, dval[e + sl].
// first: a width above 512 runs as launches over 512-column slabs in stream order; a launch
// that is not the first adds to the sum its predecessor left in dval[e] -- an ordered sum.
// wcols: the dE columns this launch writes from its base; [F, wcols) are written 0.
template <int L, int T, int MODE>
__global__ __launch_bounds__(256) void egrad_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ val,
    const void* __restrict__ dY, const void* __restrict__ X, const void* __restrict__ E, void* __restrict__ dE,
    float* __restrict__ dval, int n_rows, int F, int lddy, int ldx, int lde, int ldde, int relu, int wcols,
    int first) {
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
  const bool rl = MODE == kAdd && relu != 0;
  const bool want_de = dE != nullptr, want_dv = dval != nullptr;
  // what the requested outputs read: dE needs X for the ReLU mask and the product, dval
  // needs m_e
  const bool need_x = MODE == kMul || (MODE == kAdd && (rl || want_dv));
  const bool need_e = want_dv || rl;
  const bool wr = want_de && f0 < wcols;
  float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (fv) {
    raw8_to_f32<T>(load_raw8<T>(dY, (size_t)row * lddy + f0), g);
#pragma unroll
    for (int q = 0; q < 8; ++q) g[q] = q < nq ? g[q] : 0.f;
  }
  auto edge = [&](int e, int& j, float& v) {
    const int ec = min(e, e1 - 1);
    j = MODE != kEdgeOnly ? col[ec] : 0;
    v = val ? val[ec] : 1.f;
  };
  int nxj;
  float nxv;
  edge(e0 + sl, nxj, nxv);
  for (int e = e0; e < e1; e += L) {
    const int myj = nxj;
    const int myw = __float_as_int(nxv);
    edge(e + L + sl, nxj, nxv);
    const int cnt = min(L, e1 - e);
    const bool mine = sl < cnt;
    const float prev = (want_dv && !first && mine) ? dval[e + sl] : 0.f;
    float res = 0.f;
    for (int k = 0; k < cnt; k += 8) {
      int j[8], w[8];
      if (MODE != kEdgeOnly) sub_bcast<L, 8>(myj, sub_base, k, j);
      sub_bcast<L, 8>(myw, sub_base, k, w);
      float p[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) p[u] = 0.f;
      if (fv) {
        Raw8<T> rx[8], re[8];
        if (MODE != kEdgeOnly && need_x) {
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (k + u < cnt) rx[u] = load_raw8<T>(X, (size_t)j[u] * ldx + f0);
        }
        if (need_e) {
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (k + u < cnt) re[u] = load_raw8<T>(E, (size_t)(e + k + u) * lde + f0);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (k + u < cnt) {
            // (padding columns of X and E may hold anything: they are masked below)
            float x[8], m[8], d[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = m[q] = 0.f;
            if (MODE != kEdgeOnly && need_x) raw8_to_f32<T>(rx[u], x);
            if (need_e) raw8_to_f32<T>(re[u], m);
            const float wu = __int_as_float(w[u]);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              if (MODE == kMul) {
                d[q] = x[q];
                m[q] = x[q] * m[q];
              } else if (MODE == kAdd) {
                const float s = x[q] + m[q];
                d[q] = (!rl || s > 0.f) ? 1.f : 0.f;
                m[q] = rl ? fmaxf(s, 0.f) : s;
              } else {
                d[q] = 1.f;
              }
            }
            if (want_dv) {
#pragma unroll
              for (int q = 0; q < 8; ++q) p[u] = fmaf(g[q], q < nq ? m[q] : 0.f, p[u]);
            }
            if (wr) {
              float o[8];
#pragma unroll
              for (int q = 0; q < 8; ++q) o[q] = q < nq ? (wu * g[q]) * d[q] : 0.f;
              store8<T>(dE, (size_t)(e + k + u) * ldde + f0, o);
            }
          }
        }
      } else if (wr) {
        // a lane past F inside the written width: the zero padding of the dE rows
        const float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (k + u < cnt) store8<T>(dE, (size_t)(e + k + u) * ldde + f0, o);
      }
      if (want_dv) {                              // uniform per launch
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
    }
    if (want_dv && mine) dval[e + sl] = prev + res;
  }
}

// ---------------------------------------------------------------- launchers
// (lane dispatch, grid, type table and the slab walk: gnn_launch.h)

// fn(Const<MODE>) for the MODE of both kernels: the sum of edge rows without X, else the op
template <class Fn>
static int with_mode(const void* X, int op, Fn&& fn) {
  if (X && op != 1) return fn(Const<kAdd>{});
  if (X) return fn(Const<kMul>{});
  return fn(Const<kEdgeOnly>{});
}

// op: 0 add, 1 mul; X may be null (the sum of edge rows; op and ldx are then ignored).
// No allocation and no synchronisation: capturable into a hipGraph.  Return codes: see
// cgnn_api.h.
extern "C" int gnn_launch_espmm(const int* rowptr, const int* col, const float* val, const int* eperm,
                                const void* X, const void* E, void* Y, int n_rows, int F, int ldx, int lde, int ldy,
                                int t, int op, int relu, hipStream_t st) {
  if (F < 0 || !E || !Y || !stride_ok(lde, F) || !stride_ok(ldy, F) || (X && !stride_ok(ldx, F))) return -3;
  if (relu && op == 1) return -3;
  if (!type_ok(t)) return -5;
  if (op != 0 && op != 1) return -1;
  if (n_rows <= 0) return 0;
  if (!X) relu = 0;
  return for_slabs(F, ldy, [&](int c0, int fc, int wc) {
    const void* x = in_at(X, t, c0, fc);
    const void* e = in_at(E, t, c0, fc);
    void* y = out_at(Y, t, c0);
    return with_mode(X, op, [&](auto m) {
      constexpr int MODE = decltype(m)::value;
      return with_lanes(std::max(fc, wc), [&](auto l) {
        constexpr int L = decltype(l)::value;
        return with_type(t, [&](auto tt) {
          hipLaunchKernelGGL((espmm_kernel<L, decltype(tt)::value, MODE>), dim3(blocks(L, n_rows)), dim3(256), 0, st,
                             rowptr, col, val, eperm, x, e, y, n_rows, fc, ldx, lde, ldy, relu, wc);
          return (int)hipGetLastError();
        });
      });
    });
  });
}

// dE (storage type t, [nnz, ldde]) and dval (fp32 [nnz]) may each be null, not both; X may
// be null (the forward summed edge rows).  E is required: it fixes the forward's operands
// even where the requested outputs do not read it.
extern "C" int gnn_launch_egrad(const int* rowptr, const int* col, const float* val, const void* dY, const void* X,
                                const void* E, void* dE, float* dval, int n_rows, int F, int lddy, int ldx, int lde,
                                int ldde, int t, int op, int relu, hipStream_t st) {
  if (F < 0 || !E || !dY || (!dE && !dval) || !stride_ok(lddy, F) || !stride_ok(lde, F) ||
      (X && !stride_ok(ldx, F)) || (dE && !stride_ok(ldde, F)))
    return -3;
  if (relu && op == 1) return -3;
  if (!type_ok(t)) return -5;
  if (op != 0 && op != 1) return -1;
  if (n_rows <= 0) return 0;
  if (!X) relu = 0;
  // the feature slabs in order (dval is their ordered sum), then any slab that holds only
  // padding columns of dE; the dE width of a slab is derived here (0 without dE)
  return for_slabs(F, std::max({F, dE ? ldde : 0, 1}), [&](int c0, int fc, int) {
    const int wc = dE ? std::max(0, std::min(kSlab, ldde - c0)) : 0;
    const void* dy = in_at(dY, t, c0, fc);
    const void* x = in_at(X, t, c0, fc);
    const void* e = in_at(E, t, c0, fc);
    void* de = dE ? out_at(dE, t, c0) : nullptr;
    float* dv = (fc || c0 == 0) ? dval : nullptr;
    if (!de && !dv) return 0;                     // neither dE columns nor dval in this slab
    if (!wc) de = nullptr;
    const int first = c0 == 0;
    return with_mode(X, op, [&](auto m) {
      constexpr int MODE = decltype(m)::value;
      return with_lanes(std::max(fc, wc), [&](auto l) {
        constexpr int L = decltype(l)::value;
        return with_type(t, [&](auto tt) {
          hipLaunchKernelGGL((egrad_kernel<L, decltype(tt)::value, MODE>), dim3(blocks(L, n_rows)), dim3(256), 0, st,
                             rowptr, col, val, dy, x, e, de, dv, n_rows, fc, lddy, ldx, lde, ldde, relu, wc, first);
          return (int)hipGetLastError();
        });
      });
    });
  });
}
