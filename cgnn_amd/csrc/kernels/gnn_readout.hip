// GNN track (beyond the reference): graph-level readout for MI355X -- the reduction of the
// contiguous node rows of each graph of a block-diagonal batch to one row, and its reverse.
//
//   seg_reduce_kernel  Y[s,f]   = rscale[s] * sum_i X[i,f]              (sum)
//                      Y[s,f]   = max (or min) over i of X[i,f]         (max / min)
//                      arg[s,f] = the row i that supplied Y[s,f], or arg_in[i,f]
//                      over the rows i = ptr[s] .. ptr[s+1] - 1 of X [*, ldx]
//   seg_bcast_kernel   out[i,f] = rscale[s] * U[s,f]                    with s = seg_id[i]
//                      out[i,f] = arg[s,f] == i ? U[s,f] : 0            (with arg)
//
// ptr is int32 [S+1], starts at 0 and never decreases.  The rows of a segment are contiguous:
// there are no column ids to load or broadcast, the row addresses come from the loop counter.
//
// Contract of the sum.  fp32 accumulation; the rows are taken in steps of 8, then (at most
// once) 4, then single rows, the rows of a step loaded before its first add, and a step adds
// ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)) (resp. (a0 + a1) + (a2 + a3), a0) to the
// running sum: the order of the adds is a fixed function of the segment's length alone, not
// of its position, the grid or the other segments.  One product with rscale[s] (null: 1) in
// fp32 and one rounding to the output type.
//
// Contract of max / min: pool_fwd_kernel's rule (gnn_pool.hip).  Rows are scanned in order; a
// candidate replaces the running best only when it is strictly better (> for max, < for min)
// or when it is NaN and the best is not.  Ties go to the first row of the segment holding the
// value, a NaN propagates and arg is the first NaN row.  The output has the input's storage
// type: the value is a copy of an input element, exact in every type.  arg (optional) is the
// row index i; with arg_in (int32 [*, ldarg_in]) it is arg_in[i,f] instead, so that a second
// pass over partial results hands the first pass's indices through.
//
// An empty segment gives Y = 0, arg = -1, and so do the padding columns F <= f < ld.  No load
// sits outside [ptr[s], ptr[s+1]): an input without rows may pass a null X.
//
// Mapping (gnn_launch.h's): wave64, a sub-group of L lanes owns one output row, each lane 8
// consecutive features, L = 8 / 16 / 32 / 64 for widths up to 64 / 128 / 256 / 512; wider
// rows run as 512-column slabs in the launchers.  Eight row loads are in flight per lane.
//
// Two levels.  One sub-group per graph would leave the device idle on a few long graphs, so
// the host splits long segments into chunks of R rows counted from the segment's own start
// (ops.READOUT_CHUNK) and runs the kernel twice: over the chunks into partial rows, then over
// each graph's partial rows (gnn/readout.py).  Both passes are this kernel; a graph's result
// stays a function of its own rows only.
//
// Determinism: no atomics; nothing depends on the grid, on the other rows of the launch or
// on the run.
#include "cgnn_common.h"
#include "cgnn_api.h"
#include "gnn_gather.h"
#include "gnn_launch.h"

using namespace cgnn;
using namespace cgnn::gather;
using namespace cgnn::launch;

namespace {

// (Raw8, load_raw8, raw8_to_f32, store8: gnn_gather.h)

enum { kSum = 0, kMax = 1, kMin = 2 };

// the N rows at element offsets off, off + ldx, ... added to acc as one balanced term; the N
// rows are loaded before the first add
template <int T, int N>
__device__ __forceinline__ void sum_step(const void* __restrict__ X, size_t off, int ldx, float* acc) {
  Raw8<T> r[N];
#pragma unroll
  for (int u = 0; u < N; ++u) r[u] = load_raw8<T>(X, off + (size_t)u * ldx);
  float a[N][8];
#pragma unroll
  for (int u = 0; u < N; ++u) raw8_to_f32<T>(r[u], a[u]);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    if (N == 8) acc[q] += ((a[0][q] + a[1][q]) + (a[2][q] + a[3][q])) + ((a[4][q] + a[5][q]) + (a[6][q] + a[7][q]));
    else if (N == 4) acc[q] += (a[0][q] + a[1][q]) + (a[2][q] + a[3][q]);
    else acc[q] += a[0][q];
  }
}

// the rows i .. i + N - 1 offered to the running best in that order (pool_step's rule), the
// N rows loaded before the first compare
template <int T, int N, bool MIN>
__device__ __forceinline__ void best_step(const void* __restrict__ X, size_t off, int ldx, int i, float* best,
                                          int* bi) {
  Raw8<T> r[N];
#pragma unroll
  for (int u = 0; u < N; ++u) r[u] = load_raw8<T>(X, off + (size_t)u * ldx);
#pragma unroll
  for (int u = 0; u < N; ++u) {
    float c[8];
    raw8_to_f32<T>(r[u], c);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const bool take = (MIN ? c[q] < best[q] : c[q] > best[q]) | ((c[q] != c[q]) & (best[q] == best[q]));
      best[q] = take ? c[q] : best[q];
      bi[q] = take ? i + u : bi[q];
    }
    // one row's compare masks at a time: hoisted together, the masks of all N rows do not fit
    // the scalar registers and spill
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int T, int N, int OP>
__device__ __forceinline__ void seg_step(const void* __restrict__ X, size_t off, int ldx, int i, float* v, int* bi) {
  if (OP == kSum) sum_step<T, N>(X, off, ldx, v);
  else best_step<T, N, OP == kMin>(X, off, ldx, i, v, bi);
}

}  // namespace

// wy / wa: the columns of Y / arg this launch writes from its base (pool_fwd_kernel's); the
// columns [F, wy) of Y are written 0 and the columns [F, wa) of arg -1.  rscale is read by the
// sum only, arg_in / arg by max / min only; each may be null.
template <int L, int TIN, int TOUT, int OP>
__global__ __launch_bounds__(256) void seg_reduce_kernel(
    const int* __restrict__ ptr, const void* __restrict__ X, void* __restrict__ Y, const float* __restrict__ rscale,
    const int* __restrict__ arg_in, int* __restrict__ arg, int S, int F, int ldx, int ldy, int ldarg_in, int ldarg,
    int wy, int wa) {
  constexpr int RPW = 64 / L;
  const int lane = threadIdx.x & 63;
  const int sub = lane / L, sl = lane - sub * L;
  const unsigned blk = xcd_remap(blockIdx.x, gridDim.x);
  const int row = (blk * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + sub;
  if (row >= S) return;                           // no cross-lane traffic below
  const int f0 = sl * 8;
  // max / min start from the identity of the reduction with index -1: a candidate equal to it
  // never replaces it, so an index still -1 after a non-empty segment means every row held
  // that value, and the first row is the answer
  float v[8];
  int bi[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    v[q] = OP == kSum ? 0.f : (OP == kMin ? __builtin_inff() : -__builtin_inff());
    bi[q] = -1;
  }
  const int r0 = ptr[row], r1 = ptr[row + 1];
  if (f0 < F) {
    int i = r0;
    size_t off = (size_t)r0 * ldx + f0;
    for (; i + 8 <= r1; i += 8, off += (size_t)8 * ldx) seg_step<TIN, 8, OP>(X, off, ldx, i, v, bi);
    for (; i + 4 <= r1; i += 4, off += (size_t)4 * ldx) seg_step<TIN, 4, OP>(X, off, ldx, i, v, bi);
    for (; i < r1; ++i, off += ldx) seg_step<TIN, 1, OP>(X, off, ldx, i, v, bi);
  }
  const bool any = r1 > r0;
  if (f0 < wy) {
    const float rs = (OP == kSum && rscale) ? rscale[row] : 1.f;
    float y[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) y[q] = (any && f0 + q < F) ? (OP == kSum ? v[q] * rs : v[q]) : 0.f;
    store8<TOUT>(Y, (size_t)row * ldy + f0, y);
  }
  if (OP != kSum && arg && f0 < wa) {
    int a[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    if (any && f0 < F) {
#pragma unroll
      for (int q = 0; q < 8; ++q) a[q] = bi[q] < 0 ? r0 : bi[q];
      if (arg_in) {                               // uniform; a ragged last lane reads column F - 1
#pragma unroll
        for (int q = 0; q < 8; ++q) a[q] = arg_in[(size_t)a[q] * ldarg_in + min(f0 + q, F - 1)];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) a[q] = f0 + q < F ? a[q] : -1;
    }
    int4* p = reinterpret_cast<int4*>(arg + (size_t)row * ldarg + f0);
    p[0] = make_int4(a[0], a[1], a[2], a[3]);
    p[1] = make_int4(a[4], a[5], a[6], a[7]);
  }
}

// One sub-group per node row i.  wcols as in wspmm_kernel: the columns [F, wcols) are
// written 0.  ARG: rscale is not read.
template <int L, int TIN, int TOUT, bool ARG>
__global__ __launch_bounds__(256) void seg_bcast_kernel(
    const int* __restrict__ seg_id, const void* __restrict__ U, const float* __restrict__ rscale,
    const int* __restrict__ arg, void* __restrict__ out, int n, int F, int ldu, int ldarg, int ldo, int wcols) {
  constexpr int RPW = 64 / L;
  const int lane = threadIdx.x & 63;
  const int sub = lane / L, sl = lane - sub * L;
  const unsigned blk = xcd_remap(blockIdx.x, gridDim.x);
  const int row = (blk * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + sub;
  const int f0 = sl * 8;
  if (row >= n || f0 >= wcols) return;
  float y[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (f0 < F) {
    const int s = seg_id[row];
    float u[8];
    raw8_to_f32<TIN>(load_raw8<TIN>(U, (size_t)s * ldu + f0), u);
    if (ARG) {
      const int4* p = reinterpret_cast<const int4*>(arg + (size_t)s * ldarg + f0);
      const int4 a0 = p[0], a1 = p[1];
      const int a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
      for (int q = 0; q < 8; ++q) y[q] = (f0 + q < F && a[q] == row) ? u[q] : 0.f;
    } else {
      const float rs = rscale ? rscale[s] : 1.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) y[q] = f0 + q < F ? u[q] * rs : 0.f;
    }
  }
  store8<TOUT>(out, (size_t)row * ldo + f0, y);
}

// ---------------------------------------------------------------- launchers
// (lane dispatch, grid, type tables and the slab walk: gnn_launch.h)

namespace {

// with_pair's five (input, output) pairs and fp32 -> bf16 / fp16, which the second pass of a
// two-level sum needs (fp32 partials into a 16-bit result)
template <class Fn>
int with_sum_pair(int in, int out, Fn&& fn) {
  if (in == 0 && out == 1) return fn(Const<0>{}, Const<1>{});
  if (in == 0 && out == 2) return fn(Const<0>{}, Const<2>{});
  return with_pair(in, out, fn);
}

// fn(Const<tin>, Const<tout>, Const<op>) for every compiled (types, op): the seven pairs for
// the sum, the three same-type pairs for max / min; -5 for another pair, then -1 for an op
// outside {0, 1, 2}
template <class Fn>
int with_reduce(int tin, int tout, int op, Fn&& fn) {
  if (op == kMax || op == kMin) {
    if (tin != tout) return -5;
    return with_type(tin, [&](auto t) {
      return op == kMax ? fn(t, t, Const<kMax>{}) : fn(t, t, Const<kMin>{});
    });
  }
  return with_sum_pair(tin, tout, [&](auto ti, auto to) { return op == kSum ? fn(ti, to, Const<kSum>{}) : -1; });
}

}  // namespace

// Y [S, ldy] (and arg [S, ldarg]) from the segments ptr [S + 1] of X [*, ldx].  op: 0 sum,
// 1 max, 2 min.  rscale (fp32 [S], the sum's) and arg_in / arg (int32, max / min's) may be
// null; what the other ops do not read is ignored.  X may be null when every segment is
// empty.  No allocation and no synchronisation: capturable into a hipGraph.  Return codes:
// see cgnn_api.h.
extern "C" int gnn_launch_seg_reduce(const int* ptr, const void* X, void* Y, const float* rscale, const int* arg_in,
                                     int* arg, int S, int F, int ldx, int ldy, int ldarg_in, int ldarg, int tin,
                                     int tout, int op, hipStream_t st) {
  if (F < 0 || !stride_ok(ldx, F) || !stride_ok(ldy, F)) return -3;
  if (arg && !stride_ok(ldarg, F)) return -3;
  if (arg_in && !stride_ok(ldarg_in, F)) return -3;
  if (const int rc = with_reduce(tin, tout, op, [](auto, auto, auto) { return 0; }); rc == -5) return rc;
  if (S <= 0) return 0;
  if (!ptr || !Y) return -3;
  if (op != kSum && op != kMax && op != kMin) return -1;
  int* const aout = op == kSum ? nullptr : arg;
  const int* const ain = aout ? arg_in : nullptr;
  const int lda = aout ? ldarg : 0;
  return for_slabs(F, std::max(ldy, lda), [&](int c0, int fc, int) {
    const int wy = std::max(0, std::min(kSlab, ldy - c0));
    const int wa = std::max(0, std::min(kSlab, lda - c0));
    const void* x = in_at(X, tin, c0, fc);
    void* y = wy ? out_at(Y, tout, c0) : Y;
    const int* ai = in_at(ain, c0, fc);
    int* a = aout && wa ? aout + c0 : nullptr;
    return with_lanes(std::max({fc, wy, wa}), [&](auto l) {
      constexpr int L = decltype(l)::value;
      return with_reduce(tin, tout, op, [&](auto ti, auto to, auto o) {
        hipLaunchKernelGGL((seg_reduce_kernel<L, decltype(ti)::value, decltype(to)::value, decltype(o)::value>),
                           dim3(blocks(L, S)), dim3(256), 0, st, ptr, x, y, rscale, ai, a, S, fc, ldx, ldy, ldarg_in,
                           ldarg, wy, wa);
        return (int)hipGetLastError();
      });
    });
  });
}

// out [n, ldo] from U [S, ldu] and seg_id [n]: the scaled copy (rscale fp32 [S] or null), or
// with arg [S, ldarg] the copy masked to the rows arg names.  The (U, out) type pairs are
// gnn_launch_wspmm's.  Capturable like the reduction.
extern "C" int gnn_launch_seg_bcast(const int* seg_id, const void* U, const float* rscale, const int* arg, void* out,
                                    int n, int F, int ldu, int ldarg, int ldo, int tin, int tout, hipStream_t st) {
  if (F < 0 || !stride_ok(ldu, F) || !stride_ok(ldo, F)) return -3;
  if (arg && !stride_ok(ldarg, F)) return -3;
  if (!pair_ok(tin, tout)) return -5;
  if (n <= 0) return 0;
  if (!seg_id || !U || !out) return -3;
  return for_slabs(F, ldo, [&](int c0, int fc, int wc) {
    const void* u = in_at(U, tin, c0, fc);
    const int* a = in_at(arg, c0, fc);
    void* o = out_at(out, tout, c0);
    return with_lanes(std::max(fc, wc), [&](auto l) {
      constexpr int L = decltype(l)::value;
      return with_pair(tin, tout, [&](auto ti, auto to) {
        constexpr int TI = decltype(ti)::value, TO = decltype(to)::value;
        hipLaunchKernelGGL((arg ? seg_bcast_kernel<L, TI, TO, true> : seg_bcast_kernel<L, TI, TO, false>),
                           dim3(blocks(L, n)), dim3(256), 0, st, seg_id, u, rscale, a, o, n, fc, ldu, ldarg, ldo, wc);
        return (int)hipGetLastError();
      });
    });
  });
}
