// Host-side launch arithmetic of the row-per-sub-group CSR kernels (spmm in gnn_sparse.hip,
// gnn_wspmm.hip, gnn_pool.hip, gnn_espmm.hip), defined once.  A new kernel on this mapping
// gets its launcher from here.
//
// The mapping: wave64, 256-thread blocks, a sub-group of L lanes owns one CSR row and each
// lane 8 consecutive features, L = 8 / 16 / 32 / 64 for widths up to 64 / 128 / 256 / 512
// columns.  A wider row runs as one launch per slab of 512 columns, in stream order.
// A launch writes the columns [0, wc) of the output pointer it is given (wc <= 512): the
// fc <= wc feature columns of its slab, then zero padding up to the row stride.
//
// Host only: plain functions and function templates taking a callable; no device code.
#pragma once
#include <algorithm>
#include <cstddef>
#include <type_traits>

namespace cgnn {
namespace launch {

constexpr int kSlab = 512;

// a compile-time int handed to a generic callable: `constexpr int L = decltype(l)::value`
template <int V>
using Const = std::integral_constant<int, V>;

// fn(Const<L>) for the lane count L of a launch of width w = max(features, written columns);
// returns fn's result, or -1 for a width no sub-group covers
template <class Fn>
int with_lanes(int w, Fn&& fn) {
  if (w <= 64) return fn(Const<8>{});
  if (w <= 128) return fn(Const<16>{});
  if (w <= 256) return fn(Const<32>{});
  if (w <= 512) return fn(Const<64>{});
  return -1;
}

// 256-thread blocks for n rows: 4 waves of 64 / L sub-groups, rp rows per sub-group
constexpr int blocks(int L, int n, int rp = 1) {
  const int rpb = 4 * (64 / L) * rp;
  return (n + rpb - 1) / rpb;
}

// a row stride the 16-byte accesses can use, holding F features
constexpr bool stride_ok(int ld, int F) { return ld > 0 && ld % 8 == 0 && F <= ld; }

// element-type codes: 0 fp32, 1 bf16, 2 fp16
constexpr size_t elem_size(int t) { return t == 0 ? 4 : 2; }

// fn(Const<t>) for an element type, or -5
template <class Fn>
int with_type(int t, Fn&& fn) {
  if (t == 0) return fn(Const<0>{});
  if (t == 1) return fn(Const<1>{});
  if (t == 2) return fn(Const<2>{});
  return -5;
}

inline bool type_ok(int t) { return with_type(t, [](auto) { return 0; }) == 0; }

// fn(Const<in>, Const<out>) for the (input, output) type pairs of the kernels that
// accumulate in fp32 and store either the input's type or fp32; -5 for any other pair
template <class Fn>
int with_pair(int in, int out, Fn&& fn) {
  if (in == 1 && out == 1) return fn(Const<1>{}, Const<1>{});
  if (in == 1 && out == 0) return fn(Const<1>{}, Const<0>{});
  if (in == 2 && out == 2) return fn(Const<2>{}, Const<2>{});
  if (in == 2 && out == 0) return fn(Const<2>{}, Const<0>{});
  if (in == 0 && out == 0) return fn(Const<0>{}, Const<0>{});
  return -5;
}

inline bool pair_ok(int in, int out) { return with_pair(in, out, [](auto, auto) { return 0; }) == 0; }

// The slab walk: fn(c0, fc, wc) for every 512-column slab [c0, c0 + wc) of a row of `width`
// written columns that holds F features, fc = max(0, min(512, F - c0)) of them in this slab;
// stops at the first nonzero code.  Slabs past the features (fc == 0) write padding only.
// A row within one slab is the walk's only step, with c0 = 0, fc = F, wc = width.
// A launcher that writes two widths passes their maximum and derives the other one.
template <class Fn>
int for_slabs(int F, int width, Fn&& fn) {
  for (int c0 = 0; c0 < width; c0 += kSlab) {
    const int fc = std::max(0, std::min(kSlab, F - c0));
    const int wc = std::min(kSlab, width - c0);
    if (const int rc = fn(c0, fc, wc)) return rc;
  }
  return 0;
}

// A slab's view of an input: offset by c0 only when the slab holds features (fc != 0).  A
// padding-only slab reads nothing, and its c0 may lie past the input's row stride.  Null
// stays null.
inline const void* in_at(const void* p, int t, int c0, int fc) {
  return p && fc ? static_cast<const char*>(p) + c0 * elem_size(t) : p;
}
template <class T>
const T* in_at(const T* p, int c0, int fc) {
  return p && fc ? p + c0 : p;
}
// the same for a per-column vector the kernel tests for null (a bias): none without features
template <class T>
const T* in_or_null(const T* p, int c0, int fc) {
  return p && fc ? p + c0 : nullptr;
}
// a slab's view of an output (offsets are multiples of 512 elements: 16-byte aligned)
inline void* out_at(void* p, int t, int c0) { return static_cast<char*>(p) + c0 * elem_size(t); }

}  // namespace launch
}  // namespace cgnn
