// The C ABI of the kernel library: every extern "C" launcher and query function of
// csrc/kernels/*.hip, declared exactly once.  Each .hip file and bindings.cpp include
// this header, so a definition that drifts from its declaration is a conflicting-types
// compile error, never a silent argument mismatch at link time (extern "C" symbols
// link by name alone).  Plain C++: bindings.cpp is not compiled as HIP.
// tests/test_native_abi_cpu.py checks that no definition escapes the header.
//
// Conventions.  Device pointers are raw; the library never allocates device memory.
// `st` is the stream every launch goes to.  An int-returning launcher returns
//    0   launched
//   >0   the hipError_t of the launch (hipGetLastError)
//   -1   no compiled variant covers the shape (template width, tile, head count)
//   -2   a size the kernels cannot serve: a row range or seed count out of bounds, LDS
//        need over the limit, a missing scratch buffer (cgnn_*, rff_*, gnn_sw_*)
//   -3   bad shape: a row stride that is no multiple of 8 or narrower than the row, a
//        width or class count over the kernel's limit, a required pointer missing
//   -4   the launch grid or the per-block row-id table would overflow
//   -5   an element-type pair (X, Y storage type) that is not compiled
// The *_supported / *_variant queries return 1 / 0 (or a variant number), the *_blocks,
// *_tiles, *_chunks, *_width, *_slots, *_waves queries a count, *_bytes / *_halfwords /
// *_floats / *_scratch / *_lds a buffer size; none of them launches anything.
// The argument semantics are documented beside each definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

extern "C" {

// ---- cgnn_kernels.hip: vector MMD, generator forward / backward, Adam, init
int cgnn_mmd_supported_d(int D);
int cgnn_mmd_mirror_slots(int D, int N);
int cgnn_launch_mmd_rows(int mode, int D, const float* xhat, const float* data, float* gpart, float* lpart, int N,
                         int R, int row_tiles, int n_chunks, int tpc, float gscale, int row_begin, int n_rows,
                         hipStream_t st, int mirror);
// all N rows (the engine's call)
int cgnn_launch_mmd(int mode, int D, const float* xhat, const float* data, float* gpart, float* lpart, int N, int R,
                    int row_tiles, int n_chunks, int tpc, float gscale, hipStream_t st, int mirror);
int cgnn_launch_loss_finalize(const float* lpart, int n_parts, float* tt, float* last, float* acc, float inv_n2,
                              int flags, float* hist, int hist_stride, const int* step_base, int step_off, int R,
                              hipStream_t st);
int cgnn_gen_supported_h(int H);
size_t cgnn_gen_fwd_lds(int D, int prog_stride);
int cgnn_launch_gen_fwd(const int* prog, int prog_stride, const float* params, int P, const float* data, float* xhat,
                        float* noise, int NS, float* xnorm, const uint32_t* keys, const int* step_base, int step_off,
                        int N, int D, int H, int R, hipStream_t st, int row0);
int cgnn_gen_bwd_blocks(int N);
size_t cgnn_gen_bwd_lds(int H, int max_in, int D, int prog_stride);
// 1 the per-sample kernels, 2 the level-scheduled ones (cgnn_staged.hip), 0 neither fits
int cgnn_gen_bwd_variant(int H, int max_in, int Dt, int prog_stride);
int cgnn_gen_staged_supported(int H, int max_in, int Dt);
int cgnn_launch_gen_bwd(const int* prog, int prog_stride, const float* params, int P, const float* xhat,
                        const float* noise, int NS, const float* gradp, int n_chunks, int R, int N, int D, int Dt,
                        int H, int max_in, float* gpart, hipStream_t st);
int cgnn_launch_adam(float* params, float* m, float* v, const float* gpart, int G, const int* prog, int prog_stride,
                     int P, const int* step_base, int step_off, float lr, float b1, float b2, float eps, int R,
                     hipStream_t st);
int cgnn_launch_init(float* params, float* m, float* v, const int* prog, int prog_stride, int P, const uint32_t* keys,
                     float init_std, int R, hipStream_t st);
int cgnn_launch_advance(int* step_base, int d_rng, int d_opt, hipStream_t st);

// ---- cgnn_staged.hip: level-scheduled generator kernels (wide graphs)
// out = {fwd_xg, bwd_xg, bwd_dg, W_fwd, W_bwd}; 0, or -1 when nothing fits
int cgnn_staged_plan(int Dt, int H, int max_in, int W, int extra, int* out);
int cgnn_staged_tiles(int N);
int cgnn_launch_gen_noise(const int* prog, int ps, const uint32_t* keys, const int* step_base, int step_off,
                          float* noise, int NS, int N, int D, int Dt, int R, int row0, hipStream_t st);
// the forward that draws its own noise (keys != nullptr); only the engine calls it
int cgnn_launch_gen_fwd_staged_draw(const int* prog, int ps, const int* sched, int ss, const float* params, int P,
                                    const float* data, float* xhat, float* noise, int NS, float* xnorm, int N, int D,
                                    int Dt, int H, int max_in, int R, int W, hipStream_t st, int force,
                                    const uint32_t* keys, const int* step_base, int step_off, int row0);
int cgnn_launch_gen_fwd_staged(const int* prog, int ps, const int* sched, int ss, const float* params, int P,
                               const float* data, float* xhat, const float* noise, int NS, float* xnorm, int N, int D,
                               int Dt, int H, int max_in, int R, int W, hipStream_t st, int force);
int cgnn_launch_gen_bwd_staged(const int* prog, int ps, const int* sched, int ss, const float* params, int P,
                               const float* xhat, const float* noise, int NS, const float* gradp, int n_chunks, int R,
                               int N, int D, int Dt, int H, int max_in, int W, float* gpart, float* dxs,
                               hipStream_t st, int force);

// ---- mmd_mfma.hip: matrix-core MMD
int cgnn_mmd_mfma_supported(int D);
int cgnn_mmd_mfma_row_blocks(int N);
int cgnn_launch_mmd_mfma_rows(int mode, int D, const float* xhat, const float* data, const float* xnorm,
                              const float* ynorm, float* gpart, float* lpart, int N, int R, int n_chunks, int tpc,
                              float gscale, int row_begin, int n_rows, hipStream_t st, int wide);
// all N rows, automatic kernel choice (the engine's call)
int cgnn_launch_mmd_mfma(int mode, int D, const float* xhat, const float* data, const float* xnorm,
                         const float* ynorm, float* gpart, float* lpart, int N, int R, int n_chunks, int tpc,
                         float gscale, hipStream_t st);

// ---- rff_kernels.hip: Fourier (random-feature) MMD
long rff_wide_scratch_floats(int N, int F, int R);
int rff_launch_freqs(float* W, const uint32_t* keys, const int* step_base, int step_off, int k, int D, int n_gamma,
                     int d_true, int R, hipStream_t st);
int rff_launch_fwd_bwd(int mode, const float* xhat, const float* data, const float* W, float* diff, float* loss_part,
                       float* grad, int N, int D, int F, int R, int k, float norm, hipStream_t st, int force_valu,
                       float* scratch, int force_wide);

// ---- cgnn_engine.hip: the native step engine; the handle is a cgnn::Engine*.  icfg /
// fcfg / ptrs are positional (EngineConfig and Engine in that file name every slot).
// These throw std::runtime_error instead of returning a code.
void* cgnn_engine_create(const int* icfg, const float* fcfg, const void* const* ptrs, hipStream_t st);
void cgnn_engine_destroy(void* e);
int cgnn_engine_gen_blocks(void* e);
int cgnn_engine_n_parts(void* e);
void cgnn_engine_init(void* e);
void cgnn_engine_tt(void* e);
void cgnn_engine_run(void* e, int kind, int steps, int chunk, int hist);

// ---- gnn_sparse.hip: SpMM family, fused SpMM + cross-entropy, elementwise, Adam
int gnn_launch_spmm(const int* rowptr, const int* col, const void* X, void* Y, const float* rscale, const float* bias,
                    int n_rows, int F, int ldx, int ldy, int xbf, int ybf, int relu, int unit_col, const float* init,
                    int ldi, const float* cscale, int init_rows, int short_rows, hipStream_t st);
int gnn_slab_sum(const float* P, long S, int W, float* stage, int G, float* out, const int* map, int* bump,
                 hipStream_t st);
int gnn_spmm_ce_blocks(int n_rows, int n_long);
int gnn_launch_bias_relu_dropout(void* H, const float* bias, long rows, int F, int ld, float p, uint32_t k0,
                                 uint32_t k1, uint32_t step, uint32_t row0, hipStream_t st);
int gnn_launch_relu_dropout_bwd(void* dH, const void* H, long n, float p, hipStream_t st);
int gnn_launch_spmm_ce(const int* rowptr, const int* col, const void* Z, const float* rscale, const float* bias,
                       const int* labels, const uint8_t* mask, float* stats, void* G, const float* init, int ldi,
                       int n_rows, int C, int ld, int mode, float inv_count, const int* gslot, int n_long,
                       hipStream_t st);
int gnn_launch_ell_build(const int* rowptr, const int* col, int* ell, int n_rows, hipStream_t st);
int gnn_launch_spmm_ell(const int* ell, const int* col, const void* X, void* Y, const float* rscale, int n_rows,
                        int F, int ldx, int ldy, long n_x_rows, const int* long_rows, int n_long, hipStream_t st);
int gnn_launch_spmm_fan(const int* rowptr, const int* col, const void* X, void* Y, const float* rscale, int n_rows,
                        int F, int ldx, int ldy, long n_x_rows, long nnz, int max_deg, hipStream_t st);
int gnn_launch_adam(float* p, float* m, float* v, const float* g, int n, float lr, float b1, float b2, float eps,
                    float wd, int* step, unsigned* done, int step_done, hipStream_t st);
int gnn_launch_cast_bf16(const float* src, void* dst, long n, hipStream_t st);

// ---- gnn_wspmm.hip: edge-weighted aggregate and its edge-value gradient.  xt / yt / t:
// storage types; -3 for a bad stride, -5 for a type pair that is not compiled
int gnn_launch_wspmm(const int* rowptr, const int* col, const float* val, const int* eperm, const void* X, void* Y,
                     const float* rscale, const float* cscale, const float* bias, int n_rows, int F, int ldx, int ldy,
                     int xt, int yt, int relu, hipStream_t st);
int gnn_launch_sddmm(const int* rowptr, const int* col, const void* A, const void* B, float* out, const float* rscale,
                     const float* cscale, int n_rows, int F, int lda, int ldb, int t, hipStream_t st);

// ---- gnn_espmm.hip: the aggregate with a feature row per edge, and its gradient with
// respect to the edge rows (dE) and the edge values (dval).  X, E, Y, dY, dE share the
// storage type t; val / dval are fp32; op: 0 add, 1 mul; X may be null (the sum of edge
// rows), val and eperm too; dE or dval may be null, not both.  -3: a bad stride, E or an
// output missing, relu with op = 1; -5: t outside 0..2; -1: an op that is not compiled
int gnn_launch_espmm(const int* rowptr, const int* col, const float* val, const int* eperm, const void* X,
                     const void* E, void* Y, int n_rows, int F, int ldx, int lde, int ldy, int t, int op, int relu,
                     hipStream_t st);
int gnn_launch_egrad(const int* rowptr, const int* col, const float* val, const void* dY, const void* X,
                     const void* E, void* dE, float* dval, int n_rows, int F, int lddy, int ldx, int lde, int ldde,
                     int t, int op, int relu, hipStream_t st);

// ---- gnn_pool.hip: max / min neighbour pooling with the arg edge index, and its gradient
// over the transposed CSR.  t / tdy / tdx: storage types; arg may be null in the forward;
// -3 for a bad stride or a missing pointer, -5 for a type (pair) that is not compiled
int gnn_launch_pool_fwd(const int* rowptr, const int* col, const void* X, void* Y, int* arg, int n_rows, int F,
                        int ldx, int ldy, int ldarg, int t, int is_min, hipStream_t st);
int gnn_launch_pool_bwd(const int* rowptr_t, const int* col_t, const int* eperm, const int* arg, int ldarg,
                        const void* dY, int lddy, void* dX, int lddx, int n_src, int F, int tdy, int tdx,
                        hipStream_t st);

// ---- gnn_readout.hip: reduction of contiguous row segments (the node rows of each graph of
// a batch) and its reverse, a segment row broadcast to the segment's rows.  ptr: int32
// [S + 1]; op: 0 sum (rscale fp32 [S] or null; the seven pairs (tin, tout) of wspmm plus
// fp32 -> bf16 / fp16), 1 max, 2 min (tin == tout; arg int32 [S, ldarg] or null = the row
// that supplied the value, or arg_in[row] with arg_in).  seg_id: int32 [n]; with arg the
// broadcast writes U[s] where arg[s] names the row and 0 elsewhere.  Checks in this order:
// -3 a bad stride, -5 a type pair that is not compiled, 0 without a launch for S <= 0 /
// n <= 0, -3 a required pointer missing (X may be null when every segment is empty), -1 an
// op outside 0..2
int gnn_launch_seg_reduce(const int* ptr, const void* X, void* Y, const float* rscale, const int* arg_in, int* arg,
                          int S, int F, int ldx, int ldy, int ldarg_in, int ldarg, int tin, int tout, int op,
                          hipStream_t st);
int gnn_launch_seg_bcast(const int* seg_id, const void* U, const float* rscale, const int* arg, void* out, int n,
                         int F, int ldu, int ldarg, int ldo, int tin, int tout, hipStream_t st);

// ---- gnn_geometry.hip: graphs from positions.  pos: fp32 [n, ldp], D coordinates per point;
// gptr int32 [G + 1] / seg_id int32 [n]: the graphs of the batch.  radius_count writes deg [n],
// radius_fill col (and d2, which may be null) at rowptr[i] .. rowptr[i + 1] in ascending
// source id, for d2(i, j) <= r * r inside each graph (j != i unless loop).  pair_d2 writes
// d2 [nnz] of any CSR's edges, pair_d2_bwd dpos [n, ldp] from g [nnz] = dL / d d2 over the CSR
// and its transpose (eperm_t: transposed edge -> CSR edge).  lanes: the sub-group width, 0 =
// from n / G (the search), nnz / n (pair_d2) or 2 nnz / n (its gradient).  Checks in this
// order: -1 D outside 1..3 or a lanes value that is not compiled; -3 ldp < D, nnz < 0, or an r
// that is negative or not finite; 0 without a launch for n <= 0 (and for nnz == 0 in the pair
// kernels, whose caller then zeroes dpos); -3 a required pointer missing (every pointer but
// radius_fill's d2) or G < 1; -4 the grid would overflow
int gnn_launch_radius_count(const float* pos, const int* gptr, const int* seg_id, int* deg, int n, int G, int D,
                            int ldp, float r, int loop, int lanes, hipStream_t st);
int gnn_launch_radius_fill(const float* pos, const int* gptr, const int* seg_id, const int* rowptr, int* col,
                           float* d2, int n, int G, int D, int ldp, float r, int loop, int lanes, hipStream_t st);
int gnn_launch_pair_d2(const int* rowptr, const int* col, const float* pos, float* d2, int n, int nnz, int D, int ldp,
                       int lanes, hipStream_t st);
int gnn_launch_pair_d2_bwd(const int* rowptr, const int* col, const int* rowptr_t, const int* col_t,
                           const int* eperm_t, const float* pos, const float* g, float* dpos, int n, int nnz, int D,
                           int ldp, int lanes, hipStream_t st);
// The k nearest candidates of each point (the neighbour cap of the radius search): a
// candidate of row i is a j of its graph with j != i unless loop, a finite d2(i, j) and
// d2(i, j) <= r * r (r = +inf: no radius); the row keeps the min(k, #candidates) smallest
// keys (d2, j).  knn_select writes deg [n] and the largest kept key tau_d2 / tau_j [n]
// ((-1, -1) for an empty row); knn_fill writes col (and d2, which may be null) at rowptr[i] ..
// rowptr[i + 1] in ascending source id from those thresholds.  Checks in this order: -1 D
// outside 1..3, k outside 1..64, a lanes value that is not compiled, or 0 < lanes < k (a
// sub-group holds one key per lane); -3 ldp < D, or an r that is negative or NaN; 0 without a
// launch for n <= 0; -3 a required pointer missing (every pointer but knn_fill's d2) or
// G < 1; -4 the grid would overflow.  lanes = 0: the smallest compiled width that is >= k and
// at least the radius search's choice (select), the radius search's choice (fill)
int gnn_launch_knn_select(const float* pos, const int* gptr, const int* seg_id, int* deg, float* tau_d2, int* tau_j,
                          int n, int G, int D, int ldp, int k, float r, int loop, int lanes, hipStream_t st);
int gnn_launch_knn_fill(const float* pos, const int* gptr, const int* seg_id, const int* rowptr, const float* tau_d2,
                        const int* tau_j, int* col, float* d2, int n, int G, int D, int ldp, int loop, int lanes,
                        hipStream_t st);
// Periodic cells (gnn_geometry.hip, "Periodic cells").  cell: fp32 [G, 9], the row-major 3 x 3
// cell of each graph, row a = lattice vector a, only the leading D x D block read; nimg: int32
// [G, 3], the image range of each axis, read clamped to 0 .. 7 (0: not periodic).  A candidate
// of row i is (j, s): j of its graph, -nimg[a] <= s[a] <= nimg[a], kept when
// d2(p_i, p_j + s . cell) <= r * r, (j, s) = (i, 0) left out unless loop.  radius_pbc_count
// writes deg [n]; radius_pbc_fill col, shift (byte a = s[a] as int8, byte 3 = 0) and d2 (may
// be null) at rowptr[i] .. rowptr[i + 1] in ascending (j, s), s lexicographic with the last
// axis fastest.  pair_d2_pbc / pair_d2_pbc_bwd are pair_d2 / pair_d2_bwd for a CSR with such a
// shift array; seg_id [n] names the cell of each row, and for pair_d2_pbc_bwd both ends of an
// edge must have the same seg_id (a CSR that is block diagonal over the graphs).  The checks and their order are those
// of the four launchers above, with cell, nimg, seg_id and the fill's shift among the
// required pointers and G < 1 refused with them in the pair kernels too.  lanes = 0: from
// n / G * max_images (the search; max_images, the largest number of images of a graph, is a
// hint that only chooses the width), nnz / n (pair_d2_pbc) or 2 nnz / n (its gradient)
int gnn_launch_radius_pbc_count(const float* pos, const int* gptr, const int* seg_id, const float* cell,
                                const int* nimg, int* deg, int n, int G, int D, int ldp, float r, int loop, int lanes,
                                int max_images, hipStream_t st);
int gnn_launch_radius_pbc_fill(const float* pos, const int* gptr, const int* seg_id, const float* cell, const int* nimg,
                               const int* rowptr, int* col, int* shift, float* d2, int n, int G, int D, int ldp,
                               float r, int loop, int lanes, int max_images, hipStream_t st);
int gnn_launch_pair_d2_pbc(const int* rowptr, const int* col, const int* shift, const float* pos, const float* cell,
                           const int* seg_id, float* d2, int n, int nnz, int G, int D, int ldp, int lanes,
                           hipStream_t st);
int gnn_launch_pair_d2_pbc_bwd(const int* rowptr, const int* col, const int* shift, const int* rowptr_t,
                               const int* col_t, const int* eperm_t, const float* pos, const float* cell,
                               const int* seg_id, const float* g, float* dpos, int n, int nnz, int G, int D, int ldp,
                               int lanes, hipStream_t st);

// ---- gnn_cells.hip: the cell-list radius search, equal to radius_count / radius_fill bit for
// bit (the contract, the grid and its error argument: the file's header).  cells_grid writes
// the grid of every graph, glo fp32 [G, 8] = lo[3], scale[3], 0, 0 and gn int32 [G, 4] = n_0,
// n_1, n_2, their product, with part = gnn_cells_grid_floats(n) floats of scratch; cells_bin
// cell_id [n], a global cell id in [0, n + G) or the sentinel n + G.  The caller sorts the
// points by cell_id (stable): perm [n] the point at each sorted position, scell [n] its cell,
// cptr [n + G + 2] the first sorted position of each cell id, spos fp32 [n, 4] the positions
// in that order (ldp must be 4).  cells_count writes deg [n] under the original row ids;
// cells_fill the rows in scan order into the scratch list sj / sd [cap] at rowptr[i] ..
// rowptr[i + 1]; cells_rows col (and d2, which may be null) [cap] = every scratch row in
// ascending source id.  Nothing is written at or past cap.  Checks in this order: -1 D outside
// 1..3 or a lanes value that is not compiled; -3 ldp < D (spos: ldp != 4), cap < 0, or an r
// that is negative or not finite; 0 without a launch for n <= 0 (and cap == 0 in fill and
// rows; cells_grid then leaves glo / gn to the caller); -3 a required pointer missing (every
// pointer but cells_rows' d2) or G < 1; -4 the grid would overflow.  lanes = 0: the search's
// default width (count, fill), from cap / n (rows)
int gnn_cells_grid_floats(int n);
int gnn_launch_cells_grid(const float* pos, const int* gptr, float* part, float* glo, int* gn, int n, int G, int D,
                          int ldp, float r, hipStream_t st);
int gnn_launch_cells_bin(const float* pos, const int* gptr, const int* seg_id, const float* glo, const int* gn,
                         int* cell_id, int n, int G, int D, int ldp, hipStream_t st);
int gnn_launch_cells_count(const float* spos, const int* perm, const int* scell, const int* cptr, const int* gptr,
                           const int* seg_id, const int* gn, int* deg, int n, int G, int D, int ldp, float r, int loop,
                           int lanes, hipStream_t st);
int gnn_launch_cells_fill(const float* spos, const int* perm, const int* scell, const int* cptr, const int* gptr,
                          const int* seg_id, const int* gn, const int* rowptr, int* sj, float* sd, int n, int G, int D,
                          int ldp, float r, int loop, int lanes, int cap, hipStream_t st);
int gnn_launch_cells_rows(const int* rowptr, const int* sj, const float* sd, int* col, float* d2, int n, int cap,
                          int lanes, hipStream_t st);

// ---- gnn_edge_softmax.hip: softmax over each row's edges and its gradient.  s / p / dp / ds
// are fp32, head-major [K, ld] (head k's edge e at k * ld + e); p may alias s and ds may
// alias dp.  lanes: the sub-group width, 0 = from nnz / n_rows.  -3: a required pointer
// missing, K < 1, ld < nnz, or scale not a positive finite number; -1: a lanes value that
// is not compiled; -4: the (rows x heads) grid would overflow; 0 without a launch for
// n_rows <= 0 or nnz == 0
int gnn_launch_edge_softmax_fwd(const int* rowptr, const float* s, float* p, int n_rows, int nnz, int K, long ld,
                                float scale, int lanes, hipStream_t st);
int gnn_launch_edge_softmax_bwd(const int* rowptr, const float* p, const float* dp, float* ds, int n_rows, int nnz,
                                int K, long ld, float scale, int lanes, hipStream_t st);

// ---- gnn_dense.hip: the fused two-layer dense GCN kernels.  The launchers return -1
// when no compiled variant covers (F, HD, C); Python then raises
int gnn_launch_dense_fwd(const void* AX, const float* W1, const float* b1, const float* W2, const float* dinv,
                         void* H1, void* Z2, int n, int F, int ldx, int HD, int C, int ldc, float p, uint32_t k0,
                         uint32_t k1, uint32_t step, uint32_t row0, const int* stepp, void* kimg, hipStream_t st);
long gnn_keep_image_halfwords(int n, int HD);
int gnn_launch_keep_image(void* kimg, int n, int HD, float p, uint32_t k0, uint32_t k1, uint32_t step, uint32_t row0,
                          const int* stepp, hipStream_t st);
int gnn_launch_dense_bwd(const void* dY2, const float* W2, const void* H1, void* dP1, int n, int HD, int C, int ldc,
                         float p, hipStream_t st);
int gnn_fused_bwd_blocks(int n);
int gnn_fused_bwd_width(int K);
int gnn_fused_bwd_supported(int K, int HD, int C);
int gnn_launch_fused_bwd(const void* AX, const void* dY2, const float* W1, const float* b1, const float* W2,
                         const void* kimg, float* gpart, int n, int F, int ldx, int HD, int C, int ldc, float p,
                         hipStream_t st);

// ---- gnn_linear.hip: generic fused dense layers.  The launchers return the code to
// Python: 0 ok, -1 no variant, -3 bad shape, -4 row ids / scales do not fit
int gnn_lin_fwd_kc_wanted(int K, int N, int ldy);
// Read-only queries (host only): the kernel a launcher selects for a call of that shape, by
// the selection function the launcher itself dispatches on.  Negative: the launcher's
// error code; else family * 1000000 + a * 1000 + b with family 1 lin_ws (a = KS, b = NW),
// 2 the slab kernel (a = KS / KN, b = 10 * waves per block + staged stores), 3 lin_fwd_kc
// (a = FG), 4 lin_gemm, 5 lin_bwd_weight2 (a = KT, b = 10 * NB + HAS_YM), 6 lin_bwd_weight
// (a = KT).  gnn_lin_ws_grid: blocks of lin_ws<KS, NW> for n rows (-1: not compiled).
int gnn_lin_fwd_variant(int ld1, int K1, int has_x2, int ld2, int K2, int N, int ldy, int n, float p, int has_idx1,
                        int has_rscale, int has_tail, int nsplit, int tk, int et);
int gnn_lin_bwd_data_variant(int lddy, int has_ym, int ldym, int N, int K1, int has_dx2, int K2, int ldx1, int ldx2,
                             int n, int has_rscale, int dx1_f32);
int gnn_lin_bwd_weight_variant(int ld1, int K1, int has_x2, int ld2, int K2, int lddy, int has_ym, int ldym, int N,
                               int n, int has_idx1);
int gnn_lin_ws_grid(int ks, int nw, int et, int bwd, int n);
int gnn_launch_lin_fwd(const void* x1, int ld1, int K1, const void* x2, int ld2, int K2, const float* W, int N,
                       const float* bias, void* Y, int ldy, int n, int relu, float p, uint32_t k0, uint32_t k1,
                       uint32_t step, uint32_t row0, const int* stepp, const float* rscale, const int* idx1,
                       void* wimg, float* Yf, int nsplit, int tk, hipStream_t st, int et);
int gnn_launch_lin_bwd_data(const void* dY, int lddy, const void* Ym, int ldym, float mscale, int N, const float* W,
                            int K1, int K2, void* dX1, int ldx1, void* dX2, int ldx2, const float* rscale, int n,
                            int dx1_f32, void* wimg, hipStream_t st);
long gnn_lin_fwd_image_bytes(int K, int N, int ldy);
long gnn_lin_bwd_image_bytes(int K, int N);
int gnn_lin_wgrad_chunks(int n, int N, int K);
int gnn_launch_lin_bwd_weight(const void* x1, int ld1, int K1, const void* x2, int ld2, int K2, const void* dY,
                              int lddy, const void* Ym, int ldym, float mscale, int N, float* gpart, float* dW,
                              float* db, int n, const int* idx1, hipStream_t st);

// ---- gnn_gat.hip: graph attention forward / backward and the fused epoch's dense side
int gnn_gat_row_ce_waves();
int gnn_launch_gat_row_ce(const float* Z, int ldz, const float* bias, int C, const int* y, const uint8_t* mask,
                          float inv_count, float* dZ, void* dZb, float* stats_part, float* bpart, float* stats,
                          float* db, long n, hipStream_t st);
int gnn_launch_gat_pack_grad(const float* dWh, const float* ds_src, const float* ds_dst, int HF, int K, void* dy,
                             int ldy, long n, hipStream_t st);
// Read-only query (host only): the aggregation kernels' variant for K heads of width Fh, by
// the selection function the three launchers dispatch on: L * 100 + G (L lanes per row, G
// lanes per head); -3 a shape outside the rule (Fh % 8 == 0, Fh / 8 a power of two with
// several heads, K * Fh <= 512), -1 a pair that is not compiled.
int gnn_gat_variant(int K, int Fh);
int gnn_launch_gat_fwd(const int* rowptr, const int* col, const void* Wh, const float* s_src, const float* s_dst,
                       const int* dst_rows, float* out, float* lse, void* q, int n, int K, int Fh, int wbf,
                       const float* bias, void* H, int ldh, float p, uint32_t k0, uint32_t k1, uint32_t step,
                       const int* stepp, uint32_t row0, hipStream_t st);
int gnn_gat_row_blocks();
int gnn_launch_gat_rows(int act, const void* dout, int ldh, const float* out, const void* q, const float* lse,
                        const float* s_dst, const int* dst_rows, float* rstat, float* ds_dst, void* dy, int ldy,
                        void* dout_w, const float* bias, float* bpart, float* db, float p, uint32_t k0, uint32_t k1,
                        uint32_t step, const int* stepp, uint32_t row0, int n, int K, int Fh, int wbf,
                        hipStream_t st);
int gnn_launch_gat_col(const int* rowptr_t, const int* col_t, const void* Wh, const float* s_src, const float* rstat,
                       const void* dout, float* dWh, float* ds_src, void* dy, int ldy, int n, int K, int Fh, int wbf,
                       hipStream_t st);

// ---- gnn_halo.hip: halo row exchange between graph shards
int gnn_launch_halo_rows(const void* src, long src_pitch, const long* src_idx, void* dst, long dst_pitch,
                         const long* dst_idx, long rows, int words, int mode, hipStream_t st);

// ---- gnn_sampler.hip: neighbour sampling, the mini-batch pipeline and its worker thread.
// The per-level arguments (int* const* and friends) are host arrays of L device pointers.
// Both launchers refuse before their first HIP call (tests/test_sampler_exact_cpu.py):
// sample_neighbors returns -3 for fanout > 64, and only then 0 for n <= 0 (a fanout < 0
// copies whole rows); sample_blocks returns -3 unless L >= 1, n >= 1, every fan[l] in
// 1..64, every nd_max[l] >= 1 and 0 <= n_seeds <= nd_max[0], with nothing enqueued.
int gnn_launch_sample_neighbors(const int* rowptr, const int* col, const int* nodes, int n, int fanout,
                                const int* out_ptr, int* out_col, uint32_t k0, uint32_t k1, uint32_t salt,
                                hipStream_t st);
long gnn_sample_blocks_scratch(int n, int L, const int* fan, const int* nd_max);
long gnn_sample_flag_bytes(int n);
int gnn_launch_sample_blocks(const int* rowptr, const int* col, int n, const int* seeds, int n_seeds, int L,
                             const int* fan, const int* nd_max, int* const* optr, float* const* inv_deg,
                             int* const* picks, int* const* local, int* const* src, int* const* rp_t,
                             int* const* col_t, int* const* cnt_t, int* counts, uint8_t* flag, int* map,
                             int* bscratch, uint32_t k0, uint32_t k1, uint32_t salt, hipStream_t st,
                             int* counts_host);
// the worker: create returns an opaque handle, add_slot the slot index or < 0, submit the
// job's sequence number (>= 1) or <= 0, wait 0 or the first error any job hit
void* gnn_sw_create(int device, hipStream_t st, const int* rowptr, const int* col, int n, int L, const int* fan,
                    const int* nd_max, uint8_t* flag, int* map, int* bscratch, uint32_t k0, uint32_t k1);
int gnn_sw_add_slot(void* h, int* const* optr, float* const* inv, int* const* picks, int* const* local,
                    int* const* src, int* const* rp_t, int* const* col_t, int* const* cnt_t, int* counts, int* host);
long gnn_sw_submit(void* h, int slot, const int* seeds, int n, uint32_t salt, const hipEvent_t* waits, int nw);
int gnn_sw_wait(void* h, long seq, int slot, hipStream_t consumer);
void gnn_sw_destroy(void* h);

}  // extern "C"
