"""GNN-track device ops (HIP on GPU tensors, PyTorch reference on CPU tensors).

The CPU branch is the numerical reference used by the tests (and lets the
models run in CI); on a GPU the HIP kernels of csrc/kernels/gnn_sparse.hip (and
gnn_wspmm.hip for the edge-weighted ops, gnn_pool.hip for max / min pooling,
gnn_edge_softmax.hip for the softmax over a node's edges, gnn_espmm.hip for the aggregate
with a feature row per edge, gnn_readout.hip for the reduction of each graph's node rows
and its reverse, gnn_geometry.hip for the radius-graph and k-NN searches and the pair distances,
gnn_cells.hip for the cell-list radius search of large point clouds) are mandatory -- a missing extension raises instead of silently falling back.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import native
from ..utils import checks, philox


def _st(t):
    # the raw pointer of the device's current stream, without building a torch Stream
    # object per launch (several us of host time; ~20 launches per SAGE mini-batch)
    return torch._C._cuda_getCurrentRawStream(t.get_device())


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _ru8(x):
    return (x + 7) // 8 * 8


def _row_ids(rowptr):
    n = rowptr.numel() - 1
    counts = (rowptr[1:] - rowptr[:-1]).to(torch.int64)
    return torch.repeat_interleave(torch.arange(n, device=rowptr.device), counts)


_DT_CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def dtype_code(dt) -> int:
    """Element-type code of the sparse kernels (0 fp32, 1 bf16, 2 fp16)."""
    if dt not in _DT_CODE:
        raise TypeError("sparse kernels take fp32 / bf16 / fp16, got %s" % dt)
    return _DT_CODE[dt]


_ONE_ID = {}


def _nonempty_ids(col):
    """``col``, or for a graph with no edges a one-element id buffer (kept per device):
    the gathers issue their first column-id load unconditionally at a clamped address
    (gnn_gather.h, gather_sum), and an empty tensor's pointer is null.  The id (0) is
    never used -- no edge loop runs."""
    if col.numel():
        return col
    buf = _ONE_ID.get(col.device)
    if buf is None:
        buf = _ONE_ID[col.device] = torch.zeros(1, dtype=torch.int32, device=col.device)
    return buf


def spmm(rowptr, col, X, F, rscale=None, bias=None, relu=False, out=None, out_dtype=torch.bfloat16,
         ld_out=None, unit_col=-1, init=None, cscale=None, init_rows=None, short_rows=None):
    """Y[i,:F] = act(rscale[i] * (init[i] + sum_{j in N(i)} cscale[j] X[j,:F]) + bias); X is [*, ldx].
    Padding columns of Y are written 0, except ``unit_col`` which is written 1
    (a ones column that turns the bias gradient into one more GEMM row).
    ``init`` (optional fp32 [init_rows, >=F], default all n rows): partial sums of other
    edges (split aggregation) added to the first ``init_rows`` rows.
    ``cscale`` (optional fp32 per source row): a column scale applied in the gather.
    Rows wider than 512 columns run as 512-column slabs (one launch each); narrower
    slabs were measured slower (round 4, profiles/r04_spmm).
    ``short_rows`` (default: at most 2 entries per row on average, from ``col``'s
    length): the kernel that gives each sub-group 4 consecutive rows (a transposed
    sampled block); bit-identical to the one-row-per-sub-group kernel."""
    n = rowptr.numel() - 1
    if short_rows is None:
        short_rows = col.numel() <= 2 * n
    ldo = ld_out or X.shape[1]
    if out is None:
        out = torch.empty(n, ldo, dtype=out_dtype, device=X.device)
    if checks.enabled():
        checks.csr(rowptr, col, X.shape[0], "spmm")
        checks.rows(out, n, "spmm out")
        checks.rows(rscale, n, "spmm rscale")
        checks.rows(cscale, X.shape[0], "spmm cscale")
    if X.is_cuda:
        hip = native.hip()
        hip.gnn_spmm(rowptr.data_ptr(), _nonempty_ids(col).data_ptr(), X.data_ptr(), out.data_ptr(),
                     rscale.data_ptr() if rscale is not None else 0,
                     bias.data_ptr() if bias is not None else 0, n, F, X.shape[1], out.shape[1],
                     dtype_code(X.dtype), dtype_code(out.dtype), int(relu), int(unit_col),
                     _st(X), init.data_ptr() if init is not None else 0,
                     init.stride(0) if init is not None else 0,
                     cscale.data_ptr() if cscale is not None else 0,
                     -1 if init_rows is None else int(init_rows), int(bool(short_rows)))
        return out
    rows = _row_ids(rowptr)
    acc = torch.zeros(n, F, dtype=torch.float32)
    src = X[col.long(), :F].float()
    if cscale is not None:
        src = src * cscale[col.long()][:, None]
    acc.index_add_(0, rows, src)
    if init is not None:
        r = n if init_rows is None else int(init_rows)
        acc[:r] = acc[:r] + init[:r, :F].float()
    if rscale is not None:
        acc = acc * rscale[:, None]
    if bias is not None:
        acc = acc + bias[:F]
    if relu:
        acc = acc.clamp_min(0)
    out[:n].zero_()
    out[:n, :F] = acc.to(out.dtype)
    if unit_col >= 0:
        out[:n, unit_col] = 1
    return out


def _acc_dtype(dt):
    return torch.float64 if dt == torch.float64 else torch.float32


def wspmm(rowptr, col, val, X, F, rscale=None, cscale=None, bias=None, relu=False, eperm=None, out=None,
          out_dtype=None, ld_out=None):
    """Y[i,:F] = act(rscale[i] * sum_{e in row i} val[p(e)] * cscale[col[e]] * X[col[e],:F] + bias):
    the CSR aggregate with one caller-supplied value per edge (gnn_wspmm.hip, wspmm_kernel).
    ``val`` is fp32 (GPU); ``p(e) = eperm[e]`` with an edge permutation (int32 [nnz], e.g.
    the transposed CSR's map to the forward edges, so the forward's value array is read in
    place), else ``e``.  Padding columns of Y are written 0.  The GPU compiles the (X, Y)
    pairs (bf16, bf16), (bf16, fp32), (fp16, fp16), (fp16, fp32), (fp32, fp32); ``out_dtype``
    defaults to X's.  Per row the multiply-adds run in edge order whatever the launch: the
    output is bit-identical from run to run.  CPU tensors: PyTorch, fp32 accumulation
    (fp64 for fp64 inputs)."""
    n = rowptr.numel() - 1
    nnz = col.numel()
    ldo = ld_out or X.shape[1]
    if out is None:
        out = torch.empty(n, ldo, dtype=out_dtype or X.dtype, device=X.device)
    if checks.enabled():
        checks.csr(rowptr, col, X.shape[0], "wspmm")
        checks.rows(out, n, "wspmm out")
        checks.rows(rscale, n, "wspmm rscale")
        checks.rows(cscale, X.shape[0], "wspmm cscale")
        if eperm is None:
            if val.numel() < nnz:
                raise ValueError("CGNN_CHECK: wspmm: %d values for %d edges" % (val.numel(), nnz))
        else:
            if eperm.numel() != nnz:
                raise ValueError("CGNN_CHECK: wspmm: eperm has %d entries for %d edges" % (eperm.numel(), nnz))
            checks.index(eperm, val.numel(), "wspmm eperm")
    if X.is_cuda:
        if val.dtype != torch.float32:
            raise TypeError("wspmm: edge values must be fp32 on the GPU, got %s" % val.dtype)
        if eperm is not None and eperm.dtype != torch.int32:
            raise TypeError("wspmm: eperm must be int32")
        if not (X.is_contiguous() and out.is_contiguous() and val.is_contiguous()):
            raise ValueError("wspmm: contiguous operands expected")
        native.hip().gnn_wspmm(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(),
                               eperm.data_ptr() if eperm is not None else 0, X.data_ptr(), out.data_ptr(),
                               rscale.data_ptr() if rscale is not None else 0,
                               cscale.data_ptr() if cscale is not None else 0,
                               bias.data_ptr() if bias is not None else 0, n, F, X.shape[1], out.shape[1],
                               dtype_code(X.dtype), dtype_code(out.dtype), int(relu), _st(X))
        return out
    at = _acc_dtype(X.dtype)
    rows = _row_ids(rowptr)
    j = col.long()
    w = (val[eperm.long()] if eperm is not None else val[:nnz]).to(at)
    if cscale is not None:
        w = w * cscale[j].to(at)
    acc = torch.zeros(n, F, dtype=at).index_add_(0, rows, X[j, :F].to(at) * w[:, None])
    if rscale is not None:
        acc = acc * rscale[:n, None].to(at)
    if bias is not None:
        acc = acc + bias[:F].to(at)
    if relu:
        acc = acc.clamp_min(0)
    out[:n].zero_()
    out[:n, :F] = acc.to(out.dtype)
    return out


def sddmm(rowptr, col, A, B, F, rscale=None, cscale=None, out=None):
    """out[e] = rscale[i] * cscale[j] * sum_{f<F} A[i,f] B[j,f] for every edge e = (i, j =
    col[e]) of the CSR -- the gradient of ``wspmm`` with respect to each edge value
    (gnn_wspmm.hip, sddmm_kernel).  A [n_rows, lda] and B [n_src, ldb] share one storage
    type (fp32 / bf16 / fp16); ``out`` is fp32 [nnz] (fp64 for fp64 inputs on the CPU).
    Fixed-order sums, no atomics: bit-identical from run to run."""
    n = rowptr.numel() - 1
    nnz = col.numel()
    if A.dtype != B.dtype:
        raise TypeError("sddmm: A and B must share a dtype, got %s and %s" % (A.dtype, B.dtype))
    if out is None:
        out = torch.empty(nnz, dtype=_acc_dtype(A.dtype), device=A.device)
    if checks.enabled():
        checks.csr(rowptr, col, B.shape[0], "sddmm")
        checks.rows(A, n, "sddmm A")
        checks.rows(out, nnz, "sddmm out")
        checks.rows(rscale, n, "sddmm rscale")
        checks.rows(cscale, B.shape[0], "sddmm cscale")
    if A.is_cuda:
        if out.dtype != torch.float32:
            raise TypeError("sddmm: the output is fp32, got %s" % out.dtype)
        if not (A.is_contiguous() and B.is_contiguous() and out.is_contiguous()):
            raise ValueError("sddmm: contiguous operands expected")
        native.hip().gnn_sddmm(rowptr.data_ptr(), col.data_ptr(), A.data_ptr(), B.data_ptr(), out.data_ptr(),
                               rscale.data_ptr() if rscale is not None else 0,
                               cscale.data_ptr() if cscale is not None else 0, n, F, A.shape[1], B.shape[1],
                               dtype_code(A.dtype), _st(A))
        return out
    at = _acc_dtype(A.dtype)
    rows = _row_ids(rowptr)
    j = col.long()
    d = (A[rows, :F].to(at) * B[j, :F].to(at)).sum(1)
    if rscale is not None:
        d = d * rscale[rows].to(at)
    if cscale is not None:
        d = d * cscale[j].to(at)
    out[:nnz] = d.to(out.dtype)
    return out


_EDGE_OPS = {"add": 0, "mul": 1}


def _edge_args(what, rowptr, col, X, E, op, relu, val, eperm, others):
    """Shared validation of ``espmm`` / ``egrad``: the op code, after the type and layout
    checks that hold on every device (``others``: further (name, tensor) operands sharing
    E's storage type)."""
    if op not in _EDGE_OPS:
        raise ValueError("%s: op must be 'add' or 'mul', got %r" % (what, op))
    if relu and op == "mul":
        raise ValueError("%s: relu goes with op='add' only" % what)
    for name, t in (("X", X),) + tuple(others):
        if t is not None and t.dtype != E.dtype:
            raise TypeError("%s: %s and E must share a dtype, got %s and %s" % (what, name, t.dtype, E.dtype))
    if val is not None and val.dtype != _acc_dtype(E.dtype):
        raise TypeError("%s: edge values must be %s, got %s" % (what, _acc_dtype(E.dtype), val.dtype))
    if eperm is not None and eperm.dtype != torch.int32:
        raise TypeError("%s: eperm must be int32" % what)
    for name, t in (("X", X), ("E", E), ("val", val), ("eperm", eperm)) + tuple(others):
        if t is not None and not t.is_contiguous():
            raise ValueError("%s: contiguous operands expected (%s)" % (what, name))
    if checks.enabled():
        nnz = col.numel()
        checks.csr(rowptr, col, X.shape[0] if X is not None else 1 << 62, what)
        if eperm is None:
            checks.rows(E, nnz, what + " E")
            checks.rows(val, nnz, what + " val")
        else:
            if eperm.numel() != nnz:
                raise ValueError("CGNN_CHECK: %s: eperm has %d entries for %d edges" % (what, eperm.numel(), nnz))
            checks.index(eperm, E.shape[0] if val is None else min(E.shape[0], val.numel()), what + " eperm")
    return _EDGE_OPS[op]


def _edge_messages(col, X, E, F, op, relu, eperm, nnz, at):
    """m_e of ``espmm`` / ``egrad`` and the edge-row index p(e), in PyTorch index ops."""
    pe = eperm.long() if eperm is not None else torch.arange(nnz, device=E.device)
    m = E[pe, :F].to(at)
    if X is not None:
        x = X[col.long(), :F].to(at)
        m = x * m if op == "mul" else x + m
        if relu:
            m = m.clamp_min(0)
    return m, pe


def espmm(rowptr, col, X, E, F, op="add", relu=False, val=None, eperm=None, out=None, ld_out=None):
    """Y[i,:F] = sum_{e in row i} w_e * m_e: the CSR aggregate with a feature row per edge
    (gnn_espmm.hip, espmm_kernel).  ``E`` is ``[n_edge_rows, lde]``; ``p(e) = eperm[e]`` with
    an edge permutation (int32 [nnz], e.g. the transposed CSR's map to the forward edges),
    else ``e``; ``w_e = val[p(e)]`` (fp32, default 1).  ``op="add"``: ``m_e = X[col[e]] +
    E[p(e)]``, through ``max(., 0)`` with ``relu``; ``op="mul"``: ``m_e = X[col[e]] * E[p(e)]``;
    ``X=None``: ``m_e = E[p(e)]``, the sum of edge rows into their destinations.  X, E and Y
    share one storage type (fp32 / bf16 / fp16 on the GPU).  Padding columns of Y are
    written 0.  Per row and feature the sum is one fmaf chain in edge order whatever the
    launch: bit-identical from run to run, no atomics.  CPU tensors: PyTorch, fp32
    accumulation (fp64 for fp64 inputs)."""
    n = rowptr.numel() - 1
    nnz = col.numel()
    if out is None:
        out = torch.empty(n, ld_out or E.shape[1], dtype=E.dtype, device=E.device)
    code = _edge_args("espmm", rowptr, col, X, E, op, relu, val, eperm, (("out", out),))
    if checks.enabled():
        checks.rows(out, n, "espmm out")
    if E.is_cuda:
        if n == 0:
            return out
        if E.shape[0] == 0 and nnz:
            raise ValueError("espmm: E has no rows for %d edges" % nnz)
        # a graph without edges: the launcher wants an E, and an empty tensor's pointer is
        # null; no row has an edge, so the placeholder is never read
        e_ptr = E.data_ptr() if E.shape[0] else _nonempty_ids(col).data_ptr()
        native.hip().gnn_espmm(rowptr.data_ptr(), col.data_ptr(), _ptr(val), _ptr(eperm), _ptr(X), e_ptr,
                               out.data_ptr(), n, F, X.shape[1] if X is not None else 0, E.shape[1], out.shape[1],
                               dtype_code(E.dtype), code, int(bool(relu)), _st(E))
        return out
    at = _acc_dtype(E.dtype)
    m, pe = _edge_messages(col, X, E, F, op, relu, eperm, nnz, at)
    if val is not None:
        m = m * val[pe].to(at)[:, None]
    acc = torch.zeros(n, F, dtype=at).index_add_(0, _row_ids(rowptr), m)
    out[:n].zero_()
    out[:n, :F] = acc.to(out.dtype)
    return out


def egrad(rowptr, col, dY, X, E, F, op="add", relu=False, val=None, dE=None, dval=None, want_dE=True,
          want_dval=False):
    """The gradient of ``espmm`` (forward CSR, no edge permutation) with respect to the edge
    rows and the edge values (gnn_espmm.hip, egrad_kernel): for every edge e = (i, j),
    ``dE[e,:F] = w_e * dY[i,:F] * d`` with ``d = 1`` (add), ``1[X[j] + E[e] > 0]`` (add with
    ``relu``: 0 where the sum is 0, as ``torch.relu``), ``X[j]`` (mul), and ``dval[e] =
    <dY[i], m_e>`` (m_e as in the forward, after the ReLU).  Returns ``(dE, dval)``; an output
    that is neither passed in nor wanted is None and not computed.  ``dE`` has E's storage
    type and row stride (padding columns written 0), ``dval`` is fp32 [nnz] (fp64 for fp64
    inputs on the CPU).  Fixed-order sums, no atomics: bit-identical from run to run."""
    n = rowptr.numel() - 1
    nnz = col.numel()
    if dE is None and want_dE:
        dE = torch.empty(nnz, E.shape[1], dtype=E.dtype, device=E.device)
    if dval is None and want_dval:
        dval = torch.empty(nnz, dtype=_acc_dtype(E.dtype), device=E.device)
    if dE is None and dval is None:
        raise ValueError("egrad: neither dE nor dval requested")
    code = _edge_args("egrad", rowptr, col, X, E, op, relu, val, None, (("dY", dY), ("dE", dE)))
    if dval is not None and (dval.dtype != _acc_dtype(E.dtype) or not dval.is_contiguous()):
        raise TypeError("egrad: dval must be a contiguous %s vector, got %s" % (_acc_dtype(E.dtype), dval.dtype))
    if checks.enabled():
        checks.rows(dY, n, "egrad dY")
        checks.rows(dE, nnz, "egrad dE")
        checks.rows(dval, nnz, "egrad dval")
    if E.is_cuda:
        if nnz == 0:                                     # no edge: nothing to write
            return dE, dval
        native.hip().gnn_egrad(rowptr.data_ptr(), col.data_ptr(), _ptr(val), dY.data_ptr(), _ptr(X), E.data_ptr(),
                               _ptr(dE), _ptr(dval), n, F, dY.shape[1], X.shape[1] if X is not None else 0,
                               E.shape[1], dE.shape[1] if dE is not None else 0, dtype_code(E.dtype), code,
                               int(bool(relu)), _st(E))
        return dE, dval
    at = _acc_dtype(E.dtype)
    g = dY[_row_ids(rowptr), :F].to(at)
    if dval is not None:
        m, _ = _edge_messages(col, X, E, F, op, relu, None, nnz, at)
        dval[:nnz] = (g * m).sum(1).to(dval.dtype)
    if dE is not None:
        d = g if val is None else g * val[:nnz].to(at)[:, None]
        if X is not None and op == "mul":
            d = d * X[col.long(), :F].to(at)
        elif X is not None and relu:
            d = d * (X[col.long(), :F].to(at) + E[:nnz, :F].to(at) > 0).to(at)
        dE[:nnz].zero_()
        dE[:nnz, :F] = d.to(dE.dtype)
    return dE, dval


def _pool_reduce(reduce) -> bool:
    if reduce not in ("max", "min"):
        raise ValueError("pool: reduce must be 'max' or 'min', got %r" % (reduce,))
    return reduce == "min"


def _check_arg(arg, n, F, what):
    if arg.dtype != torch.int32:
        raise ValueError("CGNN_CHECK: %s: arg must be int32, got %s" % (what, arg.dtype))
    if arg.dim() != 2 or arg.shape[1] % 8 or arg.shape[1] < F:
        raise ValueError("CGNN_CHECK: %s: arg row stride %s must be a multiple of 8 and cover F = %d"
                         % (what, tuple(arg.shape[1:]), F))
    checks.rows(arg, n, what + " arg")


def pool(rowptr, col, X, F, reduce="max", out=None, arg=None, with_arg=True, ld_out=None):
    """Element-wise max / min over each row's neighbours (gnn_pool.hip, pool_fwd_kernel):
    ``Y[i,f] = reduce_{e in row i} X[col[e], f]`` and ``arg[i,f]`` = the edge index (global,
    int32) that supplied it.  Returns ``(Y, arg)``; ``arg`` is None with ``with_arg=False``.
    Edges are scanned in CSR order and a candidate replaces the running best only when it is
    strictly better or when it is NaN and the best is not: ties go to the first edge holding
    the value, a NaN propagates (arg = the first NaN edge).  An empty row and the padding
    columns ``F <= f < ld`` give ``Y = 0``, ``arg = -1``.  Y has X's storage type (fp32 /
    bf16 / fp16 on the GPU; fp64 too on CPU tensors): it is a copy of an input element, so
    the result is exact."""
    is_min = _pool_reduce(reduce)
    n = rowptr.numel() - 1
    ldo = ld_out or X.shape[1]
    if out is None:
        out = torch.empty(n, ldo, dtype=X.dtype, device=X.device)
    if arg is None and with_arg:
        arg = torch.empty(n, out.shape[1], dtype=torch.int32, device=X.device)
    if not with_arg:
        arg = None
    if checks.enabled():
        checks.csr(rowptr, col, X.shape[0], "pool")
        checks.rows(out, n, "pool out")
        if arg is not None:
            _check_arg(arg, n, F, "pool")
    if out.dtype != X.dtype:
        raise TypeError("pool: the output has the input's dtype, got %s for %s" % (out.dtype, X.dtype))
    if X.is_cuda:
        if arg is not None and arg.dtype != torch.int32:
            raise TypeError("pool: arg must be int32")
        if not (X.is_contiguous() and out.is_contiguous() and (arg is None or arg.is_contiguous())):
            raise ValueError("pool: contiguous operands expected")
        native.hip().gnn_pool_fwd(rowptr.data_ptr(), col.data_ptr(), X.data_ptr(), out.data_ptr(), _ptr(arg), n, F,
                                  X.shape[1], out.shape[1], arg.shape[1] if arg is not None else 0,
                                  dtype_code(X.dtype), int(is_min), _st(X))
        return out, arg
    rp = rowptr.long()
    deg = rp[1:] - rp[:-1]
    best = torch.zeros(n, F, dtype=X.dtype)
    bi = torch.full((n, F), -1, dtype=torch.int64)
    for k in range(int(deg.max()) if n else 0):          # the k-th edge of every row that has one
        r = torch.nonzero(deg > k).flatten()
        e = rp[r] + k
        c, b = X[col[e].long(), :F], best[r]
        if k == 0:
            take = torch.ones_like(c, dtype=torch.bool)
        else:
            take = ((c < b) if is_min else (c > b)) | (torch.isnan(c) & ~torch.isnan(b))
        best[r] = torch.where(take, c, b)
        bi[r] = torch.where(take, e[:, None].expand_as(c), bi[r])
    out[:n].zero_()
    out[:n, :F] = best
    if arg is not None:
        arg[:n].fill_(-1)
        arg[:n, :F] = bi.to(arg.dtype)
    return out, arg


def pool_bwd(rowptr_t, col_t, eperm, arg, dY, F, out=None, out_dtype=None, ld_out=None):
    """The gradient of ``pool`` as a gather over the transposed CSR (gnn_pool.hip,
    pool_bwd_kernel): ``dX[j,f] = sum_t (arg[i,f] == e ? dY[i,f] : 0)`` over the transposed
    edges t of source row j, ``i = col_t[t]`` the destination and ``e = eperm[t]`` the forward
    edge (``transpose_csr(..., with_perm=True)``).  Edge indices are compared, not node ids,
    so a source repeated in a row is counted once.  The terms are added in fp32 (fp64 for
    fp64 on the CPU) as one chain in transposed-edge order: bit-identical from run to run,
    no atomics.  The GPU compiles the (dY, dX) pairs of ``wspmm``; ``out_dtype`` defaults to
    dY's.  Padding columns of dX are written 0."""
    n_src = rowptr_t.numel() - 1
    nnz = col_t.numel()
    ldo = ld_out or dY.shape[1]
    if out is None:
        out = torch.empty(n_src, ldo, dtype=out_dtype or dY.dtype, device=dY.device)
    if checks.enabled():
        checks.csr(rowptr_t, col_t, min(arg.shape[0], dY.shape[0]), "pool_bwd")
        checks.rows(out, n_src, "pool_bwd out")
        if eperm.numel() != nnz:
            raise ValueError("CGNN_CHECK: pool_bwd: eperm has %d entries for %d edges" % (eperm.numel(), nnz))
        checks.index(eperm, nnz, "pool_bwd eperm")
        _check_arg(arg, 0, F, "pool_bwd")
    if dY.is_cuda:
        if arg.dtype != torch.int32 or eperm.dtype != torch.int32:
            raise TypeError("pool_bwd: arg and eperm must be int32")
        if not (dY.is_contiguous() and out.is_contiguous() and arg.is_contiguous()):
            raise ValueError("pool_bwd: contiguous operands expected")
        native.hip().gnn_pool_bwd(rowptr_t.data_ptr(), col_t.data_ptr(), eperm.data_ptr(), arg.data_ptr(),
                                  arg.shape[1], dY.data_ptr(), dY.shape[1], out.data_ptr(), out.shape[1], n_src, F,
                                  dtype_code(dY.dtype), dtype_code(out.dtype), _st(dY))
        return out
    at = _acc_dtype(dY.dtype)
    rp = rowptr_t.long()
    deg = rp[1:] - rp[:-1]
    acc = torch.zeros(n_src, F, dtype=at)
    for k in range(int(deg.max()) if n_src else 0):      # one chain per row, in transposed-edge order
        r = torch.nonzero(deg > k).flatten()
        t = rp[r] + k
        i, e = col_t[t].long(), eperm[t].long()
        acc[r] += torch.where(arg[i, :F].long() == e[:, None], dY[i, :F].to(at), torch.zeros((), dtype=at))
    out[:n_src].zero_()
    out[:n_src, :F] = acc.to(out.dtype)
    return out


# rows per chunk of the two-level graph readout (gnn/readout.py).  512: the fastest of 64 / 256 /
# 512 / 1024 on 4 graphs of 250 k nodes (docs/PERF.md, "Graph readout"); graphs of at most one
# chunk run as a single launch
READOUT_CHUNK = 512

_SEG_OPS = {"sum": 0, "max": 1, "min": 2}


def _check_ptr(ptr, n_rows, what):
    if ptr.dim() != 1 or ptr.numel() < 1:
        raise ValueError("CGNN_CHECK: %s: ptr must be a non-empty vector" % what)
    p = ptr.long()
    if int(p[0]) != 0 or bool((p[1:] < p[:-1]).any()):
        raise ValueError("CGNN_CHECK: %s: ptr must start at 0 and never decrease" % what)
    if int(p[-1]) > n_rows:
        raise ValueError("CGNN_CHECK: %s: ptr ends at %d but the input has %d rows" % (what, int(p[-1]), n_rows))


def _seg_gpu_operands(what, ints, floats, dense):
    """TypeError / ValueError for GPU operands that are not int32 (``ints``), not fp32
    (``floats``) or not contiguous (all of them and ``dense``); None entries are skipped."""
    for name, t in ints:
        if t is not None and t.dtype != torch.int32:
            raise TypeError("%s: %s must be int32, got %s" % (what, name, t.dtype))
    for name, t in floats:
        if t is not None and t.dtype != torch.float32:
            raise TypeError("%s: %s must be fp32, got %s" % (what, name, t.dtype))
    for name, t in tuple(ints) + tuple(floats) + tuple(dense):
        if t is not None and not t.is_contiguous():
            raise ValueError("%s: contiguous operands expected (%s)" % (what, name))


def seg_reduce(ptr, X, F, reduce="sum", rscale=None, arg_in=None, out=None, arg=None, with_arg=False, out_dtype=None,
               ld_out=None):
    """Reduction of contiguous row segments (gnn_readout.hip, seg_reduce_kernel): output row
    ``s`` reduces the rows ``ptr[s] .. ptr[s+1] - 1`` of ``X`` ``[*, ldx]``; ``ptr`` is int32
    ``[S + 1]``, starts at 0 and never decreases.  Returns ``(Y, arg)``.

    ``reduce="sum"``: ``Y[s,f] = rscale[s] * sum_i X[i,f]``, accumulated in fp32 in an order
    that depends on the segment's length alone, one product (``rscale`` fp32 ``[S]``, default
    1) and one rounding to ``out_dtype`` (default X's; the GPU compiles the pairs of ``wspmm``
    and fp32 -> bf16 / fp16); ``arg`` is None.  ``"max"`` / ``"min"``: the scan rule of ``pool``
    -- ties go to the first row holding the value, a NaN propagates -- Y in X's type, and
    ``arg[s,f]`` (with ``with_arg`` or an ``arg`` buffer; int32) the row index ``i`` that
    supplied it, or ``arg_in[i,f]`` with ``arg_in`` (int32 ``[*, ld]``): a second pass over
    partial results hands the first pass's indices through.  An empty segment and the padding
    columns ``F <= f < ld`` give ``Y = 0``, ``arg = -1``.  No atomics: bit-identical from run
    to run, and a segment's result does not depend on where it stands.  CPU tensors: PyTorch,
    fp32 accumulation (fp64 for fp64 inputs)."""
    if reduce not in _SEG_OPS:
        raise ValueError("seg_reduce: reduce must be 'sum', 'max' or 'min', got %r" % (reduce,))
    is_sum = reduce == "sum"
    if is_sum and (arg is not None or arg_in is not None or with_arg):
        raise ValueError("seg_reduce: the sum has no arg")
    if not is_sum and rscale is not None:
        raise ValueError("seg_reduce: rscale goes with reduce='sum' only")
    S = ptr.numel() - 1
    if out is None:
        out = torch.empty(S, ld_out or X.shape[1], dtype=(out_dtype or X.dtype) if is_sum else X.dtype,
                          device=X.device)
    if not is_sum and out.dtype != X.dtype:
        raise TypeError("seg_reduce: max / min give the input's dtype, got %s for %s" % (out.dtype, X.dtype))
    if arg is None and with_arg:
        arg = torch.empty(S, out.shape[1], dtype=torch.int32, device=X.device)
    if checks.enabled():
        _check_ptr(ptr, X.shape[0], "seg_reduce")
        checks.rows(out, S, "seg_reduce out")
        checks.rows(rscale, S, "seg_reduce rscale")
        if arg is not None:
            _check_arg(arg, S, F, "seg_reduce")
        if arg_in is not None:
            _check_arg(arg_in, int(ptr[-1]), F, "seg_reduce arg_in")
    if X.is_cuda:
        _seg_gpu_operands("seg_reduce", (("ptr", ptr), ("arg", arg), ("arg_in", arg_in)), (("rscale", rscale),),
                          (("X", X), ("out", out)))
        native.hip().gnn_seg_reduce(ptr.data_ptr(), X.data_ptr(), out.data_ptr(), _ptr(rscale), _ptr(arg_in),
                                    _ptr(arg), S, F, X.shape[1], out.shape[1],
                                    arg_in.shape[1] if arg_in is not None else 0,
                                    arg.shape[1] if arg is not None else 0, dtype_code(X.dtype),
                                    dtype_code(out.dtype), _SEG_OPS[reduce], _st(X))
        return out, arg
    at = _acc_dtype(X.dtype)
    p = ptr.long()
    cnt = p[1:] - p[:-1]
    if is_sum:
        rows = _row_ids(ptr)
        acc = torch.zeros(S, F, dtype=at).index_add_(0, rows, X[:rows.numel(), :F].to(at))
        if rscale is not None:
            acc = acc * rscale[:S, None].to(at)
        out[:S].zero_()
        out[:S, :F] = acc.to(out.dtype)
        return out, None
    is_min = reduce == "min"
    best = torch.zeros(S, F, dtype=X.dtype)
    bi = torch.full((S, F), -1, dtype=torch.int64)
    for k in range(int(cnt.max()) if S else 0):          # the k-th row of every segment that has one
        r = torch.nonzero(cnt > k).flatten()
        i = p[r] + k
        c, b = X[i, :F], best[r]
        if k == 0:
            take = torch.ones_like(c, dtype=torch.bool)
        else:
            take = ((c < b) if is_min else (c > b)) | (torch.isnan(c) & ~torch.isnan(b))
        best[r] = torch.where(take, c, b)
        bi[r] = torch.where(take, i[:, None].expand_as(c), bi[r])
    out[:S].zero_()
    out[:S, :F] = best
    if arg is not None:
        if arg_in is not None and arg_in.shape[0]:
            bi = torch.where(bi >= 0, torch.gather(arg_in[:, :F].long(), 0, bi.clamp_min(0)), bi)
        arg[:S].fill_(-1)
        arg[:S, :F] = bi.to(arg.dtype)
    return out, arg


def seg_bcast(seg_id, U, F, rscale=None, arg=None, out=None, out_dtype=None, ld_out=None):
    """A segment's row broadcast to the segment's rows (gnn_readout.hip, seg_bcast_kernel):
    ``out[i,f] = rscale[s] * U[s,f]`` with ``s = seg_id[i]`` (int32 ``[n]``), the product in
    fp32 and rounded once (``rscale`` fp32 ``[S]``, default 1) -- the gradient of ``seg_reduce``'s
    sum, and a forward op of its own (global conditioning ``x + u[batch]``).  With ``arg`` (int32
    ``[S, ld]``, a max / min reduction's): ``out[i,f] = U[s,f]`` where ``arg[s,f] == i`` and 0
    elsewhere, that reduction's gradient.  Padding columns are written 0.  The GPU compiles
    the (U, out) pairs of ``wspmm``; ``out_dtype`` defaults to U's.  CPU tensors: PyTorch."""
    if arg is not None and rscale is not None:
        raise ValueError("seg_bcast: rscale or arg, not both")
    n, S = seg_id.numel(), U.shape[0]
    if out is None:
        out = torch.empty(n, ld_out or U.shape[1], dtype=out_dtype or U.dtype, device=U.device)
    if checks.enabled():
        checks.index(seg_id, S, "seg_bcast seg_id")
        checks.rows(out, n, "seg_bcast out")
        checks.rows(rscale, S, "seg_bcast rscale")
        if arg is not None:
            _check_arg(arg, S, F, "seg_bcast")
    if n and not S:
        raise ValueError("seg_bcast: %d rows name segments of an empty U" % n)
    if U.is_cuda:
        _seg_gpu_operands("seg_bcast", (("seg_id", seg_id), ("arg", arg)), (("rscale", rscale),),
                          (("U", U), ("out", out)))
        native.hip().gnn_seg_bcast(seg_id.data_ptr(), U.data_ptr(), _ptr(rscale), _ptr(arg), out.data_ptr(), n, F,
                                   U.shape[1], arg.shape[1] if arg is not None else 0, out.shape[1],
                                   dtype_code(U.dtype), dtype_code(out.dtype), _st(U))
        return out
    at = _acc_dtype(U.dtype)
    s = seg_id.long()
    u = U[s, :F].to(at)
    if arg is not None:
        u = torch.where(arg[s, :F].long() == torch.arange(n)[:, None], u, torch.zeros((), dtype=at))
    elif rscale is not None:
        u = u * rscale[s].to(at)[:, None]
    out[:n].zero_()
    out[:n, :F] = u.to(out.dtype)
    return out


_ES_LANES = (8, 16, 32, 64)


def _edge_heads(t, what):
    """(K, ld) of a head-major edge tensor: ``[nnz]`` is one head, ``[K, ld]`` K heads."""
    if t.dim() == 1:
        return 1, t.shape[0]
    if t.dim() == 2:
        return t.shape[0], t.shape[1]
    raise ValueError("%s: [nnz] or [K, ld] expected, got shape %s" % (what, tuple(t.shape)))


def _edge_softmax_args(rowptr, ts, names, scale, lanes, nnz, what):
    """Shared validation of ``edge_softmax`` / ``edge_softmax_bwd``: (K, ld, nnz, lanes)."""
    K, ld = _edge_heads(ts[0], what)
    for t, name in zip(ts, names):
        if t.shape != ts[0].shape or t.dtype != ts[0].dtype or t.device != ts[0].device:
            raise ValueError("%s: %s must match %s in shape, dtype and device" % (what, name, names[0]))
    nnz = ld if nnz is None else int(nnz)
    lanes = 0 if lanes is None else int(lanes)
    if checks.enabled():
        if rowptr.dim() != 1 or rowptr.numel() < 1:
            raise ValueError("CGNN_CHECK: %s: rowptr must be a non-empty vector" % what)
        rp = rowptr.long()
        if int(rp[0]) != 0 or bool((rp[1:] < rp[:-1]).any()):
            raise ValueError("CGNN_CHECK: %s: rowptr must start at 0 and never decrease" % what)
        if not int(rp[-1]) <= nnz <= ld:
            raise ValueError("CGNN_CHECK: %s: rowptr ends at %d, nnz = %d, ld = %d" % (what, int(rp[-1]), nnz, ld))
        if not (float(scale) > 0 and float(scale) < float("inf")):
            raise ValueError("CGNN_CHECK: %s: scale must be positive and finite, got %r" % (what, scale))
    if ts[0].is_cuda:
        if ts[0].dtype != torch.float32:
            raise TypeError("%s: scores are fp32 on the GPU, got %s" % (what, ts[0].dtype))
        if rowptr.dtype != torch.int32:
            raise TypeError("%s: rowptr must be int32" % what)
        if not all(t.is_contiguous() for t in ts):
            raise ValueError("%s: contiguous operands expected" % what)
    return K, ld, nnz, lanes


def _segments(rowptr, t, K, ld):
    """CPU branch: (row id per edge, the [K, E] view of the edges the CSR names)."""
    rows = _row_ids(rowptr)
    return rows, t.reshape(K, ld)[:, :rows.numel()]


def edge_softmax(rowptr, score, scale=1.0, out=None, lanes=None, nnz=None):
    """Softmax over each row's edges (gnn_edge_softmax.hip, edge_softmax_fwd_kernel):
    ``p[k,e] = exp(scale (s[k,e] - m)) / sum_e' exp(scale (s[k,e'] - m))`` over the edges of
    row i, ``m`` their maximum, ``scale > 0``.  ``score`` is ``[nnz]`` or head-major ``[K, ld]``
    (``ld >= nnz``: one head is a contiguous slice that ``sddmm(out=...)`` writes and
    ``wspmm(val=...)`` reads in place); fp32 on the GPU.  ``out`` (same shape; default a new
    tensor) may be ``score`` itself; nothing outside the first ``rowptr[-1]`` elements of a
    head is written.  An empty row writes nothing, a single edge gives exactly 1, a ``-inf``
    score exactly 0, a row of ``-inf`` all 0; a NaN or ``+inf`` score makes its (row, head)
    NaN and nothing else.  No atomics: bit-identical from run to run, and a row's result
    does not depend on where it stands.  ``lanes``: force the sub-group width (8 / 16 / 32
    / 64; default: chosen from ``nnz / n_rows``); ``nnz``: the number of edges when ``ld``
    exceeds it (default ``ld``; only that choice looks at it).  CPU tensors: PyTorch in fp32,
    or fp64 for fp64 inputs."""
    if out is None:
        out = torch.empty_like(score)
    K, ld, nnz, lanes = _edge_softmax_args(rowptr, (score, out), ("score", "out"), scale, lanes, nnz, "edge_softmax")
    n = rowptr.numel() - 1
    if score.is_cuda:
        native.hip().gnn_edge_softmax_fwd(rowptr.data_ptr(), score.data_ptr(), out.data_ptr(), n, nnz, K, ld,
                                          float(scale), lanes, _st(score))
        return out
    if lanes not in (0,) + _ES_LANES:
        raise ValueError("edge_softmax: lanes must be one of %s, got %d" % (_ES_LANES, lanes))
    at = _acc_dtype(score.dtype)
    rows, s = _segments(rowptr, score, K, ld)
    if rows.numel() == 0:
        return out
    s = s.to(at)
    m = torch.full((K, n), float("-inf"), dtype=at).scatter_reduce_(1, rows.expand(K, -1), s, "amax")
    m = torch.where(m == float("-inf"), torch.zeros_like(m), m)
    ex = torch.exp(scale * (s - m[:, rows]))
    l = torch.zeros(K, n, dtype=at).index_add_(1, rows, ex)
    rinv = torch.where(l == 0, torch.zeros_like(l), 1.0 / l)           # a NaN sum stays NaN
    out.view(K, ld)[:, :rows.numel()] = (ex * rinv[:, rows]).to(out.dtype)
    return out


def edge_softmax_bwd(rowptr, p, dp, scale=1.0, out=None, lanes=None, nnz=None):
    """The gradient of ``edge_softmax`` from its saved output (gnn_edge_softmax.hip,
    edge_softmax_bwd_kernel): ``ds[k,e] = scale p[k,e] (dp[k,e] - sum_e' p[k,e'] dp[k,e'])``.
    ``p``, ``dp`` and ``out`` share one shape (``[nnz]`` or ``[K, ld]``); ``out`` may be ``dp``
    itself (not ``p``).  Layout, ``lanes``, ``nnz``, determinism and the CPU branch as in
    ``edge_softmax``."""
    if out is None:
        out = torch.empty_like(dp)
    K, ld, nnz, lanes = _edge_softmax_args(rowptr, (p, dp, out), ("p", "dp", "out"), scale, lanes, nnz,
                                           "edge_softmax_bwd")
    n = rowptr.numel() - 1
    if p.is_cuda:
        native.hip().gnn_edge_softmax_bwd(rowptr.data_ptr(), p.data_ptr(), dp.data_ptr(), out.data_ptr(), n, nnz, K,
                                          ld, float(scale), lanes, _st(p))
        return out
    if lanes not in (0,) + _ES_LANES:
        raise ValueError("edge_softmax_bwd: lanes must be one of %s, got %d" % (_ES_LANES, lanes))
    at = _acc_dtype(p.dtype)
    rows, pv = _segments(rowptr, p, K, ld)
    if rows.numel() == 0:
        return out
    pv, g = pv.to(at), dp.reshape(K, ld)[:, :rows.numel()].to(at)
    dot = torch.zeros(K, n, dtype=at).index_add_(1, rows, pv * g)
    out.view(K, ld)[:, :rows.numel()] = (scale * pv * (g - dot[:, rows])).to(out.dtype)
    return out


def _geo_args(what, pos, D, lanes):
    """Shared validation of the geometry ops: (n, ldp, lanes)."""
    if pos.dim() != 2:
        raise ValueError("%s: pos must be [n, ldp], got shape %s" % (what, tuple(pos.shape)))
    D = int(D)
    if not 1 <= D <= 3:
        raise ValueError("%s: D must be 1, 2 or 3, got %d" % (what, D))
    if pos.shape[1] < D:
        raise ValueError("%s: pos has %d columns for D = %d" % (what, pos.shape[1], D))
    lanes = 0 if lanes is None else int(lanes)
    if lanes not in (0,) + _ES_LANES:
        raise ValueError("%s: lanes must be one of %s, got %d" % (what, _ES_LANES, lanes))
    if pos.is_cuda:
        _seg_gpu_operands(what, (), (("pos", pos),), ())
    elif not pos.is_floating_point():
        raise TypeError("%s: pos must be a floating-point tensor, got %s" % (what, pos.dtype))
    return pos.shape[0], pos.shape[1], lanes


def _radius_args(what, pos, D, r, gptr, seg_id, lanes):
    n, ldp, lanes = _geo_args(what, pos, D, lanes)
    r = float(r)
    if not (r >= 0 and r < float("inf")):
        raise ValueError("%s: r must be finite and not negative, got %r" % (what, r))
    _batch_args(what, n, gptr, seg_id)
    return n, ldp, lanes, r


def _batch_args(what, n, gptr, seg_id):
    """The graphs of a batch of ``n`` points: ``gptr`` ``[G + 1]`` and ``seg_id`` ``[n]``."""
    if gptr.dim() != 1 or gptr.numel() < 2 and n:
        raise ValueError("%s: gptr must be a vector [G + 1] with G >= 1" % what)
    if seg_id.dim() != 1 or seg_id.numel() != n:
        raise ValueError("%s: seg_id must be [%d], got %s" % (what, n, tuple(seg_id.shape)))
    if checks.enabled():
        _check_ptr(gptr, n, what)
        if int(gptr[-1]) != n:
            raise ValueError("CGNN_CHECK: %s: gptr ends at %d but pos has %d rows" % (what, int(gptr[-1]), n))
        checks.index(seg_id, gptr.numel() - 1, what + " seg_id")


def _sq_dist(a, b):
    """``d2`` of the rows of ``a`` and ``b`` (``[..., D]``) by the kernels' definition: fp32
    differences, then ``fma(dz, dz, fma(dy, dy, dx * dx))``.  PyTorch has no fma on the CPU: a
    product of two fp32 values is exact in fp64, so each fma is one fp64 add rounded to fp32
    (equal to the fused result except for rare double-rounding ties).  fp64 inputs: plain fp64."""
    d = a - b
    if d.dtype != torch.float32:
        return (d * d).sum(-1)
    d2 = d[..., 0] * d[..., 0]
    for c in range(1, d.shape[-1]):
        dc = d[..., c].double()
        d2 = (dc * dc + d2.double()).float()
    return d2


def _radius_cpu(pos, D, r, gptr, loop):
    """(deg, col, d2) of the radius graph on the CPU, graph by graph, ascending ids."""
    n = pos.shape[0]
    at = _acc_dtype(pos.dtype)
    r2 = torch.tensor(r, dtype=at) * torch.tensor(r, dtype=at)
    deg = torch.zeros(n, dtype=torch.int32)
    cols, d2s = [], []
    gp = gptr.tolist()
    for g0, g1 in zip(gp[:-1], gp[1:]):
        if g1 <= g0:
            continue
        p = pos[g0:g1, :D].to(at)
        d2 = _sq_dist(p[:, None, :], p[None, :, :])          # [i (dst), j (src)]
        keep = d2 <= r2                                       # False for NaN
        if not loop:
            keep &= ~torch.eye(g1 - g0, dtype=torch.bool)
        deg[g0:g1] = keep.sum(1).to(torch.int32)
        ij = keep.nonzero()                                   # sorted by (i, j)
        cols.append((ij[:, 1] + g0).to(torch.int32))
        d2s.append(d2[keep])
    col = torch.cat(cols) if cols else torch.zeros(0, dtype=torch.int32)
    d2 = torch.cat(d2s) if d2s else torch.zeros(0, dtype=at)
    return deg, col, d2


def radius_count(pos, D, r, gptr, seg_id, loop=False, lanes=None, out=None):
    """The count pass of the radius-graph search (gnn_geometry.hip, radius_count_kernel):
    ``deg[i]``, int32 ``[n]``, the number of sources ``j`` of node i's own graph
    ``[gptr[g], gptr[g+1])``, ``g = seg_id[i]``, with ``d2(i, j) <= r * r`` and ``j != i`` unless
    ``loop``.  ``pos`` is ``[n, ldp]`` with ``D`` (1..3) coordinates per point, fp32 on the GPU;
    ``gptr`` int32 ``[G + 1]`` and ``seg_id`` int32 ``[n]`` are ``GraphBatch.gptr`` / ``.batch``.
    ``d2 = fma(dz, dz, fma(dy, dy, dx * dx))`` of fp32 differences and ``r * r`` is one fp32
    product; the boundary is inclusive, a NaN distance is no edge, coincident points are
    neighbours.  Brute force inside each graph, O(n_g^2) -- for molecules and other graphs of
    up to a few thousand points; ``cells_count`` / ``cells_fill`` are the cell-list search for
    large point clouds, with this op's result bit for bit (``knn_select`` / ``knn_fill`` cap a row
    at its k nearest; ``radius_pbc_count`` / ``radius_pbc_fill`` search the images of a periodic
    cell: both brute force only).
    ``lanes``: force the sub-group width (8 / 16 / 32 / 64; default from ``n / G``); the
    result is the same for every width.  ``out``: a preallocated ``deg``.  CPU tensors: PyTorch
    with the same contract."""
    n, ldp, lanes, r = _radius_args("radius_count", pos, D, r, gptr, seg_id, lanes)
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=pos.device)
    if checks.enabled():
        checks.rows(out, n, "radius_count out")
    if pos.is_cuda:
        _seg_gpu_operands("radius_count", (("gptr", gptr), ("seg_id", seg_id), ("out", out)), (), ())
        native.hip().gnn_radius_count(pos.data_ptr(), gptr.data_ptr(), seg_id.data_ptr(), out.data_ptr(), n,
                                      gptr.numel() - 1, int(D), ldp, r, int(bool(loop)), lanes, _st(pos))
        return out
    out[:n] = _radius_cpu(pos, int(D), r, gptr, loop)[0]
    return out


def radius_fill(pos, D, r, gptr, seg_id, rowptr, loop=False, lanes=None, out=None, d2=None, with_d2=False, nnz=None):
    """The fill pass of the radius-graph search (gnn_geometry.hip, radius_fill_kernel):
    ``col[rowptr[i] .. rowptr[i+1])`` = the neighbours of node i **in ascending source id**,
    and with ``with_d2`` or a ``d2`` buffer their squared distances (fp32 ``[nnz]``) at the same
    places.  ``rowptr`` (int32 ``[n + 1]``) is the exclusive sum of ``radius_count``'s ``deg`` for
    the same arguments; nothing at or past ``rowptr[i+1]`` is written for row i.  Returns
    ``(col, d2)``.  ``out`` / ``d2``: preallocated buffers of a known capacity; without ``out`` the
    length is ``nnz``, or ``rowptr[-1]`` read back (one host sync).  No atomics: the CSR is a
    function of ``pos`` and ``gptr`` alone -- not of ``lanes``, the grid or the run -- and a
    graph's rows, with ids relative to ``gptr[g]``, do not depend on its place in the batch.
    Contract, limits and the CPU branch as in ``radius_count``."""
    n, ldp, lanes, r = _radius_args("radius_fill", pos, D, r, gptr, seg_id, lanes)
    if rowptr.dim() != 1 or rowptr.numel() != n + 1:
        raise ValueError("radius_fill: rowptr must be [%d], got %s" % (n + 1, tuple(rowptr.shape)))
    if out is None:
        nnz = int(rowptr[-1]) if nnz is None else int(nnz)
        out = torch.empty(nnz, dtype=torch.int32, device=pos.device)
    if d2 is None and with_d2:
        d2 = torch.empty(out.numel(), dtype=_acc_dtype(pos.dtype), device=pos.device)
    if checks.enabled():
        _check_ptr(rowptr, 2 ** 31 - 1, "radius_fill")
        for name, t in (("out", out), ("d2", d2)):
            if t is not None and t.numel() < int(rowptr[-1]):
                raise ValueError("CGNN_CHECK: radius_fill: %s holds %d edges, rowptr ends at %d"
                                 % (name, t.numel(), int(rowptr[-1])))
    if pos.is_cuda:
        _seg_gpu_operands("radius_fill", (("gptr", gptr), ("seg_id", seg_id), ("rowptr", rowptr), ("out", out)),
                          (("d2", d2),), ())
        if out.numel() == 0:                                  # no edge to write (a null pointer)
            return out, d2
        native.hip().gnn_radius_fill(pos.data_ptr(), gptr.data_ptr(), seg_id.data_ptr(), rowptr.data_ptr(),
                                     out.data_ptr(), _ptr(d2), n, gptr.numel() - 1, int(D), ldp, r, int(bool(loop)),
                                     lanes, _st(pos))
        return out, d2
    deg, col, dd = _radius_cpu(pos, int(D), r, gptr, loop)
    _fill_rows(deg, col, dd, rowptr, out, d2)
    return out, d2


def _fill_rows(deg, col, dd, rowptr, out, d2):
    """The fill kernels' slots on the CPU: row i's ``deg[i]`` neighbours (``col`` / ``dd``, row
    after row) go to ``rowptr[i] ..``.  The kernels' rule for a rowptr that is not the count
    pass's: row i keeps its first ``rowptr[i+1] - rowptr[i]`` neighbours."""
    n = deg.numel()
    rp = rowptr.long()
    cnt = deg.long()
    start = torch.zeros(n + 1, dtype=torch.int64)
    start[1:] = torch.cumsum(cnt, 0)
    own = torch.repeat_interleave(torch.arange(n), cnt)
    k = torch.arange(col.numel()) - start[own]
    ok = k < (rp[1:] - rp[:-1])[own]
    slot = rp[own] + k
    out[slot[ok]] = col[ok].to(out.dtype)
    if d2 is not None:
        d2[slot[ok]] = dd[ok].to(d2.dtype)


CELLS_NA_MAX = 1024     # cells per axis (gnn_cells.hip: the cap its error argument needs)
_CELLS_SIDE = 1.0 + 2.0 ** -10          # the least cell side is r * (1 + 2^-10) ...
_CELLS_SIDE_MIN = 2.0 ** -60            # ... and at least this (r = 0, squares that underflow)
_CELLS_EXT_MAX = 2.0 ** 100             # a longer axis has one cell


def _cells_tables(what, G, glo, gn, on_gpu):
    if glo.shape != (G, 8) or gn.shape != (G, 4):
        raise ValueError("%s: glo must be [%d, 8] and gn [%d, 4], got %s and %s"
                         % (what, G, G, tuple(glo.shape), tuple(gn.shape)))
    if on_gpu:
        _seg_gpu_operands(what, (("gn", gn),), (("glo", glo),), ())
    elif gn.dtype != torch.int32:
        raise TypeError("%s: gn must be int32, got %s" % (what, gn.dtype))


def cells_grid(pos, D, r, gptr, glo=None, gn=None, part=None):
    """The grid of every graph for the cell-list radius search (gnn_cells.hip, cells_part_kernel
    / cells_grid_kernel): ``glo`` fp32 ``[G, 8]`` = ``lo[3]``, ``scale[3]``, 0, 0 and ``gn`` int32
    ``[G, 4]`` = ``n_0, n_1, n_2`` and their product, from the finite points of each graph
    ``[gptr[g], gptr[g+1])`` and ``r`` alone, on the device, with no read-back.  Along axis a:
    ``lo`` the least coordinate, ``ext = hi - lo``, ``n_a = min(1024, int(ext / s0))`` cells with
    ``s0 = max(r * (1 + 2^-10), 2^-60)``, one cell when ``ext`` is below ``2 s0``, zero, not
    finite or above ``2^100``; then the largest ``n_a`` (the lowest axis among equals) is halved,
    rounding up, until the graph has at most ``max(1, n_g)`` cells; ``scale = n_a / ext`` (0 for
    one cell).  ``bin_a(x) = min(n_a - 1, int((x - lo) * scale))`` is monotone in ``x``, and two
    points the radius search connects lie in cells that differ by at most one along every axis
    (the argument, in fp32 error terms: the header of gnn_cells.hip).  A graph with one cell is
    the brute-force search.  ``r = 0`` is legal.  ``glo`` / ``gn``: preallocated outputs;
    ``part``: fp32 scratch of ``8 * ceil(n / 1024)`` values on the GPU.  CPU tensors: PyTorch with
    the same arithmetic (fp64 positions: in fp64).  Returns ``(glo, gn)``."""
    n, ldp, _ = _geo_args("cells_grid", pos, D, None)
    D = int(D)
    r = float(r)
    if not (r >= 0 and r < float("inf")):
        raise ValueError("cells_grid: r must be finite and not negative, got %r" % r)
    if gptr.dim() != 1 or gptr.numel() < 2 and n:
        raise ValueError("cells_grid: gptr must be a vector [G + 1] with G >= 1")
    G = gptr.numel() - 1
    at = _acc_dtype(pos.dtype)
    if glo is None:
        glo = torch.empty(G, 8, dtype=at, device=pos.device)
    if gn is None:
        gn = torch.empty(G, 4, dtype=torch.int32, device=pos.device)
    _cells_tables("cells_grid", G, glo, gn, pos.is_cuda)
    if n == 0:
        glo.zero_()
        gn.fill_(1)
        return glo, gn
    if pos.is_cuda:
        need = native.hip().gnn_cells_grid_floats(n)
        if part is None:
            part = torch.empty(need, dtype=torch.float32, device=pos.device)
        if part.numel() < need:
            raise ValueError("cells_grid: part holds %d values, %d needed" % (part.numel(), need))
        _seg_gpu_operands("cells_grid", (("gptr", gptr),), (("part", part),), ())
        native.hip().gnn_cells_grid(pos.data_ptr(), gptr.data_ptr(), part.data_ptr(), glo.data_ptr(), gn.data_ptr(),
                                    n, G, D, ldp, r, _st(pos))
        return glo, gn
    s0 = torch.maximum(torch.tensor(r, dtype=at) * torch.tensor(_CELLS_SIDE, dtype=at),
                       torch.tensor(_CELLS_SIDE_MIN, dtype=at))
    glo.zero_()
    gn.fill_(1)
    gp = gptr.tolist()
    for g in range(G):
        g0 = min(max(gp[g], 0), n)
        g1 = min(max(gp[g + 1], g0), n)
        p = pos[g0:g1, :D].to(at)
        p = p[torch.isfinite(p).all(1)]
        if p.shape[0] == 0:
            continue
        lo, hi = p.min(0).values, p.max(0).values
        ext = hi - lo                                         # inf when it overflows
        na = [1, 1, 1]
        for a in range(D):
            if 0 < float(ext[a]) <= _CELLS_EXT_MAX:
                q = int(torch.clamp(ext[a] / s0, max=float(CELLS_NA_MAX)))
                if q >= 2:
                    na[a] = q
        cap = max(g1 - g0, 1)
        while na[0] * na[1] * na[2] > cap:
            a = max(range(3), key=lambda c: (na[c], -c))       # the largest, the lowest axis among equals
            na[a] = (na[a] + 1) // 2
        glo[g, :D] = lo
        for a in range(D):
            if na[a] >= 2:
                glo[g, 3 + a] = torch.tensor(na[a], dtype=at) / ext[a]
        gn[g] = torch.tensor(na + [na[0] * na[1] * na[2]], dtype=torch.int32)
    return glo, gn


def cells_bin(pos, D, gptr, seg_id, glo, gn, out=None):
    """The cell of every point (gnn_cells.hip, cells_bin_kernel): ``cell_id`` int32 ``[n]``,
    ``gptr[g] + g + (bin_0 n_1 + bin_1) n_2 + bin_2`` with ``g = seg_id[i]`` and the bins of
    ``cells_grid`` (absent axes: one cell) -- the cells of graph g fill the id range
    ``[gptr[g] + g, gptr[g+1] + g + 1)`` -- or the sentinel ``n + G`` for a point with a NaN or
    inf coordinate, a ``seg_id`` outside ``[0, G)`` or one that names another graph's range: such
    a point has an empty row and is nobody's neighbour.  ``out``: a preallocated ``cell_id``.
    CPU tensors: PyTorch with the same arithmetic."""
    n, ldp, _ = _geo_args("cells_bin", pos, D, None)
    D = int(D)
    _batch_args("cells_bin", n, gptr, seg_id)
    G = gptr.numel() - 1
    _cells_tables("cells_bin", G, glo, gn, pos.is_cuda)
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=pos.device)
    if checks.enabled():
        checks.rows(out, n, "cells_bin out")
    if n == 0:
        return out
    if pos.is_cuda:
        _seg_gpu_operands("cells_bin", (("gptr", gptr), ("seg_id", seg_id), ("out", out)), (), ())
        native.hip().gnn_cells_bin(pos.data_ptr(), gptr.data_ptr(), seg_id.data_ptr(), glo.data_ptr(), gn.data_ptr(),
                                   out.data_ptr(), n, G, D, ldp, _st(pos))
        return out
    at = _acc_dtype(pos.dtype)
    s = seg_id.long()
    sc = s.clamp(0, G - 1)
    g0 = gptr.long().clamp(0, n)[sc]
    g1 = torch.maximum(gptr.long().clamp(0, n)[sc + 1], g0)
    i = torch.arange(n)
    p = pos[:, :D].to(at)
    ok = (s >= 0) & (s < G) & (i >= g0) & (i < g1) & torch.isfinite(p).all(1)
    v = (torch.where(ok[:, None], p, torch.zeros_like(p)) - glo[sc, :D].to(at)) * glo[sc, 3:3 + D].to(at)
    v = torch.nan_to_num(v, nan=0.0)                          # inf * 0 on an axis of one cell: bin 0 either way
    idx = torch.zeros(n, dtype=torch.int64)
    for a in range(D):
        na = gn[sc, a].long().clamp(1, CELLS_NA_MAX)
        b = torch.minimum(v[:, a].clamp(0, CELLS_NA_MAX).long(), na - 1)
        idx = idx * na + b
    cell = g0 + sc + torch.minimum(idx, (g1 - g0 - 1).clamp(min=0))
    out[:n] = torch.where(ok, cell, torch.full_like(cell, n + G)).to(torch.int32)
    return out


def cells_order(pos, D, cell_id, G):
    """The points in cell order, device plumbing in PyTorch (a stable sort, so ids ascend inside
    a cell): ``(perm, scell, cptr, spos)`` -- ``perm`` int32 ``[n]`` the point at each sorted
    position, ``scell`` int32 ``[n]`` its cell, ``cptr`` int32 ``[n + G + 2]`` the first sorted
    position of every cell id (cell c holds the positions ``[cptr[c], cptr[c+1])``; the last
    entry is ``n``), ``spos`` ``[n, 4]`` the positions in that order, padded with zeros to 16
    bytes.  No host synchronisation."""
    n = cell_id.shape[0]
    scell, perm = torch.sort(cell_id[:n], stable=True)
    ids = torch.arange(n + G + 2, dtype=torch.int32, device=cell_id.device)
    cptr = torch.searchsorted(scell, ids, out_int32=True)
    spos = torch.zeros(n, 4, dtype=pos.dtype, device=pos.device)
    spos[:, :D] = pos[perm, :D]
    return perm.to(torch.int32), scell, cptr, spos


def cells_prepare(pos, D, r, gptr, seg_id):
    """Grid, bins and cell order in one call: ``(glo, gn, cell_id, perm, scell, cptr, spos)`` of
    ``cells_grid``, ``cells_bin`` and ``cells_order``, what ``cells_count`` / ``cells_fill`` take."""
    glo, gn = cells_grid(pos, D, r, gptr)
    cell_id = cells_bin(pos, D, gptr, seg_id, glo, gn)
    return (glo, gn, cell_id) + cells_order(pos, int(D), cell_id, gptr.numel() - 1)


def _cells_search_args(what, spos, perm, scell, cptr, gptr, seg_id, gn, D, r, lanes):
    n, ldp, lanes, r = _radius_args(what, spos, D, r, gptr, seg_id, lanes)
    G = gptr.numel() - 1
    if ldp != 4:
        raise ValueError("%s: spos must be [n, 4] (cells_order), got %s" % (what, tuple(spos.shape)))
    if perm.shape != (n,) or scell.shape != (n,) or cptr.shape != (n + G + 2,) or gn.shape != (G, 4):
        raise ValueError("%s: perm / scell [%d], cptr [%d] and gn [%d, 4] expected, got %s, %s, %s, %s"
                         % (what, n, n + G + 2, G, tuple(perm.shape), tuple(scell.shape), tuple(cptr.shape),
                            tuple(gn.shape)))
    if spos.is_cuda:
        _seg_gpu_operands(what, (("perm", perm), ("scell", scell), ("cptr", cptr), ("gptr", gptr), ("seg_id", seg_id),
                                 ("gn", gn)), (), ())
    return n, G, lanes, r


def _cells_cpu(spos, perm, scell, cptr, gptr, seg_id, gn, D, r, loop):
    """(deg, col, d2) of the radius graph through the cells on the CPU: every row walks the up
    to 3^D cells around its own, the kept pairs are then ordered by (row, source id)."""
    n = perm.numel()
    G = gptr.numel() - 1
    at = _acc_dtype(spos.dtype)
    r2 = torch.tensor(r, dtype=at) * torch.tensor(r, dtype=at)
    k = torch.arange(n)
    pm = perm.long()
    c = scell.long()
    s = seg_id.long()[pm]
    sc = s.clamp(0, max(G - 1, 0))
    cb = gptr.long().clamp(0, n)[sc] + sc
    na = gn.long()[sc, :3].clamp(1, CELLS_NA_MAX)
    na[:, D:] = 1
    l = c - cb
    act = (c >= 0) & (c < n + G) & (s >= 0) & (s < G) & (l >= 0) & (l < na.prod(1))
    l = torch.where(act, l, torch.zeros_like(l))
    b2 = l % na[:, 2]
    t = l // na[:, 2]
    b = (t // na[:, 1], t % na[:, 1], b2)
    cp = cptr.long()
    P = spos[:, :D].to(at)
    rows, srcs, dd = [], [], []
    for d0 in (-1, 0, 1):
        for d1 in (-1, 0, 1):
            for d2 in (-1, 0, 1):
                a = (b[0] + d0, b[1] + d1, b[2] + d2)
                ok = act.clone()
                for x in range(3):
                    ok &= (a[x] >= 0) & (a[x] < na[:, x])
                cell = torch.where(ok, cb + (a[0] * na[:, 1] + a[1]) * na[:, 2] + a[2], torch.zeros_like(cb))
                j0 = cp[cell]
                cnt = torch.where(ok, cp[cell + 1] - j0, torch.zeros_like(j0))
                own = torch.repeat_interleave(k, cnt)
                first = torch.cumsum(cnt, 0) - cnt
                kk = j0[own] + torch.arange(own.numel()) - first[own]
                d = _sq_dist(P[own], P[kk])
                keep = d <= r2                                # False for NaN
                if not loop:
                    keep &= kk != own
                rows.append(pm[own[keep]])
                srcs.append(pm[kk[keep]])
                dd.append(d[keep])
    rows, srcs, dd = torch.cat(rows), torch.cat(srcs), torch.cat(dd)
    order = torch.argsort(rows * max(n, 1) + srcs)
    deg = torch.bincount(rows, minlength=n).to(torch.int32)
    return deg, srcs[order].to(torch.int32), dd[order]


def cells_count(spos, perm, scell, cptr, gptr, seg_id, gn, D, r, loop=False, lanes=None, out=None):
    """The count pass of the cell-list radius search (gnn_cells.hip, cells_search_kernel):
    ``deg[i]``, int32 ``[n]`` under the original row ids, **equal to** ``radius_count`` **for the
    same** ``pos``, ``D``, ``r``, ``gptr``, ``seg_id`` **and** ``loop`` -- O(n) candidates instead of
    O(n_g^2).  ``spos``, ``perm``, ``scell``, ``cptr`` come from ``cells_order`` (``cells_prepare``),
    ``gn`` from ``cells_grid``.  The sub-group of row i walks the cells around its own, clipped at
    the grid's edges; the cells that differ only along the last axis are one contiguous range
    of the sorted points.  ``seg_id[i]`` must be the graph whose range holds i, or lie outside
    ``[0, G)`` (``cells_bin``).  Non-periodic, D = 1..3, radius search only: no periodic cells, no
    k-NN or neighbour cap on this path.  ``lanes``: force the sub-group width (8 / 16 / 32 / 64);
    the result is the same for every width.  ``out``: a preallocated ``deg``.  CPU tensors:
    PyTorch through the same cells."""
    n, G, lanes, r = _cells_search_args("cells_count", spos, perm, scell, cptr, gptr, seg_id, gn, D, r, lanes)
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=spos.device)
    if checks.enabled():
        checks.rows(out, n, "cells_count out")
    if n == 0:
        return out
    if spos.is_cuda:
        _seg_gpu_operands("cells_count", (("out", out),), (), ())
        native.hip().gnn_cells_count(spos.data_ptr(), perm.data_ptr(), scell.data_ptr(), cptr.data_ptr(),
                                     gptr.data_ptr(), seg_id.data_ptr(), gn.data_ptr(), out.data_ptr(), n, G, int(D),
                                     4, r, int(bool(loop)), lanes, _st(spos))
        return out
    out[:n] = _cells_cpu(spos, perm, scell, cptr, gptr, seg_id, gn, int(D), r, loop)[0]
    return out


def cells_fill(spos, perm, scell, cptr, gptr, seg_id, gn, D, r, rowptr, loop=False, lanes=None, out=None, d2=None,
               with_d2=False, nnz=None, scratch=None):
    """The fill pass of the cell-list radius search (gnn_cells.hip, cells_search_kernel with
    stores, then cells_rows_kernel): ``col`` and, with ``with_d2`` or a ``d2`` buffer, ``d2`` **equal
    to** ``radius_fill``'s: rows in ascending source id, nothing written at or past
    ``rowptr[i+1]``.  The search writes every row in scan order into ``scratch = (sj, sd)`` (int32
    and fp32, at least as long as ``out``; allocated when ``None``: the one scratch copy of the
    edge list); the row pass ranks every entry inside its row -- ids are distinct, so the slot
    is ``rowptr[i] + #{j' < j}`` -- and stores it there; any row length works.  No atomics: the
    same CSR for every ``lanes``, grid and run.  Other arguments as in ``cells_count`` /
    ``radius_fill``.  Returns ``(col, d2)``."""
    n, G, lanes, r = _cells_search_args("cells_fill", spos, perm, scell, cptr, gptr, seg_id, gn, D, r, lanes)
    if rowptr.dim() != 1 or rowptr.numel() != n + 1:
        raise ValueError("cells_fill: rowptr must be [%d], got %s" % (n + 1, tuple(rowptr.shape)))
    if out is None:
        nnz = int(rowptr[-1]) if nnz is None else int(nnz)
        out = torch.empty(nnz, dtype=torch.int32, device=spos.device)
    if d2 is None and with_d2:
        d2 = torch.empty(out.numel(), dtype=_acc_dtype(spos.dtype), device=spos.device)
    cap = out.numel() if d2 is None else min(out.numel(), d2.numel())
    if checks.enabled():
        _check_ptr(rowptr, 2 ** 31 - 1, "cells_fill")
        if cap < int(rowptr[-1]):
            raise ValueError("CGNN_CHECK: cells_fill: the buffers hold %d edges, rowptr ends at %d"
                             % (cap, int(rowptr[-1])))
    if spos.is_cuda:
        if scratch is None:
            scratch = (torch.empty(cap, dtype=torch.int32, device=spos.device),
                       torch.empty(cap, dtype=torch.float32, device=spos.device))
        sj, sd = scratch
        if sj.numel() < cap or sd.numel() < cap:
            raise ValueError("cells_fill: the scratch holds %d / %d edges, %d needed" % (sj.numel(), sd.numel(), cap))
        _seg_gpu_operands("cells_fill", (("rowptr", rowptr), ("out", out), ("scratch ids", sj)),
                          (("d2", d2), ("scratch d2", sd)), ())
        if n == 0 or cap == 0:                                # no edge to write (a null pointer)
            return out, d2
        h = native.hip()
        h.gnn_cells_fill(spos.data_ptr(), perm.data_ptr(), scell.data_ptr(), cptr.data_ptr(), gptr.data_ptr(),
                         seg_id.data_ptr(), gn.data_ptr(), rowptr.data_ptr(), sj.data_ptr(), sd.data_ptr(), n, G,
                         int(D), 4, r, int(bool(loop)), lanes, cap, _st(spos))
        h.gnn_cells_rows(rowptr.data_ptr(), sj.data_ptr(), sd.data_ptr(), out.data_ptr(), _ptr(d2), n, cap, 0,
                         _st(spos))
        return out, d2
    if n == 0:
        return out, d2
    deg, col, dd = _cells_cpu(spos, perm, scell, cptr, gptr, seg_id, gn, int(D), r, loop)
    _fill_rows(deg, col, dd, rowptr, out, d2)
    return out, d2


KNN_MAX = 64            # a sub-group holds one key per lane


def _knn_min_lanes(k):
    """The smallest compiled sub-group width that holds ``k`` keys."""
    return next(L for L in _ES_LANES if L >= k)


def _knn_cpu_d2(pos, D, g0, g1):
    """``d2[i (dst), j (src)]`` of one graph and its "no self loop" mask."""
    p = pos[g0:g1, :D].to(_acc_dtype(pos.dtype))
    return _sq_dist(p[:, None, :], p[None, :, :]), ~torch.eye(g1 - g0, dtype=torch.bool)


def knn_select(pos, D, k, gptr, seg_id, r=None, loop=False, lanes=None, deg=None, tau_d2=None, tau_j=None):
    """The select pass of the k-NN search (gnn_geometry.hip, knn_select_kernel).  The
    **candidates** of node i are the ``j`` of its own graph ``[gptr[g], gptr[g+1])``,
    ``g = seg_id[i]``, with ``j != i`` unless ``loop``, a finite ``d2(i, j)`` (not NaN, not inf)
    and ``d2(i, j) <= r * r`` (``r = None`` or ``inf``: no radius).  Row i keeps the
    ``min(k, #candidates)`` candidates with the smallest key ``(d2, j)``, lexicographic with
    ``d2`` compared as fp32: equal distances go to the lower id, so the kept set is a function
    of ``pos`` and the graphs alone -- not of ``lanes``, the grid, the run or the graph's place
    in the batch.  ``1 <= k <= 64``.  Returns ``(deg, tau_d2, tau_j)``: ``deg[i]`` int32 the
    number kept, and the row's threshold, its largest kept key (``tau_d2`` fp32, ``tau_j``
    int32; ``(-1, -1)`` for a row that keeps nothing), which ``knn_fill`` turns into the CSR.
    ``pos``, ``D``, ``gptr``, ``seg_id`` and ``d2`` as in ``radius_count``.  ``lanes``: force
    the sub-group width (8 / 16 / 32 / 64, at least ``k``: a sub-group holds one key per
    lane; default the smallest such width that is at least ``radius_count``'s choice).
    ``deg`` / ``tau_d2`` / ``tau_j``: preallocated outputs.  Brute force inside each graph,
    O(n_g^2) distances plus about ``k ln(n_g / k)`` insertions per row.  CPU tensors: PyTorch
    with the same contract (a stable sort of ``d2`` gives the tie rule; fp64 positions give
    fp64 ``tau_d2``)."""
    n, ldp, lanes = _geo_args("knn_select", pos, D, lanes)
    k = int(k)
    if not 1 <= k <= KNN_MAX:
        raise ValueError("knn_select: k must be in 1..%d, got %d" % (KNN_MAX, k))
    if lanes and lanes < k:
        raise ValueError("knn_select: lanes = %d holds fewer than k = %d keys" % (lanes, k))
    r = float("inf") if r is None else float(r)
    if not r >= 0:
        raise ValueError("knn_select: r must not be negative or NaN, got %r" % r)
    _batch_args("knn_select", n, gptr, seg_id)
    at = _acc_dtype(pos.dtype)
    if deg is None:
        deg = torch.empty(n, dtype=torch.int32, device=pos.device)
    if tau_d2 is None:
        tau_d2 = torch.empty(n, dtype=at, device=pos.device)
    if tau_j is None:
        tau_j = torch.empty(n, dtype=torch.int32, device=pos.device)
    for name, t in (("deg", deg), ("tau_d2", tau_d2), ("tau_j", tau_j)):
        if t.dim() != 1 or t.numel() < n:
            raise ValueError("knn_select: %s must hold %d rows, got %s" % (name, n, tuple(t.shape)))
    if pos.is_cuda:
        _seg_gpu_operands("knn_select", (("gptr", gptr), ("seg_id", seg_id), ("deg", deg), ("tau_j", tau_j)),
                          (("tau_d2", tau_d2),), ())
        native.hip().gnn_knn_select(pos.data_ptr(), gptr.data_ptr(), seg_id.data_ptr(), deg.data_ptr(),
                                    tau_d2.data_ptr(), tau_j.data_ptr(), n, gptr.numel() - 1, int(D), ldp, k, r,
                                    int(bool(loop)), lanes, _st(pos))
        return deg, tau_d2, tau_j
    r2 = torch.tensor(r, dtype=at) * torch.tensor(r, dtype=at)
    deg[:n] = 0
    tau_d2[:n] = -1
    tau_j[:n] = -1
    gp = gptr.tolist()
    for g0, g1 in zip(gp[:-1], gp[1:]):
        if g1 <= g0:
            continue
        d2, off = _knn_cpu_d2(pos, int(D), g0, g1)
        cand = torch.isfinite(d2) & (d2 <= r2)
        if not loop:
            cand &= off
        cnt = cand.sum(1).clamp(max=k)
        # stable: equal distances stay in ascending id; the non-candidates go last
        key, order = torch.sort(torch.where(cand, d2, torch.full_like(d2, float("inf"))), dim=1, stable=True)
        has = cnt > 0
        last = (cnt - 1).clamp(min=0)[:, None]
        deg[g0:g1] = cnt.to(deg.dtype)
        tau_d2[g0:g1] = torch.where(has, key.gather(1, last)[:, 0], torch.full_like(key[:, 0], -1)).to(tau_d2.dtype)
        tau_j[g0:g1] = torch.where(has, order.gather(1, last)[:, 0] + g0, torch.full_like(cnt, -1)).to(tau_j.dtype)
    return deg, tau_d2, tau_j


def knn_fill(pos, D, gptr, seg_id, rowptr, tau_d2, tau_j, loop=False, lanes=None, out=None, d2=None, with_d2=False,
             nnz=None):
    """The fill pass of the k-NN search (gnn_geometry.hip, knn_fill_kernel):
    ``col[rowptr[i] .. rowptr[i+1])`` = the ``j`` of node i's graph whose key ``(d2(i, j), j)``
    is at most the row's threshold ``(tau_d2[i], tau_j[i])`` from ``knn_select`` (``j != i``
    unless ``loop``; a NaN or infinite distance is above every threshold), **in ascending
    source id** -- not in distance order -- and with ``with_d2`` or a ``d2`` buffer their
    squared distances at the same places.  ``rowptr`` (int32 ``[n + 1]``) is the exclusive sum
    of ``knn_select``'s ``deg`` for the same arguments; nothing at or past ``rowptr[i+1]`` is
    written for row i.  Takes no ``k`` and no ``r`` (the thresholds hold both), and ``lanes``
    may be any compiled width whatever ``k`` was.  Returns ``(col, d2)``; ``out`` / ``d2`` /
    ``nnz`` as in ``radius_fill``.  A row is a subset of the same row of ``radius_fill`` for
    the same ``r``, and bit-equal to it when that has at most ``k`` entries."""
    n, ldp, lanes = _geo_args("knn_fill", pos, D, lanes)
    _batch_args("knn_fill", n, gptr, seg_id)
    if rowptr.dim() != 1 or rowptr.numel() != n + 1:
        raise ValueError("knn_fill: rowptr must be [%d], got %s" % (n + 1, tuple(rowptr.shape)))
    for name, t in (("tau_d2", tau_d2), ("tau_j", tau_j)):
        if t.dim() != 1 or t.numel() < n:
            raise ValueError("knn_fill: %s must hold %d rows, got %s" % (name, n, tuple(t.shape)))
    if out is None:
        nnz = int(rowptr[-1]) if nnz is None else int(nnz)
        out = torch.empty(nnz, dtype=torch.int32, device=pos.device)
    if d2 is None and with_d2:
        d2 = torch.empty(out.numel(), dtype=_acc_dtype(pos.dtype), device=pos.device)
    if checks.enabled():
        _check_ptr(rowptr, 2 ** 31 - 1, "knn_fill")
        for name, t in (("out", out), ("d2", d2)):
            if t is not None and t.numel() < int(rowptr[-1]):
                raise ValueError("CGNN_CHECK: knn_fill: %s holds %d edges, rowptr ends at %d"
                                 % (name, t.numel(), int(rowptr[-1])))
    if pos.is_cuda:
        _seg_gpu_operands("knn_fill", (("gptr", gptr), ("seg_id", seg_id), ("rowptr", rowptr), ("tau_j", tau_j),
                                       ("out", out)), (("tau_d2", tau_d2), ("d2", d2)), ())
        if out.numel() == 0:                                  # no edge to write (a null pointer)
            return out, d2
        native.hip().gnn_knn_fill(pos.data_ptr(), gptr.data_ptr(), seg_id.data_ptr(), rowptr.data_ptr(),
                                  tau_d2.data_ptr(), tau_j.data_ptr(), out.data_ptr(), _ptr(d2), n,
                                  gptr.numel() - 1, int(D), ldp, int(bool(loop)), lanes, _st(pos))
        return out, d2
    deg = torch.zeros(n, dtype=torch.int32)
    cols, d2s = [], []
    gp = gptr.tolist()
    for g0, g1 in zip(gp[:-1], gp[1:]):
        if g1 <= g0:
            continue
        dd, off = _knn_cpu_d2(pos, int(D), g0, g1)
        td = tau_d2[g0:g1, None].to(dd.dtype)
        ids = torch.arange(g0, g1)[None, :]
        keep = (dd < td) | ((dd == td) & (ids <= tau_j[g0:g1, None]))       # False for NaN
        if not loop:
            keep &= off
        deg[g0:g1] = keep.sum(1).to(torch.int32)
        cols.append((keep.nonzero()[:, 1] + g0).to(torch.int32))              # sorted by (i, j)
        d2s.append(dd[keep])
    col = torch.cat(cols) if cols else torch.zeros(0, dtype=torch.int32)
    dd = torch.cat(d2s) if d2s else torch.zeros(0, dtype=_acc_dtype(pos.dtype))
    _fill_rows(deg, col, dd, rowptr, out, d2)
    return out, d2


def _pair_args(what, rowptr, col, pos, D, lanes, nnz):
    n, ldp, lanes = _geo_args(what, pos, D, lanes)
    if rowptr.dim() != 1 or rowptr.numel() < 1 or rowptr.numel() - 1 > n:
        raise ValueError("%s: rowptr describes %d rows for %d positions" % (what, rowptr.numel() - 1, n))
    nnz = col.numel() if nnz is None else int(nnz)
    if not 0 <= nnz <= col.numel():
        raise ValueError("%s: nnz = %d with %d column ids" % (what, nnz, col.numel()))
    checks.csr(rowptr, col, n, what)
    if checks.enabled() and int(rowptr[-1]) > nnz:
        raise ValueError("CGNN_CHECK: %s: rowptr ends at %d, nnz = %d" % (what, int(rowptr[-1]), nnz))
    return rowptr.numel() - 1, ldp, lanes, nnz


def pair_d2(rowptr, col, pos, D, out=None, lanes=None, nnz=None):
    """The squared distance of each edge of a CSR (gnn_geometry.hip, pair_d2_kernel):
    ``d2[e] = fma(dz, dz, fma(dy, dy, dx * dx))`` with ``dx = pos[i, 0] - pos[col[e], 0]`` ... in
    fp32 for the edges e of row i (row = destination), fp32 ``[nnz]``.  ``pos`` is ``[n, ldp]``
    with ``D`` (1..3) coordinates.  For graphs that do not come from the radius search (bond
    graphs from ``GraphBatch.from_graphs``); on a radius graph it reproduces ``radius_fill``'s
    ``d2`` bit for bit.  ``out``: a preallocated buffer of at least ``nnz`` (default
    ``col.numel()``) elements; ``lanes`` as in ``edge_softmax``.  CPU tensors: PyTorch (fp64 for
    fp64 positions)."""
    n, ldp, lanes, nnz = _pair_args("pair_d2", rowptr, col, pos, D, lanes, nnz)
    if out is None:
        out = torch.empty(nnz, dtype=_acc_dtype(pos.dtype), device=pos.device)
    if out.numel() < nnz:
        raise ValueError("pair_d2: out holds %d edges, nnz = %d" % (out.numel(), nnz))
    if pos.is_cuda:
        _seg_gpu_operands("pair_d2", (("rowptr", rowptr), ("col", col)), (("out", out),), ())
        native.hip().gnn_pair_d2(rowptr.data_ptr(), col.data_ptr(), pos.data_ptr(), out.data_ptr(), n, nnz, int(D),
                                 ldp, lanes, _st(pos))
        return out
    rows = _row_ids(rowptr)
    E = rows.numel()
    at = _acc_dtype(pos.dtype)
    out[:E] = _sq_dist(pos[rows, :D].to(at), pos[col[:E].long(), :D].to(at)).to(out.dtype)
    return out


def pair_d2_bwd(rowptr, col, rowptr_t, col_t, eperm_t, pos, g, D, out=None, lanes=None, nnz=None):
    """The gradient of a scalar with respect to the positions through ``pair_d2``
    (gnn_geometry.hip, pair_d2_bwd_kernel), given ``g[e] = dL / d d2[e]`` (fp32 ``[nnz]``):

        dpos[i] = 2 (sum_{e in in(i)} g[e] (p_i - p_src(e)) + sum_{e in out(i)} g[e] (p_i - p_dst(e)))

    The in-edges are row i of the CSR, the out-edges row i of the transposed CSR
    (``rowptr_t``, ``col_t``, ``eperm_t`` as ``transposed_perm()`` returns them); the CSR is
    square.  fp32 accumulation, in-edges in CSR order then out-edges in transposed order, in a
    tree that is a fixed function of the two degrees and ``lanes``; the factor 2 once at the
    end.  ``out`` is ``[n, ldp]`` like ``pos``: the columns ``D <= c < ldp`` are written 0 and a
    node without edges gets 0.  No atomics: bit-identical from run to run.  CPU tensors:
    PyTorch ``index_add_`` (fp64 for fp64 positions)."""
    n, ldp, lanes, nnz = _pair_args("pair_d2_bwd", rowptr, col, pos, D, lanes, nnz)
    if n != pos.shape[0] or rowptr_t.numel() != n + 1:
        raise ValueError("pair_d2_bwd: a square CSR over the %d positions expected (%d rows, %d transposed rows)"
                         % (pos.shape[0], n, rowptr_t.numel() - 1))
    if g.dim() != 1 or g.numel() < nnz or col_t.numel() < nnz or eperm_t.numel() < nnz:
        raise ValueError("pair_d2_bwd: g, col_t and eperm_t must hold %d edges" % nnz)
    if out is None:
        out = torch.empty_like(pos)
    if out.shape != pos.shape:
        raise ValueError("pair_d2_bwd: out must be %s like pos, got %s" % (tuple(pos.shape), tuple(out.shape)))
    if checks.enabled():
        checks.csr(rowptr_t, col_t, n, "pair_d2_bwd (transposed)")
        checks.index(eperm_t[:nnz], max(nnz, 1), "pair_d2_bwd eperm_t")
    if n == 0 or nnz == 0:
        return out.zero_()
    if pos.is_cuda:
        _seg_gpu_operands("pair_d2_bwd", (("rowptr", rowptr), ("col", col), ("rowptr_t", rowptr_t), ("col_t", col_t),
                                          ("eperm_t", eperm_t)), (("g", g), ("out", out)), ())
        native.hip().gnn_pair_d2_bwd(rowptr.data_ptr(), col.data_ptr(), rowptr_t.data_ptr(), col_t.data_ptr(),
                                     eperm_t.data_ptr(), pos.data_ptr(), g.data_ptr(), out.data_ptr(), n, nnz,
                                     int(D), ldp, lanes, _st(pos))
        return out
    at = _acc_dtype(pos.dtype)
    rows = _row_ids(rowptr)
    E = rows.numel()
    src = col[:E].long()
    p = pos[:, :D].to(at)
    w = g[:E].to(at)[:, None] * (p[rows] - p[src])
    acc = torch.zeros(n, D, dtype=at).index_add_(0, rows, w).index_add_(0, src, -w)
    out.zero_()
    out[:, :D] = (2 * acc).to(out.dtype)
    return out


PBC_NIMG_MAX = 7        # the largest image range of an axis; the kernels clamp what they read to it


def _pbc_args(what, G, cell, nimg, on_gpu):
    """The cells ``[G, 9]`` and, for the search, the image ranges ``[G, 3]`` of ``G`` graphs."""
    if cell.dim() != 2 or tuple(cell.shape) != (G, 9):
        raise ValueError("%s: cell must be [%d, 9], got %s" % (what, G, tuple(cell.shape)))
    if nimg is not None and tuple(nimg.shape) != (G, 3):
        raise ValueError("%s: nimg must be [%d, 3], got %s" % (what, G, tuple(nimg.shape)))
    if on_gpu:
        _seg_gpu_operands(what, (("nimg", nimg),), (("cell", cell),), ())
    elif not cell.is_floating_point() or (nimg is not None and nimg.is_floating_point()):
        raise TypeError("%s: a floating-point cell and integer nimg expected" % what)
    if checks.enabled() and nimg is not None and nimg.numel():
        if int(nimg.min()) < 0 or int(nimg.max()) > PBC_NIMG_MAX:
            raise ValueError("CGNN_CHECK: %s: nimg outside 0..%d" % (what, PBC_NIMG_MAX))


def _pbc_images(ni):
    """The image box of one graph, int64 ``[M, D]``: ``-ni[a] .. ni[a]`` per axis in
    lexicographic order, the last axis fastest."""
    return torch.cartesian_prod(*[torch.arange(-k, k + 1) for k in ni]).reshape(-1, len(ni))


def _pbc_offset(S, C):
    """``S . C`` by the kernels' definition, ``fma(s2, C[2], fma(s1, C[1], s0 * C[0]))``, for
    shifts ``S`` ``[..., D]`` and cells ``C`` ``[..., D, D]`` (fp32: the fma emulated as in
    ``_sq_dist``; fp64: plain fp64 in the same order)."""
    at = C.dtype
    off = S[..., 0:1].to(at) * C[..., 0, :]
    for a in range(1, S.shape[-1]):
        if at == torch.float32:
            off = (S[..., a:a + 1].double() * C[..., a, :].double() + off.double()).float()
        else:
            off = S[..., a:a + 1].to(at) * C[..., a, :] + off
    return off


def _pack_shift(S):
    """int32 ``[...]`` from shifts ``[..., D]``: byte a = ``S[..., a]`` as an int8, byte 3 = 0."""
    w = torch.zeros(S.shape[:-1], dtype=torch.int64)
    for a in range(S.shape[-1]):
        w |= (S[..., a].long() & 0xFF) << (8 * a)
    return w.to(torch.int32)


def unpack_shift(shift, D=3):
    """int32 ``[nnz, D]`` from the packed ``shift`` ``[nnz]`` of ``radius_pbc_fill``."""
    b = torch.stack([(shift >> (8 * a)) & 0xFF for a in range(int(D))], -1)
    return torch.where(b >= 128, b - 256, b).to(torch.int32)


def _radius_pbc_cpu(pos, D, r, gptr, cell, nimg, loop):
    """(deg, col, shift, d2) of the periodic radius graph on the CPU, graph by graph, in
    ascending (j, image)."""
    n = pos.shape[0]
    at = _acc_dtype(pos.dtype)
    r2 = torch.tensor(r, dtype=at) * torch.tensor(r, dtype=at)
    deg = torch.zeros(n, dtype=torch.int32)
    cols, shs, d2s = [], [], []
    gp = gptr.tolist()
    for g, (g0, g1) in enumerate(zip(gp[:-1], gp[1:])):
        if g1 <= g0:
            continue
        p = pos[g0:g1, :D].to(at)
        S = _pbc_images(nimg[g, :D].clamp(0, PBC_NIMG_MAX).tolist())
        q = p[:, None, :] + _pbc_offset(S, cell[g].view(3, 3)[:D, :D].to(at))[None, :, :]    # [j, m, D]
        d2 = _sq_dist(p[:, None, None, :], q[None, :, :, :])                                     # [i, j, m]
        keep = d2 <= r2                                       # False for NaN
        if not loop:
            home = int((S == 0).all(1).nonzero()[0])
            idx = torch.arange(g1 - g0)
            keep[idx, idx, home] = False
        deg[g0:g1] = keep.sum((1, 2)).to(torch.int32)
        ijm = keep.nonzero()                                  # sorted by (i, j, m)
        cols.append((ijm[:, 1] + g0).to(torch.int32))
        shs.append(_pack_shift(S[ijm[:, 2]]))
        d2s.append(d2[keep])
    col = torch.cat(cols) if cols else torch.zeros(0, dtype=torch.int32)
    shift = torch.cat(shs) if shs else torch.zeros(0, dtype=torch.int32)
    d2 = torch.cat(d2s) if d2s else torch.zeros(0, dtype=at)
    return deg, col, shift, d2


def _max_images(max_images):
    return 1 if max_images is None else max(1, min(int(max_images), (2 * PBC_NIMG_MAX + 1) ** 3))


def radius_pbc_count(pos, D, r, gptr, seg_id, cell, nimg, loop=False, lanes=None, max_images=None, out=None):
    """The count pass of the periodic radius search (gnn_geometry.hip, radius_pbc_kernel):
    ``deg[i]``, int32 ``[n]``, the number of candidates ``(j, s)`` of node i that are kept.  ``j``
    runs over node i's own graph ``g``, the image ``s`` over the box ``-nimg[g, a] <= s[a] <=
    nimg[g, a]``, ``a < D``; kept when ``d2(p_i, p_j + s . C_g) <= r * r``, where ``(j, s) = (i,
    0)`` is left out unless ``loop`` -- ``(i, s != 0)`` is an edge: an atom sees its own images.
    ``cell`` is fp32 ``[G, 9]``, the row-major 3 x 3 cell of each graph (row a = lattice vector
    a, only the leading ``D x D`` block is read); ``nimg`` int32 ``[G, 3]`` with values in
    ``0..PBC_NIMG_MAX`` (0: the axis is not periodic; the kernels clamp to that range).  The
    offset is ``off[c] = fma(s2, C[2][c], fma(s1, C[1][c], s0 * C[0][c]))`` in fp32 with the terms
    of absent axes dropped, the image ``q = p_j + off`` one fp32 add and ``d2`` that of
    ``radius_count`` between ``p_i`` and ``q``: with ``nimg`` all zero the result is
    ``radius_count``'s bit for bit.  Inclusive boundary, a NaN distance is no edge.  For finite
    inputs ``(i, j, s)`` is an edge iff ``(j, i, -s)`` is.  ``pos``, ``gptr``, ``seg_id``, ``lanes``
    and ``out`` as in ``radius_count``; the default ``lanes`` comes from ``n / G * max_images``
    (``max_images``: the largest number of images of a graph, a hint for that choice only).
    Brute force, ``O(n_g^2 M_g)`` per graph.  CPU tensors: PyTorch with the same contract."""
    n, ldp, lanes, r = _radius_args("radius_pbc_count", pos, D, r, gptr, seg_id, lanes)
    _pbc_args("radius_pbc_count", gptr.numel() - 1, cell, nimg, pos.is_cuda)
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=pos.device)
    if checks.enabled():
        checks.rows(out, n, "radius_pbc_count out")
    if pos.is_cuda:
        _seg_gpu_operands("radius_pbc_count", (("gptr", gptr), ("seg_id", seg_id), ("out", out)), (), ())
        native.hip().gnn_radius_pbc_count(pos.data_ptr(), gptr.data_ptr(), seg_id.data_ptr(), cell.data_ptr(),
                                          nimg.data_ptr(), out.data_ptr(), n, gptr.numel() - 1, int(D), ldp, r,
                                          int(bool(loop)), lanes, _max_images(max_images), _st(pos))
        return out
    out[:n] = _radius_pbc_cpu(pos, int(D), r, gptr, cell, nimg, loop)[0]
    return out


def radius_pbc_fill(pos, D, r, gptr, seg_id, cell, nimg, rowptr, loop=False, lanes=None, max_images=None, out=None,
                    shift=None, d2=None, with_d2=False, nnz=None):
    """The fill pass of the periodic radius search: ``col`` / ``shift`` (and ``d2``) at
    ``rowptr[i] .. rowptr[i+1])`` = the kept candidates ``(j, s)`` of node i **in ascending (j,
    m)**, ``m`` the index of ``s`` in lexicographic order with the last axis fastest.  ``shift``
    is int32 ``[nnz]``: byte a holds ``s[a]`` as a two's-complement int8, byte 3 is 0, so 0 is
    the home image (``unpack_shift``).  Returns ``(col, shift, d2)``.  ``rowptr``, ``out`` / ``shift``
    / ``d2`` / ``nnz`` as in ``radius_fill``: nothing at or past ``rowptr[i+1]`` is written for
    row i.  No atomics: the CSR is a function of ``pos``, the graphs, ``cell`` and ``nimg`` alone
    -- not of ``lanes``, the grid or the run.  Contract as in ``radius_pbc_count``."""
    n, ldp, lanes, r = _radius_args("radius_pbc_fill", pos, D, r, gptr, seg_id, lanes)
    _pbc_args("radius_pbc_fill", gptr.numel() - 1, cell, nimg, pos.is_cuda)
    if rowptr.dim() != 1 or rowptr.numel() != n + 1:
        raise ValueError("radius_pbc_fill: rowptr must be [%d], got %s" % (n + 1, tuple(rowptr.shape)))
    if out is None:
        nnz = int(rowptr[-1]) if nnz is None else int(nnz)
        out = torch.empty(nnz, dtype=torch.int32, device=pos.device)
    if shift is None:
        shift = torch.empty(out.numel(), dtype=torch.int32, device=pos.device)
    if d2 is None and with_d2:
        d2 = torch.empty(out.numel(), dtype=_acc_dtype(pos.dtype), device=pos.device)
    if shift.numel() < out.numel():
        raise ValueError("radius_pbc_fill: shift holds %d edges, out %d" % (shift.numel(), out.numel()))
    if checks.enabled():
        _check_ptr(rowptr, 2 ** 31 - 1, "radius_pbc_fill")
        for name, t in (("out", out), ("shift", shift), ("d2", d2)):
            if t is not None and t.numel() < int(rowptr[-1]):
                raise ValueError("CGNN_CHECK: radius_pbc_fill: %s holds %d edges, rowptr ends at %d"
                                 % (name, t.numel(), int(rowptr[-1])))
    if pos.is_cuda:
        _seg_gpu_operands("radius_pbc_fill", (("gptr", gptr), ("seg_id", seg_id), ("rowptr", rowptr), ("out", out),
                                              ("shift", shift)), (("d2", d2),), ())
        if out.numel() == 0:                                  # no edge to write (a null pointer)
            return out, shift, d2
        native.hip().gnn_radius_pbc_fill(pos.data_ptr(), gptr.data_ptr(), seg_id.data_ptr(), cell.data_ptr(),
                                         nimg.data_ptr(), rowptr.data_ptr(), out.data_ptr(), shift.data_ptr(),
                                         _ptr(d2), n, gptr.numel() - 1, int(D), ldp, r, int(bool(loop)), lanes,
                                         _max_images(max_images), _st(pos))
        return out, shift, d2
    deg, col, sh, dd = _radius_pbc_cpu(pos, int(D), r, gptr, cell, nimg, loop)
    _fill_rows(deg, col, dd, rowptr, out, d2)
    _fill_rows(deg, sh, dd, rowptr, shift, None)
    return out, shift, d2


def _pair_pbc_args(what, n, shift, nnz, cell, seg_id, on_gpu):
    if shift.dim() != 1 or shift.numel() < nnz:
        raise ValueError("%s: shift must hold %d edges, got %s" % (what, nnz, tuple(shift.shape)))
    if seg_id.dim() != 1 or seg_id.numel() < n:
        raise ValueError("%s: seg_id must hold %d rows, got %s" % (what, n, tuple(seg_id.shape)))
    if cell.dim() != 2 or cell.shape[1] != 9 or (cell.shape[0] < 1 and n):
        raise ValueError("%s: cell must be [G, 9] with G >= 1, got %s" % (what, tuple(cell.shape)))
    _pbc_args(what, cell.shape[0], cell, None, on_gpu)
    if on_gpu:
        _seg_gpu_operands(what, (("shift", shift), ("seg_id", seg_id)), (), ())
    if checks.enabled():
        checks.index(seg_id[:n], max(cell.shape[0], 1), what + " seg_id")


def _edge_offsets(rows, shift, cell, seg_id, D, at):
    """``shift[e] . cell(graph of row(e))`` ``[E, D]`` in ``at``, by the kernels' definition."""
    C = cell.view(-1, 3, 3)[seg_id[rows].long()][:, :D, :D].to(at)
    return _pbc_offset(unpack_shift(shift[:rows.numel()], D).long(), C)


def pair_d2_pbc(rowptr, col, shift, pos, D, cell, seg_id, out=None, lanes=None, nnz=None):
    """``pair_d2`` for a CSR with image shifts (gnn_geometry.hip, pair_d2_pbc_kernel):
    ``d2[e] = d2(p_i, p_col[e] + s_e . C)`` for the edges e of row i, ``s_e`` unpacked from
    ``shift[e]`` (``radius_pbc_fill``'s format; any int8 values) and ``C = cell[seg_id[i]]``
    (``cell`` fp32 ``[G, 9]``, ``seg_id`` int32 ``[n]``; a ``seg_id`` outside ``[0, G)`` reads a zero
    cell).  The offset and the sum are those of ``radius_pbc_count``: on a periodic radius graph
    it reproduces ``radius_pbc_fill``'s ``d2`` bit for bit.  ``out`` / ``lanes`` / ``nnz`` as in
    ``pair_d2``.  CPU tensors: PyTorch (fp64 for fp64 positions)."""
    n, ldp, lanes, nnz = _pair_args("pair_d2_pbc", rowptr, col, pos, D, lanes, nnz)
    _pair_pbc_args("pair_d2_pbc", n, shift, nnz, cell, seg_id, pos.is_cuda)
    if out is None:
        out = torch.empty(nnz, dtype=_acc_dtype(pos.dtype), device=pos.device)
    if out.numel() < nnz:
        raise ValueError("pair_d2_pbc: out holds %d edges, nnz = %d" % (out.numel(), nnz))
    if pos.is_cuda:
        _seg_gpu_operands("pair_d2_pbc", (("rowptr", rowptr), ("col", col)), (("out", out),), ())
        native.hip().gnn_pair_d2_pbc(rowptr.data_ptr(), col.data_ptr(), shift.data_ptr(), pos.data_ptr(),
                                     cell.data_ptr(), seg_id.data_ptr(), out.data_ptr(), n, nnz, cell.shape[0],
                                     int(D), ldp, lanes, _st(pos))
        return out
    D = int(D)
    rows = _row_ids(rowptr)
    E = rows.numel()
    at = _acc_dtype(pos.dtype)
    q = pos[col[:E].long(), :D].to(at) + _edge_offsets(rows, shift, cell, seg_id, D, at)
    out[:E] = _sq_dist(pos[rows, :D].to(at), q).to(out.dtype)
    return out


def pair_d2_pbc_bwd(rowptr, col, shift, rowptr_t, col_t, eperm_t, pos, g, D, cell, seg_id, out=None, lanes=None,
                    nnz=None):
    """``pair_d2_bwd`` through ``pair_d2_pbc`` (gnn_geometry.hip, pair_d2_pbc_bwd_kernel):

        dpos[i] = 2 (sum_{e in in(i)} g[e] (p_i - (p_src(e) + off_e)) + sum_{e in out(i)} g[e] (p_i - (p_dst(e) - off_e)))

    with ``off_e = s_e . C`` as in ``pair_d2_pbc``.  Operands, order of the sum, ``out`` and the
    CPU branch as in ``pair_d2_bwd``; the gradient goes to the positions only (none to the
    cell).  The CSR must be **block diagonal over the graphs** -- both ends of every edge with
    the same ``seg_id``, as in every ``GraphBatch``: the offset of an edge is defined by the cell
    of its destination row, and the kernel reads the out-edges of a node with the node's own
    cell (``CGNN_CHECK`` verifies it)."""
    n, ldp, lanes, nnz = _pair_args("pair_d2_pbc_bwd", rowptr, col, pos, D, lanes, nnz)
    _pair_pbc_args("pair_d2_pbc_bwd", n, shift, nnz, cell, seg_id, pos.is_cuda)
    if n != pos.shape[0] or rowptr_t.numel() != n + 1:
        raise ValueError("pair_d2_pbc_bwd: a square CSR over the %d positions expected (%d rows, %d transposed rows)"
                         % (pos.shape[0], n, rowptr_t.numel() - 1))
    if g.dim() != 1 or g.numel() < nnz or col_t.numel() < nnz or eperm_t.numel() < nnz:
        raise ValueError("pair_d2_pbc_bwd: g, col_t and eperm_t must hold %d edges" % nnz)
    if out is None:
        out = torch.empty_like(pos)
    if out.shape != pos.shape:
        raise ValueError("pair_d2_pbc_bwd: out must be %s like pos, got %s" % (tuple(pos.shape), tuple(out.shape)))
    if checks.enabled():
        checks.csr(rowptr_t, col_t, n, "pair_d2_pbc_bwd (transposed)")
        checks.index(eperm_t[:nnz], max(nnz, 1), "pair_d2_pbc_bwd eperm_t")
        ends = _row_ids(rowptr)
        if not torch.equal(seg_id[ends.long()], seg_id[col[:ends.numel()].long()]):
            raise ValueError("CGNN_CHECK: pair_d2_pbc_bwd: an edge joins two graphs (seg_id of its ends differ)")
    if n == 0 or nnz == 0:
        return out.zero_()
    if pos.is_cuda:
        _seg_gpu_operands("pair_d2_pbc_bwd", (("rowptr", rowptr), ("col", col), ("rowptr_t", rowptr_t),
                                              ("col_t", col_t), ("eperm_t", eperm_t)), (("g", g), ("out", out)), ())
        native.hip().gnn_pair_d2_pbc_bwd(rowptr.data_ptr(), col.data_ptr(), shift.data_ptr(), rowptr_t.data_ptr(),
                                         col_t.data_ptr(), eperm_t.data_ptr(), pos.data_ptr(), cell.data_ptr(),
                                         seg_id.data_ptr(), g.data_ptr(), out.data_ptr(), n, nnz, cell.shape[0],
                                         int(D), ldp, lanes, _st(pos))
        return out
    D = int(D)
    at = _acc_dtype(pos.dtype)
    rows = _row_ids(rowptr)
    E = rows.numel()
    src = col[:E].long()
    p = pos[:, :D].to(at)
    w = g[:E].to(at)[:, None] * (p[rows] - (p[src] + _edge_offsets(rows, shift, cell, seg_id, D, at)))
    acc = torch.zeros(n, D, dtype=at).index_add_(0, rows, w).index_add_(0, src, -w)
    out.zero_()
    out[:, :D] = (2 * acc).to(out.dtype)
    return out


def spmm_fan(rowptr, col, X, F, max_deg, rscale=None, out=None):
    """``spmm`` (bf16, no bias / init / column scale) for rows of at most ``max_deg``
    entries -- a sampled block whose fanout bounds every row: at most 8, a pipelined
    persistent kernel (gnn_sparse.hip, spmm_fan_pipe_kernel); same sums, bit for bit."""
    n = rowptr.numel() - 1
    if out is None:
        out = torch.empty(n, X.shape[1], dtype=torch.bfloat16, device=X.device)
    if not X.is_cuda:
        return spmm(rowptr, col, X, F, rscale=rscale, out=out)
    if X.dtype != torch.bfloat16 or out.dtype != torch.bfloat16:
        raise TypeError("spmm_fan: bf16 in and out")
    if checks.enabled():
        checks.csr(rowptr, col, X.shape[0], "spmm_fan")
        checks.rows(out, n, "spmm_fan out")
        checks.rows(rscale, n, "spmm_fan rscale")
        if n > 0 and int((rowptr[1:] - rowptr[:-1]).max()) > max_deg:
            raise ValueError("spmm_fan: a row has more than max_deg = %d entries" % max_deg)
    # (the pipelined kernel reads col through a descriptor of nnz records, but a bound
    # above 8 or a wide row falls back to the CSR SpMM and its unconditional first load)
    native.hip().gnn_spmm_fan(rowptr.data_ptr(), _nonempty_ids(col).data_ptr(), X.data_ptr(), out.data_ptr(),
                              rscale.data_ptr() if rscale is not None else 0, n, F, X.shape[1], out.shape[1],
                              X.shape[0], col.numel(), int(max_deg), _st(X))
    return out


_DB_INDEX = {}


class EllImage:
    """ELL image of a CSR for ``spmm_ell``.  ``ell``: int32 [n, 8], the row's column ids
    (-1 past its end), or {-2, e0, e1, -1...} for a row of more than 8 entries (its CSR
    range); ``long_rows``: int32 [n_long], the ids of those rows, ascending (the GPU
    sums them in a launch of their own, so the short-row loop has no data-dependent
    inner loop); ``long_buf``: the buffer whose pointer the GPU launch gets -- ``long_rows``,
    or one unused element when there is none (an empty tensor's pointer is null, which the
    launcher reads as "no list" and answers with the one-shot kernel)."""
    __slots__ = ("ell", "long_rows", "n_long", "long_buf")

    def __init__(self, ell, long_rows):
        self.ell, self.long_rows, self.n_long = ell, long_rows, int(long_rows.numel())
        self.long_buf = long_rows if self.n_long else torch.zeros(1, dtype=torch.int32, device=long_rows.device)

    @property
    def n(self):
        return self.ell.shape[0]


def ell_image(rowptr, col):
    """:class:`EllImage` of the CSR (rowptr, col), built once at setup."""
    n = rowptr.numel() - 1
    ell = torch.empty(n, 8, dtype=torch.int32, device=col.device)
    rp = rowptr.long()
    deg = rp[1:] - rp[:-1]
    long_rows = torch.nonzero(deg > 8).flatten().to(torch.int32).contiguous()
    if col.is_cuda:
        native.hip().gnn_ell_build(rowptr.data_ptr(), col.data_ptr(), ell.data_ptr(), n, _st(col))
        return EllImage(ell, long_rows)
    ell.fill_(-1)
    for u in range(8):
        has = deg > u
        ell[has, u] = col[(rp[:-1] + u)[has]]
    longr = deg > 8
    ell[longr] = -1
    ell[longr, 0] = -2
    ell[longr, 1] = rp[:-1][longr].to(torch.int32)
    ell[longr, 2] = rp[1:][longr].to(torch.int32)
    return EllImage(ell, long_rows)


def spmm_ell(img, col, X, F, rscale=None, out=None, oneshot=False):
    """Y[i,:F] = rscale[i] * sum_{j in N(i)} X[j,:F] from an :class:`EllImage` (bf16,
    F <= 64; the same sums as ``spmm`` over the CSR the image was built from).
    ``oneshot`` (GPU): the one-shot kernel (the launcher's choice for tables of 2^31
    bytes or more) instead of the pipelined one; bit-identical."""
    ell = img.ell
    n = ell.shape[0]
    if out is None:
        out = torch.empty(n, X.shape[1], dtype=torch.bfloat16, device=X.device)
    if X.is_cuda:
        native.hip().gnn_spmm_ell(ell.data_ptr(), col.data_ptr(), X.data_ptr(), out.data_ptr(),
                                  rscale.data_ptr() if rscale is not None else 0, n, F, X.shape[1],
                                  out.shape[1], X.shape[0], 0 if oneshot else img.long_buf.data_ptr(),
                                  img.n_long, _st(X))
        return out
    acc = torch.zeros(n, F, dtype=torch.float32)
    short = ell[:, 0] != -2                    # a long row's slots hold its CSR range
    for u in range(8):
        j = ell[:, u].long()
        ok = (j >= 0) & short
        acc[ok] += X[j[ok], :F].float()
    longr = (~short).nonzero().flatten()
    for i in longr.tolist():
        e0, e1 = int(ell[i, 1]), int(ell[i, 2])
        acc[i] = X[col[e0:e1].long(), :F].float().sum(0)
    if rscale is not None:
        acc = acc * rscale[:, None]
    out[:n].zero_()
    out[:n, :F] = acc.to(out.dtype)
    return out


CE_LONG_DEGREE = 256     # rows above this degree get a wave of their own in spmm_ce


def long_row_order(deg: torch.Tensor, threshold: Optional[int] = None):
    """Row order for ``spmm_ce(..., n_long=k)``: the rows of degree > threshold first (in
    their original order), then the others; returns (order, k).  Default threshold
    CE_LONG_DEGREE; 0 disables the long-row mode."""
    if threshold is None:
        threshold = CE_LONG_DEGREE
    if threshold <= 0:
        return torch.arange(deg.numel(), device=deg.device), 0
    longr = deg > threshold
    order = torch.cat([torch.nonzero(longr).flatten(), torch.nonzero(~longr).flatten()])
    return order, int(longr.sum())


def spmm_ce(rowptr, col, Z, C, rscale, bias, labels, mask, inv_count, mode=0, G=None, init=None, gslot=None,
            db_out=None, n_long=0, stats_out=None, bump=None):
    """Layer-2 aggregate + log-softmax + NLL.  Returns (stats[68] summed, G).
    ``init`` (optional fp32 [n, >=C]): partial sums of other edges.
    ``gslot`` (optional int32 [n]): G is compact -- row i (a train row, gslot[i] >= 0)
    goes to G[gslot[i]], other rows (whose dlogits are zero) are not written.
    ``db_out`` (optional fp32 [C], GPU): the per-class dlogits sums (the bias gradient,
    stats[4:4 + C]) are also summed straight into it -- a second fixed-order pass over
    the partials instead of a device-to-device copy.
    ``n_long``: rows [0, n_long) are long rows the caller ordered first; the GPU kernel
    gives each of them a whole wave (see ``long_row_order``).  Results do not depend on it.
    ``stats_out`` = (buffer, index) (GPU): ONE fixed-order reduction writes column c of
    the 68 to buffer[index[c]] (index < 0: dropped) and that buffer is returned -- e.g.
    the loss / accuracy sums to a scratch tail and the per-class dlogits sums straight
    into the bias gradient, with no copy or second pass."""
    if checks.enabled():
        checks.csr(rowptr, col, Z.shape[0], "spmm_ce")
        checks.rows(labels, rowptr.numel() - 1, "spmm_ce labels")
        checks.rows(mask, rowptr.numel() - 1, "spmm_ce mask")
    n = rowptr.numel() - 1
    ld = Z.shape[1]
    if Z.is_cuda:
        hip = native.hip()
        nb = hip.gnn_spmm_ce_blocks(n, int(n_long))
        stats = torch.empty(nb, 68, dtype=torch.float32, device=Z.device)
        if G is None and mode == 0:
            if gslot is not None:
                raise ValueError("a compact G (gslot) must be allocated by the caller")
            G = torch.empty(n, ld, dtype=torch.bfloat16, device=Z.device)
        if gslot is not None and gslot.dtype != torch.int32:
            raise TypeError("gslot must be int32")
        hip.gnn_spmm_ce(rowptr.data_ptr(), _nonempty_ids(col).data_ptr(), Z.data_ptr(), rscale.data_ptr(),
                        bias.data_ptr(), labels.data_ptr(), mask.data_ptr(), stats.data_ptr(),
                        G.data_ptr() if G is not None else 0,
                        init.data_ptr() if init is not None else 0, init.shape[1] if init is not None else 0,
                        n, C, ld, mode, float(inv_count), _st(Z),
                        gslot.data_ptr() if gslot is not None else 0, int(n_long))
        if stats_out is not None:
            buf, index = stats_out
            slab_sum(stats, buf, index=index)
            return buf, G
        out = torch.empty(68, dtype=torch.float32, device=Z.device)
        slab_sum(stats, out)
        if db_out is not None:
            key = (Z.device, C)
            idx = _DB_INDEX.get(key)
            if idx is None:
                c = torch.arange(68, dtype=torch.int32)
                idx = _DB_INDEX[key] = torch.where((c >= 4) & (c < 4 + C), c - 4, -1).to(torch.int32).to(Z.device)
            slab_sum(stats, db_out, index=idx, bump=bump)
        elif bump is not None:
            raise ValueError("spmm_ce: bump rides on the db_out reduction")
        return out, G
    rows = _row_ids(rowptr)
    acc = torch.zeros(n, C, dtype=torch.float32)
    acc.index_add_(0, rows, Z[col.long(), :C].float())
    if init is not None:
        acc = acc + init[:n, :C].float()
    logits = acc * rscale[:, None] + bias[:C]
    lsm = torch.log_softmax(logits, 1)
    y = labels.long()
    tr = mask == 1
    stats = torch.zeros(68)
    stats[0] = -(lsm[tr, y[tr]]).sum()
    pred = logits.argmax(1)
    for k in (1, 2, 3):
        stats[k] = ((pred == y) & (mask == k)).sum().float()
    dl = torch.softmax(logits, 1)
    dl[torch.arange(n), y] -= 1
    dl = dl * (tr[:, None].float() * inv_count)
    stats[4:4 + C] = dl.sum(0)
    if mode == 0:
        gval = (dl * rscale[:, None]).to(Z.dtype)
        if gslot is not None:
            sel = gslot >= 0
            G[gslot[sel].long(), :C] = gval[sel].to(G.dtype)
            G[gslot[sel].long(), C:] = 0
        else:
            if G is None:
                G = torch.zeros(n, ld, dtype=Z.dtype)
            G.zero_()
            G[:, :C] = gval.to(G.dtype)
    return stats, G


_STAGE = {}


def slab_sum(P, out, index=None, groups=None, bump=None):
    """out[index[c]] = sum_r P[r, c] (``index`` None: out[c]; index < 0: dropped) -- the
    fixed-order column sum of per-block partials (deterministic, no atomics), in one pass
    or, for more than 256 rows, two (``groups`` row groups: 512 above 4096 rows, else one
    group per 32 rows -- a one-pass sum of a few thousand rows is a serial load chain per
    lane in the two blocks of a 68-column reduce, 14 us on arxiv's cross-entropy stats).
    On the CPU: the same sums with torch.
    ``bump`` (GPU, int32[1]): incremented by the final pass (a step counter advanced
    without a launch of its own)."""
    S, W = P.shape
    if not P.is_cuda:
        v = P.sum(0)
        if index is None:
            out[:W] = v
        else:
            keep = index >= 0
            out[index[keep].long()] = v[keep]
        return out
    if not (P.dtype == torch.float32 and out.dtype == torch.float32 and P.is_contiguous()):
        raise TypeError("slab_sum: contiguous fp32 partials and fp32 output expected")
    if index is not None and (index.dtype != torch.int32 or index.numel() != W):
        raise TypeError("slab_sum: index must be int32 of the partials' width")
    G = groups if groups is not None else (512 if S > 4096 else (-(-S // 32) if S > 256 else 1))
    stage = None
    if G > 1:
        key = (P.device, G * W)
        stage = _STAGE.get(key)
        if stage is None:
            stage = _STAGE[key] = torch.empty(G * W, dtype=torch.float32, device=P.device)
    native.hip().gnn_slab_sum(P.data_ptr(), S, W, stage.data_ptr() if stage is not None else 0, G,
                              out.data_ptr(), index.data_ptr() if index is not None else 0, _st(P),
                              bump.data_ptr() if bump is not None else 0)
    return out


def tall_gemm_tn(A: torch.Tensor, B: torch.Tensor, chunk: int = 8192) -> torch.Tensor:
    """A^T B (fp32) for tall A [M, k1], B [M, k2] with tiny k1 x k2: a plain GEMM
    would give the whole M-long reduction to k1*k2/tile^2 workgroups (16 for
    256 x 256 on 64 x 64 tiles -- 6 % of the CUs); instead split K into row
    chunks as ONE batched GEMM with fp32 partials and sum them in fixed order."""
    M = A.shape[0]
    S = M // chunk
    cuda = A.is_cuda
    out = None
    if S:
        a = A[:S * chunk].reshape(S, chunk, A.shape[1]).transpose(1, 2)
        b = B[:S * chunk].reshape(S, chunk, B.shape[1])
        if cuda and A.dtype != torch.float32:
            out = torch.bmm(a, b, out_dtype=torch.float32).sum(0)
        else:
            out = torch.bmm(a.float(), b.float()).sum(0)
    if M > S * chunk:
        a, b = A[S * chunk:], B[S * chunk:]
        if cuda and A.dtype != torch.float32:
            tail = torch.mm(a.t(), b, out_dtype=torch.float32)
        else:
            tail = a.float().t() @ b.float()
        out = tail if out is None else out + tail
    return out


DROP_BIT_CTR = 0x80000000


def dropout_keep_mask(rows: int, F: int, p: float, key, step, row0: int = 0) -> torch.Tensor:
    """Keep mask of the fused dropout (host mirror of cgnn_common.h drop_draw /
    drop_keep16).  Element (row, n), n = 32 t + 8 g + 4 h + i, q = 4 g + i:
      byte mode (any p): byte q of the Philox draw keyed (row, 2 t + h, step), kept if
      >= thr8 = round(256 p);
      bit mode (p = 1/2, thr8 = 128): bit 16 (t % 8) + q of the draw keyed
      (row, DROP_BIT_CTR + 2 (t // 8) + h, step), kept if set (one bit per decision)."""
    import numpy as np
    thr8 = min(255, int(np.floor(p * 256.0 + 0.5)))
    if thr8 == 0:
        return torch.ones(rows, F, dtype=torch.bool)
    r = (row0 + np.arange(rows)).astype(np.uint32)[:, None]
    n = np.arange(F)
    t, h = n // 32, (n // 4) % 2
    q = (n % 4) + 4 * ((n % 32) // 8)
    if thr8 == 128:
        ctr = (DROP_BIT_CTR + 2 * (t // 8) + h).astype(np.uint32)[None, :]
        b = 16 * (t % 8) + q
    else:
        ctr = (2 * t + h).astype(np.uint32)[None, :]
        b = 8 * q
    words = np.stack(philox.philox4x32_10(r, ctr, step, philox.RNG_DROPOUT, key[0], key[1]), -1)
    wsel = np.take_along_axis(words, (b // 32)[None, :, None].repeat(rows, 0), -1)[..., 0]
    bits = wsel >> (b % 32).astype(np.uint32)[None, :]
    if thr8 == 128:
        return torch.from_numpy((bits & 1) == 1)
    return torch.from_numpy((bits & 0xFF) >= thr8)


def bias_relu_dropout_(H, bias, F, p, key, step, row0=0):
    """In place: H = dropout(relu(H + bias)); the mask is keyed by the GLOBAL row
    (row0 + local row), so it does not depend on how rows are partitioned."""
    if H.is_cuda:
        native.hip().gnn_bias_relu_dropout(H.data_ptr(), bias.data_ptr(), H.shape[0], F, H.shape[1],
                                           float(p), int(key[0]), int(key[1]), int(step), int(row0), _st(H))
        return H
    x = torch.relu(H[:, :F].float() + bias[:F])
    if p > 0:
        keep = dropout_keep_mask(H.shape[0], F, p, key, step, row0)
        x = torch.where(keep, x / (1 - p), torch.zeros_like(x))
    H.zero_()
    H[:, :F] = x.to(H.dtype)
    return H


def _step_args(step):
    """(scalar step, device pointer): a device int32 tensor is read by the kernel at
    launch time (hipGraph replays see the current value), an int is passed by value."""
    if isinstance(step, torch.Tensor):
        return 0, step.data_ptr()
    return int(step), 0


def _step_value(step):
    return int(step.item()) if isinstance(step, torch.Tensor) else int(step)


def keep_image(n, hidden, device):
    """Buffer of a keep image (the dropout masks of an n-row, ``hidden``-wide GCN layer as
    the fused backward reads them: 1 bit per element, whole 32-row tiles)."""
    hw = native.hip().gnn_keep_image_halfwords(int(n), int(hidden))
    return torch.empty(hw, dtype=torch.int16, device=device)


def draw_keep_image(kimg, n, hidden, p, key, step, row0=0):
    """Fill ``kimg`` with the masks dense_fwd draws for the same (n, p, key, step, row0)."""
    sv, sp = _step_args(step)
    rc = native.hip().gnn_keep_image(kimg.data_ptr(), int(n), int(hidden), float(p), int(key[0]), int(key[1]), sv,
                                     int(row0), _st(kimg), step_ptr=sp)
    if rc != 0:
        raise RuntimeError("gnn_keep_image failed (%d)" % rc)
    return kimg


def dense_fwd(AX, W1, b1, W2, dinv, H1, Z2, F, p, key, step, row0=0, kimg=None):
    """H1 = dropout(relu(AX[:, :F] W1 + b1)), Z2 = dinv * (H1 W2) (fused MFMA kernel on GPU).
    ``H1=None`` (GPU only): H1 is not stored -- the fused backward recomputes it.
    ``step``: the dropout step, an int or a device int32[1] tensor.  ``kimg`` (GPU, a
    ``keep_image`` buffer): also write the dropout masks for the fused backward."""
    n = Z2.shape[0]
    HD, C = W1.shape[1], W2.shape[1]
    if AX.is_cuda:
        sv, sp = _step_args(step)
        rc = native.hip().gnn_dense_fwd(AX.data_ptr(), W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
                                        dinv.data_ptr(), H1.data_ptr() if H1 is not None else 0,
                                        Z2.data_ptr(), n, F, AX.shape[1],
                                        HD, C, Z2.shape[1], float(p), int(key[0]), int(key[1]), sv,
                                        int(row0), _st(AX), step_ptr=sp,
                                        kimg=kimg.data_ptr() if kimg is not None else 0)
        if rc == 0:
            return True
        if rc != -1:
            raise RuntimeError("gnn_dense_fwd failed (%d)" % rc)
        return False          # shape not covered by a compiled variant
    H1.copy_((AX[:n, :F].float() @ W1.to(torch.bfloat16).float()).to(torch.bfloat16))
    bias_relu_dropout_(H1, b1, HD, p, key, _step_value(step), row0)
    y2 = H1.float() @ W2.to(torch.bfloat16).float()
    Z2.zero_()
    Z2[:, :C] = (y2 * dinv[:n, None]).to(torch.bfloat16)
    return True


def dense_bwd(dY2, W2, H1, dP1, p):
    """dP1 = (dY2 W2^T) * [H1 > 0] / (1-p)."""
    n = dP1.shape[0]
    HD, C = W2.shape
    if dY2.is_cuda:
        rc = native.hip().gnn_dense_bwd(dY2.data_ptr(), W2.data_ptr(), H1.data_ptr(), dP1.data_ptr(), n,
                                        HD, C, dY2.shape[1], float(p), _st(dY2))
        if rc == 0:
            return True
        if rc != -1:
            raise RuntimeError("gnn_dense_bwd failed (%d)" % rc)
        return False
    g = dY2[:n, :C].float() @ W2.to(torch.bfloat16).float().t()
    dP1.copy_(torch.where(H1[:n].float() > 0, g / (1 - p), torch.zeros_like(g)).to(torch.bfloat16))
    return True


def fused_bwd_supported(F, hidden, C):
    """Whether a compiled fused-backward variant covers F features (+ the ones column),
    ``hidden`` units and C classes (the row pitches only need to cover them)."""
    return bool(native.hip().gnn_fused_bwd_supported(int(F) + 1, int(hidden), int(C)))


def fused_bwd(AX, dY2, W1, b1, W2, n, F, p, key, step, row0=0, gpart=None, grads=None, grad_index=None,
              kimg=None):
    """Fused GCN dense backward (GPU): recomputes H1 from AX, then
    dP1 = (dY2 W2^T) * [H1 > 0] / (1-p) and the weight gradients in one pass.
    The dropout masks come from ``kimg``, the keep image the forward wrote
    (``dense_fwd(..., kimg=)``); without one they are drawn here from (key, step, row0).
    Returns (gW1 [F, HD], gb1 [HD], gW2 [HD, C], gpart); with ``grads`` (the flat fp32
    gradient buffer, gW1 | gb1 | gW2 at its start) the sums are written there instead
    and (None, None, None, gpart) is returned."""
    hip = native.hip()
    HD, C = W1.shape[1], W2.shape[1]
    ldx = AX.shape[1]
    nb, width = hip.gnn_fused_bwd_blocks(n), hip.gnn_fused_bwd_width(F + 1)
    if gpart is None or gpart.shape != (nb, HD, width):
        gpart = torch.empty(nb, HD, width, dtype=torch.float32, device=AX.device)
    if p > 0 and kimg is None:
        kimg = draw_keep_image(keep_image(n, HD, AX.device), n, HD, p, key, step, row0)
    rc = hip.gnn_fused_bwd(AX.data_ptr(), dY2.data_ptr(), W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
                           kimg.data_ptr() if kimg is not None else 0, gpart.data_ptr(), n, F, ldx, HD, C,
                           dY2.shape[1], float(p), _st(AX))
    if rc != 0:
        raise RuntimeError("gnn_fused_bwd failed (%d)" % rc)
    if grads is not None:
        # fixed-order reduction over the block slabs, scattered straight into the flat
        # gradient buffer [gW1 (F x HD) | gb1 | gW2 (HD x C) | ...]
        if grad_index is None:
            grad_index = fused_bwd_grad_index(F, HD, C, width, device=AX.device)
        slab_sum(gpart.view(nb, HD * width), grads, grad_index)
        return None, None, None, gpart
    g = gpart.sum(0)                     # fixed-order reduction over the block slabs
    kf = width - 64
    return g[:, :F].t(), g[:, F], g[:, kf:kf + C], gpart


def fused_bwd_width(F):
    """Row width of a fused-backward slab for F features (+ the ones column)."""
    return native.hip().gnn_fused_bwd_width(int(F) + 1)


def fused_bwd_grad_index(F, HD, C, width, device=None):
    """Destination in the flat gradient buffer [gW1 (F x HD) | gb1 (HD) | gW2 (HD x C)] of
    every element (h, j) of a fused-backward slab [HD][width] (-1: padding)."""
    kf = width - 64
    h = torch.arange(HD).view(HD, 1)
    j = torch.arange(width).view(1, width)
    n1 = F * HD
    idx = torch.full((HD, width), -1, dtype=torch.int64)
    idx = torch.where(j < F, j * HD + h, idx)
    idx = torch.where(j == F, n1 + h, idx)
    idx = torch.where((j >= kf) & (j < kf + C), n1 + HD + h * C + (j - kf), idx)
    return idx.view(-1).to(torch.int32).to(device)


def relu_dropout_bwd_(dH, H, p):
    if dH.is_cuda:
        native.hip().gnn_relu_dropout_bwd(dH.data_ptr(), H.data_ptr(), dH.numel(), float(p), _st(dH))
        return dH
    dH.copy_(torch.where(H.float() > 0, dH.float() / (1 - p), torch.zeros_like(dH, dtype=torch.float32)).to(dH.dtype))
    return dH


_ADAM_DONE = {}


def adam_(param, grad, m, v, lr, step_t, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, step_done=False):
    """PyTorch-semantics Adam on flat fp32 buffers; ``step_t`` is a device int32[1]
    holding the number of completed steps (incremented here).  On a GPU, for up to 256
    blocks of parameters, the kernel's last-arriving block increments it (a zeroed
    arrival counter kept per step tensor) instead of a separate launch: the GCN epoch
    +0.3 % (profiles/r06_sage/adam_fold).  Larger grids keep the launch -- 1.2 K blocks
    counting on one address measured slower (GraphSAGE).  ``step_done`` (GPU): a
    reduction before this update already advanced ``step_t`` (slab_sum's bump)."""
    if param.is_cuda and step_done:
        native.hip().gnn_adam(param.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), param.numel(),
                              float(lr), float(b1), float(b2), float(eps), float(wd), step_t.data_ptr(),
                              _st(param), 0, 1)
        return param
    if param.is_cuda:
        fold = param.numel() <= 256 * 256
        done = None
        if fold:
            key = (step_t.device.index, step_t.data_ptr())
            done = _ADAM_DONE.get(key)
            if done is None:
                done = _ADAM_DONE[key] = torch.zeros(1, dtype=torch.int32, device=step_t.device)
        native.hip().gnn_adam(param.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), param.numel(),
                              float(lr), float(b1), float(b2), float(eps), float(wd), step_t.data_ptr(),
                              _st(param), done.data_ptr() if fold else 0)
        if not fold:
            step_t.add_(1)
        return param
    t = float(step_t.item()) + 1
    m.mul_(b1).add_(grad, alpha=1 - b1)
    v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
    mh = m / (1 - b1 ** t)
    vh = v / (1 - b2 ** t)
    param.sub_(lr * (mh / (vh.sqrt() + eps) + wd * param))
    step_t.add_(1)
    return param
