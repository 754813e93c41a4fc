"""Autograd building blocks for GNNs of any depth on the HIP kernels -- GNN
track, not in the reference.

* ``norm_aggregate`` -- ``Y = D^-1/2 (A+I) D^-1/2 X`` on the CSR of A + I.  The
  column scale is applied in the gather (one float per gathered row), the row
  scale in the SpMM epilogue, so no per-edge value is read.  The normalised adjacency is
  symmetric, so the backward is the same SpMM on the incoming gradient (no
  transposed CSR).
* ``gcn_layer`` / ``GCNConv`` -- ``act(Â (H W) + b)`` (transform first: the
  gathered rows are the narrower of the two widths) with the normalisation,
  bias and ReLU inside the SpMM and a split-K weight gradient.
* ``GCN`` -- L layers with ReLU + dropout between them.
* ``WeightedGraph`` / ``weighted_aggregate`` -- the same layers over a directed graph
  with one value per edge (``ops.wspmm``): the backward runs over the transposed CSR,
  and the edge values receive a gradient (``ops.sddmm``) when they require one.
* ``pool_aggregate`` -- element-wise max / min over each node's neighbours
  (``ops.pool``), the gradient routed through the saved edge index (``ops.pool_bwd``).
* ``edge_softmax`` / ``edge_dot`` / ``AttentionConv`` -- attention of any score form: a
  softmax over each node's incoming edges (``ops.edge_softmax``), per-edge dot products
  (``ops.sddmm``, differentiable through ``ops.wspmm``), and multi-head dot-product
  attention built from them.
* ``edge_aggregate`` / ``GINEConv`` / ``CFConv`` -- message passing with a feature row per
  edge (``ops.espmm``): ``sum_j relu(x_j + e_ij)`` or ``sum_j x_j * e_ij``, differentiable in
  the node rows, the edge rows (``ops.egrad``) and optional per-edge weights; GIN with edge
  features and SchNet's continuous-filter convolution built on it.

The step these models end in -- one row per graph of a batch of graphs -- is in
``gnn/readout.py`` (``GraphBatch``, ``graph_readout``, ``graph_broadcast``, ``GlobalAttention``).

Everything runs on the same ``ops.spmm`` as the fused 2-layer trainer (HIP on
GPU tensors, PyTorch index ops on CPU tensors); dense products are hipBLASLt
GEMMs.  Storage dtype follows the input (fp32 / bf16 / fp16); aggregation
accumulates in fp32.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import ops


def pad_cols(x: torch.Tensor, mult: int = 8) -> torch.Tensor:
    F = x.shape[1]
    return x if F % mult == 0 else torch.nn.functional.pad(x, (0, mult - F % mult))


class NormGraph:
    """CSR of A + I with the symmetric normalisation vector ``dinv``."""

    def __init__(self, rowptr: torch.Tensor, col: torch.Tensor, dinv: torch.Tensor):
        self.rowptr, self.col, self.dinv = rowptr.contiguous(), col.contiguous(), dinv.contiguous()
        self.n = rowptr.numel() - 1
        self._tperm = None

    @classmethod
    def from_data(cls, g) -> "NormGraph":
        return cls(g.rowptr, g.col, g.dinv)

    def transposed_perm(self):
        """``(rowptr_t, col_t, eperm)`` of the transpose, as ``WeightedGraph.transposed``
        (the pooling backward needs the edge permutation).  Built once."""
        if self._tperm is None:
            from .sage import transpose_csr
            self._tperm = transpose_csr(self.rowptr, self.col, self.n, with_perm=True)
        return self._tperm


def aggregate(x: torch.Tensor, g: NormGraph, prescaled: bool = False, bias=None, relu: bool = False):
    """act(dinv * (A+I) (dinv * x) + bias) in the storage dtype of x; ``prescaled``:
    x already carries the column scale.  Bias / ReLU run in the SpMM epilogue."""
    F = x.shape[1]
    xs = pad_cols(x).contiguous()
    out = ops.spmm(g.rowptr, g.col, xs, F, rscale=g.dinv, bias=bias, relu=relu, out_dtype=x.dtype,
                   ld_out=xs.shape[1], cscale=None if prescaled else g.dinv)
    return out[:, :F] if out.shape[1] != F else out


class _NormAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g: NormGraph):
        ctx.g = g
        return aggregate(x, g)

    @staticmethod
    def backward(ctx, gy):
        return aggregate(gy.contiguous(), ctx.g), None


def norm_aggregate(x: torch.Tensor, g: NormGraph) -> torch.Tensor:
    return _NormAggregate.apply(x, g)


class _GCNLayer(torch.autograd.Function):
    """``act(Â (H W) + b)`` with the normalisation, bias and ReLU inside the SpMM
    (column scale in the gather, row scale + bias + ReLU in the epilogue).
    Backward: ReLU mask, ``db = sum dY``, ``dZ = Â dY`` (same SpMM, Â symmetric),
    ``dW = H^T dZ`` as a split-K batched GEMM (``ops.tall_gemm_tn``), ``dH = dZ W^T``."""

    @staticmethod
    def forward(ctx, h, W, b, g: NormGraph, relu: bool):
        Wc = W.to(h.dtype)
        z = h @ Wc
        out_dim = z.shape[1]
        zp = pad_cols(z).contiguous()
        y = ops.spmm(g.rowptr, g.col, zp, out_dim, rscale=g.dinv, cscale=g.dinv, bias=b.float().contiguous(),
                     relu=relu, out_dtype=h.dtype, ld_out=zp.shape[1])
        if y.shape[1] != out_dim:
            y = y[:, :out_dim]
        ctx.g, ctx.relu = g, relu
        ctx.save_for_backward(h, Wc, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        h, Wc, y = ctx.saved_tensors
        g = ctx.g
        dy = dy.contiguous()
        if ctx.relu:
            dy = torch.ops.aten.threshold_backward(dy, y, 0)
        db = dy.float().sum(0)
        out_dim = dy.shape[1]
        dyp = pad_cols(dy).contiguous()
        dz = ops.spmm(g.rowptr, g.col, dyp, out_dim, rscale=g.dinv, cscale=g.dinv, out_dtype=dy.dtype,
                      ld_out=dyp.shape[1])
        if dz.shape[1] != out_dim:
            dz = dz[:, :out_dim]
        dW = ops.tall_gemm_tn(h, dz)
        dh = dz @ Wc.t() if ctx.needs_input_grad[0] else None
        return dh, dW, db, None, None


class WeightedGraph:
    """Directed CSR with one fp32 value per edge (row = destination, column = source) and
    optional row / column scales: ``Â[i, j] = rscale[i] * val[e] * cscale[j]`` for the edge
    e = (i, j).  ``n_src`` (default: the number of rows) is the number of source nodes of a
    rectangular graph."""

    def __init__(self, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, n_src: Optional[int] = None,
                 rscale: Optional[torch.Tensor] = None, cscale: Optional[torch.Tensor] = None):
        self.rowptr, self.col, self.val = rowptr.contiguous(), col.contiguous(), val.contiguous()
        self.n = rowptr.numel() - 1
        self.n_src = self.n if n_src is None else int(n_src)
        self.rscale = rscale.contiguous() if rscale is not None else None
        self.cscale = cscale.contiguous() if cscale is not None else None
        if self.val.numel() != self.col.numel():
            raise ValueError("WeightedGraph: %d values for %d edges" % (self.val.numel(), self.col.numel()))
        self._t = None

    def transposed(self):
        """``(rowptr_t, col_t, eperm)``: the CSR of the transpose and, per transposed edge,
        the index of its forward edge (so the backward reads ``val`` in place).  Built once."""
        if self._t is None:
            from .sage import transpose_csr
            self._t = transpose_csr(self.rowptr, self.col, self.n_src, with_perm=True)
        return self._t

    transposed_perm = transposed

    @classmethod
    def from_edges(cls, n: int, src, dst, weight=None, self_loops: Optional[float] = 1.0,
                   normalize: Optional[str] = "sym", device=None) -> "WeightedGraph":
        """Graph of the directed edges src -> dst (``data.build_weighted_csr``: duplicates
        summed, self loops of weight ``self_loops`` added where missing).  ``normalize``:
        ``"sym"``: val_ij = w_ij / sqrt(d_i d_j); ``"rw"``: val_ij = w_ij / d_i; ``None``:
        the weights as they are -- d_i the sum of the weights of row i after self loops; a
        row with d_i = 0 gets scale 0.  The normalised values are computed in fp64 and
        rounded once to fp32."""
        from .data import _weighted_csr64
        rowptr, col, w = _weighted_csr64(n, src, dst, weight, self_loops)
        if normalize is not None:
            rows = ops._row_ids(rowptr)
            d = torch.zeros(n, dtype=torch.float64).index_add_(0, rows, w)
            pos = d > 0
            if normalize == "sym":
                ok = pos[rows] & pos[col.long()]
                dd = torch.where(ok, d[rows] * d[col.long()], torch.ones_like(w))
                w = torch.where(ok, w / dd.sqrt(), torch.zeros_like(w))
            elif normalize == "rw":
                w = torch.where(pos[rows], w / torch.where(pos, d, torch.ones_like(d))[rows], torch.zeros_like(w))
            else:
                raise ValueError("normalize must be 'sym', 'rw' or None, got %r" % (normalize,))
        device = torch.device(device) if device is not None else torch.device("cpu")
        return cls(rowptr.to(device), col.to(device), w.float().to(device))

    @classmethod
    def from_norm(cls, g: NormGraph) -> "WeightedGraph":
        """The normalised adjacency of a :class:`NormGraph` in factored form: unit values,
        ``rscale = cscale = dinv``."""
        return cls(g.rowptr, g.col, torch.ones(g.col.numel(), dtype=torch.float32, device=g.col.device),
                   rscale=g.dinv, cscale=g.dinv)


def _wspmm_fwd(x, g: WeightedGraph, val, bias=None, relu=False):
    """act(Â x + bias) in the storage dtype of x (columns padded to a multiple of 8)."""
    F = x.shape[1]
    xs = pad_cols(x).contiguous()
    out = ops.wspmm(g.rowptr, g.col, val, xs, F, rscale=g.rscale, cscale=g.cscale, bias=bias, relu=relu,
                    out_dtype=x.dtype, ld_out=xs.shape[1])
    return out[:, :F] if out.shape[1] != F else out


def _wspmm_bwd(dy, g: WeightedGraph, val):
    """Âᵀ dy: the aggregate over the transposed CSR, the forward's values read through the
    edge permutation, the roles of the row and column scale swapped."""
    rp_t, col_t, eperm = g.transposed()
    F = dy.shape[1]
    dyp = pad_cols(dy).contiguous()
    out = ops.wspmm(rp_t, col_t, val, dyp, F, rscale=g.cscale, cscale=g.rscale, eperm=eperm, out_dtype=dy.dtype,
                    ld_out=dyp.shape[1])
    return out[:, :F] if out.shape[1] != F else out


def _edge_grad(dy, x, g: WeightedGraph, val):
    """d loss / d val[e] = rscale[i] cscale[j] <dy[i], x[j]> for e = (i, j)."""
    F = dy.shape[1]
    d = ops.sddmm(g.rowptr, g.col, pad_cols(dy).contiguous(), pad_cols(x).contiguous(), F, rscale=g.rscale,
                  cscale=g.cscale)
    return d.to(val.dtype)


class _WeightedAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, val, g: WeightedGraph):
        ctx.g = g
        ctx.save_for_backward(x, val)
        return _wspmm_fwd(x, g, val.detach())

    @staticmethod
    def backward(ctx, gy):
        x, val = ctx.saved_tensors
        gy = gy.contiguous()
        dx = _wspmm_bwd(gy, ctx.g, val) if ctx.needs_input_grad[0] else None
        dval = _edge_grad(gy, x, ctx.g, val) if ctx.needs_input_grad[1] else None
        return dx, dval, None


def weighted_aggregate(x: torch.Tensor, g: WeightedGraph, val: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``Â x`` over an edge-weighted, possibly directed graph.  ``val`` (default ``g.val``):
    the edge values; a tensor that requires grad receives d loss / d val (fp32), which is how
    edge weights are learned or explained."""
    return _WeightedAggregate.apply(x, g.val if val is None else val, g)


class _PoolAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g, reduce):
        F = x.shape[1]
        xs = pad_cols(x).contiguous()
        y, arg = ops.pool(g.rowptr, g.col, xs, F, reduce=reduce, with_arg=ctx.needs_input_grad[0],
                          ld_out=xs.shape[1])
        ctx.g, ctx.F = g, F
        ctx.save_for_backward(arg)
        return y[:, :F] if y.shape[1] != F else y

    @staticmethod
    def backward(ctx, gy):
        arg, = ctx.saved_tensors
        rp_t, col_t, eperm = ctx.g.transposed_perm()
        F = ctx.F
        dyp = pad_cols(gy).contiguous()
        dx = ops.pool_bwd(rp_t, col_t, eperm, arg, dyp, F, out_dtype=gy.dtype, ld_out=dyp.shape[1])
        return (dx[:, :F] if dx.shape[1] != F else dx), None, None


def pool_aggregate(x: torch.Tensor, g, reduce: str = "max") -> torch.Tensor:
    """Element-wise max / min of ``x`` over each node's neighbours (``ops.pool``); an empty
    neighbourhood gives 0.  ``g``: anything with ``rowptr``, ``col`` (row = destination,
    column = source) and ``transposed_perm()`` -- a :class:`WeightedGraph` (its values and
    scales are ignored), a :class:`NormGraph`, a ``sage.Block``.  The gradient goes to the
    element that supplied each result (the first edge on ties), through the saved edge index
    and a gather over the transposed CSR (``ops.pool_bwd``): deterministic, no atomics."""
    return _PoolAggregate.apply(x, g, reduce)


def _pad_last(x: torch.Tensor, mult: int = 8) -> torch.Tensor:
    F = x.shape[-1]
    return x if F % mult == 0 else torch.nn.functional.pad(x, (0, mult - F % mult))


class _EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score, g, scale):
        p = ops.edge_softmax(g.rowptr, score.contiguous(), scale=scale, nnz=g.col.numel())
        ctx.g, ctx.scale = g, scale
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, dp):
        p, = ctx.saved_tensors
        ds = ops.edge_softmax_bwd(ctx.g.rowptr, p, dp.contiguous(), scale=ctx.scale, nnz=ctx.g.col.numel())
        return ds, None, None


def edge_softmax(score: torch.Tensor, g, scale: float = 1.0) -> torch.Tensor:
    """Softmax of per-edge scores over each destination node's incoming edges
    (``ops.edge_softmax``): ``score`` is ``[nnz]`` or head-major ``[K, nnz]`` in the edge order
    of ``g`` (anything with ``rowptr`` and ``col``), the result has its shape; the scores are
    multiplied by ``scale > 0`` first.  The backward runs ``ops.edge_softmax_bwd`` on the saved
    output.  Deterministic, no atomics; fp32 on the GPU."""
    return _EdgeSoftmax.apply(score, g, float(scale))


def _n_rows(g) -> int:
    return g.rowptr.numel() - 1


class _EdgeDot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, a, b, g):
        F = a.shape[1]
        ap, bp = pad_cols(a).contiguous(), pad_cols(b).contiguous()
        if out is not None:
            ctx.mark_dirty(out)
        out = ops.sddmm(g.rowptr, g.col, ap, bp, F, out=out)
        ctx.g, ctx.F = g, F
        ctx.save_for_backward(ap, bp)
        return out

    @staticmethod
    def backward(ctx, dout):
        ap, bp = ctx.saved_tensors
        g, F = ctx.g, ctx.F
        dout = dout.contiguous()
        da = db = None
        if ctx.needs_input_grad[1]:
            da = ops.wspmm(g.rowptr, g.col, dout, bp, F)[:, :F]
        if ctx.needs_input_grad[2]:
            rp_t, col_t, eperm = g.transposed_perm()
            db = ops.wspmm(rp_t, col_t, dout, ap, F, eperm=eperm)[:, :F]
        # the overwritten buffer comes first (autograd takes input 0 of an in-place function
        # for the tensor it changed); what it held before does not reach the result
        return (torch.zeros_like(dout) if ctx.needs_input_grad[0] else None), da, db, None


def edge_dot(a: torch.Tensor, b: torch.Tensor, g, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[e] = <a[i], b[j]>`` for every edge e = (i, j) of ``g`` (``ops.sddmm``), in fp32
    (fp64 for fp64 inputs): ``a`` holds one row per destination, ``b`` one per source, in one
    storage dtype.  ``out`` (optional, a contiguous ``[nnz]`` tensor, e.g. one head's row of a
    ``[K, nnz]`` score buffer) is written in place and returned.  Differentiable in both
    operands with no kernel of its own: ``da = wspmm(val=dout, X=b)`` over the forward CSR,
    ``db = wspmm(val=dout, X=a, eperm=...)`` over ``g.transposed_perm()``."""
    return _EdgeDot.apply(out, a, b, g)


class _HeadsAggregate(torch.autograd.Function):
    """``Y[k] = A_k V[k]`` for K heads: ``V`` is ``[K, n_src, D]`` (D a multiple of 8), ``alpha``
    the head-major fp32 edge values ``[K, nnz]``, each head's slice read in place by
    ``ops.wspmm``.  Backward: ``dV[k] = A_k^T dY[k]`` over the transposed CSR and
    ``d alpha[k] = sddmm(dY[k], V[k])``, written into one ``[K, nnz]`` buffer."""

    @staticmethod
    def forward(ctx, V, alpha, g):
        K, D = V.shape[0], V.shape[2]
        Y = torch.empty(K, _n_rows(g), D, dtype=V.dtype, device=V.device)
        for k in range(K):
            ops.wspmm(g.rowptr, g.col, alpha[k], V[k], D, out=Y[k])
        ctx.g = g
        ctx.save_for_backward(V, alpha)
        return Y

    @staticmethod
    def backward(ctx, dY):
        V, alpha = ctx.saved_tensors
        g = ctx.g
        K, D = V.shape[0], V.shape[2]
        dY = dY.contiguous()
        dV = dalpha = None
        if ctx.needs_input_grad[0]:
            rp_t, col_t, eperm = g.transposed_perm()
            dV = torch.empty_like(V)
            for k in range(K):
                ops.wspmm(rp_t, col_t, alpha[k], dY[k], D, eperm=eperm, out=dV[k])
        if ctx.needs_input_grad[1]:
            dalpha = torch.empty_like(alpha)
            for k in range(K):
                ops.sddmm(g.rowptr, g.col, dY[k], V[k], D, out=dalpha[k])
        return dV, dalpha, None


class AttentionConv(torch.nn.Module):
    """Multi-head dot-product attention over a graph: PyG's ``TransformerConv`` without edge
    features or gating.  With ``Q = h_dst Wq + bq``, ``K = h_src Wk + bk``, ``V = h_src Wv + bv``
    projected as ``[heads, n, head_dim]`` (each head contiguous),

        alpha^k_ij = softmax_j(<Q^k_i, K^k_j> / sqrt(head_dim))   over the edges (i, j) of g
        out_i      = concat_k (or mean_k) sum_j alpha^k_ij V^k_j  (+ h_dst W_root) (+ bias)

    The scores of all heads fill one fp32 ``[heads, nnz]`` buffer (``edge_dot`` per head) and
    are normalised in one launch (``edge_softmax``); the aggregation and its gradient with
    respect to alpha run on ``ops.wspmm`` / ``ops.sddmm``.  ``g``: anything ``pool_aggregate``
    accepts; on a rectangular graph the destinations are the first rows of ``h``, as in
    ``SAGE``.  Storage dtype follows the input; scores and alpha stay fp32.  Glorot-uniform
    weights, zero biases."""

    def __init__(self, in_dim: int, heads: int, head_dim: int, concat: bool = True, root_weight: bool = True,
                 bias: bool = True, generator: Optional[torch.Generator] = None):
        super().__init__()
        self.in_dim, self.heads, self.head_dim, self.concat = in_dim, heads, head_dim, bool(concat)
        self.out_dim = heads * head_dim if concat else head_dim

        def glorot(fan_out, *shape):
            bound = math.sqrt(6.0 / (in_dim + fan_out))
            return torch.nn.Parameter((torch.rand(*shape, generator=generator) * 2 - 1) * bound)

        hd = heads * head_dim
        self.w_q = glorot(hd, heads, in_dim, head_dim)
        self.w_k = glorot(hd, heads, in_dim, head_dim)
        self.w_v = glorot(hd, heads, in_dim, head_dim)
        self.b_q = torch.nn.Parameter(torch.zeros(heads, 1, head_dim))
        self.b_k = torch.nn.Parameter(torch.zeros(heads, 1, head_dim))
        self.b_v = torch.nn.Parameter(torch.zeros(heads, 1, head_dim))
        self.w_root = glorot(self.out_dim, in_dim, self.out_dim) if root_weight else None
        self.bias = torch.nn.Parameter(torch.zeros(self.out_dim)) if bias else None

    def forward(self, h: torch.Tensor, g, return_attention: bool = False):
        n, dt = _n_rows(g), h.dtype
        n_src = getattr(g, "n_src", None) or n
        if h.shape[0] < n_src:
            raise ValueError("AttentionConv: %d feature rows for %d source nodes" % (h.shape[0], n_src))
        h_src, h_dst = h[:n_src], h[:n]
        q = _pad_last(torch.matmul(h_dst, self.w_q.to(dt)) + self.b_q.to(dt))
        k = _pad_last(torch.matmul(h_src, self.w_k.to(dt)) + self.b_k.to(dt))
        v = _pad_last(torch.matmul(h_src, self.w_v.to(dt)) + self.b_v.to(dt))
        score = torch.empty(self.heads, g.col.numel(), dtype=ops._acc_dtype(dt), device=h.device)
        for i in range(self.heads):                          # in place: score carries the history
            edge_dot(q[i], k[i], g, out=score[i])
        alpha = edge_softmax(score, g, scale=self.head_dim ** -0.5)
        y = _HeadsAggregate.apply(v.contiguous(), alpha, g)[:, :, :self.head_dim]
        out = y.permute(1, 0, 2).reshape(n, self.out_dim) if self.concat else y.mean(0)
        if self.w_root is not None:
            out = out + h_dst @ self.w_root.to(dt)
        if self.bias is not None:
            out = out + self.bias.to(dt)
        return (out, alpha) if return_attention else out


class _EdgeAggregate(torch.autograd.Function):
    """``ops.espmm`` with its three gradients: ``de`` / ``dval`` from one ``ops.egrad`` call
    (only what is asked for), ``dx`` from ``ops.espmm`` over the transposed CSR."""

    @staticmethod
    def forward(ctx, x, e, val, g, op, relu):
        F = e.shape[1]
        ep = pad_cols(e).contiguous()
        xp = pad_cols(x).contiguous() if x is not None else None
        vc = val.detach().to(ops._acc_dtype(e.dtype)).contiguous() if val is not None else None
        y = ops.espmm(g.rowptr, g.col, xp, ep, F, op=op, relu=relu, val=vc)
        ctx.g, ctx.F, ctx.op, ctx.relu = g, F, op, relu
        ctx.val_dtype = val.dtype if val is not None else None
        ctx.save_for_backward(xp, ep, vc)
        return y[:, :F] if y.shape[1] != F else y

    @staticmethod
    def backward(ctx, gy):
        xp, ep, vc = ctx.saved_tensors
        g, F, op, relu = ctx.g, ctx.F, ctx.op, ctx.relu
        need_x, need_e, need_v = ctx.needs_input_grad[:3]
        dyp = pad_cols(gy).contiguous()
        # op="add": dx is the sum of the dE rows, which are then computed (into a scratch
        # buffer) even when e needs no gradient
        want_de = need_e or (need_x and op == "add")
        dE = dval = dx = None
        if want_de or need_v:
            dE, dval = ops.egrad(g.rowptr, g.col, dyp, xp, ep, F, op=op, relu=relu, val=vc, want_dE=want_de,
                                 want_dval=need_v)
        if need_x:
            rp_t, col_t, eperm = g.transposed_perm()
            if op == "mul":
                dx = ops.espmm(rp_t, col_t, dyp, ep, F, op="mul", val=vc, eperm=eperm)
            else:                                    # the ReLU mask and w_e are already in dE
                dx = ops.espmm(rp_t, col_t, None, dE, F, eperm=eperm)
            if dx.shape[0] < xp.shape[0]:            # rows of x beyond the graph's sources
                dx = torch.cat([dx, dx.new_zeros(xp.shape[0] - dx.shape[0], dx.shape[1])])
            dx = dx[:, :F] if dx.shape[1] != F else dx
        de = (dE[:, :F] if dE.shape[1] != F else dE) if need_e else None
        return dx, de, (dval.to(ctx.val_dtype) if need_v else None), None, None, None


def edge_aggregate(x: Optional[torch.Tensor], e: torch.Tensor, g, op: str = "add", relu: bool = False,
                   val: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Message passing with a feature row per edge (``ops.espmm``): ``y_i = sum_j w_ij m_ij``
    over the edges (i, j) of ``g`` with ``m_ij = x_j + e_ij`` (``op="add"``; through a ReLU with
    ``relu=True``) or ``m_ij = x_j * e_ij`` (``op="mul"``).  ``e`` is ``[nnz, F]`` in the edge
    order of ``g``, ``x`` is ``[n_src, F]`` in the same storage dtype; ``x=None`` sums the edge
    rows into their destinations.  ``val`` (optional, ``[nnz]``, fp32): the weights ``w_ij``,
    default 1.  ``g``: anything ``pool_aggregate`` accepts.  Differentiable in ``x``, ``e`` and
    ``val``: ``de`` and ``dval`` come from one ``ops.egrad`` call that computes only what is
    required; ``dx`` is ``ops.espmm`` over ``g.transposed_perm()`` -- for ``"mul"`` of the
    incoming gradient times ``e``, for ``"add"`` the sum of the ``de`` rows (which carry the
    ReLU mask and ``w_ij``).  In bf16 / fp16 those rows are rounded to the storage type
    before they are summed.  Deterministic, no atomics."""
    return _EdgeAggregate.apply(x, e, val, g, op, bool(relu))


class _Dense(torch.nn.Module):
    """``x W (+ b)``: Glorot-uniform ``W`` ``[in_dim, out_dim]``, zero ``b``; the parameters
    are cast to the input's dtype."""

    def __init__(self, in_dim: int, out_dim: int, bias: bool = True, generator: Optional[torch.Generator] = None):
        super().__init__()
        bound = math.sqrt(6.0 / (in_dim + out_dim))
        self.weight = torch.nn.Parameter((torch.rand(in_dim, out_dim, generator=generator) * 2 - 1) * bound)
        self.bias = torch.nn.Parameter(torch.zeros(out_dim)) if bias else None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = x @ self.weight.to(x.dtype)
        return y + self.bias.to(x.dtype) if self.bias is not None else y


def _src_dst(h, g, what):
    n = _n_rows(g)
    n_src = getattr(g, "n_src", None) or n
    if h.shape[0] < max(n_src, n):
        raise ValueError("%s: %d feature rows for %d source and %d destination nodes" % (what, h.shape[0], n_src, n))
    return h[:n_src], h[:n]


class GINEConv(torch.nn.Module):
    """GIN with edge features (PyG's ``GINEConv``):

        out_i = nn((1 + eps) x_i + sum_j relu(x_j + lin(e_ij)))   over the edges (i, j) of g

    ``nn`` is any module mapping ``[n, in_dim]`` rows; ``lin``, a ``Linear(edge_dim, in_dim)``
    (Glorot-uniform weight, zero bias), exists only when ``edge_dim`` is given -- otherwise the
    edge rows must already have the width of ``x``.  ``eps`` is a parameter with
    ``train_eps=True``.  The sum runs on ``edge_aggregate`` (``ops.espmm``, add + ReLU).  ``g``:
    anything ``pool_aggregate`` accepts; on a rectangular graph the destinations are the first
    rows of ``x``, as in ``SAGE``."""

    def __init__(self, nn: torch.nn.Module, eps: float = 0.0, train_eps: bool = False, in_dim: Optional[int] = None,
                 edge_dim: Optional[int] = None, generator: Optional[torch.Generator] = None):
        super().__init__()
        self.nn = nn
        if train_eps:
            self.eps = torch.nn.Parameter(torch.tensor([float(eps)]))
        else:
            self.register_buffer("eps", torch.tensor([float(eps)]))
        if edge_dim is not None:
            if in_dim is None:
                raise ValueError("GINEConv: edge_dim needs in_dim (the width of x)")
            self.lin = _Dense(edge_dim, in_dim, generator=generator)
        else:
            self.lin = None

    def forward(self, x: torch.Tensor, g, e: torch.Tensor) -> torch.Tensor:
        x_src, x_dst = _src_dst(x, g, "GINEConv")
        if self.lin is not None:
            e = self.lin(e)
        if e.shape[1] != x.shape[1]:
            raise ValueError("GINEConv: edge rows of width %d for node rows of width %d (pass edge_dim)"
                             % (e.shape[1], x.shape[1]))
        agg = edge_aggregate(x_src, e, g, "add", relu=True)
        return self.nn((1 + self.eps.to(x.dtype)) * x_dst + agg)


class CFConv(torch.nn.Module):
    """SchNet's continuous-filter convolution:

        h = x W1,   W_ij = Linear(ssp(Linear(e_ij))),   out_i = Linear(sum_j c_ij h_j * W_ij)

    with ``ssp(z) = softplus(z) - log 2``, ``W1`` ``[in_dim, n_filters]`` without bias, the filter
    network ``edge_dim -> n_filters -> n_filters`` and the output layer ``n_filters -> out_dim``.
    ``cutoff`` (optional, ``[nnz]``): the per-edge weights ``c_ij`` (e.g. a cosine cutoff of the
    distance), differentiable.  The sum runs on ``edge_aggregate`` (``ops.espmm``, mul).
    Glorot-uniform weights, zero biases.  ``g``: anything ``pool_aggregate`` accepts."""

    def __init__(self, in_dim: int, out_dim: int, n_filters: int, edge_dim: int,
                 generator: Optional[torch.Generator] = None):
        super().__init__()
        self.lin1 = _Dense(in_dim, n_filters, bias=False, generator=generator)
        self.filter1 = _Dense(edge_dim, n_filters, generator=generator)
        self.filter2 = _Dense(n_filters, n_filters, generator=generator)
        self.lin2 = _Dense(n_filters, out_dim, generator=generator)

    def forward(self, x: torch.Tensor, g, e: torch.Tensor, cutoff: Optional[torch.Tensor] = None) -> torch.Tensor:
        x_src, _ = _src_dst(x, g, "CFConv")
        h = self.lin1(x_src)
        w = self.filter2(torch.nn.functional.softplus(self.filter1(e)) - math.log(2.0))
        return self.lin2(edge_aggregate(h, w, g, "mul", val=cutoff))


class _WeightedGCNLayer(torch.autograd.Function):
    """``act(Â (H W) + b)`` on a :class:`WeightedGraph`: bias and ReLU in the weighted
    SpMM's epilogue.  Backward: ReLU mask, ``db = sum dY``, ``dZ = Âᵀ dY`` (transposed
    pass), ``dW = H^T dZ`` (``ops.tall_gemm_tn``), ``dH = dZ W^T`` and, when asked for,
    ``d val[e] = rscale_i cscale_j <dY_i, (H W)_j>`` (``ops.sddmm``)."""

    @staticmethod
    def forward(ctx, h, W, b, val, g: WeightedGraph, relu: bool):
        Wc = W.to(h.dtype)
        z = h @ Wc
        y = _wspmm_fwd(z, g, val.detach(), bias=b.float().contiguous(), relu=relu)
        ctx.g, ctx.relu = g, relu
        ctx.save_for_backward(h, Wc, val, y if relu else None, z if ctx.needs_input_grad[3] else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        h, Wc, val, y, z = ctx.saved_tensors
        g = ctx.g
        dy = dy.contiguous()
        if ctx.relu:
            dy = torch.ops.aten.threshold_backward(dy, y, 0)
        db = dy.float().sum(0)
        dz = _wspmm_bwd(dy, g, val)
        dW = ops.tall_gemm_tn(h, dz)
        dh = dz @ Wc.t() if ctx.needs_input_grad[0] else None
        dval = _edge_grad(dy, z, g, val) if ctx.needs_input_grad[3] else None
        return dh, dW, db, dval, None, None


def gcn_layer(h: torch.Tensor, W: torch.Tensor, b: torch.Tensor, g, relu: bool,
              edge_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``act(Â (H W) + b)``; ``g`` a :class:`NormGraph`, or a :class:`WeightedGraph` with
    optional ``edge_weight`` (default ``g.val``) in place of its values."""
    if isinstance(g, WeightedGraph):
        return _WeightedGCNLayer.apply(h, W, b, g.val if edge_weight is None else edge_weight, g, relu)
    if edge_weight is not None:
        raise TypeError("edge_weight needs a WeightedGraph (WeightedGraph.from_norm(g))")
    return _GCNLayer.apply(h, W, b, g, relu)


class GCNConv(torch.nn.Module):
    """``Â (H W) + b``; glorot-uniform W, zero b (the PyG GCNConv initialisation)."""

    def __init__(self, in_dim: int, out_dim: int, generator: Optional[torch.Generator] = None):
        super().__init__()
        bound = math.sqrt(6.0 / (in_dim + out_dim))
        self.weight = torch.nn.Parameter((torch.rand(in_dim, out_dim, generator=generator) * 2 - 1) * bound)
        self.bias = torch.nn.Parameter(torch.zeros(out_dim))

    def forward(self, h: torch.Tensor, g, relu: bool = False, edge_weight: Optional[torch.Tensor] = None):
        return gcn_layer(h, self.weight, self.bias, g, relu, edge_weight)


class GCN(torch.nn.Module):
    """L-layer GCN: ``dims = [in, hidden..., out]``; ReLU + dropout between layers."""

    def __init__(self, dims: Sequence[int], dropout: float = 0.5, seed: int = 0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.dims = list(dims)
        self.convs = torch.nn.ModuleList(GCNConv(a, b, gen) for a, b in zip(dims[:-1], dims[1:]))
        self.dropout = float(dropout)

    def forward(self, x: torch.Tensor, g, edge_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        h = x
        L = len(self.convs)
        for k, conv in enumerate(self.convs):
            h = conv(h, g, relu=k < L - 1, edge_weight=edge_weight)
            if k < L - 1 and self.training and self.dropout > 0:
                h = torch.nn.functional.dropout(h, self.dropout)
        return h
