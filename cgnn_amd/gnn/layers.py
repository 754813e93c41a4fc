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
