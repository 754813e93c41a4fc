"""Graph-level readout for batches of small graphs -- GNN track, not in the reference.

* ``GraphBatch`` -- a list of graphs packed into one block-diagonal CSR (row = destination),
  with the edge permutation the per-edge layers need, the node -> graph map and the segment
  tables of the reduction.  Every layer that takes "anything ``pool_aggregate`` accepts"
  takes it.
* ``graph_readout`` -- one row per graph from the node rows: sum, mean, max or min
  (``ops.seg_reduce``); the backward is ``ops.seg_bcast``.
* ``graph_broadcast`` -- one graph row to each of the graph's nodes (``ops.seg_bcast``):
  global conditioning ``x + graph_broadcast(u, batch)``, virtual nodes, GraphNorm; the backward
  is the sum readout.
* ``GlobalAttention`` -- PyG's ``AttentionalAggregation``: a softmax of one gate score per node
  over each graph (``ops.edge_softmax`` on the graph pointer), then the weighted sum.

The two-level schedule.  One sub-group of the kernel owns one output row, so a few long
graphs would leave the device idle.  A graph longer than ``R = ops.READOUT_CHUNK`` rows is
therefore split into chunks of R rows counted from the graph's own start; pass 1 reduces the
chunks to partial rows (fp32 for the sums), pass 2 the partial rows of each graph, both with
the one kernel.  When no graph is longer than R a single launch writes the result.  Either
way a graph's result is a function of its own rows only: moving it inside the batch or
changing its neighbours does not change a bit.  No atomics anywhere.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional, Sequence

import torch

from . import ops
from .layers import edge_softmax, pad_cols

_REDUCE = ("sum", "mean", "max", "min")


def _i32(t, what):
    if t.numel() and int(t.max()) >= 2 ** 31:
        raise ValueError("GraphBatch: %s does not fit int32" % what)
    return t.to(torch.int32).contiguous()


class GraphBatch:
    """Graphs packed side by side: node ids of graph ``g`` are ``gptr[g] .. gptr[g+1] - 1``.

    ``rowptr`` / ``col`` (int32): the block-diagonal CSR, row = destination, column = source,
    multi-edges kept, no self loops added; ``n = n_src`` nodes.  ``eperm`` (int64): the index
    in the concatenated input edge list of each CSR edge -- the sort is stable by (dst, input
    order) -- so edge rows go into CSR order as ``e_in[eperm]``.  ``gptr`` (int32 ``[G + 1]``),
    ``batch`` (int32 ``[n]``, node -> graph), ``n_graphs``; ``count`` (int32 ``[G]``), ``max_count`` and
    ``inv_count`` (fp32: ``1 / count`` computed in fp64 and rounded once, 0 for an empty
    graph).  The chunk tables of the two-level reduction, for ``chunk = ops.READOUT_CHUNK``
    rows at construction: ``cptr`` (int32 ``[C + 1]``, the row boundaries of the chunks),
    ``gchunk`` (int32 ``[G + 1]``, the chunks of each graph), ``n_chunks`` and ``single_pass``
    (no graph is longer than a chunk).  Graph lengths 70, 0, 10 with chunks of 64 rows give
    ``cptr = [0, 64, 70, 80]`` and ``gchunk = [0, 2, 2, 3]``.

    A periodic ``geometry.radius_graph`` also sets ``shift`` (int32 ``[nnz]``, the lattice image
    of each edge's source: byte a = ``s[a]`` as an int8, 0 = the home image) and ``cell`` (fp32
    ``[G, 9]``, row-major 3 x 3 per graph); both are ``None`` otherwise."""

    shift = None
    cell = None

    def __init__(self, gptr: torch.Tensor, rowptr: Optional[torch.Tensor] = None, col: Optional[torch.Tensor] = None,
                 eperm: Optional[torch.Tensor] = None, chunk: Optional[int] = None):
        gp = gptr.detach().to("cpu", torch.int64)
        if gp.dim() != 1 or gp.numel() < 1 or int(gp[0]) != 0 or bool((gp[1:] < gp[:-1]).any()):
            raise ValueError("GraphBatch: gptr must start at 0 and never decrease")
        R = int(ops.READOUT_CHUNK if chunk is None else chunk)
        if R < 1:
            raise ValueError("GraphBatch: chunk must be positive, got %d" % R)
        G, n = gp.numel() - 1, int(gp[-1])
        cnt = gp[1:] - gp[:-1]
        nch = (cnt + R - 1) // R
        gchunk = torch.zeros(G + 1, dtype=torch.int64)
        gchunk[1:] = torch.cumsum(nch, 0)
        C = int(gchunk[-1])
        owner = torch.repeat_interleave(torch.arange(G), nch)
        start = gp[:-1][owner] + (torch.arange(C) - gchunk[:-1][owner]) * R
        self.chunk, self.n, self.n_src, self.n_graphs, self.n_chunks = R, n, n, G, C
        self.max_count = int(cnt.max()) if G else 0
        self.single_pass = bool(C == 0 or self.max_count <= R)
        self.gptr = _i32(gp, "the node count")
        self.batch = torch.repeat_interleave(torch.arange(G, dtype=torch.int32), cnt)
        self.count = cnt.to(torch.int32)
        inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1).double(), torch.zeros(G, dtype=torch.float64))
        self.inv_count = inv.float()
        self.cptr = torch.cat([start, torch.tensor([n])]).to(torch.int32)
        self.gchunk = gchunk.to(torch.int32)
        dev = gptr.device
        self.rowptr = rowptr.contiguous() if rowptr is not None else torch.zeros(n + 1, dtype=torch.int32, device=dev)
        self.col = col.contiguous() if col is not None else torch.zeros(0, dtype=torch.int32, device=dev)
        self.eperm = eperm.contiguous() if eperm is not None else torch.zeros(0, dtype=torch.int64, device=dev)
        if self.rowptr.numel() != n + 1:
            raise ValueError("GraphBatch: rowptr describes %d rows for %d nodes" % (self.rowptr.numel() - 1, n))
        self._tperm = None
        self._segments = None
        self._move(dev)

    _TENSORS = ("rowptr", "col", "eperm", "gptr", "batch", "count", "inv_count", "cptr", "gchunk")

    def _move(self, device):
        for name in self._TENSORS:
            setattr(self, name, getattr(self, name).to(device))
        for name in ("shift", "cell"):
            if getattr(self, name) is not None:
                setattr(self, name, getattr(self, name).to(device))
        return self

    @classmethod
    def from_graphs(cls, graphs: Sequence, device=None) -> "GraphBatch":
        """The batch of ``graphs``, a sequence of ``(n_nodes, src, dst)`` with the directed
        edges ``src[k] -> dst[k]`` in the graph's own node ids."""
        sizes, srcs, dsts = [], [], []
        for k, (n_nodes, src, dst) in enumerate(graphs):
            s = torch.as_tensor(src, dtype=torch.int64).reshape(-1)
            d = torch.as_tensor(dst, dtype=torch.int64).reshape(-1)
            if int(n_nodes) < 0 or s.numel() != d.numel():
                raise ValueError("GraphBatch: graph %d: %d nodes, %d sources, %d destinations"
                                 % (k, int(n_nodes), s.numel(), d.numel()))
            if s.numel() and (min(int(s.min()), int(d.min())) < 0 or max(int(s.max()), int(d.max())) >= int(n_nodes)):
                raise ValueError("GraphBatch: graph %d: node id outside [0, %d)" % (k, int(n_nodes)))
            off = sum(sizes)
            sizes.append(int(n_nodes))
            srcs.append(s + off)
            dsts.append(d + off)
        gptr = torch.zeros(len(sizes) + 1, dtype=torch.int64)
        gptr[1:] = torch.cumsum(torch.tensor(sizes, dtype=torch.int64), 0)
        n = int(gptr[-1])
        src = torch.cat(srcs) if srcs else torch.zeros(0, dtype=torch.int64)
        dst = torch.cat(dsts) if dsts else torch.zeros(0, dtype=torch.int64)
        eperm = torch.sort(dst, stable=True).indices
        rowptr = torch.zeros(n + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
        b = cls(gptr, _i32(rowptr, "the edge count"), src[eperm].to(torch.int32), eperm)
        return b if device is None else b._move(torch.device(device))

    @classmethod
    def from_ptr(cls, gptr: torch.Tensor) -> "GraphBatch":
        """A batch without edges, for readout only, on ``gptr``'s device."""
        return cls(gptr)

    def to(self, device) -> "GraphBatch":
        """A copy on ``device`` (the same chunk size)."""
        b = GraphBatch(self.gptr, self.rowptr, self.col, self.eperm, chunk=self.chunk)
        b.shift, b.cell = self.shift, self.cell
        return b._move(torch.device(device))

    def shifts(self):
        """The lattice image of each edge's source, int32 ``[nnz, 3]``, unpacked from ``shift``:
        edge e of row i joins ``pos[i]`` and ``pos[col[e]] + shifts()[e] @ cell[g]``.  Only for a
        periodic ``geometry.radius_graph``."""
        if self.shift is None:
            raise ValueError("GraphBatch.shifts: not a periodic graph (no cell was given)")
        return ops.unpack_shift(self.shift, 3)

    def transposed_perm(self):
        """``(rowptr_t, col_t, eperm)`` of the transposed CSR, as ``WeightedGraph.transposed``
        (that ``eperm`` maps transposed edges to CSR edges; it is not ``self.eperm``).  Built
        once."""
        if self._tperm is None:
            from .sage import transpose_csr
            self._tperm = transpose_csr(self.rowptr, self.col, self.n, with_perm=True)
        return self._tperm

    def segments(self):
        """The graphs as the rows of a CSR whose "edges" are the nodes: what
        ``layers.edge_softmax`` needs for a softmax over each graph's nodes."""
        if self._segments is None:
            self._segments = SimpleNamespace(rowptr=self.gptr, col=self.batch)
        return self._segments


def _check_rows(t, n, what, name):
    if t.dim() != 2 or t.shape[0] != n:
        raise ValueError("%s: %s must be [%d, F], got %s" % (what, name, n, tuple(t.shape)))


def _reduce(xp, F, b: GraphBatch, op, rscale=None, with_arg=False):
    """(Y [G, ld], arg or None) of the padded, contiguous node rows ``xp``, ``op`` one of
    ``ops.seg_reduce``'s: one launch, or chunks -> partial rows -> graphs."""
    if op == "sum":
        if b.single_pass:
            return ops.seg_reduce(b.gptr, xp, F, "sum", rscale=rscale)
        part, _ = ops.seg_reduce(b.cptr, xp, F, "sum", out_dtype=ops._acc_dtype(xp.dtype))
        return ops.seg_reduce(b.gchunk, part, F, "sum", rscale=rscale, out_dtype=xp.dtype)
    if b.single_pass:
        return ops.seg_reduce(b.gptr, xp, F, op, with_arg=with_arg)
    part, parg = ops.seg_reduce(b.cptr, xp, F, op, with_arg=with_arg)
    return ops.seg_reduce(b.gchunk, part, F, op, arg_in=parg, with_arg=with_arg)


def _cut(t, F):
    return t[:, :F] if t.shape[1] != F else t


class _GraphReadout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, b, reduce):
        F = x.shape[1]
        xp = pad_cols(x).contiguous()
        if reduce in ("sum", "mean"):
            y, arg = _reduce(xp, F, b, "sum", rscale=b.inv_count if reduce == "mean" else None)
        else:
            y, arg = _reduce(xp, F, b, reduce, with_arg=ctx.needs_input_grad[0])
        ctx.b, ctx.F, ctx.reduce = b, F, reduce
        ctx.save_for_backward(arg)
        return _cut(y, F)

    @staticmethod
    def backward(ctx, gy):
        arg, = ctx.saved_tensors
        b, F = ctx.b, ctx.F
        gp = pad_cols(gy).contiguous()
        dx = ops.seg_bcast(b.batch, gp, F, rscale=b.inv_count if ctx.reduce == "mean" else None, arg=arg)
        return _cut(dx, F), None, None


def graph_readout(x: torch.Tensor, batch: GraphBatch, reduce: str = "sum") -> torch.Tensor:
    """One row per graph from the node rows ``x`` ``[n, F]``: ``[n_graphs, F]`` in x's dtype.
    ``"sum"`` / ``"mean"`` accumulate in fp32 (``mean`` multiplies the sum by ``batch.inv_count``,
    one product and one rounding); ``"max"`` / ``"min"`` follow the scan rule of ``ops.pool``
    (ties to the first node, a NaN propagates).  An empty graph gives 0.  Differentiable: the
    gradient of a sum or mean is the graph's row broadcast to its nodes, that of a max or min
    goes to the node that supplied each value through the saved index, which is computed only
    when ``x`` requires a gradient.  Deterministic, no atomics; a graph's result does not
    depend on its place in the batch."""
    if reduce not in _REDUCE:
        raise ValueError("graph_readout: reduce must be one of %s, got %r" % (_REDUCE, reduce))
    _check_rows(x, batch.n, "graph_readout", "x")
    return _GraphReadout.apply(x, batch, reduce)


class _GraphBroadcast(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, b, scale):
        F = u.shape[1]
        ctx.b, ctx.F, ctx.scale = b, F, scale
        return _cut(ops.seg_bcast(b.batch, pad_cols(u).contiguous(), F, rscale=scale), F)

    @staticmethod
    def backward(ctx, gy):
        b, F, scale = ctx.b, ctx.F, ctx.scale
        du, _ = _reduce(pad_cols(gy).contiguous(), F, b, "sum", rscale=scale)
        return _cut(du, F), None, None


def graph_broadcast(u: torch.Tensor, batch: GraphBatch, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The row of its graph for every node: ``out[i] = scale[g] * u[g]`` with ``g = batch.batch[i]``,
    ``[n, F]`` in u's dtype.  ``scale`` (optional, fp32 ``[n_graphs]``, a constant) is applied
    in fp32 with one rounding.  The backward is the scaled sum readout of the incoming
    gradient, through the kernels of ``graph_readout``."""
    _check_rows(u, batch.n_graphs, "graph_broadcast", "u")
    if scale is not None:
        if scale.requires_grad:
            raise ValueError("graph_broadcast: scale is a constant; multiply u for a learned scale")
        if scale.shape != (batch.n_graphs,):
            raise ValueError("graph_broadcast: scale must be [%d], got %s" % (batch.n_graphs, tuple(scale.shape)))
        scale = scale.contiguous()
    return _GraphBroadcast.apply(u, batch, scale)


class GlobalAttention(torch.nn.Module):
    """Attention readout (PyG's ``AttentionalAggregation``):

        alpha_i = softmax over the nodes i of a graph of gate_nn(x)_i,   out_g = sum_i alpha_i nn(x)_i

    ``gate_nn`` maps ``[n, F]`` to one gate column ``[n, 1]``; ``nn`` (optional) maps the node
    rows before they are summed.  The softmax runs on ``ops.edge_softmax`` over the graph
    pointer (fp32; fp64 for fp64 inputs on the CPU), the sum on ``graph_readout``."""

    def __init__(self, gate_nn: torch.nn.Module, nn: Optional[torch.nn.Module] = None):
        super().__init__()
        self.gate_nn, self.nn = gate_nn, nn

    def forward(self, x: torch.Tensor, batch: GraphBatch, return_attention: bool = False):
        gate = self.gate_nn(x)
        if gate.dim() != 2 or gate.shape != (batch.n, 1):
            raise ValueError("GlobalAttention: gate_nn must give one column [%d, 1], got %s"
                             % (batch.n, tuple(gate.shape)))
        h = self.nn(x) if self.nn is not None else x
        alpha = edge_softmax(gate.to(ops._acc_dtype(gate.dtype)).t(), batch.segments())[0]
        out = graph_readout(alpha[:, None].to(h.dtype) * h, batch, "sum")
        return (out, alpha) if return_attention else out
