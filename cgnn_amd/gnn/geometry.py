"""Graphs from positions -- GNN track, not in the reference.

A molecular model starts from atomic numbers and positions: its edges are "all pairs closer
than a cutoff", its edge features are functions of the pair distances, and its most wanted
output is the force ``-dE/dpos``.  This module is the path from ``pos`` to the ``e`` / ``cutoff``
arguments of ``layers.CFConv``:

* ``radius_graph`` -- the neighbour search on the device (``ops.radius_count`` /
  ``ops.radius_fill``), returning a ``GraphBatch`` every layer accepts.
* ``pair_distance`` -- the distance of each edge of a graph, differentiable with respect to
  the positions (``ops.pair_d2`` / ``ops.pair_d2_bwd``): exact, deterministic, no atomics.
* ``GaussianSmearing`` / ``cosine_cutoff`` -- SchNet's radial basis and cutoff envelope, plain
  PyTorch: elementwise on ``[nnz, K]``.

Limits.  The search is brute force inside each graph, O(n_g^2): right for molecules and other
graphs of up to a few thousand points.  There are no cell lists for one large point cloud, no
periodic boundaries, no ``max_num_neighbors`` cap and no k-NN.  ``pair_distance`` is
differentiable once: a double backward (training on forces) is not implemented.
"""
from __future__ import annotations

import copy
import math
from typing import Optional, Union

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .readout import GraphBatch


def _auto_lanes(max_count: int) -> int:
    """The sub-group width for graphs of at most ``max_count`` points: the longest graph takes
    at most two steps of its sub-group (docs/PERF.md, "Radius graph")."""
    for L in (8, 16, 32):
        if max_count <= 2 * L:
            return L
    return 64


def _positions(pos, what):
    if pos.dim() != 2 or not 1 <= pos.shape[1] <= 3:
        raise ValueError("%s: pos must be [n, D] with D = 1, 2 or 3, got shape %s" % (what, tuple(pos.shape)))
    if not pos.is_floating_point() or (pos.is_cuda and pos.dtype != torch.float32):
        raise TypeError("%s: pos must be fp32 (fp64 too on the CPU), got %s" % (what, pos.dtype))


def radius_graph(pos: torch.Tensor, r: float, batch: Union[GraphBatch, torch.Tensor, None] = None,
                 loop: bool = False, lanes: Optional[int] = None) -> GraphBatch:
    """The graph of all pairs of points of the same graph at most ``r`` apart.

    ``pos`` is ``[n, D]``, ``D`` in 1..3.  ``batch``: a ``GraphBatch`` (its ``gptr`` / ``batch``
    name the graphs; its edges are ignored), a ``gptr`` tensor ``[G + 1]``, or ``None`` for one
    graph.  Returns a new ``GraphBatch`` on ``pos``'s device over the same graphs: row i of
    ``rowptr`` / ``col`` holds the sources j with ``|p_i - p_j|^2 <= r * r`` (inclusive; fp32, see
    ``ops.radius_count``) in ascending id, ``j != i`` unless ``loop``; ``eperm`` is the identity;
    ``.d2`` keeps the fill pass's squared distances (fp32 ``[nnz]``, not differentiable -- use
    ``pair_distance`` for a gradient).  Everything that takes "anything ``pool_aggregate``
    accepts" takes the result.  The edges are symmetric unless a coordinate is inf or NaN.

    Cost: two kernel launches and a device ``cumsum``, and **one host synchronisation** to read
    ``nnz`` (a ``gptr`` tensor on the device is read back once more to build its batch; pass a
    ``GraphBatch`` to avoid that).  Deterministic: no atomics, the same CSR for every ``lanes``
    (the sub-group width, default from the longest graph), grid and run.

    Brute force inside each graph, O(n_g^2): for molecules and graphs of up to a few thousand
    points.  No cell lists, no periodic boundaries, no ``max_num_neighbors`` cap, no k-NN."""
    _positions(pos, "radius_graph")
    p = pos.detach().contiguous()
    n, D = p.shape
    if batch is None:
        base = GraphBatch(torch.tensor([0, n], dtype=torch.int64))
    elif isinstance(batch, GraphBatch):
        base = batch
    elif isinstance(batch, torch.Tensor):
        if batch.is_floating_point():
            raise TypeError("radius_graph: gptr must be an integer tensor, got %s" % batch.dtype)
        base = GraphBatch(batch)
    else:
        raise TypeError("radius_graph: batch must be a GraphBatch, a gptr tensor or None, got %s" % type(batch))
    if base.n != n:
        raise ValueError("radius_graph: the batch describes %d nodes, pos has %d rows" % (base.n, n))
    out = copy.copy(base)
    out._move(p.device)
    L = _auto_lanes(out.max_count) if lanes is None else lanes
    deg = ops.radius_count(p, D, r, out.gptr, out.batch, loop=loop, lanes=L)
    rp = torch.zeros(n + 1, dtype=torch.int64, device=p.device)
    rp[1:] = torch.cumsum(deg, 0, dtype=torch.int64)
    nnz = int(rp[-1])                                         # the one host sync
    if nnz >= 2 ** 31:
        raise ValueError("radius_graph: %d edges do not fit int32" % nnz)
    out.rowptr = rp.to(torch.int32)
    out.col, out.d2 = ops.radius_fill(p, D, r, out.gptr, out.batch, out.rowptr, loop=loop, lanes=L, nnz=nnz,
                                      with_d2=True)
    out.eperm = torch.arange(nnz, dtype=torch.int64, device=p.device)
    out._tperm = None
    return out


class _PairDistance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, g, squared):
        p = pos.detach().contiguous()
        d2 = ops.pair_d2(g.rowptr, g.col, p, p.shape[1])
        out = d2 if squared else torch.sqrt(d2)
        ctx.g, ctx.squared = g, squared
        ctx.save_for_backward(p, out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gd):
        p, out = ctx.saved_tensors
        g = ctx.g
        if ctx.squared:
            w = gd
        else:                                                # d sqrt(d2) = 1 / (2 d), 0 at d = 0
            w = torch.where(out == 0, torch.zeros_like(gd), gd / (2 * out))
        rp_t, col_t, eperm_t = g.transposed_perm()
        dpos = ops.pair_d2_bwd(g.rowptr, g.col, rp_t, col_t, eperm_t, p, w.to(out.dtype).contiguous(), p.shape[1])
        return dpos, None, None


def pair_distance(pos: torch.Tensor, g, squared: bool = False) -> torch.Tensor:
    """The distance ``|p_i - p_j|`` (``squared``: its square) of every edge (i, j) of ``g``, in
    ``g``'s edge order, ``[nnz]`` in fp32 (fp64 for fp64 positions on the CPU).  ``g``: a square
    graph with ``rowptr`` / ``col`` / ``transposed_perm()`` -- a ``radius_graph``, or a bond graph
    from ``GraphBatch.from_graphs``.  Differentiable with respect to ``pos`` ``[n, D]``: the
    forward is ``ops.pair_d2`` (and one square root), the backward ``ops.pair_d2_bwd`` over the
    graph and its transpose, built once per graph -- fp32, deterministic, no atomics.  The
    gradient of the distance is defined as 0 where the distance is 0 (coincident points, self
    loops).  Differentiable **once**: a double backward, as training on forces needs, is not
    implemented and raises."""
    _positions(pos, "pair_distance")
    n = g.rowptr.numel() - 1
    if pos.shape[0] != n or getattr(g, "n_src", n) != n:
        raise ValueError("pair_distance: a square graph over the %d positions expected, got %d rows"
                         % (pos.shape[0], n))
    return _PairDistance.apply(pos, g, bool(squared))


class GaussianSmearing(torch.nn.Module):
    """SchNet's radial basis: ``out[e, k] = exp(-(d[e] - mu_k)^2 / (2 delta^2))`` with
    ``n_gaussians >= 2`` centres ``mu_k`` evenly spaced over ``[start, stop]`` and ``delta`` their
    spacing.  ``d`` is ``[nnz]``, the result ``[nnz, n_gaussians]`` in d's dtype.  Plain PyTorch,
    differentiable."""

    def __init__(self, start: float = 0.0, stop: float = 5.0, n_gaussians: int = 50):
        super().__init__()
        if n_gaussians < 2 or not stop > start:
            raise ValueError("GaussianSmearing: n_gaussians >= 2 and stop > start expected, got %d, [%r, %r]"
                             % (n_gaussians, start, stop))
        offset = torch.linspace(float(start), float(stop), int(n_gaussians))
        self.coeff = -0.5 / ((float(stop) - float(start)) / (int(n_gaussians) - 1)) ** 2
        self.register_buffer("offset", offset)

    def forward(self, d: torch.Tensor) -> torch.Tensor:
        diff = d[:, None] - self.offset.to(d.dtype)[None, :]
        return torch.exp(self.coeff * diff * diff)


def cosine_cutoff(d: torch.Tensor, r_cut: float) -> torch.Tensor:
    """Behler's cosine envelope: ``0.5 (cos(pi d / r_cut) + 1)`` for ``d < r_cut``, else 0.
    Plain PyTorch, differentiable."""
    c = 0.5 * (torch.cos(d * (math.pi / float(r_cut))) + 1.0)
    return torch.where(d < r_cut, c, torch.zeros_like(c))
