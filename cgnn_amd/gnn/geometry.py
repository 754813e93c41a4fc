"""Graphs from positions -- GNN track, not in the reference.

A molecular model starts from atomic numbers and positions: its edges are "all pairs closer
than a cutoff", its edge features are functions of the pair distances, and its most wanted
output is the force ``-dE/dpos``.  This module is the path from ``pos`` to the ``e`` / ``cutoff``
arguments of ``layers.CFConv``:

* ``radius_graph`` -- the neighbour search on the device (``ops.radius_count`` /
  ``ops.radius_fill``), returning a ``GraphBatch`` every layer accepts; ``max_num_neighbors``
  caps every row at its nearest neighbours.
* ``knn_graph`` -- the k nearest neighbours of every point (``ops.knn_select`` /
  ``ops.knn_fill``), optionally within a radius: the fixed fan-in entry of point-cloud models.
* ``pair_distance`` -- the distance of each edge of a graph, differentiable with respect to
  the positions (``ops.pair_d2`` / ``ops.pair_d2_bwd``): exact, deterministic, no atomics.
* ``GaussianSmearing`` / ``cosine_cutoff`` -- SchNet's radial basis and cutoff envelope, plain
  PyTorch: elementwise on ``[nnz, K]``.

Limits.  The search is brute force inside each graph, O(n_g^2): right for molecules and other
graphs of up to a few thousand points.  There are no cell lists for one large point cloud, no
periodic boundaries and no k-NN in feature space (``D > 3``).  ``pair_distance`` is
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


_KNN_WAVES = 4096       # waves that keep the select pass busy: four per SIMD of an MI355X


def _knn_lanes(k: int, max_count: int, n: int):
    """The sub-group widths of the two k-NN passes for ``n`` rows.  Select: the smallest width
    that holds ``k`` keys -- a wave inserts into all its sub-groups at once, so narrow
    sub-groups mean more insertions in flight -- widened while the launch would have fewer than
    ``_KNN_WAVES`` waves (one large point cloud: few rows, long candidate lists).  The fill is
    the radius loop and takes the radius search's width.  Evidence: docs/PERF.md, "k-NN"."""
    L = ops._knn_min_lanes(k)
    while L < 64 and n * L < _KNN_WAVES * 64:
        L *= 2
    return L, _auto_lanes(max_count)


def _positions(pos, what):
    if pos.dim() != 2 or not 1 <= pos.shape[1] <= 3:
        raise ValueError("%s: pos must be [n, D] with D = 1, 2 or 3, got shape %s" % (what, tuple(pos.shape)))
    if not pos.is_floating_point() or (pos.is_cuda and pos.dtype != torch.float32):
        raise TypeError("%s: pos must be fp32 (fp64 too on the CPU), got %s" % (what, pos.dtype))


def _graphs_of(what, p, batch):
    """A shallow copy of the batch that names the graphs of the points ``p``, on ``p``'s device."""
    n = p.shape[0]
    if batch is None:
        base = GraphBatch(torch.tensor([0, n], dtype=torch.int64))
    elif isinstance(batch, GraphBatch):
        base = batch
    elif isinstance(batch, torch.Tensor):
        if batch.is_floating_point():
            raise TypeError("%s: gptr must be an integer tensor, got %s" % (what, batch.dtype))
        base = GraphBatch(batch)
    else:
        raise TypeError("%s: batch must be a GraphBatch, a gptr tensor or None, got %s" % (what, type(batch)))
    if base.n != n:
        raise ValueError("%s: the batch describes %d nodes, pos has %d rows" % (what, base.n, n))
    out = copy.copy(base)
    out._move(p.device)
    return out


def radius_graph(pos: torch.Tensor, r: float, batch: Union[GraphBatch, torch.Tensor, None] = None,
                 loop: bool = False, lanes: Optional[int] = None,
                 max_num_neighbors: Optional[int] = None) -> GraphBatch:
    """The graph of all pairs of points of the same graph at most ``r`` apart.

    ``pos`` is ``[n, D]``, ``D`` in 1..3.  ``batch``: a ``GraphBatch`` (its ``gptr`` / ``batch``
    name the graphs; its edges are ignored), a ``gptr`` tensor ``[G + 1]``, or ``None`` for one
    graph.  Returns a new ``GraphBatch`` on ``pos``'s device over the same graphs: row i of
    ``rowptr`` / ``col`` holds the sources j with ``|p_i - p_j|^2 <= r * r`` (inclusive; fp32, see
    ``ops.radius_count``) in ascending id, ``j != i`` unless ``loop``; ``eperm`` is the identity;
    ``.d2`` keeps the fill pass's squared distances (fp32 ``[nnz]``, not differentiable -- use
    ``pair_distance`` for a gradient).  Everything that takes "anything ``pool_aggregate``
    accepts" takes the result.  The edges are symmetric unless a coordinate is inf or NaN.

    ``max_num_neighbors``: ``None`` for no cap, or an integer ``k`` in 1..64 for
    ``knn_graph(pos, k, batch, loop, r=r, lanes=lanes)``: every row keeps its ``k`` **nearest**
    neighbours within ``r`` (ties to the lower id) -- not an arbitrary ``k`` of them, as the cap
    of PyTorch Geometric's ``radius_graph`` does.  A capped graph is in general directed; a row
    of at most ``k`` neighbours is the uncapped row bit for bit.

    Cost: two kernel launches and a device ``cumsum``, and **one host synchronisation** to read
    ``nnz`` (a ``gptr`` tensor on the device is read back once more to build its batch; pass a
    ``GraphBatch`` to avoid that).  Deterministic: no atomics, the same CSR for every ``lanes``
    (the sub-group width, default from the longest graph), grid and run.

    Brute force inside each graph, O(n_g^2): for molecules and graphs of up to a few thousand
    points.  No cell lists, no periodic boundaries."""
    if max_num_neighbors is not None:
        return knn_graph(pos, max_num_neighbors, batch, loop, r=r, lanes=lanes)
    _positions(pos, "radius_graph")
    p = pos.detach().contiguous()
    n, D = p.shape
    out = _graphs_of("radius_graph", p, batch)
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


def knn_graph(pos: torch.Tensor, k: int, batch: Union[GraphBatch, torch.Tensor, None] = None, loop: bool = False,
              r: Optional[float] = None, lanes: Optional[int] = None) -> GraphBatch:
    """The graph of the ``k`` nearest neighbours of every point inside its own graph.

    ``pos`` and ``batch`` as in ``radius_graph``; ``k`` in 1..64.  Row i of the returned
    ``GraphBatch`` holds the ``min(k, #candidates)`` nearest candidates j of node i -- the points
    of its graph with ``j != i`` unless ``loop``, a finite distance (a point with a NaN or inf
    coordinate has no neighbours and is nobody's) and, with ``r``, ``|p_i - p_j|^2 <= r * r`` --
    by the key ``(d2, j)``: equal distances go to the lower id (``ops.knn_select``).  The
    neighbours are stored **in ascending source id**, not in distance order, with ``.d2`` their
    squared distances; ``eperm`` is the identity.  The graph is in general **directed** (j among
    the nearest of i does not make i one of j's); ``pair_distance`` and every layer take it as
    it is.  A graph of fewer than ``k + 1`` points gives rows of ``n_g - 1`` neighbours.

    Cost and determinism as ``radius_graph``: two launches, a device ``cumsum``, one host
    synchronisation for ``nnz``; the same CSR for every ``lanes`` (at least ``k``; default: for
    the select pass the smallest such width that still fills the device, for the fill
    ``radius_graph``'s), grid and run, and a graph's rows do not depend on its place in the batch.  Brute force inside each graph:
    O(n_g^2) distances, plus about ``k ln(n_g / k)`` insertions per row."""
    _positions(pos, "knn_graph")
    k = int(k)
    if not 1 <= k <= ops.KNN_MAX:
        raise ValueError("knn_graph: k must be in 1..%d, got %d" % (ops.KNN_MAX, k))
    p = pos.detach().contiguous()
    n, D = p.shape
    if n * k >= 2 ** 31:
        raise ValueError("knn_graph: %d rows of up to %d edges do not fit int32" % (n, k))
    out = _graphs_of("knn_graph", p, batch)
    L, LF = _knn_lanes(k, out.max_count, n) if lanes is None else (lanes, lanes)
    deg, tau_d2, tau_j = ops.knn_select(p, D, k, out.gptr, out.batch, r=r, loop=loop, lanes=L)
    rp = torch.zeros(n + 1, dtype=torch.int64, device=p.device)
    rp[1:] = torch.cumsum(deg, 0, dtype=torch.int64)
    nnz = int(rp[-1])                                         # the one host sync
    out.rowptr = rp.to(torch.int32)
    out.col, out.d2 = ops.knn_fill(p, D, out.gptr, out.batch, out.rowptr, tau_d2, tau_j, loop=loop, lanes=LF, nnz=nnz,
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
    graph with ``rowptr`` / ``col`` / ``transposed_perm()`` -- a ``radius_graph``, a (directed)
    ``knn_graph``, or a bond graph
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
