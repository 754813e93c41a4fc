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
* periodic cells -- ``radius_graph(..., cell=, pbc=)`` searches the lattice images of every
  source too (``ops.radius_pbc_count`` / ``ops.radius_pbc_fill``) and the graph carries the image
  shift of each edge, which ``pair_distance`` adds to the source position
  (``ops.pair_d2_pbc`` / ``ops.pair_d2_pbc_bwd``); ``image_ranges`` gives the image box of a
  cutoff, ``wrap_positions`` brings positions into the cell.
* ``GaussianSmearing`` / ``cosine_cutoff`` -- SchNet's radial basis and cutoff envelope, plain
  PyTorch: elementwise on ``[nnz, K]``.

* cell lists -- ``radius_graph(..., method="cells")``, and ``"auto"`` for graphs of at least
  ``_CELLS_MIN_POINTS`` points: the binned search for large point clouds (``ops.cells_grid`` /
  ``cells_bin`` / ``cells_order`` / ``cells_count`` / ``cells_fill``), O(n) instead of O(n_g^2) and
  the brute-force graph bit for bit.

Limits.  Below ``_CELLS_MIN_POINTS`` the search is brute force inside each graph, O(n_g^2):
right for molecules and other graphs of up to a few thousand points.  The cell lists serve the
plain radius search only: no periodic cells, no k-NN and no neighbour cap on the cell path
(those stay brute force), ``D <= 3``; no k-NN in feature space (``D > 3``).  Periodic cells: the
radius search only (no k-NN and no
neighbour cap over images), at most ``ops.PBC_NIMG_MAX`` images per direction, no gradient
with respect to the cell (stress).  ``pair_distance`` is differentiable once: a double backward
(training on forces) is not implemented.
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


_METHODS = ("auto", "brute", "cells")

# method = "auto": the longest graph from which radius_graph takes the cell lists.  The
# measured crossover -- one cloud of 8192 points: brute force 105 us, cells 124 us; 16384
# points: 353 us against 110 us (docs/PERF.md, "Cell lists") -- rounded up to a power of two,
# and never below 4096: every shape measured on the brute-force kernels stays on them.
_CELLS_MIN_POINTS = 16384

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
    out.shift = out.cell = None                                # a periodic graph's edges are not taken over
    out._move(p.device)
    return out


def _cells_of(what, cell, pbc, G, D):
    """``(cells, periodic)``: the cells as fp32 ``[G, D, D]`` on the CPU (one small read-back
    for a cell on the device) and the periodic axes as bool ``[G, D]``."""
    if not isinstance(cell, torch.Tensor) or not cell.is_floating_point():
        raise TypeError("%s: cell must be a floating-point tensor" % what)
    c = cell.detach().to("cpu", torch.float32)
    if c.dim() == 2:
        c = c[None].expand(G, -1, -1)
    if c.dim() != 3 or c.shape[0] != G or c.shape[1] != c.shape[2] or c.shape[1] not in (D, 3):
        raise ValueError("%s: cell must be [%d, %d], [3, 3] or [%d, ., .] for %d graphs, got %s"
                         % (what, D, D, G, G, tuple(cell.shape)))
    c = c[:, :D, :D].contiguous()
    if not bool(torch.isfinite(c).all()):
        raise ValueError("%s: the cell must be finite" % what)
    pb = torch.as_tensor(pbc).to("cpu")
    if pb.dtype != torch.bool:
        raise TypeError("%s: pbc must be a bool, a bool per axis or bool [G, D]" % what)
    if pb.dim() == 0:
        pb = pb.expand(D)
    if pb.dim() == 1 and pb.numel() in (D, 3):
        pb = pb[None].expand(G, -1)
    if pb.dim() != 2 or pb.shape[0] != G or pb.shape[1] not in (D, 3):
        raise ValueError("%s: pbc must be a bool, %d (or 3) bools or [%d, %d], got shape %s"
                         % (what, D, G, D, tuple(pb.shape)))
    return c, pb[:, :D].contiguous()


def image_ranges(cell: torch.Tensor, pbc, r: float) -> torch.Tensor:
    """The lattice images a cutoff ``r`` reaches: int32 ``[G, 3]`` for cells ``[G, D, D]`` (or one
    ``[D, D]`` cell: ``[1, 3]``), row a of a cell being lattice vector a.  ``pbc``: a bool, one per
    axis, or ``[G, D]``.  Computed on the host in fp64: ``nimg[a] = ceil(r |b_a| (1 + 2^-20))`` for
    a periodic axis, where ``b_a`` is column a of ``inv(cell)`` -- ``1 / |b_a|`` is the height of
    the cell along a -- and 0 for any other axis (and for ``a >= D``).  With these ranges the
    periodic ``radius_graph`` misses no pair of positions that lie in the cell
    (``wrap_positions``): their fractional coordinates differ by less than 1, and a difference
    vector of length at most ``r`` spans at most ``r |b_a|`` along axis a.  The fractional
    coordinates are those of the whole cell, so an axis that is not periodic needs a lattice
    vector too (a slab: its vacuum height).  Raises ``ValueError`` for a singular cell with a
    periodic axis, and for a range above ``ops.PBC_NIMG_MAX``."""
    r = float(r)
    if not (r >= 0 and r < float("inf")):
        raise ValueError("image_ranges: r must be finite and not negative, got %r" % r)
    if not isinstance(cell, torch.Tensor) or cell.dim() not in (2, 3):
        raise ValueError("image_ranges: cell must be [D, D] or [G, D, D]")
    D = cell.shape[-1]
    if not 1 <= D <= 3:
        raise ValueError("image_ranges: cells of 1 to 3 dimensions expected, got %s" % (tuple(cell.shape),))
    G = 1 if cell.dim() == 2 else cell.shape[0]
    c, pb = _cells_of("image_ranges", cell, pbc, G, D)
    nimg = torch.zeros(G, 3, dtype=torch.int32)
    for g in range(G):
        if not bool(pb[g].any()):
            continue
        C = c[g].double()
        scale = float(C.abs().max())
        if scale == 0 or abs(float(torch.linalg.det(C / scale))) < 1e-12:
            raise ValueError("image_ranges: the cell of graph %d is singular and has a periodic axis" % g)
        b = torch.linalg.inv(C).norm(dim=0)                    # |b_a|, the inverse heights
        for a in range(D):
            if not bool(pb[g, a]):
                continue
            k = math.ceil(r * float(b[a]) * (1.0 + 2.0 ** -20))
            if k > ops.PBC_NIMG_MAX:
                raise ValueError("image_ranges: the cutoff %g reaches %d images along axis %d of graph %d, whose "
                                 "cell is %g high; at most %d are searched (use a supercell)"
                                 % (r, k, a, g, 1.0 / float(b[a]), ops.PBC_NIMG_MAX))
            nimg[g, a] = k
    return nimg


def wrap_positions(pos: torch.Tensor, cell: torch.Tensor, pbc=True,
                   batch: Union[GraphBatch, torch.Tensor, None] = None) -> torch.Tensor:
    """``pos`` moved by lattice vectors so that the fractional coordinates ``pos @ inv(cell)`` of
    the periodic axes lie in ``[0, 1)`` (up to the rounding of ``pos``'s dtype): ``pos -
    floor(frac) @ cell`` over the periodic axes.  ``cell``, ``pbc`` and ``batch`` as in
    ``radius_graph``.  Plain PyTorch on ``pos``'s device, differentiable with respect to ``pos``
    (the shift is piecewise constant)."""
    _positions(pos, "wrap_positions")
    n, D = pos.shape
    b = _graphs_of("wrap_positions", pos, batch)
    c, pb = _cells_of("wrap_positions", cell, pbc, b.n_graphs, D)
    if n == 0:
        return pos
    C = c.to(pos.device, pos.dtype)[b.batch.long()]             # [n, D, D]
    frac = torch.linalg.solve(C.transpose(1, 2), pos.detach()[:, :, None])[:, :, 0]       # frac @ C = pos
    k = torch.floor(frac) * pb.to(pos.device, pos.dtype)[b.batch.long()]
    return pos - (k[:, None, :] @ C)[:, 0, :]


def radius_graph(pos: torch.Tensor, r: float, batch: Union[GraphBatch, torch.Tensor, None] = None,
                 loop: bool = False, lanes: Optional[int] = None,
                 max_num_neighbors: Optional[int] = None, cell: Optional[torch.Tensor] = None, pbc=True,
                 method: str = "auto") -> GraphBatch:
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

    ``cell``: ``None``, or the periodic cell -- ``[D, D]`` (or ``[3, 3]``, of which the leading
    ``D x D`` block is used) for all graphs, or one per graph ``[G, D, D]``; row a is lattice
    vector a.  ``pbc``: which axes are periodic, a bool, one per axis, or ``[G, D]``.  A source
    is then searched in the lattice images ``image_ranges(cell, pbc, r)`` of every periodic
    axis too: row i holds the pairs (j, s) with ``|p_i - (p_j + s @ cell)|^2 <= r * r`` in
    ascending (j, s), without (i, 0) unless ``loop`` -- (i, s != 0) is an edge, an atom sees its
    own images, and two atoms may share several edges.  The result also carries ``.shift`` (int32
    ``[nnz]``, the packed s of each edge: ``ops.radius_pbc_fill``), ``.cell`` (fp32 ``[G, 9]`` on the
    device) and ``shifts()`` (int32 ``[nnz, 3]``); ``pair_distance`` and ``SchNet`` use them, every
    other layer sees an ordinary CSR.  **The neighbour list is complete when the positions lie
    in the cell** -- bring them there with ``wrap_positions`` -- and for positions outside it
    misses the images beyond the ranges.  A cell on the device costs one small read-back (like
    a ``gptr`` on the device), a CPU cell none.  ``max_num_neighbors`` together with ``cell``
    raises ``NotImplementedError``; a cutoff that needs more than ``ops.PBC_NIMG_MAX`` images
    along an axis raises (``image_ranges``).

    ``method``: ``"brute"`` searches every pair of a graph, O(n_g^2) (times the number of
    images): for molecules, crystal cells and graphs of up to a few thousand points.
    ``"cells"`` bins every graph into a grid of cells at least ``r`` wide, built on the device
    from its bounding box, and searches the neighbouring cells only (``ops.cells_grid`` /
    ``cells_bin`` / ``cells_order`` / ``cells_count`` / ``cells_fill``): O(n) for a point cloud of
    bounded density, and **the same** ``GraphBatch`` **bit for bit** (``rowptr``, ``col``, ``d2``,
    ``eperm``); still one host synchronisation, a handful of launches more and one scratch copy of
    the edge list.  ``"auto"`` (the default) takes the cells when the longest graph has at least
    ``_CELLS_MIN_POINTS`` points (docs/PERF.md, "Cell lists") and the brute search below.  The
    cell path is the plain radius search: together with ``cell=`` or ``max_num_neighbors=``
    ``"cells"`` raises ``NotImplementedError``, and ``"auto"`` leaves those two on their own
    (brute-force) paths.  Its default ``lanes`` does not depend on the graph lengths."""
    if method not in _METHODS:
        raise ValueError("radius_graph: method must be one of %s, got %r" % (_METHODS, method))
    if method == "cells" and (cell is not None or max_num_neighbors is not None):
        raise NotImplementedError("radius_graph: method = 'cells' searches neither periodic images (cell=) nor the "
                                  "nearest neighbours (max_num_neighbors=)")
    if cell is not None:
        if max_num_neighbors is not None:
            raise NotImplementedError("radius_graph: max_num_neighbors over periodic images is not implemented")
        return _radius_graph_pbc(pos, r, batch, loop, lanes, cell, pbc)
    if max_num_neighbors is not None:
        return knn_graph(pos, max_num_neighbors, batch, loop, r=r, lanes=lanes)
    _positions(pos, "radius_graph")
    p = pos.detach().contiguous()
    n, D = p.shape
    out = _graphs_of("radius_graph", p, batch)
    cells = method == "cells" or (method == "auto" and out.max_count >= _CELLS_MIN_POINTS)
    if cells:
        # grid, bins and cell order: launches and device plumbing, no read-back
        _, gn, _, perm, scell, cptr, spos = ops.cells_prepare(p, D, r, out.gptr, out.batch)
        deg = ops.cells_count(spos, perm, scell, cptr, out.gptr, out.batch, gn, D, r, loop=loop, lanes=lanes)
    else:
        L = _auto_lanes(out.max_count) if lanes is None else lanes
        deg = ops.radius_count(p, D, r, out.gptr, out.batch, loop=loop, lanes=L)
    rp = torch.zeros(n + 1, dtype=torch.int64, device=p.device)
    rp[1:] = torch.cumsum(deg, 0, dtype=torch.int64)
    nnz = int(rp[-1])                                         # the one host sync
    if nnz >= 2 ** 31:
        raise ValueError("radius_graph: %d edges do not fit int32" % nnz)
    out.rowptr = rp.to(torch.int32)
    if cells:
        out.col, out.d2 = ops.cells_fill(spos, perm, scell, cptr, out.gptr, out.batch, gn, D, r, out.rowptr, loop=loop,
                                         lanes=lanes, nnz=nnz, with_d2=True)
    else:
        out.col, out.d2 = ops.radius_fill(p, D, r, out.gptr, out.batch, out.rowptr, loop=loop, lanes=L, nnz=nnz,
                                          with_d2=True)
    out.eperm = torch.arange(nnz, dtype=torch.int64, device=p.device)
    out._tperm = None
    return out


def _radius_graph_pbc(pos, r, batch, loop, lanes, cell, pbc):
    _positions(pos, "radius_graph")
    p = pos.detach().contiguous()
    n, D = p.shape
    out = _graphs_of("radius_graph", p, batch)
    G = out.n_graphs
    c, pb = _cells_of("radius_graph", cell, pbc, G, D)
    nimg = image_ranges(c, pb, r) if G else torch.zeros(0, 3, dtype=torch.int32)
    cell9 = torch.zeros(G, 3, 3)
    cell9[:, :D, :D] = c
    out.cell = cell9.view(G, 9).to(p.device)
    images = (2 * nimg.long() + 1).prod(1)
    M = int(images.max()) if G else 1
    # the sub-group width as in the radius search, from a bound on the candidates of the longest
    # row that needs no read-back: the longest graph (a host integer) times the most images
    L = _auto_lanes(out.max_count * M) if lanes is None else lanes
    nd = nimg.to(p.device)
    deg = ops.radius_pbc_count(p, D, r, out.gptr, out.batch, out.cell, nd, loop=loop, lanes=L, max_images=M)
    rp = torch.zeros(n + 1, dtype=torch.int64, device=p.device)
    rp[1:] = torch.cumsum(deg, 0, dtype=torch.int64)
    nnz = int(rp[-1])                                         # the one host sync
    if nnz >= 2 ** 31:
        raise ValueError("radius_graph: %d edges do not fit int32" % nnz)
    out.rowptr = rp.to(torch.int32)
    out.col, out.shift, out.d2 = ops.radius_pbc_fill(p, D, r, out.gptr, out.batch, out.cell, nd, out.rowptr,
                                                     loop=loop, lanes=L, max_images=M, nnz=nnz, with_d2=True)
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
        if getattr(g, "shift", None) is not None:
            d2 = ops.pair_d2_pbc(g.rowptr, g.col, g.shift, p, p.shape[1], g.cell, g.batch)
        else:
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
        w = w.to(out.dtype).contiguous()
        if getattr(g, "shift", None) is not None:
            dpos = ops.pair_d2_pbc_bwd(g.rowptr, g.col, g.shift, rp_t, col_t, eperm_t, p, w, p.shape[1], g.cell,
                                       g.batch)
        else:
            dpos = ops.pair_d2_bwd(g.rowptr, g.col, rp_t, col_t, eperm_t, p, w, p.shape[1])
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
    loops).  A periodic ``radius_graph`` (one with ``.shift`` and ``.cell``) gives
    ``|p_i - (p_j + s @ cell)|`` through ``ops.pair_d2_pbc`` / ``ops.pair_d2_pbc_bwd``; the gradient
    goes to the positions only, not to the cell.  Differentiable **once**: a double backward,
    as training on forces needs, is not implemented and raises."""
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
