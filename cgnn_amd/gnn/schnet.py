"""SchNet (Schuett et al., 2017) on the layer API -- GNN track, not in the reference.

Positions -> energy -> forces end to end: ``radius_graph`` builds the neighbour list on the
device, ``pair_distance`` gives the edge distances with their gradient to the positions,
``GaussianSmearing`` / ``cosine_cutoff`` the filter inputs, ``CFConv`` the continuous-filter
convolutions (``ops.espmm``) and ``graph_readout`` the sum over each molecule's atoms.  No
PyTorch scatter sits on the path: the embedding is a one-hot product, every sum over edges
or atoms is one of the deterministic kernels.
"""
from __future__ import annotations

import math
from typing import Optional, Union

import torch

from .geometry import GaussianSmearing, cosine_cutoff, pair_distance, radius_graph
from .layers import CFConv, _Dense
from .readout import GraphBatch, graph_readout


def shifted_softplus(x: torch.Tensor) -> torch.Tensor:
    """``softplus(x) - log 2``: SchNet's activation, 0 at 0."""
    return torch.nn.functional.softplus(x) - math.log(2.0)


class _Interaction(torch.nn.Module):
    """``x + Dense(ssp(CFConv(x)))``: one SchNet interaction block with its residual."""

    def __init__(self, hidden, n_filters, n_gaussians, generator):
        super().__init__()
        self.conv = CFConv(hidden, hidden, n_filters, n_gaussians, generator=generator)
        self.dense = _Dense(hidden, hidden, generator=generator)

    def forward(self, x, g, e, c):
        return x + self.dense(shifted_softplus(self.conv(x, g, e, cutoff=c)))


class SchNet(torch.nn.Module):
    """``E_g = sum_{i in g} MLP(x_i^T)`` with ``x^0 = embedding[z]`` and ``T = n_interactions``
    blocks ``x <- x + Dense(ssp(CFConv(x, e, c)))``, where ``e = GaussianSmearing(0, cutoff,
    n_gaussians)(d)`` and ``c = cosine_cutoff(d, cutoff)`` of the pair distances ``d`` of the
    radius graph of ``cutoff`` (with ``max_num_neighbors``: of each atom's that many nearest
    neighbours inside it, a directed neighbour list).  The output MLP is ``hidden -> hidden // 2 -> 1`` with a shifted
    softplus between.  ``z``: atomic numbers in ``[0, max_z)``.  The embedding rows are standard
    normal, the dense layers Glorot-uniform with zero biases, all drawn from ``generator``.

    Periodic systems: ``neighbors``, ``forward`` and ``energy_and_forces`` take ``cell=`` / ``pbc=``
    as ``radius_graph`` does (positions inside the cell: ``geometry.wrap_positions``); an atom then
    interacts with the lattice images of the others and of itself.

    ``method``: ``radius_graph``'s -- ``"auto"`` (cell lists for large point clouds), ``"brute"`` or
    ``"cells"``; the neighbour list, and so the energy and the forces, are the same bit for bit.

    Out of scope: training on forces (a double backward through ``pair_distance``), the
    gradient with respect to the cell (stress) and ``max_num_neighbors`` over periodic images."""

    def __init__(self, hidden: int = 128, n_filters: int = 128, n_interactions: int = 3, n_gaussians: int = 50,
                 cutoff: float = 5.0, max_z: int = 100, generator: Optional[torch.Generator] = None,
                 max_num_neighbors: Optional[int] = None, method: str = "auto"):
        super().__init__()
        if hidden < 2 or n_interactions < 0 or not cutoff > 0:
            raise ValueError("SchNet: hidden >= 2, n_interactions >= 0 and cutoff > 0 expected")
        self.cutoff, self.max_z = float(cutoff), int(max_z)
        self.method = method
        self.max_num_neighbors = None if max_num_neighbors is None else int(max_num_neighbors)
        self.embedding = torch.nn.Parameter(torch.randn(self.max_z, hidden, generator=generator))
        self.smearing = GaussianSmearing(0.0, self.cutoff, n_gaussians)
        self.interactions = torch.nn.ModuleList(
            _Interaction(hidden, n_filters, n_gaussians, generator) for _ in range(n_interactions))
        self.out1 = _Dense(hidden, hidden // 2, generator=generator)
        self.out2 = _Dense(hidden // 2, 1, generator=generator)

    def neighbors(self, pos: torch.Tensor, batch: Union[GraphBatch, torch.Tensor, None] = None,
                  cell: Optional[torch.Tensor] = None, pbc=True) -> GraphBatch:
        """The radius graph of the model's cutoff, capped at the ``max_num_neighbors`` nearest
        (one host sync: ``radius_graph``); with ``cell`` the periodic one.  The model's ``method``
        (``"auto"`` / ``"brute"`` / ``"cells"``) goes to ``radius_graph``: the same list either way."""
        return radius_graph(pos, self.cutoff, batch, max_num_neighbors=self.max_num_neighbors, cell=cell, pbc=pbc,
                            method=self.method)

    def forward(self, z: torch.Tensor, pos: torch.Tensor, batch: Union[GraphBatch, torch.Tensor, None] = None,
                graph: Optional[GraphBatch] = None, cell: Optional[torch.Tensor] = None, pbc=True) -> torch.Tensor:
        """The energy of each graph, ``[n_graphs]``.  ``z`` integer ``[n]``, ``pos`` ``[n, D]``;
        ``batch``, ``cell`` and ``pbc`` as in ``radius_graph``.  ``graph``: a neighbour list from
        ``neighbors`` to reuse (``batch``, ``cell`` and ``pbc`` are then ignored: a periodic list
        carries its cell)."""
        if z.dim() != 1 or z.shape[0] != pos.shape[0] or z.is_floating_point():
            raise ValueError("SchNet: z must be an integer vector [%d], got %s %s"
                             % (pos.shape[0], z.dtype, tuple(z.shape)))
        g = self.neighbors(pos, batch, cell, pbc) if graph is None else graph
        d = pair_distance(pos, g)
        e = self.smearing(d)
        c = cosine_cutoff(d, self.cutoff)
        x = torch.nn.functional.one_hot(z.long(), self.max_z).to(d.dtype) @ self.embedding.to(d.dtype)
        for block in self.interactions:
            x = block(x, g, e, c)
        y = self.out2(shifted_softplus(self.out1(x)))
        return graph_readout(y, g, "sum")[:, 0]

    def energy_and_forces(self, z: torch.Tensor, pos: torch.Tensor,
                          batch: Union[GraphBatch, torch.Tensor, None] = None, graph: Optional[GraphBatch] = None,
                          cell: Optional[torch.Tensor] = None, pbc=True):
        """``(E [n_graphs], F [n, D])`` with ``F = -dE/dpos`` through ``torch.autograd.grad``.
        The parameters receive no gradient and the force is not differentiable."""
        p = pos.detach().requires_grad_(True)
        with torch.enable_grad():
            E = self.forward(z, p, batch, graph, cell, pbc)
            dpos, = torch.autograd.grad(E.sum(), p)
        return E.detach(), -dpos
