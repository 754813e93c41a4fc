"""The cell-list radius search on the GPU (gnn_cells.hip) against the fp64 numpy reference of
test_gnn_geometry_gpu.py, against closed forms, and -- for general fp32 positions -- against
the brute-force kernels of gnn_geometry.hip, which their own exact tests pin.  Every
comparison is ``torch.equal``: the cell path must return the brute-force CSR bit for bit.

The row pass (cells_rows_kernel) has no fast path and no capacity: one code path for every
row length, exercised here with rows of 4 to more than 700 entries.
"""
import numpy as np
import pytest
import torch

import test_gnn_geometry_gpu as gg
from cgnn_amd.gnn import geometry, ops
from cgnn_amd.gnn.geometry import pair_distance, radius_graph
from cgnn_amd.gnn.readout import GraphBatch
from cgnn_amd.gnn.schnet import SchNet

pytestmark = pytest.mark.gpu

DEV = gg.DEV
SENT = gg.SENT
R = gg.R
SIZES = gg.SIZES
LANES = (8, 16, 32, 64)


def batch_of(sizes):
    gp = torch.tensor(gg.gptr_of(sizes), dtype=torch.int32, device=DEV)
    seg = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes)).to(DEV)
    return gp, seg


def run_cells(pos, D, r, sizes, loop, lanes=None, tail=5):
    """The five steps through the ops with sentinel rows and tails, checked: a dict of deg,
    rowptr, col, d2 (CPU) and the grid tables and cell ids (CPU)."""
    n, G = pos.shape[0], len(sizes)
    gp, seg = batch_of(sizes)
    p = torch.tensor(pos, device=DEV)
    glo = torch.full((G, 8), float(SENT), device=DEV)
    gn = torch.full((G, 4), SENT, dtype=torch.int32, device=DEV)
    ops.cells_grid(p, D, r, gp, glo=glo, gn=gn)
    cid = torch.full((n + tail,), SENT, dtype=torch.int32, device=DEV)
    ops.cells_bin(p, D, gp, seg, glo, gn, out=cid)
    assert bool((cid[n:] == SENT).all()), "bin wrote past its rows"
    assert bool(((cid[:n] >= 0) & (cid[:n] <= n + G)).all())
    perm, scell, cptr, spos = ops.cells_order(p, D, cid[:n], G)
    assert cptr.numel() == n + G + 2 and spos.shape == (n, 4)
    deg = torch.full((n + tail,), SENT, dtype=torch.int32, device=DEV)
    ops.cells_count(spos, perm, scell, cptr, gp, seg, gn, D, r, loop=loop, lanes=lanes, out=deg)
    assert bool((deg[n:] == SENT).all()), "count wrote past its rows"
    rp = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    rp[1:] = torch.cumsum(deg[:n], 0, dtype=torch.int64)
    nnz = int(rp[-1])
    col = torch.full((nnz + tail,), SENT, dtype=torch.int32, device=DEV)
    d2 = torch.full((nnz + tail,), float(SENT), dtype=torch.float32, device=DEV)
    sj = torch.full((nnz + tail,), SENT, dtype=torch.int32, device=DEV)
    sd = torch.full((nnz + tail,), float(SENT), dtype=torch.float32, device=DEV)
    ops.cells_fill(spos, perm, scell, cptr, gp, seg, gn, D, r, rp.to(torch.int32), loop=loop, lanes=lanes, out=col,
                   d2=d2, scratch=(sj, sd))
    assert bool((col[nnz:] == SENT).all()) and bool((d2[nnz:] == SENT).all()), "fill wrote past nnz"
    assert bool((sj[nnz:] == SENT).all()) and bool((sd[nnz:] == SENT).all()), "the scratch list was written past nnz"
    return dict(deg=deg[:n].cpu(), rowptr=rp.to(torch.int32).cpu(), col=col[:nnz].cpu(), d2=d2[:nnz].cpu(),
                glo=glo.cpu(), gn=gn.cpu(), cid=cid[:n].cpu())


def run_brute(pos, D, r, sizes, loop):
    """(rowptr, col, d2) of the brute-force kernels (CPU tensors)."""
    n = pos.shape[0]
    gp, seg = batch_of(sizes)
    p = torch.tensor(pos, device=DEV)
    deg = ops.radius_count(p, D, r, gp, seg, loop=loop)
    rp = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    rp[1:] = torch.cumsum(deg, 0, dtype=torch.int64)
    col, d2 = ops.radius_fill(p, D, r, gp, seg, rp.to(torch.int32), loop=loop, with_d2=True)
    return rp.to(torch.int32).cpu(), col.cpu(), d2.cpu()


def assert_csr(c, rowptr, col, d2):
    assert torch.equal(c["rowptr"], rowptr)
    assert torch.equal(c["deg"], rowptr[1:] - rowptr[:-1])
    assert torch.equal(c["col"], col)
    assert torch.equal(c["d2"].view(torch.int32), d2.view(torch.int32))


def rows_of(rowptr):
    return torch.repeat_interleave(torch.arange(rowptr.numel() - 1), (rowptr[1:] - rowptr[:-1]).long())


# ---------------------------------------------------------------- 1: exact edge sets

@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("D,ldp", [(1, 1), (1, 4), (2, 2), (2, 4), (3, 3), (3, 4)])
def test_cells_exact_edge_sets(D, ldp, loop):
    pos, rowptr, col, d2 = gg.reference(D, ldp, loop)
    c = run_cells(pos, D, R, SIZES, loop)
    assert_csr(c, rowptr, col, d2)
    off = int(gg.gptr_of(SIZES)[SIZES.index(200)])
    n, G = pos.shape[0], len(SIZES)
    assert int(c["deg"][off + 50]) == 0 and int(c["deg"][off + 60]) == 0
    assert int(c["cid"][off + 50]) == n + G and int(c["cid"][off + 60]) == n + G       # the sentinel cell
    # the grids are real grids: some graph has at least 3 cells on every axis ...
    assert bool((c["gn"][:, :D] >= 3).all(1).any()), c["gn"].tolist()
    # ... never more cells than points, and a pair exactly on the boundary lies in two cells
    sizes = torch.tensor(SIZES)
    assert bool((c["gn"][:, 3].long() <= sizes.clamp(min=1)).all())
    on = d2 == np.float32(R) * np.float32(R)
    i, j = rows_of(rowptr)[on], col[on].long()
    assert i.numel() > 0 and bool((c["cid"][i] != c["cid"][j]).any()), "no boundary pair across two cells"


# ---------------------------------------------------------------- 2: pairs on cell boundaries

def test_chain_with_every_pair_on_the_boundary():
    pos = (1.25 * np.arange(41, dtype=np.float32))[:, None]
    for loop in (False, True):
        c = run_cells(pos, 1, 1.25, [41], loop)
        want = torch.full((41,), 2, dtype=torch.int32)
        want[0] = want[40] = 1
        assert torch.equal(c["deg"], want + int(loop))
        assert int(c["gn"][0, 0]) >= 3
        d = c["d2"]
        assert bool(((d == 1.5625) | (d == 0)).all()) and int((d == 1.5625).sum()) == 80
        rows = rows_of(c["rowptr"])
        assert bool(((c["col"].long() - rows).abs() <= 1).all())


def test_integer_lattice_has_its_lattice_neighbours():
    m = 12
    ax = np.arange(m, dtype=np.float32)
    pos = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    c = run_cells(pos, 3, 1.0, [m ** 3], False)
    want = ((pos > 0).sum(1) + (pos < m - 1).sum(1)).astype(np.int32)
    assert want.min() == 3 and want.max() == 6
    assert torch.equal(c["deg"], torch.tensor(want))
    assert bool((c["d2"] == 1).all())
    assert bool((c["gn"][0, :3] >= 3).all())
    rows = rows_of(c["rowptr"])
    assert bool((c["col"][1:] > c["col"][:-1])[rows[1:] == rows[:-1]].all()), "rows not in ascending id"


# ---------------------------------------------------------------- 3: long rows, a crowded cell

def crowded():
    """700 points of 27 positions inside one cell and 300 sparse ones around, one graph."""
    rng = np.random.default_rng(5)
    dense = rng.integers(0, 3, size=(700, 3)).astype(np.float32) / 4           # [0, 1/2]^3
    sparse = rng.integers(-24, 25, size=(300, 3)).astype(np.float32) / 4
    sparse[0], sparse[1] = -6.0, 6.0                                            # the corners of the box
    pos = np.concatenate([sparse[:150], dense, sparse[150:]])
    return pos


def test_long_rows_and_a_crowded_cell():
    pos = crowded()
    rowptr, col, d2 = gg.ref_radius(pos, 3, R, [1000], False)
    c = run_cells(pos, 3, R, [1000], False)
    assert int(torch.bincount(c["cid"]).max()) >= 700, "the dense points do not share a cell"
    assert int(c["deg"].max()) >= 699
    assert_csr(c, rowptr, col, d2)


# ---------------------------------------------------------------- 4: general fp32 positions

_GENERAL = {}


def general(D):
    """Three graphs: 20,000 uniform points in a 16^3 box, 3,000 with constant z, one point."""
    if D not in _GENERAL:
        rng = np.random.default_rng(21)
        a = rng.uniform(0, 16, size=(20000, 3)).astype(np.float32)
        b = rng.uniform(0, 16, size=(3000, 3)).astype(np.float32)
        b[:, 2] = 3.5
        pos = np.concatenate([a, b, np.float32([[1.0, 2.0, 3.0]])])[:, :D].copy()
        _GENERAL[D] = pos
    return _GENERAL[D], [20000, 3000, 1]


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("D", [3, 2])
def test_general_positions_equal_the_brute_force_kernels(D, loop):
    pos, sizes = general(D)
    rowptr, col, d2 = run_brute(pos, D, 1.0, sizes, loop)
    c = run_cells(pos, D, 1.0, sizes, loop)
    assert col.numel() > 100000
    assert_csr(c, rowptr, col, d2)
    assert bool((c["gn"][0, :D] >= 8).all())
    if D == 3:
        assert int(c["gn"][1, 2]) == 1 and int(c["gn"][1, 0]) > 1               # one cell along the constant z
    assert c["gn"][2].tolist() == [1, 1, 1, 1]


# ---------------------------------------------------------------- 5: degenerate grids

def degenerate_cases():
    rng = np.random.default_rng(9)
    quarter = lambda n, w: rng.integers(-4 * w, 4 * w + 1, size=(n, 3)).astype(np.float32) / 4
    coincident = np.tile(np.float32([[0.25, -1.5, 2.0]]), (100, 1))
    huge = quarter(90, 4)
    huge[3] = 3e38
    huge[7] = -3e38
    huge[11, 1] = 3e38
    huge[12, 1] = -3e38
    zero = quarter(300, 2)
    zero[5] = zero[4]
    wide = quarter(200, 2)
    padded = gg.grid_positions([9, 130, 64], 3, 4, seed=3, special=False)
    return [("coincident", coincident, 3, 0.5, [100]), ("overflow", huge, 3, R, [40, 50]),
            ("r = 0", zero, 3, 0.0, [300]), ("r > cloud", wide, 3, 100.0, [120, 80]),
            ("ldp = 4", padded, 3, R, [9, 130, 64]), ("overflow 1-D", huge[:, :1].copy(), 1, R, [90])]


@pytest.mark.parametrize("case", degenerate_cases(), ids=lambda c: c[0])
def test_degenerate_grids_equal_the_brute_path(case):
    name, pos, D, r, sizes = case
    if name == "ldp = 4":
        assert bool((pos[:, 3] == gg.BIG).all())
    for loop in (False, True):
        rowptr, col, d2 = run_brute(pos, D, r, sizes, loop)
        c = run_cells(pos, D, r, sizes, loop)
        assert_csr(c, rowptr, col, d2)
        if name in ("coincident", "r > cloud"):
            assert bool((c["gn"] == 1).all())
            assert col.numel() == sum(s * (s - 1 + int(loop)) for s in sizes)
        if name == "overflow":
            assert int(c["gn"][0, 0]) == 1 and int(c["gn"][0, 1]) == 1           # the extent is not finite
        if name == "r = 0":
            assert bool((d2 == 0).all()) and col.numel() >= 2 + 300 * int(loop)
            assert int(c["gn"][0, 3]) > 1


# ---------------------------------------------------------------- 6: invariance

@pytest.mark.parametrize("lanes", LANES)
def test_every_lanes_value_gives_the_same_csr(lanes):
    pos, rowptr, col, d2 = gg.reference(3, 4, False)
    assert_csr(run_cells(pos, 3, R, SIZES, False, lanes=lanes), rowptr, col, d2)
    pos = crowded()
    rowptr, col, d2 = gg.ref_radius(pos, 3, R, [1000], False)
    assert_csr(run_cells(pos, 3, R, [1000], False, lanes=lanes), rowptr, col, d2)


def test_two_runs_give_the_same_csr():
    pos, sizes = general(3)
    a = run_cells(pos, 3, 1.0, sizes, False)
    b = run_cells(pos, 3, 1.0, sizes, False)
    for k in ("rowptr", "col", "cid", "gn"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["d2"].view(torch.int32), b["d2"].view(torch.int32))


def test_a_graph_keeps_its_rows_wherever_it_stands():
    sizes = [65, 9, 130, 33, 600]
    pos = gg.grid_positions(sizes, 3, 3, seed=7, special=False)
    gp = gg.gptr_of(sizes)
    a = run_cells(pos, 3, R, sizes, False)
    perm = [2, 4, 0, 3, 1]
    pos2 = np.concatenate([pos[gp[k]:gp[k + 1]] for k in perm])
    sizes2 = [sizes[k] for k in perm]
    gp2 = gg.gptr_of(sizes2)
    b = run_cells(pos2, 3, R, sizes2, False)
    assert a["col"].numel() == b["col"].numel()
    for new, old in enumerate(perm):
        rp, rp2 = a["rowptr"], b["rowptr"]
        a0, a1 = int(rp[gp[old]]), int(rp[gp[old + 1]])
        b0, b1 = int(rp2[gp2[new]]), int(rp2[gp2[new + 1]])
        assert a1 - a0 == b1 - b0 and a1 > a0
        assert torch.equal(rp[gp[old]:gp[old + 1] + 1] - a0, rp2[gp2[new]:gp2[new + 1] + 1] - b0)
        assert torch.equal(a["col"][a0:a1] - int(gp[old]), b["col"][b0:b1] - int(gp2[new]))
        assert torch.equal(a["d2"][a0:a1].view(torch.int32), b["d2"][b0:b1].view(torch.int32))
        assert torch.equal(a["gn"][old], b["gn"][new]) and torch.equal(a["glo"][old], b["glo"][new])


# ---------------------------------------------------------------- 7: the public API

def same_graph(a, b):
    for k in ("rowptr", "col", "eperm", "gptr", "batch"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert getattr(a, k).dtype == getattr(b, k).dtype, k
    assert torch.equal(a.d2.view(torch.int32), b.d2.view(torch.int32))
    assert a.n_graphs == b.n_graphs and a.rowptr.device.type == "cuda"


def test_radius_graph_methods_agree_and_pair_distance_is_bitwise_equal():
    pos = torch.tensor(gg.grid_positions(SIZES, 3, 3, seed=103, special=False), device=DEV)
    batch = GraphBatch(torch.tensor(gg.gptr_of(SIZES)))
    for loop in (False, True):
        a = radius_graph(pos, R, batch, loop=loop, method="brute")
        b = radius_graph(pos, R, batch, loop=loop, method="cells")
        same_graph(a, b)
        assert torch.equal(b.eperm.cpu(), torch.arange(b.col.numel()))
    out = []
    for g in (a, b):
        p = pos.clone().requires_grad_(True)
        d = pair_distance(p, g)
        w = torch.arange(d.numel(), device=DEV, dtype=torch.float32) % 7 - 3
        (d * w).sum().backward()
        out.append((d.detach(), p.grad))
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32))
    assert torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32))
    assert float(out[0][1].abs().max()) > 0


def test_schnet_methods_give_the_same_energy_and_forces():
    rng = np.random.default_rng(4)
    sizes = [40, 1, 300, 0, 90]
    n = sum(sizes)
    pos = torch.tensor(rng.uniform(0, 6, size=(n, 3)).astype(np.float32), device=DEV)
    z = torch.tensor(rng.integers(1, 10, n), device=DEV)
    batch = GraphBatch(torch.tensor(gg.gptr_of(sizes))).to(DEV)
    res = []
    for method in ("brute", "cells", "auto"):
        model = SchNet(hidden=32, n_filters=32, n_interactions=2, n_gaussians=16, cutoff=1.5,
                       generator=torch.Generator().manual_seed(8), method=method).to(DEV)
        res.append(model.energy_and_forces(z, pos, batch))
    for E, F in res[1:]:
        assert torch.equal(E.view(torch.int32), res[0][0].view(torch.int32))
        assert torch.equal(F.view(torch.int32), res[0][1].view(torch.int32))
    assert float(res[0][1].abs().max()) > 0


def test_auto_equals_both_methods_on_either_side_of_the_threshold():
    rng = np.random.default_rng(6)
    big = geometry._CELLS_MIN_POINTS + 37
    for n in (big, 1500):
        side = (n / 3.0) ** (1 / 3)                                   # about 12 neighbours inside r = 1
        pos = torch.tensor(rng.uniform(0, side, size=(n, 3)).astype(np.float32), device=DEV)
        g = {m: radius_graph(pos, 1.0, method=m) for m in ("auto", "brute", "cells")}
        assert g["auto"].col.numel() > 4 * n
        same_graph(g["auto"], g["brute"])
        same_graph(g["auto"], g["cells"])
