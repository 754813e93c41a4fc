"""The CPU branches of the cell-list radius search (ops.cells_grid / cells_bin / cells_order /
cells_count / cells_fill) against ``ops._radius_cpu`` and the fp64 numpy reference of
test_gnn_geometry_gpu.py, at the shapes of test_gnn_cells_gpu.py, in fp32 and with fp64
positions; the grid's properties checked directly; the ``method`` argument of ``radius_graph``.
"""
import numpy as np
import pytest
import torch

import test_gnn_geometry_gpu as gg
from cgnn_amd.gnn import geometry, ops
from cgnn_amd.gnn.geometry import radius_graph
from cgnn_amd.gnn.readout import GraphBatch
from cgnn_amd.gnn.schnet import SchNet

R = gg.R
SIZES = gg.SIZES
SENT = gg.SENT


def batch_of(sizes):
    gp = torch.tensor(gg.gptr_of(sizes), dtype=torch.int32)
    seg = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes))
    return gp, seg


def run_cells(pos, D, r, sizes, loop, dtype=torch.float32, tail=4):
    n = pos.shape[0]
    gp, seg = batch_of(sizes)
    p = torch.tensor(pos).to(dtype)
    glo, gn, cid, perm, scell, cptr, spos = ops.cells_prepare(p, D, r, gp, seg)
    deg = torch.full((n + tail,), SENT, dtype=torch.int32)
    ops.cells_count(spos, perm, scell, cptr, gp, seg, gn, D, r, loop=loop, out=deg)
    assert bool((deg[n:] == SENT).all())
    rp = torch.zeros(n + 1, dtype=torch.int32)
    rp[1:] = torch.cumsum(deg[:n], 0)
    nnz = int(rp[-1])
    col = torch.full((nnz + tail,), SENT, dtype=torch.int32)
    d2 = torch.full((nnz + tail,), float(SENT), dtype=dtype)
    ops.cells_fill(spos, perm, scell, cptr, gp, seg, gn, D, r, rp, loop=loop, out=col, d2=d2)
    assert bool((col[nnz:] == SENT).all()) and bool((d2[nnz:] == SENT).all())
    return dict(deg=deg[:n], rowptr=rp, col=col[:nnz], d2=d2[:nnz], glo=glo, gn=gn, cid=cid, p=p)


def brute(pos, D, r, sizes, loop, dtype=torch.float32):
    gp, _ = batch_of(sizes)
    deg, col, d2 = ops._radius_cpu(torch.tensor(pos).to(dtype), D, r, gp, loop)
    rp = torch.zeros(pos.shape[0] + 1, dtype=torch.int32)
    rp[1:] = torch.cumsum(deg, 0)
    return rp, col, d2


def assert_csr(c, rowptr, col, d2):
    assert torch.equal(c["rowptr"], rowptr) and torch.equal(c["col"], col)
    assert c["d2"].dtype == d2.dtype and torch.equal(c["d2"], d2)


def check_grid(c, D, r, sizes):
    """At most max(1, n_g) cells, every id in its graph's range, bins monotone in the
    coordinate, and every kept pair in cells that differ by at most one along every axis."""
    gn, glo, cid, p = c["gn"].long(), c["glo"], c["cid"].long(), c["p"]
    n, G = p.shape[0], len(sizes)
    gp = gg.gptr_of(sizes)
    sz = torch.tensor(sizes)
    assert torch.equal(gn[:, 3], gn[:, 0] * gn[:, 1] * gn[:, 2])
    assert bool((gn[:, 3] <= sz.clamp(min=1)).all()) and bool((gn[:, :3] >= 1).all())
    assert bool((gn[:, :3] <= ops.CELLS_NA_MAX).all()) and bool((gn[:, D:3] == 1).all())
    seg = torch.repeat_interleave(torch.arange(G), sz)
    base = torch.tensor(gp[:-1])[seg] + seg
    real = cid < n + G
    assert bool(((cid >= base) & (cid < base + gn[seg, 3]))[real].all())
    assert bool(torch.isfinite(p[real][:, :D]).all()) and not bool(torch.isfinite(p[~real][:, :D]).all(1).any())
    local = cid - base
    bins = []
    for a in reversed(range(3)):
        bins.append(local % gn[seg, a])
        local = local // gn[seg, a]
    bins = torch.stack(bins[::-1], 1)                         # [n, 3], the digits of the cell id (absent axes: 0)
    for g in range(G):
        m = real & (seg == g)
        for a in range(D):
            x, b = p[m, a], bins[m, a]
            order = torch.argsort(x, stable=True)
            assert bool((b[order][1:] >= b[order][:-1]).all()), "bins are not monotone"
    rows = torch.repeat_interleave(torch.arange(n), c["deg"].long())
    j = c["col"].long()
    assert bool(real[rows].all()) and bool(real[j].all())
    assert bool(((bins[rows] - bins[j]).abs() <= 1).all()), "a kept pair in cells that are not adjacent"


# ---------------------------------------------------------------- the cases of the GPU tests

@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("D,ldp", [(1, 1), (1, 4), (2, 2), (2, 4), (3, 3), (3, 4)])
def test_exact_edge_sets(D, ldp, loop, dtype):
    pos, rowptr, col, d2 = gg.reference(D, ldp, loop)
    c = run_cells(pos, D, R, SIZES, loop, dtype)
    assert_csr(c, rowptr, col, d2.to(dtype))
    assert_csr(c, *brute(pos, D, R, SIZES, loop, dtype))
    assert bool((c["gn"][:, :D] >= 3).all(1).any())
    on = d2 == np.float32(R) * np.float32(R)
    i = torch.repeat_interleave(torch.arange(pos.shape[0]), (rowptr[1:] - rowptr[:-1]).long())[on]
    assert bool((c["cid"][i] != c["cid"][col[on].long()]).any()), "no boundary pair across two cells"
    check_grid(c, D, R, SIZES)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_chain_and_lattice_on_cell_boundaries(dtype):
    pos = (1.25 * np.arange(41, dtype=np.float32))[:, None]
    c = run_cells(pos, 1, 1.25, [41], False, dtype)
    want = torch.full((41,), 2, dtype=torch.int32)
    want[0] = want[40] = 1
    assert torch.equal(c["deg"], want) and bool((c["d2"] == 1.5625).all()) and int(c["gn"][0, 0]) >= 3
    check_grid(c, 1, 1.25, [41])
    m = 12
    ax = np.arange(m, dtype=np.float32)
    pos = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    c = run_cells(pos, 3, 1.0, [m ** 3], False, dtype)
    want = ((pos > 0).sum(1) + (pos < m - 1).sum(1)).astype(np.int32)
    assert torch.equal(c["deg"], torch.tensor(want)) and bool((c["d2"] == 1).all())
    assert bool((c["gn"][0, :3] >= 3).all())
    check_grid(c, 3, 1.0, [m ** 3])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_long_rows_and_a_crowded_cell(dtype):
    rng = np.random.default_rng(5)
    dense = rng.integers(0, 3, size=(700, 3)).astype(np.float32) / 4
    sparse = rng.integers(-24, 25, size=(300, 3)).astype(np.float32) / 4
    sparse[0], sparse[1] = -6.0, 6.0
    pos = np.concatenate([sparse[:150], dense, sparse[150:]])
    rowptr, col, d2 = gg.ref_radius(pos, 3, R, [1000], False)
    c = run_cells(pos, 3, R, [1000], False, dtype)
    assert int(torch.bincount(c["cid"].long()).max()) >= 700 and int(c["deg"].max()) >= 699
    assert_csr(c, rowptr, col, d2.to(dtype))
    check_grid(c, 3, R, [1000])


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
    for loop in (False, True):
        c = run_cells(pos, D, r, sizes, loop)
        assert_csr(c, *brute(pos, D, r, sizes, loop))
        check_grid(c, D, r, sizes)
        if name in ("coincident", "r > cloud"):
            assert bool((c["gn"] == 1).all())
        if name == "overflow":
            assert int(c["gn"][0, 0]) == 1 and int(c["gn"][0, 1]) == 1
        if name == "r = 0":
            assert int(c["gn"][0, 3]) > 1 and c["col"].numel() >= 2


def test_general_fp32_positions_and_a_bad_seg_id():
    """Uniform positions (nothing exact) against ``_radius_cpu``; then a seg_id outside [0, G):
    an empty row, and the point is nobody's neighbour."""
    rng = np.random.default_rng(2)
    sizes = [1500, 400, 1]
    pos = rng.uniform(0, 8, size=(1901, 3)).astype(np.float32)
    pos[1500:1900, 2] = 3.5
    for D in (3, 2):
        q = pos[:, :D].copy()
        c = run_cells(q, D, 1.0, sizes, False)
        assert_csr(c, *brute(q, D, 1.0, sizes, False))
        check_grid(c, D, 1.0, sizes)
    gp, seg = batch_of(sizes)
    seg[7] = 9
    seg[8] = -1
    p = torch.tensor(pos)
    glo, gn, cid, perm, scell, cptr, spos = ops.cells_prepare(p, 3, 1.0, gp, seg)
    assert int(cid[7]) == 1901 + 3 and int(cid[8]) == 1901 + 3
    deg = ops.cells_count(spos, perm, scell, cptr, gp, seg, gn, 3, 1.0)
    assert int(deg[7]) == 0 and int(deg[8]) == 0
    rp = torch.zeros(1902, dtype=torch.int32)
    rp[1:] = torch.cumsum(deg, 0)
    col, _ = ops.cells_fill(spos, perm, scell, cptr, gp, seg, gn, 3, 1.0, rp)
    assert not bool(((col == 7) | (col == 8)).any())


# ---------------------------------------------------------------- the public API

def test_radius_graph_methods_agree_on_the_cpu():
    pos = torch.tensor(gg.grid_positions(SIZES, 3, 3, seed=103, special=False))
    batch = GraphBatch(torch.tensor(gg.gptr_of(SIZES)))
    a = radius_graph(pos, R, batch, method="brute")
    for m in ("cells", "auto"):
        b = radius_graph(pos, R, batch, method=m)
        for k in ("rowptr", "col", "d2", "eperm", "gptr"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(radius_graph(pos, R, batch).col, a.col)


def test_method_validation():
    pos = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="method"):
        radius_graph(pos, 1.0, method="grid")
    with pytest.raises(ValueError, match="method"):
        radius_graph(pos, 1.0, method=None)
    with pytest.raises(NotImplementedError):
        radius_graph(pos, 1.0, method="cells", cell=torch.eye(3) * 4)
    with pytest.raises(NotImplementedError):
        radius_graph(pos, 1.0, method="cells", max_num_neighbors=3)
    # "auto" leaves the two on their own paths
    assert radius_graph(pos, 1.0, method="auto", max_num_neighbors=3).col.numel() == 12
    assert radius_graph(pos, 1.0, method="auto", cell=torch.eye(3) * 4).shift is not None
    with pytest.raises(ValueError, match="method"):
        SchNet(hidden=8, n_filters=8, n_interactions=1, n_gaussians=4, cutoff=1.0, method="grid").neighbors(pos)


def test_the_threshold_of_auto_is_at_least_4096():
    assert isinstance(geometry._CELLS_MIN_POINTS, int) and geometry._CELLS_MIN_POINTS >= 4096
    assert geometry._CELLS_MIN_POINTS & (geometry._CELLS_MIN_POINTS - 1) == 0
