"""The CPU branches of the k-NN ops (ops.knn_select / ops.knn_fill) and the layers above them
(knn_graph, radius_graph(max_num_neighbors=), SchNet(max_num_neighbors=)) on CPU tensors,
against a numpy fp64 reference computed here from the definition, and their argument errors.

The reference (``knn_base`` / ``knn_from_base``, shared with test_gnn_knn_gpu.py): per graph,
the fp64 matrix of squared distances; the candidates of row i are the j with j != i unless
loop, a finite d2 and d2 <= fp32(r) * fp32(r); a stable argsort of the row (the non-candidates
at +inf) orders them by the key (d2, j); the first min(k, #candidates) are kept and written in
ascending id.  On the 1/4 grid of test_gnn_geometry_cpu.py every d2 is exact in fp32, so the
fp64 order is the fp32 order and every comparison is ``torch.equal``.
"""
import numpy as np
import pytest
import torch

import test_gnn_geometry_cpu as gc
from cgnn_amd.gnn import ops
from cgnn_amd.gnn.geometry import knn_graph, radius_graph
from cgnn_amd.gnn.readout import GraphBatch
from cgnn_amd.gnn.schnet import SchNet

R = gc.R
SIZES = gc.SIZES
NAN, INF = float("nan"), float("inf")


def knn_base(pos, D, r, sizes, loop):
    """Per graph ``(offset, d2 [s, s] fp64, #candidates [s], order [s, s])``: everything of the
    reference that does not depend on k."""
    r2 = np.inf if r is None else float(np.float32(r) * np.float32(r))
    base, off = [], 0
    with np.errstate(invalid="ignore", over="ignore"):
        for s in sizes:
            p = pos[off:off + s, :D].astype(np.float64)
            d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(2)
            cand = np.isfinite(d) & (d <= r2)
            if not loop:
                cand &= ~np.eye(s, dtype=bool)
            order = np.argsort(np.where(cand, d, np.inf), axis=1, kind="stable")
            base.append((off, d, cand.sum(1), order))
            off += s
    return base


def knn_from_base(base, k):
    """``(deg, tau_d2, tau_j, rowptr, col, d2, ties)`` for one k; ``ties``: the number of rows
    whose k-th and (k+1)-th candidates are equally far (the id decides)."""
    deg, td, tj, col, d2, ties = [], [], [], [], [], 0
    for off, d, cnt, order in base:
        s = d.shape[0]
        if s == 0:
            continue
        kept = np.minimum(cnt, k)
        rows = np.arange(s)
        last = order[rows, np.maximum(kept - 1, 0)]
        deg.append(kept)
        td.append(np.where(kept > 0, d[rows, last], -1.0))
        tj.append(np.where(kept > 0, last + off, -1))
        mask = np.zeros((s, s), dtype=bool)
        take = np.arange(s)[None, :] < kept[:, None]            # the first kept[i] of row i's order
        mask[np.repeat(rows, kept), order[take]] = True
        ii, jj = np.nonzero(mask)                                # sorted by (i, j)
        col.append(jj + off)
        d2.append(d[ii, jj])
        more = rows[cnt > k]
        if k < s:
            ties += int((d[more, order[more, k - 1]] == d[more, order[more, k]]).sum())
    cat = lambda xs, dt: torch.tensor(np.concatenate(xs) if xs else np.zeros(0), dtype=dt)   # noqa: E731
    deg = cat(deg, torch.int32)
    rowptr = torch.zeros(deg.numel() + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0)
    return (deg, cat(td, torch.float64), cat(tj, torch.int32), rowptr, cat(col, torch.int32),
            cat(d2, torch.float64), ties)


def ref_knn(pos, D, k, r, sizes, loop):
    return knn_from_base(knn_base(pos, D, r, sizes, loop), k)


def run_cpu(pos, D, k, r, sizes, loop, lanes=None):
    gp, seg = gc.batch_of(sizes)
    p = torch.as_tensor(pos)
    deg, td, tj = ops.knn_select(p, D, k, gp, seg, r=r, loop=loop, lanes=lanes)
    rp = torch.zeros(p.shape[0] + 1, dtype=torch.int32)
    rp[1:] = torch.cumsum(deg, 0)
    col, d2 = ops.knn_fill(p, D, gp, seg, rp, td, tj, loop=loop, with_d2=True)
    return deg, td, tj, rp, col, d2


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("r", [None, R])
@pytest.mark.parametrize("D,ldp", [(1, 1), (2, 4), (3, 3), (3, 4)])
def test_knn_ops_cpu_branch_on_the_grid(D, ldp, r, loop):
    pos = gc.grid_positions(SIZES, D, ldp, seed=D)
    base = knn_base(pos, D, r, SIZES, loop)
    tied = 0
    for k in (1, 2, 8, 9, 33, 64):
        deg, td, tj, rowptr, col, d2, ties = knn_from_base(base, k)
        tied += ties
        got = run_cpu(pos, D, k, r, SIZES, loop)
        assert got[1].dtype == torch.float32 and got[5].dtype == torch.float32
        for g, w in zip(got, (deg, td.float(), tj, rowptr, col, d2.float())):
            assert torch.equal(g, w), "k = %d" % k
        off = int(gc.gptr_of(SIZES)[SIZES.index(70)])           # the NaN and the inf point
        for i in (off + 50, off + 60):
            assert int(got[0][i]) == 0 and float(got[1][i]) == -1 and int(got[2][i]) == -1
            assert not bool((got[4] == i).any())
    assert tied > 0, "no tie at the k-th place"


def test_short_graphs_keep_everything_and_lanes_change_nothing():
    pos = gc.grid_positions(SIZES, 3, 3, seed=5, special=False)
    sizes = torch.tensor(SIZES)
    per_row = torch.repeat_interleave(sizes, sizes)
    deg = run_cpu(pos, 3, 64, None, SIZES, False)[0]
    assert torch.equal(deg.long(), (per_row - 1).clamp(max=64))
    deg = run_cpu(pos, 3, 64, None, SIZES, True)[0]
    assert torch.equal(deg.long(), per_row.clamp(max=64))
    want = run_cpu(pos, 3, 7, R, SIZES, False)
    for lanes in (8, 16, 32, 64):
        for g, w in zip(run_cpu(pos, 3, 7, R, SIZES, False, lanes=lanes), want):
            assert torch.equal(g, w)


def test_fp64_positions_on_the_cpu():
    rng = np.random.default_rng(3)
    sizes = [5, 40, 0, 17]
    pos = rng.normal(size=(sum(sizes), 3))
    for k, r in ((3, None), (6, 1.5)):
        deg, td, tj, rowptr, col, d2, _ = ref_knn(pos, 3, k, r, sizes, False)
        got = run_cpu(pos, 3, k, r, sizes, False)
        assert got[1].dtype == torch.float64 and got[5].dtype == torch.float64
        assert torch.equal(got[0], deg) and torch.equal(got[2], tj)
        assert torch.equal(got[3], rowptr) and torch.equal(got[4], col)
        assert torch.allclose(got[1], td, rtol=1e-14, atol=0) and torch.allclose(got[5], d2, rtol=1e-14, atol=0)


def test_all_points_coincident_the_lowest_ids_win():
    pos = np.full((50, 2), 0.75, dtype=np.float32)
    deg, td, tj, rp, col, d2 = run_cpu(pos, 2, 4, None, [50], False)
    assert bool((deg == 4).all()) and bool((td == 0).all()) and bool((d2 == 0).all())
    for i in range(50):
        assert col[4 * i:4 * i + 4].tolist() == [j for j in range(6) if j != i][:4]
    assert tj.tolist() == [4] * 4 + [3] * 46


def test_knn_graph_and_the_cap_of_radius_graph():
    pos = gc.grid_positions(SIZES, 3, 3, seed=9, special=False)
    p = torch.tensor(pos)
    gp = torch.tensor(gc.gptr_of(SIZES))
    for k, r in ((5, None), (5, R)):
        deg, td, tj, rowptr, col, d2, _ = ref_knn(pos, 3, k, r, SIZES, False)
        for g in (knn_graph(p, k, gp, r=r), knn_graph(p, k, GraphBatch(gp), r=r)) + (
                (radius_graph(p, r, gp, max_num_neighbors=k),) if r is not None else ()):
            assert g.n_graphs == len(SIZES) and g.n == p.shape[0]
            assert torch.equal(g.rowptr, rowptr) and torch.equal(g.col, col) and torch.equal(g.d2, d2.float())
            assert torch.equal(g.eperm, torch.arange(col.numel()))
    uncapped = radius_graph(p, R, gp)
    assert int((uncapped.rowptr[1:] - uncapped.rowptr[:-1]).max()) > 5            # the cap above bites
    capped = radius_graph(p, R, gp, max_num_neighbors=64, loop=True)
    full = radius_graph(p, R, gp, loop=True)
    assert torch.equal(capped.rowptr, full.rowptr) and torch.equal(capped.col, full.col)
    assert torch.equal(capped.d2, full.d2)
    one = knn_graph(p[:9], 3)                                                       # batch=None: one graph
    assert one.n_graphs == 1 and one.rowptr.tolist() == list(range(0, 28, 3))


@pytest.mark.parametrize("loop", [False, True])
def test_radius_graph_without_a_cap_is_unchanged(loop):
    pos = gc.grid_positions(SIZES, 3, 4, seed=2)
    rowptr, col, d2 = gc.ref_radius(pos, 3, R, SIZES, loop)
    g = radius_graph(torch.tensor(pos[:, :3].copy()), R, torch.tensor(gc.gptr_of(SIZES)), loop=loop,
                     max_num_neighbors=None)
    assert torch.equal(g.rowptr, rowptr) and torch.equal(g.col, col) and torch.equal(g.d2, d2)


def test_schnet_passes_the_cap_on():
    torch.manual_seed(0)
    pos = torch.randn(30, 3)
    gp = torch.tensor([0, 12, 30])
    model = SchNet(hidden=8, n_filters=8, n_interactions=1, n_gaussians=4, cutoff=2.5, max_num_neighbors=3,
                   generator=torch.Generator().manual_seed(1))
    g, want = model.neighbors(pos, gp), knn_graph(pos, 3, gp, r=2.5)
    assert torch.equal(g.rowptr, want.rowptr) and torch.equal(g.col, want.col)
    assert int((g.rowptr[1:] - g.rowptr[:-1]).max()) == 3
    plain = SchNet(hidden=8, n_filters=8, n_interactions=1, n_gaussians=4, cutoff=2.5,
                   generator=torch.Generator().manual_seed(1))
    assert plain.max_num_neighbors is None
    assert plain.neighbors(pos, gp).col.numel() > g.col.numel()
    E = model(torch.randint(1, 5, (30,)), pos, gp)
    assert E.shape == (2,) and bool(torch.isfinite(E).all())


def test_argument_errors():
    pos = torch.zeros(6, 3)
    gp, seg = gc.batch_of([2, 4])
    for k in (0, -1, 65):
        with pytest.raises(ValueError, match="k must be in 1..64"):
            ops.knn_select(pos, 3, k, gp, seg)
        with pytest.raises(ValueError, match="k must be in 1..64"):
            knn_graph(pos, k)
        with pytest.raises(ValueError, match="k must be in 1..64"):
            radius_graph(pos, 1.0, max_num_neighbors=k)
    for k, lanes in ((9, 8), (17, 16), (33, 32), (64, 8)):
        with pytest.raises(ValueError, match="fewer than k"):
            ops.knn_select(pos, 3, k, gp, seg, lanes=lanes)
    with pytest.raises(ValueError, match="lanes must be one of"):
        ops.knn_select(pos, 3, 4, gp, seg, lanes=12)
    with pytest.raises(ValueError, match="lanes must be one of"):
        ops.knn_fill(pos, 3, gp, seg, torch.zeros(7, dtype=torch.int32), torch.zeros(6), torch.zeros(6, dtype=torch.int32),
                     lanes=4)
    for r in (-0.5, NAN, -INF):
        with pytest.raises(ValueError, match="r must not be negative or NaN"):
            ops.knn_select(pos, 3, 2, gp, seg, r=r)
        with pytest.raises(ValueError):
            knn_graph(pos, 2, r=r)
    ops.knn_select(pos, 3, 2, gp, seg, r=INF)                                       # no radius
    with pytest.raises(ValueError, match="D must be 1, 2 or 3"):
        ops.knn_select(torch.zeros(6, 4), 4, 2, gp, seg)
    with pytest.raises(ValueError, match="seg_id must be"):
        ops.knn_select(pos, 3, 2, gp, seg[:5])
    with pytest.raises(ValueError, match="gptr must be a vector"):
        ops.knn_select(pos, 3, 2, gp[:1], seg)
    with pytest.raises(ValueError, match="deg must hold 6 rows"):
        ops.knn_select(pos, 3, 2, gp, seg, deg=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="tau_d2 must hold 6 rows"):
        ops.knn_select(pos, 3, 2, gp, seg, tau_d2=torch.zeros(3))
    deg, td, tj = ops.knn_select(pos, 3, 2, gp, seg)
    rp = torch.zeros(7, dtype=torch.int32)
    rp[1:] = torch.cumsum(deg, 0)
    with pytest.raises(ValueError, match=r"rowptr must be \[7\]"):
        ops.knn_fill(pos, 3, gp, seg, rp[:6], td, tj)
    with pytest.raises(ValueError, match="tau_j must hold 6 rows"):
        ops.knn_fill(pos, 3, gp, seg, rp, td, tj[:5])
    with pytest.raises(ValueError, match="seg_id must be"):
        ops.knn_fill(pos, 3, gp, seg[:2], rp, td, tj)
    with pytest.raises(ValueError, match="pos must be"):
        knn_graph(torch.zeros(6, 4), 2)
    with pytest.raises(ValueError, match="the batch describes 6 nodes"):
        knn_graph(torch.zeros(5, 3), 2, gp)
    with pytest.raises(TypeError, match="gptr must be an integer tensor"):
        knn_graph(pos, 2, gp.float())


def test_preallocated_outputs_and_a_short_rowptr():
    pos = gc.grid_positions([9, 33], 2, 2, seed=4, special=False)
    gp, seg = gc.batch_of([9, 33])
    p = torch.tensor(pos)
    n = p.shape[0]
    deg = torch.full((n + 3,), -7, dtype=torch.int32)
    td = torch.full((n + 3,), -7.0)
    tj = torch.full((n + 3,), -7, dtype=torch.int32)
    out = ops.knn_select(p, 2, 4, gp, seg, deg=deg, tau_d2=td, tau_j=tj)
    assert out[0] is deg and out[1] is td and out[2] is tj
    assert bool((deg[n:] == -7).all()) and bool((td[n:] == -7).all()) and bool((tj[n:] == -7).all())
    want = ref_knn(pos, 2, 4, None, [9, 33], False)
    assert torch.equal(deg[:n], want[0]) and torch.equal(tj[:n], want[2])
    # rows cut to two slots: each keeps its first two neighbours in ascending id
    rp = torch.arange(0, 2 * n + 1, 2, dtype=torch.int32)
    col = torch.full((2 * n + 3,), -7, dtype=torch.int32)
    d2 = torch.full((2 * n + 3,), -7.0)
    ops.knn_fill(p, 2, gp, seg, rp, td, tj, out=col, d2=d2)
    assert bool((col[2 * n:] == -7).all()) and bool((d2[2 * n:] == -7).all())
    full = want[4]
    for i in range(n):
        assert col[2 * i:2 * i + 2].tolist() == full[4 * i:4 * i + 2].tolist()
