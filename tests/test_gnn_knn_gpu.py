"""The k-NN kernels on the GPU (gnn_geometry.hip: knn_select_kernel, knn_fill_kernel) and what
stands on them -- knn_graph, radius_graph(max_num_neighbors=), pair_distance on a directed
graph, SchNet(max_num_neighbors=) -- against numpy fp64 references computed from the
definition (test_gnn_knn_cpu.knn_base / knn_from_base), never through the CPU branches of
``ops``.

Exactness.  As in test_gnn_geometry_gpu.py the exact tests put every coordinate on multiples
of 1/4 in [-8, 8] (the adversarial 1-D graphs: on integers below 256), so every squared
distance is exact in fp32, the fp64 order of the keys (d2, j) is the fp32 order, and ``deg``,
``tau_d2``, ``tau_j``, ``rowptr``, ``col`` and ``d2`` are compared with ``torch.equal``.  The
narrow grid produces masses of equal distances: the tests assert that the k-th place is tied
in their inputs, so the "lower id wins" rule decides edges.
"""
import numpy as np
import pytest
import torch

import test_gnn_geometry_gpu as gg
import test_gnn_knn_cpu as kc
from cgnn_amd.gnn import ops
from cgnn_amd.gnn.geometry import knn_graph, pair_distance, radius_graph
from cgnn_amd.gnn.readout import GraphBatch
from cgnn_amd.gnn.schnet import SchNet
from cgnn_amd.utils.hipgraph import StepGraph

pytestmark = pytest.mark.gpu

DEV = gg.DEV
SENT = gg.SENT
R = gg.R
U = gg.U
LANES = gg.LANES
SIZES = gg.SIZES
KS = (1, 2, 7, 8, 9, 16, 17, 32, 33, 63, 64)            # crosses every sub-group width


def batch_on_device(sizes):
    gp = torch.tensor(gg.gptr_of(sizes), dtype=torch.int32, device=DEV)
    seg = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes)).to(DEV)
    return gp, seg


def run_knn(pos, D, k, r, sizes, loop, lanes=None, fill_lanes=None, tail=5):
    """(deg, tau_d2, tau_j, rowptr, col, d2) from the two passes with sentinel rows and tails,
    checked: select writes nothing past n, fill nothing past nnz."""
    n = pos.shape[0]
    gp, seg = batch_on_device(sizes)
    p = torch.tensor(pos, device=DEV)
    deg = torch.full((n + tail,), SENT, dtype=torch.int32, device=DEV)
    td = torch.full((n + tail,), float(SENT), dtype=torch.float32, device=DEV)
    tj = torch.full((n + tail,), SENT, dtype=torch.int32, device=DEV)
    ops.knn_select(p, D, k, gp, seg, r=r, loop=loop, lanes=lanes, deg=deg, tau_d2=td, tau_j=tj)
    assert bool((deg[n:] == SENT).all()) and bool((td[n:] == SENT).all()) and bool((tj[n:] == SENT).all()), \
        "select wrote past its rows"
    rp = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    rp[1:] = torch.cumsum(deg[:n], 0, dtype=torch.int64)
    nnz = int(rp[-1])
    col = torch.full((nnz + tail,), SENT, dtype=torch.int32, device=DEV)
    d2 = torch.full((nnz + tail,), float(SENT), dtype=torch.float32, device=DEV)
    ops.knn_fill(p, D, gp, seg, rp.to(torch.int32), td, tj, loop=loop, lanes=lanes if fill_lanes is None else fill_lanes,
                 out=col, d2=d2)
    assert bool((col[nnz:] == SENT).all()) and bool((d2[nnz:] == SENT).all()), "fill wrote past nnz"
    return deg[:n].cpu(), td[:n].cpu(), tj[:n].cpu(), rp.to(torch.int32).cpu(), col[:nnz].cpu(), d2[:nnz].cpu()


def want_of(base, k):
    """The reference in the dtypes of the kernels, and its number of tied k-th places."""
    deg, td, tj, rowptr, col, d2, ties = kc.knn_from_base(base, k)
    return (deg, td.float(), tj, rowptr, col, d2.float()), ties


def assert_same(got, want, what=""):
    for name, g, w in zip(("deg", "tau_d2", "tau_j", "rowptr", "col", "d2"), got, want):
        assert torch.equal(g, w), "%s %s" % (name, what)


_REF = {}


def reference(D, ldp, loop, r):
    """(pos, base) of the batch of test_gnn_geometry_gpu.py, computed once per case."""
    key = (D, ldp, loop, r)
    if key not in _REF:
        pos = gg.grid_positions(SIZES, D, ldp, seed=100 + D)
        _REF[key] = (pos, kc.knn_base(pos, D, r, SIZES, loop))
    return _REF[key]


# every (D, ldp), both loops and both radii twice, each with every k
CASES = [(1, 1, False, None), (2, 4, True, None), (3, 3, False, R), (3, 4, True, R),
         (1, 1, True, R), (2, 4, False, R), (3, 3, True, None), (3, 4, False, None)]


@pytest.mark.parametrize("D,ldp,loop,r", CASES)
def test_knn_exact_rows_thresholds_and_ties(D, ldp, loop, r):
    pos, base = reference(D, ldp, loop, r)
    sizes = torch.tensor(SIZES)
    per_row = torch.repeat_interleave(sizes, sizes)
    off = int(gg.gptr_of(SIZES)[SIZES.index(200)])
    tied = 0
    for k in KS:
        want, ties = want_of(base, k)
        if r is None:
            assert ties > 0, "no tie at the k-th place for k = %d" % k
        tied += ties
        got = run_knn(pos, D, k, r, SIZES, loop)
        assert_same(got, want, "k = %d" % k)
        deg, td, tj, rp, col, d2 = got
        if r is None:
            # graphs shorter than k keep everything (the graph of 200 holds the two non-finite points)
            short = (per_row <= k) & (per_row != 200)
            assert bool(short.any())
            assert torch.equal(deg[short].long(), per_row[short] - (0 if loop else 1))
        # the NaN point and the inf point: empty rows, in nobody's row
        for i in (off + 50, off + 60):
            assert int(deg[i]) == 0 and float(td[i]) == -1.0 and int(tj[i]) == -1
            assert not bool((col == i).any())
        assert bool(torch.isfinite(d2).all())
    assert tied > 0, "no tie at the k-th place"


@pytest.mark.parametrize("k", [2, 8, 9, 17, 33, 64])
def test_every_allowed_lanes_value_gives_the_same_csr(k):
    pos, base = reference(3, 4, False, None)
    want, _ = want_of(base, k)
    allowed = [L for L in LANES if L >= k]
    for L in allowed:
        assert_same(run_knn(pos, 3, k, None, SIZES, False, lanes=L), want, "select and fill lanes %d" % L)
    for L in LANES:                                           # the fill takes any width, whatever k was
        assert_same(run_knn(pos, 3, k, None, SIZES, False, lanes=allowed[0], fill_lanes=L), want, "fill lanes %d" % L)


def test_fill_writes_nothing_at_or_past_the_end_of_a_row():
    sizes = [9, 65, 33]
    pos = gg.grid_positions(sizes, 2, 2, seed=4, special=False)
    n = pos.shape[0]
    gp, seg = batch_on_device(sizes)
    p = torch.tensor(pos, device=DEV)
    deg, td, tj = ops.knn_select(p, 2, 4, gp, seg)
    assert bool((deg == 4).all())
    full = want_of(kc.knn_base(pos, 2, None, sizes, False), 4)[0][4]
    # every row gets two slots for its four neighbours; every other row's threshold is emptied,
    # so its slots stay untouched unless the row before it writes past its end
    rowptr = torch.arange(0, 2 * n + 1, 2, dtype=torch.int32, device=DEV)
    for lanes in (None,) + LANES:
        for i0 in (0, 1):
            td2, tj2 = td.clone(), tj.clone()
            td2[1 - i0::2] = -1.0
            tj2[1 - i0::2] = -1
            col = torch.full((2 * n + 3,), SENT, dtype=torch.int32, device=DEV)
            d2 = torch.full((2 * n + 3,), float(SENT), device=DEV)
            ops.knn_fill(p, 2, gp, seg, rowptr, td2, tj2, lanes=lanes, out=col, d2=d2)
            c = col[:2 * n].cpu().view(n, 2)
            assert torch.equal(c[i0::2], full.view(n, 4)[i0::2, :2]), "a row keeps its first two neighbours"
            assert bool((c[1 - i0::2] == SENT).all()) and bool((d2[:2 * n].view(n, 2)[1 - i0::2] == SENT).all())
            assert bool((d2[:2 * n].view(n, 2)[i0::2] >= 0).all())
            assert bool((col[2 * n:] == SENT).all()) and bool((d2[2 * n:] == SENT).all())


def line_graph(kind):
    """A batch [5, 200, 3] in 1-D on integers below 256 (every d2 < 2^16 is exact).  Seen from
    row 0 of the graph of 200, the candidates come in strictly decreasing distance (every one
    displaces a held key), strictly increasing distance (none after the first k does), or all
    points coincide (every key ties: the k lowest ids win)."""
    sizes = [5, 200, 3]
    pos = np.zeros((sum(sizes), 1), dtype=np.float32)
    pos[:5, 0] = [3, 1, 4, 1, 5]
    pos[205:, 0] = [2, 7, 2]
    j = np.arange(200, dtype=np.float32)
    pos[5:205, 0] = {"decreasing": np.where(j == 0, 0, 200 - j), "increasing": j, "coincident": 0 * j + 7}[kind]
    return sizes, pos


@pytest.mark.parametrize("kind", ["decreasing", "increasing", "coincident"])
def test_adversarial_candidate_order(kind):
    sizes, pos = line_graph(kind)
    d0 = np.abs(pos[6:205, 0] - pos[5, 0])
    if kind == "decreasing":
        assert np.all(np.diff(d0) < 0)
    elif kind == "increasing":
        assert np.all(np.diff(d0) > 0)
    base = kc.knn_base(pos, 1, None, sizes, False)
    for k in (1, 7, 8, 33, 64):
        want, ties = want_of(base, k)
        for L in [L for L in LANES if L >= k]:
            got = run_knn(pos, 1, k, None, sizes, False, lanes=L)
            assert_same(got, want, "%s k = %d lanes = %d" % (kind, k, L))
        deg, td, tj, rp, col, d2 = got
        row0 = col[int(rp[5]):int(rp[6])].tolist()
        if kind == "decreasing":
            assert row0 == list(range(205 - k, 205))             # the last k ids are the nearest
        elif kind == "increasing":
            assert row0 == list(range(6, 6 + k))
        else:
            assert ties >= 200 and bool((d2[int(rp[5]):int(rp[205])] == 0).all())
            assert row0 == list(range(6, 6 + k)) and int(tj[5]) == 5 + k
            assert col[int(rp[204]):int(rp[205])].tolist() == list(range(5, 5 + k))


def test_cross_checks_against_the_radius_search_and_pair_d2():
    sizes = [65, 9, 130, 33]
    pos = gg.grid_positions(sizes, 3, 3, seed=7, special=False)
    p = torch.tensor(pos, device=DEV)
    gp = torch.tensor(gg.gptr_of(sizes), device=DEV)
    for loop in (False, True):
        full = radius_graph(p, R, gp, loop=loop)
        degs = (full.rowptr[1:] - full.rowptr[:-1]).cpu()
        assert 4 < int(degs.max()) <= 64
        cap = radius_graph(p, R, gp, loop=loop, max_num_neighbors=64)
        assert torch.equal(cap.rowptr, full.rowptr) and torch.equal(cap.col, full.col)
        assert torch.equal(cap.d2.view(torch.int32), full.d2.view(torch.int32))
        assert torch.equal(cap.eperm.cpu(), torch.arange(full.col.numel()))
        few = radius_graph(p, R, gp, loop=loop, max_num_neighbors=4)
        assert few.n_graphs == len(sizes) and few.rowptr.device.type == "cuda"
        assert torch.equal((few.rowptr[1:] - few.rowptr[:-1]).cpu(), degs.clamp(max=4))
        n = p.shape[0]
        key = lambda g: (torch.repeat_interleave(torch.arange(n), (g.rowptr[1:] - g.rowptr[:-1]).long().cpu()) * n  # noqa: E731
                         + g.col.cpu().long())
        fk, ck = key(full), key(few)
        where = torch.searchsorted(fk, ck)
        assert torch.equal(fk[where], ck), "a capped row is not a subset of the uncapped row"
        assert torch.equal(full.d2.cpu()[where].view(torch.int32), few.d2.cpu().view(torch.int32))
        want = want_of(kc.knn_base(pos, 3, R, sizes, loop), 4)[0]
        assert torch.equal(few.rowptr.cpu(), want[3]) and torch.equal(few.col.cpu(), want[4])
    g = knn_graph(p, 9, gp)
    for lanes in (None,) + LANES:
        out = ops.pair_d2(g.rowptr, g.col, p, 3, lanes=lanes)
        assert torch.equal(out.view(torch.int32), g.d2.view(torch.int32))


def test_a_graph_keeps_its_rows_wherever_it_stands():
    sizes = [65, 9, 130, 33]
    pos = gg.grid_positions(sizes, 3, 3, seed=7, special=False)
    gp = gg.gptr_of(sizes)
    k = 9
    assert want_of(kc.knn_base(pos, 3, None, sizes, False), k)[1] > 0          # ids decide some rows
    _, _, tj, rp, col, d2 = run_knn(pos, 3, k, None, sizes, False)
    perm = [2, 0, 3, 1]
    pos2 = np.concatenate([pos[gp[q]:gp[q + 1]] for q in perm])
    sizes2 = [sizes[q] for q in perm]
    gp2 = gg.gptr_of(sizes2)
    _, _, tj2, rp2, col2, d22 = run_knn(pos2, 3, k, None, sizes2, False)
    for new, old in enumerate(perm):
        a0, a1 = int(rp[gp[old]]), int(rp[gp[old + 1]])
        b0, b1 = int(rp2[gp2[new]]), int(rp2[gp2[new + 1]])
        assert a1 - a0 == b1 - b0 and a1 > a0
        assert torch.equal(rp[gp[old]:gp[old + 1] + 1] - a0, rp2[gp2[new]:gp2[new + 1] + 1] - b0)
        assert torch.equal(col[a0:a1] - int(gp[old]), col2[b0:b1] - int(gp2[new]))
        assert torch.equal(tj[gp[old]:gp[old + 1]] - int(gp[old]), tj2[gp2[new]:gp2[new + 1]] - int(gp2[new]))
        assert torch.equal(d2[a0:a1].view(torch.int32), d22[b0:b1].view(torch.int32))


def test_two_runs_give_the_same_graph_and_the_api_returns_it():
    pos, base = reference(3, 3, False, R)
    want, _ = want_of(base, 3)
    p = torch.tensor(pos, device=DEV)
    a = knn_graph(p, 3, torch.tensor(gg.gptr_of(SIZES), device=DEV), r=R)
    b = knn_graph(p, 3, GraphBatch(torch.tensor(gg.gptr_of(SIZES))), r=R)
    for g in (a, b):
        assert g.rowptr.device.type == "cuda" and g.n_graphs == len(SIZES)
        assert torch.equal(g.rowptr.cpu(), want[3]) and torch.equal(g.col.cpu(), want[4])
        assert torch.equal(g.d2.cpu(), want[5]) and torch.equal(g.eperm.cpu(), torch.arange(want[4].numel()))


def test_select_cumsum_and_fill_replay_under_step_graph():
    sizes = [12, 40, 0, 33, 70]
    n, k = sum(sizes), 6
    gp, seg = batch_on_device(sizes)
    cap = n * k
    p = torch.zeros(n, 4, device=DEV)
    deg = torch.zeros(n, dtype=torch.int32, device=DEV)
    td = torch.zeros(n, device=DEV)
    tj = torch.zeros(n, dtype=torch.int32, device=DEV)
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    col = torch.zeros(cap, dtype=torch.int32, device=DEV)
    d2 = torch.zeros(cap, device=DEV)

    def inputs(seed):
        p.copy_(torch.tensor(gg.grid_positions(sizes, 3, 4, seed, special=False)))

    def step():
        ops.knn_select(p, 3, k, gp, seg, r=R, deg=deg, tau_d2=td, tau_j=tj)
        rowptr[1:] = torch.cumsum(deg, 0, dtype=torch.int32)
        ops.knn_fill(p, 3, gp, seg, rowptr, td, tj, out=col, d2=d2)

    bufs = (deg, td, tj, rowptr, col, d2)
    eager = []
    for seed in (31, 33):
        inputs(seed)
        for b in bufs:
            b.fill_(SENT)
        rowptr[0] = 0
        step()
        torch.cuda.synchronize()
        want = want_of(kc.knn_base(p.cpu().numpy(), 3, R, sizes, False), k)[0]
        nnz = int(rowptr[-1])
        assert_same((deg.cpu(), td.cpu(), tj.cpu(), rowptr.cpu(), col[:nnz].cpu(), d2[:nnz].cpu()), want)
        assert int(deg.max()) == k and int(deg.min()) < k and bool((col[nnz:] == SENT).all())
        eager.append([b.clone() for b in bufs])
    assert not torch.equal(eager[0][4], eager[1][4])
    inputs(35)
    sg = StepGraph(step, warmup=1, device=torch.device(DEV))
    sg()                                                   # eager warm-up
    for q, seed in enumerate((31, 33)):
        inputs(seed)
        for b in bufs:
            b.fill_(SENT)
        rowptr[0] = 0
        sg()
        assert sg.graph is not None
        torch.cuda.synchronize()
        for b, e in zip(bufs, eager[q]):
            assert torch.equal(b, e), "replay %d" % q


def test_empty_inputs():
    e = knn_graph(torch.zeros(0, 3, device=DEV), 4)
    assert e.n == 0 and e.col.numel() == 0 and e.rowptr.tolist() == [0]
    e = knn_graph(torch.zeros(0, 2, device=DEV), 4, torch.zeros(4, dtype=torch.int64))
    assert e.n_graphs == 3 and e.col.numel() == 0 and e.rowptr.tolist() == [0]
    e = radius_graph(torch.zeros(0, 2, device=DEV), 1.0, torch.zeros(4, dtype=torch.int64), max_num_neighbors=2)
    assert e.n_graphs == 3 and e.col.numel() == 0 and e.d2.numel() == 0
    pos = torch.tensor(gg.grid_positions([40, 9], 3, 3, seed=2, special=False), device=DEV)
    pos = torch.unique(pos, dim=0)                          # distinct points
    n = pos.shape[0]
    gp = torch.tensor([0, 5, n])
    g = knn_graph(pos, 4, gp, r=0.0)
    assert g.col.numel() == 0 and g.d2.numel() == 0 and g.rowptr.tolist() == [0] * (n + 1)
    deg, td, tj = ops.knn_select(pos, 3, 4, g.gptr, g.batch, r=0.0)
    assert bool((deg == 0).all()) and bool((td == -1).all()) and bool((tj == -1).all())
    assert knn_graph(pos, 4, gp, r=0.0, loop=True).col.tolist() == list(range(n))
    one = knn_graph(pos[:1], 4)                             # a single point has no neighbour
    assert one.rowptr.tolist() == [0, 0]
    p = pos.clone().requires_grad_(True)
    d = pair_distance(p, g)
    assert d.shape == (0,)
    d.sum().backward()
    assert bool((p.grad == 0).all())


@pytest.mark.parametrize("squared", [True, False])
def test_pair_distance_autograd_on_a_knn_graph_against_fp64(squared):
    """``pair_distance`` on the directed k-NN graph, random fp32 positions, with the bounds
    derived in test_gnn_geometry_gpu.test_pair_distance_autograd_against_fp64: forward
    ``6 u t`` (squared) / ``4 u d``; gradient ``8 deg u S`` per node and coordinate with
    ``S = 2 sum_e |g_e| |p_i - p_j|_1`` over the ``deg`` in- and out-edges.  The fp64 edge list
    is the GPU's ``col``.  Largest observed fraction of the bounds on an MI355X: forward 0.49
    (squared), 0.52 (distance); gradient 0.013 (squared), 0.016 (distance)."""
    torch.manual_seed(4)
    sizes = [30, 1, 64, 17]
    n = sum(sizes)
    pos = (torch.randn(n, 3) * 1.2).to(DEV)
    g = knn_graph(pos, 5, torch.tensor(gg.gptr_of(sizes)))
    nnz = g.col.numel()
    assert nnz == 5 * (n - 1)
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), (g.rowptr[1:] - g.rowptr[:-1]).long())
    cols = g.col.long()
    fwd = set((rows * n + cols).tolist())
    assert any((j * n + i) not in fwd for i, j in zip(rows.tolist(), cols.tolist())), "the graph is symmetric"
    wgt = torch.randn(nnz, device=DEV)
    p32 = pos.clone().requires_grad_(True)
    out = pair_distance(p32, g, squared=squared)
    (out * wgt).sum().backward()
    p64 = pos.double().requires_grad_(True)
    t = ((p64[rows] - p64[cols]) ** 2).sum(1)
    ref = t if squared else torch.sqrt(t)
    (ref * wgt.double()).sum().backward()
    err = (out.detach().double() - ref.detach()).abs()
    bound = (6 if squared else 4) * U * ref.detach()
    print("forward: largest fraction of the bound %.3f" % float((err / bound).max()))
    assert bool((err <= bound).all())
    ge = wgt.double() if squared else wgt.double() / (2 * ref.detach())
    mag = ge.abs() * (p64.detach()[rows] - p64.detach()[cols]).abs().sum(1)
    s = torch.zeros(n, dtype=torch.float64, device=DEV).index_add_(0, rows, mag).index_add_(0, cols, mag)
    deg = torch.zeros(n, dtype=torch.float64, device=DEV).index_add_(0, rows, torch.ones_like(mag))
    deg = deg.index_add_(0, cols, torch.ones_like(mag))
    gbound = 8 * deg * U * 2 * s
    gerr = (p32.grad.double() - p64.grad).abs().max(1).values
    has = deg > 0
    print("gradient: largest fraction of the bound %.3f" % float((gerr[has] / gbound[has]).max()))
    assert bool((gerr <= gbound).all())
    assert bool((p32.grad[~has] == 0).all())


def schnet_inputs(sizes, rc, k, seed=12):
    """Seeded positions, redrawn until, in every row, no pair sits within 1e-3 of the cutoff
    and the k-th and (k+1)-th candidate distances differ by at least 1e-3: the fp64 selection
    is then the fp32 selection.  Returns (pos fp64 [n, 3], rows, cols, largest radius degree)."""
    rng = np.random.default_rng(seed)
    n, G = sum(sizes), len(sizes)
    gp = gg.gptr_of(sizes)
    for _ in range(100):
        pos = rng.normal(size=(n, 3)) * 1.3
        pos = pos.astype(np.float32).astype(np.float64)
        rows, cols, margin, widest = [], [], np.inf, 0
        for q in range(G):
            p = pos[gp[q]:gp[q + 1]]
            s = sizes[q]
            d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(2))
            margin = min(margin, np.abs(d - rc).min())
            cand = (d <= rc) & ~np.eye(s, dtype=bool)
            key = np.where(cand, d, np.inf)
            order = np.argsort(key, axis=1, kind="stable")
            srt = np.take_along_axis(key, order, 1)
            cnt = cand.sum(1)
            widest = max(widest, int(cnt.max()))
            more = cnt > k                                       # rows the cap cuts
            if more.any():
                margin = min(margin, (srt[more, k] - srt[more, k - 1]).min())
            keep = np.zeros((s, s), dtype=bool)
            take = np.arange(s)[None, :] < np.minimum(cnt, k)[:, None]
            keep[np.repeat(np.arange(s), np.minimum(cnt, k)), order[take]] = True
            i, j = np.nonzero(keep)
            rows.append(i + gp[q])
            cols.append(j + gp[q])
        if margin >= 1e-3:
            break
    assert margin >= 1e-3
    return pos, torch.tensor(np.concatenate(rows)), torch.tensor(np.concatenate(cols)), widest


def test_schnet_with_a_neighbour_cap_end_to_end():
    """Energy and forces of the HIP path with ``max_num_neighbors`` against fp64 on the same
    (directed) edge list; allowed: 4x the error of a plain PyTorch fp32 evaluation of the same
    formula against that fp64, the rule of test_schnet_energy_and_forces_end_to_end.  Observed
    on an MI355X: energy error 1.43e-6, 1.86x that of the PyTorch fp32 evaluation (7.7e-7);
    force error 4.3e-7, 1.21x (3.5e-7)."""
    sizes = [3, 20, 7, 12, 5, 16]
    rc, k = 2.0, 4
    n, G = sum(sizes), len(sizes)
    pos, rows, cols, widest = schnet_inputs(sizes, rc, k)
    assert widest > k, "the cap does not bite"
    pairs = set((rows * n + cols).tolist())
    assert any((j * n + i) not in pairs for i, j in zip(rows.tolist(), cols.tolist())), "the graph is symmetric"
    assert rows.numel() > 100
    rng = np.random.default_rng(13)
    z = torch.tensor(rng.integers(1, 10, n))
    gid = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes))
    model = SchNet(hidden=32, n_filters=32, n_interactions=2, n_gaussians=16, cutoff=rc, max_num_neighbors=k,
                   generator=torch.Generator().manual_seed(8)).to(DEV)
    post = torch.tensor(pos, dtype=torch.float32)
    batch = GraphBatch(torch.tensor(gg.gptr_of(sizes))).to(DEV)
    g = model.neighbors(post.to(DEV), batch)
    grow = torch.repeat_interleave(torch.arange(n), (g.rowptr[1:] - g.rowptr[:-1]).long().cpu())
    assert torch.equal(grow, rows) and torch.equal(g.col.cpu().long(), cols)
    E, F = model.energy_and_forces(z.to(DEV), post.to(DEV), batch)
    E64, F64 = gg.schnet_formula(model, z, post, rows, cols, gid, G, torch.float64)
    E32, F32 = gg.schnet_formula(model, z, post, rows, cols, gid, G, torch.float32)
    assert float(F64.abs().max()) > 1e-3 and float(E64.abs().max()) > 1e-3
    eE, rE = (E.cpu().double() - E64).abs().max(), (E32.double() - E64).abs().max()
    eF, rF = (F.cpu().double() - F64).abs().max(), (F32.double() - F64).abs().max()
    print("SchNet, max_num_neighbors = %d: energy error %.3e (PyTorch fp32 %.3e, ratio %.2f), force error %.3e "
          "(PyTorch fp32 %.3e, ratio %.2f)" % (k, eE, rE, eE / rE, eF, rF, eF / rF))
    assert eE <= 4 * rE and eF <= 4 * rF
