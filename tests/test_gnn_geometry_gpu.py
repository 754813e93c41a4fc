"""The geometry kernels on the GPU (gnn_geometry.hip) against numpy / fp64 references computed
here from the definitions -- never through the CPU branches of ``ops`` -- and SchNet end to
end against an fp64 evaluation of the same parameters.

Exactness.  The exact tests put every coordinate on multiples of 1/4 in [-8, 8].  A difference
is then a multiple of 1/4 of magnitude <= 16, a squared distance a multiple of 1/16 below
3 * 256 < 2^10: 14 significant bits at most, exact in fp32 whatever the contraction, so the
edge sets, ``d2`` and (with integer ``g``) every partial sum of the gradient are compared with
``torch.equal``.
"""
import math

import numpy as np
import pytest
import torch

from cgnn_amd.gnn import ops
from cgnn_amd.gnn.geometry import pair_distance, radius_graph
from cgnn_amd.gnn.readout import GraphBatch
from cgnn_amd.gnn.schnet import SchNet
from cgnn_amd.utils.hipgraph import StepGraph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -7               # sentinel of rows / tails a kernel must not write
BIG = 1.0e4             # fills the padding columns of pos: must never reach a result
R = 1.25                # r * r = 1.5625 exactly; the offset (0.75, 1, 0) sits on the boundary
LANES = (8, 16, 32, 64)
U = 2.0 ** -24          # fp32 unit roundoff
NAN, INF = float("nan"), float("inf")

# empty graphs first, in the middle and last
SIZES = [0, 0, 1, 2, 3, 7, 8, 9, 0, 63, 64, 65, 127, 128, 129, 0, 200, 600, 0]


def half_width(s):
    return 2 if s <= 129 else (4 if s <= 200 else 6)


def grid_positions(sizes, D, ldp, seed, special=True):
    """fp32 ``[n, ldp]`` on the 1/4 grid, the padding columns BIG.  Planted in every graph of
    at least 8 points: a pair exactly on the boundary and a coincident pair; with ``special``
    one NaN and one inf coordinate in the graph of 200 points."""
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    pos = np.full((n, ldp), BIG, dtype=np.float32)
    off = 0
    for s in sizes:
        w = half_width(s)
        p = rng.integers(-4 * w, 4 * w + 1, size=(s, D)).astype(np.float32) / 4
        if s >= 8:
            step = np.array([0.75, 1.0, 0.0][:D] if D > 1 else [1.25], dtype=np.float32)
            p[1] = p[0] + step                      # on the boundary: d2 = r * r
            p[s - 1] = p[0] - step
            p[3] = p[2]                             # coincident
        if special and s == 200:
            p[50, 0] = NAN
            p[60, D - 1] = INF
        pos[off:off + s, :D] = p
        off += s
    finite = pos[:, :D][np.isfinite(pos[:, :D])]
    assert np.all(finite * 4 == np.round(finite * 4)) and np.abs(finite).max() <= 8
    return pos


def gptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def ref_radius(pos, D, r, sizes, loop):
    """(rowptr, col, d2) by brute force per graph in fp64, ascending ids."""
    r2 = float(np.float32(r) * np.float32(r))
    rowptr, col, d2 = [0], [], []
    off = 0
    with np.errstate(invalid="ignore"):
        for s in sizes:
            p = pos[off:off + s, :D].astype(np.float64)
            for i in range(s):
                d = ((p[i] - p) ** 2).sum(1)
                fin = d[np.isfinite(d)]             # every candidate's d2 is exact in fp32
                assert fin.size == 0 or (fin.max() < 2 ** 10 and np.all(fin * 16 == np.round(fin * 16)))
                keep = d <= r2                      # False for NaN
                if not loop:
                    keep[i] = False
                js = np.nonzero(keep)[0]
                col.append(js + off)
                d2.append(d[js])
                rowptr.append(rowptr[-1] + js.size)
            off += s
    col = np.concatenate(col) if col else np.zeros(0)
    d2 = np.concatenate(d2) if d2 else np.zeros(0)
    return (torch.tensor(rowptr, dtype=torch.int32), torch.tensor(col, dtype=torch.int32),
            torch.tensor(d2, dtype=torch.float64).float())


def run_search(pos, D, r, sizes, loop, lanes=None, tail=5):
    """(deg, rowptr, col, d2) from the two passes with sentinel rows and tails, checked."""
    n = pos.shape[0]
    gp = torch.tensor(gptr_of(sizes), dtype=torch.int32, device=DEV)
    seg = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes)).to(DEV)
    p = torch.tensor(pos, device=DEV)
    deg = torch.full((n + tail,), SENT, dtype=torch.int32, device=DEV)
    ops.radius_count(p, D, r, gp, seg, loop=loop, lanes=lanes, out=deg)
    assert bool((deg[n:] == SENT).all()), "count wrote past its rows"
    rp = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    rp[1:] = torch.cumsum(deg[:n], 0, dtype=torch.int64)
    nnz = int(rp[-1])
    col = torch.full((nnz + tail,), SENT, dtype=torch.int32, device=DEV)
    d2 = torch.full((nnz + tail,), float(SENT), dtype=torch.float32, device=DEV)
    ops.radius_fill(p, D, r, gp, seg, rp.to(torch.int32), loop=loop, lanes=lanes, out=col, d2=d2)
    assert bool((col[nnz:] == SENT).all()) and bool((d2[nnz:] == SENT).all()), "fill wrote past nnz"
    return deg[:n].cpu(), rp.to(torch.int32).cpu(), col[:nnz].cpu(), d2[:nnz].cpu()


_REF = {}


def reference(D, ldp, loop):
    key = (D, ldp, loop)
    if key not in _REF:
        pos = grid_positions(SIZES, D, ldp, seed=100 + D)
        _REF[key] = (pos,) + ref_radius(pos, D, R, SIZES, loop)
    return _REF[key]


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("D,ldp", [(1, 1), (1, 4), (2, 2), (2, 4), (3, 3), (3, 4)])
def test_radius_graph_exact_edge_sets(D, ldp, loop):
    pos, rowptr, col, d2 = reference(D, ldp, loop)
    assert bool((d2 == np.float32(R) * np.float32(R)).any()), "no pair on the boundary"
    assert bool((d2 == 0).any()), "no coincident pair"
    deg, rp, c, dd = run_search(pos, D, R, SIZES, loop)
    assert torch.equal(rp, rowptr)
    assert torch.equal(deg, rowptr[1:] - rowptr[:-1])
    assert torch.equal(c, col)
    assert torch.equal(dd, d2)
    # the NaN point has no edge at all; the inf point none either (inf - inf is NaN)
    off = int(gptr_of(SIZES)[SIZES.index(200)])
    assert int(deg[off + 50]) == 0 and int(deg[off + 60]) == 0


@pytest.mark.parametrize("lanes", LANES)
def test_every_compiled_lanes_value_gives_the_same_csr(lanes):
    pos, rowptr, col, d2 = reference(3, 4, False)
    _, rp, c, dd = run_search(pos, 3, R, SIZES, False, lanes=lanes)
    assert torch.equal(rp, rowptr) and torch.equal(c, col) and torch.equal(dd, d2)


def test_two_runs_give_the_same_csr_and_the_api_returns_it():
    pos, rowptr, col, d2 = reference(3, 3, False)
    p = torch.tensor(pos, device=DEV)
    gp = torch.tensor(gptr_of(SIZES), device=DEV)
    a = radius_graph(p, R, gp)
    b = radius_graph(p, R, GraphBatch(torch.tensor(gptr_of(SIZES))))
    for g in (a, b):
        assert g.rowptr.device.type == "cuda" and g.n_graphs == len(SIZES)
        assert torch.equal(g.rowptr.cpu(), rowptr) and torch.equal(g.col.cpu(), col) and torch.equal(g.d2.cpu(), d2)
        assert torch.equal(g.eperm.cpu(), torch.arange(col.numel()))


def test_a_graph_keeps_its_edges_wherever_it_stands():
    sizes = [65, 9, 130, 33]
    pos = grid_positions(sizes, 3, 3, seed=7, special=False)
    gp = gptr_of(sizes)
    _, rp, col, d2 = run_search(pos, 3, R, sizes, False)
    perm = [2, 0, 3, 1]
    pos2 = np.concatenate([pos[gp[k]:gp[k + 1]] for k in perm])
    sizes2 = [sizes[k] for k in perm]
    gp2 = gptr_of(sizes2)
    _, rp2, col2, d22 = run_search(pos2, 3, R, sizes2, False)
    for new, old in enumerate(perm):
        a0, a1 = int(rp[gp[old]]), int(rp[gp[old + 1]])
        b0, b1 = int(rp2[gp2[new]]), int(rp2[gp2[new + 1]])
        assert a1 - a0 == b1 - b0 and a1 > a0
        assert torch.equal(rp[gp[old]:gp[old + 1] + 1] - a0, rp2[gp2[new]:gp2[new + 1] + 1] - b0)
        assert torch.equal(col[a0:a1] - int(gp[old]), col2[b0:b1] - int(gp2[new]))
        assert torch.equal(d2[a0:a1].view(torch.int32), d22[b0:b1].view(torch.int32))


# ---------------------------------------------------------------- pair_d2

def multigraph(seed=3):
    """A directed multigraph of three components through ``GraphBatch.from_graphs``: repeated
    edges, self loops, in-degrees that differ from the out-degrees."""
    rng = np.random.default_rng(seed)
    graphs = []
    for s, m in ((5, 12), (0, 0), (40, 300), (9, 4)):
        src = rng.integers(0, max(s, 1), m)
        dst = (rng.integers(0, max(s, 1), m) ** 2) % max(s, 1)         # skewed in-degrees
        graphs.append((s, src, dst))
    return GraphBatch.from_graphs(graphs)


@pytest.mark.parametrize("D,ldp", [(1, 4), (2, 2), (3, 3), (3, 4)])
def test_pair_d2_reproduces_the_fill_pass_bit_for_bit(D, ldp):
    pos, rowptr, col, d2 = reference(D, ldp, False)
    p = torch.tensor(pos, device=DEV)
    for lanes in (None,) + LANES:
        out = torch.full((col.numel() + 3,), float(SENT), device=DEV)
        ops.pair_d2(rowptr.to(DEV), col.to(DEV), p, D, out=out, lanes=lanes, nnz=col.numel())
        # NaN-free: the NaN / inf points have no edges
        assert torch.equal(out[:col.numel()].cpu().view(torch.int32), d2.view(torch.int32))
        assert bool((out[col.numel():] == SENT).all())


def test_pair_d2_on_a_directed_multigraph_equals_fp64():
    g = multigraph()
    pos = grid_positions([g.n], 3, 4, seed=11, special=False)
    rows = np.repeat(np.arange(g.n), np.diff(g.rowptr.numpy()))
    diff = pos[rows, :3].astype(np.float64) - pos[g.col.numpy(), :3].astype(np.float64)
    want = torch.tensor((diff ** 2).sum(1)).float()
    gd = g.to(DEV)
    got = ops.pair_d2(gd.rowptr, gd.col, torch.tensor(pos, device=DEV), 3)
    assert torch.equal(got.cpu(), want)


# ---------------------------------------------------------------- pair_d2_bwd

def ref_bwd(pos, D, rowptr, col, g):
    """fp64 dpos from the definition."""
    n = pos.shape[0]
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    p = pos[:, :D].astype(np.float64)
    w = g[:, None].astype(np.float64) * (p[rows] - p[col])
    out = np.zeros((n, D))
    np.add.at(out, rows, w)
    np.add.at(out, col, -w)
    return 2 * out


def hub_graph(n, seed, lanes_probe=LANES):
    """A directed graph on ``n`` nodes: in-degrees 0, 1, L - 1, L, L + 1 for every sub-group
    width L, a hub with a few hundred in-edges and another with a few hundred out-edges; the
    last five nodes have no edge."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    node = 2                                                 # nodes 0 and 1 stay without in-edges
    degs = [1] + [L + k for L in lanes_probe for k in (-1, 0, 1)]
    for d in degs:
        src += list(rng.integers(0, n - 5, d))
        dst += [node] * d
        node += 1
    src += list(rng.integers(0, n - 5, 300))                      # hub of in-edges
    dst += [node] * 300
    dst += list(rng.integers(2, n - 5, 400))                      # hub of out-edges
    src += [node + 1] * 400
    return GraphBatch.from_graphs([(n, np.array(src), np.array(dst))])


@pytest.mark.parametrize("D,ldp", [(1, 1), (2, 4), (3, 3), (3, 4)])
def test_pair_d2_bwd_exact(D, ldp):
    n = 160
    g = hub_graph(n, seed=D)
    deg_in = np.diff(g.rowptr.numpy())
    deg_out = np.bincount(g.col.numpy(), minlength=n)
    assert deg_in.min() == 0 and deg_in.max() >= 300 and deg_out.max() >= 400 and (deg_in != deg_out).any()
    pos = grid_positions([n], D, ldp, seed=21 + D, special=False)
    rng = np.random.default_rng(9)
    gv = rng.integers(-2, 3, g.col.numel()).astype(np.float32)
    want = ref_bwd(pos, D, g.rowptr.numpy(), g.col.numpy(), gv)
    # |g| <= 2, |difference| <= 16, multiples of 1/4: any partial sum of the at most
    # deg_in + deg_out terms is a multiple of 1/4 below 32 * 1024 = 2^15, exact in fp32
    assert (deg_in + deg_out).max() <= 1024 and np.abs(want).max() < 2 ** 17
    gd = g.to(DEV)
    rp_t, col_t, eperm_t = gd.transposed_perm()
    p = torch.tensor(pos, device=DEV)
    for lanes in (None,) + LANES:
        out = torch.full((n, ldp), float(SENT), device=DEV)
        ops.pair_d2_bwd(gd.rowptr, gd.col, rp_t, col_t, eperm_t, p, torch.tensor(gv, device=DEV), D, out=out,
                        lanes=lanes)
        assert torch.equal(out[:, :D].cpu(), torch.tensor(want).float()), "lanes %s" % lanes
        assert bool((out[:, D:] == 0).all()), "padding columns"
    iso = np.nonzero((deg_in == 0) & (deg_out == 0))[0]
    assert iso.size >= 5                                      # a node without edges gets 0
    assert bool((out[torch.tensor(iso, device=DEV)] == 0).all())


# ---------------------------------------------------------------- autograd

@pytest.mark.parametrize("squared", [True, False])
def test_pair_distance_autograd_against_fp64(squared):
    """Forward bound.  d2 is three subtractions, one product and two fmas.  A difference
    carries one rounding, which enters its square twice; the square of dx then passes three
    roundings (the product and two fmas), that of dy two, that of dz one.  All terms are
    positive, so |d2 - t| <= (5 u + O(u^2)) t for the exact t: 6 u t is asserted.  The square
    root halves that relative error and adds one rounding: 3.5 u, asserted as 4 u d.
    Gradient bound.  A term g_e (p_i - p_j) carries the rounding of the difference (1), of its
    fma (1) and, for the distance, of the incoming g = gd / (2 d) (3.5 for d, 1 for the
    division): at most 7 u relative; the sum of a node's deg terms adds at most deg roundings.
    Per node and coordinate: (7 + deg) u S <= 8 deg u S with S = 2 sum_e |g_e| |p_i - p_j|_1
    over the deg in- and out-edges.  Largest observed fraction of the bounds on an MI355X:
    forward 0.49 (squared), 0.52 (distance); gradient 0.017 (squared), 0.048 (distance)."""
    torch.manual_seed(4)
    sizes = [30, 1, 64, 17]
    n = sum(sizes)
    pos = (torch.randn(n, 3) * 1.2).to(DEV)
    g = radius_graph(pos, 1.7, torch.tensor(gptr_of(sizes)))
    nnz = g.col.numel()
    assert nnz > 200
    wgt = torch.randn(nnz, device=DEV)
    p32 = pos.clone().requires_grad_(True)
    out = pair_distance(p32, g, squared=squared)
    (out * wgt).sum().backward()
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), (g.rowptr[1:] - g.rowptr[:-1]).long())
    cols = g.col.long()
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


# ---------------------------------------------------------------- capture

def test_search_and_pair_ops_replay_under_step_graph():
    sizes = [12, 40, 0, 33, 70]
    n = sum(sizes)
    gp = torch.tensor(gptr_of(sizes), dtype=torch.int32, device=DEV)
    seg = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes)).to(DEV)
    cap = 20000
    p = torch.zeros(n, 4, device=DEV)
    gv = torch.zeros(cap, device=DEV)
    deg = torch.zeros(n, dtype=torch.int32, device=DEV)
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    col = torch.zeros(cap, dtype=torch.int32, device=DEV)
    d2 = torch.zeros(cap, device=DEV)
    d2b = torch.zeros(cap, device=DEV)
    dpos = torch.zeros(n, 4, device=DEV)
    # a fixed bond graph for the gradient: the transposed CSR is built outside the capture
    bond = radius_graph(torch.tensor(grid_positions(sizes, 3, 3, 1, special=False), device=DEV), R, gp)
    rp_t, col_t, eperm_t = bond.transposed_perm()

    def inputs(seed):
        p.copy_(torch.tensor(grid_positions(sizes, 3, 4, seed, special=False)))
        gv.copy_(torch.randint(-2, 3, (cap,), generator=torch.Generator().manual_seed(seed)).float())

    def step():
        ops.radius_count(p, 3, R, gp, seg, out=deg)
        rowptr[1:] = torch.cumsum(deg, 0, dtype=torch.int32)
        ops.radius_fill(p, 3, R, gp, seg, rowptr, out=col, d2=d2)
        ops.pair_d2(bond.rowptr, bond.col, p, 3, out=d2b)
        ops.pair_d2_bwd(bond.rowptr, bond.col, rp_t, col_t, eperm_t, p, gv, 3, out=dpos, nnz=bond.col.numel())

    bufs = (deg, rowptr, col, d2, d2b, dpos)
    eager = []
    for seed in (31, 33):
        inputs(seed)
        for b in bufs:
            b.fill_(SENT)
        rowptr[0] = 0
        step()
        torch.cuda.synchronize()
        assert int(rowptr[-1]) < cap
        eager.append([b.clone() for b in bufs])
    assert not torch.equal(eager[0][2], eager[1][2])
    inputs(35)
    sg = StepGraph(step, warmup=1, device=torch.device(DEV))
    sg()                                                   # eager warm-up
    for k, seed in enumerate((31, 33)):
        inputs(seed)
        for b in bufs:
            b.fill_(SENT)
        rowptr[0] = 0
        sg()
        assert sg.graph is not None
        torch.cuda.synchronize()
        for b, e in zip(bufs, eager[k]):
            assert torch.equal(b, e), "replay %d" % k


# ---------------------------------------------------------------- empty inputs

def test_empty_inputs():
    e = radius_graph(torch.zeros(0, 3, device=DEV), 1.0)
    assert e.n == 0 and e.col.numel() == 0 and e.rowptr.tolist() == [0]
    e = radius_graph(torch.zeros(0, 2, device=DEV), 1.0, torch.zeros(4, dtype=torch.int64))
    assert e.n_graphs == 3 and e.col.numel() == 0 and e.rowptr.tolist() == [0]
    pos = torch.tensor(grid_positions([40, 9], 3, 3, seed=2, special=False), device=DEV)
    pos = torch.unique(pos, dim=0)                          # distinct points
    n = pos.shape[0]
    g = radius_graph(pos, 0.0, torch.tensor([0, 5, n]))
    assert g.col.numel() == 0 and g.d2.numel() == 0 and g.rowptr.tolist() == [0] * (n + 1)
    assert radius_graph(pos, 0.0, torch.tensor([0, 5, n]), loop=True).col.tolist() == list(range(n))
    p = pos.clone().requires_grad_(True)
    d = pair_distance(p, g)
    assert d.shape == (0,)
    d.sum().backward()
    assert bool((p.grad == 0).all())


# ---------------------------------------------------------------- SchNet end to end

def ssp(x):
    return torch.nn.functional.softplus(x) - math.log(2.0)


def schnet_formula(model, z, pos, rows, cols, gid, G, dtype):
    """The model written with plain indexing and index_add, in ``dtype``, on the CPU:
    (E [G], F [n, 3])."""
    P = {k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items()}
    p = pos.detach().cpu().to(dtype).requires_grad_(True)
    rc = model.cutoff
    d = torch.sqrt(((p[rows] - p[cols]) ** 2).sum(1))
    mu = P["smearing.offset"]
    delta = rc / (mu.numel() - 1)
    e = torch.exp(-0.5 / delta ** 2 * (d[:, None] - mu[None, :]) ** 2)
    c = torch.where(d < rc, 0.5 * (torch.cos(d * (math.pi / rc)) + 1), torch.zeros_like(d))
    x = P["embedding"][z.cpu()]
    for t in range(len(model.interactions)):
        k = "interactions.%d." % t
        h = x @ P[k + "conv.lin1.weight"]
        w = ssp(e @ P[k + "conv.filter1.weight"] + P[k + "conv.filter1.bias"]) @ P[k + "conv.filter2.weight"] \
            + P[k + "conv.filter2.bias"]
        m = c[:, None] * h[cols] * w
        agg = torch.zeros_like(h).index_add(0, rows, m)
        v = agg @ P[k + "conv.lin2.weight"] + P[k + "conv.lin2.bias"]
        x = x + ssp(v) @ P[k + "dense.weight"] + P[k + "dense.bias"]
    y = ssp(x @ P["out1.weight"] + P["out1.bias"]) @ P["out2.weight"] + P["out2.bias"]
    E = torch.zeros(G, dtype=dtype).index_add(0, gid, y[:, 0])
    F, = torch.autograd.grad(E.sum(), p)
    return E.detach(), -F


def test_schnet_energy_and_forces_end_to_end():
    """Energy and forces of the HIP path against fp64; allowed: 4x the error of a plain
    PyTorch fp32 evaluation of the same formula against that fp64 (both are fp32 evaluations
    that differ in summation order and fused contractions only).  Observed on an MI355X:
    energy error 1.5e-6, 2.82x that of the PyTorch fp32 evaluation (5.3e-7); force error
    6.6e-7, 0.96x (7.0e-7)."""
    rng = np.random.default_rng(12)
    sizes = [3, 20, 7, 12, 5, 16]
    rc = 2.0
    n, G = sum(sizes), len(sizes)
    gp = gptr_of(sizes)
    # seeded positions, redrawn until no pair sits within 1e-3 of the cutoff
    for _ in range(100):
        pos = rng.normal(size=(n, 3)) * 1.3
        pos = pos.astype(np.float32).astype(np.float64)
        rows, cols, margin = [], [], np.inf
        for k in range(G):
            p = pos[gp[k]:gp[k + 1]]
            d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(2))
            margin = min(margin, np.abs(d - rc).min())
            i, j = np.nonzero((d <= rc) & ~np.eye(sizes[k], dtype=bool))
            rows.append(i + gp[k])
            cols.append(j + gp[k])
        if margin >= 1e-3:
            break
    assert margin >= 1e-3
    rows, cols = torch.tensor(np.concatenate(rows)), torch.tensor(np.concatenate(cols))
    assert rows.numel() > 100
    z = torch.tensor(rng.integers(1, 10, n))
    gid = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes))
    model = SchNet(hidden=32, n_filters=32, n_interactions=2, n_gaussians=16, cutoff=rc,
                   generator=torch.Generator().manual_seed(8)).to(DEV)
    post = torch.tensor(pos, dtype=torch.float32)
    batch = GraphBatch(torch.tensor(gp)).to(DEV)
    g = model.neighbors(post.to(DEV), batch)
    grow = torch.repeat_interleave(torch.arange(n), (g.rowptr[1:] - g.rowptr[:-1]).long().cpu())
    assert torch.equal(grow, rows) and torch.equal(g.col.cpu().long(), cols)
    E, F = model.energy_and_forces(z.to(DEV), post.to(DEV), batch)
    E64, F64 = schnet_formula(model, z, post, rows, cols, gid, G, torch.float64)
    E32, F32 = schnet_formula(model, z, post, rows, cols, gid, G, torch.float32)
    assert float(F64.abs().max()) > 1e-3 and float(E64.abs().max()) > 1e-3
    eE, rE = (E.cpu().double() - E64).abs().max(), (E32.double() - E64).abs().max()
    eF, rF = (F.cpu().double() - F64).abs().max(), (F32.double() - F64).abs().max()
    print("SchNet: energy error %.3e (PyTorch fp32 %.3e, ratio %.2f), force error %.3e (PyTorch fp32 %.3e, "
          "ratio %.2f)" % (eE, rE, eE / rE, eF, rF, eF / rF))
    assert eE <= 4 * rE and eF <= 4 * rF
