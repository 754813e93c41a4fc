"""The CPU branches of the geometry ops (ops.radius_count / radius_fill / pair_d2 / pair_d2_bwd)
against numpy references computed here from the definitions, and the layers above them on the
CPU: radius_graph, pair_distance, GaussianSmearing, cosine_cutoff, SchNet.

The exact comparisons put every coordinate on multiples of 1/4 in [-8, 8]: every squared
distance is then a multiple of 1/16 below 2^10 and exact in fp32, and with integer ``g`` so is
every partial sum of the gradient.
"""
import math

import numpy as np
import pytest
import torch

from cgnn_amd.gnn import ops
from cgnn_amd.gnn.geometry import GaussianSmearing, cosine_cutoff, pair_distance, radius_graph
from cgnn_amd.gnn.layers import CFConv
from cgnn_amd.gnn.readout import GraphBatch, graph_readout
from cgnn_amd.gnn.schnet import SchNet

BIG = 1.0e4
R = 1.25                # r * r = 1.5625 exactly; the offset (0.75, 1, 0) sits on the boundary
NAN, INF = float("nan"), float("inf")
SIZES = [0, 1, 2, 9, 0, 33, 70, 0]


def grid_positions(sizes, D, ldp, seed, special=True):
    rng = np.random.default_rng(seed)
    pos = np.full((sum(sizes), ldp), BIG, dtype=np.float32)
    off = 0
    for s in sizes:
        p = rng.integers(-8, 9, size=(s, D)).astype(np.float32) / 4
        if s >= 8:
            step = np.array([0.75, 1.0, 0.0][:D] if D > 1 else [1.25], dtype=np.float32)
            p[1] = p[0] + step                      # on the boundary
            p[3] = p[2]                             # coincident
        if special and s == 70:
            p[50, 0] = NAN
            p[60, D - 1] = INF
        pos[off:off + s, :D] = p
        off += s
    return pos


def gptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def ref_radius(pos, D, r, sizes, loop):
    r2 = float(np.float32(r) * np.float32(r))
    rowptr, col, d2 = [0], [], []
    off = 0
    with np.errstate(invalid="ignore"):
        for s in sizes:
            p = pos[off:off + s, :D].astype(np.float64)
            for i in range(s):
                d = ((p[i] - p) ** 2).sum(1)
                keep = d <= r2
                if not loop:
                    keep[i] = False
                js = np.nonzero(keep)[0]
                col.append(js + off)
                d2.append(d[js])
                rowptr.append(rowptr[-1] + js.size)
            off += s
    return (torch.tensor(rowptr, dtype=torch.int32), torch.tensor(np.concatenate(col), dtype=torch.int32),
            torch.tensor(np.concatenate(d2)).float())


def batch_of(sizes):
    gp = torch.tensor(gptr_of(sizes), dtype=torch.int32)
    seg = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes))
    return gp, seg


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("D,ldp", [(1, 1), (2, 4), (3, 3), (3, 4)])
def test_radius_ops_cpu_branch(D, ldp, loop):
    pos = grid_positions(SIZES, D, ldp, seed=D)
    rowptr, col, d2 = ref_radius(pos, D, R, SIZES, loop)
    assert bool((d2 == 1.5625).any()) and bool((d2 == 0).any())
    gp, seg = batch_of(SIZES)
    p = torch.tensor(pos)
    deg = ops.radius_count(p, D, R, gp, seg, loop=loop)
    assert deg.dtype == torch.int32 and torch.equal(deg, rowptr[1:] - rowptr[:-1])
    off = int(gp[SIZES.index(70)])
    assert int(deg[off + 50]) == 0 and int(deg[off + 60]) == 0        # NaN, inf: no edges
    c, dd = ops.radius_fill(p, D, R, gp, seg, rowptr, loop=loop, with_d2=True)
    assert torch.equal(c, col) and torch.equal(dd, d2)
    out = torch.full((col.numel() + 4,), -7, dtype=torch.int32)
    c2, none = ops.radius_fill(p, D, R, gp, seg, rowptr, loop=loop, out=out)
    assert none is None and c2 is out and torch.equal(out[:col.numel()], col) and bool((out[col.numel():] == -7).all())


def directed_graph(n=40, m=300, seed=3):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n - 3, m)
    dst = (rng.integers(0, n - 3, m) ** 2) % (n - 3)
    return GraphBatch.from_graphs([(n, src, dst)])


@pytest.mark.parametrize("D,ldp", [(1, 2), (2, 2), (3, 4)])
def test_pair_ops_cpu_branch(D, ldp):
    g = directed_graph()
    n = g.n
    pos = grid_positions([n], D, ldp, seed=5, special=False)
    rows = np.repeat(np.arange(n), np.diff(g.rowptr.numpy()))
    col = g.col.numpy()
    p64 = pos[:, :D].astype(np.float64)
    want = ((p64[rows] - p64[col]) ** 2).sum(1)
    got = ops.pair_d2(g.rowptr, g.col, torch.tensor(pos), D)
    assert got.dtype == torch.float32 and torch.equal(got, torch.tensor(want).float())
    gv = np.random.default_rng(1).integers(-2, 3, col.size).astype(np.float32)
    w = gv[:, None] * (p64[rows] - p64[col])
    ref = np.zeros((n, D))
    np.add.at(ref, rows, w)
    np.add.at(ref, col, -w)
    rp_t, col_t, eperm_t = g.transposed_perm()
    out = torch.full((n, ldp), -7.0)
    ops.pair_d2_bwd(g.rowptr, g.col, rp_t, col_t, eperm_t, torch.tensor(pos), torch.tensor(gv), D, out=out)
    assert torch.equal(out[:, :D], torch.tensor(2 * ref).float())
    assert bool((out[:, D:] == 0).all()) and bool((out[n - 3:] == 0).all())


def test_radius_graph_feeds_readout_and_cfconv():
    sizes = [5, 0, 12, 30]
    pos = torch.tensor(grid_positions(sizes, 3, 3, seed=8, special=False))
    g = radius_graph(pos, R, torch.tensor(gptr_of(sizes)))
    rowptr, col, d2 = ref_radius(pos.numpy(), 3, R, sizes, False)
    assert isinstance(g, GraphBatch) and g.n == sum(sizes) and g.n_graphs == 4
    assert torch.equal(g.rowptr, rowptr) and torch.equal(g.col, col) and torch.equal(g.d2, d2)
    assert torch.equal(g.eperm, torch.arange(col.numel()))
    one = radius_graph(pos, R)                                        # one graph
    assert one.n_graphs == 1 and one.col.numel() >= col.numel()
    via = radius_graph(pos, R, GraphBatch(torch.tensor(gptr_of(sizes))), loop=True)
    assert via.col.numel() == col.numel() + sum(sizes)
    x = torch.randn(g.n, 6, generator=torch.Generator().manual_seed(0))
    y = graph_readout(x, g, "sum")
    want = torch.zeros(4, 6).index_add_(0, g.batch.long(), x)
    assert torch.allclose(y, want, atol=1e-5)
    d = pair_distance(pos, g)
    assert torch.equal(d, torch.sqrt(d2))
    conv = CFConv(6, 6, 8, 4, generator=torch.Generator().manual_seed(1))
    e = GaussianSmearing(0.0, R, 4)(d)
    out = conv(x, g, e, cutoff=cosine_cutoff(d, R))
    rows = torch.repeat_interleave(torch.arange(g.n), (rowptr[1:] - rowptr[:-1]).long())
    h = x @ conv.lin1.weight
    w = (torch.nn.functional.softplus(e @ conv.filter1.weight + conv.filter1.bias) - math.log(2.0)) \
        @ conv.filter2.weight + conv.filter2.bias
    agg = torch.zeros(g.n, 8).index_add_(0, rows, cosine_cutoff(d, R)[:, None] * h[col.long()] * w)
    assert torch.allclose(out, agg @ conv.lin2.weight + conv.lin2.bias, atol=1e-5)


@pytest.mark.parametrize("squared", [True, False])
def test_pair_distance_gradcheck(squared):
    torch.manual_seed(2)
    g = directed_graph(n=12, m=40)
    keep = g.col.long() != torch.repeat_interleave(torch.arange(12), (g.rowptr[1:] - g.rowptr[:-1]).long())
    assert bool(keep.any())
    pos = torch.randn(12, 3, dtype=torch.float64, requires_grad=True)
    if squared:
        assert torch.autograd.gradcheck(lambda p: pair_distance(p, g, squared=True), (pos,))
    else:                                           # away from the self loops, where d = 0
        assert torch.autograd.gradcheck(lambda p: pair_distance(p, g)[keep], (pos,))
    # the gradient of the distance is defined as 0 at d = 0
    loops = GraphBatch.from_graphs([(3, [0, 1, 2, 0], [0, 1, 2, 1])])
    p = torch.randn(3, 2, requires_grad=True)
    d = pair_distance(p, loops)
    d.sum().backward()
    assert torch.isfinite(p.grad).all() and bool((p.grad[2] == 0).all())
    with pytest.raises(RuntimeError):               # differentiable once
        q = torch.randn(3, 2, dtype=torch.float64, requires_grad=True)
        gq, = torch.autograd.grad(pair_distance(q, loops, squared=True).sum(), q, create_graph=True)
        gq.sum().backward()


def test_smearing_and_cutoff_closed_forms():
    d = torch.tensor([0.0, 0.3, 1.0, 2.5, 4.999, 5.0, 6.0], dtype=torch.float64, requires_grad=True)
    sm = GaussianSmearing(0.0, 5.0, 11)
    mu = np.linspace(0.0, 5.0, 11)
    out = sm(d)
    want = np.exp(-0.5 / 0.25 * (d.detach().numpy()[:, None] - mu[None, :]) ** 2)
    assert out.shape == (7, 11) and np.allclose(out.detach().numpy(), want, rtol=1e-6, atol=1e-12)
    out.sum().backward()
    dwant = (want * (-(d.detach().numpy()[:, None] - mu[None, :]) / 0.25)).sum(1)
    assert np.allclose(d.grad.numpy(), dwant, rtol=1e-6, atol=1e-9)
    assert sm(torch.rand(4)).dtype == torch.float32
    d.grad = None
    c = cosine_cutoff(d, 5.0)
    dn = d.detach().numpy()
    cw = np.where(dn < 5.0, 0.5 * (np.cos(np.pi * dn / 5.0) + 1), 0.0)
    cd = c.detach()
    assert np.allclose(cd.numpy(), cw, atol=1e-12) and float(cd[0]) == 1.0 and float(cd[5]) == 0 == float(cd[6])
    c.sum().backward()
    gw = np.where(dn < 5.0, -0.5 * np.pi / 5.0 * np.sin(np.pi * dn / 5.0), 0.0)
    assert np.allclose(d.grad.numpy(), gw, atol=1e-12)
    with pytest.raises(ValueError):
        GaussianSmearing(0.0, 5.0, 1)


def rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    return torch.tensor(q * np.sign(np.linalg.det(q)), dtype=torch.float32)


def test_schnet_invariances_cpu():
    rng = np.random.default_rng(3)
    sizes = [4, 11, 7, 16]
    n, G = sum(sizes), len(sizes)
    gp = gptr_of(sizes)
    pos = torch.tensor(rng.normal(size=(n, 3)) * 1.2, dtype=torch.float32)
    z = torch.tensor(rng.integers(1, 9, n))
    model = SchNet(hidden=16, n_filters=16, n_interactions=2, n_gaussians=8, cutoff=2.0,
                   generator=torch.Generator().manual_seed(5))
    E, F = model.energy_and_forces(z, pos, torch.tensor(gp))
    assert E.shape == (G,) and F.shape == (n, 3) and float(F.abs().max()) > 1e-4
    assert not any(p.grad is not None for p in model.parameters())
    # the forces of a graph sum to zero (translation invariance)
    tot = torch.zeros(G, 3).index_add_(0, torch.repeat_interleave(torch.arange(G), torch.tensor(sizes)), F)
    assert float(tot.abs().max()) < 1e-4
    Q = rotation(1)
    E2, F2 = model.energy_and_forces(z, pos @ Q.t() + torch.tensor([0.5, -1.0, 2.0]), torch.tensor(gp))
    assert torch.allclose(E2, E, atol=2e-4, rtol=1e-4)
    assert torch.allclose(F2, F @ Q.t(), atol=2e-4, rtol=1e-3)
    perm = [2, 0, 3, 1]
    idx = torch.cat([torch.arange(gp[k], gp[k + 1]) for k in perm])
    E3, F3 = model.energy_and_forces(z[idx], pos[idx], torch.tensor(gptr_of([sizes[k] for k in perm])))
    assert torch.allclose(E3, E[perm], atol=1e-5) and torch.allclose(F3, F[idx], atol=1e-5)
    # a reused neighbour list gives the same bits
    g = model.neighbors(pos, torch.tensor(gp))
    E4, F4 = model.energy_and_forces(z, pos, graph=g)
    assert torch.equal(E4, E) and torch.equal(F4, F)


def test_argument_errors():
    pos = torch.zeros(6, 3)
    gp, seg = batch_of([2, 4])
    with pytest.raises(ValueError):
        radius_graph(torch.zeros(6, 4), 1.0)                           # D = 4
    with pytest.raises(ValueError):
        ops.radius_count(torch.zeros(6, 4), 4, 1.0, gp, seg)
    with pytest.raises(ValueError):
        ops.radius_count(pos, 0, 1.0, gp, seg)
    with pytest.raises(TypeError):
        radius_graph(pos.long(), 1.0)
    with pytest.raises(TypeError):
        radius_graph(pos, 1.0, torch.tensor([0.0, 6.0]))
    with pytest.raises(TypeError):
        radius_graph(pos, 1.0, [0, 6])
    for r in (-1.0, NAN, INF):
        with pytest.raises(ValueError):
            radius_graph(pos, r)
        with pytest.raises(ValueError):
            ops.radius_fill(pos, 3, r, gp, seg, torch.zeros(7, dtype=torch.int32))
    with pytest.raises(ValueError):
        radius_graph(pos, 1.0, torch.tensor([0, 2, 5]))                # gptr does not match pos
    with pytest.raises(ValueError):
        radius_graph(pos, 1.0, GraphBatch(torch.tensor([0, 7])))
    with pytest.raises(ValueError):
        ops.radius_count(pos, 3, 1.0, gp, seg[:5])
    with pytest.raises(ValueError):
        ops.radius_count(pos, 3, 1.0, gp, seg, lanes=12)
    with pytest.raises(ValueError):
        ops.radius_fill(pos, 3, 1.0, gp, seg, torch.zeros(6, dtype=torch.int32))
    g = radius_graph(pos, 1.0, gp)
    with pytest.raises(ValueError):
        pair_distance(torch.zeros(5, 3), g)
    with pytest.raises(ValueError):
        ops.pair_d2(g.rowptr, g.col, pos, 4)
    with pytest.raises(ValueError):
        ops.pair_d2_bwd(g.rowptr, g.col, *g.transposed_perm(), pos, torch.zeros(3), 3)
    with pytest.raises(ValueError):
        SchNet(8, 8, 1, 4, 2.0)(torch.zeros(5, dtype=torch.long), pos)
