"""Edge features without a GPU: the CPU branches of ``ops.espmm`` / ``ops.egrad`` against a
reference written here from dense fp64 index ops, ``torch.autograd.gradcheck`` of
``edge_aggregate`` in fp64, and the shapes / initialisation of ``GINEConv`` and ``CFConv``."""
import math

import numpy as np
import pytest
import torch

from cgnn_amd.gnn import ops
from cgnn_amd.gnn.layers import CFConv, GINEConv, NormGraph, WeightedGraph, edge_aggregate

F64 = torch.float64


def _graph(n=11, n_src=17, seed=0):
    """A rectangular CSR with an empty row, a row repeating one source and a long row."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 6, n)
    deg[2], deg[5] = 0, 9
    rp = torch.from_numpy(np.concatenate([[0], np.cumsum(deg)]).astype(np.int32))
    col = torch.from_numpy(rng.integers(0, n_src, int(rp[-1])).astype(np.int32))
    col[int(rp[5]):int(rp[6])] = 3
    return rp, col


def _rows(rp):
    return torch.repeat_interleave(torch.arange(rp.numel() - 1), (rp[1:] - rp[:-1]).long())


def _ref(rp, col, X, E, op, relu, val):
    """(Y, dE, dval, dX) for the cotangent G, computed edge by edge in fp64 on dense
    (destination, edge) incidence products."""
    n, nnz = rp.numel() - 1, col.numel()
    S = torch.zeros(n, nnz, dtype=F64)
    S[_rows(rp), torch.arange(nnz)] = 1                       # destination x edge incidence
    x = X.double()[col.long()] if X is not None else None
    e = E.double()
    if X is None:
        m = e
    elif op == "mul":
        m = x * e
    else:
        m = (x + e).clamp_min(0) if relu else x + e
    w = val.double() if val is not None else torch.ones(nnz, dtype=F64)
    return S @ (w[:, None] * m), S, m, w, x


@pytest.mark.parametrize("dt", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("op,relu,with_x", [("add", False, True), ("add", True, True), ("mul", False, True),
                                            ("add", False, False)])
@pytest.mark.parametrize("with_val", [False, True])
def test_ops_cpu_branches_against_dense_fp64(dt, op, relu, with_x, with_val):
    rp, col = _graph()
    n, nnz, n_src, F, ld = rp.numel() - 1, col.numel(), 17, 5, 8
    rng = np.random.default_rng(1)
    ints = lambda *s: torch.from_numpy(rng.integers(-3, 4, s).astype(np.float64))
    X = torch.full((n_src, ld), 5.0, dtype=F64)
    E = torch.full((nnz, ld), 5.0, dtype=F64)
    G = torch.zeros(n, ld, dtype=F64)
    X[:, :F], E[:, :F], G[:, :F] = ints(n_src, F), ints(nnz, F), ints(n, F)
    val = torch.from_numpy(rng.choice([-2.0, -0.5, 0.0, 0.25, 1.0], nnz)) if with_val else None
    at = F64 if dt == F64 else torch.float32
    Xt = X.to(dt) if with_x else None
    vt = val.to(at) if with_val else None
    yr, S, m, w, x = _ref(rp, col, X[:, :F] if with_x else None, E[:, :F], op, relu, val)
    # small integers and quarter weights: exact in every type used here
    out = torch.full((n + 2, ld), 7.0, dtype=dt)
    ops.espmm(rp, col, Xt, E.to(dt), F, op=op, relu=relu, val=vt, out=out[:n])
    assert torch.equal(out[:n, :F].double(), yr)
    assert torch.all(out[:n, F:] == 0) and torch.all(out[n:] == 7.0)
    # the same through a shuffled edge storage
    perm = torch.from_numpy(np.random.default_rng(2).permutation(nnz)).to(torch.int32)
    Es = torch.empty_like(E)
    Es[perm.long()] = E
    vs = None
    if with_val:
        vs = torch.empty_like(vt)
        vs[perm.long()] = vt
    y2 = ops.espmm(rp, col, Xt, Es.to(dt), F, op=op, relu=relu, val=vs, eperm=perm)
    assert torch.equal(y2[:, :F].double(), yr)
    # the edge gradients
    g = G[_rows(rp), :F]
    if not with_x:
        d = torch.ones_like(m)
    elif op == "mul":
        d = x
    else:
        d = ((x + E[:, :F]) > 0).double() if relu else torch.ones_like(m)
    dE, dval = ops.egrad(rp, col, G.to(dt), Xt, E.to(dt), F, op=op, relu=relu, val=vt, want_dval=True)
    assert dval.dtype == at
    assert torch.equal(dE[:, :F].double(), w[:, None] * g * d) and torch.all(dE[:, F:] == 0)
    assert torch.equal(dval.double(), (g * m).sum(1))
    only_de, none = ops.egrad(rp, col, G.to(dt), Xt, E.to(dt), F, op=op, relu=relu, val=vt)
    assert none is None and torch.equal(only_de, dE)
    none, only_dv = ops.egrad(rp, col, G.to(dt), Xt, E.to(dt), F, op=op, relu=relu, val=vt, want_dE=False,
                              want_dval=True)
    assert none is None and torch.equal(only_dv, dval)


def test_ops_reject_bad_arguments():
    rp, col = _graph()
    nnz = col.numel()
    X, E = torch.zeros(17, 8), torch.zeros(nnz, 8)
    with pytest.raises(ValueError):
        ops.espmm(rp, col, X, E, 8, op="mul", relu=True)
    with pytest.raises(ValueError):
        ops.espmm(rp, col, X, E, 8, op="sub")
    with pytest.raises(TypeError):
        ops.espmm(rp, col, X.double(), E, 8)
    with pytest.raises(TypeError):
        ops.espmm(rp, col, X, E, 8, val=torch.ones(nnz, dtype=torch.float16))
    with pytest.raises(TypeError):
        ops.espmm(rp, col, X, E, 8, eperm=torch.arange(nnz))
    with pytest.raises(ValueError):
        ops.espmm(rp, col, X, torch.zeros(nnz, 16)[:, :8], 8)
    with pytest.raises(TypeError):
        ops.egrad(rp, col, torch.zeros(11, 8, dtype=torch.bfloat16), X, E, 8)
    with pytest.raises(ValueError):
        ops.egrad(rp, col, torch.zeros(11, 8), X, E, 8, want_dE=False)
    with pytest.raises(ValueError):
        ops.egrad(rp, col, torch.zeros(11, 8), X, E, 8, op="mul", relu=True)


@pytest.mark.parametrize("op,relu", [("add", False), ("add", True), ("mul", False)])
@pytest.mark.parametrize("rect", [False, True])
def test_edge_aggregate_gradcheck(op, relu, rect):
    n_src = 17 if rect else 11
    rp, col = _graph(n_src=n_src)
    nnz, F = col.numel(), 3
    g = WeightedGraph(rp, col, torch.ones(nnz), n_src=n_src)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(n_src, F, dtype=F64, generator=gen)
    e = torch.randn(nnz, F, dtype=F64, generator=gen)
    if relu:                      # keep x_j + e_ij at least 0.1 away from the kink
        s = x[col.long()] + e
        e = e + torch.where(s.abs() < 0.1, torch.where(s >= 0, 0.2, -0.2).to(F64), torch.zeros((), dtype=F64))
        assert float((x[col.long()] + e).abs().min()) >= 0.1
    val = torch.randn(nnz, dtype=F64, generator=gen)
    x.requires_grad_(), e.requires_grad_(), val.requires_grad_()
    f = lambda x, e, val: edge_aggregate(x, e, g, op, relu, val)
    assert torch.autograd.gradcheck(f, (x, e, val), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda x, e: edge_aggregate(x, e, g, op, relu), (x, e), eps=1e-6, atol=1e-7)
    if op == "add" and not relu:  # the sum of edge rows
        assert torch.autograd.gradcheck(lambda e, val: edge_aggregate(None, e, g, val=val), (e, val), eps=1e-6,
                                        atol=1e-7)


def test_edge_aggregate_computes_only_required_gradients():
    rp, col = _graph(n_src=11)
    g = NormGraph(rp, col, torch.ones(11))
    nnz = col.numel()
    x, e, val = torch.randn(11, 4), torch.randn(nnz, 4), torch.rand(nnz)
    xr = x.clone().requires_grad_()
    edge_aggregate(xr, e, g, "add", True, val).sum().backward()
    S = torch.zeros(11, nnz).index_put((_rows(rp), torch.arange(nnz)), torch.ones(nnz))
    m = ((x[col.long()] + e) > 0).float() * val[:, None]
    T = torch.zeros(11, nnz).index_put((col.long(), torch.arange(nnz)), torch.ones(nnz))
    assert torch.allclose(xr.grad, T @ m, atol=1e-6)
    er = e.clone().requires_grad_()
    edge_aggregate(x, er, g, "mul").sum().backward()
    assert torch.allclose(er.grad, x[col.long()], atol=1e-6)
    assert S.shape == (11, nnz)


def _mlp(i, o, gen):
    lin = torch.nn.Linear(i, o)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(o, i, generator=gen) * 0.3)
        lin.bias.zero_()
    return lin


@pytest.mark.parametrize("rect", [False, True])
def test_gineconv_shapes_init_and_semantics(rect):
    n_src = 17 if rect else 11
    rp, col = _graph(n_src=n_src)
    n, nnz = rp.numel() - 1, col.numel()
    g = WeightedGraph(rp, col, torch.ones(nnz), n_src=n_src)
    a = GINEConv(_mlp(6, 4, torch.Generator().manual_seed(1)), eps=0.25, in_dim=6, edge_dim=3,
                 generator=torch.Generator().manual_seed(5))
    b = GINEConv(_mlp(6, 4, torch.Generator().manual_seed(1)), eps=0.25, in_dim=6, edge_dim=3,
                 generator=torch.Generator().manual_seed(5))
    assert torch.equal(a.lin.weight, b.lin.weight) and a.lin.weight.shape == (3, 6)
    assert float(a.lin.weight.detach().abs().max()) <= math.sqrt(6.0 / 9) and torch.all(a.lin.bias == 0)
    assert not list(GINEConv(torch.nn.Identity()).parameters())
    assert [p.shape for p in GINEConv(torch.nn.Identity(), train_eps=True).parameters()] == [torch.Size([1])]
    with pytest.raises(ValueError):
        GINEConv(torch.nn.Identity(), edge_dim=3)
    gen = torch.Generator().manual_seed(2)
    x, e = torch.randn(n_src, 6, generator=gen), torch.randn(nnz, 3, generator=gen)
    out = a(x, g, e)
    assert out.shape == (n, 4)
    le = e @ a.lin.weight + a.lin.bias
    agg = torch.zeros(n, 6).index_add_(0, _rows(rp), (x[col.long()] + le).relu())
    assert torch.allclose(out, a.nn(1.25 * x[:n] + agg), atol=1e-5)
    with pytest.raises(ValueError):
        GINEConv(torch.nn.Identity())(x, g, e)                # widths differ, no lin


@pytest.mark.parametrize("rect", [False, True])
def test_cfconv_shapes_init_and_semantics(rect):
    n_src = 17 if rect else 11
    rp, col = _graph(n_src=n_src)
    n, nnz = rp.numel() - 1, col.numel()
    g = WeightedGraph(rp, col, torch.ones(nnz), n_src=n_src)
    a = CFConv(6, 5, 7, 3, generator=torch.Generator().manual_seed(9))
    b = CFConv(6, 5, 7, 3, generator=torch.Generator().manual_seed(9))
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    assert a.lin1.bias is None and a.lin1.weight.shape == (6, 7) and a.lin2.weight.shape == (7, 5)
    assert a.filter1.weight.shape == (3, 7) and a.filter2.weight.shape == (7, 7)
    assert all(torch.all(m.bias == 0) for m in (a.filter1, a.filter2, a.lin2))
    gen = torch.Generator().manual_seed(2)
    x, e = torch.randn(n_src, 6, generator=gen), torch.randn(nnz, 3, generator=gen)
    cut = torch.rand(nnz, generator=gen)
    out = a(x, g, e, cutoff=cut)
    assert out.shape == (n, 5)
    w = (torch.nn.functional.softplus(e @ a.filter1.weight) - math.log(2.0)) @ a.filter2.weight
    agg = torch.zeros(n, 7).index_add_(0, _rows(rp), (x @ a.lin1.weight)[col.long()] * w * cut[:, None])
    assert torch.allclose(out, agg @ a.lin2.weight, atol=1e-5)
    assert torch.allclose(a(x, g, e), a(x, g, e, cutoff=torch.ones(nnz)), atol=1e-6)
