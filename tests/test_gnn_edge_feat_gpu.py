"""Exact oracle tests of the edge-feature HIP kernels (gnn_espmm.hip: espmm_kernel,
egrad_kernel) and of the layer API on top of them (``edge_aggregate``, ``GINEConv``,
``CFConv``).

Every reference is computed here, in fp64, from dense index ops -- never through the CPU
branches of ``ops``.  X, E and dY are integers in [-3, 3], edge values come from {+-0.25,
+-0.5, +-1, +-2} plus about 1/8 exact zeros: every product is a multiple of 2^-2 and at most
18 in magnitude, every row sum stays below 8192 at 197 edges and every dval below 18 * 520, so
fp32 is exact whatever the order of the operations, and every dE element (at most 72
quarter-units) is exact in bf16 and fp16.  Each test asserts that with an fp32 round trip of
its reference and a magnitude bound.  The comparison is ``torch.equal`` against the fp64
result cast to the storage type.
"""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from cgnn_amd.gnn import ops
from cgnn_amd.gnn.layers import CFConv, GINEConv, WeightedGraph, edge_aggregate
from cgnn_amd.utils.hipgraph import StepGraph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 7.0            # sentinel of rows / buffers a kernel must not write
PAD = 5.0             # what the padding columns of the inputs hold
BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
VALS = [-2.0, -1.0, -0.5, -0.25, 0.25, 0.5, 1.0, 2.0]
N_SRC = 257


# ------------------------------------------------------------------ helpers
def _csr(deg, n_src, rng):
    """CSR (int32 rowptr, col) and fp32 values of the given row degrees with random source
    ids; some rows repeat one id (with different values), some hold source 0 and source
    n_src - 1; about one value in eight is an exact zero."""
    deg = np.asarray(deg, dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = rng.integers(0, n_src, int(rp[-1])).astype(np.int32)
    for i, d in enumerate(deg):
        if d == 0:
            continue
        e0 = int(rp[i])
        if i % 5 == 1:
            col[e0:e0 + d] = col[e0]
        if i % 7 == 2:
            col[e0] = 0
            col[e0 + d - 1] = n_src - 1
    val = rng.choice(VALS, col.size)
    val[rng.random(col.size) < 0.125] = 0.0
    return torch.from_numpy(rp), torch.from_numpy(col), torch.from_numpy(val).float()


def _rows(rp):
    return torch.repeat_interleave(torch.arange(rp.numel() - 1), (rp[1:] - rp[:-1]).long())


def _ints(rng, lo, hi, shape):
    return torch.from_numpy(rng.integers(lo, hi + 1, shape).astype(np.float64))


def _exact(ref, bound):
    """The reference survives a round trip through fp32 and stays below ``bound``."""
    return torch.equal(ref.float().double(), ref) and (ref.numel() == 0 or float(ref.abs().max()) < bound)


def _assert_same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero()
        idx = tuple(int(x) for x in bad[0])
        raise AssertionError("%s: %d elements differ, first at %r: got %r, expected %r"
                             % (what, bad.shape[0], idx, float(got[idx]), float(exp[idx])))


def _degrees(L):
    d = [0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, L - 1, L, L + 1, L + 4, L + 8, L + 13,
         2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 5]
    # the list, the list reversed, and three more rows: 53 rows, no multiple of the
    # 4 * (64 / L) rows of a block for any L
    return d + d[::-1] + [2, L + 1, 0]


@functools.lru_cache(maxsize=None)
def _graph(L):
    rng = np.random.default_rng(300 + L)
    deg = _degrees(L)
    assert len(deg) == 53 and len(deg) % (4 * (64 // L)) != 0
    rp, col, val = _csr(deg, N_SRC, rng)
    n, nnz = len(deg), col.numel()
    # rows that repeat one source id (and do not have their ends overwritten)
    dup = [(int(rp[i]), int(rp[i + 1])) for i in range(n) if i % 5 == 1 and i % 7 != 2
           and int(rp[i + 1]) - int(rp[i]) >= 2]
    assert dup
    perm = torch.from_numpy(np.random.default_rng(L).permutation(nnz)).to(torch.int32)
    assert not torch.equal(perm, torch.arange(nnz, dtype=torch.int32))
    val_s = torch.empty(nnz)
    val_s[perm.long()] = val
    return dict(n=n, nnz=nnz, rp=rp, col=col, val=val, rows=_rows(rp), dup=dup, perm=perm, rp_d=rp.to(DEV),
                col_d=col.to(DEV), val_d=val.to(DEV), perm_d=perm.to(DEV), val_s_d=val_s.to(DEV))


# (F, ld, L): L lanes per row, from the written width; the last crosses a 512-column slab
WIDTHS = [(8, 8, 8), (41, 48, 8), (65, 72, 16), (129, 136, 32), (257, 264, 64), (520, 528, 64)]
DTYPES = [F32, BF16, F16]
# (op, relu, with X)
CASES = [("add", False, True), ("add", True, True), ("mul", False, True), ("add", False, False)]


@functools.lru_cache(maxsize=None)
def _inputs(F, ld, L):
    """fp64 X [257, ld], E [nnz, ld], dY [53, ld] with integer features and PAD in the padding
    columns; the E rows of a row that repeats one source are equal (duplicate edges)."""
    g = _graph(L)
    rng = np.random.default_rng(4000 + F)
    X = torch.full((N_SRC, ld), PAD, dtype=F64)
    E = torch.full((g["nnz"], ld), PAD, dtype=F64)
    G = torch.full((g["n"], ld), PAD, dtype=F64)
    X[:, :F], E[:, :F], G[:, :F] = _ints(rng, -3, 3, (N_SRC, F)), _ints(rng, -3, 3, (g["nnz"], F)), \
        _ints(rng, -3, 3, (g["n"], F))
    for e0, e1 in g["dup"]:
        E[e0:e1] = E[e0]
    Es = torch.empty_like(E)
    Es[g["perm"].long()] = E
    return X, E, G, Es


def _messages(g, X, E, F, case):
    """m_e [nnz, F] and the derivative factor d_e [nnz, F] of one case, fp64."""
    op, relu, with_x = case
    e = E[:, :F]
    if not with_x:
        return e, torch.ones_like(e)
    x = X[g["col"].long(), :F]
    if op == "mul":
        return x * e, x
    s = x + e
    return (s.clamp_min(0), (s > 0).double()) if relu else (s, torch.ones_like(s))


def _segsum(g, t):
    return torch.zeros(g["n"], t.shape[1], dtype=F64).index_add_(0, g["rows"], t)


# ------------------------------------------------------------------ 1. espmm
@pytest.mark.parametrize("F,ld,L", WIDTHS)
def test_espmm_exact_over_row_lengths_widths_and_dtypes(F, ld, L):
    """espmm_kernel against the fp64 sum per destination, bit for bit: rows of every chunk /
    remainder class for L lanes per row; add, add + relu, mul and the sum of edge rows; with
    and without edge values; E and val in edge order and shuffled behind a non-identity
    edge permutation; three storage types; padding columns of X and E that must not be
    read into the result; three sentinel rows past the output; zero padding columns."""
    g = _graph(L)
    n = g["n"]
    X, E, _, Es = _inputs(F, ld, L)
    for case in CASES:
        op, relu, with_x = case
        m, _ = _messages(g, X, E, F, case)
        for with_val in (False, True):
            ref = _segsum(g, m * g["val"].double()[:, None] if with_val else m)
            assert _exact(ref, 8192) and float(ref.abs().max()) > 8
            for dt in DTYPES:
                exp = torch.zeros(n, ld, dtype=F64)
                exp[:, :F] = ref
                exp = exp.to(dt)
                Xd = X.to(dt).to(DEV) if with_x else None
                for Ed, vd, ep in ((E.to(dt).to(DEV), g["val_d"], None), (Es.to(dt).to(DEV), g["val_s_d"], g["perm_d"])):
                    full = torch.full((n + 3, ld), SENT, dtype=dt, device=DEV)
                    ops.espmm(g["rp_d"], g["col_d"], Xd, Ed, F, op=op, relu=relu, val=vd if with_val else None,
                              eperm=ep, out=full[:n])
                    got = full.cpu()
                    what = "%s relu=%d X=%d val=%d eperm=%d %s" % (op, relu, with_x, with_val, ep is not None, dt)
                    _assert_same(got[:n], exp, what)
                    assert torch.all(got[n:] == SENT), what + ": rows past n_rows written"
                    assert torch.all(got[:n, F:] == 0), what + ": padding columns"


# ------------------------------------------------------------------ 2. egrad
@pytest.mark.parametrize("F,ld,L", WIDTHS)
def test_egrad_exact_over_row_lengths_widths_and_dtypes(F, ld, L):
    """egrad_kernel: dE[e] = w_e dY[i] d_e and dval[e] = <dY[i], m_e> per edge, bit for bit,
    for the cases of the forward test; a sentinel tail past nnz in both outputs; zero dE
    padding columns; dE-only and dval-only calls; equal dval for duplicate edges of a row;
    the ReLU mask is 0 where x + e is exactly 0."""
    g = _graph(L)
    n, nnz = g["n"], g["nnz"]
    X, E, G, _ = _inputs(F, ld, L)
    gy = G[g["rows"], :F]
    for case in CASES:
        op, relu, with_x = case
        m, d = _messages(g, X, E, F, case)
        ref_dv = (gy * m).sum(1)
        assert _exact(ref_dv, 18 * 520)
        if relu:
            zero = (X[g["col"].long(), :F] + E[:, :F]) == 0
            assert int(zero.sum()) > nnz // 2 and torch.all(d[zero] == 0)
        for with_val in (False, True):
            ref_de = gy * d * (g["val"].double()[:, None] if with_val else 1.0)
            assert _exact(ref_de, 18.25)
            for dt in DTYPES:
                exp = torch.zeros(nnz, ld, dtype=F64)
                exp[:, :F] = ref_de
                exp = exp.to(dt)
                assert torch.equal(exp.double()[:, :F], ref_de)             # exact in the storage type
                Xd = X.to(dt).to(DEV) if with_x else None
                Ed, Gd = E.to(dt).to(DEV), G.to(dt).to(DEV)
                kw = dict(op=op, relu=relu, val=g["val_d"] if with_val else None)
                what = "%s relu=%d X=%d val=%d %s" % (op, relu, with_x, with_val, dt)
                de = torch.full((nnz + 3, ld), SENT, dtype=dt, device=DEV)
                dv = torch.full((nnz + 5,), SENT, device=DEV)
                r = ops.egrad(g["rp_d"], g["col_d"], Gd, Xd, Ed, F, dE=de[:nnz], dval=dv[:nnz], **kw)
                assert r[0].data_ptr() == de.data_ptr() and r[1].data_ptr() == dv.data_ptr()
                got_de, got_dv = de.cpu(), dv.cpu()
                _assert_same(got_de[:nnz], exp, what + " dE")
                _assert_same(got_dv[:nnz], ref_dv.float(), what + " dval")
                assert torch.all(got_de[nnz:] == SENT) and torch.all(got_dv[nnz:] == SENT), what + ": tail written"
                assert torch.all(got_de[:nnz, F:] == 0), what + ": dE padding columns"
                for e0, e1 in g["dup"]:
                    assert torch.all(got_dv[e0:e1] == got_dv[e0]), what + ": duplicate edges differ"
                if relu:
                    assert torch.all(got_de[:nnz, :F][zero] == 0), what + ": mask at x + e == 0"
                # one output at a time
                de1, none = ops.egrad(g["rp_d"], g["col_d"], Gd, Xd, Ed, F, **kw)
                assert none is None
                _assert_same(de1.cpu(), exp, what + " dE alone")
                dv2 = torch.full((nnz + 5,), SENT, device=DEV)
                none, r2 = ops.egrad(g["rp_d"], g["col_d"], Gd, Xd, Ed, F, dval=dv2[:nnz], want_dE=False, **kw)
                assert none is None
                _assert_same(dv2.cpu()[:nnz], ref_dv.float(), what + " dval alone")
                assert torch.all(dv2.cpu()[nnz:] == SENT)


# ------------------------------------------------------------------ 2b. past the second slab
@functools.lru_cache(maxsize=None)
def _small_graph():
    """9 rows, 40 edges, one row empty."""
    rng = np.random.default_rng(45)
    rp, col, val = _csr([3, 0, 1, 9, 4, 5, 7, 9, 2], N_SRC, rng)
    assert col.numel() == 40
    return dict(n=9, nnz=40, rp=rp, col=col, val=val, rows=_rows(rp), rp_d=rp.to(DEV), col_d=col.to(DEV),
                val_d=val.to(DEV))


# (F, ld of X / E / Y / dY, ld of dE).  (1030, 1032): a third 512-column slab holding 6
# features and 2 padding columns, dval the ordered sum of three launches; (500, 1032): slabs
# two and three hold padding only; (8, 8, 520): a second slab that writes 8 padding columns
# of dE and no dval
@pytest.mark.parametrize("F,ld,ldde", [(1030, 1032, 1032), (500, 1032, 1032), (8, 8, 520)])
def test_espmm_and_egrad_exact_past_the_second_slab(F, ld, ldde):
    g = _small_graph()
    n, nnz = g["n"], g["nnz"]
    rng = np.random.default_rng(4200 + F)
    X = torch.full((N_SRC, ld), PAD, dtype=F64)
    E = torch.full((nnz, ld), PAD, dtype=F64)
    G = torch.full((n, ld), PAD, dtype=F64)
    X[:, :F], E[:, :F], G[:, :F] = _ints(rng, -3, 3, (N_SRC, F)), _ints(rng, -3, 3, (nnz, F)), _ints(rng, -3, 3, (n, F))
    gy, w = G[g["rows"], :F], g["val"].double()[:, None]
    for case in CASES:
        op, relu, with_x = case
        m, d = _messages(g, X, E, F, case)
        ref, ref_dv, ref_de = _segsum(g, m * w), (gy * m).sum(1), gy * d * w
        # 9 edges of |w m| <= 18 per row; |dY m| <= 27 per feature; |w dY d| <= 18 in quarter units
        assert _exact(ref, 8192) and _exact(ref_dv, 27 * 1032) and _exact(ref_de, 18.25)
        for dt in DTYPES:
            Xd = X.to(dt).to(DEV) if with_x else None
            Ed, Gd = E.to(dt).to(DEV), G.to(dt).to(DEV)
            kw = dict(op=op, relu=relu, val=g["val_d"])
            what = "%s relu=%d X=%d %s F=%d ldde=%d" % (op, relu, with_x, dt, F, ldde)
            exp = torch.zeros(n, ld, dtype=F64)
            exp[:, :F] = ref
            full = torch.full((n + 3, ld), SENT, dtype=dt, device=DEV)
            ops.espmm(g["rp_d"], g["col_d"], Xd, Ed, F, out=full[:n], **kw)
            got = full.cpu()
            _assert_same(got[:n], exp.to(dt), what)
            assert torch.all(got[:n, F:] == 0), what + ": padding columns"
            assert torch.all(got[n:] == SENT), what + ": written past the last row's stride"
            exp_de = torch.zeros(nnz, ldde, dtype=F64)
            exp_de[:, :F] = ref_de
            de = torch.full((nnz + 3, ldde), SENT, dtype=dt, device=DEV)
            dv = torch.full((nnz + 5,), SENT, device=DEV)
            ops.egrad(g["rp_d"], g["col_d"], Gd, Xd, Ed, F, dE=de[:nnz], dval=dv[:nnz], **kw)
            got_de, got_dv = de.cpu(), dv.cpu()
            _assert_same(got_de[:nnz], exp_de.to(dt), what + " dE")
            _assert_same(got_dv[:nnz], ref_dv.float(), what + " dval")
            assert torch.all(got_de[:nnz, F:] == 0), what + ": dE padding columns"
            assert torch.all(got_de[nnz:] == SENT) and torch.all(got_dv[nnz:] == SENT), what + ": tail written"


# ------------------------------------------------------------------ 3. transposed dx pass
def test_transposed_pass_is_the_gradient_with_respect_to_the_node_rows():
    """On the rectangular 53 x 257 graph: espmm mul over ``transposed_perm()`` with X = dY
    gives dX[j] = sum_{e = (i, j)} w_e dY[i] E[e], and the X = None sum of the dE rows gives
    the add / add + relu gradient."""
    L, F, ld = 16, 41, 48
    g = _graph(L)
    n, nnz = g["n"], g["nnz"]
    X, E, G, _ = _inputs(F, ld, L)
    wg = WeightedGraph(g["rp_d"], g["col_d"], g["val_d"], n_src=N_SRC)
    rp_t, col_t, eperm = wg.transposed_perm()
    assert rp_t.numel() == N_SRC + 1 and n != N_SRC and not torch.equal(eperm.cpu(), torch.arange(nnz, dtype=torch.int32))
    gy, w = G[g["rows"], :F], g["val"].double()[:, None]
    scatter = lambda t: torch.zeros(N_SRC, F, dtype=F64).index_add_(0, g["col"].long(), t)
    ref_mul = scatter(w * gy * E[:, :F])
    assert _exact(ref_mul, 8192)
    for dt in DTYPES:
        got = ops.espmm(rp_t, col_t, G.to(dt).to(DEV), E.to(dt).to(DEV), F, op="mul", val=g["val_d"], eperm=eperm)
        exp = torch.zeros(N_SRC, ld, dtype=F64)
        exp[:, :F] = ref_mul
        _assert_same(got.cpu(), exp.to(dt), "transposed mul %s" % dt)
        for relu in (False, True):
            _, d = _messages(g, X, E, F, ("add", relu, True))
            ref = scatter(w * gy * d)
            assert _exact(ref, 8192)
            dE, _ = ops.egrad(g["rp_d"], g["col_d"], G.to(dt).to(DEV), X.to(dt).to(DEV), E.to(dt).to(DEV), F, relu=relu,
                              val=g["val_d"])
            got = ops.espmm(rp_t, col_t, None, dE, F, eperm=eperm)
            exp = torch.zeros(N_SRC, ld, dtype=F64)
            exp[:, :F] = ref
            _assert_same(got.cpu(), exp.to(dt), "sum of dE rows relu=%d %s" % (relu, dt))


# ------------------------------------------------------------------ 4. autograd
@functools.lru_cache(maxsize=None)
def _directed():
    """40 nodes, ~200 directed edges through ``from_edges``; the values are then overwritten
    by exact ones."""
    n = 40
    rng = np.random.default_rng(11)
    src, dst = rng.integers(0, n, 200), rng.integers(0, n, 200)
    g = WeightedGraph.from_edges(n, src, dst, rng.uniform(0.5, 2.0, 200), normalize="rw", device=DEV)
    nnz = g.col.numel()
    assert 150 <= nnz <= 240
    val = torch.from_numpy(rng.choice(VALS, nnz)).float()
    val[::9] = 0.0
    g.val = val.to(DEV)
    return g, val


def _autograd_graphs():
    g, val = _directed()
    r = _graph(16)
    return [("directed", g, g.rowptr.cpu(), g.col.cpu(), val, g.n),
            ("rectangular", WeightedGraph(r["rp_d"], r["col_d"], r["val_d"], n_src=N_SRC), r["rp"], r["col"],
             r["val"], N_SRC)]


@pytest.mark.parametrize("op,relu", [("add", False), ("add", True), ("mul", False)])
def test_edge_aggregate_forward_dx_de_dval_exact(op, relu):
    F = 12
    for name, g, rp, col, val, n_src in _autograd_graphs():
        n, nnz = rp.numel() - 1, col.numel()
        rng = np.random.default_rng(12)
        xd, ed, gd = _ints(rng, -3, 3, (n_src, F)), _ints(rng, -3, 3, (nnz, F)), _ints(rng, -3, 3, (n, F))
        xr, er, vr = xd.clone().requires_grad_(), ed.clone().requires_grad_(), val.double().requires_grad_()
        m = xr[col.long()] * er if op == "mul" else xr[col.long()] + er
        if relu:
            m = m.relu()
        yr = torch.zeros(n, F, dtype=F64).index_add(0, _rows(rp), vr[:, None] * m)
        yr.backward(gd)
        for t in (yr.detach(), xr.grad, er.grad, vr.grad):
            assert _exact(t, 8192)
        for dt in (F32, BF16):
            what = "%s %s relu=%d %s" % (name, op, relu, dt)
            assert torch.equal(er.grad.to(dt).double(), er.grad)              # de exact in the storage type
            x = xd.to(dt).to(DEV).requires_grad_()
            e = ed.to(dt).to(DEV).requires_grad_()
            v = val.clone().to(DEV).requires_grad_()
            y = edge_aggregate(x, e, g, op, relu, v)
            y.backward(gd.to(dt).to(DEV))
            _assert_same(y.detach().cpu(), yr.detach().to(dt), what + " y")
            _assert_same(x.grad.cpu(), xr.grad.to(dt), what + " dx")
            _assert_same(e.grad.cpu(), er.grad.to(dt), what + " de")
            assert v.grad.dtype == F32
            _assert_same(v.grad.cpu(), vr.grad.float(), what + " dval")
            # gradients that are not required are absent, the others unchanged
            x2 = xd.to(dt).to(DEV).requires_grad_()
            e2, v2 = ed.to(dt).to(DEV), val.clone().to(DEV)
            edge_aggregate(x2, e2, g, op, relu, v2).backward(gd.to(dt).to(DEV))
            assert e2.grad is None and v2.grad is None
            _assert_same(x2.grad.cpu(), xr.grad.to(dt), what + " dx alone")
            e3 = ed.to(dt).to(DEV).requires_grad_()
            edge_aggregate(xd.to(dt).to(DEV), e3, g, op, relu, v2).backward(gd.to(dt).to(DEV))
            _assert_same(e3.grad.cpu(), er.grad.to(dt), what + " de alone")


# ------------------------------------------------------------------ 5. launch mates
@pytest.mark.parametrize("L,F", [(8, 41), (16, 128), (32, 129), (64, 257)])
def test_a_row_does_not_depend_on_its_launch_mates(L, F):
    """A row's espmm output and its edges' egrad outputs are the same bits in the 53-row
    graph and in a graph that holds that row alone, and from run to run.  Non-exact inputs
    here (random normal), so any change in the order of a row's operations would show."""
    g = _graph(L)
    n, nnz, ld = g["n"], g["nnz"], -(-F // 8) * 8
    gen = torch.Generator().manual_seed(L)
    X, E, G = torch.zeros(N_SRC, ld), torch.zeros(nnz, ld), torch.zeros(n, ld)
    X[:, :F], E[:, :F], G[:, :F] = torch.randn(N_SRC, F, generator=gen), torch.randn(nnz, F, generator=gen), \
        torch.randn(n, F, generator=gen)
    val_d = torch.randn(nnz, generator=gen).to(DEV)
    for dt in (F32, BF16):
        Xd, Ed, Gd = X.to(dt).to(DEV), E.to(dt).to(DEV), G.to(dt).to(DEV)
        for op, relu in (("add", True), ("mul", False)):
            kw = dict(op=op, relu=relu)
            y = ops.espmm(g["rp_d"], g["col_d"], Xd, Ed, F, val=val_d, **kw)
            de, dv = ops.egrad(g["rp_d"], g["col_d"], Gd, Xd, Ed, F, val=val_d, want_dval=True, **kw)
            y2 = ops.espmm(g["rp_d"], g["col_d"], Xd, Ed, F, val=val_d, **kw)
            de2, dv2 = ops.egrad(g["rp_d"], g["col_d"], Gd, Xd, Ed, F, val=val_d, want_dval=True, **kw)
            assert torch.equal(y, y2) and torch.equal(de, de2) and torch.equal(dv, dv2)      # run to run
            assert float(y.float().abs().max()) > 1 and float(dv.abs().max()) > 1
            for i in (3, 15, 24, 27, 51):                                 # degrees 3, L - 1, 3 L + 5, 2 L, L + 1
                e0, e1 = int(g["rp"][i]), int(g["rp"][i + 1])
                rp1 = torch.tensor([0, e1 - e0], dtype=torch.int32, device=DEV)
                c1, v1, E1 = g["col_d"][e0:e1].contiguous(), val_d[e0:e1].contiguous(), Ed[e0:e1].contiguous()
                y1 = ops.espmm(rp1, c1, Xd, E1, F, val=v1, **kw)
                de1, dv1 = ops.egrad(rp1, c1, Gd[i:i + 1].contiguous(), Xd, E1, F, val=v1, want_dval=True, **kw)
                assert torch.equal(y1[0], y[i]), "espmm row %d %s %s" % (i, op, dt)
                assert torch.equal(de1, de[e0:e1]), "egrad dE row %d %s %s" % (i, op, dt)
                assert torch.equal(dv1, dv[e0:e1]), "egrad dval row %d %s %s" % (i, op, dt)


# ------------------------------------------------------------------ 6. edge cases
def test_graph_with_rows_but_no_edges_and_no_rows():
    n, F = 9, 24
    rp = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    col = torch.zeros(0, dtype=torch.int32, device=DEV)
    X = torch.ones(5, F, dtype=BF16, device=DEV)
    E = torch.ones(0, F, dtype=BF16, device=DEV)
    G = torch.ones(n, F, dtype=BF16, device=DEV)
    for x in (X, None):
        y = torch.full((n + 1, F), SENT, dtype=BF16, device=DEV)
        ops.espmm(rp, col, x, E, 20, relu=x is not None, out=y[:n])
        assert torch.all(y[:n] == 0) and torch.all(y[n:] == SENT)
    de = torch.full((2, F), SENT, dtype=BF16, device=DEV)
    dv = torch.full((4,), SENT, device=DEV)
    ops.egrad(rp, col, G, X, E, 20, dE=de[:0], dval=dv[:0])
    # no rows at all
    ops.espmm(rp[:1], col, X, E, 20, out=torch.empty(0, F, dtype=BF16, device=DEV))
    ops.egrad(rp[:1], col, G[:0], X, E, 20, dE=de[:0], dval=dv[:0])
    torch.cuda.synchronize()
    assert torch.all(de == SENT) and torch.all(dv == SENT)


def test_one_row_and_single_edge():
    rng = np.random.default_rng(8)
    F, ld = 20, 24
    X = torch.full((N_SRC, ld), PAD, dtype=F64)
    X[:, :F] = _ints(rng, -3, 3, (N_SRC, F))
    G = torch.zeros(1, ld, dtype=F64)
    G[:, :F] = _ints(rng, -3, 3, (1, F))
    for deg in (1, 19):                                  # a single edge; one row of 19
        rp, col, val = _csr([deg], N_SRC, rng)
        E = torch.full((deg, ld), PAD, dtype=F64)
        E[:, :F] = _ints(rng, -3, 3, (deg, F))
        s = X[col.long(), :F] + E[:, :F]
        ref = (val.double()[:, None] * s.clamp_min(0)).sum(0, keepdim=True)
        ref_de = val.double()[:, None] * G[:, :F] * (s > 0)
        ref_dv = (G[:, :F] * s.clamp_min(0)).sum(1)
        assert _exact(ref, 4096) and _exact(ref_de, 18.25) and _exact(ref_dv, 4096)
        args = (rp.to(DEV), col.to(DEV))
        full = torch.full((4, ld), SENT, device=DEV)
        ops.espmm(*args, X.float().to(DEV), E.float().to(DEV), F, relu=True, val=val.to(DEV), out=full[:1])
        got = full.cpu()
        _assert_same(got[:1, :F], ref.float(), "n_rows = 1, degree %d" % deg)
        assert torch.all(got[1:] == SENT) and torch.all(got[:1, F:] == 0)
        de = torch.full((deg + 2, ld), SENT, device=DEV)
        dv = torch.full((deg + 2,), SENT, device=DEV)
        ops.egrad(*args, G.float().to(DEV), X.float().to(DEV), E.float().to(DEV), F, relu=True, val=val.to(DEV),
                  dE=de[:deg], dval=dv[:deg])
        _assert_same(de.cpu()[:deg, :F], ref_de.float(), "egrad dE n_rows = 1, degree %d" % deg)
        _assert_same(dv.cpu()[:deg], ref_dv.float(), "egrad dval n_rows = 1, degree %d" % deg)
        assert torch.all(de.cpu()[deg:] == SENT) and torch.all(dv.cpu()[deg:] == SENT)
        assert torch.all(de.cpu()[:deg, F:] == 0)


# ------------------------------------------------------------------ 7. capture
def test_forward_egrad_and_transposed_pass_in_a_captured_graph():
    """espmm, egrad and the transposed sum of the dE rows into preallocated outputs, captured
    and replayed twice: the eager bits both times (the launchers allocate nothing and do not
    synchronise)."""
    L, F, ld = 16, 100, 104
    g = _graph(L)
    n, nnz = g["n"], g["nnz"]
    rng = np.random.default_rng(77)
    Xf, Ef, Gf = torch.zeros(N_SRC, ld, dtype=F64), torch.zeros(nnz, ld, dtype=F64), torch.zeros(n, ld, dtype=F64)
    Xf[:, :F], Ef[:, :F], Gf[:, :F] = _ints(rng, -3, 3, (N_SRC, F)), _ints(rng, -3, 3, (nnz, F)), \
        _ints(rng, -3, 3, (n, F))
    X, E, G = Xf.to(BF16).to(DEV), Ef.to(BF16).to(DEV), Gf.to(BF16).to(DEV)
    rp_t, col_t, eperm = WeightedGraph(g["rp_d"], g["col_d"], g["val_d"], n_src=N_SRC).transposed_perm()
    y = torch.empty(n, ld, dtype=BF16, device=DEV)
    de = torch.empty(nnz, ld, dtype=BF16, device=DEV)
    dv = torch.empty(nnz, device=DEV)
    dx = torch.empty(N_SRC, ld, dtype=BF16, device=DEV)

    def step():
        ops.espmm(g["rp_d"], g["col_d"], X, E, F, relu=True, val=g["val_d"], out=y)
        ops.egrad(g["rp_d"], g["col_d"], G, X, E, F, relu=True, val=g["val_d"], dE=de, dval=dv)
        ops.espmm(rp_t, col_t, None, de, F, eperm=eperm, out=dx)

    step()
    torch.cuda.synchronize()
    y0, de0, dv0, dx0 = y.clone(), de.clone(), dv.clone(), dx.clone()
    s = Xf[g["col"].long(), :F] + Ef[:, :F]
    ref = _segsum(g, g["val"].double()[:, None] * s.clamp_min(0))
    assert _exact(ref, 8192)
    _assert_same(y0.cpu()[:, :F], ref.to(BF16), "eager espmm")
    ref_dx = torch.zeros(N_SRC, F, dtype=F64).index_add_(
        0, g["col"].long(), g["val"].double()[:, None] * Gf[g["rows"], :F] * (s > 0))
    assert _exact(ref_dx, 8192)
    _assert_same(dx0.cpu()[:, :F], ref_dx.to(BF16), "eager transposed pass")
    sg = StepGraph(step, warmup=1, device=torch.device(DEV))
    sg()                                                   # eager warm-up
    for k in range(2):
        for t in (y, de, dv, dx):
            t.fill_(SENT)
        sg()
        assert sg.graph is not None
        torch.cuda.synchronize()
        assert torch.equal(y, y0) and torch.equal(de, de0) and torch.equal(dv, dv0) and torch.equal(dx, dx0), \
            "replay %d" % k


# ------------------------------------------------------------------ 8. rejections
def test_rejections_raise_before_any_launch():
    g = _graph(8)
    n, nnz = g["n"], g["nnz"]
    a = (g["rp_d"], g["col_d"])
    X = torch.ones(N_SRC, 16, device=DEV)
    E = torch.ones(nnz, 16, device=DEV)
    G = torch.ones(n, 16, device=DEV)
    y = torch.full((n, 16), SENT, device=DEV)
    de = torch.full((nnz, 16), SENT, device=DEV)
    dv = torch.full((nnz,), SENT, device=DEV)
    with pytest.raises(TypeError):                         # mixed storage types
        ops.espmm(*a, X.to(BF16), E, 16, out=y)
    with pytest.raises(TypeError):
        ops.espmm(*a, X, E, 16, out=y.to(BF16))
    with pytest.raises(TypeError):
        ops.egrad(*a, G.to(F16), X, E, 16, dE=de, dval=dv)
    with pytest.raises(TypeError):                         # fp64 is not a kernel type
        ops.espmm(*a, X.double(), E.double(), 16)
    with pytest.raises(RuntimeError, match="-3"):          # ld % 8 != 0: X, E, then the output
        ops.espmm(*a, torch.ones(N_SRC, 12, device=DEV), E, 12, out=y)
    with pytest.raises(RuntimeError, match="-3"):
        ops.espmm(*a, X, torch.ones(nnz, 12, device=DEV), 12, out=y)
    y12 = torch.full((n, 12), SENT, device=DEV)
    with pytest.raises(RuntimeError, match="-3"):
        ops.espmm(*a, X, E, 12, out=y12)
    with pytest.raises(RuntimeError, match="-3"):
        ops.egrad(*a, torch.ones(n, 12, device=DEV), X, E, 12, dE=de, dval=dv)
    de12 = torch.full((nnz, 12), SENT, device=DEV)
    with pytest.raises(RuntimeError, match="-3"):
        ops.egrad(*a, G, X, E, 12, dE=de12)
    with pytest.raises(RuntimeError, match="-3"):          # F > ld
        ops.espmm(*a, X, E, 17, out=y)
    with pytest.raises(RuntimeError, match="-3"):
        ops.egrad(*a, G, X, E, 17, dE=de, dval=dv)
    with pytest.raises(ValueError):                        # relu goes with add
        ops.espmm(*a, X, E, 16, op="mul", relu=True, out=y)
    with pytest.raises(ValueError):
        ops.egrad(*a, G, X, E, 16, op="mul", relu=True, dE=de, dval=dv)
    with pytest.raises(TypeError):                         # fp16 values
        ops.espmm(*a, X, E, 16, val=g["val_d"].to(F16), out=y)
    with pytest.raises(TypeError):
        ops.egrad(*a, G, X, E, 16, val=g["val_d"].to(F16), dE=de, dval=dv)
    with pytest.raises(TypeError):                         # int64 permutation
        ops.espmm(*a, X, E, 16, eperm=g["perm_d"].long(), out=y)
    with pytest.raises(ValueError):                        # neither output
        ops.egrad(*a, G, X, E, 16, want_dE=False)
    torch.cuda.synchronize()
    for t in (y, y12, de, de12, dv):
        assert torch.all(t == SENT)


# ------------------------------------------------------------------ 9. layers
def _layer_graph(kind, dev):
    if kind == "rectangular":
        g = _graph(16)
        return WeightedGraph(g["rp"].to(dev), g["col"].to(dev), g["val"].to(dev), n_src=N_SRC), g["n"], N_SRC, g["nnz"]
    g, val = _directed()
    return WeightedGraph(g.rowptr.to(dev), g.col.to(dev), val.to(dev)), g.n, g.n, g.col.numel()


def _gine(seed=3):
    torch.manual_seed(seed)
    nn = torch.nn.Sequential(torch.nn.Linear(12, 16), torch.nn.ReLU(), torch.nn.Linear(16, 8))
    return GINEConv(nn, eps=0.25, train_eps=True, in_dim=12, edge_dim=5, generator=torch.Generator().manual_seed(seed))


def _cfconv(seed=3):
    m = CFConv(12, 8, 16, 5, generator=torch.Generator().manual_seed(seed))
    with torch.no_grad():
        m.filter1.bias.fill_(0.25)
        m.lin2.bias.fill_(-0.5)
    return m


@pytest.mark.parametrize("kind", ["directed", "rectangular"])
@pytest.mark.parametrize("layer", ["gine", "cfconv"])
def test_layers_gpu_fp32_match_cpu_fp64(layer, kind):
    _, n, n_src, nnz = _layer_graph(kind, "cpu")
    rng = np.random.default_rng(6)
    h0, e0, c0 = rng.standard_normal((n_src, 12)), rng.standard_normal((nnz, 5)), rng.standard_normal((n, 8))
    cut0 = rng.uniform(0, 1, nnz)
    base = _gine() if layer == "gine" else _cfconv()

    def run(dev, dt):
        m = copy.deepcopy(base).to(dt).to(dev)
        g = _layer_graph(kind, dev)[0]
        h = torch.from_numpy(h0).to(dt).to(dev).requires_grad_()
        e = torch.from_numpy(e0).to(dt).to(dev).requires_grad_()
        grads = {}
        if layer == "gine":
            out = m(h, g, e)
        else:
            cut = torch.from_numpy(cut0).to(dt).to(dev).requires_grad_()
            out = m(h, g, e, cutoff=cut)
        out.backward(torch.from_numpy(c0).to(dt).to(dev))
        grads = {k: p.grad.double().cpu().numpy() for k, p in m.named_parameters()}
        grads["h"], grads["e"] = h.grad.double().cpu().numpy(), e.grad.double().cpu().numpy()
        if layer == "cfconv":
            grads["cutoff"] = cut.grad.double().cpu().numpy()
        return out.detach().double().cpu().numpy(), grads

    out_c, grads_c = run("cpu", F64)
    out_g, grads_g = run(DEV, F32)
    assert out_g.shape == (n, 8)
    np.testing.assert_allclose(out_g, out_c, rtol=1e-4, atol=1e-4)
    assert len(grads_c) == (9 if layer == "gine" else 10)
    for k in grads_c:
        np.testing.assert_allclose(grads_g[k], grads_c[k], rtol=1e-4, atol=1e-4, err_msg=k)
        assert float(np.abs(grads_c[k]).max()) > 1e-3, k


@pytest.mark.parametrize("layer", ["gine", "cfconv"])
def test_layers_bf16_forward(layer):
    g, n, n_src, nnz = _layer_graph("directed", DEV)
    m = (_gine() if layer == "gine" else _cfconv()).to(DEV)
    gen = torch.Generator().manual_seed(8)
    h = torch.randn(n_src, 12, generator=gen).to(BF16).to(DEV)
    e = torch.randn(nnz, 5, generator=gen).to(BF16).to(DEV)
    mb = copy.deepcopy(m)
    if layer == "gine":
        mb.nn.to(BF16)                                   # the caller's module runs in the storage dtype
    out = mb(h, g, e)
    assert out.dtype == BF16 and out.shape == (n, 8) and torch.isfinite(out.float()).all()
    ref = m(h.float(), g, e.float()).detach()
    assert torch.allclose(out.detach().float(), ref, rtol=5e-2, atol=5e-2)    # bf16 storage: 2^-8 per rounding
