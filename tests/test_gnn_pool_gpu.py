"""Exact oracle tests of the max / min pooling HIP kernels (gnn_pool.hip: pool_fwd_kernel,
pool_bwd_kernel) and of the layer API on top of them.

Every reference is computed here, in fp64 / numpy from the CSR -- never through the CPU
branches of ``ops``.  The forward accumulates nothing (its result is a copy of an input
element), so it is compared bit for bit on arbitrary data; the backward sums integers in
[-3, 3], exact in fp32 in any order (asserted with an fp32 round trip and a magnitude bound).
The comparison is ``torch.equal`` against the fp64 result cast to the output type.
"""
import functools

import numpy as np
import pytest
import torch

from cgnn_amd import native
from cgnn_amd.gnn import ops
from cgnn_amd.gnn.layers import NormGraph, WeightedGraph, pool_aggregate
from cgnn_amd.gnn.sage import SAGE, Block, transpose_csr
from cgnn_amd.utils.hipgraph import StepGraph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 7              # sentinel of rows / buffers a kernel must not write
BIG = 1.0e4           # fills the padding columns of X: must never reach a result
BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
N_SRC = 257
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------ helpers
def _csr(deg, n_src, rng):
    """CSR (int32 rowptr, col) of the given row degrees with random source ids; some rows
    repeat one id, some hold source 0 and source n_src - 1."""
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
    return rp, col


def _degrees(L):
    d = [0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, L - 1, L, L + 1, L + 4, L + 8, L + 13,
         2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 5]
    # the list, the list reversed, and three more rows: 53 rows, no multiple of the
    # 4 * (64 / L) rows of a block for any L
    return d + d[::-1] + [2, L + 1, 0]


@functools.lru_cache(maxsize=None)
def _graph(L):
    rng = np.random.default_rng(700 + L)
    deg = _degrees(L)
    assert len(deg) == 53 and len(deg) % (4 * (64 // L)) != 0
    rp, col = _csr(deg, N_SRC, rng)
    assert 0 in col and N_SRC - 1 in col
    return dict(n=len(deg), rp=rp, col=col, rp_d=torch.from_numpy(rp).to(DEV), col_d=torch.from_numpy(col).to(DEV))


def _pool_ref(rp, col, X, F, is_min):
    """(Y, arg) of the definition from an fp64 numpy X.  ``np.argmax`` / ``np.argmin`` return
    the FIRST index of the extreme value and treat a NaN as the extreme (the first NaN
    wins): the scan rule, ties to the first edge, a NaN propagates.  test_nan_and_infinities
    spells the same rule out as a loop."""
    n = len(rp) - 1
    Y = np.zeros((n, F))
    A = np.full((n, F), -1, dtype=np.int64)
    for i in range(n):
        e0, e1 = int(rp[i]), int(rp[i + 1])
        if e1 > e0:
            v = X[col[e0:e1], :F]
            k = np.argmin(v, axis=0) if is_min else np.argmax(v, axis=0)
            Y[i] = v[k, np.arange(F)]
            A[i] = e0 + k
    return Y, A


def _pool_bwd_ref(rp, col, A, dY, n_src, F):
    """dX[j, f] = sum over the edges e = (i, j) of (A[i, f] == e) dY[i, f], in fp64."""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    sel = A[rows, :F] == np.arange(len(col))[:, None]
    dX = np.zeros((n_src, F))
    np.add.at(dX, col, np.where(sel, dY[rows, :F], 0.0))
    return dX


def _assert_same(got, exp, what):
    """Bit for bit, except that a NaN equals a NaN."""
    got, exp = got.double(), exp.double()
    gn, en = torch.isnan(got), torch.isnan(exp)
    g0, e0 = torch.nan_to_num(got, nan=0.0), torch.nan_to_num(exp, nan=0.0)
    if not (torch.equal(gn, en) and torch.equal(g0, e0)):
        bad = ((gn != en) | (g0 != e0)).nonzero()
        idx = tuple(int(x) for x in bad[0])
        raise AssertionError("%s: %d elements differ, first at %r: got %r, expected %r"
                             % (what, bad.shape[0], idx, float(got[idx]), float(exp[idx])))


# (F, ld, L): L lanes per row, from the written width; the last is two 512-column slabs
WIDTHS = [(8, 8, 8), (41, 48, 8), (64, 64, 8), (65, 72, 16), (128, 128, 16), (129, 136, 32),
          (256, 256, 32), (257, 264, 64), (512, 512, 64), (520, 528, 64)]
PAIRS = [(BF16, BF16), (BF16, F32), (F16, F16), (F16, F32), (F32, F32)]


def _features(kind, F, ld, seed, n=N_SRC):
    """fp64 [n, ld]: random normal values (a) or integers in [-2, 2] (b); padding = BIG."""
    rng = np.random.default_rng(seed)
    X = torch.full((n, ld), BIG, dtype=F64)
    if kind == "normal":
        X[:, :F] = torch.from_numpy(rng.standard_normal((n, F)))
    else:
        X[:, :F] = torch.from_numpy(rng.integers(-2, 3, (n, F)).astype(np.float64))
    return X


def _run_pool(g, X, F, ld, reduce, with_arg=True):
    """ops.pool into outputs with three sentinel rows; returns the CPU copies."""
    n = g["n"]
    ofull = torch.full((n + 3, ld), SENT, dtype=X.dtype, device=DEV)
    afull = torch.full((n + 3, ld), SENT, dtype=torch.int32, device=DEV)
    Y, A = ops.pool(g["rp_d"], g["col_d"], X, F, reduce=reduce, out=ofull[:n], arg=afull[:n] if with_arg else None,
                    with_arg=with_arg)
    assert Y.data_ptr() == ofull.data_ptr() and (A is None) == (not with_arg)
    return ofull.cpu(), afull.cpu()


# ------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("F,ld,L", WIDTHS)
def test_pool_forward_exact_over_row_lengths_widths_and_dtypes(F, ld, L):
    """pool_fwd_kernel against the definition, bit for bit: rows of every chunk / remainder
    class for L lanes per row, three storage types, max and min, random values (a) and
    tie-heavy integers (b, arg = the first edge holding the extreme value), zero / -1
    padding columns and empty rows, three sentinel rows past both outputs, padding columns of
    X that must not be read."""
    g = _graph(L)
    n, rp, col = g["n"], g["rp"], g["col"]
    empty = np.flatnonzero(np.diff(rp) == 0)
    assert empty.size >= 3
    for kind in ("normal", "ties"):
        Xd = _features(kind, F, ld, 4000 + F)
        for dt in (F32, BF16, F16):
            Xs = Xd.to(dt)                                     # rounded to the storage type
            X = Xs.to(DEV)
            for reduce in ("max", "min"):
                Yr, Ar = _pool_ref(rp, col, Xs.double().numpy(), F, reduce == "min")
                if kind == "ties":                             # most (row, feature) pairs have a tie
                    xs = Xs.double().numpy()
                    tied = [((xs[col[rp[i]:rp[i + 1]], :F] == Yr[i]).sum(0) > 1).mean()
                            for i in range(n) if rp[i + 1] - rp[i] >= 8]
                    assert np.mean(tied) > 0.6
                got, garg = _run_pool(g, X, F, ld, reduce)
                what = "%s %s %s F=%d" % (kind, dt, reduce, F)
                _assert_same(got[:n, :F], torch.from_numpy(Yr), what)
                assert torch.equal(garg[:n, :F].long(), torch.from_numpy(Ar)), what + ": arg"
                assert torch.all(got[:n, F:] == 0) and torch.all(garg[:n, F:] == -1), what + ": padding columns"
                assert torch.all(got[empty] == 0) and torch.all(garg[empty] == -1), what + ": empty rows"
                assert torch.all(got[n:] == SENT) and torch.all(garg[n:] == SENT), what + ": rows past n_rows"


# ------------------------------------------------------------------ 2. NaN and infinities
def _scan_ref(vals, is_min):
    """The replacement rule as a loop over one row's candidates: (value, position)."""
    best, pos = vals[0], 0
    for k, c in enumerate(vals[1:], 1):
        if (c < best if is_min else c > best) or (np.isnan(c) and not np.isnan(best)):
            best, pos = c, k
    return best, pos


@pytest.mark.parametrize("dt", [F32, BF16, F16])
def test_nan_and_infinities(dt):
    """Rows whose only finite competitors are the reduction's own identity (-inf for max,
    +inf for min), a row with one NaN in the middle, a row with the NaN first, two NaNs, and
    a row of 20 edges with a NaN in its second chunk (L = 8): value and arg follow the rule."""
    rows = [[-INF, -INF, -INF], [INF, INF], [-INF, 1.0, -INF], [INF, -1.0, INF], [1.0, NAN, 3.0], [NAN, 5.0, -5.0],
            [2.0, NAN, NAN, 9.0], [-INF, INF, -INF], [-INF], [INF], [NAN],
            [float(k % 5) for k in range(11)] + [NAN] + [float(k) for k in range(8)]]
    deg = [len(r) for r in rows]
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    nnz = int(rp[-1])
    col = np.arange(nnz, dtype=np.int32)[::-1].copy()          # edge e reads source nnz - 1 - e
    F, ld = 9, 16                                            # two lanes of features
    X = torch.full((nnz, ld), BIG, dtype=F64)
    flat = np.array([v for r in rows for v in r])
    X[torch.from_numpy(col.astype(np.int64)), :F] = torch.from_numpy(flat)[:, None].expand(nnz, F)
    X[:, 4] = torch.arange(nnz, dtype=F64) % 7                 # one plain column between them
    Xs = X.to(dt)
    for reduce in ("max", "min"):
        is_min = reduce == "min"
        Y, A = ops.pool(torch.from_numpy(rp).to(DEV), torch.from_numpy(col).to(DEV), Xs.to(DEV), F, reduce=reduce)
        Y, A = Y.cpu(), A.cpu()
        xs = Xs.double().numpy()
        for i, r in enumerate(rows):
            e0 = int(rp[i])
            for f in (0, 4, 8):
                best, pos = _scan_ref([xs[col[e0 + k], f] for k in range(len(r))], is_min)
                got = float(Y[i, f])
                assert (np.isnan(best) and np.isnan(got)) or got == best, (reduce, i, f, got, best)
                assert int(A[i, f]) == e0 + pos, (reduce, i, f, int(A[i, f]), e0 + pos)
        # spot checks of the rule itself: NaN rows give NaN at the first NaN edge
        assert torch.isnan(Y[4, 0]) and int(A[4, 0]) == int(rp[4]) + 1
        assert torch.isnan(Y[5, 0]) and int(A[5, 0]) == int(rp[5])
        assert torch.isnan(Y[6, 0]) and int(A[6, 0]) == int(rp[6]) + 1
        assert torch.isnan(Y[11, 0]) and int(A[11, 0]) == int(rp[11]) + 11
        # all candidates equal to the identity: that value, at the first edge
        i = 1 if is_min else 0
        assert float(Y[i, 0]) == (INF if is_min else -INF) and int(A[i, 0]) == int(rp[i])
        assert torch.all(Y[:, F:] == 0) and torch.all(A[:, F:] == -1)


# ------------------------------------------------------------------ 3. without the index
def test_without_arg_same_values_and_no_index_store():
    for (F, ld, L) in [(41, 48, 8), (129, 136, 32), (520, 528, 64)]:
        g = _graph(L)
        n = g["n"]
        X = _features("normal", F, ld, 50 + F).to(BF16).to(DEV)
        for reduce in ("max", "min"):
            y1, a1 = _run_pool(g, X, F, ld, reduce)
            y0, a0 = _run_pool(g, X, F, ld, reduce, with_arg=False)
            assert torch.equal(y0, y1)
            assert torch.all(a0 == SENT) and not torch.all(a1[:n] == SENT)
        Y, A = ops.pool(g["rp_d"], g["col_d"], X, F, reduce="min", with_arg=False)     # allocating form
        assert A is None and torch.equal(Y.cpu(), y1[:n])


# ------------------------------------------------------------------ 4. backward
@functools.lru_cache(maxsize=None)
def _bwd_graph(L):
    """The forward graph whose TRANSPOSE is the degree-list graph: 257 destination rows over
    53 sources, so the transposed CSR the backward kernel walks has exactly the row lengths
    of _degrees(L)."""
    g = _graph(L)
    n_src = g["n"]                                           # 53 sources
    rp, col = g["rp"], g["col"].copy()
    # source NEVER goes to destinations that two other sources reach too
    d = rp[NEVER + 1] - rp[NEVER]
    col[rp[NEVER]:rp[NEVER + 1]] = col[rp[NEVER - 2]:rp[NEVER]][:d]
    rp_f, col_f = transpose_csr(torch.from_numpy(rp), torch.from_numpy(col), N_SRC)
    rp_t, col_t, eperm = transpose_csr(rp_f, col_f, n_src, with_perm=True)
    assert torch.equal((rp_t[1:] - rp_t[:-1]).long(), torch.tensor(_degrees(L)))
    return dict(n=N_SRC, n_src=n_src, rp=rp_f.numpy(), col=col_f.numpy(), rp_d=rp_f.to(DEV), col_d=col_f.to(DEV),
                t=(rp_t.to(DEV), col_t.to(DEV), eperm.to(DEV)))


NEVER = 24            # the source with 3 L + 5 edges: made the worst candidate everywhere


@pytest.mark.parametrize("F,ld,L", WIDTHS)
def test_pool_backward_exact_over_row_lengths_widths_and_dtypes(F, ld, L):
    """pool_bwd_kernel against the fp64 sum, bit for bit, for the five type pairs: arg from
    the forward kernel on tie-heavy integer features (and equal to the reference's), dY
    integers in [-3, 3], three sentinel rows past n_src, zero padding columns; source NEVER
    is referenced by 3 L + 5 edges and selected by none, so its gradient row is exactly 0."""
    g = _bwd_graph(L)
    n, n_src, rp, col = g["n"], g["n_src"], g["rp"], g["col"]
    Xd = _features("ties", F, ld, 5000 + F, n=n_src)
    Xd[NEVER, :F] = -5.0
    # every destination that lists NEVER lists another source too: it never wins a max
    deg = np.diff(rp)
    rows = np.repeat(np.arange(n), deg)
    for i in np.unique(rows[col == NEVER]):
        assert (col[rp[i]:rp[i + 1]] != NEVER).any()
    rng = np.random.default_rng(6000 + F)
    dYd = torch.full((n, ld), BIG, dtype=F64)                  # padding of dY must not be read either
    dYd[:, :F] = torch.from_numpy(rng.integers(-3, 4, (n, F)).astype(np.float64))
    Yr, Ar = _pool_ref(rp, col, Xd.numpy(), F, False)
    _, A = ops.pool(g["rp_d"], g["col_d"], Xd.float().to(DEV), F, reduce="max")
    assert torch.equal(A.cpu()[:, :F].long(), torch.from_numpy(Ar))
    ref = torch.from_numpy(_pool_bwd_ref(rp, col, Ar, dYd.numpy(), n_src, F))
    # at most 3 * 64 + 5 terms of magnitude <= 3 per sum: exact in fp32 in any order
    assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) <= 3 * (3 * 64 + 5)
    assert (col == NEVER).sum() == 3 * L + 5 and torch.all(ref[NEVER] == 0) and float(ref.abs().sum()) > 0
    rp_t, col_t, eperm = g["t"]
    for ydt, xdt in PAIRS:
        dY = dYd.to(ydt).to(DEV)
        full = torch.full((n_src + 3, ld), SENT, dtype=xdt, device=DEV)
        out = ops.pool_bwd(rp_t, col_t, eperm, A, dY, F, out=full[:n_src])
        assert out.data_ptr() == full.data_ptr()
        got = full.cpu()
        what = "pool_bwd %s->%s F=%d" % (ydt, xdt, F)
        _assert_same(got[:n_src, :F], ref.to(xdt), what)
        assert torch.all(got[:n_src, F:] == 0), what + ": padding columns"
        assert torch.all(got[n_src:] == SENT), what + ": rows past n_src"
        assert torch.all(got[NEVER] == 0), what + ": a source never selected"


# ------------------------------------------------------------------ 4b. past the second slab
@functools.lru_cache(maxsize=None)
def _small_graph():
    """9 rows over 9 sources, 40 edges, one row empty; with its transpose."""
    rng = np.random.default_rng(43)
    deg = [3, 0, 1, 9, 4, 5, 7, 9, 2]
    rp, col = _csr(deg, 9, rng)
    assert col.size == 40
    rp_t, col_t, eperm = transpose_csr(torch.from_numpy(rp), torch.from_numpy(col), 9, with_perm=True)
    return dict(n=9, rp=rp, col=col, rp_d=torch.from_numpy(rp).to(DEV), col_d=torch.from_numpy(col).to(DEV),
                t=(rp_t.to(DEV), col_t.to(DEV), eperm.to(DEV)))


# (F, ld of X / Y / dY / dX, ld of arg).  (1030, 1032): a third 512-column slab holding 6
# features and 2 padding columns; (500, 1032): slabs two and three hold padding only;
# (8, 8, 520): a second slab that writes 8 padding columns of arg and nothing of Y
@pytest.mark.parametrize("F,ld,ldarg", [(1030, 1032, 1032), (500, 1032, 1032), (8, 8, 520)])
def test_pool_forward_and_backward_exact_past_the_second_slab(F, ld, ldarg):
    g = _small_graph()
    n, rp, col = g["n"], g["rp"], g["col"]
    Xd = _features("ties", F, ld, 7000 + F, n=n)
    A_max = None
    for dt in (F32, BF16, F16):
        Xs = Xd.to(dt)
        for reduce in ("max", "min"):
            Yr, Ar = _pool_ref(rp, col, Xs.double().numpy(), F, reduce == "min")
            ofull = torch.full((n + 3, ld), SENT, dtype=dt, device=DEV)
            afull = torch.full((n + 3, ldarg), SENT, dtype=torch.int32, device=DEV)
            ops.pool(g["rp_d"], g["col_d"], Xs.to(DEV), F, reduce=reduce, out=ofull[:n], arg=afull[:n])
            got, garg = ofull.cpu(), afull.cpu()
            what = "%s %s F=%d ldarg=%d" % (dt, reduce, F, ldarg)
            _assert_same(got[:n, :F], torch.from_numpy(Yr), what)
            assert torch.equal(garg[:n, :F].long(), torch.from_numpy(Ar)), what + ": arg"
            assert torch.all(got[:n, F:] == 0) and torch.all(garg[:n, F:] == -1), what + ": padding columns"
            assert torch.all(got[1] == 0) and torch.all(garg[1] == -1), what + ": the empty row"
            assert torch.all(got[n:] == SENT) and torch.all(garg[n:] == SENT), what + ": past the last row's stride"
            if dt == F32 and reduce == "max":
                A_max, Ar_max = afull[:n], Ar
    rng = np.random.default_rng(7100 + F)
    dYd = torch.full((n, ld), BIG, dtype=F64)
    dYd[:, :F] = torch.from_numpy(rng.integers(-3, 4, (n, F)).astype(np.float64))
    ref = torch.from_numpy(_pool_bwd_ref(rp, col, Ar_max, dYd.numpy(), n, F))
    assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) <= 3 * 40 and float(ref.abs().sum()) > 0
    rp_t, col_t, eperm = g["t"]
    for ydt, xdt in PAIRS:
        full = torch.full((n + 3, ld), SENT, dtype=xdt, device=DEV)
        ops.pool_bwd(rp_t, col_t, eperm, A_max, dYd.to(ydt).to(DEV), F, out=full[:n])
        got = full.cpu()
        what = "pool_bwd %s->%s F=%d ldarg=%d" % (ydt, xdt, F, ldarg)
        _assert_same(got[:n, :F], ref.to(xdt), what)
        assert torch.all(got[:n, F:] == 0), what + ": padding columns"
        assert torch.all(got[n:] == SENT), what + ": past the last row's stride"


# ------------------------------------------------------------------ 5. duplicate edges
def test_duplicate_edges_are_not_double_counted():
    """A row lists source 1 three times (equal values, so the first edge wins the tie): the
    gradient lands once and equals dY, not 3 dY.  A second row lists it twice among others."""
    rp = torch.tensor([0, 3, 7], dtype=torch.int32, device=DEV)
    col = torch.tensor([1, 1, 1, 0, 1, 2, 1], dtype=torch.int32, device=DEV)
    F = 16
    x = torch.zeros(3, F, device=DEV)
    x[1] = 2.0
    x[2, 8:] = 3.0                                          # row 1: source 1 wins f < 8, source 2 the rest
    x.requires_grad_()
    g = WeightedGraph(rp, col, torch.ones(7, device=DEV), n_src=3)
    y = pool_aggregate(x, g)
    dy = torch.arange(1.0, 2 * F + 1, device=DEV).view(2, F)
    y.backward(dy)
    exp_y = torch.full((2, F), 2.0)
    exp_y[1, 8:] = 3.0
    assert torch.equal(y.detach().cpu(), exp_y)
    dyc = dy.cpu()
    exp = torch.zeros(3, F)
    exp[1] = dyc[0]
    exp[1, :8] += dyc[1, :8]
    exp[2, 8:] = dyc[1, 8:]
    assert torch.equal(x.grad.cpu(), exp)


# ------------------------------------------------------------------ 6. autograd
def test_pool_aggregate_on_the_three_graph_types():
    """pool_aggregate forward and backward on a WeightedGraph, a NormGraph and a sage.Block:
    the fp64 reference bit for bit; min equals the negated max of -x."""
    g = _graph(16)
    n, rp, col = g["n"], g["rp"], g["col"]
    F = 20
    rng = np.random.default_rng(21)
    # a square graph for the NormGraph: the first 53 sources only
    sq_col = (col % n).astype(np.int32)
    cases = [
        ("weighted", WeightedGraph(g["rp_d"], g["col_d"], torch.ones(col.size, device=DEV), n_src=N_SRC), col, N_SRC),
        ("norm", NormGraph(g["rp_d"], torch.from_numpy(sq_col).to(DEV), torch.ones(n, device=DEV)), sq_col, n),
        ("block", Block(rp, col, N_SRC, DEV), col, N_SRC),
    ]
    for name, graph, c, n_src in cases:
        xd = torch.from_numpy(rng.integers(-2, 3, (n_src, F)).astype(np.float64))
        gd = torch.from_numpy(rng.integers(-3, 4, (n, F)).astype(np.float64))
        for dt in (F32, BF16):
            for reduce in ("max", "min"):
                Yr, Ar = _pool_ref(rp, c, xd.numpy(), F, reduce == "min")
                dXr = torch.from_numpy(_pool_bwd_ref(rp, c, Ar, gd.numpy(), n_src, F))
                assert torch.equal(dXr.float().double(), dXr)
                x = xd.to(dt).to(DEV).requires_grad_()
                y = pool_aggregate(x, graph, reduce)
                assert y.dtype == dt and y.shape == (n, F)
                y.backward(gd.to(dt).to(DEV))
                what = "%s %s %s" % (name, dt, reduce)
                _assert_same(y.detach().cpu(), torch.from_numpy(Yr), what)
                _assert_same(x.grad.cpu(), dXr.to(dt), what + " dx")
        xn = torch.from_numpy(rng.standard_normal((n_src, F))).float().to(DEV)
        assert torch.equal(pool_aggregate(xn, graph, "min"), -pool_aggregate(-xn, graph, "max"))
        assert graph.transposed_perm() is graph.transposed_perm()


# ------------------------------------------------------------------ 7. capture
def test_pool_forward_and_backward_in_a_captured_graph():
    """pool + pool_bwd into preallocated buffers, captured and replayed twice with new inputs
    written into the captured buffers: the eager bits each time."""
    g = _bwd_graph(16)
    n, n_src, F, ld = g["n"], g["n_src"], 100, 104
    rp_t, col_t, eperm = g["t"]
    X = torch.zeros(n_src, ld, dtype=BF16, device=DEV)
    dY = torch.zeros(n, ld, dtype=BF16, device=DEV)
    Y = torch.empty(n, ld, dtype=BF16, device=DEV)
    A = torch.empty(n, ld, dtype=torch.int32, device=DEV)
    dX = torch.empty(n_src, ld, dtype=BF16, device=DEV)

    def step():
        ops.pool(g["rp_d"], g["col_d"], X, F, reduce="max", out=Y, arg=A)
        ops.pool_bwd(rp_t, col_t, eperm, A, dY, F, out=dX)

    def inputs(seed):
        X.copy_(_features("ties", F, ld, seed, n=n_src).to(BF16))
        rng = np.random.default_rng(seed + 1)
        dY.zero_()
        dY[:, :F] = torch.from_numpy(rng.integers(-3, 4, (n, F)).astype(np.float32)).to(BF16).to(DEV)

    eager = []
    for seed in (31, 33):
        inputs(seed)
        step()
        torch.cuda.synchronize()
        eager.append((Y.clone(), A.clone(), dX.clone()))
    assert not torch.equal(eager[0][2], eager[1][2])
    Yr, Ar = _pool_ref(g["rp"], g["col"], X.cpu().double().numpy(), F, False)
    _assert_same(eager[1][0].cpu()[:, :F], torch.from_numpy(Yr), "eager forward")
    sg = StepGraph(step, warmup=1, device=torch.device(DEV))
    sg()                                                   # eager warm-up
    for k, seed in enumerate((31, 33)):
        inputs(seed)
        Y.fill_(SENT)
        A.fill_(SENT)
        dX.fill_(SENT)
        sg()
        assert sg.graph is not None
        torch.cuda.synchronize()
        y0, a0, d0 = eager[k]
        assert torch.equal(Y, y0) and torch.equal(A, a0) and torch.equal(dX, d0), "replay %d" % k


# ------------------------------------------------------------------ 8. launcher codes
def test_launcher_codes_and_empty_graphs():
    hip = native.hip()
    g = _graph(8)
    n = g["n"]
    st = torch.cuda.current_stream().cuda_stream
    X = torch.ones(N_SRC, 16, device=DEV)
    Y = torch.full((n, 16), float(SENT), device=DEV)
    A = torch.full((n, 16), SENT, dtype=torch.int32, device=DEV)
    rp, col = g["rp_d"].data_ptr(), g["col_d"].data_ptr()

    def fwd(F=16, ldx=16, ldy=16, lda=16, t=0, n_rows=n, arg=A.data_ptr()):
        hip.gnn_pool_fwd(rp, col, X.data_ptr(), Y.data_ptr(), arg, n_rows, F, ldx, ldy, lda, t, 0, st)

    # the weighted bindings raise RuntimeError carrying the launcher's code
    with pytest.raises(RuntimeError, match="-5") as weighted:
        ops.wspmm(g["rp_d"], g["col_d"], torch.ones(g["col"].size, device=DEV), X, 16, out=Y.to(BF16))
    for kw in (dict(ldx=12, F=12), dict(ldy=12, F=12), dict(lda=12, F=12), dict(F=17), dict(F=-1)):
        with pytest.raises(RuntimeError, match="-3") as ei:          # a stride no multiple of 8; F > ld
            fwd(**kw)
        assert ei.type is weighted.type
    with pytest.raises(RuntimeError, match="-5"):                    # not a storage type
        fwd(t=3)
    fwd(lda=12, F=12, ldx=16, arg=0)                                 # no arg: its stride is not looked at
    Y.fill_(SENT)
    rp_t, col_t, eperm = transpose_csr(g["rp_d"], g["col_d"], N_SRC, with_perm=True)
    dX = torch.full((N_SRC, 16), float(SENT), device=DEV)

    def bwd(F=16, lda=16, lddy=16, lddx=16, tdy=0, tdx=0, n_src=N_SRC):
        hip.gnn_pool_bwd(rp_t.data_ptr(), col_t.data_ptr(), eperm.data_ptr(), A.data_ptr(), lda, Y.data_ptr(), lddy,
                         dX.data_ptr(), lddx, n_src, F, tdy, tdx, st)

    for kw in (dict(lda=12, F=12), dict(lddy=12, F=12), dict(lddx=12, F=12), dict(F=17)):
        with pytest.raises(RuntimeError, match="-3"):
            bwd(**kw)
    for tdy, tdx in ((0, 1), (1, 2), (2, 1), (0, 2), (3, 0)):        # pairs that are not compiled
        with pytest.raises(RuntimeError, match="-5") as ei:
            bwd(tdy=tdy, tdx=tdx)
        assert ei.type is weighted.type
    with pytest.raises(RuntimeError, match="-5"):                    # the same through ops
        ops.pool_bwd(rp_t, col_t, eperm, A, Y, 16, out=dX.to(BF16))
    with pytest.raises(RuntimeError, match="-3"):
        ops.pool(g["rp_d"], g["col_d"], torch.ones(N_SRC, 12, device=DEV), 12)
    with pytest.raises(TypeError):                                   # fp64 is not a kernel type
        ops.pool(g["rp_d"], g["col_d"], X.double(), 16)
    # n_rows = 0: code 0 and nothing is launched or written
    fwd(n_rows=0)
    bwd(n_src=0)
    torch.cuda.synchronize()
    assert torch.all(Y == SENT) and torch.all(A == SENT) and torch.all(dX == SENT)
    # rows but no edges: col / col_t / eperm are empty tensors (null pointers)
    n0, F = 9, 24
    rp0 = torch.zeros(n0 + 1, dtype=torch.int32, device=DEV)
    col0 = torch.zeros(0, dtype=torch.int32, device=DEV)
    x0 = torch.ones(5, F, dtype=BF16, device=DEV)
    y0, a0 = ops.pool(rp0, col0, x0, F)
    assert torch.all(y0 == 0) and torch.all(a0 == -1)
    t0 = transpose_csr(rp0, col0, 5, with_perm=True)
    d0 = ops.pool_bwd(t0[0], t0[1], t0[2], a0, torch.ones(n0, F, dtype=BF16, device=DEV), F)
    assert d0.shape == (5, F) and torch.all(d0 == 0)
    xg = torch.ones(5, F, device=DEV, requires_grad=True)
    pool_aggregate(xg, Block(rp0.cpu().numpy(), col0.cpu().numpy(), 5, DEV)).sum().backward()
    assert torch.all(xg.grad == 0)


# ------------------------------------------------------------------ 9. SAGE(aggr="max")
def _bf16_exact(t):
    return torch.equal(t.detach().double().to(BF16).double(), t.detach().double())


def test_sage_max_gpu_matches_fp64_cpu():
    """One forward / backward of SAGE(aggr="max") on a three-block toy batch against the same
    module in fp64 on the CPU, within the tolerance of test_sage_aggregate_gpu_matches_cpu
    (rtol = atol = 1e-5, the unfused GPU-vs-CPU test of the "mean" aggregator).

    The GPU module multiplies in bf16 and stores the hidden layers in bf16, so that tolerance
    can only hold where bf16 loses nothing: the inputs are integers in [-1, 1], the weights
    in {-1, 0, 1} (two non-zeros per row in layer 2), the cotangent in {-1, 0, 1}.  Then
    every hidden value is an integer <= 256 (asserted on the CPU run), and every gradient
    that is cast to bf16 is an integer bounded by (1 + 2) r3 (1 + 4) r2 <= 256, r the
    largest row sum of |[W_self; W_neigh]| of a layer, 2 destinations in block 3 and 4 in
    block 2 (a hidden row collects its own gradient and one per destination that selected
    it; asserted below): the two runs compute the same integers."""
    rng = np.random.default_rng(17)
    sizes = [12, 7, 4, 2]
    raw = []
    for ns, nd in zip(sizes[:-1], sizes[1:]):
        deg = rng.integers(0, 5, nd)
        deg[0] = 3
        rp = np.concatenate([[0], np.cumsum(deg)])
        raw.append((rp, rng.integers(0, ns, int(rp[-1])), ns))
    dims = [8, 8, 8, 4]
    ints = lambda lo, hi, shape: torch.from_numpy(rng.integers(lo, hi + 1, shape).astype(np.float64))
    x = ints(-1, 1, (12, 8))
    cot = ints(-1, 1, (2, 4))
    Ws = []
    for k, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        ws, wn, bias = ints(-1, 1, (a, b)), ints(-1, 1, (a, b)), ints(-1, 1, (b,))
        if k == 1:                                           # two non-zeros per row in each half
            keep = torch.zeros(a, b)
            for r in range(a):
                keep[r, [(r + 0) % b, (r + 3) % b]] = 1
            ws, wn = ws * keep, wn * keep
        Ws.append((ws, wn, bias))
    r2 = float(torch.cat([Ws[1][0], Ws[1][1]], 0).abs().sum(1).max())
    r3 = float(torch.cat([Ws[2][0], Ws[2][1]], 0).abs().sum(1).max())
    assert (1 + sizes[3]) * r3 * (1 + sizes[2]) * r2 <= 256

    def run(dev, dt):
        model = SAGE(8, 8, 4, layers=3, dropout=0.0, seed=0, aggr="max").to(dev).to(dt)
        with torch.no_grad():
            for k, (ws, wn, bias) in enumerate(Ws):
                model.w_self[k].copy_(ws)
                model.w_neigh[k].copy_(wn)
                model.bias[k].copy_(bias)
        blocks = [Block(rp, col, ns, dev) for rp, col, ns in raw]
        model.train()
        out = model(x.to(dt).to(dev), blocks)
        out.backward(cot.to(out.dtype).to(dev))
        return model, blocks, out.detach().double().cpu(), [p.grad.double().cpu() for p in model.parameters()]

    cpu_model, cpu_blocks, out_c, grads_c = run("cpu", F64)
    h = x
    for k in range(2):                                       # the hidden layers of the CPU run
        h = cpu_model.layer(k, h, cpu_blocks[k], False).detach().double()
        assert _bf16_exact(h) and float(h.abs().max()) <= 256
    _, _, out_g, grads_g = run(DEV, F32)
    np.testing.assert_allclose(out_g.numpy(), out_c.numpy(), rtol=1e-5, atol=1e-5)
    assert float(out_c.abs().max()) > 0 and len(grads_c) == 9
    for gg, gc in zip(grads_g, grads_c):
        np.testing.assert_allclose(gg.numpy(), gc.numpy(), rtol=1e-5, atol=1e-5)
    assert sum(float(gc.abs().sum()) > 0 for gc in grads_c) >= 7
