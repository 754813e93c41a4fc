"""Exact oracle tests of the edge-weighted HIP kernels (gnn_wspmm.hip: wspmm_kernel,
sddmm_kernel) and of the layer API on top of them.

Every reference is computed here, in fp64, from a dense weighted matrix of the graph --
never through the CPU branches of ``ops``.  Features are integers in [-3, 3], edge values
come from {+-0.25, +-0.5, +-1, +-2} plus exact zeros, scales from {0.5, 1, 2}, bias terms
are small integers: every product and partial sum is a multiple of 2^-5 well below 2^19,
exactly representable in fp32 whatever the order of the multiply-adds (fused or not).  Each
test asserts that with an fp32 round trip of its reference and a magnitude bound.  The
comparison is ``torch.equal`` against the fp64 result cast to the output type.
"""
import functools

import numpy as np
import pytest
import torch

from cgnn_amd.gnn import layers, ops
from cgnn_amd.gnn.layers import GCN, GCNConv, NormGraph, WeightedGraph, weighted_aggregate
from cgnn_amd.utils.hipgraph import StepGraph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 7.0            # sentinel of rows / buffers a kernel must not write
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


def _dense(rp, col, val, n_src):
    """Dense fp64 matrix A[i, j] = sum of the values of the entries j of row i."""
    A = torch.zeros(rp.numel() - 1, n_src, dtype=F64)
    A.index_put_((_rows(rp), col.long()), val.double(), accumulate=True)
    return A


def _ints(rng, lo, hi, shape):
    return torch.from_numpy(rng.integers(lo, hi + 1, shape).astype(np.float64))


def _pow2(rng, n):
    return torch.from_numpy(rng.choice([0.5, 1.0, 2.0], n))


def _exact(ref, bound):
    """The reference survives a round trip through fp32 and stays below ``bound``."""
    return torch.equal(ref.float().double(), ref) and float(ref.abs().max()) < bound


def _assert_same(got, exp, what):
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
    return dict(n=len(deg), rp=rp, col=col, val=val, rp_d=rp.to(DEV), col_d=col.to(DEV), val_d=val.to(DEV),
                A=_dense(rp, col, val, N_SRC), rs=_pow2(rng, len(deg)), cs=_pow2(rng, N_SRC))


# (F, ld, L): L lanes per row, from the written width; the last is two 512-column slabs
WIDTHS = [(8, 8, 8), (41, 48, 8), (64, 64, 8), (65, 72, 16), (128, 128, 16), (129, 136, 32),
          (256, 256, 32), (257, 264, 64), (512, 512, 64), (520, 528, 64)]
PAIRS = [(BF16, BF16), (BF16, F32), (F16, F16), (F16, F32), (F32, F32)]
# (row scale, column scale, bias, relu)
CONFIGS = [(False, False, False, False), (True, True, True, True), (True, False, True, False),
           (False, True, False, True)]


def _features(F, ld, seed):
    rng = np.random.default_rng(seed)
    Xd = torch.zeros(N_SRC, ld, dtype=F64)
    Xd[:, :F] = _ints(rng, -3, 3, (N_SRC, F))
    return Xd, _ints(rng, -2, 2, (F,))


def _wspmm_ref(g, Xd, bias, F, cfg):
    use_rs, use_cs, use_bias, relu = cfg
    A = g["A"] * g["cs"][None, :] if use_cs else g["A"]
    ref = A @ Xd[:, :F]
    if use_rs:
        ref = ref * g["rs"][:, None]
    if use_bias:
        ref = ref + bias
    if relu:
        ref = ref.clamp_min(0)
    # |value * scale * feature| <= 12 per edge, <= 3 * 64 + 5 edges, row scale <= 2
    assert _exact(ref, 8192)
    return ref


# ------------------------------------------------------------------ 1, 2. wspmm
@pytest.mark.parametrize("F,ld,L", WIDTHS)
def test_wspmm_exact_over_row_lengths_widths_and_dtypes(F, ld, L):
    """wspmm_kernel against the dense fp64 product, bit for bit: rows of every chunk /
    remainder class for L lanes per row, the five type pairs, four epilogues, three sentinel
    rows past the output, zero padding columns -- and (2) the same sums from a shuffled
    value array through a non-identity edge permutation."""
    g = _graph(L)
    n = g["n"]
    Xd, bias = _features(F, ld, 2000 + F)
    rs_d, cs_d, bias_d = g["rs"].float().to(DEV), g["cs"].float().to(DEV), bias.float().to(DEV)
    nnz = g["col"].numel()
    perm = torch.from_numpy(np.random.default_rng(F).permutation(nnz)).to(torch.int32)
    assert not torch.equal(perm, torch.arange(nnz, dtype=torch.int32))
    shuffled = torch.empty(nnz)
    shuffled[perm.long()] = g["val"]
    perm_d, shuffled_d = perm.to(DEV), shuffled.to(DEV)
    for xdt, ydt in PAIRS:
        X = Xd.to(xdt).to(DEV)
        for cfg in CONFIGS:
            use_rs, use_cs, use_bias, relu = cfg
            exp = torch.zeros(n, ld, dtype=F64)
            exp[:, :F] = _wspmm_ref(g, Xd, bias, F, cfg)
            exp = exp.to(ydt)
            kw = dict(rscale=rs_d if use_rs else None, cscale=cs_d if use_cs else None,
                      bias=bias_d if use_bias else None, relu=relu)
            for vals, ep in ((g["val_d"], None), (shuffled_d, perm_d)):
                full = torch.full((n + 3, ld), SENT, dtype=ydt, device=DEV)
                ops.wspmm(g["rp_d"], g["col_d"], vals, X, F, eperm=ep, out=full[:n], **kw)
                got = full.cpu()
                what = "%s->%s rs=%d cs=%d bias=%d relu=%d eperm=%d" % (xdt, ydt, use_rs, use_cs, use_bias, relu,
                                                                       ep is not None)
                _assert_same(got[:n], exp, what)
                assert torch.all(got[n:] == SENT), what + ": rows past n_rows written"
                assert torch.all(got[:n, F:] == 0), what + ": padding columns"


# ------------------------------------------------------------------ 3. transpose identity
def test_wspmm_over_the_transposed_csr_is_the_transposed_product():
    """wspmm over ``transposed()`` with its edge permutation equals A^T times the input,
    on a rectangular graph (53 rows over 257 sources), scales swapped."""
    g = _graph(16)
    n, F = g["n"], 40
    wg = WeightedGraph(g["rp_d"], g["col_d"], g["val_d"], n_src=N_SRC, rscale=g["rs"].float().to(DEV),
                       cscale=g["cs"].float().to(DEV))
    rp_t, col_t, eperm = wg.transposed()
    assert rp_t.numel() == N_SRC + 1 and n != N_SRC
    rng = np.random.default_rng(5)
    Gd = _ints(rng, -3, 3, (n, F))
    ref = (g["rs"][:, None] * g["A"] * g["cs"][None, :]).t() @ Gd
    assert _exact(ref, 8192)
    for dt in (F32, BF16, F16):
        got = ops.wspmm(rp_t, col_t, wg.val, Gd.to(dt).to(DEV), F, rscale=wg.cscale, cscale=wg.rscale, eperm=eperm)
        _assert_same(got.cpu(), ref.to(dt), "transposed %s" % dt)
    # and through the autograd function: d/dx of sum(G * (A x))
    x = torch.zeros(N_SRC, F, device=DEV, requires_grad=True)
    weighted_aggregate(x, wg).backward(Gd.float().to(DEV))
    _assert_same(x.grad.cpu(), ref.float(), "weighted_aggregate dx")


# ------------------------------------------------------------------ 4. sddmm
@pytest.mark.parametrize("F,ld,L", WIDTHS)
def test_sddmm_exact_over_row_lengths_widths_and_dtypes(F, ld, L):
    """sddmm_kernel against rscale_i cscale_j (A B^T)[i, col[e]] per edge, bit for bit;
    the padding columns of A and B hold a value that must not be read; a sentinel tail past
    nnz stays untouched; duplicate edges of a row get equal results."""
    g = _graph(L)
    n, nnz = g["n"], g["col"].numel()
    rng = np.random.default_rng(3000 + F)
    Ad = torch.full((n, ld), 5.0, dtype=F64)
    Bd = torch.full((N_SRC, ld), 5.0, dtype=F64)
    Ad[:, :F] = _ints(rng, -3, 3, (n, F))
    Bd[:, :F] = _ints(rng, -3, 3, (N_SRC, F))
    rows, colj = _rows(g["rp"]), g["col"].long()
    P = Ad[:, :F] @ Bd[:, :F].t()
    rs_d, cs_d = g["rs"].float().to(DEV), g["cs"].float().to(DEV)
    # duplicate edges: the rows that repeat one source id
    dup = [(int(g["rp"][i]), int(g["rp"][i + 1])) for i in range(n) if i % 5 == 1 and i % 7 != 2
           and int(g["rp"][i + 1]) - int(g["rp"][i]) >= 2]
    assert dup
    for dt in (F32, BF16, F16):
        A, B = Ad.to(dt).to(DEV), Bd.to(dt).to(DEV)
        for use_s in (False, True):
            ref = P[rows, colj]
            if use_s:
                ref = ref * g["rs"][rows] * g["cs"][colj]
            assert _exact(ref, 9 * 520 * 4 + 1)
            out = torch.full((nnz + 5,), SENT, device=DEV)
            ops.sddmm(g["rp_d"], g["col_d"], A, B, F, rscale=rs_d if use_s else None,
                      cscale=cs_d if use_s else None, out=out)
            got = out.cpu()
            what = "sddmm %s scales=%d" % (dt, use_s)
            _assert_same(got[:nnz], ref.float(), what)
            assert torch.all(got[nnz:] == SENT), what + ": tail past nnz written"
            for e0, e1 in dup:
                assert torch.all(got[e0:e1] == got[e0]), what + ": duplicate edges differ"


# ------------------------------------------------------------------ 4b. past the second slab
@functools.lru_cache(maxsize=None)
def _small_graph():
    """9 rows, 40 edges, one row empty."""
    rng = np.random.default_rng(41)
    deg = [3, 0, 1, 9, 4, 5, 7, 9, 2]
    rp, col, val = _csr(deg, N_SRC, rng)
    assert col.numel() == 40
    return dict(n=len(deg), rp=rp, col=col, val=val, rp_d=rp.to(DEV), col_d=col.to(DEV), val_d=val.to(DEV),
                A=_dense(rp, col, val, N_SRC), rs=_pow2(rng, len(deg)), cs=_pow2(rng, N_SRC))


# (1030, 1032): a third 512-column slab holding 6 features and 2 padding columns;
# (500, 1032): slabs two and three hold padding only, the third is 8 columns wide
@pytest.mark.parametrize("F,ld", [(1030, 1032), (500, 1032)])
def test_wspmm_and_sddmm_exact_past_the_second_slab(F, ld):
    g = _small_graph()
    n, nnz = g["n"], g["col"].numel()
    Xd, bias = _features(F, ld, 4000 + F)
    rs_d, cs_d, bias_d = g["rs"].float().to(DEV), g["cs"].float().to(DEV), bias.float().to(DEV)
    for xdt, ydt in PAIRS:
        X = Xd.to(xdt).to(DEV)
        for cfg in (CONFIGS[0], CONFIGS[1]):
            use_rs, use_cs, use_bias, relu = cfg
            exp = torch.zeros(n, ld, dtype=F64)
            exp[:, :F] = _wspmm_ref(g, Xd, bias, F, cfg)
            full = torch.full((n + 3, ld), SENT, dtype=ydt, device=DEV)
            ops.wspmm(g["rp_d"], g["col_d"], g["val_d"], X, F, rscale=rs_d if use_rs else None,
                      cscale=cs_d if use_cs else None, bias=bias_d if use_bias else None, relu=relu, out=full[:n])
            got = full.cpu()
            what = "%s->%s F=%d epilogue=%d" % (xdt, ydt, F, use_rs)
            _assert_same(got[:n], exp.to(ydt), what)
            assert torch.all(got[:n, F:] == 0), what + ": padding columns"
            assert torch.all(got[n:] == SENT), what + ": written past the last row's stride"
    rng = np.random.default_rng(4100 + F)
    Ad = torch.full((n, ld), 5.0, dtype=F64)
    Bd = torch.full((N_SRC, ld), 5.0, dtype=F64)
    Ad[:, :F] = _ints(rng, -3, 3, (n, F))
    Bd[:, :F] = _ints(rng, -3, 3, (N_SRC, F))
    rows, colj = _rows(g["rp"]), g["col"].long()
    ref = (Ad[:, :F] @ Bd[:, :F].t())[rows, colj] * g["rs"][rows] * g["cs"][colj]
    assert _exact(ref, 9 * 1032 * 4 + 1)
    for dt in (F32, BF16, F16):
        out = torch.full((nnz + 5,), SENT, device=DEV)
        ops.sddmm(g["rp_d"], g["col_d"], Ad.to(dt).to(DEV), Bd.to(dt).to(DEV), F, rscale=rs_d, cscale=cs_d, out=out)
        got = out.cpu()
        _assert_same(got[:nnz], ref.float(), "sddmm %s F=%d" % (dt, F))
        assert torch.all(got[nnz:] == SENT), "sddmm: tail past nnz written"


# ------------------------------------------------------------------ 5. edge cases
def test_graph_with_rows_but_no_edges():
    n, F = 9, 24
    rp = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    col = torch.zeros(0, dtype=torch.int32, device=DEV)
    val = torch.zeros(0, device=DEV)
    X = torch.ones(5, F, dtype=BF16, device=DEV)
    bias = torch.arange(F, dtype=F32, device=DEV) - 3
    y = ops.wspmm(rp, col, val, X, F, bias=bias, out_dtype=F32)
    assert torch.equal(y.cpu(), (torch.arange(F, dtype=F32) - 3).expand(n, F))
    y = ops.wspmm(rp, col, val, X, F, rscale=torch.ones(n, device=DEV), cscale=torch.ones(5, device=DEV))
    assert torch.all(y == 0)
    out = torch.full((4,), SENT, device=DEV)
    ops.sddmm(rp, col, torch.ones(n, F, dtype=BF16, device=DEV), X, F, out=out)
    assert torch.all(out == SENT)
    # no rows at all
    ops.wspmm(rp[:1], col, val, X, F, out=torch.empty(0, F, dtype=BF16, device=DEV))
    ops.sddmm(rp[:1], col, torch.ones(0, F, dtype=BF16, device=DEV), X, F, out=out)
    torch.cuda.synchronize()
    assert torch.all(out == SENT)


def test_one_row_and_single_edge():
    rng = np.random.default_rng(8)
    F = 20
    Xd = torch.zeros(N_SRC, 24, dtype=F64)
    Xd[:, :F] = _ints(rng, -3, 3, (N_SRC, F))
    Ad = torch.zeros(1, 24, dtype=F64)
    Ad[:, :F] = _ints(rng, -3, 3, (1, F))
    for deg in (1, 19):                                  # a single edge; one row of 19
        rp, col, val = _csr([deg], N_SRC, rng)
        A = _dense(rp, col, val, N_SRC)
        ref = A @ Xd[:, :F]
        assert _exact(ref, 4096)
        full = torch.full((4, 24), SENT, device=DEV)
        ops.wspmm(rp.to(DEV), col.to(DEV), val.to(DEV), Xd.float().to(DEV), F, out=full[:1])
        got = full.cpu()
        _assert_same(got[:1, :F], ref.float(), "n_rows = 1, degree %d" % deg)
        assert torch.all(got[1:] == SENT) and torch.all(got[:1, F:] == 0)
        out = torch.full((deg + 2,), SENT, device=DEV)
        ops.sddmm(rp.to(DEV), col.to(DEV), Ad.float().to(DEV), Xd.float().to(DEV), F, out=out)
        refd = (Ad[:, :F] @ Xd[:, :F].t())[0, col.long()]
        _assert_same(out.cpu()[:deg], refd.float(), "sddmm n_rows = 1, degree %d" % deg)
        assert torch.all(out.cpu()[deg:] == SENT)


@pytest.mark.parametrize("L,F", [(8, 41), (16, 128), (32, 129), (64, 257)])
def test_a_row_does_not_depend_on_its_launch_mates(L, F):
    """A row's wspmm output and its edges' sddmm outputs are the same bits in the 53-row
    graph and in a graph that holds that row alone.  Non-exact inputs here (random normal
    features and values), so any change in the order of a row's multiply-adds would show."""
    g = _graph(L)
    n, ld = g["n"], -(-F // 8) * 8
    gen = torch.Generator().manual_seed(L)
    X = torch.zeros(N_SRC, ld)
    X[:, :F] = torch.randn(N_SRC, F, generator=gen)
    Am = torch.zeros(n, ld)
    Am[:, :F] = torch.randn(n, F, generator=gen)
    val = torch.randn(g["col"].numel(), generator=gen)
    rs, cs = g["rs"].float().to(DEV), g["cs"].float().to(DEV)
    for dt in (F32, BF16):
        Xd, Ad, val_d = X.to(dt).to(DEV), Am.to(dt).to(DEV), val.to(DEV)
        y = ops.wspmm(g["rp_d"], g["col_d"], val_d, Xd, F, rscale=rs, cscale=cs)
        d = ops.sddmm(g["rp_d"], g["col_d"], Ad, Xd, F, rscale=rs, cscale=cs)
        y2 = ops.wspmm(g["rp_d"], g["col_d"], val_d, Xd, F, rscale=rs, cscale=cs)
        assert torch.equal(y, y2)                                     # run to run
        for i in (3, 15, 24, 27, 51):                                 # degrees 3, L - 1, 3 L + 5, 2 L, L + 1
            e0, e1 = int(g["rp"][i]), int(g["rp"][i + 1])
            rp1 = torch.tensor([0, e1 - e0], dtype=torch.int32, device=DEV)
            y1 = ops.wspmm(rp1, g["col_d"][e0:e1].contiguous(), val_d[e0:e1].contiguous(), Xd, F,
                           rscale=rs[i:i + 1].contiguous(), cscale=cs)
            d1 = ops.sddmm(rp1, g["col_d"][e0:e1].contiguous(), Ad[i:i + 1].contiguous(), Xd, F,
                           rscale=rs[i:i + 1].contiguous(), cscale=cs)
            assert torch.equal(y1[0], y[i]), "wspmm row %d %s" % (i, dt)
            assert torch.equal(d1, d[e0:e1]), "sddmm row %d %s" % (i, dt)


# ------------------------------------------------------------------ 6. capture
def test_wspmm_then_sddmm_in_a_captured_graph():
    """wspmm followed by sddmm into preallocated outputs, captured and replayed twice: the
    eager bits both times (the launchers allocate nothing and do not synchronise)."""
    g = _graph(16)
    n, F, ld = g["n"], 100, 104
    Xd, bias = _features(F, ld, 77)
    rng = np.random.default_rng(78)
    Ad = torch.zeros(n, ld, dtype=F64)
    Ad[:, :F] = _ints(rng, -3, 3, (n, F))
    X, A = Xd.to(BF16).to(DEV), Ad.to(BF16).to(DEV)
    rs_d, cs_d, bias_d = g["rs"].float().to(DEV), g["cs"].float().to(DEV), bias.float().to(DEV)
    y = torch.empty(n, ld, dtype=BF16, device=DEV)
    d = torch.empty(g["col"].numel(), device=DEV)

    def step():
        ops.wspmm(g["rp_d"], g["col_d"], g["val_d"], X, F, rscale=rs_d, cscale=cs_d, bias=bias_d, relu=True, out=y)
        ops.sddmm(g["rp_d"], g["col_d"], A, X, F, rscale=rs_d, cscale=cs_d, out=d)

    step()
    torch.cuda.synchronize()
    y0, d0 = y.clone(), d.clone()
    exp = torch.zeros(n, ld, dtype=F64)
    exp[:, :F] = _wspmm_ref(g, Xd, bias, F, (True, True, True, True))
    _assert_same(y0.cpu(), exp.to(BF16), "eager wspmm")
    sg = StepGraph(step, warmup=1, device=torch.device(DEV))
    sg()                                                   # eager warm-up
    for k in range(2):
        y.fill_(SENT)
        d.fill_(SENT)
        sg()
        assert sg.graph is not None
        torch.cuda.synchronize()
        assert torch.equal(y, y0) and torch.equal(d, d0), "replay %d" % k


# ------------------------------------------------------------------ 7. autograd on the layer API
@functools.lru_cache(maxsize=None)
def _directed():
    """40 nodes, ~200 directed weighted edges through ``from_edges``; the values are then
    overwritten by exact ones."""
    n = 40
    rng = np.random.default_rng(11)
    src, dst = rng.integers(0, n, 200), rng.integers(0, n, 200)
    g = WeightedGraph.from_edges(n, src, dst, rng.uniform(0.5, 2.0, 200), normalize="rw", device=DEV)
    nnz = g.col.numel()
    assert 150 <= nnz <= 240
    val = torch.from_numpy(rng.choice(VALS, nnz)).float()
    val[::9] = 0.0
    g.val = val.to(DEV)
    A_of = lambda v: torch.zeros(n, n, dtype=F64).index_put((_rows(g.rowptr.cpu()), g.col.cpu().long()), v,
                                                             accumulate=True)
    # directed: the matrix is not symmetric
    assert not torch.equal(A_of(val.double()), A_of(val.double()).t())
    return g, val, A_of, rng


def test_weighted_aggregate_forward_dx_dval_exact():
    g, val, A_of, _ = _directed()
    n, F = g.n, 12
    rng = np.random.default_rng(12)
    xd, gd = _ints(rng, -3, 3, (n, F)), _ints(rng, -3, 3, (n, F))
    xr, vr = xd.clone().requires_grad_(), val.double().clone().requires_grad_()
    yr = A_of(vr) @ xr
    yr.backward(gd)
    assert _exact(yr.detach(), 4096) and _exact(xr.grad, 4096) and _exact(vr.grad, 4096)
    x = xd.float().to(DEV).requires_grad_()
    v = val.clone().to(DEV).requires_grad_()
    y = weighted_aggregate(x, g, v)
    y.backward(gd.float().to(DEV))
    _assert_same(y.detach().cpu(), yr.detach().float(), "forward")
    _assert_same(x.grad.cpu(), xr.grad.float(), "dx")
    assert v.grad.dtype == F32
    _assert_same(v.grad.cpu(), vr.grad.float(), "dval")
    # dval is computed only when asked for
    x2 = xd.float().to(DEV).requires_grad_()
    weighted_aggregate(x2, g).backward(gd.float().to(DEV))
    _assert_same(x2.grad.cpu(), xr.grad.float(), "dx without dval")


def test_two_layer_gcn_on_a_weighted_graph_exact():
    """A 2-layer GCN (16-8-4, no dropout) with integer weights in [-2, 2] and integer
    features in [-1, 1] on the directed graph: logits, dW, db and d edge_weight equal the
    dense fp64 model's.  Magnitudes: |A| row sums <= ~30 (asserted below), so layer 1 is
    <= 16 * 2 * 30 + 2 and layer 2 <= 8 * 2 * 30 * that < 2^19; the gradients of a +-1
    cotangent stay below 2^24 (all asserted on the fp64 model)."""
    g, val, A_of, _ = _directed()
    n = g.n
    rng = np.random.default_rng(13)
    xd = _ints(rng, -1, 1, (n, 16))
    Ws = [_ints(rng, -2, 2, (16, 8)), _ints(rng, -2, 2, (8, 4))]
    bs = [_ints(rng, -2, 2, (8,)), _ints(rng, -2, 2, (4,))]
    cot = _ints(rng, -1, 1, (n, 4))
    assert float(A_of(val.double()).abs().sum(1).max()) <= 32
    # the dense fp64 model
    Wr = [w.clone().requires_grad_() for w in Ws]
    br = [b.clone().requires_grad_() for b in bs]
    vr = val.double().clone().requires_grad_()
    Ar = A_of(vr)
    h1 = (Ar @ (xd @ Wr[0]) + br[0]).relu()
    out_r = Ar @ (h1 @ Wr[1]) + br[1]
    out_r.backward(cot)
    refs = [out_r.detach(), h1.detach(), vr.grad] + [w.grad for w in Wr] + [b.grad for b in br]
    for r in refs:
        assert _exact(r, 2 ** 24)
    # partial sums: bounded by the sums of absolute values along every reduction
    Aa = A_of(val.double().abs())
    h1a = Aa @ (xd.abs() @ Ws[0].abs()) + bs[0].abs()
    oa = Aa @ (h1a @ Ws[1].abs()) + bs[1].abs()
    dz2a = Aa.t() @ cot.abs()
    dh1a = dz2a @ Ws[1].abs().t()
    dz1a = Aa.t() @ dh1a
    bounds = [oa, h1a.t() @ dz2a, xd.abs().t() @ dz1a, cot.abs().sum(0), dh1a.sum(0),
              cot.abs() @ (h1a @ Ws[1].abs()).t() + dh1a @ (xd.abs() @ Ws[0].abs()).t()]
    assert max(float(b.max()) for b in bounds) < 2 ** 24
    model = GCN([16, 8, 4], dropout=0.0).to(DEV)
    with torch.no_grad():
        for conv, w, b in zip(model.convs, Ws, bs):
            conv.weight.copy_(w.float())
            conv.bias.copy_(b.float())
    ew = val.clone().to(DEV).requires_grad_()
    out = model(xd.float().to(DEV), g, edge_weight=ew)
    out.backward(cot.float().to(DEV))
    _assert_same(out.detach().cpu(), out_r.detach().float(), "logits")
    for k in range(2):
        _assert_same(model.convs[k].weight.grad.cpu(), Wr[k].grad.float(), "dW%d" % (k + 1))
        assert torch.equal(model.convs[k].bias.grad.cpu(), br[k].grad.float()), "db%d" % (k + 1)
    assert torch.equal(ew.grad.cpu(), vr.grad.float()), "d edge_weight"


def test_gcnconv_on_a_normgraph_is_untouched():
    """The NormGraph branch computes what it did: ``ops.spmm`` called as the layer calls it."""
    from cgnn_amd.gnn import data
    gd = data.synthetic("cora", scale=0.1, device=DEV)
    ng = NormGraph.from_data(gd)
    conv = GCNConv(24, 12, torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        conv.bias.copy_(torch.linspace(-1, 1, 12))
    h = torch.randn(gd.n, 24, generator=torch.Generator().manual_seed(4)).to(DEV).to(BF16)
    for relu in (False, True):
        y = conv(h, ng, relu=relu)
        zp = layers.pad_cols(h @ conv.weight.to(BF16)).contiguous()
        ref = ops.spmm(ng.rowptr, ng.col, zp, 12, rscale=ng.dinv, cscale=ng.dinv,
                       bias=conv.bias.detach().float().contiguous(), relu=relu, out_dtype=BF16, ld_out=zp.shape[1])
        assert torch.equal(y.detach(), ref[:, :12])
    with pytest.raises(TypeError):
        conv(h, ng, edge_weight=torch.ones(ng.col.numel(), device=DEV))


# ------------------------------------------------------------------ 8. rejections
def test_rejections_raise_before_any_launch():
    g = _graph(8)
    n, nnz = g["n"], g["col"].numel()
    X = torch.ones(N_SRC, 16, device=DEV)
    sent = torch.full((n, 16), SENT, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError, match="-5"):          # (fp32, bf16) is not compiled
        ops.wspmm(g["rp_d"], g["col_d"], g["val_d"], X, 16, out=sent)
    with pytest.raises(RuntimeError, match="-5"):          # (bf16, fp16)
        ops.wspmm(g["rp_d"], g["col_d"], g["val_d"], X.to(BF16), 16, out=sent.view(F16))
    assert torch.all(sent == SENT)
    out12 = torch.full((n, 12), SENT, device=DEV)
    with pytest.raises(RuntimeError, match="-3"):          # ld % 8 != 0 (input, then output)
        ops.wspmm(g["rp_d"], g["col_d"], g["val_d"], torch.ones(N_SRC, 12, device=DEV), 12)
    with pytest.raises(RuntimeError, match="-3"):
        ops.wspmm(g["rp_d"], g["col_d"], g["val_d"], X, 12, out=out12)
    assert torch.all(out12 == SENT)
    with pytest.raises(RuntimeError, match="-3"):          # F > ld
        ops.wspmm(g["rp_d"], g["col_d"], g["val_d"], X, 17)
    with pytest.raises(TypeError):                         # fp16 values
        ops.wspmm(g["rp_d"], g["col_d"], g["val_d"].to(F16), X, 16)
    d = torch.full((nnz,), SENT, device=DEV)
    A = torch.ones(n, 16, device=DEV)
    with pytest.raises(TypeError):                         # A / B dtypes differ
        ops.sddmm(g["rp_d"], g["col_d"], A.to(BF16), X, 16, out=d)
    with pytest.raises(RuntimeError, match="-3"):
        ops.sddmm(g["rp_d"], g["col_d"], torch.ones(n, 12, device=DEV), X, 12, out=d)
    with pytest.raises(TypeError):                         # fp64 is not a kernel type
        ops.sddmm(g["rp_d"], g["col_d"], A.double(), X.double(), 16, out=d)
    torch.cuda.synchronize()
    assert torch.all(d == SENT)
