"""Exact oracle tests of the graph-readout HIP kernels (gnn_readout.hip: seg_reduce_kernel,
seg_bcast_kernel), of their two-level schedule and of the public API on top of them
(gnn/readout.py).

Every reference is computed here, in fp64 / numpy from the segment pointer -- never through
the CPU branches of ``ops``.  Max / min accumulate nothing (the result is a copy of an input
element) and are compared bit for bit on arbitrary data; the exact sum tests use integers in
[-2, 2], whose partial sums are exact in fp32 in any order (asserted with a magnitude bound),
so the comparison is ``torch.equal`` against the fp64 result cast to the output type.  The
segment lengths are built from ``ops.READOUT_CHUNK`` and never hard-code it.
"""
import functools

import numpy as np
import pytest
import torch

from cgnn_amd.gnn import ops
from cgnn_amd.gnn.layers import GINEConv
from cgnn_amd.gnn.readout import GlobalAttention, GraphBatch, graph_broadcast, graph_readout
from cgnn_amd.utils.hipgraph import StepGraph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 7              # sentinel of rows / buffers a kernel must not write
BIG = 1.0e4           # fills the padding columns of inputs: must never reach a result
BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
NAN, INF = float("nan"), float("inf")
R = ops.READOUT_CHUNK

# (F, ld, L): L lanes per row, from the written width; the last is two 512-column slabs
WIDTHS = [(8, 8, 8), (41, 48, 8), (64, 64, 8), (65, 72, 16), (128, 128, 16), (129, 136, 32),
          (256, 256, 32), (257, 264, 64), (512, 512, 64), (520, 528, 64)]
PAIRS = [(BF16, BF16), (BF16, F32), (F16, F16), (F16, F32), (F32, F32)]
SUM_PAIRS = PAIRS + [(F32, BF16), (F32, F16)]


# ------------------------------------------------------------------ helpers
def _lengths(short=False):
    d = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 3 * R + 5]
    lens = d + d[::-1] + [2, R + 1, 0]
    return [min(m, R) for m in lens] if short else lens


@functools.lru_cache(maxsize=None)
def _batch(short=False):
    """The 41 segments (every 8- / 4- / 1-step remainder, lengths around one, two and three
    chunks, empty ones first, last and in the middle); ``short``: every length cut to R, the
    single-launch path."""
    lens = _lengths(short)
    assert len(lens) == 41 and all(len(lens) % (4 * (64 // L)) for L in (8, 16, 32, 64))
    gp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    b = GraphBatch.from_ptr(torch.from_numpy(gp)).to(DEV)
    assert b.chunk == R and b.single_pass == short and (short or b.n_chunks > b.n_graphs)
    return dict(b=b, lens=lens, gp=gp, n=int(gp[-1]), G=len(lens), seg=np.repeat(np.arange(len(lens)), lens))


def _features(kind, n, F, ld, seed, extra=2):
    """fp64 [n + extra, ld]: random normal values or integers in [-2, 2]; the padding columns
    and the ``extra`` rows past the last segment hold BIG."""
    rng = np.random.default_rng(seed)
    X = torch.full((n + extra, ld), BIG, dtype=F64)
    if kind == "normal":
        X[:n, :F] = torch.from_numpy(rng.standard_normal((n, F)))
    else:
        X[:n, :F] = torch.from_numpy(rng.integers(-2, 3, (n, F)).astype(np.float64))
    return X


def _sum_ref(gp, X, F):
    """fp64 [G, F] segment sums of a numpy X."""
    S = np.zeros((len(gp) - 1, F))
    for g in range(len(gp) - 1):
        S[g] = X[gp[g]:gp[g + 1], :F].sum(0)
    return S


def _best_ref(gp, X, F, is_min):
    """(Y, arg) of the definition.  ``np.argmax`` / ``np.argmin`` return the FIRST index of the
    extreme value and treat a NaN as the extreme (the first NaN wins): the scan rule."""
    G = len(gp) - 1
    Y, A = np.zeros((G, F)), np.full((G, F), -1, dtype=np.int64)
    for g in range(G):
        if gp[g + 1] > gp[g]:
            v = X[gp[g]:gp[g + 1], :F]
            k = np.argmin(v, axis=0) if is_min else np.argmax(v, axis=0)
            Y[g] = v[k, np.arange(F)]
            A[g] = gp[g] + k
    return Y, A


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


def _sum_into(ptr, X, F, ld, dt, rscale=None):
    """ops.seg_reduce (sum) into an output with three sentinel rows; the CPU copy."""
    S = ptr.numel() - 1
    full = torch.full((S + 3, ld), SENT, dtype=dt, device=DEV)
    Y, A = ops.seg_reduce(ptr, X, F, "sum", rscale=rscale, out=full[:S])
    assert Y.data_ptr() == full.data_ptr() and A is None
    return full.cpu()


def _best_into(ptr, X, F, ld, reduce, arg_in=None, with_arg=True):
    S = ptr.numel() - 1
    full = torch.full((S + 3, ld), SENT, dtype=X.dtype, device=DEV)
    afull = torch.full((S + 3, ld), SENT, dtype=torch.int32, device=DEV)
    Y, A = ops.seg_reduce(ptr, X, F, reduce, arg_in=arg_in, out=full[:S], arg=afull[:S] if with_arg else None)
    assert Y.data_ptr() == full.data_ptr() and (A is None) == (not with_arg)
    return full, afull


# ------------------------------------------------------------------ 1. sum / mean, bit exact
@pytest.mark.parametrize("F,ld,L", WIDTHS)
def test_sum_and_mean_exact_over_lengths_widths_and_type_pairs(F, ld, L):
    """seg_reduce_kernel (sum) against the fp64 sum, bit for bit: the seven type pairs, with and
    without the row scale, as one launch over the graphs (long segments included) and as the
    two passes chunks -> fp32 partial rows -> graphs; zero padding columns and empty segments,
    three sentinel rows, padding columns and trailing rows of X that must not be read."""
    t = _batch()
    b, gp, n, G = t["b"], t["gp"], t["n"], t["G"]
    Xd = _features("ints", n, F, ld, 1000 + F)
    S64 = torch.from_numpy(_sum_ref(gp, Xd.numpy(), F))
    # at most 3 R + 5 terms of magnitude <= 2 per sum: exact in fp32 in any order
    assert float(S64.abs().max()) <= 2 * (3 * R + 5) < 2 ** 24 and torch.equal(S64.float().double(), S64)
    mean64 = S64 * b.inv_count.cpu().double()[:, None]       # one fp32 product, rounded by .float()
    empty = np.flatnonzero(np.diff(gp) == 0)
    assert empty.size >= 3
    for tin, tout in SUM_PAIRS:
        X = Xd.to(tin).to(DEV)
        for name, rs, ref in (("sum", None, S64), ("mean", b.inv_count, mean64)):
            exp = ref.float().to(tout)
            part = _sum_into(b.cptr, X, F, ld, F32)
            two = torch.full((G + 3, ld), SENT, dtype=tout, device=DEV)
            ops.seg_reduce(b.gchunk, part[:b.n_chunks].to(DEV), F, "sum", rscale=rs, out=two[:G])
            for how, got in (("one launch", _sum_into(b.gptr, X, F, ld, tout, rs)), ("two passes", two.cpu())):
                what = "%s %s->%s F=%d %s" % (name, tin, tout, F, how)
                _assert_same(got[:G, :F], exp, what)
                assert torch.all(got[:G, F:] == 0), what + ": padding columns"
                assert torch.all(got[empty] == 0), what + ": empty segments"
                assert torch.all(got[G:] == SENT), what + ": rows past the last segment"
            assert torch.all(part[b.n_chunks:] == SENT) and torch.all(part[:b.n_chunks, F:] == 0)


@pytest.mark.parametrize("short", [False, True], ids=["two_level", "single_launch"])
def test_graph_readout_sum_and_mean_exact(short):
    """graph_readout on the two-level batch and on the all-short batch (one launch), three
    storage types, ragged and two-slab widths: the fp64 oracle bit for bit."""
    t = _batch(short)
    b, gp, n = t["b"], t["gp"], t["n"]
    for F in (41, 128, 520):
        Xd = _features("ints", n, F, F, 1100 + F, extra=0)
        S64 = torch.from_numpy(_sum_ref(gp, Xd.numpy(), F))
        mean64 = S64 * b.inv_count.cpu().double()[:, None]
        for dt in (F32, BF16, F16):
            x = Xd.to(dt).to(DEV)
            for reduce, ref in (("sum", S64), ("mean", mean64)):
                y = graph_readout(x, b, reduce)
                assert y.dtype == dt and y.shape == (t["G"], F)
                _assert_same(y.cpu(), ref.float().to(dt), "%s %s F=%d" % (reduce, dt, F))


# ------------------------------------------------------------------ 2. sum on normal data
@pytest.mark.parametrize("dt", [F32, BF16])
def test_sum_on_normal_data_is_reproducible_accurate_and_position_independent(dt):
    """Two runs are bit-identical; every result is within (m - 1) 2^-24 sum|x_i| of the fp64 sum
    of the stored values -- the bound of any summation order of m terms in fp32 -- plus half
    an ulp of the output type (relative 2^-24 / 2^-8); and the same graphs batched in a
    permuted order give, graph for graph, the same bits."""
    t = _batch()
    b, gp, n, G, lens = t["b"], t["gp"], t["n"], t["G"], t["lens"]
    half_ulp = 2.0 ** -24 if dt == F32 else 2.0 ** -8
    perm = np.random.default_rng(5).permutation(G)
    gp_p = np.concatenate([[0], np.cumsum(np.asarray(lens)[perm])]).astype(np.int64)
    bp = GraphBatch.from_ptr(torch.from_numpy(gp_p)).to(DEV)
    rows_p = np.concatenate([np.arange(gp[g], gp[g + 1]) for g in perm])
    for F in (41, 128, 520):
        xs = _features("normal", n, F, F, 2000 + F, extra=0).to(dt)
        x = xs.to(DEV)
        y1, y2 = graph_readout(x, b, "sum"), graph_readout(x, b, "sum")
        assert torch.equal(y1, y2)
        x64 = xs.double().numpy()
        S = _sum_ref(gp, x64, F)
        absum = _sum_ref(gp, np.abs(x64), F)
        m1 = np.maximum(np.asarray(lens) - 1, 0)[:, None]
        B = m1 * 2.0 ** -24 * absum
        bound = B + half_ulp * (np.abs(S) + B)
        err = np.abs(y1.double().cpu().numpy() - S)
        assert np.all(err <= bound), (dt, F, float((err - bound).max()))
        yp = graph_readout(x[torch.from_numpy(rows_p).to(DEV)], bp, "sum")
        assert torch.equal(yp, y1[torch.from_numpy(perm).to(DEV)]), (dt, F)


# ------------------------------------------------------------------ 3. max / min
@pytest.mark.parametrize("F,ld,L", WIDTHS)
def test_max_and_min_exact_values_and_arg(F, ld, L):
    """seg_reduce_kernel (max / min), value and arg bit for bit, as one launch over the graphs
    and as two passes with the first pass's indices handed through ``arg_in``; random values and
    tie-heavy integers; in the longest segment rows R - 1 and R, either side of a chunk
    boundary, hold the extreme value of every column and the first must win."""
    t = _batch()
    b, gp, n, G = t["b"], t["gp"], t["n"], t["G"]
    long_g = int(np.argmax(np.diff(gp)))
    r0 = int(gp[long_g])
    empty = np.flatnonzero(np.diff(gp) == 0)
    for kind in ("normal", "ties"):
        Xd = _features(kind, n, F, ld, 3000 + F)
        for dt in (F32, BF16, F16):
            for reduce in ("max", "min"):
                Xs = Xd.to(dt)
                Xs[r0 + R - 1:r0 + R + 1, :F] = -50.0 if reduce == "min" else 50.0
                Yr, Ar = _best_ref(gp, Xs.double().numpy(), F, reduce == "min")
                assert np.all(Ar[long_g] == r0 + R - 1)
                X = Xs.to(DEV)
                P, PA = _best_into(b.cptr, X, F, ld, reduce)
                C = b.n_chunks
                assert torch.all(P[C:] == SENT) and torch.all(PA[C:] == SENT)
                two = _best_into(b.gchunk, P[:C], F, ld, reduce, arg_in=PA[:C])
                for how, (Y, A) in (("one launch", _best_into(b.gptr, X, F, ld, reduce)), ("two passes", two)):
                    got, garg = Y.cpu(), A.cpu()
                    what = "%s %s %s F=%d %s" % (kind, dt, reduce, F, how)
                    _assert_same(got[:G, :F], torch.from_numpy(Yr), what)
                    assert torch.equal(garg[:G, :F].long(), torch.from_numpy(Ar)), what + ": arg"
                    assert torch.all(got[:G, F:] == 0) and torch.all(garg[:G, F:] == -1), what + ": padding columns"
                    assert torch.all(got[empty] == 0) and torch.all(garg[empty] == -1), what + ": empty segments"
                    assert torch.all(got[G:] == SENT) and torch.all(garg[G:] == SENT), what + ": past the last row"


def _scan_ref(vals, is_min):
    """The replacement rule as a loop over one segment's candidates: (value, position)."""
    best, pos = vals[0], 0
    for k, c in enumerate(vals[1:], 1):
        if (c < best if is_min else c > best) or (np.isnan(c) and not np.isnan(best)):
            best, pos = c, k
    return best, pos


@pytest.mark.parametrize("dt", [F32, BF16, F16])
def test_nan_and_infinities(dt):
    """Segments whose only candidates are the reduction's own identity, NaNs first / in the
    middle / twice, and a segment of 2 R + 3 rows with NaNs in its second and third chunk:
    value and arg follow the rule through graph-level two passes and through one launch."""
    long_row = [float(k % 5) for k in range(R + 2)] + [NAN] + [float(k % 3) for k in range(R)]
    long_row[2 * R + 1] = NAN
    rows = [[-INF, -INF, -INF], [INF, INF], [-INF, 1.0, -INF], [INF, -1.0, INF], [1.0, NAN, 3.0], [NAN, 5.0, -5.0],
            [2.0, NAN, NAN, 9.0], [-INF, INF, -INF], [-INF], [INF], [NAN], [], long_row]
    assert len(long_row) == 2 * R + 3
    lens = [len(r) for r in rows]
    gp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(gp[-1])
    b = GraphBatch.from_ptr(torch.from_numpy(gp)).to(DEV)
    assert not b.single_pass
    F, ld = 9, 16                                            # two lanes of features
    X = torch.full((n, ld), BIG, dtype=F64)
    X[:, :F] = torch.tensor([v for r in rows for v in r], dtype=F64)[:, None]
    X[:, 4] = torch.arange(n, dtype=F64) % 7                   # one plain column between them
    Xs = X.to(dt)
    xs = Xs.double().numpy()
    for reduce in ("max", "min"):
        is_min = reduce == "min"
        P, PA = ops.seg_reduce(b.cptr, Xs.to(DEV), F, reduce, with_arg=True)
        Y2, A2 = ops.seg_reduce(b.gchunk, P, F, reduce, arg_in=PA, with_arg=True)
        Y1, A1 = ops.seg_reduce(b.gptr, Xs.to(DEV), F, reduce, with_arg=True)
        _assert_same(Y2.cpu(), Y1.cpu(), reduce)
        assert torch.equal(A1, A2)
        Y, A = Y2.cpu(), A2.cpu()
        for g, r in enumerate(rows):
            for f in (0, 4, 8):
                if not r:
                    assert float(Y[g, f]) == 0 and int(A[g, f]) == -1
                    continue
                best, pos = _scan_ref([xs[gp[g] + k, f] for k in range(len(r))], is_min)
                got = float(Y[g, f])
                assert (np.isnan(best) and np.isnan(got)) or got == best, (reduce, g, f, got, best)
                assert int(A[g, f]) == gp[g] + pos, (reduce, g, f, int(A[g, f]), gp[g] + pos)
        assert torch.isnan(Y[4, 0]) and int(A[4, 0]) == gp[4] + 1
        assert torch.isnan(Y[5, 0]) and int(A[5, 0]) == gp[5]
        assert torch.isnan(Y[12, 0]) and int(A[12, 0]) == gp[12] + R + 2          # the first NaN, second chunk
        i = 1 if is_min else 0
        assert float(Y[i, 0]) == (INF if is_min else -INF) and int(A[i, 0]) == gp[i]
        assert torch.all(Y[:, F:] == 0) and torch.all(A[:, F:] == -1)


def test_without_arg_same_values_and_no_index_store():
    t = _batch()
    b, n, G = t["b"], t["n"], t["G"]
    for (F, ld) in [(41, 48), (129, 136), (520, 528)]:
        X = _features("normal", n, F, ld, 50 + F).to(BF16).to(DEV)
        for reduce in ("max", "min"):
            y1, a1 = _best_into(b.gptr, X, F, ld, reduce)
            y0, a0 = _best_into(b.gptr, X, F, ld, reduce, with_arg=False)
            assert torch.equal(y0, y1)
            assert torch.all(a0 == SENT) and not torch.all(a1[:G] == SENT)
    Y, A = ops.seg_reduce(b.gptr, X, F, "min")                     # allocating form: with_arg defaults to False
    assert A is None and torch.equal(Y, y1[:G])
    with torch.no_grad():                                        # the layer asks for no index without a gradient
        assert torch.equal(graph_readout(X[:n, :F], b, "min"), Y[:, :F])


# ------------------------------------------------------------------ 4. broadcast
@pytest.mark.parametrize("F,ld,L", WIDTHS)
def test_seg_bcast_exact_over_widths_and_type_pairs(F, ld, L):
    """seg_bcast_kernel for the five type pairs: the plain copy, the scaled copy (one fp32
    product, one rounding: emulated exactly in fp64) and the copy masked by ``arg`` with integer
    gradients; zero padding columns, three sentinel rows, padding columns of U and arg that
    must not be read."""
    t = _batch()
    b, gp, n, G, seg = t["b"], t["gp"], t["n"], t["G"], t["seg"]
    rng = np.random.default_rng(4000 + F)
    Un = _features("normal", G, F, ld, 4100 + F, extra=0)
    Ui = torch.full((G, ld), BIG, dtype=F64)
    Ui[:, :F] = torch.from_numpy(rng.integers(-3, 4, (G, F)).astype(np.float64))
    rs = torch.from_numpy(rng.standard_normal(G).astype(np.float32))
    arg = torch.full((G, ld), 10 ** 6, dtype=torch.int32)      # a padding value that names no row
    for g in range(G):
        if gp[g + 1] > gp[g]:
            arg[g, :F] = torch.from_numpy(rng.integers(gp[g], gp[g + 1], F).astype(np.int32))
        else:
            arg[g, :F] = -1
    exp_arg = torch.zeros(n, F, dtype=F64)
    sel = arg[:, :F].long()
    cols = torch.arange(F).expand(G, F)
    exp_arg[sel[sel >= 0], cols[sel >= 0]] = Ui[:, :F][sel >= 0]
    assert float(exp_arg.abs().sum()) > 0
    rs_d, arg_d = rs.to(DEV), arg.to(DEV)
    for tin, tout in PAIRS:
        Us = Un.to(tin)
        cases = [("copy", Us, None, None, Us[seg, :F].double().to(tout)),
                 ("scaled", Us, rs_d, None, (Us[seg, :F].double() * rs.double()[seg, None]).float().to(tout)),
                 ("arg", Ui.to(tin), None, arg_d, exp_arg.to(tout))]
        for name, U, scale, a, exp in cases:
            full = torch.full((n + 3, ld), SENT, dtype=tout, device=DEV)
            out = ops.seg_bcast(b.batch, U.to(DEV), F, rscale=scale, arg=a, out=full[:n])
            assert out.data_ptr() == full.data_ptr()
            got = full.cpu()
            what = "bcast %s %s->%s F=%d" % (name, tin, tout, F)
            _assert_same(got[:n, :F], exp, what)
            assert torch.all(got[:n, F:] == 0), what + ": padding columns"
            assert torch.all(got[n:] == SENT), what + ": rows past n"


# ------------------------------------------------------------------ 5. autograd on the device
@pytest.mark.parametrize("short", [False, True], ids=["two_level", "single_launch"])
def test_graph_readout_and_broadcast_gradients_match_the_fp64_oracle(short):
    t = _batch(short)
    b, gp, n, G, seg = t["b"], t["gp"], t["n"], t["G"], t["seg"]
    F = 41
    rng = np.random.default_rng(77)
    xd = torch.from_numpy(rng.integers(-2, 3, (n, F)).astype(np.float64))
    gd = torch.from_numpy(rng.integers(-3, 4, (G, F)).astype(np.float64))
    inv = b.inv_count.cpu().double()
    for dt in (F32, BF16):
        for reduce in ("sum", "mean", "max", "min"):
            x = xd.to(dt).to(DEV).requires_grad_()
            y = graph_readout(x, b, reduce)
            y.backward(gd.to(dt).to(DEV))
            if reduce in ("sum", "mean"):
                scale = inv if reduce == "mean" else torch.ones(G, dtype=F64)
                yr = (torch.from_numpy(_sum_ref(gp, xd.numpy(), F)) * scale[:, None]).float().to(dt)
                dxr = (gd * scale[:, None]).float().to(dt)[seg]
            else:
                Yr, Ar = _best_ref(gp, xd.numpy(), F, reduce == "min")
                yr = torch.from_numpy(Yr).to(dt)
                dxr = torch.zeros(n, F, dtype=F64)
                A = torch.from_numpy(Ar)
                cols = torch.arange(F).expand(G, F)
                dxr[A[A >= 0], cols[A >= 0]] = gd[A >= 0]
                dxr = dxr.to(dt)
            what = "%s %s" % (reduce, dt)
            _assert_same(y.detach().cpu(), yr, what)
            _assert_same(x.grad.cpu(), dxr, what + " dx")
        # broadcast: forward the scaled copy, backward the scaled sum of integers (exact)
        u = gd.to(dt).to(DEV).requires_grad_()
        scale = torch.from_numpy(rng.integers(1, 4, G).astype(np.float32))
        out = graph_broadcast(u, b, scale.to(DEV))
        gout = xd.to(dt).to(DEV)
        out.backward(gout)
        _assert_same(out.detach().cpu(), (gd * scale.double()[:, None]).float().to(dt)[seg], "broadcast %s" % dt)
        dur = (torch.from_numpy(_sum_ref(gp, xd.numpy(), F)) * scale.double()[:, None]).float().to(dt)
        _assert_same(u.grad.cpu(), dur, "broadcast %s du" % dt)
        assert torch.equal(graph_broadcast(u.detach(), b), u.detach()[b.batch.long()])


def test_global_attention_matches_a_dense_per_graph_softmax():
    """GlobalAttention in fp32 on the device against a dense per-graph softmax and weighted sum
    in fp64, forward and the gradients of the input and of both modules, rtol = atol = 1e-4:
    the tolerance of the layer test of test_gnn_edge_softmax_gpu.py (inputs O(1))."""
    t = _batch()
    b, gp, n, G = t["b"], t["gp"], t["n"], t["G"]
    F, H = 24, 20
    gen = torch.Generator().manual_seed(3)
    xd = torch.randn(n, F, generator=gen, dtype=F64)
    gate = torch.nn.Linear(F, 1).double()
    nn = torch.nn.Linear(F, H).double()
    with torch.no_grad():
        for p in list(gate.parameters()) + list(nn.parameters()):
            p.copy_(torch.randn(p.shape, generator=gen, dtype=F64) * 0.3)
    cot = torch.randn(G, H, generator=gen, dtype=F64)
    # dense fp64
    x64 = xd.clone().requires_grad_()
    s, h = gate(x64)[:, 0], nn(x64)
    rows = []
    for g in range(G):
        sl = slice(int(gp[g]), int(gp[g + 1]))
        rows.append((torch.softmax(s[sl], 0)[:, None] * h[sl]).sum(0) if gp[g + 1] > gp[g] else torch.zeros(H, dtype=F64))
    out64 = torch.stack(rows)
    out64.backward(cot)
    ref = [out64.detach(), x64.grad] + [p.grad.clone() for p in list(gate.parameters()) + list(nn.parameters())]
    for p in list(gate.parameters()) + list(nn.parameters()):
        p.grad = None
    layer = GlobalAttention(gate, nn).float().to(DEV)
    x = xd.float().to(DEV).requires_grad_()
    out, alpha = layer(x, b, return_attention=True)
    out.backward(cot.float().to(DEV))
    got = [out.detach(), x.grad] + [p.grad for p in layer.parameters()]
    assert alpha.shape == (n,) and len(got) == len(ref) == 6
    names = ("out", "dx", "gate.weight", "gate.bias", "nn.weight", "nn.bias")
    for name, o, r in zip(names, got, ref):
        # (a constant added to every score changes no softmax: the gate bias has gradient 0)
        assert float(r.abs().max()) > 1e-2 or name == "gate.bias", name
        np.testing.assert_allclose(o.double().cpu().numpy(), r.numpy(), rtol=1e-4, atol=1e-4, err_msg=name)


# ------------------------------------------------------------------ 6. capture
def test_two_pass_sum_and_its_backward_in_a_captured_graph():
    """The two-pass sum and its backward (the broadcast) into preallocated buffers, captured on
    one stream as a linear chain and replayed twice with new inputs written into the captured
    buffers: the eager bits each time."""
    t = _batch()
    b, n, G = t["b"], t["n"], t["G"]
    F, ld = 100, 104
    X = torch.zeros(n, ld, dtype=BF16, device=DEV)
    dY = torch.zeros(G, ld, dtype=BF16, device=DEV)
    P = torch.empty(b.n_chunks, ld, dtype=F32, device=DEV)
    Y = torch.empty(G, ld, dtype=BF16, device=DEV)
    dX = torch.empty(n, ld, dtype=BF16, device=DEV)

    def step():
        ops.seg_reduce(b.cptr, X, F, "sum", out=P)
        ops.seg_reduce(b.gchunk, P, F, "sum", rscale=b.inv_count, out=Y)
        ops.seg_bcast(b.batch, dY, F, rscale=b.inv_count, out=dX)

    def inputs(seed):
        X.copy_(_features("normal", n, F, ld, seed, extra=0).to(BF16))
        dY.copy_(_features("normal", G, F, ld, seed + 1, extra=0).to(BF16))

    eager = []
    for seed in (31, 33):
        inputs(seed)
        step()
        torch.cuda.synchronize()
        eager.append((Y.clone(), dX.clone()))
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[0][1], eager[1][1])
    sg = StepGraph(step, warmup=1, device=torch.device(DEV))
    sg()                                                   # eager warm-up
    for k, seed in enumerate((31, 33)):
        inputs(seed)
        P.fill_(SENT)
        Y.fill_(SENT)
        dX.fill_(SENT)
        sg()
        assert sg.graph is not None
        torch.cuda.synchronize()
        assert torch.equal(Y, eager[k][0]) and torch.equal(dX, eager[k][1]), "replay %d" % k


# ------------------------------------------------------------------ 7. empty inputs, operand checks
def test_empty_inputs_and_operand_rejections():
    F = 24
    for reduce in ("sum", "mean", "max", "min"):
        # no graph at all
        b0 = GraphBatch.from_ptr(torch.tensor([0])).to(DEV)
        x0 = torch.zeros(0, F, dtype=BF16, device=DEV, requires_grad=True)
        y0 = graph_readout(x0, b0, reduce)
        assert y0.shape == (0, F)
        y0.sum().backward()
        assert x0.grad.shape == (0, F)
        # graphs, all of them empty: null X
        b1 = GraphBatch.from_graphs([(0, [], [])] * 5, device=DEV)
        x1 = torch.zeros(0, F, dtype=F32, device=DEV, requires_grad=True)
        y1 = graph_readout(x1, b1, reduce)
        assert y1.shape == (5, F) and torch.all(y1 == 0)
        y1.sum().backward()
        assert x1.grad.shape == (0, F)
    Y, A = ops.seg_reduce(b1.gptr, torch.zeros(0, F, device=DEV), F, "max", with_arg=True)
    assert torch.all(Y == 0) and torch.all(A == -1)
    u = torch.ones(5, F, device=DEV, requires_grad=True)
    out = graph_broadcast(u, b1)
    assert out.shape == (0, F)
    out.sum().backward()
    assert torch.all(u.grad == 0)
    # operands that are not int32 / not contiguous / of a type that is not compiled
    t = _batch()
    b, n, G = t["b"], t["n"], t["G"]
    X = torch.ones(n, F, device=DEV)
    with pytest.raises(TypeError):
        ops.seg_reduce(b.gptr.long(), X, F)
    with pytest.raises(TypeError):
        ops.seg_reduce(b.gptr, X, F, "max", arg=torch.zeros(G, F, dtype=torch.int64, device=DEV))
    with pytest.raises(TypeError):
        ops.seg_reduce(b.gptr, X, F, rscale=b.inv_count.double())
    with pytest.raises(TypeError):
        ops.seg_reduce(b.gptr, X.double(), F)
    with pytest.raises(ValueError):
        ops.seg_reduce(b.gptr, torch.ones(n, 2 * F, device=DEV)[:, ::2], F)
    with pytest.raises(TypeError):
        ops.seg_bcast(b.batch.long(), torch.ones(G, F, device=DEV), F)
    with pytest.raises(ValueError):
        ops.seg_bcast(b.batch, torch.ones(G, 2 * F, device=DEV)[:, ::2], F)
    with pytest.raises(RuntimeError, match="-5"):
        ops.seg_reduce(b.gptr, X.to(BF16), F, out_dtype=F16)
    with pytest.raises(RuntimeError, match="-5"):
        ops.seg_bcast(b.batch, torch.ones(G, F, device=DEV), F, out_dtype=BF16)
    with pytest.raises(RuntimeError, match="-3"):
        ops.seg_reduce(b.gptr, torch.ones(n, 12, device=DEV), 12)


# ------------------------------------------------------------------ 8. end to end
def test_gine_mean_readout_linear_trains_and_is_bit_reproducible():
    """Eight graphs of 3-20 nodes with edge features: GINEConv -> graph_readout("mean") ->
    Linear; three Adam steps lower the loss, and two runs give the same bits."""
    rng = np.random.default_rng(11)
    graphs = []
    for _ in range(8):
        m = int(rng.integers(3, 21))
        k = int(rng.integers(m, 3 * m))
        graphs.append((m, rng.integers(0, m, k), rng.integers(0, m, k)))
    b = GraphBatch.from_graphs(graphs, device=DEV)
    assert b.n_graphs == 8 and b.single_pass
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(b.n, 16, generator=gen).to(DEV)
    e = torch.randn(b.col.numel(), 5, generator=gen)[b.eperm.cpu()].to(DEV)
    target = torch.randn(8, 4, generator=gen).to(DEV)

    def run():
        g2 = torch.Generator().manual_seed(2)
        torch.manual_seed(0)
        conv = GINEConv(torch.nn.Linear(16, 16), in_dim=16, edge_dim=5, generator=g2).to(DEV)
        head = torch.nn.Linear(16, 4).to(DEV)
        params = list(conv.parameters()) + list(head.parameters())
        opt = torch.optim.Adam(params, lr=0.02)
        losses = []
        for _ in range(4):
            opt.zero_grad()
            loss = ((head(graph_readout(conv(x, b, e), b, "mean")) - target) ** 2).mean()
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        return torch.stack(losses), [p.detach().clone() for p in params]

    l1, p1 = run()
    l2, p2 = run()
    assert float(l1[3]) < float(l1[0])                       # the loss after three steps
    assert torch.equal(l1, l2) and all(torch.equal(a, c) for a, c in zip(p1, p2))
