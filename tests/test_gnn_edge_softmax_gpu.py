"""Oracle tests of the edge-softmax HIP kernels (gnn_edge_softmax.hip: edge_softmax_fwd_kernel,
edge_softmax_bwd_kernel) and of the layer API on top of them (``edge_softmax``, ``edge_dot``,
``AttentionConv``).

Every reference is computed here, in fp64 / numpy from the CSR -- never through the CPU
branches of ``ops``.  The backward takes its ``p`` as an input, so it is fed dyadic values and
compared bit for bit; the forward is compared with the fp64 softmax of the same fp32 scores
under an error bound derived from the kernel's operation sequence (test_forward_...).

The graphs: for every compiled sub-group width L the 53 row lengths of
test_gnn_pool_gpu.py's ``_degrees(L)`` (empty rows, 1, L - 1, L, L + 1, 2 L +- 1, 3 L + 5, ...)
and one row of 4099 edges, which leaves the in-register path (at most 4 L <= 256 edges).
Scores are head-major [K, ld] with ld = nnz + 5; the 5 gap elements of every head and a tail
past the last head hold a sentinel that must survive.
"""
import functools
import math

import numpy as np
import pytest
import torch

from cgnn_amd import native
from cgnn_amd.gnn import ops
from cgnn_amd.gnn.layers import AttentionConv, NormGraph, WeightedGraph, edge_dot, edge_softmax, weighted_aggregate
from cgnn_amd.gnn.sage import Block
from cgnn_amd.utils.hipgraph import StepGraph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -7.0           # sentinel of the elements a kernel must not write
GAP, TAIL = 5, 7
LANES = (8, 16, 32, 64)
HEADS = (1, 3, 8)
HUB = 4099
N_SRC = 257
U = 2.0 ** -24        # the unit roundoff of fp32
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------ helpers
def _degrees(L):
    """The row-length list of test_gnn_pool_gpu.py."""
    d = [0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, L - 1, L, L + 1, L + 4, L + 8, L + 13,
         2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 5]
    return d + d[::-1] + [2, L + 1, 0]


@functools.lru_cache(maxsize=None)
def _graph(L, hub=True, reverse=False):
    deg = _degrees(L) + ([HUB] if hub else [])
    assert len(deg) == 53 + int(hub)
    if reverse:
        deg = deg[::-1]
    deg = np.asarray(deg, dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    return dict(n=len(deg), deg=deg, rp=rp, nnz=int(rp[-1]), rows=np.repeat(np.arange(len(deg)), deg),
                rp_d=torch.from_numpy(rp).to(DEV))


def _auto_lanes(n_rows, nnz):
    """The launcher's rule, from its header."""
    return 8 if nnz <= 16 * n_rows else 16 if nnz <= 32 * n_rows else 32 if nnz <= 64 * n_rows else 64


def _buf(vals):
    """[K, nnz] fp64/fp32 values -> (device [K, nnz + GAP] view, its flat buffer with TAIL more
    elements); gaps and tail hold SENT."""
    K, nnz = vals.shape
    ld = nnz + GAP
    flat = torch.full((K * ld + TAIL,), SENT, dtype=F32)
    view = flat[:K * ld].view(K, ld)
    view[:, :nnz] = vals.to(F32)
    flat = flat.to(DEV)
    return flat[:K * ld].view(K, ld), flat


def _untouched(flat, K, nnz, what):
    ld = nnz + GAP
    f = flat.cpu()
    assert torch.all(f[:K * ld].view(K, ld)[:, nnz:] == SENT), what + ": the gap of a head was written"
    assert torch.all(f[K * ld:] == SENT), what + ": the tail past the last head was written"


def _same(got, exp):
    """Bit for bit, except that a NaN equals a NaN."""
    got, exp = got.double(), exp.double()
    return bool(torch.equal(torch.isnan(got), torch.isnan(exp))
                and torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(exp, nan=0.0)))


def _segsum(rows, n, v):
    """[K, nnz] fp64 numpy -> per-row sums [K, n] (np.add.at: plain fp64 adds in edge order)."""
    out = np.zeros((v.shape[0], n))
    for k in range(v.shape[0]):
        np.add.at(out[k], rows, v[k])
    return out


def _softmax_ref(g, s, scale):
    """fp64 softmax of the fp64 array s [K, nnz] per row; also max |scale (s - m)| per (head, row)."""
    n, rows = g["n"], g["rows"]
    m = np.full((s.shape[0], n), -INF)
    for k in range(s.shape[0]):
        np.maximum.at(m[k], rows, s[k])
    x = scale * (s - m[:, rows])
    ex = np.exp(x)
    p = ex / _segsum(rows, n, ex)[:, rows]
    X = np.zeros((s.shape[0], n))
    for k in range(s.shape[0]):
        np.maximum.at(X[k], rows, np.abs(x[k]))
    return p, X


def _scores(g, K, seed, spread=None):
    """fp32-representable scores [K, nnz] (fp64 tensor): normal times 3; ``spread``: every row of
    two or more edges is rescaled so that its maximum minus its minimum is that number."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((K, g["nnz"])) * 3
    if spread is not None:
        for i in range(g["n"]):
            e0, e1 = int(g["rp"][i]), int(g["rp"][i + 1])
            if e1 - e0 >= 2:
                seg = s[:, e0:e1]
                lo, hi = seg.min(1, keepdims=True), seg.max(1, keepdims=True)
                s[:, e0:e1] = (seg - lo) / (hi - lo) * spread
    return torch.from_numpy(s).float().double()


# ------------------------------------------------------------------ 1. backward, bit for bit
@pytest.mark.parametrize("L", LANES)
def test_backward_bit_for_bit_on_dyadic_values(L):
    """ds = scale p (dp - sum p dp) with p in {0, 1/8, ..., 1}, dp integers in [-3, 3], scale in
    {1, 1/2}: every product p dp is a multiple of 1/8, every partial sum of them a multiple of
    1/8 of magnitude at most 3 * 4099 < 2^14, (dp - sum) likewise, scale p a multiple of 1/16,
    the result a multiple of 1/128 below 2^14: all exact in fp32 (24 bits) in any order and
    with or without fused multiply-adds.  Asserted on the fp64 reference."""
    g = _graph(L)
    n, nnz, rows = g["n"], g["nnz"], g["rows"]
    for K in HEADS:
        rng = np.random.default_rng(100 * L + K)
        p = rng.integers(0, 9, (K, nnz)) / 8.0
        dp = rng.integers(-3, 4, (K, nnz)).astype(np.float64)
        assert float(_segsum(rows, n, np.abs(p * dp)).max()) < 2 ** 14
        for scale in (1.0, 0.5):
            ref = torch.from_numpy(scale * p * (dp - _segsum(rows, n, p * dp)[:, rows]))
            assert torch.equal(ref.float().double(), ref) and torch.equal((ref * 128).round(), ref * 128)
            assert float(ref.abs().max()) > 1
            P, _ = _buf(torch.from_numpy(p))
            for lanes in (L, None) if K == 3 else (L,):
                DP, _ = _buf(torch.from_numpy(dp))
                DS, flat = _buf(torch.zeros(K, nnz))
                out = ops.edge_softmax_bwd(g["rp_d"], P, DP, scale=scale, out=DS, lanes=lanes, nnz=nnz)
                assert out.data_ptr() == DS.data_ptr()
                what = "bwd L=%s K=%d scale=%g" % (lanes, K, scale)
                assert torch.equal(DS[:, :nnz].cpu().double(), ref), what
                _untouched(flat, K, nnz, what)
                # in place: ds over dp
                inp = ops.edge_softmax_bwd(g["rp_d"], P, DP, scale=scale, out=DP, lanes=lanes, nnz=nnz)
                assert inp.data_ptr() == DP.data_ptr() and torch.equal(DP, DS), what + " in place"


# ------------------------------------------------------------------ 2. forward against fp64
@pytest.mark.parametrize("L", LANES)
def test_forward_within_the_derived_bound_of_fp64(L):
    """The kernel computes, with u = 2^-24 and x = scale (s - m) the exact exponent,

        c = fl(scale log2 e)   one rounding (host)                     (1 + d1), |d1| <= u
        d = fl(s - m)          one rounding                            (1 + d2)
        t = fl(d c)            one rounding                            (1 + d3)
          so t = x log2 e (1 + th), |th| <= 3 u, and 2^t = e^x e^(x th): relative error 3 |x| u
        a = v_exp_f32(t)       one ulp, at most 2 u relative            -> (3 |x| + 2) u per term
        l = sum a              positive terms: the error of l is at most the largest error of a
                               term, (3 X + 2) u with X = max |x| over the row, plus one u per
                               inexact addition on the longest path: a lane adds its
                               ceil(deg / L) terms in a chain (the first addition, to 0, is
                               exact), then log2 L butterfly steps: depth = ceil(deg / L) - 1
                               + log2 L
        r = fl(1 / l)          correctly rounded division: u
        p = fl(a r)            u

    Summed to first order: |p - p*| / p* <= (3 |x| + 2 + 3 X + 2 + depth + 2) u
    <= (6 X + depth + 6) u; the neglected products of these terms are below
    ((6 X + depth + 6) u)^2 < u for every row here (6 * 16 + 516 + 6 = 618, 618^2 u < 0.03), so
    the bound asserted is (6 X + depth + 7) u, and never more than 1e-4 (the relative tolerance
    test_gat_fused_gpu.py gives the existing attention forward).  The reference results are far
    above the range where v_exp_f32 would flush (asserted: p* > 2^-100).

    The sum of a row's outputs: sum fl(a r) = (sum a) / l^ (1 + e_div)(1 + e_mul), where l^ is
    the computed sum of the very same a: the errors of the exponentials cancel and what is
    left is the summation error, at most min(deg - 1, depth) u (adding a lane's 0 is exact), and
    2 u: within (deg + 1) u <= deg 2^-23.

    Largest error observed on an MI355X as a fraction of the bound: see docs/KERNELS.md (the
    test prints it)."""
    g = _graph(L)
    n, nnz, deg, rows = g["n"], g["nnz"], g["deg"], g["rows"]
    depth = np.ceil(deg / L) - 1 + math.log2(L)
    worst = 0.0
    for K in HEADS:
        for scale, spread in ((1.0, None), (0.5, None), (1.0, 16.0)):
            s = _scores(g, K, 10 * L + K, spread)
            ref, X = _softmax_ref(g, s.numpy(), scale)
            if spread is not None:
                assert abs(float(X[:, deg >= 2].min()) - 16.0) < 1e-5
            assert float(ref.min()) > 2.0 ** -100
            bound = np.minimum((6 * X + depth[None, :] + 7) * U, 1e-4)[:, rows]
            S, _ = _buf(s)
            P, flat = _buf(torch.zeros(K, nnz))
            ops.edge_softmax(g["rp_d"], S, scale=scale, out=P, lanes=L, nnz=nnz)
            got = P[:, :nnz].cpu().double().numpy()
            what = "fwd L=%d K=%d scale=%g spread=%s" % (L, K, scale, spread)
            _untouched(flat, K, nnz, what)
            frac = np.abs(got - ref) / ref / bound
            worst = max(worst, float(frac.max()))
            print("%s: largest error / bound = %.3f (bound there %.3g)" % (what, frac.max(), bound.flat[frac.argmax()]))
            assert float(frac.max()) <= 1.0, what
            sums = _segsum(rows, n, got)
            assert np.all(np.abs(sums[:, deg > 0] - 1.0) <= deg[deg > 0] * 2.0 ** -23), what + ": row sums"
            assert np.all(sums[:, deg == 0] == 0)
            assert np.all(got[:, g["rp"][:-1][deg == 1]] == 1.0), what + ": single-edge rows"
    print("edge_softmax_fwd L=%d: largest error / bound over all cases = %.3f" % (L, worst))


# ------------------------------------------------------------------ 3. edge cases, exact
EDGE_ROWS = [[4.0], [1e30, 0.0, -1e30], [100.0, 100.0], [-INF, 1.0, -INF, 1.0], [-INF, -INF, -INF], [],
             [0.5, -INF, 2.0], [-INF], [1.0, 2.0, 3.0], [-INF] * 300, [-INF] * 150 + [7.0, 7.0] + [-INF] * 150]


@pytest.mark.parametrize("lanes", LANES + (None,))
def test_edge_cases_exact(lanes):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in EDGE_ROWS])]).astype(np.int32)
    rp_d = torch.from_numpy(rp).to(DEV)
    flat = torch.tensor([v for r in EDGE_ROWS for v in r], dtype=F64)
    nnz = flat.numel()
    S, _ = _buf(flat[None, :])
    P, pf = _buf(torch.full((1, nnz), 5.0))
    ops.edge_softmax(rp_d, S, out=P, lanes=lanes, nnz=nnz)
    p = P[0, :nnz].cpu()
    seg = [p[rp[i]:rp[i + 1]].tolist() for i in range(len(EDGE_ROWS))]
    assert seg[0] == [1.0]
    assert seg[1] == [1.0, 0.0, 0.0]
    assert seg[2] == [0.5, 0.5]
    assert seg[3] == [0.0, 0.5, 0.0, 0.5]
    assert seg[4] == [0.0, 0.0, 0.0]
    assert seg[6][1] == 0.0 and seg[6][0] > 0 and abs(seg[6][0] + seg[6][2] - 1) < 1e-6
    assert seg[7] == [0.0]
    assert seg[9] == [0.0] * 300
    assert seg[10] == [0.0] * 150 + [0.5, 0.5] + [0.0] * 150
    assert torch.isfinite(p).all()
    _untouched(pf, 1, nnz, "edge cases")
    # the scale is applied before the exponential: {100, 100} and 1e30 stay finite
    ops.edge_softmax(rp_d, S, scale=4.0, out=P, lanes=lanes, nnz=nnz)
    q = P[0, :nnz].cpu()
    assert q[rp[1]:rp[2]].tolist() == [1.0, 0.0, 0.0] and q[rp[2]:rp[3]].tolist() == [0.5, 0.5]


@pytest.mark.parametrize("L", LANES)
def test_a_nan_or_inf_poisons_exactly_its_row_and_head(L):
    """A NaN, or a +inf, in one (row, head): that segment is all NaN; every other output has the
    bits of a run in which the score is finite."""
    g = _graph(L)
    nnz, rp, deg = g["nnz"], g["rp"], g["deg"]
    K = 3
    s = _scores(g, K, 900 + L)
    S, _ = _buf(s)
    clean = ops.edge_softmax(g["rp_d"], S, lanes=L, nnz=nnz)[:, :nnz].cpu()
    assert torch.isfinite(clean).all()
    # a row of one edge, a short row, a row of 3 L + 5 edges, the hub row
    targets = [int(np.flatnonzero(deg == 1)[0]), int(np.flatnonzero(deg == 5)[0]),
               int(np.flatnonzero(deg == 3 * L + 5)[0]), int(np.flatnonzero(deg == HUB)[0])]
    for bad in (NAN, INF):
        for i in targets:
            e0, e1 = int(rp[i]), int(rp[i + 1])
            e = e0 + (e1 - e0) * 2 // 3                        # not the first element of the row
            s2 = s.clone()
            s2[1, e] = bad
            S2, _ = _buf(s2)
            P, flat = _buf(torch.zeros(K, nnz))
            ops.edge_softmax(g["rp_d"], S2, out=P, lanes=L, nnz=nnz)
            got = P[:, :nnz].cpu()
            what = "%s in row %d (deg %d), L=%d" % (bad, i, e1 - e0, L)
            assert torch.isnan(got[1, e0:e1]).all(), what
            exp = clean.clone()
            exp[1, e0:e1] = NAN
            assert _same(got, exp), what + ": another segment changed"
            _untouched(flat, K, nnz, what)


# ------------------------------------------------------------------ 4. determinism, position
@pytest.mark.parametrize("L", LANES)
def test_deterministic_and_independent_of_the_rows_position(L):
    g, gr = _graph(L), _graph(L, reverse=True)
    n, nnz, rp, rpr = g["n"], g["nnz"], g["rp"], gr["rp"]
    K = 3
    s = _scores(g, K, 40 + L)
    sr = torch.empty_like(s)
    for i in range(n):                                           # row i of g is row n - 1 - i of gr
        j = n - 1 - i
        sr[:, rpr[j]:rpr[j + 1]] = s[:, rp[i]:rp[i + 1]]
    dp = torch.from_numpy(np.random.default_rng(L).standard_normal((K, nnz))).float().double()
    dpr = torch.empty_like(dp)
    for i in range(n):
        j = n - 1 - i
        dpr[:, rpr[j]:rpr[j + 1]] = dp[:, rp[i]:rp[i + 1]]
    S, _ = _buf(s)
    DP, _ = _buf(dp)
    p1 = ops.edge_softmax(g["rp_d"], S, scale=0.5, lanes=L, nnz=nnz)
    p2 = ops.edge_softmax(g["rp_d"], S, scale=0.5, lanes=L, nnz=nnz)
    d1 = ops.edge_softmax_bwd(g["rp_d"], p1, DP, scale=0.5, lanes=L, nnz=nnz)
    d2 = ops.edge_softmax_bwd(g["rp_d"], p1, DP, scale=0.5, lanes=L, nnz=nnz)
    assert torch.equal(p1[:, :nnz], p2[:, :nnz]) and torch.equal(d1[:, :nnz], d2[:, :nnz])
    SR, _ = _buf(sr)
    DPR, _ = _buf(dpr)
    pr = ops.edge_softmax(gr["rp_d"], SR, scale=0.5, lanes=L, nnz=nnz)
    dr = ops.edge_softmax_bwd(gr["rp_d"], pr, DPR, scale=0.5, lanes=L, nnz=nnz)
    p1c, prc, d1c, drc = p1.cpu(), pr.cpu(), d1.cpu(), dr.cpu()
    for i in range(n):
        j = n - 1 - i
        assert torch.equal(prc[:, rpr[j]:rpr[j + 1]], p1c[:, rp[i]:rp[i + 1]]), "forward, row %d" % i
        assert torch.equal(drc[:, rpr[j]:rpr[j + 1]], d1c[:, rp[i]:rp[i + 1]]), "backward, row %d" % i


def test_auto_lanes_is_the_variant_the_rule_selects():
    """lanes=None on four graphs whose nnz / n_rows selects each compiled width in turn: the
    bits of that forced width."""
    seen = set()
    for L, hub in ((8, False), (32, False), (64, False), (16, True)):
        g = _graph(L, hub=hub)
        n, nnz = g["n"], g["nnz"]
        want = _auto_lanes(n, nnz)
        seen.add(want)
        s = _scores(g, 3, 60 + L)
        S, _ = _buf(s)
        auto = ops.edge_softmax(g["rp_d"], S, scale=0.5, nnz=nnz)
        forced = ops.edge_softmax(g["rp_d"], S, scale=0.5, lanes=want, nnz=nnz)
        assert torch.equal(auto[:, :nnz], forced[:, :nnz]), (L, hub, want)
        dp, _ = _buf(_scores(g, 3, 61 + L))
        assert torch.equal(ops.edge_softmax_bwd(g["rp_d"], auto, dp, scale=0.5, nnz=nnz)[:, :nnz],
                           ops.edge_softmax_bwd(g["rp_d"], auto, dp, scale=0.5, lanes=want, nnz=nnz)[:, :nnz])
    assert seen == set(LANES)


# ------------------------------------------------------------------ 5. in place
@pytest.mark.parametrize("L", LANES)
def test_forward_in_place(L):
    g = _graph(L)
    nnz = g["nnz"]
    for K in HEADS:
        s = _scores(g, K, 70 + L + K)
        S, _ = _buf(s)
        P, _ = _buf(torch.zeros(K, nnz))
        ops.edge_softmax(g["rp_d"], S, scale=0.5, out=P, lanes=L, nnz=nnz)
        S2, flat = _buf(s)
        out = ops.edge_softmax(g["rp_d"], S2, scale=0.5, out=S2, lanes=L, nnz=nnz)
        assert out.data_ptr() == S2.data_ptr() and torch.equal(S2[:, :nnz], P[:, :nnz])
        _untouched(flat, K, nnz, "in place L=%d K=%d" % (L, K))


# ------------------------------------------------------------------ 6. autograd composition
def _col(g, seed):
    rng = np.random.default_rng(seed)
    col = rng.integers(0, N_SRC, g["nnz"]).astype(np.int32)
    e0 = int(g["rp"][10])
    col[e0 + 1] = col[e0]                                        # a source repeated in one row
    col[0], col[-1] = 0, N_SRC - 1
    return col


def test_edge_dot_softmax_aggregate_composition_matches_fp64_cpu():
    """scores = edge_dot(a, b), alpha = edge_softmax(scores, scale), y = weighted_aggregate(x,
    val=alpha): one forward / backward on the GPU in fp32 against the same code in fp64 on the
    CPU, rtol = atol = 1e-4 (inputs O(1))."""
    g = _graph(16)
    n, nnz = g["n"], g["nnz"]
    col = _col(g, 1)
    rng = np.random.default_rng(2)
    a0, b0 = rng.standard_normal((n, 16)), rng.standard_normal((N_SRC, 16))
    x0, c0 = rng.standard_normal((N_SRC, 24)), rng.standard_normal((n, 24))

    def run(dev, dt):
        wg = WeightedGraph(torch.from_numpy(g["rp"]).to(dev), torch.from_numpy(col).to(dev),
                           torch.ones(nnz, device=dev), n_src=N_SRC)
        a, b, x = (torch.from_numpy(t).to(dt).to(dev).requires_grad_() for t in (a0, b0, x0))
        alpha = edge_softmax(edge_dot(a, b, wg), wg, scale=0.25)
        y = weighted_aggregate(x, wg, val=alpha)
        y.backward(torch.from_numpy(c0).to(dt).to(dev))
        return [t.detach().double().cpu().numpy() for t in (alpha, y, a.grad, b.grad, x.grad)]

    ref = run("cpu", F64)
    got = run(DEV, F32)
    for name, r, o in zip(("alpha", "y", "da", "db", "dx"), ref, got):
        assert float(np.abs(r).max()) > 1e-2, name
        np.testing.assert_allclose(o, r, rtol=1e-4, atol=1e-4, err_msg=name)


def test_edge_dot_gradients_bit_exact_on_integers():
    """a, b integers in [-2, 2] (F = 12), the cotangent integers in [-3, 3]: the products and
    every partial sum are integers below 2^24, so fp32 is exact in any order."""
    g = _graph(16)
    n, nnz, rows = g["n"], g["nnz"], g["rows"]
    col = _col(g, 3)
    rng = np.random.default_rng(4)
    a0 = rng.integers(-2, 3, (n, 12)).astype(np.float64)
    b0 = rng.integers(-2, 3, (N_SRC, 12)).astype(np.float64)
    c0 = rng.integers(-3, 4, nnz).astype(np.float64)
    blk = Block(g["rp"], col, N_SRC, DEV)
    a, b = (torch.from_numpy(t).float().to(DEV).requires_grad_() for t in (a0, b0))
    buf = torch.full((2, nnz), SENT, device=DEV)
    out = edge_dot(a, b, blk, out=buf[1])
    assert out.dtype == F32 and out.data_ptr() == buf[1].data_ptr()
    out.backward(torch.from_numpy(c0).float().to(DEV))
    assert torch.equal(out.detach().cpu().double(), torch.from_numpy((a0[rows] * b0[col]).sum(1)))
    assert torch.all(buf[0] == SENT)
    da, db = np.zeros_like(a0), np.zeros_like(b0)
    np.add.at(da, rows, c0[:, None] * b0[col])
    np.add.at(db, col, c0[:, None] * a0[rows])
    assert 10 < float(np.abs(da).max()) < 2 ** 24 and 10 < float(np.abs(db).max()) < 2 ** 24
    assert torch.equal(a.grad.cpu().double(), torch.from_numpy(da))
    assert torch.equal(b.grad.cpu().double(), torch.from_numpy(db))


# ------------------------------------------------------------------ 7. AttentionConv
@pytest.mark.parametrize("kind", ["block", "norm"])
def test_attention_conv_gpu_fp32_matches_cpu_fp64(kind):
    g = _graph(16, hub=False)
    n = g["n"]
    col = _col(g, 5)
    n_src = N_SRC if kind == "block" else n
    if kind == "norm":
        col = (col % n).astype(np.int32)
    rng = np.random.default_rng(6)
    h0, c0 = rng.standard_normal((n_src, 12)), rng.standard_normal((n, 32))

    def graph(dev):
        if kind == "block":
            return Block(g["rp"], col, N_SRC, dev)
        return NormGraph(torch.from_numpy(g["rp"]).to(dev), torch.from_numpy(col).to(dev), torch.ones(n, device=dev))

    def run(dev, dt):
        m = AttentionConv(12, 4, 8, generator=torch.Generator().manual_seed(7))
        with torch.no_grad():
            m.b_q.fill_(0.25)
            m.b_v.fill_(-0.5)
        m = m.to(dt).to(dev)
        h = torch.from_numpy(h0).to(dt).to(dev).requires_grad_()
        out, alpha = m(h, graph(dev), return_attention=True)
        out.backward(torch.from_numpy(c0).to(dt).to(dev))
        grads = {k: p.grad.double().cpu().numpy() for k, p in m.named_parameters()}
        grads["h"] = h.grad.double().cpu().numpy()
        return out.detach().double().cpu().numpy(), alpha.detach().double().cpu().numpy(), grads

    out_c, alpha_c, grads_c = run("cpu", F64)
    out_g, alpha_g, grads_g = run(DEV, F32)
    assert out_g.shape == (n, 32) and alpha_g.shape == (4, g["nnz"])
    np.testing.assert_allclose(out_g, out_c, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(alpha_g, alpha_c, rtol=1e-4, atol=1e-4)
    assert len(grads_c) == 9
    for k in grads_c:
        np.testing.assert_allclose(grads_g[k], grads_c[k], rtol=1e-4, atol=1e-4, err_msg=k)
    # (the key bias shifts every score of a row alike: its gradient is 0 up to rounding)
    assert sum(float(np.abs(v).max()) > 1e-3 for v in grads_c.values()) >= len(grads_c) - 1


def test_attention_conv_bf16_input():
    g = _graph(16, hub=False)
    blk = Block(g["rp"], _col(g, 5), N_SRC, DEV)
    m = AttentionConv(12, 4, 8, concat=False, generator=torch.Generator().manual_seed(7)).to(DEV)
    h = torch.randn(N_SRC, 12, generator=torch.Generator().manual_seed(8)).to(BF16).to(DEV)
    out, alpha = m(h, blk, return_attention=True)
    assert out.dtype == BF16 and out.shape == (g["n"], 8) and alpha.dtype == F32
    assert torch.isfinite(out.float()).all()
    sums = _segsum(g["rows"], g["n"], alpha.detach().double().cpu().numpy())
    assert np.all(np.abs(sums[:, g["deg"] > 0] - 1) < 1e-5)
    ref = m(h.float(), blk).detach()
    assert torch.allclose(out.detach().float(), ref, rtol=5e-2, atol=5e-2)    # bf16 storage: 2^-8 per rounding


# ------------------------------------------------------------------ 8. capture
def test_forward_and_backward_in_a_captured_graph():
    """edge_softmax + edge_softmax_bwd into preallocated buffers, captured and replayed twice
    with new inputs written into the captured buffers: the eager bits each time."""
    g = _graph(16)
    nnz, K = g["nnz"], 3
    S, _ = _buf(torch.zeros(K, nnz))
    DP, _ = _buf(torch.zeros(K, nnz))
    P, pf = _buf(torch.zeros(K, nnz))
    DS, df = _buf(torch.zeros(K, nnz))

    def step():
        ops.edge_softmax(g["rp_d"], S, scale=0.5, out=P, nnz=nnz)
        ops.edge_softmax_bwd(g["rp_d"], P, DP, scale=0.5, out=DS, nnz=nnz)

    def inputs(seed):
        S[:, :nnz] = _scores(g, K, seed).float().to(DEV)
        DP[:, :nnz] = _scores(g, K, seed + 1).float().to(DEV)

    eager = []
    for seed in (31, 33):
        inputs(seed)
        step()
        torch.cuda.synchronize()
        eager.append((P.clone(), DS.clone()))
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[0][1], eager[1][1])
    sg = StepGraph(step, warmup=1, device=torch.device(DEV))
    sg()                                                   # eager warm-up
    for k, seed in enumerate((31, 33)):
        inputs(seed)
        P[:, :nnz] = 3.0
        DS[:, :nnz] = 3.0
        sg()
        assert sg.graph is not None
        torch.cuda.synchronize()
        assert torch.equal(P, eager[k][0]) and torch.equal(DS, eager[k][1]), "replay %d" % k
    _untouched(pf, K, nnz, "captured forward")
    _untouched(df, K, nnz, "captured backward")


# ------------------------------------------------------------------ 9. launcher codes
def test_launcher_codes_and_empty_inputs():
    hip = native.hip()
    g = _graph(8)
    n, nnz = g["n"], g["nnz"]
    st = torch.cuda.current_stream().cuda_stream
    K, ld = 2, nnz + GAP
    S = torch.zeros(K, ld, device=DEV)
    P = torch.full((K, ld), SENT, device=DEV)
    D = torch.full((K, ld), SENT, device=DEV)
    rp = g["rp_d"].data_ptr()

    def fwd(rowptr=rp, s=S.data_ptr(), p=P.data_ptr(), n_rows=n, nnz=nnz, K=K, ld=ld, scale=1.0, lanes=0):
        hip.gnn_edge_softmax_fwd(rowptr, s, p, n_rows, nnz, K, ld, scale, lanes, st)

    def bwd(rowptr=rp, p=S.data_ptr(), dp=P.data_ptr(), ds=D.data_ptr(), n_rows=n, nnz=nnz, K=K, ld=ld, scale=1.0,
            lanes=0):
        hip.gnn_edge_softmax_bwd(rowptr, p, dp, ds, n_rows, nnz, K, ld, scale, lanes, st)

    with pytest.raises(RuntimeError, match="-5") as weighted:           # the type of the other bindings' error
        ops.wspmm(g["rp_d"], torch.zeros(nnz, dtype=torch.int32, device=DEV), torch.ones(nnz, device=DEV),
                  torch.ones(4, 16, device=DEV), 16, out=torch.empty(n, 16, dtype=BF16, device=DEV))
    bad = [dict(ld=nnz - 1), dict(K=0), dict(scale=0.0), dict(scale=-1.0), dict(scale=NAN), dict(scale=INF),
           dict(p=0)]
    for f in (fwd, bwd):
        for kw in bad:
            with pytest.raises(RuntimeError, match="-3") as ei:
                f(**kw)
            assert ei.type is weighted.type
        with pytest.raises(RuntimeError, match="-1"):
            f(lanes=3)
        with pytest.raises(RuntimeError, match="-4"):                    # heads x row blocks over the grid limit
            f(K=1 << 24, ld=nnz)
        f(n_rows=0)                                                      # code 0, nothing launched
        f(nnz=0, ld=0, s=0, p=0) if f is fwd else f(nnz=0, ld=0, p=0, dp=0, ds=0)
    with pytest.raises(RuntimeError, match="-3"):
        fwd(s=0)
    with pytest.raises(RuntimeError, match="-3"):
        bwd(dp=0)
    with pytest.raises(RuntimeError, match="-3"):
        bwd(ds=0)
    torch.cuda.synchronize()
    assert torch.all(P == SENT) and torch.all(D == SENT)
    # rows but no edges: an empty score (null pointer)
    rp0 = torch.zeros(10, dtype=torch.int32, device=DEV)
    e = torch.zeros(0, device=DEV)
    assert ops.edge_softmax(rp0, e).numel() == 0 and ops.edge_softmax_bwd(rp0, e, e).numel() == 0
    e2 = torch.zeros(3, 0, device=DEV)
    assert ops.edge_softmax(rp0, e2).shape == (3, 0)
    blk0 = Block(np.zeros(10, dtype=np.int32), np.zeros(0, dtype=np.int32), 5, DEV)
    sc = torch.zeros(2, 0, device=DEV, requires_grad=True)
    edge_softmax(sc, blk0).sum().backward()
    assert sc.grad.shape == (2, 0)
    # fp32 only on the GPU
    for dt in (F64, BF16):
        with pytest.raises(TypeError):
            ops.edge_softmax(g["rp_d"], S.to(dt))
        with pytest.raises(TypeError):
            ops.edge_softmax_bwd(g["rp_d"], S.to(dt), S.to(dt))
    with pytest.raises(ValueError):
        ops.edge_softmax(g["rp_d"], S[:, ::2])                           # not contiguous
