"""Exact oracle tests of the GNN sparse and elementwise HIP kernels (gnn_sparse.hip,
gnn_gather.h).

Every reference is computed here, in fp64, from a dense count matrix of the graph --
never through the CPU branches of ``ops``, which are fp32 and share helper code with the
GPU callers.  The sparse inputs are small integers and the scales powers of two, so every
partial sum is exactly representable in fp32 whatever the order of the adds: the
comparison is ``torch.equal`` against the fp64 result cast to the output type, not a
tolerance.  Tolerances appear only for Adam and for the transcendental part of the fused
cross-entropy, each with its basis at the assertion.
"""
import functools

import numpy as np
import pytest
import torch

from cgnn_amd import native
from cgnn_amd.gnn import ops
from cgnn_amd.utils.hipgraph import StepGraph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 7.0            # sentinel of rows / buffers a kernel must not write
BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64


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
    return torch.from_numpy(rp), torch.from_numpy(col)


def _count_matrix(rp, col, n_src):
    """Dense fp64 count matrix A[i, j] = number of entries j in row i."""
    n = rp.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n), (rp[1:] - rp[:-1]).long())
    A = torch.zeros(n, n_src, dtype=F64)
    A.index_put_((rows, col.long()), torch.ones(col.numel(), dtype=F64), accumulate=True)
    return A


def _ints(rng, lo, hi, shape):
    """fp64 tensor of integers in [lo, hi]."""
    return torch.from_numpy(rng.integers(lo, hi + 1, shape).astype(np.float64))


def _pow2(rng, n):
    """fp64 scales drawn from {0.5, 1, 2}."""
    return torch.from_numpy(rng.choice([0.5, 1.0, 2.0], n))


def _fp32_exact(ref):
    """The reference survives a round trip through fp32 (what makes the test exact)."""
    return torch.equal(ref.float().double(), ref)


def _assert_same(got, exp, what):
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero()
        i, j = (int(x) for x in bad[0])
        raise AssertionError("%s: %d elements differ, first at [%d, %d]: got %r, expected %r"
                             % (what, bad.shape[0], i, j, float(got[i, j]), float(exp[i, j])))


# ------------------------------------------------------------------ 1. SpMM
N_SRC = 257


def _spmm_degrees(L):
    d = [0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, L - 1, L, L + 1, L + 4, L + 8, L + 13,
         2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 5]
    # the list, the list reversed (neighbouring sub-groups on different trip counts), and
    # three more rows: 53 rows, no multiple of the 4 * (64 / L) rows of a block for any L
    return d + d[::-1] + [2, L + 1, 0]


@functools.lru_cache(maxsize=None)
def _spmm_graph(L):
    rng = np.random.default_rng(100 + L)
    deg = _spmm_degrees(L)
    assert len(deg) % (4 * (64 // L)) != 0
    rp, col = _csr(deg, N_SRC, rng)
    return dict(n=len(deg), rp=rp.to(DEV), col=col.to(DEV), A=_count_matrix(rp, col, N_SRC),
                rs=_pow2(rng, len(deg)), cs=_pow2(rng, N_SRC))


# (F, ld, L): L lanes per row, from max(F, written columns); the last is two 512-column slabs
SPMM_WIDTHS = [(8, 8, 8), (41, 48, 8), (64, 64, 8), (65, 72, 16), (128, 128, 16), (129, 136, 32),
               (256, 256, 32), (257, 264, 64), (512, 512, 64), (520, 528, 64)]
# every (input, output, column scale) combination the launcher compiles
SPMM_PAIRS = [(BF16, BF16, False), (BF16, F32, False), (F32, BF16, False), (F32, F32, False),
              (F16, F16, False), (F16, F32, False), (F32, F16, False),
              (BF16, BF16, True), (F16, F16, True), (F32, F32, True)]
# (relu, init on a prefix of the rows, bias, row scale)
SPMM_CONFIGS = [(False, False, False, False), (True, True, True, True), (False, True, True, True),
                (True, False, True, False)]


@pytest.mark.parametrize("F,ld,L", SPMM_WIDTHS)
def test_spmm_exact_over_row_lengths_and_dtypes(F, ld, L):
    """spmm_kernel / spmm_short_kernel against the fp64 count-matrix product, bit for bit:
    rows of every length class of gather_sum<L> (16-, 8-, 4- and 1-steps, one to four
    chunks), all seven dtype pairs and the three with a column scale, relu on and off, an
    init on a prefix of the rows, and three sentinel rows past the output."""
    g = _spmm_graph(L)
    n, A = g["n"], g["A"]
    rng = np.random.default_rng(1000 + F)
    Xd = torch.zeros(N_SRC, ld, dtype=F64)
    Xd[:, :F] = _ints(rng, -3, 3, (N_SRC, F))
    bias = _ints(rng, -2, 2, (F,))
    init_rows = n - 11
    init = torch.zeros(init_rows, ld, dtype=F64)
    init[:, :F] = _ints(rng, -4, 4, (init_rows, F))
    unit_col = F if ld > 512 else -1
    agg = {False: A @ Xd[:, :F], True: A @ (g["cs"][:, None] * Xd[:, :F])}
    rs_d, cs_d = g["rs"].float().to(DEV), g["cs"].float().to(DEV)
    bias_d, init_d = bias.float().to(DEV), init.float().to(DEV)
    for xdt, ydt, use_cs in SPMM_PAIRS:
        X = Xd.to(xdt).to(DEV)
        for relu, use_init, use_bias, use_rs in SPMM_CONFIGS:
            ref = agg[use_cs].clone()
            if use_init:
                ref[:init_rows] += init[:, :F]
            if use_rs:
                ref = ref * g["rs"][:, None]
            if use_bias:
                ref = ref + bias
            if relu:
                ref = ref.clamp_min(0)
            assert _fp32_exact(ref) and float(ref.abs().max()) < 4096
            exp = torch.zeros(n, ld, dtype=F64)
            exp[:, :F] = ref
            if unit_col >= 0:
                exp[:, unit_col] = 1
            exp = exp.to(ydt)
            for short in (False, True):
                full = torch.full((n + 3, ld), SENT, dtype=ydt, device=DEV)
                ops.spmm(g["rp"], g["col"], X, F, rscale=rs_d if use_rs else None,
                         bias=bias_d if use_bias else None, relu=relu, out=full[:n], unit_col=unit_col,
                         init=init_d if use_init else None, init_rows=init_rows if use_init else None,
                         cscale=cs_d if use_cs else None, short_rows=short)
                got = full.cpu()
                what = "%s->%s cs=%d relu=%d init=%d bias=%d rs=%d short=%d" % (
                    xdt, ydt, use_cs, relu, use_init, use_bias, use_rs, short)
                _assert_same(got[:n], exp, what)
                assert torch.all(got[n:] == SENT), what + ": rows past n_rows written"


# (1030, 1032): a third 512-column slab holding 6 features, the ones column and one padding
# column; (500, 1032): slabs two and three hold padding only, the ones column in the third
@pytest.mark.parametrize("F,ld,unit_col", [(1030, 1032, 1030), (500, 1032, 1030)])
def test_spmm_exact_past_the_second_slab(F, ld, unit_col):
    """9 rows, 40 edges: every dtype pair, both kernels, the epilogue with everything on and
    with everything off; zero padding columns, and nothing written past the last row."""
    rng = np.random.default_rng(1500 + F)
    rp, col = _csr([3, 0, 1, 9, 4, 5, 7, 9, 2], N_SRC, rng)
    n, A = 9, _count_matrix(rp, col, N_SRC)
    assert col.numel() == 40
    rs, cs = _pow2(rng, n), _pow2(rng, N_SRC)
    Xd = torch.zeros(N_SRC, ld, dtype=F64)
    Xd[:, :F] = _ints(rng, -3, 3, (N_SRC, F))
    bias = _ints(rng, -2, 2, (F,))
    init_rows = n - 2
    init = torch.zeros(init_rows, ld, dtype=F64)
    init[:, :F] = _ints(rng, -4, 4, (init_rows, F))
    agg = {False: A @ Xd[:, :F], True: A @ (cs[:, None] * Xd[:, :F])}
    rp_d, col_d, rs_d, cs_d = rp.to(DEV), col.to(DEV), rs.float().to(DEV), cs.float().to(DEV)
    bias_d, init_d = bias.float().to(DEV), init.float().to(DEV)
    for xdt, ydt, use_cs in SPMM_PAIRS:
        X = Xd.to(xdt).to(DEV)
        for on in (False, True):
            ref = agg[use_cs].clone()
            if on:
                ref[:init_rows] += init[:, :F]
                ref = (ref * rs[:, None] + bias).clamp_min(0)
            assert _fp32_exact(ref) and float(ref.abs().max()) < 4096
            exp = torch.zeros(n, ld, dtype=F64)
            exp[:, :F] = ref
            exp[:, unit_col] = 1
            for short in (False, True):
                full = torch.full((n + 3, ld), SENT, dtype=ydt, device=DEV)
                ops.spmm(rp_d, col_d, X, F, rscale=rs_d if on else None, bias=bias_d if on else None, relu=on,
                         out=full[:n], unit_col=unit_col, init=init_d if on else None,
                         init_rows=init_rows if on else None, cscale=cs_d if use_cs else None, short_rows=short)
                got = full.cpu()
                what = "%s->%s cs=%d epilogue=%d short=%d F=%d" % (xdt, ydt, use_cs, on, short, F)
                _assert_same(got[:n], exp.to(ydt), what)
                assert torch.all(got[n:] == SENT), what + ": written past the last row's stride"


def test_spmm_mixed_pair_with_column_scale_raises():
    """A column scale is compiled for the same-type pairs only: the launcher's code -5."""
    g = _spmm_graph(8)
    X = torch.ones(N_SRC, 8, dtype=BF16, device=DEV)
    cs = torch.ones(N_SRC, device=DEV)
    for short in (False, True):
        with pytest.raises(RuntimeError, match="-5"):
            ops.spmm(g["rp"], g["col"], X, 8, cscale=cs, out_dtype=F32, short_rows=short)


# ------------------------------------------------------------------ 2. ELL
ELL_DEG = [0, 1, 7, 8, 9, 16, 17, 70]


def _ell_check(deg, F, seed):
    """One-shot kernel, pipelined kernel and the fp64 reference agree bit for bit."""
    n, ld = len(deg), -(-F // 8) * 8
    rng = np.random.default_rng(seed)
    rp, col = _csr(deg, N_SRC, rng)
    A = _count_matrix(rp, col, N_SRC)
    Xd = torch.zeros(N_SRC, ld, dtype=F64)
    Xd[:, :F] = _ints(rng, -3, 3, (N_SRC, F))
    rs = _pow2(rng, n)
    rp_d, col_d, X = rp.to(DEV), col.to(DEV), Xd.to(BF16).to(DEV)
    img = ops.ell_image(rp_d, col_d)
    assert img.n_long == sum(d > 8 for d in deg) == img.long_rows.numel()
    for use_rs in (True, False):
        ref = A @ Xd[:, :F]
        if use_rs:
            ref = ref * rs[:, None]
        assert _fp32_exact(ref)
        exp = torch.zeros(n, ld, dtype=F64)       # padding columns are written 0
        exp[:, :F] = ref
        exp = exp.to(BF16)
        for oneshot in (False, True):
            full = torch.full((n + 3, ld), SENT, dtype=BF16, device=DEV)
            ops.spmm_ell(img, col_d, X, F, rscale=rs.float().to(DEV) if use_rs else None, out=full[:n],
                         oneshot=oneshot)
            got = full.cpu()
            what = "n=%d F=%d rs=%d oneshot=%d" % (n, F, use_rs, oneshot)
            _assert_same(got[:n], exp, what)
            assert torch.all(got[n:] == SENT), what + ": rows past n written"
    return img


@pytest.mark.parametrize("F", [8, 47, 64])
@pytest.mark.parametrize("n", [1, 7, 9, 33, 257])
def test_spmm_ell_oneshot_and_pipelined_exact(n, F):
    """spmm_ell_kernel (``oneshot=True``: a null long-row pointer) and spmm_ell_pipe_kernel
    on interleaved degrees {0, 1, 7, 8, 9, 16, 17, 70} (short rows, the 8-entry row, long
    rows of one to nine chunks), from two starting points of the cycle."""
    for rot in (0, 5):
        _ell_check([ELL_DEG[(i + rot) % 8] for i in range(n)], F, 10 * n + F + rot)


def test_spmm_ell_image_without_long_rows_exact():
    """An image with no row above 8 entries: its long-row list is empty and the launch gets
    a valid one-element buffer with n_long = 0 (which kernel ran cannot be seen from here:
    both forms must give the exact result)."""
    img = _ell_check([[0, 1, 7, 8][i % 4] for i in range(33)], 47, 5)
    assert img.n_long == 0 and img.long_rows.numel() == 0 and img.long_buf.numel() == 1


# ------------------------------------------------------------------ 5. fused cross-entropy (+ its reference, used by 3.)
def _ce_reference(logits, labels, mask, rs, inv):
    """fp64 log-softmax / NLL / softmax - one-hot of fp32 ``logits`` (the kernel's logits
    are exact sums with one fp32 rounding at the bias add, so they are inputs here).
    Returns (loss, accuracy counts of masks 1..3, per-class dlogits sums, G values)."""
    n, C = logits.shape
    lg = logits.double()
    lsm = torch.log_softmax(lg, 1)
    y = labels.long()
    tr = mask == 1
    loss = -(lsm[tr, y[tr]]).sum()
    ismax = logits == logits.max(1, keepdim=True).values
    pred = torch.where(ismax, torch.arange(C)[None, :], C).min(1).values     # ties: lowest class id
    counts = torch.tensor([int(((pred == y) & (mask == k)).sum()) for k in (1, 2, 3)], dtype=F32)
    dl = torch.softmax(lg, 1)
    dl[torch.arange(n), y] -= 1
    dl = dl * (tr[:, None].double() * inv)
    return loss, counts, dl.sum(0), dl * rs[:, None]


def _ce_check(stats, G, ref, C, ld):
    """Tolerances of test_spmm_ce_matches_reference (the loss and gradients pass through
    __expf / __logf and a bf16 store); the accuracy counts are integers: exact."""
    loss, counts, dsum, gval = ref
    s = stats.cpu()
    assert torch.equal(s[1:4], counts), (s[1:4], counts)
    np.testing.assert_allclose(s[0].numpy(), loss.numpy(), rtol=1e-3, atol=1e-2)
    np.testing.assert_allclose(s[4:4 + C].numpy(), dsum.numpy(), atol=1e-5)
    if G is not None:
        g = G.cpu().float()
        np.testing.assert_allclose(g[:, :C].numpy(), gval.numpy(), atol=2e-5, rtol=2e-2)
        assert torch.all(g[:, C:] == 0)


CE_DEG = [0, 1, 8, 9, 63, 64, 65, 130]


@functools.lru_cache(maxsize=None)
def _ce_graph():
    """43 rows (no multiple of 8) of degrees {0, 1, 8, 9, 63, 64, 65, 130}, ordered long
    rows (above 60 entries) first as spmm_ce's n_long mode wants them."""
    rng = np.random.default_rng(55)
    n = 43
    deg = torch.tensor([CE_DEG[i % 8] for i in range(n)])
    order, k = ops.long_row_order(deg, threshold=60)
    assert k == 20
    rp, col = _csr(deg[order].tolist(), n, rng)
    return dict(n=n, k=k, rp=rp, col=col, A=_count_matrix(rp, col, n), rs=_pow2(rng, n),
                mask=torch.from_numpy(rng.integers(0, 4, n).astype(np.uint8)))


def _ce_inputs(C, ld, ties, seed):
    g = _ce_graph()
    n = g["n"]
    rng = np.random.default_rng(seed)
    Zd = torch.zeros(n, ld, dtype=F64)
    Zd[:, :C] = _ints(rng, -3, 3, (n, C))
    labels = torch.from_numpy(rng.integers(0, C, n).astype(np.int32))
    if ties and C > 1:
        # two classes (in different lanes when C > 8) share every row's top logit: both
        # columns are 3 in every source row, the others at most 2; zero bias.  Rows
        # without entries tie over all classes.
        ta, tb = (3, 40) if C > 40 else (min(3, C - 2), C - 1)
        Zd[:, :C] = Zd[:, :C].clamp_max(2)
        Zd[:, ta] = Zd[:, tb] = 3
        labels = torch.from_numpy(rng.choice([0, ta, tb, C // 2], n).astype(np.int32))
        bias = torch.zeros(C)
    else:
        bias = torch.from_numpy(rng.standard_normal(C).astype(np.float32))
    agg = (g["A"] @ Zd[:, :C]) * g["rs"][:, None]
    assert _fp32_exact(agg)
    logits = agg.float() + bias            # one fp32 rounding, as in the kernel (fused or not)
    inv = 1.0 / float((g["mask"] == 1).sum())
    ref = _ce_reference(logits, labels, g["mask"], g["rs"], inv)
    dev = dict(rp=g["rp"].to(DEV), col=g["col"].to(DEV), Z=Zd.to(BF16).to(DEV), rs=g["rs"].float().to(DEV),
               bias=bias.to(DEV), labels=labels.to(DEV), mask=g["mask"].to(DEV))
    return g, dev, inv, ref


def _ce_run(d, C, inv, **kw):
    return ops.spmm_ce(d["rp"], d["col"], d["Z"], C, d["rs"], d["bias"], d["labels"], d["mask"], inv, **kw)


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("C,ld", [(1, 8), (8, 8), (9, 16), (9, 32), (47, 48), (64, 64)])
def test_spmm_ce_class_counts_modes_and_ties(C, ld, ties):
    """spmm_ce_kernel over class counts and row pitches, masks {0, 1, 2, 3}, rows of 0 to
    130 entries with and without the whole-wave mode for the long ones, a compact G
    through gslot, mode 1, and arg-max ties.  Per row the two row modes give identical
    bits (the aggregate is exact, the rest is per row): G and the integer counts must
    agree bit for bit.  The loss and the per-class sums are fixed-order fp32 sums over the
    rows of a wave, a block and the grid, and n_long changes which rows share a wave: they
    are compared bit for bit only between launches of the same n_long."""
    g, d, inv, ref = _ce_inputs(C, ld, ties, 7 * C + ld)
    n, k = g["n"], g["k"]
    s0, G0 = _ce_run(d, C, inv, mode=0, n_long=0)
    _ce_check(s0, G0, ref, C, ld)
    s1, G1 = _ce_run(d, C, inv, mode=0, n_long=k)
    _ce_check(s1, G1, ref, C, ld)
    assert torch.equal(s0[1:4], s1[1:4])
    same = {0: s0[:4 + C].view(torch.int32), k: s1[:4 + C].view(torch.int32)}
    assert torch.equal(G0.view(torch.int16), G1.view(torch.int16))
    # compact G: the train rows to every second slot, nothing else written
    train = (g["mask"] == 1).nonzero().flatten()
    gslot = torch.full((n,), -1, dtype=torch.int32)
    gslot[train] = 2 * torch.arange(train.numel(), dtype=torch.int32)
    for n_long in (0, k):
        Gc = torch.full((2 * train.numel() + 2, ld), SENT, dtype=BF16, device=DEV)
        sc, _ = _ce_run(d, C, inv, mode=0, G=Gc, gslot=gslot.to(DEV), n_long=n_long)
        Gc = Gc.cpu()
        assert torch.equal(Gc[0:2 * train.numel():2].view(torch.int16), G0.cpu()[train].view(torch.int16))
        assert torch.all(Gc[1::2] == SENT) and torch.all(Gc[2 * train.numel():] == SENT)
        assert torch.equal(sc[:4 + C].view(torch.int32), same[n_long])
    # mode 1 writes no G; same statistics
    Gs = torch.full((n, ld), SENT, dtype=BF16, device=DEV)
    sm, _ = _ce_run(d, C, inv, mode=1, G=Gs, n_long=k)
    assert torch.all(Gs == SENT)
    assert torch.equal(sm[:4 + C].view(torch.int32), same[k])


def test_spmm_ce_more_than_64_classes_raises():
    g, d, inv, _ = _ce_inputs(9, 72, False, 1)
    with pytest.raises(RuntimeError, match="-3"):
        _ce_run(d, 65, inv, mode=1)


# ------------------------------------------------------------------ 3. a graph with no edges
@pytest.mark.parametrize("n", [1, 37])
def test_spmm_without_edges(n):
    """nnz = 0 (an empty ``col``): Y = act(rscale * init + bias), exactly, from both row
    kernels (the launch gets a valid one-element id buffer), and spmm_fan writes zeros on
    its pipelined path and on its fallback to the CSR kernel."""
    rng = np.random.default_rng(n)
    rp = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    col = torch.empty(0, dtype=torch.int32, device=DEV)
    n_src = 5
    rs, cs = _pow2(rng, n), _pow2(rng, n_src)
    for F, ld in [(8, 8), (41, 48), (129, 136)]:
        bias = _ints(rng, -2, 2, (F,))
        init = torch.zeros(n, ld, dtype=F64)
        init[:, :F] = _ints(rng, -4, 4, (n, F))
        for dt, use_cs, relu in [(BF16, False, True), (F32, True, False), (F16, False, False)]:
            X = _ints(rng, -3, 3, (n_src, ld)).to(dt).to(DEV)
            ref = init[:, :F] * rs[:, None] + bias
            if relu:
                ref = ref.clamp_min(0)
            exp = torch.zeros(n, ld, dtype=F64)
            exp[:, :F] = ref
            exp = exp.to(dt)
            for short in (None, False, True):
                full = torch.full((n + 3, ld), SENT, dtype=dt, device=DEV)
                ops.spmm(rp, col, X, F, rscale=rs.float().to(DEV), bias=bias.float().to(DEV), relu=relu,
                         out=full[:n], init=init.float().to(DEV), cscale=cs.float().to(DEV) if use_cs else None,
                         short_rows=short)
                got = full.cpu()
                _assert_same(got[:n], exp, "F=%d %s short=%s" % (F, dt, short))
                assert torch.all(got[n:] == SENT)
        if F <= 128:
            X = _ints(rng, -3, 3, (n_src, ld)).to(BF16).to(DEV)
            for max_deg in (8, 9):
                full = torch.full((n + 3, ld), SENT, dtype=BF16, device=DEV)
                ops.spmm_fan(rp, col, X, F, max_deg, rscale=rs.float().to(DEV), out=full[:n])
                got = full.cpu()
                assert torch.all(got[:n] == 0) and torch.all(got[n:] == SENT)


@pytest.mark.parametrize("n", [1, 37])
def test_spmm_ce_without_edges(n):
    """nnz = 0: the logits are the bias alone.  Accuracy counts exact; the loss and the
    gradients pass through __expf / __logf, so they take the tolerances of
    test_spmm_ce_matches_reference."""
    rng = np.random.default_rng(20 + n)
    C, ld = 9, 16
    rp = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    col = torch.empty(0, dtype=torch.int32, device=DEV)
    Z = _ints(rng, -3, 3, (n, ld)).to(BF16).to(DEV)
    rs = _pow2(rng, n)
    bias = torch.from_numpy(rng.standard_normal(C).astype(np.float32))
    labels = torch.from_numpy(rng.integers(0, C, n).astype(np.int32))
    mask = torch.from_numpy(rng.integers(0, 4, n).astype(np.uint8))
    mask[0] = 1
    inv = 1.0 / float((mask == 1).sum())
    ref = _ce_reference(bias[None, :].repeat(n, 1), labels, mask, rs, inv)
    stats, G = ops.spmm_ce(rp, col, Z, C, rs.float().to(DEV), bias.to(DEV), labels.to(DEV), mask.to(DEV), inv,
                           mode=0)
    _ce_check(stats, G, ref, C, ld)


# ------------------------------------------------------------------ 4. Adam
# Hyper-parameters exactly representable in fp32 (the kernel takes them as float
# arguments): the fp64 reference, the fp32 CPU branch and the kernel then run the same
# constants, and what is left between them is rounding.
ADAM_N = 65537                  # ops.adam_ folds the step counter up to 256 * 256 elements
ADAM_HP = dict(lr=2.0 ** -7, b1=0.875, b2=1 - 2.0 ** -10, eps=1e-8)
ADAM_STEPS = 5


def _adam_ref_step(p, m, v, g, t, wd):
    """The update of gnn_adam_kernel (PyTorch semantics, decoupled decay) in fp64."""
    lr, b1, b2, eps = ADAM_HP["lr"], ADAM_HP["b1"], ADAM_HP["b2"], ADAM_HP["eps"]
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    mh = m / (1 - b1 ** t)
    vh = v / (1 - b2 ** t)
    return p - lr * (mh / (vh.sqrt() + eps) + wd * p), m, v


@functools.lru_cache(maxsize=None)
def _adam_case(wd):
    """Inputs of the largest size (the smaller sizes take prefixes: the update is
    elementwise), the fp64 trajectory, and the tolerance: 4 x the largest error of the
    fp32 CPU branch of ops.adam_ against it after the same five steps."""
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(ADAM_N, generator=gen)
    grads = [torch.randn(ADAM_N, generator=gen) for _ in range(ADAM_STEPS)]
    traj, state = [], (p0.double(), torch.zeros(ADAM_N, dtype=F64), torch.zeros(ADAM_N, dtype=F64))
    for t in range(1, ADAM_STEPS + 1):
        state = _adam_ref_step(*state, grads[t - 1].double(), t, wd)
        traj.append(state)
    p, m, v = p0.clone(), torch.zeros(ADAM_N), torch.zeros(ADAM_N)
    step = torch.zeros(1, dtype=torch.int32)
    for g in grads:
        ops.adam_(p, g, m, v, step_t=step, wd=wd, **ADAM_HP)
    cpu_err = [float((a.double() - b).abs().max()) for a, b in zip((p, m, v), traj[-1])]
    return p0, grads, traj, cpu_err


def _adam_close(got, ref, cpu_err, what):
    # tolerance: 4 x the fp32 CPU branch's own largest error against the fp64 reference
    # on these inputs (measured: param 4.6e-07 without and 5.0e-07 with decay, m 1.1e-07, v 3.3e-09) --
    # the device powf, sqrtf and divide are each within a few ulp of the CPU's
    for name, a, b, e in zip(("param", "m", "v"), got, ref, cpu_err):
        err = float((a.cpu().double() - b).abs().max())
        print("adam %s %s: max error %.3e, CPU branch %.3e, bound %.3e" % (what, name, err, e, 4 * e))
        assert err <= 4 * e, (what, name, err, 4 * e)


def _adam_gpu_state(p0, n):
    return (p0[:n].clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV),
            torch.zeros(1, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65536, 65537])
def test_adam_values_and_step_counter(n, wd):
    """Five steps with fresh gradients against the fp64 update; the counter is 5 exactly
    and, where the last block advances it (up to 65536 elements), the arrival counter
    is back at 0.  65537 elements: the separate increment."""
    p0, grads, traj, cpu_err = _adam_case(wd)
    p, m, v, step = _adam_gpu_state(p0, n)
    for g in grads:
        ops.adam_(p, g[:n].to(DEV), m, v, step_t=step, wd=wd, **ADAM_HP)
    assert int(step.item()) == ADAM_STEPS
    if n <= 256 * 256:
        assert int(ops._ADAM_DONE[(step.device.index, step.data_ptr())].item()) == 0
    _adam_close((p, m, v), [x[:n] for x in traj[-1]], cpu_err, "n=%d wd=%g" % (n, wd))


@pytest.mark.parametrize("n", [1, 257, 65537])
def test_adam_step_done_uses_the_counter_as_is(n):
    """``step_done=True`` (a slab_sum bump advanced the counter): t = step_t, not
    step_t + 1, and step_t is left alone."""
    wd = 0.01
    p0, grads, traj, cpu_err = _adam_case(wd)
    start = [x[:n].float() for x in traj[1]]              # the state after two steps, as fp32
    ref3 = _adam_ref_step(*[x.double() for x in start], grads[2][:n].double(), 3, wd)
    ref4 = _adam_ref_step(*[x.double() for x in start], grads[2][:n].double(), 4, wd)
    assert float((ref3[0] - ref4[0]).abs().max()) > 100 * 4 * cpu_err[0]     # t + 1 would be seen
    p, m, v = (x.clone().to(DEV) for x in start)
    step = torch.full((1,), 3, dtype=torch.int32, device=DEV)
    ops.adam_(p, grads[2][:n].to(DEV), m, v, step_t=step, wd=wd, step_done=True, **ADAM_HP)
    assert int(step.item()) == 3
    _adam_close((p, m, v), ref3, cpu_err, "step_done n=%d" % n)


def test_adam_folded_counter_in_a_captured_graph():
    """A folded adam_ captured in a hipGraph (one stream, no parallel branches): one
    eager step, then three replays -- the counter, read and advanced on the device, moves
    by 3 and the values follow the reference."""
    n, wd = 257, 0.0
    p0, grads, traj, cpu_err = _adam_case(wd)
    p, m, v, step = _adam_gpu_state(p0, n)
    g = torch.zeros(n, device=DEV)
    sg = StepGraph(lambda: ops.adam_(p, g, m, v, step_t=step, wd=wd, **ADAM_HP), warmup=1, device=torch.device(DEV))
    g.copy_(grads[0][:n])
    sg()                                                   # eager
    assert sg.graph is None and int(step.item()) == 1
    for t in (1, 2, 3):
        g.copy_(grads[t][:n])
        sg()
        assert sg.graph is not None
    torch.cuda.synchronize()
    assert int(step.item()) == 4
    assert int(ops._ADAM_DONE[(step.device.index, step.data_ptr())].item()) == 0
    _adam_close((p, m, v), [x[:n] for x in traj[3]], cpu_err, "graph")


def test_adam_counter_passes_2_to_the_24():
    """The folded counter is an integer: from 2**24 one step leaves 2**24 + 1 (a counter
    stored from the float t of the powers would stay at 2**24)."""
    n = 257
    p0, grads, _, _ = _adam_case(0.0)
    p, m, v, step = _adam_gpu_state(p0, n)
    step.fill_(2 ** 24)
    ops.adam_(p, grads[0][:n].to(DEV), m, v, step_t=step, **ADAM_HP)
    assert int(step.item()) == 2 ** 24 + 1
    assert bool(torch.isfinite(p).all())


# ------------------------------------------------------------------ 6. elementwise kernels
def test_cast_bf16_every_rounding_case_bitwise():
    """cast_bf16_kernel against torch's fp32 -> bf16 conversion on every fp32 whose high
    half is a non-NaN bf16 and whose low half is one of {0x0000, 0x7fff, 0x8000, 0x8001,
    0xffff}: ties to even both ways, the carry into the exponent, max-finite -> inf,
    denormals and both zeros.  NaN inputs are out of scope (an infinity's high half with a
    non-zero low half is a NaN: left out)."""
    hi = torch.arange(0x10000, dtype=torch.int64)
    lo = torch.tensor([0x0000, 0x7fff, 0x8000, 0x8001, 0xffff], dtype=torch.int64)
    bits = ((hi[:, None] << 16) | lo[None, :]).flatten()
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    x = bits.view(F32)
    x = x[~torch.isnan(x)].contiguous()
    assert x.numel() == 5 * (0x10000 - 2 * 128) + 2      # + the two infinities themselves
    exp = x.to(BF16)
    src = x.to(DEV)
    dst = torch.zeros(x.numel() + 8, dtype=BF16, device=DEV)
    native.hip().gnn_cast_bf16(src.data_ptr(), dst.data_ptr(), x.numel(), ops._st(src))
    got = dst.cpu()
    assert torch.equal(got[:x.numel()].view(torch.int16), exp.view(torch.int16))
    assert torch.all(got[x.numel():].view(torch.int16) == 0)


@pytest.mark.parametrize("n", [8, 2056])
@pytest.mark.parametrize("p", [0.0, 0.5, 0.3])
def test_relu_dropout_bwd_bitwise(n, p):
    """relu_dropout_bwd_kernel: dH * [H > 0] / (1 - p), the scale formed in fp32 as the
    launcher forms it, the product rounded once to bf16; H holds +0, -0, positive and
    negative values."""
    rng = np.random.default_rng(n)
    H = torch.from_numpy(rng.choice([0.0, -0.0, 1.5, -2.0, 0.0078125, -1e-3], n).astype(np.float32)).to(BF16)
    dH = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(BF16)
    dH[::5] = 0
    dH[1::7] = -dH[1::7].abs()
    scale = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
    exp = torch.where(H.float() > 0, dH.float() * scale, torch.zeros(n)).to(BF16)
    got = ops.relu_dropout_bwd_(dH.clone().to(DEV), H.to(DEV), p).cpu()
    assert torch.equal(got.view(torch.int16), exp.view(torch.int16))


def test_relu_dropout_bwd_rejects_a_length_off_the_vector_width():
    dH = torch.zeros(12, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError, match="-3"):
        ops.relu_dropout_bwd_(dH, torch.ones(12, dtype=BF16, device=DEV), 0.5)
