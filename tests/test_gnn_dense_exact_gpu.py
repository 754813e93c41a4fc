"""Exact oracle tests of the fused dense GCN kernels on MFMA (gnn_dense.hip):
gcn_dense_fwd_kernel, gcn_dense_bwd_kernel, gcn_fused_bwd_kernel and the keep image.

Every reference is computed here, in fp64 -- never through the CPU branches of
``ops.dense_fwd`` / ``ops.dense_bwd``, which round P1 to bf16 before the bias and so are a
different function.  AX and dY2 hold small integers, W1 / b1 / W2 multiples of 1/4 in
[-1, 1] (bf16-exact: the in-kernel fp32 -> bf16 conversion changes nothing) and dinv
values from {0.5, 1, 2}.  Every MFMA product is then exact and every partial sum a
multiple of a known quantum; each case builder asserts, on its own data, that
sum|terms| / quantum < 2^24 for every output element, so the fp32 accumulation is exact in
any order.  H1, Z2, dP1 and the weight gradients are then single correct roundings of
exactly known numbers and are compared with ``torch.equal``.  The only tolerances are at
p = 0.3, where bf16(W2 / 0.7) has arbitrary low bits; each is derived at its assertion.

The case builders and references (everything above the ``GPU runs`` line) make no GPU
call: tests/test_gnn_dense_exact_cpu.py runs their exactness preconditions and
self-checks without a device.
"""
import functools

import numpy as np
import pytest
import torch

from cgnn_amd.gnn import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 7.0            # sentinel of rows / buffers a kernel must not write
PAD = 5.0             # finite junk in the padding columns of a row (they meet zero weights)
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
KEY, STEP = (31, 41), 5
PS = (0.0, 0.5, 0.3)  # no dropout, bit mode, byte mode
TILE = 32
EXACT = float(2 ** 24)


# ------------------------------------------------------------------ number helpers
def _ints(rng, lo, hi, shape):
    """fp64 tensor of integers in [lo, hi]."""
    return torch.from_numpy(rng.integers(lo, hi + 1, shape).astype(np.float64))


def _quarters(rng, shape):
    """fp64 multiples of 1/4 in [-1, 1] (bf16-exact)."""
    return torch.from_numpy(rng.integers(-4, 5, shape).astype(np.float64) / 4.0)


def _pow2(rng, n):
    """fp64 scales drawn from {0.5, 1, 2}."""
    return torch.from_numpy(rng.choice([0.5, 1.0, 2.0], n))


def _fp32_exact(x):
    """x (fp64) survives a round trip through fp32."""
    return torch.equal(x.float().double(), x)


def _bf16r(x):
    """Round-to-nearest-even bf16 image of an fp32-exact fp64 tensor, as fp64: ONE rounding
    (fp64 -> fp32 is exact by the assertion, fp32 -> bf16 rounds to nearest even)."""
    assert _fp32_exact(x), "reference value is not fp32-exact: the case is mis-sized"
    return x.float().to(BF16).double()


def scale32(p):
    """The kernels' 1.f / (1.f - p), evaluated in fp32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def _mul32(x, s):
    """float32(x) * float32(s) rounded to fp32 (x fp32-exact fp64), as fp64."""
    assert _fp32_exact(x)
    return (x.float() * torch.tensor(s, dtype=F32)).double()


def assert_exact_sums(abs_sum, quantum, what):
    """sum|terms| / quantum < 2^24 for every output element: every partial sum, in any
    order, is an integer multiple of ``quantum`` below 2^24 quanta -- exact in fp32."""
    worst = float(abs_sum.max()) / quantum if abs_sum.numel() else 0.0
    assert worst < EXACT, "%s: sum|terms| / quantum = %g >= 2^24; shrink the input ranges" % (what, worst)


def relu_bf16(P1):
    """bf16(P1) then relu, negative values and -0 to +0 (the kernels' signed 16-bit max)."""
    h = _bf16r(P1)
    return torch.where(h > 0, h, torch.zeros_like(h))


def tight(k):
    """Smallest multiple of 8 that covers k columns."""
    return (k + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def keep_mask(n, HD, p, row0):
    """Reference dropout mask (numpy Philox mirror), bool [n][HD]."""
    return ops.dropout_keep_mask(n, HD, p, KEY, STEP, row0)


def encode_keep_image(keep, HD):
    """The documented keep image of a bool mask [n][HD] (int16 halfwords): halfword
    (T * HD/32 + t) * 64 + 32 uh + r, bit 4 g + i  <->  row 32 T + r, unit
    32 t + 8 g + 4 uh + i.  Rows past n are not defined by the layout (zero here)."""
    n = keep.shape[0]
    nt, NB = (n + TILE - 1) // TILE, HD // 32
    full = torch.zeros(nt * TILE, HD, dtype=torch.int64)
    full[:n] = keep.long()
    q = torch.arange(16)
    g, i = q // 4, q % 4
    words = torch.zeros(nt, NB, 2, TILE, dtype=torch.int64)
    for uh in range(2):
        for t in range(NB):
            units = 32 * t + 8 * g + 4 * uh + i
            bits = full[:, units].view(nt, TILE, 16)
            words[:, t, uh] = (bits << q).sum(-1)
    words = torch.where(words >= 32768, words - 65536, words)
    return words.to(torch.int16).view(-1)


def decode_keep_image(kimg, n, HD):
    """bool mask [n][HD] of a keep image (any device), the inverse of encode_keep_image."""
    nt, NB = (n + TILE - 1) // TILE, HD // 32
    dev = kimg.device
    words = kimg.view(nt, NB, 2, TILE).to(torch.int32) & 0xffff
    q = torch.arange(16, device=dev)
    bits = ((words[..., None] >> q) & 1).bool()                    # [T][t][uh][r][q]
    g, i = q // 4, q % 4
    keep = torch.zeros(nt * TILE, HD, dtype=torch.bool, device=dev)
    for uh in range(2):
        for t in range(NB):
            keep[:, 32 * t + 8 * g + 4 * uh + i] = bits[:, t, uh].reshape(nt * TILE, 16)
    return keep[:n]


# ------------------------------------------------------------------ forward: cases and reference
# (F, ldx): exactly on a template (KS = 4, 7, 8), and below one with a tight row pitch
FWD_WIDTHS = [(64, 64), (112, 112), (128, 128), (1, 8), (17, 24), (20, 24), (40, 48), (65, 72), (80, 88),
              (100, 104), (113, 120)]
# (C, ldc), cycled across the widths: one class, C <= 32 (second accumulator all padding),
# both accumulators partly / fully used
FWD_CLASSES = [(1, 8), (7, 8), (32, 32), (33, 40), (47, 48), (49, 56), (64, 64)]
FWD_CASES = [(F, ldx) + FWD_CLASSES[k % len(FWD_CLASSES)] for k, (F, ldx) in enumerate(FWD_WIDTHS)]
FWD_N = 77            # 3 tiles, the last one partial


@functools.lru_cache(maxsize=None)
def fwd_case(n, F, ldx, C, ldc, HD):
    """Inputs of one forward case and the dropout-independent part of its reference."""
    rng = np.random.default_rng(1000 * F + 10 * C + HD)
    AX = torch.full((n, ldx), PAD, dtype=F64)         # padding (ones column included): finite junk
    AX[:, :F] = _ints(rng, -3, 3, (n, F))
    W1, b1, W2 = _quarters(rng, (F, HD)), _quarters(rng, (HD,)), _quarters(rng, (HD, C))
    dinv = _pow2(rng, n)
    assert_exact_sums(AX[:, :F].abs() @ W1.abs() + b1.abs(), 0.25, "P1 + b1")
    Hu = relu_bf16(AX[:, :F] @ W1 + b1)               # before dropout, without 1/(1-p)
    return dict(n=n, F=F, ldx=ldx, C=C, ldc=ldc, HD=HD, AX=AX, W1=W1, b1=b1, W2=W2, dinv=dinv, Hu=Hu)


def fwd_expected(c, p, keep):
    """(H1, Z2, zraw, zabs) of a forward case under the keep mask (None: no dropout).
    H1 = bf16(float32(Hk) * float32(w2s)), Hk the kept bf16 values; Z2 = bf16(zraw) padded
    to ldc with zeros, zraw = dinv * (Hk @ bf16(W2 * w2s)) -- exact for p in {0, 1/2};
    for other p Z2 is None and (zraw, zabs = dinv * sum|terms|) feed the derived bound."""
    w2s = scale32(p) if p > 0 else 1.0
    Hk = c["Hu"] if keep is None else torch.where(keep, c["Hu"], torch.zeros_like(c["Hu"]))
    H1 = _bf16r(_mul32(Hk, w2s))
    W2s = _bf16r(_mul32(c["W2"], w2s))
    zraw = c["dinv"][:, None] * (Hk @ W2s)
    zabs = c["dinv"][:, None] * (Hk.abs() @ W2s.abs())
    Z2 = None
    if p in (0.0, 0.5):
        # Hk: multiples of 1/4; W2s: multiples of 1/4 (p = 0) or 1/2 (p = 1/2)
        assert_exact_sums(Hk.abs() @ W2s.abs(), 1.0 / 16, "H1 W2")
        Z2 = torch.zeros(c["n"], c["ldc"], dtype=F64)
        Z2[:, :c["C"]] = _bf16r(zraw)
    return H1, Z2, zraw, zabs


def z2_from_h1(c, p, H1_got):
    """(zraw, zabs) of layer 2 alone, from the H1 the kernel itself stored (fp64 [n][HD]):
    dinv * (H1_got / scale) @ bf16(W2 * scale).  Separates a layer-1 fault from a layer-2 one."""
    w2s = scale32(p) if p > 0 else 1.0
    W2s = _bf16r(_mul32(c["W2"], w2s))
    Hk = H1_got / w2s
    return c["dinv"][:, None] * (Hk @ W2s), c["dinv"][:, None] * (Hk.abs() @ W2s.abs())


# ------------------------------------------------------------------ dense_bwd: cases and reference
BWD_NS = [1, 32, 77]
BWD_CLASSES = [(7, 8), (33, 40), (47, 48), (49, 56), (64, 64)]         # (C, ldc): KC = 1, 3, 3, 4, 4
# bf16 bit patterns of H1: +0, -0, the smallest positive subnormal, a negative subnormal,
# positive and negative normals; the derivative is 1 only for the positive ones
H1_BITS = [0x0000, 0x8000, 0x0001, 0x8001, 0x3FC0, 0xC000, 0x4248, 0xBE80, 0x3C00, 0x0000]


@functools.lru_cache(maxsize=None)
def bwd_case(n, C, ldc, HD):
    rng = np.random.default_rng(7000 + 100 * n + C + HD)
    dY2 = torch.full((n, ldc), PAD, dtype=F64)        # padding columns: finite junk
    dY2[:, :C] = _ints(rng, -3, 3, (n, C))
    W2 = _quarters(rng, (HD, C))
    bits = np.asarray(H1_BITS, dtype=np.uint16)[rng.integers(0, len(H1_BITS), (n, HD))]
    H1 = torch.from_numpy(bits.view(np.int16).copy()).view(BF16)
    assert_exact_sums(dY2[:, :C].abs() @ W2.abs().t(), 0.25, "dY2 W2^T")
    dh = dY2[:, :C] @ W2.t()
    return dict(n=n, C=C, ldc=ldc, HD=HD, dY2=dY2, W2=W2, H1=H1, dh=dh, alive=H1.float() > 0)


def bwd_expected(c, p):
    """dP1 = bf16(float32(dh) * m), m = float32(1 / (1 - p)) where H1 > 0, else 0."""
    return _bf16r(_mul32(c["dh"], scale32(p))) * c["alive"]


# ------------------------------------------------------------------ fused_bwd: cases and reference
FUSED_NS = [1, 31, 32, 33, 77]
FUSED_F = {4: (48, 63), 7: (96, 100, 111), 8: (112, 127)}             # by KS = ceil((F + 1) / 16)
FUSED_CLASSES = [(33, 40), (47, 48), (48, 48), (49, 56), (64, 64)]     # (C, ldc): KC = 3, 3, 3, 4, 4
# the (KS, KC, HD) combinations gnn_launch_fused_bwd compiles
FUSED_TABLE = {(7, 3, 256), (7, 4, 256), (8, 3, 256), (8, 4, 256), (4, 3, 256), (4, 4, 256),
               (7, 3, 128), (8, 3, 128), (4, 3, 128), (8, 4, 128)}


def fused_width(F):
    """Row width of a slab: the feature columns (F + 1, with the ones column) padded to
    whole 16-tiles and then to 32, plus 64 class columns."""
    KP = (F + 1 + 15) // 16 * 16
    return (KP + 31) // 32 * 32 + 64


@functools.lru_cache(maxsize=8)
def fused_case(n, F, ldx, C, ldc, HD, amp=3):
    """Inputs of a fused-backward case; AX[:, F] = 1 (the ones column), all other padding 0
    (so that every padding column of a slab is exactly 0)."""
    rng = np.random.default_rng(9000 + 1000 * F + 10 * C + HD + n)
    AX = torch.zeros(n, ldx, dtype=F64)
    AX[:, :F] = _ints(rng, -amp, amp, (n, F))
    AX[:, F] = 1.0
    dY2 = torch.zeros(n, ldc, dtype=F64)
    dY2[:, :C] = _ints(rng, -amp, amp, (n, C))
    W1, b1, W2 = _quarters(rng, (F, HD)), _quarters(rng, (HD,)), _quarters(rng, (HD, C))
    assert_exact_sums(AX[:, :F].abs() @ W1.abs() + b1.abs(), 0.25, "P1 + b1")
    assert_exact_sums(dY2[:, :C].abs() @ W2.abs().t(), 0.25, "dY2 W2^T")
    Hu = relu_bf16(AX[:, :F] @ W1 + b1)
    dhb = _bf16r(dY2[:, :C] @ W2.t())
    return dict(n=n, F=F, ldx=ldx, C=C, ldc=ldc, HD=HD, AX=AX, dY2=dY2, W1=W1, b1=b1, W2=W2, Hu=Hu, dhb=dhb,
                dinv=torch.ones(n, dtype=F64))


def fused_expected(c, p, keep, nb):
    """The per-block slabs [nb][HD][width] (fp64 holding fp32 values) of a fused backward
    on ``nb`` blocks (block b contracts the tiles b, b + nb, ...): the fp64 contraction of
    the bf16 images of H1 (without 1/(1-p)) and dP1 with the rows of AX / dY2, times
    float32(1/(1-p)) in fp32.  Also the totals (gW1 [F][HD], gb1, gW2) where they are
    order-independent (p in {0, 1/2}), else None."""
    n, F, C, HD = c["n"], c["F"], c["C"], c["HD"]
    Hk = c["Hu"] if keep is None else torch.where(keep, c["Hu"], torch.zeros_like(c["Hu"]))
    D = c["dhb"] * (Hk > 0)
    width = fused_width(F)
    kf = width - 64
    # Hk, D: multiples of 1/4; AX, dY2: integers
    assert_exact_sums(D.abs().t() @ c["AX"].abs(), 0.25, "gW1 / gb1")
    assert_exact_sums(Hk.abs().t() @ c["dY2"].abs(), 0.25, "gW2")
    nt = (n + TILE - 1) // TILE

    def tiles(x):
        out = torch.zeros(nt * TILE, x.shape[1], dtype=F64)
        out[:n] = x
        return out.view(nt, TILE, x.shape[1])
    # the kernel stages min(ldx, 16 KS) feature and min(ldc, 16 KC) class columns
    xs, ys = min(c["ldx"], (F + 1 + 15) // 16 * 16), min(c["ldc"], (C + 15) // 16 * 16)
    per_tile = torch.zeros(nt, HD, width, dtype=F64)
    per_tile[:, :, :xs] = torch.einsum("trh,trf->thf", tiles(D), tiles(c["AX"][:, :xs]))
    per_tile[:, :, kf:kf + ys] = torch.einsum("trh,trc->thc", tiles(Hk), tiles(c["dY2"][:, :ys]))
    slabs = torch.zeros(nb, HD, width, dtype=F64)
    slabs.index_add_(0, torch.arange(nt) % nb, per_tile)
    if p > 0:
        slabs = _mul32(slabs, scale32(p))
    total = None
    if p in (0.0, 0.5):
        t = slabs.sum(0)
        assert _fp32_exact(t)
        total = (t[:, :F].t().contiguous(), t[:, F].contiguous(), t[:, kf:kf + C].contiguous())
    return slabs, total


def fused_big_n(cus):
    """At least 3 tiles per block (the double buffer behind the tile-after-next prefetch),
    some blocks a 4th, the last tile partial."""
    return TILE * (3 * cus + 2) + 5


# ------------------------------------------------------------------ forward, several tiles per wave
FWD_BIG = dict(F=100, ldx=104, C=47, ldc=48, HD=256, period=1009)


def fwd_big_n(cus):
    """Waves of the persistent forward grid (16 per CU) get 2 or 3 tiles; last tile partial."""
    return TILE * (2 * 16 * cus + 5) + 7


@functools.lru_cache(maxsize=None)
def fwd_big_case():
    """One period (1009 rows, prime: no alignment with tiles, waves or blocks) of the
    periodic big forward case."""
    b = FWD_BIG
    return fwd_case(b["period"], b["F"], b["ldx"], b["C"], b["ldc"], b["HD"])


def big_mask_ranges(n, cus):
    """Row ranges whose masks are checked against the Philox mirror: the first 64 tiles,
    64 tiles from tile 16 * CUs (every wave's second tile starts there), the last 6."""
    nt = (n + TILE - 1) // TILE
    return [(0, 64 * TILE), (16 * cus * TILE, (16 * cus + 64) * TILE), ((nt - 6) * TILE, n)]


# ================================================================== GPU runs
def _assert_same(got, exp, what):
    if got.shape != exp.shape or not torch.equal(got, exp):
        assert got.shape == exp.shape, "%s: shape %r, expected %r" % (what, tuple(got.shape), tuple(exp.shape))
        bad = (got != exp).nonzero()
        idx = tuple(int(x) for x in bad[0])
        raise AssertionError("%s: %d elements differ, first at %r: got %r, expected %r"
                             % (what, bad.shape[0], idx, float(got[idx]), float(exp[idx])))


def _dev(x, dtype, canary=False, tail=float("nan")):
    """x on the device as ``dtype``; ``canary``: as the leading slice of a larger
    allocation whose remainder is ``tail`` (a read past the tensor then meets NaN, in
    memory the test owns)."""
    x = x.to(dtype)
    if not canary:
        return x.to(DEV)
    extra = 4 if x.dim() == 2 else 64
    big = torch.full((x.shape[0] + extra,) + tuple(x.shape[1:]), tail, dtype=dtype, device=DEV)
    big[:x.shape[0]] = x.to(DEV)
    return big[:x.shape[0]]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run_fwd(c, p, row0, store_h1, canary=False, tail=float("nan")):
    """One dense_fwd launch into sentinel-framed buffers; (H1 | None, Z2, kimg | None) with
    H1 / Z2 on the CPU as fp64, sentinel rows checked."""
    n, HD, ldc = c["n"], c["HD"], c["ldc"]
    Hbuf = torch.full((n + 3, HD), SENT, dtype=BF16, device=DEV)
    Zbuf = torch.full((n + 3, ldc), SENT, dtype=BF16, device=DEV)
    kimg = None
    if not store_h1 and p > 0:
        kimg = ops.keep_image(n, HD, DEV).fill_(0x5555)
    ok = ops.dense_fwd(_dev(c["AX"], BF16, canary, tail), _dev(c["W1"], F32), _dev(c["b1"], F32), _dev(c["W2"], F32),
                       _dev(c["dinv"], F32, canary, tail), Hbuf[:n] if store_h1 else None, Zbuf[:n], c["F"], p, KEY, STEP,
                       row0, kimg=kimg)
    assert ok, "dense_fwd: no compiled variant for F = %d, HD = %d" % (c["F"], HD)
    torch.cuda.synchronize()
    Hc, Zc = Hbuf.cpu().double(), Zbuf.cpu().double()
    assert bool((Zc[n:] == SENT).all()), "Z2: rows past n written"
    assert bool((Hc[n:] == SENT).all()), "H1: rows past n written"
    if not store_h1:
        assert bool((Hc == SENT).all()), "H1 = None: the buffer was written"
    return (Hc[:n] if store_h1 else None), Zc[:n], kimg


def _check_z2(c, p, Zgot, exp, H1_got, tag):
    H1, Z2, zraw, zabs = exp
    C = c["C"]
    _assert_same(Zgot[:, C:], torch.zeros_like(Zgot[:, C:]), tag + " Z2 padding columns")
    if Z2 is not None:
        _assert_same(Zgot, Z2, tag + " Z2")
    else:
        # p = 0.3: bf16(W2 / 0.7) has 8 arbitrary bits, the sums depend on the order.
        # |got - ref| <= 2^-8 |ref| (one bf16 rounding) + 256 * 2^-24 * sum|terms|
        # (fp32 accumulation over 256 terms)
        bound = 2.0 ** -8 * zraw.abs() + 256 * 2.0 ** -24 * zabs
        err = (Zgot[:, :C] - zraw).abs()
        assert bool((err <= bound).all()), "%s Z2: max excess %g" % (tag, float((err - bound).max()))
    if H1_got is None:
        return
    # layer 2 alone, from the kernel's own stored H1
    zr, za = z2_from_h1(c, p, H1_got)
    if p in (0.0, 0.5):
        exp2 = torch.zeros_like(Zgot)
        exp2[:, :C] = _bf16r(zr)
        _assert_same(Zgot, exp2, tag + " Z2 against the stored H1")
    else:
        # as above, plus 2^-8 sum|terms|: the stored H1 = bf16(Hk * scale) carries one more
        # bf16 rounding per term than the Hk the kernel multiplied
        bound = 2.0 ** -8 * zr.abs() + (256 * 2.0 ** -24 + 2.0 ** -8) * za
        err = (Zgot[:, :C] - zr).abs()
        assert bool((err <= bound).all()), "%s Z2 against the stored H1: max excess %g" % (tag, float((err - bound).max()))


def _row0(HD):
    return 4096 if HD == 128 else 0


@pytest.mark.parametrize("F,ldx,C,ldc", FWD_CASES)
def test_dense_fwd_exact_every_template(F, ldx, C, ldc):
    """gcn_dense_fwd_kernel at every compiled (KS, HD, dropout mode), exactly on a template
    and below it with a tight row pitch (the KS <= ks dispatch), 3 tiles with a partial
    last one: H1 and Z2 bit for bit against fp64 (Z2 at p = 0.3 within the derived bound),
    Z2 also against the kernel's own H1, Z2 identical with H1 = None plus a keep image,
    that image equal to the reference mask, sentinel rows and zero padding columns."""
    for HD in (256, 128):
        c = fwd_case(FWD_N, F, ldx, C, ldc, HD)
        for p in PS:
            tag = "F=%d ldx=%d C=%d ldc=%d HD=%d p=%g" % (F, ldx, C, ldc, HD, p)
            keep = keep_mask(FWD_N, HD, p, _row0(HD)) if p > 0 else None
            exp = fwd_expected(c, p, keep)
            Hgot, Zgot, _ = _run_fwd(c, p, _row0(HD), True)
            _assert_same(Hgot, exp[0], tag + " H1")
            _check_z2(c, p, Zgot, exp, Hgot, tag)
            _, Znone, kimg = _run_fwd(c, p, _row0(HD), False)
            _assert_same(Znone, Zgot, tag + " Z2 with H1 = None")
            if p > 0:
                _assert_same(decode_keep_image(kimg, FWD_N, HD).cpu(), keep, tag + " keep image")


@pytest.mark.parametrize("F,ldx,C,ldc", FWD_CASES)
def test_dense_fwd_reads_nothing_past_its_inputs(F, ldx, C, ldc):
    """AX and dinv as leading slices of allocations whose remainder is NaN: the outputs
    equal the fp64 reference and the run with zeros in place of the NaN.  A k-step that
    reads past the row pitch on the last row meets NaN there; NaN * 0 weight = NaN, which
    the MFMA returns with the sign bit set, so the signed-integer relu turns that whole
    row of H1 (and Z2) into zeros -- measured on the p = 1/2 forms at (20, 24) and
    (80, 88) before the launcher kept the hoisted row loads to shapes that fill their
    template.  The comparison run has its own zero tail: on a plain tensor the same read
    meets whatever the allocator left behind it, stale NaN included."""
    for HD in (256, 128):
        c = fwd_case(FWD_N, F, ldx, C, ldc, HD)
        for p in PS:
            tag = "F=%d ldx=%d HD=%d p=%g canary" % (F, ldx, HD, p)
            keep = keep_mask(FWD_N, HD, p, _row0(HD)) if p > 0 else None
            exp = fwd_expected(c, p, keep)
            Hp, Zp, _ = _run_fwd(c, p, _row0(HD), True, canary=True, tail=0.0)
            Hc, Zc, _ = _run_fwd(c, p, _row0(HD), True, canary=True)
            assert bool(torch.isfinite(Hc).all()), tag + ": H1 not finite"
            assert bool(torch.isfinite(Zc).all()), tag + ": Z2 not finite"
            _assert_same(Hc, exp[0], tag + " H1 against fp64")
            _assert_same(Hc, Hp, tag + " H1")
            _assert_same(Zc, Zp, tag + " Z2")
            _check_z2(c, p, Zc, exp, Hc, tag)


@pytest.mark.parametrize("p", [0.5, 0.0])
def test_dense_fwd_exact_several_tiles_per_wave(p):
    """Every wave of the persistent grid gets 2 or 3 tiles (p = 1/2: the hoisted next-tile
    prefetch, the form the benchmark times).  Rows periodic with period 1009, so the
    reference is computed once per period.  ALL rows: H1 = the reference under the mask
    decoded from the keep image the launch wrote, Z2 exact against the stored H1; that
    image equals the standalone draw everywhere and the Philox mirror on the first 64
    tiles, 64 tiles from tile 16 * CUs and the last 6."""
    cus = _cus()
    n = fwd_big_n(cus)
    c = fwd_big_case()
    HD, C, ldc, F, P = c["HD"], c["C"], c["ldc"], c["F"], FWD_BIG["period"]
    idx = torch.arange(n, device=DEV) % P
    AX = _dev(c["AX"], BF16)[idx]
    dinv = _dev(c["dinv"], F32)[idx]
    H1 = torch.full((n + 3, HD), SENT, dtype=BF16, device=DEV)
    Z2 = torch.full((n + 3, ldc), SENT, dtype=BF16, device=DEV)
    kimg = ops.keep_image(n, HD, DEV).fill_(0x5555) if p > 0 else None
    assert ops.dense_fwd(AX, _dev(c["W1"], F32), _dev(c["b1"], F32), _dev(c["W2"], F32), dinv, H1[:n], Z2[:n], F, p,
                         KEY, STEP, 0, kimg=kimg)
    torch.cuda.synchronize()
    assert bool((H1[n:] == SENT).all()) and bool((Z2[n:] == SENT).all()), "rows past n written"
    w2s = scale32(p) if p > 0 else 1.0
    Hexp = _dev(_bf16r(_mul32(c["Hu"], w2s)), BF16)[idx]               # every unit kept
    if p > 0:
        drawn = ops.draw_keep_image(ops.keep_image(n, HD, DEV), n, HD, p, KEY, STEP, 0)
        assert torch.equal(kimg, drawn), "keep image differs from the standalone draw"
        keep = decode_keep_image(kimg, n, HD)
        for lo, hi in big_mask_ranges(n, cus):
            _assert_same(keep[lo:hi].cpu(), ops.dropout_keep_mask(hi - lo, HD, p, KEY, STEP, lo),
                         "mask of rows %d..%d" % (lo, hi))
        Hexp = torch.where(keep, Hexp, torch.zeros_like(Hexp))
    _assert_same(H1[:n], Hexp, "H1")
    # layer 2 from the stored H1, fp64 on the device: exact in any order (fwd_expected
    # asserts sum|terms| / quantum < 2^24 for the period's rows with every unit kept, an
    # upper bound of any masked row's)
    fwd_expected(c, p, None)
    W2s = _dev(_bf16r(_mul32(c["W2"], w2s)), F64)
    z = dinv.double()[:, None] * ((H1[:n].double() / w2s) @ W2s)
    assert torch.equal(z.float().double(), z)
    Zexp = torch.zeros(n, ldc, dtype=BF16, device=DEV)
    Zexp[:, :C] = z.float().to(BF16)
    _assert_same(Z2[:n], Zexp, "Z2 against the stored H1")
    if p == 0:
        Zref = _dev(fwd_expected(c, p, None)[1], BF16)[idx]
        _assert_same(Z2[:n], Zref, "Z2")


# ------------------------------------------------------------------ dense_bwd
@pytest.mark.parametrize("n", BWD_NS)
def test_dense_bwd_exact_every_variant(n):
    """gcn_dense_bwd_kernel at both hidden widths, KC = 1 (tiny ldc, on the KC = 3
    template), 3 and 4, one row, one full tile and 3 tiles with a partial one, H1 holding
    +0, -0, subnormals and both signs: dP1 bit for bit, sentinel rows, and the same with
    dY2 inside a NaN-filled allocation."""
    for HD in (128, 256):
        for C, ldc in BWD_CLASSES:
            c = bwd_case(n, C, ldc, HD)
            for p in PS:
                tag = "n=%d HD=%d C=%d ldc=%d p=%g" % (n, HD, C, ldc, p)
                exp = bwd_expected(c, p)
                outs = []
                for canary in (False, True):
                    buf = torch.full((n + 3, HD), SENT, dtype=BF16, device=DEV)
                    assert ops.dense_bwd(_dev(c["dY2"], BF16, canary), _dev(c["W2"], F32), c["H1"].to(DEV), buf[:n], p)
                    torch.cuda.synchronize()
                    got = buf.cpu().double()
                    assert bool((got[n:] == SENT).all()), tag + ": rows past n written"
                    outs.append(got[:n])
                _assert_same(outs[0], exp, tag + " dP1")
                _assert_same(outs[1], exp, tag + " dP1 (dY2 in a NaN-filled allocation)")


# ------------------------------------------------------------------ fused_bwd
def _run_fused(c, p, row0, kimg, canary=False, **kw):
    n = c["n"]
    out = ops.fused_bwd(_dev(c["AX"], BF16, canary), _dev(c["dY2"], BF16, canary), _dev(c["W1"], F32),
                        _dev(c["b1"], F32), _dev(c["W2"], F32), n, c["F"], p, KEY, STEP, row0, kimg=kimg, **kw)
    torch.cuda.synchronize()
    return out


def _check_fused(c, p, keep, got, tag):
    gW1, gb1, gW2, gpart = got
    F, C = c["F"], c["C"]
    nb, width = gpart.shape[0], gpart.shape[2]
    assert width == fused_width(F)
    slabs, total = fused_expected(c, p, keep, nb)
    gp = gpart.cpu().double()
    kf = width - 64
    pad = torch.ones(width, dtype=torch.bool)
    pad[:F + 1] = False
    pad[kf:kf + C] = False
    _assert_same(gp[:, :, pad], torch.zeros_like(gp[:, :, pad]), tag + " slab padding columns")
    _assert_same(gp, slabs, tag + " slabs")
    got3 = (gW1.cpu().double(), gb1.cpu().double(), gW2.cpu().double())
    if total is not None:
        for g, r, name in zip(got3, total, ("gW1", "gb1", "gW2")):
            _assert_same(g, r, "%s %s" % (tag, name))
    else:
        # p = 0.3: each slab carries its own fp32 rounding of (sum * gs), so the sum over
        # the nb slabs depends on the order: every one of its nb - 1 adds rounds by at
        # most 2^-24 of a partial sum that is at most sum_b |slab_b|
        t, ta = slabs.sum(0), slabs.abs().sum(0)
        for g, r, a, name in zip(got3, (t[:, :F].t(), t[:, F], t[:, kf:kf + C]),
                                 (ta[:, :F].t(), ta[:, F], ta[:, kf:kf + C]), ("gW1", "gb1", "gW2")):
            assert bool(((g - r).abs() <= nb * 2.0 ** -24 * a).all()), "%s %s" % (tag, name)
    return gp


@pytest.mark.parametrize("n", FUSED_NS)
@pytest.mark.parametrize("ks", sorted(FUSED_F))
def test_fused_bwd_exact_every_variant(ks, n):
    """gcn_fused_bwd_kernel at every compiled (KS, KC, HD) with and without dropout, row
    pitches tight and padded to 128, one row to 3 tiles: every block slab (padding columns
    included) and gW1 / gb1 / gW2 bit for bit against the fp64 contraction of the bf16
    images of H1 and dP1; identical with the keep image taken from dense_fwd or drawn by
    fused_bwd itself, and with AX / dY2 inside NaN-filled allocations."""
    ran = set()
    for F in FUSED_F[ks]:
        assert (F + 1 + 15) // 16 == ks
        for ldx in sorted({tight(F + 1), 128}):
            for C, ldc in FUSED_CLASSES:
                for HD in (256, 128):
                    kc = (C + 15) // 16
                    sup = ops.fused_bwd_supported(F, HD, C)
                    assert sup == ((ks, kc, HD) in FUSED_TABLE), "fused_bwd_supported(%d, %d, %d)" % (F, HD, C)
                    if not sup:
                        continue
                    ran.add((ks, kc, HD))
                    c = fused_case(n, F, ldx, C, ldc, HD)
                    row0 = _row0(HD)
                    for p in PS:
                        tag = "n=%d F=%d ldx=%d C=%d ldc=%d HD=%d p=%g" % (n, F, ldx, C, ldc, HD, p)
                        keep = keep_mask(n, HD, p, row0) if p > 0 else None
                        kimg = None
                        if p > 0:
                            _, _, kimg = _run_fwd(c, p, row0, False)
                        gp = _check_fused(c, p, keep, _run_fused(c, p, row0, kimg), tag)
                        if p > 0:
                            own = _run_fused(c, p, row0, None)
                            _assert_same(own[3].cpu().double(), gp, tag + " slabs, keep image drawn by fused_bwd")
                        can = _run_fused(c, p, row0, kimg, canary=True)
                        _assert_same(can[3].cpu().double(), gp, tag + " slabs, inputs in NaN-filled allocations")
    assert ran == {v for v in FUSED_TABLE if v[0] == ks}


def test_fused_bwd_supported_is_the_launchers_table():
    """fused_bwd_supported is True exactly where fused_bwd launches and False exactly
    where the launcher returns -1 (no compiled variant), on a grid of (K, HD, C)."""
    n = 1
    for F in (1, 15, 16, 47, 48, 62, 63, 64, 79, 80, 95, 96, 111, 112, 126, 127, 128):
        for HD in (64, 128, 256, 512):
            for C in (1, 16, 17, 32, 33, 48, 49, 64):
                ldx, ldc = tight(F + 1), tight(C)
                AX = torch.zeros(n, ldx, dtype=BF16, device=DEV)
                dY2 = torch.zeros(n, ldc, dtype=BF16, device=DEV)
                W1, b1 = torch.zeros(F, HD, device=DEV), torch.zeros(HD, device=DEV)
                W2 = torch.zeros(HD, C, device=DEV)
                sup = ops.fused_bwd_supported(F, HD, C)
                assert sup == (((F + 16) // 16, (C + 15) // 16, HD) in FUSED_TABLE), (F, HD, C)
                try:
                    ops.fused_bwd(AX, dY2, W1, b1, W2, n, F, 0.0, KEY, STEP)
                    launched = True
                except RuntimeError as e:
                    assert "(-1)" in str(e), "F=%d HD=%d C=%d: %s" % (F, HD, C, e)
                    launched = False
                assert launched == sup, "F=%d HD=%d C=%d: supported %r, launched %r" % (F, HD, C, sup, launched)
    torch.cuda.synchronize()


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_fused_bwd_exact_three_tiles_per_block(p):
    """Every block gets 3 or 4 tiles (the staging double buffer behind the register
    prefetch of the tile after next), the last tile partial: slabs and gradients bit for
    bit against fp64, and the ``grads=`` path (slab_sum into a flat buffer between
    sentinels) bit for bit equal to the ``.sum(0)`` path."""
    cus = _cus()
    n = fused_big_n(cus)
    F, ldx, C, ldc, HD = 100, 104, 47, 48, 256
    c = fused_case(n, F, ldx, C, ldc, HD)
    keep = kimg = None
    if p > 0:
        # the mask: the standalone draw, decoded (checked against the Philox mirror in
        # test_keep_image_*); the mirror itself takes seconds at this many rows
        kimg = ops.draw_keep_image(ops.keep_image(n, HD, DEV), n, HD, p, KEY, STEP, 0)
        keep = decode_keep_image(kimg, n, HD).cpu()
    got = _run_fused(c, p, 0, kimg)
    assert got[3].shape[0] == cus
    _check_fused(c, p, keep, got, "n=%d p=%g" % (n, p))
    size = F * HD + HD + HD * C
    flat = torch.full((size + 16,), SENT, dtype=F32, device=DEV)
    _run_fused(c, p, 0, kimg, grads=flat[8:8 + size])
    flat = flat.cpu()
    assert bool((flat[:8] == SENT).all()) and bool((flat[8 + size:] == SENT).all()), "grads: written outside"
    g = flat[8:8 + size]
    _assert_same(g[:F * HD].view(F, HD), got[0].cpu(), "grads= gW1")
    _assert_same(g[F * HD:F * HD + HD], got[1].cpu(), "grads= gb1")
    _assert_same(g[F * HD + HD:].view(HD, C), got[2].cpu(), "grads= gW2")


# ------------------------------------------------------------------ keep image
@pytest.mark.parametrize("p", [0.5, 0.3])
@pytest.mark.parametrize("HD,n,row0", [(128, 1, 77), (128, 33, 4096), (256, 1, 5), (256, 33, 64)])
def test_keep_image_matches_mask_and_forward(p, HD, n, row0):
    """The keep image drawn on its own decodes to the Philox mirror's mask, and the image
    dense_fwd writes (bit mode: from its own draw; byte mode: the side launch) equals it
    bit for bit -- one row, one row past a tile, row0 != 0, both hidden widths."""
    drawn = ops.draw_keep_image(ops.keep_image(n, HD, DEV).fill_(0x5555), n, HD, p, KEY, STEP, row0)
    _assert_same(decode_keep_image(drawn, n, HD).cpu(), ops.dropout_keep_mask(n, HD, p, KEY, STEP, row0), "mask")
    c = fwd_case(n, 100, 104, 47, 48, HD)
    _, _, kimg = _run_fwd(c, p, row0, False)
    assert torch.equal(kimg, drawn), "forward-written image differs from the drawn one"
