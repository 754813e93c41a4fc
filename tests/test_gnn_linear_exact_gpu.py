"""Exact oracle tests of the generic linear kernels (gnn_linear.hip): lin_ws, lin_fwd,
lin_fwd_kc, lin_gemm, lin_bwd_data, lin_bwd_weight2 and the two reduce kernels.

Every reference is computed here, in fp64 -- never through the CPU branches of
``gnn/linear.py`` (which round ``bf16(g * mscale)`` before the data-backward product and so
are a different function).  X, dY and Ym hold small integers (Ym also signed zeros and
subnormal bit patterns), W and b multiples of 1/4 in [-1, 1], row scales values from
{0.5, 1, 2}.  Every MFMA product is then exact and every partial sum a multiple of a known
quantum; each builder asserts on its own data that sum|terms| / quantum < 2^24, so the fp32
accumulation is exact in any order, split-K included.  Outputs are single correct roundings
of exactly known numbers and are compared with ``torch.equal``.  The only tolerance is the
forward at p = 0.3 (``bf16(W / 0.7)`` has arbitrary low bits), derived at its assertion.

Which kernel a case reaches is asked of the launcher's own selection function
(``gnn_lin_*_variant``) and asserted by every test; one test asserts that the cases reach
the launchers' whole table, another that the query says "none" exactly where a launch
fails.

Not covered, and why: the v1 ``lin_bwd_weight_kernel`` is selected only when the staged row
ids of a gathered chunk overflow LDS beside the images (rows per chunk * 4 B > ~100 KB:
millions of rows), and the fall-back of the weight-stationary form to the slab kernel only
past 64 tiles per block (row ids / row scales staged in LDS; 64 * 32 * CUs * occupancy rows).
Neither is reachable at test sizes and no hook forces them.  ``lin_fwd_kc_kernel<2, *>`` was
never launched (two feature groups always take lin_gemm) and is no longer instantiated.

The case builders and references (everything above the ``GPU runs`` line) make no GPU
call: tests/test_gnn_linear_exact_cpu.py runs their preconditions without a device.
"""
import functools

import numpy as np
import pytest
import torch

from cgnn_amd.gnn import ops
from test_gnn_dense_exact_gpu import (_bf16r, _ints, _mul32, _pow2, _quarters, assert_exact_sums, relu_bf16,  # noqa: F401
                                      scale32, tight)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 7.0            # sentinel of rows / buffers a kernel must not write
PAD = 5.0             # finite junk in the padding columns of a row
NAN = float("nan")
BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
KEY, STEP, ROW0 = (31, 41), 5, 64
TILE = 32
WS_RING = 3           # register ring depth of lin_ws
WS, SLAB, KC, GEMM, WGT2, WGT1 = 1, 2, 3, 4, 5, 6
# bf16 bit patterns of Ym: +0, -0, the smallest positive and negative subnormals, positive
# and negative normals; the unit is kept only for a set magnitude with a clear sign bit
YM_BITS = [0x0000, 0x8000, 0x0001, 0x8001, 0x3FC0, 0xC000, 0x4248, 0xBE80, 0x3C00, 0x3F80]


def decode(code):
    """(family, a, b) of a gnn_lin_*_variant code, or the negative launcher code."""
    return code if code < 0 else (code // 1000000, code // 1000 % 1000, code % 1000)


def _f16r(x):
    """Round-to-nearest-even fp16 image of an fp32-exact fp64 tensor, as fp64."""
    assert torch.equal(x.float().double(), x), "reference value is not fp32-exact"
    return x.float().to(F16).double()


def _rows(rng, rows, K, ld, amp, fill):
    """[rows][ld] fp64: integers in [-amp, amp] in the first K columns, ``fill`` after."""
    x = torch.full((rows, ld), fill, dtype=F64)
    x[:, :K] = _ints(rng, -amp, amp, (rows, K))
    return x


def _ym(rng, n, N, ld, fill):
    """Stored outputs [n][ld] (bf16) drawn from YM_BITS, ``fill`` in the padding columns."""
    y = torch.full((n, ld), fill, dtype=BF16)
    bits = np.asarray(YM_BITS, dtype=np.uint16)[rng.integers(0, len(YM_BITS), (n, N))]
    y[:, :N] = torch.from_numpy(bits.view(np.int16).copy()).view(BF16)
    return y


def alive(Ym, N):
    """[Ym > 0] by the bit pattern: sign clear and magnitude set (subnormals included)."""
    return Ym[:, :N].contiguous().view(torch.int16) > 0


# ------------------------------------------------------------------ forward: cases and reference
# name: (K1, K2, N, ldy, fp16, variant (family, a, b), options).  b of a slab variant is
# 10 * waves per block + staged stores.  Options: pad = extra row pitch of x1, tail =
# (nsplit, tk), idx = gathered x1, drop = dropout allowed (bf16, no kc / gemm).
def _f(K1, K2, N, ldy, fp16, var, **kw):
    return dict(K1=K1, K2=K2, N=N, ldy=ldy, fp16=fp16, var=var, **kw)


FWD = {}
for _et, _h in ((0, "bf"), (1, "h")):
    FWD.update({
        # weight-stationary: six (KS, NW)
        "ws_4_2_" + _h: _f(64, 0, 40, 40, _et, (WS, 4, 2)),
        "ws_4_4_" + _h: _f(24, 24, 96, 96, _et, (WS, 4, 4), pad=24),
        "ws_4_8_" + _h: _f(64, 0, 136, 136, _et, (WS, 4, 8)),
        "ws_8_4_" + _h: _f(128, 0, 33, 40, _et, (WS, 8, 4), idx=True),
        "ws_8_8_" + _h: _f(104, 0, 200, 200, _et, (WS, 8, 8), pad=24),
        "ws_16_8_" + _h: _f(128, 128, 33, 48, _et, (WS, 16, 8)),
        # slab, KS 4 / 8 / 16 through a ragged K (the masking loader) and through N > 256
        "slab_4_rag_" + _h: _f(47, 0, 40, 40, _et, (SLAB, 4, 161)),
        "slab_4_wide_" + _h: _f(64, 0, 264, 264, _et, (SLAB, 4, 161)),
        "slab_8_rag_" + _h: _f(100, 0, 47, 48, _et, (SLAB, 8, 81), pad=24),
        "slab_8_wide_" + _h: _f(128, 0, 264, 264, _et, (SLAB, 8, 81), idx=True),
        "slab_16_rag_" + _h: _f(250, 0, 40, 40, _et, (SLAB, 16, 81)),
        "slab_16_wide_" + _h: _f(256, 0, 288, 288, _et, (SLAB, 16, 81)),
        "slab_24_rag_" + _h: _f(300, 0, 40, 40, _et, (SLAB, 24, 81)),
        "slab_24_al_" + _h: _f(384, 0, 64, 64, _et, (SLAB, 24, 81)),
        "slab_32_rag_" + _h: _f(500, 0, 47, 48, _et, (SLAB, 32, 81), pad=24),
        # two column slabs (128 + 32): the concatenation keeps it off lin_gemm
        "slab_32_two_" + _h: _f(256, 256, 160, 160, _et, (SLAB, 32, 81)),
        # weights too wide for LDS: one feature group (lin_fwd_kc<1>), two (lin_gemm) with K
        # no multiple of 8, a multiple of 8 but not of 64, and of 64
        "kc_" + _h: _f(520, 0, 100, 104, _et, (KC, 1, 0)),
        "gemm_odd_" + _h: _f(301, 0, 200, 200, _et, (GEMM, 0, 0)),
        "gemm_8_" + _h: _f(520, 0, 136, 136, _et, (GEMM, 0, 0), pad=24),
        "gemm_64_" + _h: _f(320, 0, 250, 256, _et, (GEMM, 0, 0)),
    })
FWD.update({
    # the un-staged store path: only KS = 4 with >= 832 output columns
    "slab_4_unstaged_bf": _f(40, 0, 840, 840, 0, (SLAB, 4, 160)),
    # two slabs wider than 256 columns (the weight image must hold 2 x 512 rows)
    "slab_8_two_wide_bf": _f(128, 0, 520, 520, 0, (SLAB, 8, 81)),
    # fp32 tail planes (GAT's folded scores): nsplit % 8 == 4 and ldy > nsplit
    "tail_4_bf": _f(64, 0, 44, 40, 0, (SLAB, 4, 160), tail=(36, 4)),
    "tail_8_bf": _f(128, 0, 136, 136, 0, (SLAB, 8, 80), tail=(128, 4)),
    "tail_16_bf": _f(200, 0, 72, 64, 0, (SLAB, 16, 80), tail=(64, 1), idx=True),
    # fp16 alone has KS = 40 and 48
    "slab_40_h": _f(602, 0, 64, 64, 1, (SLAB, 40, 81)),
    "slab_48_h": _f(768, 0, 40, 40, 1, (SLAB, 48, 81)),
})
# every launchable template of gnn_launch_lin_fwd, as (family, a, b without the waves / staged
# digit of a slab, element type)
FWD_TABLE = ({(WS, ks, nw, et) for ks, nw in ((4, 2), (4, 4), (4, 8), (8, 4), (8, 8), (16, 8)) for et in (0, 1)}
             | {(SLAB, ks, 0, 0) for ks in (4, 8, 16, 24, 32)} | {(SLAB, ks, 0, 1) for ks in (4, 8, 16, 24, 32, 40, 48)}
             | {(KC, 1, 0, et) for et in (0, 1)} | {(GEMM, 0, 0, et) for et in (0, 1)})
FWD_N = 77            # 3 tiles, the last one partial
ROW_COUNTS = (1, 31, 32, 33, 65)
PS_EXACT = (0.5, 0.75)    # bit mode (s = 2) and byte mode with s = 4 exactly


def table_key(var, et=0):
    return (var[0], var[1], 0 if var[0] == SLAB else var[2], et)


@functools.lru_cache(maxsize=None)
def fwd_case(name, n=FWD_N, fill=PAD, posbias=False):
    """Inputs of one forward case.  ``posbias``: a bias that makes every pre-activation
    positive (so that with dropout an output is zero exactly where the unit is dropped)."""
    s = FWD[name]
    K1, K2, N, ldy = s["K1"], s["K2"], s["N"], s["ldy"]
    rng = np.random.default_rng(sum(map(ord, name)) * 131 + n)
    ld1, ld2 = tight(K1) + s.get("pad", 0), tight(K2)
    table = 2 * n + 3 if s.get("idx") else n
    X1 = _rows(rng, table, K1, ld1, 2 if K1 + K2 > 256 else 3, fill)
    X2 = _rows(rng, n, K2, ld2, 3, fill) if K2 else None
    idx = None
    if s.get("idx"):                                  # repeats, out of order, table larger than n
        idx = torch.from_numpy(rng.integers(0, table, n).astype(np.int32))
        idx[n // 2] = idx[0]
    W, b = _quarters(rng, (K1 + K2, N)), _quarters(rng, (N,))
    rs = _pow2(rng, n)
    X = X1[:n, :K1] if idx is None else X1[idx.long(), :K1]
    if K2:
        X = torch.cat([X, X2[:, :K2]], 1)
    if posbias:
        b = b + torch.ceil((X.abs() @ W.abs()).max(0).values) + 1
    return dict(s, name=name, n=n, ld1=ld1, ld2=ld2, X1=X1, X2=X2, idx=idx, W=W, b=b, rs=rs, X=X)


def fwd_expected(c, p=0.0, keep=None, relu=True):
    """(y16 [n][ldy], tail planes | None, pre, absum): the 16-bit output
    mask * max(0, r16((X W' + b') * rs)) with W' = r16(fp32(W) * s), b' = fp32(b) * s,
    s = 1.f / (1.f - p); the fp32 tail planes hold the same value without the rounding.
    Exact for p in {0, 1/2, 3/4} (asserted); ``pre`` / ``absum`` (the scaled sum and the sum
    of |terms|) feed the derived bound at p = 0.3."""
    r16 = _f16r if c["fp16"] else _bf16r
    s = scale32(p) if p > 0 else 1.0
    Ws, bs = r16(_mul32(c["W"], s)), _mul32(c["b"], s)
    pre = c["X"] @ Ws + bs
    absum = c["X"].abs() @ Ws.abs() + bs.abs()
    if p in (0.0, 0.5, 0.75):
        assert_exact_sums(absum, 0.25, "%s: X W' + b'" % c["name"])
    v = pre * c["rs"][:, None]                        # fp32 multiply by a power of two: exact
    n, N, ldy = c["n"], c["N"], c["ldy"]
    if p not in (0.0, 0.5, 0.75):
        return None, None, v, absum * c["rs"][:, None]
    y = r16(v)
    if relu:
        y = torch.where(y > 0, y, torch.zeros_like(y))
        v = torch.where(v > 0, v, torch.zeros_like(v))
    if keep is not None:
        y, v = y * keep, v * keep
    nsplit = c["tail"][0] if c.get("tail") else N
    y16 = torch.zeros(n, ldy, dtype=F64)
    y16[:, :nsplit] = y[:, :nsplit]
    planes = None
    if c.get("tail"):
        tk = c["tail"][1]
        planes = v[:, nsplit:].reshape(n, (N - nsplit) // tk, tk).transpose(0, 1).contiguous()
    return y16, planes, v, absum


@functools.lru_cache(maxsize=None)
def keep_mask(n, N, p, row0=ROW0, step=STEP):
    return ops.dropout_keep_mask(n, N, p, KEY, step, row0)


def ws_rows(grid, nt):
    """Rows that give blocks 0 and 1 of a ``grid``-block lin_ws launch ``nt`` tiles and the
    others nt - 1 (one tile more than a whole number of rounds plus one), last tile partial."""
    return TILE * (grid * (nt - 1) + 2) - 11 if nt > 1 else TILE * 2 - 11


WS_NTS = (1, 2, 3, 4, 7)      # every residue mod the ring depth, 3 taking the final store
PERIOD = 1009                 # prime: no alignment with tiles, waves or blocks


# ------------------------------------------------------------------ data backward: cases and reference
# name: (N, K1, K2, variant, options): f32 = fp32 dX1, pad = extra pitch of dY / Ym / dX
def _d(N, K1, K2, var, **kw):
    return dict(N=N, K1=K1, K2=K2, var=var, **kw)


BWD = {
    "ws_4_2": _d(64, 40, 0, (WS, 4, 2)),
    "ws_4_4": _d(40, 48, 52, (WS, 4, 4), pad=24),
    "ws_4_8": _d(64, 200, 0, (WS, 4, 8)),
    "ws_8_4": _d(128, 64, 64, (WS, 8, 4)),
    "ws_8_8": _d(104, 256, 0, (WS, 8, 8), pad=24),
    "ws_16_8": _d(256, 47, 0, (WS, 16, 8)),
    # slab: the ragged branch with the straddling chunk in the upper (N = 47, 250) and the
    # lower (N = 100, 36) half; the aligned branch through fp32 dX1 or K > 256; only KN = 16
    # runs on 8-wave blocks and prefetches
    "slab_4_rag": _d(47, 64, 0, (SLAB, 4, 161)),
    "slab_4_rag_lo": _d(36, 40, 24, (SLAB, 4, 161), pad=24),
    "slab_4_f32": _d(64, 40, 0, (SLAB, 4, 160), f32=True),
    "slab_4_unstaged": _d(40, 870, 0, (SLAB, 4, 160)),
    "slab_4_two_wide": _d(40, 1000, 0, (SLAB, 4, 160)),       # two slabs of 992 rows of W
    "slab_8_rag": _d(100, 256, 0, (SLAB, 8, 161)),
    "slab_8_wide": _d(128, 264, 0, (SLAB, 8, 161)),
    "slab_16_rag": _d(250, 40, 0, (SLAB, 16, 81)),
    "slab_16_f32": _d(256, 64, 64, (SLAB, 16, 80), f32=True),
    "slab_16_wide": _d(256, 264, 0, (SLAB, 16, 81), pad=24),
    "slab_24_rag": _d(300, 64, 0, (SLAB, 24, 81)),
    "slab_24_al": _d(384, 128, 128, (SLAB, 24, 81)),
    "slab_32_rag": _d(500, 40, 0, (SLAB, 32, 81)),
    "slab_32_al": _d(512, 64, 0, (SLAB, 32, 80), f32=True),
}
BWD_TABLE = ({(WS, ks, nw, 0) for ks, nw in ((4, 2), (4, 4), (4, 8), (8, 4), (8, 8), (16, 8))}
             | {(SLAB, kn, 0, 0) for kn in (4, 8, 16, 24, 32)})
MSCALES = (1.0, 2.0, scale32(0.3))


@functools.lru_cache(maxsize=None)
def bwd_case(name, n=FWD_N, fill=PAD):
    s = BWD[name]
    N, K1, K2 = s["N"], s["K1"], s["K2"]
    rng = np.random.default_rng(sum(map(ord, name)) * 137 + n)
    ldd = tight(N) + s.get("pad", 0)
    dY = _rows(rng, n, N, ldd, 2 if N > 256 else 3, fill)
    Ym = _ym(rng, n, N, ldd, fill)
    W = _quarters(rng, (K1 + K2, N))
    rs = _pow2(rng, n)
    g = dY[:, :N] * alive(Ym, N)
    assert_exact_sums(dY[:, :N].abs() @ W.abs().t(), 0.25, name + ": dY W^T")
    return dict(s, name=name, n=n, ldd=ldd, dY=dY, Ym=Ym, W=W, rs=rs, acc=g @ W.t(), acc_nomask=dY[:, :N] @ W.t())


def bwd_expected(c, mscale, mask=True, rscale=True, f32=False):
    """dX = bf16(fp32(sum_c W[k][c] g[c]) * fp32(rs * mscale)): ONE fp32 multiply, then one
    bf16 rounding (rs a power of two: the product rs * mscale and the scaling by rs are
    exact, so the fp32 multiply by mscale is the only rounding before the bf16 one)."""
    t = _mul32(c["acc"] if mask else c["acc_nomask"], mscale)
    if not f32:
        t = _bf16r(t)
    return t * c["rs"][:, None] if rscale else t


# ------------------------------------------------------------------ weight backward: cases and reference
# name: (K1, K2, N, (KT, NB), k-tiles): every (KT, NB) of the launcher's list, k-tile counts
# below the template's KT (3 on 4, 6 and 7 on 8, 10 on 12, 13 on 16) included
def _w(K1, K2, N, ktnb, **kw):
    return dict(K1=K1, K2=K2, N=N, ktnb=ktnb, **kw)


WGT = {
    "2_2": _w(64, 0, 40, (2, 2)), "2_4": _w(40, 0, 100, (2, 4)), "2_8": _w(32, 32, 256, (2, 8)),
    "4_2": _w(96, 0, 47, (4, 2)), "4_4": _w(128, 0, 128, (4, 4)), "4_8": _w(100, 0, 200, (4, 8), pad=24),
    "5_2": _w(160, 0, 64, (5, 2)), "5_4": _w(136, 0, 100, (5, 4)),
    "8_2": _w(192, 0, 33, (8, 2)), "8_4": _w(104, 104, 128, (8, 4), idx=True), "8_8": _w(256, 0, 256, (8, 8)),
    "9_2": _w(288, 0, 40, (9, 2)), "9_4": _w(264, 0, 136, (9, 4)),
    "12_2": _w(320, 0, 64, (12, 2)), "12_4": _w(384, 0, 100, (12, 4), pad=24),
    "16_2": _w(416, 0, 47, (16, 2)), "16_4": _w(256, 256, 256, (16, 4)),
    "17_2": _w(544, 0, 47, (17, 2)),
}
WGT_TABLE = {(WGT2,) + s["ktnb"] + (ym,) for s in WGT.values() for ym in (0, 1)}
WGT_LIST = [(2, 2), (2, 4), (2, 8), (4, 2), (4, 4), (4, 8), (5, 2), (5, 4), (8, 2), (8, 4), (8, 8), (9, 2), (9, 4),
            (12, 2), (12, 4), (16, 2), (16, 4), (17, 2)]
WGT_N = 300           # 10 tiles, the last one partial: 10 chunks of one tile


@functools.lru_cache(maxsize=None)
def wgt_case(name, n=WGT_N, fill=PAD, amp=3, period=None):
    s = WGT[name]
    K1, K2, N = s["K1"], s["K2"], s["N"]
    rows = period or n
    rng = np.random.default_rng(sum(map(ord, name)) * 139 + rows)
    ld1, ld2, ldd = tight(K1) + s.get("pad", 0), tight(K2), tight(N) + s.get("pad", 0)
    table = 2 * rows + 3 if s.get("idx") else rows
    X1 = _rows(rng, table, K1, ld1, amp, fill)
    X2 = _rows(rng, rows, K2, ld2, amp, fill) if K2 else None
    idx = None
    if s.get("idx"):
        idx = torch.from_numpy(rng.integers(0, table, rows).astype(np.int32))
        idx[rows // 2] = idx[0]
    dY = _rows(rng, rows, N, ldd, amp, fill)
    Ym = _ym(rng, rows, N, ldd, fill)
    X = X1[:rows, :K1] if idx is None else X1[idx.long(), :K1]
    if K2:
        X = torch.cat([X, X2[:, :K2]], 1)
    return dict(s, name=name, n=n, rows=rows, ld1=ld1, ld2=ld2, ldd=ldd, X1=X1, X2=X2, idx=idx, dY=dY, Ym=Ym, X=X)


def wgt_expected(c, mscale, mask, reps=1, last=None):
    """(dW, db): g = bf16(fp32(dY) * mscale) on the kept units (one rounding, as mask8),
    dW = X^T g and db = sum g as exact sums.  The case's rows ``reps`` times over plus its
    first ``last`` rows (the periodic large-n cases).  The quantum of a term is 1 for a
    power-of-two mscale and 2^-7 at mscale = 1/(1 - 0.3) (|g| < 8 holds 8 significant bits
    down to 2^-7 for |dY| >= 1), asserted on the data."""
    N = c["N"]
    g = _mul32(c["dY"][:, :N], mscale)
    if mask or mscale != 1.0:
        g = _bf16r(g)
    if mask:
        g = g * alive(c["Ym"], N)
    quantum = 1.0 if mscale in (1.0, 2.0) else 2.0 ** -7
    assert torch.equal(torch.round(g / quantum) * quantum, g), "%s: g is no multiple of the quantum" % c["name"]
    X = c["X"]
    dW, db = X.t() @ g, g.sum(0)
    aW, ab = X.abs().t() @ g.abs(), g.abs().sum(0)
    if last is not None:
        dW, db = reps * dW + X[:last].t() @ g[:last], reps * db + g[:last].sum(0)
        aW, ab = reps * aW + X[:last].abs().t() @ g[:last].abs(), reps * ab + g[:last].abs().sum(0)
    assert_exact_sums(aW, quantum, c["name"] + ": dW")
    assert_exact_sums(ab, quantum, c["name"] + ": db")
    return dW, db


def wgt_rows(cus, tpc, slabs=1):
    """Rows that give the chunks of a weight gradient ``tpc`` tiles each (the last chunk
    fewer), the last tile ragged."""
    chunks = max(1, cus // slabs)
    return TILE * (chunks * tpc - (1 if tpc > 1 else 0)) - 13


# ================================================================== GPU runs
def _hip():
    from cgnn_amd import native
    return native.hip()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _same(got, exp, what):
    if got.shape != exp.shape or not torch.equal(got, exp):
        assert got.shape == exp.shape, "%s: shape %r, expected %r" % (what, tuple(got.shape), tuple(exp.shape))
        bad = (got != exp).nonzero()
        i = tuple(int(x) for x in bad[0])
        raise AssertionError("%s: %d elements differ, first at %r: got %r, expected %r"
                             % (what, bad.shape[0], i, float(got[i]), float(exp[i])))


def _dev(x, dtype=None, canary=False):
    """x on the device; ``canary``: in the middle of a NaN-filled allocation (a read before
    or past the tensor meets NaN, in memory the test owns)."""
    if x is None:
        return None
    x = x.to(dtype) if dtype is not None else x
    if not canary or not x.dtype.is_floating_point:
        return x.to(DEV)
    guard = 4 if x.dim() == 2 else 64
    big = torch.full((x.shape[0] + 2 * guard,) + tuple(x.shape[1:]), NAN, dtype=x.dtype, device=DEV)
    big[guard:guard + x.shape[0]] = x.to(DEV)
    return big[guard:guard + x.shape[0]]


class _Out:
    """A sentinel-framed output: ``t`` ([n][ld]) lies inside a flat sentinel-filled buffer with
    3 rows after it and 8 elements on either side."""

    def __init__(self, n, ld, dtype):
        self.n, self.ld = n, ld
        self.flat = torch.full(((n + 3) * ld + 16,), SENT, dtype=dtype, device=DEV)
        self.all = self.flat[8:8 + (n + 3) * ld].view(n + 3, ld)
        self.t = self.all[:n]

    def get(self, what):
        f = self.flat.cpu().double()
        body = f[8:8 + (self.n + 3) * self.ld].view(self.n + 3, self.ld)
        assert bool((body[self.n:] == SENT).all()), what + ": rows past n written"
        assert bool((f[:8] == SENT).all()) and bool((f[-8:] == SENT).all()), what + ": written outside the buffer"
        return body[:self.n]

    def untouched(self):
        return bool((self.flat == SENT).all())


def _fwd_query(c, n, p=0.0, rscale=True):
    t = c.get("tail")
    return decode(_hip().gnn_lin_fwd_variant(c["ld1"], c["K1"], int(c["K2"] > 0), c["ld2"], c["K2"], c["N"], c["ldy"], n,
                                             p, int(c["idx"] is not None), int(rscale), int(t is not None),
                                             t[0] if t else 0, t[1] if t else 1, c["fp16"]))


def _run_fwd(c, p=0.0, canary=False, relu=True, rscale=True, step=STEP, check=True):
    """One lin_fwd into sentinel-framed buffers: (y16 [n][ldy] fp64, planes | None)."""
    from cgnn_amd.gnn import linear
    n, dt = c["n"], (F16 if c["fp16"] else BF16)
    if check:
        assert _fwd_query(c, n, p, rscale) == c["var"], "%s: variant %r" % (c["name"], _fwd_query(c, n, p, rscale))
    out = _Out(n, c["ldy"], dt)
    t, planes = c.get("tail"), None
    if t:
        planes = _Out((c["N"] - t[0]) // t[1] * n, t[1], F32)
    linear.lin_fwd(_dev(c["X1"], dt, canary), _dev(c["W"], F32, canary), _dev(c["b"], F32, canary),
                   x2=_dev(c["X2"], dt, canary), K1=c["K1"], K2=c["K2"] or None, relu=relu, p=p, key=KEY, step=step,
                   row0=ROW0, rscale=_dev(c["rs"], F32, canary) if rscale else None, out=out.t,
                   idx1=_dev(c["idx"]), n=n, tail=planes.t if t else None, nsplit=t[0] if t else None,
                   tk=t[1] if t else 1)
    torch.cuda.synchronize()
    y = out.get(c["name"] + " out")
    pl = planes.get(c["name"] + " tail").view(-1, n, t[1]) if t else None
    return y, pl


def _check_fwd(c, p, got, what, relu=True):
    keep = keep_mask(c["n"], c["N"], p).double() if p > 0 else None
    y16, planes, _, _ = fwd_expected(c, p, keep, relu)
    _same(got[0][:, c["N"] if not c.get("tail") else c["tail"][0]:],
          torch.zeros_like(got[0][:, c["N"] if not c.get("tail") else c["tail"][0]:]), what + " padding columns")
    _same(got[0], y16, what + " out")
    if planes is not None:
        _same(got[1], planes, what + " tail planes")


@pytest.mark.parametrize("name", sorted(FWD))
def test_lin_fwd_exact_every_template(name):
    """Every launchable forward template, 3 tiles with a partial last one, padding columns
    holding finite junk: out (and the fp32 tail planes) bit for bit against fp64 with and
    without ReLU / row scale, the same with every operand inside a NaN-filled allocation
    and NaN in the padding columns, columns N..ldy exactly zero, sentinel rows untouched,
    a repeated call bitwise equal."""
    c = fwd_case(name)
    got = _run_fwd(c)
    _check_fwd(c, 0.0, got, name)
    again = _run_fwd(c)
    _same(again[0], got[0], name + " repeated call")
    _check_fwd(c, 0.0, _run_fwd(fwd_case(name, fill=NAN), canary=True), name + " (NaN padding, canary)")
    plain = dict(c, rs=torch.ones_like(c["rs"]))
    _check_fwd(plain, 0.0, _run_fwd(c, relu=False, rscale=False, check=False), name + " (no relu, no row scale)",
               relu=False)


@pytest.mark.parametrize("name", ["ws_4_2_bf", "ws_16_8_h", "slab_8_rag_bf", "slab_24_rag_h", "kc_bf", "gemm_odd_h",
                                  "tail_4_bf"])
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_lin_fwd_exact_row_counts(name, n):
    """1, 31, 32, 33 and 65 rows on each forward family."""
    c = fwd_case(name, n=n)
    _check_fwd(c, 0.0, _run_fwd(c), "%s n=%d" % (name, n))


DROP_CASES = [k for k, s in sorted(FWD.items()) if not s["fp16"] and s["var"][0] in (WS, SLAB)]


@pytest.mark.parametrize("name", DROP_CASES)
def test_lin_fwd_exact_with_dropout(name):
    """Bit mode (p = 1/2) and byte mode with an exact scale (p = 3/4, s = 4) on every bf16
    weight-stationary and slab template: bit for bit, and -- the bias making every
    pre-activation positive -- zero exactly where ops.dropout_keep_mask drops."""
    c = fwd_case(name, posbias=True)
    for p in PS_EXACT:
        got = _run_fwd(c, p)
        _check_fwd(c, p, got, "%s p=%g" % (name, p))
        nsplit = c["tail"][0] if c.get("tail") else c["N"]
        keep = keep_mask(c["n"], c["N"], p)
        _same(got[0][:, :nsplit] != 0, keep[:, :nsplit], "%s p=%g zero pattern" % (name, p))
        if c.get("tail"):
            flat = got[1].transpose(0, 1).reshape(c["n"], -1)
            _same(flat != 0, keep[:, nsplit:], "%s p=%g zero pattern of the tail" % (name, p))


@pytest.mark.parametrize("name", ["ws_8_8_bf", "slab_16_rag_bf", "slab_32_two_bf", "tail_8_bf"])
def test_lin_fwd_inexact_dropout_scale(name):
    """p = 0.3: s = 1/0.7 is inexact, W' = bf16(W s) has arbitrary low bits.  The zero
    pattern equals ops.dropout_keep_mask exactly (every pre-activation positive) and the
    kept values obey the bound derived below."""
    p = 0.3
    c = fwd_case(name, posbias=True)
    got = _run_fwd(c, p)
    _, _, v, absum = fwd_expected(c, p)
    keep = keep_mask(c["n"], c["N"], p)
    nsplit = c["tail"][0] if c.get("tail") else c["N"]
    _same(got[0][:, :nsplit] != 0, keep[:, :nsplit], name + " zero pattern")
    _same(got[0][:, nsplit:], torch.zeros_like(got[0][:, nsplit:]), name + " padding columns")
    # v = (X W' + b') * rs with the SAME rounded W' and b' the kernel multiplies, in fp64.
    # The kernel adds the K + 1 exact products in fp32 in some order: each add rounds by at
    # most 2^-24 of a partial sum that is at most sum|terms| (= absum, times rs: exact), so
    # |acc - v| <= (K + 1) 2^-24 absum; the bf16 rounding adds at most 2^-8 |acc|
    # (half an ulp of 8 significant bits); the fp32 tail planes carry the first term only.
    K = c["K1"] + c["K2"]
    acc_err = (K + 1) * 2.0 ** -24 * absum
    bound = acc_err + 2.0 ** -8 * (v.abs() + acc_err)
    err = (got[0][:, :nsplit] - v[:, :nsplit] * keep[:, :nsplit]).abs()
    assert bool((err <= bound[:, :nsplit]).all()), "%s: max excess %g" % (name, float((err - bound[:, :nsplit]).max()))
    if c.get("tail"):
        flat = got[1].transpose(0, 1).reshape(c["n"], -1)
        _same(flat != 0, keep[:, nsplit:], name + " zero pattern of the tail")
        err = (flat - v[:, nsplit:] * keep[:, nsplit:]).abs()
        assert bool((err <= acc_err[:, nsplit:]).all()), name + " tail planes"


def test_lin_fwd_tail_zeroes_the_padding_of_out():
    """With an fp32 tail the 16-bit columns [nsplit, ldy) of ``out`` are written as zeros
    (nsplit % 8 == 4, and ldy > nsplit by a whole chunk): consumers read whole pitches."""
    for name in ("tail_4_bf", "tail_8_bf"):
        c = fwd_case(name)
        y, _ = _run_fwd(c)
        nsplit = c["tail"][0]
        assert c["ldy"] > nsplit
        _same(y[:, nsplit:], torch.zeros_like(y[:, nsplit:]), name + " out[:, nsplit:ldy]")


@pytest.mark.parametrize("name", ["ws_8_4_bf", "slab_8_wide_bf", "ws_16_8_bf"])
def test_lin_fwd_two_inputs_gather_and_launch_mates(name):
    """The gathered / two-input forms equal the one-input call on the materialised
    concatenation bitwise, and a row's result does not depend on its launch mates: the
    same rows inside a larger launch give the same bits."""
    from cgnn_amd.gnn import linear
    c = fwd_case(name)
    got, _ = _run_fwd(c)
    cat = torch.full((c["n"], tight(c["K1"] + c["K2"])), PAD, dtype=F64)
    cat[:, :c["K1"] + c["K2"]] = c["X"]
    one = linear.lin_fwd(_dev(cat, BF16), _dev(c["W"], F32), _dev(c["b"], F32), K1=c["K1"] + c["K2"], relu=True,
                         rscale=_dev(c["rs"], F32), ldy=c["ldy"])
    _same(one.cpu().double(), got, name + " against the concatenated one-input call")
    big = 5 * c["n"] + 9
    reps = torch.arange(big) % c["n"]
    many = linear.lin_fwd(_dev(cat[reps], BF16), _dev(c["W"], F32), _dev(c["b"], F32), K1=c["K1"] + c["K2"], relu=True,
                          rscale=_dev(c["rs"][reps], F32), ldy=c["ldy"])
    _same(many.cpu().double(), got[reps], name + " inside a larger launch")


@pytest.mark.parametrize("nt", WS_NTS)
def test_lin_ws_fwd_exact_tiles_per_block(nt):
    """lin_ws forward with nt tiles on blocks 0 and 1 and nt - 1 on the others (n from the
    launcher's own grid): every residue of nt mod the ring depth, nt % 3 == 0 taking the
    store after the loop.  Rows periodic (period 1009), gathered, with row scales; p = 1/2
    draws the masks of tile i + 1 during tile i: all rows bit for bit, against the
    reference under the Philox mirror's mask of all n rows."""
    from cgnn_amd.gnn import linear
    name = "ws_8_4_bf"
    base = fwd_case(name, n=PERIOD, posbias=True)
    grid = _hip().gnn_lin_ws_grid(8, 4, 0, 0, 1 << 30)
    n = ws_rows(grid, nt)
    tiles = (n + TILE - 1) // TILE
    assert _hip().gnn_lin_ws_grid(8, 4, 0, 0, n) == min(grid, tiles) and (tiles - 1) // min(grid, tiles) + 1 == nt
    c = dict(base, n=n)
    assert _fwd_query(c, n, 0.5) == c["var"]
    rows = torch.arange(n, device=DEV) % PERIOD
    idx = _dev(base["idx"])[rows]
    rs = _dev(base["rs"], F32)[rows]
    for p in (0.0, 0.5):
        y16 = fwd_expected(base, p)[0]
        out = _Out(n, c["ldy"], BF16)
        linear.lin_fwd(_dev(base["X1"], BF16), _dev(base["W"], F32), _dev(base["b"], F32), K1=c["K1"], relu=True, p=p,
                       key=KEY, step=STEP, row0=ROW0, rscale=rs, out=out.t, idx1=idx, n=n)
        torch.cuda.synchronize()
        exp = _dev(y16, BF16)[rows]
        if p > 0:
            # the Philox mirror over ALL n rows (every tile's draw, the prologue's and the
            # pipelined ones): the zero pattern is the mask (every pre-activation is
            # positive) and the expected values are the reference under that mask
            keep = torch.zeros(n, c["ldy"], dtype=torch.bool)
            keep[:, :c["N"]] = ops.dropout_keep_mask(n, c["N"], p, KEY, STEP, ROW0)
            keep = keep.to(DEV)
            _same(out.t != 0, keep, "nt=%d zero pattern" % nt)
            exp = exp * keep
        _same(out.t, exp, "nt=%d p=%g" % (nt, p))
        assert bool((out.all[n:] == SENT).all()), "rows past n written"


def test_lin_fwd_slab_exact_three_tiles_per_wave():
    """The prefetching slab kernel (KS = 8, ragged loader) with 2 or 3 tiles per wave: both
    register sets of the next-tile prefetch and the hand-over between them."""
    from cgnn_amd.gnn import linear
    name = "slab_8_rag_bf"
    base = fwd_case(name, n=PERIOD)
    n = TILE * (2 * 8 * _cus() + 5) + 7
    c = dict(base, n=n)
    assert _fwd_query(c, n) == c["var"]
    rows = torch.arange(n, device=DEV) % PERIOD
    out = _Out(n, c["ldy"], BF16)
    linear.lin_fwd(_dev(base["X1"], BF16)[rows], _dev(base["W"], F32), _dev(base["b"], F32), K1=c["K1"], relu=True,
                   rscale=_dev(base["rs"], F32)[rows], out=out.t)
    torch.cuda.synchronize()
    _same(out.t, _dev(fwd_expected(base)[0], BF16)[rows], name)
    assert bool((out.all[n:] == SENT).all()), "rows past n written"


# ------------------------------------------------------------------ data backward
def _bwd_query(c, n, f32=False, rscale=True):
    K1, K2 = c["K1"], c["K2"]
    pad = c.get("pad", 0)
    return decode(_hip().gnn_lin_bwd_data_variant(c["ldd"], 1, c["ldd"], c["N"], K1, int(K2 > 0), K2, tight(K1) + pad,
                                                  tight(K2) if K2 else 0, n, int(rscale), int(f32)))


def _run_bwd(c, mscale, canary=False, mask=True, rscale=True, check=True):
    from cgnn_amd.gnn import linear
    n, K1, K2 = c["n"], c["K1"], c["K2"]
    f32 = bool(c.get("f32"))
    if check:
        assert _bwd_query(c, n, f32, rscale) == c["var"], "%s: variant %r" % (c["name"], _bwd_query(c, n, f32, rscale))
    o1 = _Out(n, tight(K1) + c.get("pad", 0), F32 if f32 else BF16)
    o2 = _Out(n, tight(K2), BF16) if K2 else None
    linear.lin_bwd_data(_dev(c["dY"], BF16, canary), _dev(c["W"], F32, canary), K1, K2,
                        Ym=_dev(c["Ym"], None, canary) if mask else None, mscale=mscale,
                        rscale=_dev(c["rs"], F32, canary) if rscale else None, out1=o1.t, out2=o2.t if K2 else None)
    torch.cuda.synchronize()
    return o1.get(c["name"] + " dX1"), (o2.get(c["name"] + " dX2") if K2 else None)


def _check_bwd(c, mscale, got, what, mask=True, rscale=True):
    K1, K2 = c["K1"], c["K2"]
    exp = bwd_expected(c, mscale, mask, rscale, bool(c.get("f32")))
    _same(got[0][:, :K1], exp[:, :K1], what + " dX1")
    pad = got[0][:, K1:]
    assert bool(((pad == 0) | (pad == SENT)).all()), what + ": dX1 padding columns hold neither zero nor the sentinel"
    if K2:
        exp2 = _bf16r(_mul32(c["acc"] if mask else c["acc_nomask"], mscale))[:, K1:]
        _same(got[1][:, :K2], exp2 * c["rs"][:, None] if rscale else exp2, what + " dX2")
        pad = got[1][:, K2:]
        assert bool(((pad == 0) | (pad == SENT)).all()), what + ": dX2 padding columns"


@pytest.mark.parametrize("name", sorted(BWD))
def test_lin_bwd_data_exact_every_template(name):
    """Every launchable data-backward template at mscale 1, 2 and fp32(1 / 0.7) (ONE fp32
    multiply by rs * mscale, then one bf16 rounding -- bit-exact at the inexact scale too;
    fp32 dX1 exactly), Ym holding signed zeros and subnormals, junk / NaN in the padding
    columns, operands inside NaN-filled allocations, without mask and row scale."""
    c = bwd_case(name)
    for ms in MSCALES:
        _check_bwd(c, ms, _run_bwd(c, ms), "%s mscale=%g" % (name, ms))
    cn = bwd_case(name, fill=NAN)
    _check_bwd(cn, 2.0, _run_bwd(cn, 2.0, canary=True), name + " (NaN padding, canary)")
    _check_bwd(c, 1.0, _run_bwd(c, 1.0, mask=False, rscale=False, check=False), name + " (no mask, no row scale)",
               mask=False, rscale=False)
    _same(_run_bwd(c, 2.0)[0], _run_bwd(c, 2.0)[0], name + " repeated call")


@pytest.mark.parametrize("name", ["ws_8_4", "slab_4_rag_lo", "slab_16_f32"])
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_lin_bwd_data_exact_row_counts(name, n):
    c = bwd_case(name, n=n)
    _check_bwd(c, MSCALES[2], _run_bwd(c, MSCALES[2]), "%s n=%d" % (name, n))


@pytest.mark.parametrize("name", ["ws_4_4", "slab_16_rag"])
def test_lin_bwd_data_rows_do_not_depend_on_launch_mates(name):
    """The same rows inside a larger launch (5 n + 9 rows, other blocks and waves) give the
    same bits, on the weight-stationary and the slab form."""
    from cgnn_amd.gnn import linear
    c = bwd_case(name)
    ms = MSCALES[2]
    got = _run_bwd(c, ms)
    reps = torch.arange(5 * c["n"] + 9) % c["n"]
    o1, o2 = linear.lin_bwd_data(_dev(c["dY"][reps], BF16), _dev(c["W"], F32), c["K1"], c["K2"], Ym=_dev(c["Ym"][reps]),
                                 mscale=ms, rscale=_dev(c["rs"][reps], F32))
    _same(o1.cpu().double()[:, :c["K1"]], got[0][reps][:, :c["K1"]], name + " dX1 inside a larger launch")
    if c["K2"]:
        _same(o2.cpu().double()[:, :c["K2"]], got[1][reps][:, :c["K2"]], name + " dX2 inside a larger launch")


@pytest.mark.parametrize("nt", WS_NTS)
def test_lin_ws_bwd_exact_tiles_per_block(nt):
    """lin_ws data backward with nt tiles on blocks 0 and 1 and nt - 1 on the others."""
    from cgnn_amd.gnn import linear
    name = "ws_4_4"
    base = bwd_case(name, n=PERIOD)
    grid = _hip().gnn_lin_ws_grid(4, 4, 0, 1, 1 << 30)
    n = ws_rows(grid, nt)
    tiles = (n + TILE - 1) // TILE
    assert (tiles - 1) // min(grid, tiles) + 1 == nt
    assert _bwd_query(dict(base, n=n), n) == base["var"]
    rows = torch.arange(n, device=DEV) % PERIOD
    K1, K2 = base["K1"], base["K2"]
    o1, o2 = _Out(n, tight(K1) + 24, BF16), _Out(n, tight(K2), BF16)
    ms = MSCALES[2]
    linear.lin_bwd_data(_dev(base["dY"], BF16)[rows], _dev(base["W"], F32), K1, K2, Ym=_dev(base["Ym"])[rows],
                        mscale=ms, rscale=_dev(base["rs"], F32)[rows], out1=o1.t, out2=o2.t)
    torch.cuda.synchronize()
    exp = _dev(bwd_expected(base, ms), BF16)[rows]
    _same(o1.t[:, :K1], exp[:, :K1], "nt=%d dX1" % nt)
    _same(o2.t[:, :K2], exp[:, K1:], "nt=%d dX2" % nt)
    assert bool((o1.all[n:] == SENT).all()) and bool((o2.all[n:] == SENT).all()), "rows past n written"


def test_lin_bwd_data_slab_exact_three_tiles_per_wave():
    """The prefetching branch of the slab kernel (KN = 16 on 8-wave blocks, fp32 dX1) with
    2 or 3 tiles per wave."""
    from cgnn_amd.gnn import linear
    name = "slab_16_f32"
    base = bwd_case(name, n=PERIOD)
    n = TILE * (2 * 8 * _cus() + 5) + 7
    assert _bwd_query(dict(base, n=n), n, True) == base["var"]
    rows = torch.arange(n, device=DEV) % PERIOD
    K1, K2 = base["K1"], base["K2"]
    o1, o2 = _Out(n, K1, F32), _Out(n, K2, BF16)
    ms = MSCALES[2]
    linear.lin_bwd_data(_dev(base["dY"], BF16)[rows], _dev(base["W"], F32), K1, K2, Ym=_dev(base["Ym"])[rows],
                        mscale=ms, rscale=_dev(base["rs"], F32)[rows], out1=o1.t, out2=o2.t)
    torch.cuda.synchronize()
    _same(o1.t, _dev(bwd_expected(base, ms, f32=True)[:, :K1], F32)[rows], name + " dX1")
    _same(o2.t, _dev(bwd_expected(base, ms)[:, K1:], BF16)[rows], name + " dX2")


# ------------------------------------------------------------------ weight backward
def _wgt_query(c, n, mask):
    return decode(_hip().gnn_lin_bwd_weight_variant(c["ld1"], c["K1"], int(c["K2"] > 0), c["ld2"], c["K2"], c["ldd"],
                                                    int(mask), c["ldd"], c["N"], n, int(c["idx"] is not None)))


def _poison_gpart(n, N, K):
    """The split-K scratch of the next lin_bwd_weight of this shape, filled with NaN."""
    from cgnn_amd.gnn import linear
    chunks = _hip().gnn_lin_wgrad_chunks(max(n, 1), N, K)
    shape = (chunks, K + 1, N)
    key = (torch.device(DEV).index, shape)
    gp = linear._GPART.get(key)
    if gp is None:
        gp = linear._GPART[key] = torch.empty(shape, dtype=F32, device=DEV)
    gp.fill_(NAN)
    return chunks


def _run_wgt(c, mscale, mask, canary=False, x1=None, x2=None, dY=None, Ym=None, idx=None, n=None):
    from cgnn_amd.gnn import linear
    n = c["n"] if n is None else n
    K, N = c["K1"] + c["K2"], c["N"]
    assert _wgt_query(c, n, mask) == (WGT2, c["ktnb"][0], 10 * c["ktnb"][1] + int(mask)), \
        "%s: variant %r" % (c["name"], _wgt_query(c, n, mask))
    chunks = _poison_gpart(n, N, K)
    dW, db = _Out(K, N, F32), _Out(1, N, F32)
    linear.lin_bwd_weight(_dev(c["X1"], BF16, canary) if x1 is None else x1,
                          _dev(c["dY"], BF16, canary) if dY is None else dY, N,
                          x2=(_dev(c["X2"], BF16, canary) if x2 is None else x2) if c["K2"] else None,
                          K1=c["K1"], K2=c["K2"] or None,
                          Ym=(_dev(c["Ym"], None, canary) if Ym is None else Ym) if mask else None, mscale=mscale,
                          dW=dW.t, db=db.t[0], idx1=_dev(c["idx"]) if idx is None else idx, n=n)
    torch.cuda.synchronize()
    return dW.get(c["name"] + " dW"), db.get(c["name"] + " db")[0], chunks


@pytest.mark.parametrize("name", sorted(WGT))
def test_lin_bwd_weight_exact_every_template(name):
    """Every (KT, NB) of lin_bwd_weight2 with and without Ym, 10 chunks of one tile (the last
    ragged), the split-K scratch NaN before every call: dW and db bit for bit at mscale 1,
    2 and fp32(1 / 0.7); junk / NaN padding columns; operands in NaN-filled allocations;
    both reduce kernels ((K + 1) N % 4 zero and non-zero) across the cases."""
    c = wgt_case(name)
    for mask in (True, False):
        for ms in MSCALES:
            dW, db, chunks = _run_wgt(c, ms, mask)
            assert chunks == 10
            eW, eb = wgt_expected(c, ms, mask)
            _same(dW, eW, "%s mask=%d mscale=%g dW" % (name, mask, ms))
            _same(db, eb, "%s mask=%d mscale=%g db" % (name, mask, ms))
    cn = wgt_case(name, fill=NAN)
    dW, db, _ = _run_wgt(cn, 2.0, True, canary=True)
    eW, eb = wgt_expected(cn, 2.0, True)
    _same(dW, eW, name + " dW (NaN padding, canary)")
    _same(db, eb, name + " db (NaN padding, canary)")
    again = _run_wgt(cn, 2.0, True, canary=True)
    _same(again[0], dW, name + " repeated call")


def test_lin_bwd_weight_cases_reach_both_reduce_kernels():
    counts = {((s["K1"] + s["K2"] + 1) * s["N"]) % 4 == 0 for s in WGT.values()}
    assert counts == {True, False}


@pytest.mark.parametrize("n,chunks", [(1, 1), (31, 1), (32, 1), (33, 2), (65, 3), (280, 9), (33 * TILE - 5, 33)])
def test_lin_bwd_weight_exact_row_and_chunk_counts(n, chunks):
    """1, 31, 32, 33 and 65 rows; 1, 9 and 33 chunks (the reduce kernels' 8 lane groups and
    their 4-deep unrolled loop)."""
    for name in ("4_2", "8_4"):
        c = wgt_case(name, n=n)
        dW, db, got_chunks = _run_wgt(c, 2.0, True)
        assert got_chunks == chunks
        eW, eb = wgt_expected(c, 2.0, True)
        _same(dW, eW, "%s n=%d dW" % (name, n))
        _same(db, eb, "%s n=%d db" % (name, n))


@pytest.mark.parametrize("tpc", [1, 2, 3, 4, 5, 0])
def test_lin_bwd_weight_exact_tiles_per_chunk(tpc):
    """The maximum chunk count (one per CU) with 1 to 5 tiles per chunk, the last tile
    ragged (the double-buffered images behind the loads of tile t + 2); tpc = 0: CUs + 1
    tiles, two per chunk, so the trailing chunks have no rows and must still write zero
    slabs into the NaN-filled scratch.  Rows periodic, x1 gathered."""
    cus = _cus()
    name = "8_4"
    base = wgt_case(name, period=PERIOD)
    n = wgt_rows(cus, tpc) if tpc else TILE * (cus + 1) - 13
    reps, last = divmod(n, PERIOD)
    rows = torch.arange(n, device=DEV) % PERIOD
    dW, db, chunks = _run_wgt(base, 2.0, True, x1=_dev(base["X1"], BF16), x2=_dev(base["X2"], BF16)[rows],
                              dY=_dev(base["dY"], BF16)[rows], Ym=_dev(base["Ym"])[rows], idx=_dev(base["idx"])[rows], n=n)
    assert chunks == cus
    eW, eb = wgt_expected(base, 2.0, True, reps, last)
    _same(dW, eW, "tpc=%d dW" % tpc)
    _same(db, eb, "tpc=%d db" % tpc)


def test_lin_bwd_weight_gathered_equals_materialised():
    """idx1 with repeats, out of order, into a larger table: bitwise the call on the
    gathered rows."""
    from cgnn_amd.gnn import linear
    c = wgt_case("8_4")
    dW, db, _ = _run_wgt(c, MSCALES[2], True)
    x1 = _dev(c["X1"], BF16)[_dev(c["idx"]).long()].contiguous()
    dW2, db2 = linear.lin_bwd_weight(x1, _dev(c["dY"], BF16), c["N"], x2=_dev(c["X2"], BF16), K1=c["K1"],
                                     Ym=_dev(c["Ym"]), mscale=MSCALES[2])
    _same(dW2.cpu().double(), dW, "dW")
    _same(db2.cpu().double(), db, "db")


# ------------------------------------------------------------------ coverage, agreement, rejections
def test_cases_reach_every_launchable_template():
    """The variants the launchers' own selection reports for the cases above are the
    launchers' whole tables (the exact tests assert the same variant before each launch)."""
    fwd = {table_key(_fwd_query(fwd_case(k), FWD_N), s["fp16"]) for k, s in FWD.items()}
    assert fwd == FWD_TABLE, (sorted(fwd - FWD_TABLE), sorted(FWD_TABLE - fwd))
    for k in FWD:
        assert _fwd_query(fwd_case(k), FWD_N) == FWD[k]["var"], k
    bwd = {table_key(_bwd_query(bwd_case(k), FWD_N, bool(s.get("f32")))) for k, s in BWD.items()}
    assert bwd == BWD_TABLE, (sorted(bwd - BWD_TABLE), sorted(BWD_TABLE - bwd))
    staged = {(v[0], v[2] % 10) for v in (s["var"] for s in list(BWD.values()) + list(FWD.values())) if v[0] == SLAB}
    assert staged == {(SLAB, 0), (SLAB, 1)}
    wgt = set()
    for k in WGT:
        for mask in (0, 1):
            f, a, b = _wgt_query(wgt_case(k), WGT_N, mask)
            wgt.add((f, a, b // 10, b % 10))
    assert wgt == WGT_TABLE and {v[1:3] for v in wgt} == set(WGT_LIST)


def _launch_code(call, out):
    """0 if ``call`` ran; the launcher's code if it raised with one; "none" if the Python
    layer found no weight image for the shape before any launch.  A refused call leaves
    ``out`` untouched."""
    try:
        call()
        return 0
    except RuntimeError as e:
        assert out.untouched(), "a refused call wrote its output"
        for code in (-1, -3):
            if "(code %d)" % code in str(e):
                return code
        assert "no HIP variant for this weight shape" in str(e), str(e)
        return "none"


def _agree(q, rc):
    """The query reports a variant exactly where the launch runs, and the launcher's own
    code where it refuses."""
    return q < 0 if rc == "none" else (q if q < 0 else 0) == rc


def test_variant_queries_agree_with_the_launchers():
    """On a grid of shapes with one row of zeros: the query reports no variant (-1) or a bad
    shape (-3) exactly where the launch returns that code, and a variant where it runs."""
    from cgnn_amd.gnn import linear
    hip = _hip()
    seen = set()
    for et, dt in ((0, BF16), (1, F16)):
        for K in (8, 64, 100, 256, 264, 512, 520, 602, 768, 776, 1000):
            for N in (8, 64, 100, 136, 256, 264):
                for p in (0.0, 0.5):
                    ld, ldy = tight(K), tight(N)
                    q = hip.gnn_lin_fwd_variant(ld, K, 0, 0, 0, N, ldy, 1, p, 0, 0, 0, 0, 1, et)
                    x, W = torch.zeros(1, ld, dtype=dt, device=DEV), torch.zeros(K, N, device=DEV)
                    out = _Out(1, ldy, dt)
                    rc = _launch_code(lambda: linear.lin_fwd(x, W, None, K1=K, p=p, out=out.t), out)
                    assert _agree(q, rc), "fwd et=%d K=%d N=%d p=%g: query %d, launch %r" % (et, K, N, p, q, rc)
                    seen.add(q if q < 0 else q // 1000000)
    assert seen == {-1, -3, WS, SLAB, KC, GEMM}
    seen = set()
    for N in (8, 100, 256, 512, 520, 640, 776):
        for K in (8, 100, 256, 264, 1000):
            for f32 in (0, 1):
                ldd, ldx = tight(N), tight(K)
                q = hip.gnn_lin_bwd_data_variant(ldd, 0, 0, N, K, 0, 0, ldx, 0, 1, 0, f32)
                out = _Out(1, ldx, F32 if f32 else BF16)
                dY, W = torch.zeros(1, ldd, dtype=BF16, device=DEV), torch.zeros(K, N, device=DEV)
                rc = _launch_code(lambda: linear.lin_bwd_data(dY, W, K, out1=out.t), out)
                assert _agree(q, rc), "bwd N=%d K=%d: query %d, launch %r" % (N, K, q, rc)
                seen.add(q if q < 0 else q // 1000000)
    assert seen == {-1, WS, SLAB}
    seen = set()
    for K in (8, 100, 288, 544, 552, 1000):
        for N in (8, 100, 256, 300):
            q = hip.gnn_lin_bwd_weight_variant(tight(K), K, 0, 0, 0, tight(N), 0, 0, N, 1, 0)
            dW = _Out(K, N, F32)
            x, dY = torch.zeros(1, tight(K), dtype=BF16, device=DEV), torch.zeros(1, tight(N), dtype=BF16, device=DEV)
            rc = _launch_code(lambda: linear.lin_bwd_weight(x, dY, N, K1=K, dW=dW.t), dW)
            assert _agree(q, rc), "wgt K=%d N=%d: query %d, launch %r" % (K, N, q, rc)
            seen.add(q if q < 0 else q // 1000000)
    assert seen == {-1, WGT2}
    torch.cuda.synchronize()


def slab_cols(cols, KP):
    """(Mirror of gnn_linear.hip's slab_cols and its 144 KiB budget; if that budget changes,
    change it here too, or ``need`` below no longer is what the launcher writes.)
    Width of a slab: the widest multiple of 32 columns whose 16-bit image rows (KP + 8
    values) and fp32 bias fit 144 KiB of LDS."""
    w = (cols + 31) // 32 * 32
    while w > 32 and w * (KP + 8) * 2 + w * 4 > 144 * 1024:
        w -= 32
    return w


def test_weight_image_scratch_covers_every_slab():
    """gnn_lin_fwd_image_bytes / gnn_lin_bwd_image_bytes size the scratch the image kernels
    fill: slabs * width rows of KP + 8 values.  (The former bound, columns + 256 rows, fell
    short once a slab was wider than 256 columns and there were two: the image kernel wrote
    past the scratch, e.g. forward K = 128 x N = 520, backward N = 8 x K = 1000.)"""
    hip = _hip()
    short = 0
    for red in (8, 40, 64, 100, 128, 200, 256, 384, 512):            # the reduction (K fwd, N bwd)
        KP = next(16 * c for c in (4, 8, 16, 24, 32) if (red + 15) // 16 <= c)
        for cols in (8, 256, 264, 520, 544, 840, 992, 1000, 1024, 2000, 4100):
            w = slab_cols(cols, KP)
            need = 2 * ((cols + w - 1) // w) * w * (KP + 8)
            short += need > 2 * ((cols + 31) // 32 * 32 + 256) * (KP + 8)
            assert hip.gnn_lin_fwd_image_bytes(red, cols, tight(cols)) >= need, ("fwd", red, cols)
            assert hip.gnn_lin_bwd_image_bytes(cols, red) >= need, ("bwd", red, cols)
    assert short > 0                                                  # the grid holds shapes the old bound missed


def test_bad_shapes_are_rejected_before_any_launch():
    """Every -3 condition of the three launchers: the selection query says -3, the launcher
    returns -3 through its binding, and the Python op raises (for three tail conditions by
    its own check, before the launcher) -- with the outputs untouched."""
    from cgnn_amd.gnn import linear
    n = 5

    def z(rows, cols, dt=BF16):
        return torch.zeros(rows, cols, dtype=dt, device=DEV)

    def wide(rows, cols, pitch, dt=BF16):
        return torch.zeros(rows, pitch, dtype=dt, device=DEV)[:, :cols]

    W = torch.zeros(32, 16, device=DEV)
    fwd_bad = [
        dict(x1=wide(n, 12, 16), x2=z(n, 24), K1=12, K2=20),          # x2 with K1 % 8
        dict(x1=z(n, 36)[:, :32], K1=32),                             # ld1 % 8
        dict(x1=z(n, 16), x2=wide(n, 16, 20), K1=16, K2=16),          # ld2 % 8
        dict(x1=z(n, 32), K1=32, ldy=20),                             # ldy % 8
        dict(x1=z(n, 24), K1=32),                                     # K1 > ld1
        dict(x1=z(n, 16), x2=z(n, 8), K1=16, K2=16),                  # K2 > ld2
        dict(x1=z(n, 32), K1=32, ldy=8),                              # N > ldy
        dict(x1=z(n, 32), K1=32, tail=True, nsplit=12, ldy=8),        # nsplit > ldy
        dict(x1=z(n, 32), K1=32, tail=True, nsplit=20, ldy=24),       # nsplit > N (= 16)
        dict(x1=z(n, 32), K1=32, tail=True, nsplit=8, tk=-1),         # tk <= 0
        dict(x1=z(n, 32), K1=32, tail=True, nsplit=8, tk=0, py=ZeroDivisionError),
        dict(x1=z(n, 32), K1=32, tail=True, nsplit=6, py=ValueError),           # nsplit % 4
        dict(x1=z(n, 32), K1=32, tail=True, nsplit=8, tk=3, py=ValueError),     # (N - nsplit) % tk
        dict(x1=z(n, 32, F16), K1=32, p=0.5),                         # fp16 with dropout
        dict(x1=z(n, 32, F16), K1=32, tail=True, nsplit=8),           # fp16 with a tail
    ]
    hip = _hip()
    img = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    for kw in fwd_bad:
        kw = dict(kw)
        x1, x2 = kw.pop("x1"), kw.get("x2")
        dt, et = x1.dtype, int(x1.dtype == F16)
        out = _Out(n, kw.pop("ldy", 16), dt)
        planes = _Out(n * 16, 1, F32)
        o = out.t if out.ld % 8 == 0 else out.flat[:n * out.ld].view(n, out.ld)
        tail, py = kw.pop("tail", False), kw.pop("py", None)
        K1, K2, pp = kw["K1"], kw.get("K2", 0), kw.get("p", 0.0)
        nsplit, tk = kw.get("nsplit", 0), kw.get("tk", 1)
        ld2 = x2.stride(0) if x2 is not None else 0
        # the launcher's own selection, the launcher through its binding, and lin_fwd (which
        # refuses three of the tail conditions itself, before the launcher sees them)
        assert hip.gnn_lin_fwd_variant(x1.stride(0), K1, int(x2 is not None), ld2, K2, 16, out.ld, n, pp, 0, 0, int(tail),
                                       nsplit, tk, et) == -3, kw
        rc = hip.gnn_lin_fwd(x1.data_ptr(), x1.stride(0), K1, ops._ptr(x2), ld2, K2, W.data_ptr(), 16, 0, o.data_ptr(),
                             out.ld, n, 0, pp, 0, 0, 0, 0, 0, 0, ops._st(x1), idx1=0, wimg=img.data_ptr(),
                             yf=planes.t.data_ptr() if tail else 0, nsplit=nsplit, tk=tk, et=et)
        assert rc == -3, kw
        if tail:
            kw.update(tail=planes.t)
        with (pytest.raises(py) if py else pytest.raises(RuntimeError, match="code -3")):
            linear.lin_fwd(x1, W, None, out=o, n=n, **kw)
        torch.cuda.synchronize()
        assert out.untouched() and planes.untouched(), kw
    Wb = torch.zeros(16, 32, device=DEV)
    bwd_bad = [
        dict(dY=wide(n, 32, 36)),                                     # lddy % 8
        dict(dY=z(n, 32), Ym=wide(n, 32, 36)),                        # ldym % 8
        dict(dY=z(n, 32), K1=12, K2=4, out2=z(n, 8)),                 # dX2 with K1 % 8
        dict(dY=z(n, 32), ld1=20),                                    # ldx1 % 8
        dict(dY=z(n, 32), K1=8, K2=8, out2=wide(n, 8, 12)),           # ldx2 % 8
        dict(dY=z(n, 24)),                                            # N > lddy
    ]
    for kw in bwd_bad:
        kw = dict(kw)
        ld1 = kw.pop("ld1", 16)
        out = _Out(n, ld1, BF16)
        o = out.t if ld1 % 8 == 0 else out.flat[:n * ld1].view(n, ld1)
        with pytest.raises(RuntimeError, match="code -3"):
            linear.lin_bwd_data(kw.pop("dY"), Wb, kw.pop("K1", 16), kw.pop("K2", 0), out1=o, **kw)
        torch.cuda.synchronize()
        assert out.untouched(), kw
    wgt_bad = [
        dict(x1=wide(n, 12, 16), x2=z(n, 8), K1=12),                  # x2 with K1 % 8
        dict(x1=wide(n, 16, 20)),                                     # ld1 % 8
        dict(x1=z(n, 8), x2=wide(n, 8, 12), K1=8),                    # ld2 % 8
        dict(x1=z(n, 16), dY=wide(n, 32, 36)),                        # lddy % 8
        dict(x1=z(n, 16), Ym=wide(n, 32, 36)),                        # ldym % 8
        dict(x1=z(n, 16), dY=z(n, 24)),                               # N > lddy
    ]
    for kw in wgt_bad:
        kw = dict(kw)
        dW, db = _Out(24, 32, F32), _Out(1, 32, F32)
        with pytest.raises(RuntimeError, match="code -3"):
            linear.lin_bwd_weight(kw.pop("x1"), kw.pop("dY", z(n, 32)), 32, dW=dW.t, db=db.t[0], **kw)
        torch.cuda.synchronize()
        assert dW.untouched() and db.untouched(), kw


def test_zero_rows_return_cleanly():
    """n = 0: the forward and the data backward write nothing; lin_bwd_weight gives zero
    dW and db out of a NaN-filled scratch."""
    from cgnn_amd.gnn import linear
    W = torch.ones(16, 32, device=DEV)
    out = _Out(0, 32, BF16)
    linear.lin_fwd(torch.zeros(0, 16, dtype=BF16, device=DEV), W, None, out=out.t, n=0)
    o1 = _Out(0, 16, BF16)
    linear.lin_bwd_data(torch.zeros(0, 32, dtype=BF16, device=DEV), W, 16, out1=o1.t)
    _poison_gpart(0, 32, 16)
    dW, db = _Out(16, 32, F32), _Out(1, 32, F32)
    linear.lin_bwd_weight(torch.zeros(0, 16, dtype=BF16, device=DEV), torch.zeros(0, 32, dtype=BF16, device=DEV), 32,
                          dW=dW.t, db=db.t[0], n=0)
    torch.cuda.synchronize()
    assert out.untouched() and o1.untouched()
    _same(dW.get("dW"), torch.zeros(16, 32, dtype=F64), "dW")
    _same(db.get("db"), torch.zeros(1, 32, dtype=F64), "db")


def test_layer_step_in_a_captured_graph_equals_eager():
    """Forward (dropout keyed by a device step counter), data backward and weight backward
    of one layer: replayed from a captured graph, bit for bit the eager results, at the
    step value current at replay time."""
    from cgnn_amd.gnn import linear
    c = fwd_case("ws_8_8_bf", posbias=True)
    n, K, N, ldy = c["n"], c["K1"], c["N"], c["ldy"]
    x, W, b, rs = _dev(c["X1"], BF16), _dev(c["W"], F32), _dev(c["b"], F32), _dev(c["rs"], F32)
    dY = _dev(_rows(np.random.default_rng(3), n, N, ldy, 3, PAD), BF16)
    step = torch.tensor([STEP], dtype=torch.int32, device=DEV)

    def bufs():
        return (torch.full((n, ldy), SENT, dtype=BF16, device=DEV), torch.full((n, c["ld1"]), SENT, dtype=BF16, device=DEV),
                torch.full((K, N), SENT, device=DEV), torch.full((N,), SENT, device=DEV))

    def layer(y, dX, dW, db):
        linear.lin_fwd(x, W, b, K1=K, relu=True, p=0.5, key=KEY, step=step, row0=ROW0, rscale=rs, out=y)
        linear.lin_bwd_data(dY, W, K, Ym=y, mscale=2.0, rscale=rs, out1=dX)
        linear.lin_bwd_weight(x, dY, N, K1=K, Ym=y, mscale=2.0, dW=dW, db=db)

    eager = bufs()
    layer(*eager)
    torch.cuda.synchronize()
    _check_fwd(c, 0.5, (eager[0].cpu().double(), None), "eager forward")
    replay = bufs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer(*replay)                                # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layer(*replay)
    for t in replay:
        t.fill_(SENT)
    graph.replay()
    torch.cuda.synchronize()
    for e, r, what in zip(eager, replay, ("out", "dX", "dW", "db")):
        _same(r, e, "graph replay " + what)
    step.fill_(STEP + 1)
    graph.replay()
    layer(*eager)
    torch.cuda.synchronize()
    for e, r, what in zip(eager, replay, ("out", "dX", "dW", "db")):
        _same(r, e, "graph replay at the next step, " + what)
    keep = ops.dropout_keep_mask(n, N, 0.5, KEY, STEP + 1, ROW0)
    _same((replay[0][:, :N] != 0).cpu(), keep, "mask at the next step")
