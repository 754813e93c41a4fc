"""Oracle tests of the GAT attention kernels (gnn_gat.hip: gat_fwd_kernel, gat_row_kernel,
gat_col_kernel, gat_row_ce_kernel, gat_pack_grad_kernel, gat_colsum_kernel), one (heads, head
width) per compiled (L, G) variant, each in bf16 and in fp32 storage.

Every reference is computed here, in fp64 / numpy from the CSR (dense [n, n_cols] attention
matrices per head) -- never through ``_gat_aggregate_torch``, the CPU branches of
``gat_fused`` or ``ops``.  The builders and references are shared with
tests/test_gat_exact_cpu.py, which checks them without a GPU.

Graphs: for the variant's sub-group width L the 53 row lengths of test_gnn_pool_gpu.py's
``_degrees(L)`` (0, 1, L - 1, L, L + 1, 2 L +- 1, 3 L + 5, ...) and two hub rows of 4099 and
4096 edges; 257 source rows (!= n); column ids include 0 and 256 and repeat within a row, and
a third of all edges read five popular sources, so the transposed CSR (built in numpy) has
long rows of its own.  The column half is also run on the degree list itself as the
transposed CSR, which gives it the exact row lengths around the chunk boundaries.

Exact tier (bit for bit; every builder asserts sum|terms| / quantum < 2^24):
  forward      every edge of a (row, head) has the same score (s_src = 0, or a per-head
               constant with arbitrary s_dst, both signs of the raw score): every exp2
               argument is 0 or -inf, l = deg, acc an exact sum of dyadic Wh, and
               out = fl32(acc * fl32(1 / deg)) for EVERY degree (the division is correctly
               rounded).  q is exactly 0 on the positive side; on the 0.2-slope side it is the
               rounding residual out- - c- out, asserted below 4 u |out|.  lse is bounded (the
               hardware log2): u (4 M + 2 log2(deg + 1) + 4 |lse| + 6).
  row half     D, ds_dst = fl32(fl32(-0.8) dq), rstat.x / .y = fl32(s fl32(log2 e)), .w = 0,
               the bf16 dy column HF + K + k.
  column half  alpha = 1 and slope 1 (s_src = 0, rstat.x > 0, rstat.y = rstat.x): dWh, ds_src in
               fp32 and as bf16 dy columns [0, HF + K).
  pack_grad    bf16(cat), pads zeroed, rows past n untouched.

Bounded tier (random inputs on a grid that keeps every raw score at least 2^-11 from 0, so the
LeakyReLU side of the reference is the kernel's; fp64 reference of the same stored inputs;
u = 2^-24, M = max over the row's edges of (|s_dst| + |s_src|) log2 e, deg the row length):
  score   sd = fl(s_dst c), t = fma(s_src, c, sd), c = fl(log2 e): absolute error <= 3 u M;
          leaky2 multiplies by fl(0.2): <= 3.25 u M.  The kernel is an exact online softmax
          of these scores up to the roundings below; softmax is shift invariant, so
          alpha~ / alpha is within 2^(+-2 * 3.25 u M): 4.5 u M relative.
  exp2    of a rounded difference: the differences of an edge telescope to m_final - sc_j
          <= 2 M, so ln2 * 2 M u for the numerator and as much for the denominator, and one
          v_exp_f32 (2 u) per factor.
  rescale one factor sa per batch of 2 edges (2 u) and one multiply (u): 1.5 u deg.
  chain   one fmaf per edge: u deg.  Numerator 2.5 u deg, denominator (l) as much.
  final   fl(1 / l), the multiply, the edge's own exp2 twice: 6 u, 2 u slack.
  out     |out - out*| <= E sum_j alpha_j |Wh_j|,  E = (8 M + 5 deg + 8) u (1 + that)
  lse     u (4 M + 2.5 deg + 2 log2(deg + 1) + 4 |lse| + 6)   (log-sum-exp is 1-Lipschitz)
  q       (2 E + 4 u) (sum n alpha |Wh| + c- sum alpha |Wh|), plus 2^-8 |q| stored as bf16
  rstat.z, ds_dst   chains of 8 fmaf and log2 G adds: (9 + log2 G) u sum |d o|, and
          (11 + log2 G) u 0.8 sum |d q|; against the per-edge fp64 sum (the identity
          ds_dst = -0.8 <dout, q>) the error of q enters as 0.8 sum_f |dout_f| bound_q_f
  column half   alpha from the stored rstat: relative (3 Mc + 2) u, Mc = max (|x_i| + |ss_j| +
          |y_i|); dWh: (3 Mc + deg_t + 3) u sum alpha |dout|; ds_src: (3 Mc + deg_t + log2 G +
          14) u sum alpha slope (sum |dout Wh| + |D|).
None of these constants was tuned to a result.  Largest error / bound observed on an MI355X
over every case (the tests print them): out 0.11, lse 0.23, q 0.08 in fp32 storage and 0.99 in
bf16 (the storage rounding itself, which the bound includes as 2^-8 |q|), rstat.z 0.31, ds_dst
0.27, ds_dst against the per-edge sum 0.02 (0.64 with bf16 q), dWh 0.58, ds_src 0.19.  The
forward's out matched the mirror bit for bit on every degree, so no degree is left to the
bounded tier.

Not covered: NaN / inf inputs, the halo (sharded) callers, hipGraph capture (covered by
tests/test_gat_fused_gpu.py), gat_colsum_kernel beyond the sums it forms for row_ce and db.
"""
import functools
import math

import numpy as np
import pytest
import torch

from cgnn_amd import native

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -7.0
HUBS = (4099, 4096)
N_SRC = 257
POPULAR = (0, 256, 100, 7, 31)
U = 2.0 ** -24
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
L2E32 = float(np.float32(1.4426950408889634))
LN2_32 = float(np.float32(0.6931471805599453))
LOG2E = math.log2(math.e)

# one (K, Fh) per compiled (L, G) pair, and a second one-head shape that does not fill its
# sub-group; code = L * 100 + G
SHAPES = [
    (3, 8, 801), (3, 16, 802), (2, 32, 804), (1, 24, 808), (1, 40, 808),
    (13, 8, 1601), (5, 16, 1602), (3, 32, 1604), (2, 64, 1608), (1, 72, 1616),
    (19, 8, 3201), (11, 16, 3202), (8, 32, 3204), (3, 64, 3208), (2, 128, 3216), (1, 176, 3232),
    (37, 8, 6401), (21, 16, 6402), (16, 32, 6404), (5, 64, 6408), (3, 128, 6416), (2, 256, 6432), (1, 280, 6464),
]
TABLE = {L * 100 + G for L in (8, 16, 32, 64) for G in (1, 2, 4, 8, 16, 32, 64) if G <= L // 2 or G == L}
FORMERLY_MISSING = {3201, 6401, 6402, 6432}
CASES = [(K, Fh, wbf) for K, Fh, _ in SHAPES for wbf in (1, 0)]
CODE = {(K, Fh): c for K, Fh, c in SHAPES}
PATTERNS = ("normal3", "asc", "desc", "plus120", "minus120", "straddle")
# the shapes that run every score pattern (one per L); the others run one each, in rotation
ALL_PATTERNS = {(2, 32), (3, 32), (8, 32), (5, 64)}


def _id(c):
    return "K%d_Fh%d_%s" % (c[0], c[1], "bf16" if c[2] else "fp32")


def rule(K, Fh):
    """The documented shape rule of the HIP aggregation (gat_aggregate / FusedGAT.supported)."""
    return Fh % 8 == 0 and (K == 1 or (Fh // 8) & (Fh // 8 - 1) == 0) and K * Fh <= 512


def expected_variant(K, Fh):
    c = (K * Fh + 7) // 8
    L = 8 if c <= 8 else 16 if c <= 16 else 32 if c <= 32 else 64
    return L * 100 + (L if K == 1 else Fh // 8)


# ------------------------------------------------------------------ graphs
def _degrees(L):
    """The row-length list of test_gnn_pool_gpu.py."""
    d = [0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, L - 1, L, L + 1, L + 4, L + 8, L + 13,
         2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 5]
    return d + d[::-1] + [2, L + 1, 0]


def transpose(rp, col, n_cols):
    """Transposed CSR in numpy: (rowptr_t, col_t); the destinations of a source in increasing
    order (stable sort)."""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    perm = np.argsort(col, kind="stable")
    rpt = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n_cols))]).astype(np.int32)
    return rpt, rows[perm].astype(np.int32)


@functools.lru_cache(maxsize=None)
def graph(L, order=None, reverse=False):
    """order: None, or 'asc' / 'desc': every row's sources sorted by RANK[source]."""
    deg = _degrees(L) + list(HUBS)
    assert len(deg) == 55
    if reverse:
        deg = deg[::-1]
    deg = np.asarray(deg, dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    nnz = int(rp[-1])
    rng = np.random.default_rng(1000 + L)
    col = rng.integers(0, N_SRC, nnz)
    pop = rng.random(nnz) < 1 / 3
    col[pop] = np.asarray(POPULAR)[rng.integers(0, len(POPULAR), int(pop.sum()))]
    rows = np.repeat(np.arange(len(deg)), deg)
    if reverse:                                        # the same rows, in the reversed order
        fwd = graph(L)
        for i in range(len(deg)):
            j = len(deg) - 1 - i
            col[rp[i]:rp[i + 1]] = fwd["col"][fwd["rp"][j]:fwd["rp"][j + 1]]
    else:
        first = np.flatnonzero(deg >= 3)
        col[rp[first[0]]], col[rp[first[1]] + 1] = 0, N_SRC - 1
        e0 = int(rp[first[2]])
        col[e0 + 1] = col[e0]                          # a source repeated within a row
    if order is not None:
        key = RANK[col] if order == "asc" else -RANK[col]
        col = col[np.lexsort((key, rows))]
    col = col.astype(np.int32)
    rpt, colt = transpose(rp, col, N_SRC)
    return dict(n=len(deg), deg=deg, rp=rp, col=col, nnz=nnz, rows=rows, rpt=rpt, colt=colt)


RANK = np.random.default_rng(7).permutation(N_SRC).astype(np.float64)


def lanes_of(K, Fh):
    return CODE[(K, Fh)] // 100 if (K, Fh) in CODE else expected_variant(K, Fh) // 100


def dev_graph(g):
    """Device arrays of a graph (cached on the dict)."""
    if "d" not in g:
        g["d"] = {k: torch.from_numpy(g[k]).to(DEV) for k in ("rp", "col", "rpt", "colt")}
    return g["d"]


# ------------------------------------------------------------------ roundings
def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def bf16r(x):
    """bf16 round-to-nearest-even of fp32-representable values (fp64 in, fp64 out)."""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
    return t.to(BF16).double().numpy()


def store(x, wbf):
    """The values as the kernel's storage type holds them."""
    return bf16r(x) if wbf else f32(x)


def dyadic(rng, shape, steps, lim):
    """Multiples of 1 / steps in [-lim, lim]."""
    return rng.integers(-lim * steps, lim * steps + 1, shape).astype(np.float64) / steps


# ------------------------------------------------------------------ fp64 references
def dense(g, w):
    """[nnz, K] edge weights -> [K, n, N_SRC] (duplicate edges add)."""
    K = w.shape[1]
    flat = g["rows"] * N_SRC + g["col"]
    out = np.empty((K, g["n"] * N_SRC))
    for k in range(K):
        out[k] = np.bincount(flat, weights=w[:, k], minlength=g["n"] * N_SRC)
    return out.reshape(K, g["n"], N_SRC)


def heads(x, K):
    """[r, K Fh] -> [K, r, Fh]"""
    return np.ascontiguousarray(x.reshape(x.shape[0], K, -1).transpose(1, 0, 2))


def unheads(x):
    """[K, r, Fh] -> [r, K Fh]"""
    return np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(x.shape[1], -1)


def attention(g, s_src, s_dst):
    """fp64: raw [nnz, K], alpha [nnz, K], lse [n, K] (0 for an empty row), neg [nnz, K]."""
    rows, col, n = g["rows"], g["col"], g["n"]
    raw = s_dst[rows] + s_src[col]
    e = np.where(raw > 0, raw, 0.2 * raw)
    m = np.full((n, raw.shape[1]), -np.inf)
    np.maximum.at(m, rows, e)
    ex = np.exp(e - m[rows])
    l = np.zeros_like(m)
    np.add.at(l, rows, ex)
    alpha = ex / l[rows]
    lse = np.where(l > 0, np.where(l > 0, m, 0) + np.log(np.where(l > 0, l, 1)), 0.0)
    return raw, alpha, lse, raw <= 0


def forward_ref(g, Wh, s_src, s_dst, K):
    """out, lse, q and the sums of |terms| of out and q, and M per (row, head) -- all fp64."""
    raw, alpha, lse, neg = attention(g, s_src, s_dst)
    A, An = dense(g, alpha), dense(g, alpha * neg)
    W = heads(Wh, K)                                          # [K, N_SRC, Fh]
    out, outn = A @ W, An @ W
    aout, aoutn = A @ np.abs(W), An @ np.abs(W)
    cn = An.sum(2)[:, :, None]
    q = outn - cn * out
    M = np.zeros((g["n"], K))
    np.maximum.at(M, g["rows"], (np.abs(s_dst[g["rows"]]) + np.abs(s_src[g["col"]])) * LOG2E)
    return dict(out=unheads(out), q=unheads(q), lse=lse, aout=unheads(aout), aq=unheads(aoutn + cn * aout), M=M,
                alpha=alpha, raw=raw)


def forward_bounds(g, ref, K, wbf):
    """Per-element bounds of out, lse, q (module docstring)."""
    deg = g["deg"][:, None].astype(np.float64)
    E = (8 * ref["M"] + 5 * deg + 8) * U
    E = E * (1 + E)
    Fh = ref["out"].shape[1] // K
    Ef = np.repeat(E, Fh, axis=1)
    b_out = Ef * ref["aout"]
    b_lse = U * (4 * ref["M"] + 2.5 * deg + 2 * np.log2(deg + 1) + 4 * np.abs(ref["lse"]) + 6)
    b_q = (2 * Ef + 4 * U) * ref["aq"]
    if wbf:
        b_q = b_q + 2.0 ** -8 * (np.abs(ref["q"]) + b_q)
    return b_out, b_lse, b_q


def rows_ref(dout, out, q, lse, s_dst, K):
    """The row half from its stored inputs (fp64): D, ds_dst, sums of |terms|, rstat x / y."""
    d, o, qq = heads(dout, K), heads(out, K), heads(q, K)
    D, dq = (d * o).sum(2).T, (d * qq).sum(2).T
    aD, adq = np.abs(d * o).sum(2).T, np.abs(d * qq).sum(2).T
    return dict(D=D, dq=dq, aD=aD, adq=adq, x=f32(f32(s_dst) * L2E32), y=f32(f32(lse) * L2E32))


def cols_ref(rpt, colt, Wh, s_src, rstat, dout, K, G):
    """The column half from its stored inputs: rstat [n_dst, K, 4] fp32 values, dout [n_dst, HF];
    rows of the transposed CSR (rpt, colt) are the sources.  fp64 dWh, ds_src and their bounds."""
    ns = len(rpt) - 1
    srow = np.repeat(np.arange(ns), np.diff(rpt))
    nd = rstat.shape[0]
    x, y, z = rstat[colt, :, 0], rstat[colt, :, 1], rstat[colt, :, 2]        # [nnz, K]
    ss = s_src[srow] * LOG2E
    raw2 = x + ss
    alpha = np.exp2(np.where(raw2 > 0, raw2, 0.2 * raw2) - y)
    slope = np.where(raw2 > 0, 1.0, 0.2)
    Mc = np.zeros((ns, K))
    np.maximum.at(Mc, srow, np.abs(x) + np.abs(ss) + np.abs(y))
    flat = srow * nd + colt
    At, Bt, Zt = (np.stack([np.bincount(flat, weights=w[:, k], minlength=ns * nd).reshape(ns, nd)
                            for k in range(K)]) for w in (alpha, alpha * slope, alpha * slope * np.abs(z)))
    # sum_i B (P - z): z depends on the edge's destination only
    zd = rstat[:, :, 2].T                                                      # [K, nd]
    d, W = heads(dout, K), heads(Wh, K)                                        # [K, nd, Fh], [K, ns, Fh]
    P, aP = W @ d.transpose(0, 2, 1), np.abs(W) @ np.abs(d).transpose(0, 2, 1)  # [K, ns, nd]
    dWh, adWh = At @ d, At @ np.abs(d)
    dss = (Bt * (P - zd[:, None, :])).sum(2).T
    adss = ((Bt * aP).sum(2) + Zt.sum(2)).T
    degt = np.diff(rpt)[:, None].astype(np.float64)
    Fh = Wh.shape[1] // K
    b_dWh = np.repeat((3 * Mc + degt + 3) * U, Fh, axis=1) * unheads(adWh)
    b_dss = (3 * Mc + degt + math.log2(G) + 14) * U * adss
    return dict(dWh=unheads(dWh), dss=dss, b_dWh=b_dWh, b_dss=b_dss, margin=np.abs(raw2) / np.maximum(np.abs(x) + np.abs(ss), 1e-30))


# ------------------------------------------------------------------ builders: exact tier
def exact_fwd_case(K, Fh, wbf, mode):
    """mode 'zero': s_src = 0; 'const': a per-head constant s_src, arbitrary s_dst.  Returns the
    inputs and the mirrored outputs."""
    L = lanes_of(K, Fh)
    g = graph(L)
    rng = np.random.default_rng(10 * K + Fh + (1 if mode == "zero" else 2))
    HF = K * Fh
    Wh = dyadic(rng, (N_SRC, HF), 8, 4)
    assert np.array_equal(store(Wh, wbf), Wh)
    s_dst = rng.standard_normal((g["n"], K)) * 3
    c = np.zeros(K) if mode == "zero" else f32(np.where(np.arange(K) % 2 == 0, 1.5, -1.25) + 0.01 * np.arange(K))
    s_src = np.tile(c, (N_SRC, 1))
    s_dst = f32(np.where(np.abs(s_dst + c) < 1e-2, s_dst + 0.05, s_dst))   # no raw score at the kink
    raw = s_dst + c                                                # per (row, head)
    assert (raw > 0).any() and (raw < 0).any() and np.abs(raw).min() > 1e-3
    A = dense(g, np.ones((g["nnz"], K)))
    S, aS = A @ heads(Wh, K), A @ np.abs(heads(Wh, K))
    assert aS.max() * 8 < 2 ** 24 and np.array_equal(S * 8, np.round(S * 8))
    deg = g["deg"].astype(np.float64)
    inv = f32(1.0 / np.where(deg > 0, deg, 1)) * (deg > 0)
    out = unheads(f32(S * inv[None, :, None]))
    e = np.where(raw > 0, raw, 0.2 * raw)
    lse = np.where(deg[:, None] > 0, e + np.log(np.where(deg > 0, deg, 1))[:, None], 0.0)
    M = (np.abs(s_dst) + np.abs(c)) * LOG2E
    b_lse = U * (4 * M + 2 * np.log2(deg + 1)[:, None] + 4 * np.abs(lse) + 6)
    return dict(g=g, L=L, Wh=Wh, s_src=s_src, s_dst=s_dst, out=out, lse=lse, b_lse=b_lse,
                pos=np.repeat(raw > 0, Fh, axis=1), deg=deg)


def exact_rows_case(K, Fh, wbf, n=55):
    rng = np.random.default_rng(20 * K + Fh)
    HF = K * Fh
    out, q, dout = (dyadic(rng, (n, HF), 4, 2) for _ in range(3))
    lse, s_dst = f32(rng.standard_normal((n, K)) * 4), f32(rng.standard_normal((n + 9, K)) * 4)
    assert np.array_equal(store(q, wbf), q) and np.array_equal(store(dout, wbf), dout)
    r = rows_ref(dout, out, q, lse, s_dst[:n], K)
    assert max(r["aD"].max(), r["adq"].max()) * 16 < 2 ** 24
    dsd = f32(float(np.float32(-0.8)) * r["dq"])
    return dict(out=out, q=q, dout=dout, lse=lse, s_dst=s_dst, D=r["D"], dsd=dsd, x=r["x"], y=r["y"])


def exact_cols_case(K, Fh, wbf, rpt, colt, n_dst):
    rng = np.random.default_rng(30 * K + Fh)
    HF, ns = K * Fh, len(rpt) - 1
    Wh, dout = dyadic(rng, (ns, HF), 2, 1), dyadic(rng, (n_dst, HF), 2, 1)
    assert np.array_equal(store(Wh, wbf), Wh)
    rstat = np.zeros((n_dst, K, 4))
    rstat[:, :, 0] = f32(rng.uniform(0.5, 3.0, (n_dst, K)))
    rstat[:, :, 1] = rstat[:, :, 0]                                # leaky2(x) = x in fp32 for x > 0
    rstat[:, :, 2] = dyadic(rng, (n_dst, K), 4, 1)
    srow = np.repeat(np.arange(ns), np.diff(rpt))
    flat = srow * n_dst + colt
    A = np.bincount(flat, minlength=ns * n_dst).reshape(ns, n_dst).astype(np.float64)
    d, W = heads(dout, K), heads(Wh, K)
    dWh = A @ d
    P = W @ d.transpose(0, 2, 1)
    zd = rstat[:, :, 2].T
    dss = (A * (P - zd[:, None, :])).sum(2).T
    budget = (A * (np.abs(W) @ np.abs(d).transpose(0, 2, 1) + np.abs(zd)[:, None, :])).sum(2)
    assert budget.max() * 4 < 2 ** 24 and (A @ np.abs(d)).max() * 2 < 2 ** 24
    return dict(Wh=Wh, dout=dout, rstat=rstat, s_src=np.zeros((ns, K)), dWh=unheads(dWh), dss=dss)


# ------------------------------------------------------------------ builders: bounded tier
def bounded_case(K, Fh, wbf, pattern):
    """Random inputs; s_dst on the grid 2^-10 Z, s_src on 2^-10 (Z + 1/2): no raw score is closer
    to 0 than 2^-11, far more than the error of the kernel's fp32 score (3 u M <= 2^-13)."""
    L = lanes_of(K, Fh)
    g = graph(L, pattern if pattern in ("asc", "desc") else None)
    rng = np.random.default_rng(10007 * K + 101 * Fh + PATTERNS.index(pattern))
    n = g["n"]
    if pattern == "normal3":
        sd, ss = rng.standard_normal((n, K)) * 3, rng.standard_normal((N_SRC, K)) * 3
    elif pattern in ("asc", "desc"):
        sd = rng.standard_normal((n, K))
        ss = (RANK[:, None] / N_SRC * 12 - 6) * rng.uniform(0.5, 1.0, K)[None, :]
    elif pattern in ("plus120", "minus120"):
        sign = 1 if pattern == "plus120" else -1
        sd, ss = sign * 120 + rng.standard_normal((n, K)), rng.standard_normal((N_SRC, K)) * 2
    else:
        sd, ss = rng.standard_normal((n, K)), rng.standard_normal((N_SRC, K))
    s_dst = np.round(sd * 1024) / 1024
    s_src = (np.round(ss * 1024) + 0.5) / 1024
    assert np.array_equal(f32(s_dst), s_dst) and np.array_equal(f32(s_src), s_src)
    Wh = store(rng.standard_normal((N_SRC, K * Fh)), wbf)
    dout = store(rng.standard_normal((n, K * Fh)), wbf)
    ref = forward_ref(g, Wh, s_src, s_dst, K)
    assert np.abs(ref["raw"]).min() >= 2.0 ** -11 and ref["M"].max() * 3 * U <= 2.0 ** -13
    if pattern == "asc":
        assert all(np.all(np.diff(ref["raw"][g["rp"][i]:g["rp"][i + 1]], axis=0) >= 0) for i in range(n))
    if pattern == "desc":
        assert all(np.all(np.diff(ref["raw"][g["rp"][i]:g["rp"][i + 1]], axis=0) <= 0) for i in range(n))
    if pattern == "plus120":
        assert ref["raw"].min() > 88.8                      # exp overflows fp32 unshifted
    if pattern == "straddle":
        both = [(ref["raw"][g["rp"][i]:g["rp"][i + 1]] > 0).any(0) & (ref["raw"][g["rp"][i]:g["rp"][i + 1]] < 0).any(0)
                for i in range(n) if g["deg"][i] >= 8]
        assert np.mean(both) > 0.5 and np.abs(ref["q"]).max() > 0.1     # most (row, head) see both sides
    return dict(g=g, L=L, Wh=Wh, s_src=s_src, s_dst=s_dst, dout=dout, ref=ref)


def edge_ds_dst(g, c, K):
    """The per-edge fp64 sum d s_dst[i, k] = sum_j alpha_ij (<dout_i, Wh_j> - D_i) LeakyReLU', and
    its sum of |terms| (the sum cancels -- to 0 where a row has no edge on the 0.2 side -- so the
    fp64 result itself carries an error of up to nnz 2^-53 of that)."""
    ref = c["ref"]
    slope = np.where(ref["raw"] > 0, 1.0, 0.2)
    B = dense(g, ref["alpha"] * slope)
    d, W, o = heads(c["dout"], K), heads(c["Wh"], K), heads(ref["out"], K)
    P = d @ W.transpose(0, 2, 1)                                   # [K, n, N_SRC]
    D = (d * o).sum(2)
    mag = (B * (np.abs(d) @ np.abs(W).transpose(0, 2, 1) + np.abs(D)[:, :, None])).sum(2).T
    return (B * (P - D[:, :, None])).sum(2).T, mag


# ------------------------------------------------------------------ device plumbing
def to_dev(x, dt=F32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(DEV)


def wdt(wbf):
    return BF16 if wbf else F32


def sent(shape, dt=F32):
    return torch.full(shape, SENT, dtype=dt, device=DEV)


def host(t):
    return t.detach().double().cpu().numpy()


def st():
    return torch.cuda.current_stream().cuda_stream


def run_fwd(g, Wh, s_src, s_dst, K, Fh, wbf, dst_rows=None, with_q=True, n=None, **kw):
    d = dev_graph(g)
    n = g["n"] if n is None else n
    HF = K * Fh
    out, lse = sent((n + 1, HF)), sent((n + 1, K))
    q = sent((n + 1, HF), wdt(wbf)) if with_q else None
    native.hip().gnn_gat_fwd(d["rp"].data_ptr(), d["col"].data_ptr(), Wh.data_ptr(), s_src.data_ptr(),
                             s_dst.data_ptr(), out.data_ptr(), lse.data_ptr(), n, K, Fh, st(), wbf,
                             dst_rows=dst_rows.data_ptr() if dst_rows is not None else 0,
                             q=q.data_ptr() if with_q else 0, **kw)
    torch.cuda.synchronize()
    for t in (out, lse) + ((q,) if with_q else ()):
        assert torch.all(t[n:] == SENT), "a row past n was written"
    return out[:n], lse[:n], (q[:n] if with_q else None)


def run_rows(dout, out, q, lse, s_dst, K, Fh, wbf, dst_rows=None, ds_rows=None, dy=None, act=0, ldh=0, **kw):
    n = out.shape[0]
    rstat = sent((n + 1, K, 4))
    ds_dst = ds_rows if ds_rows is not None else sent((n + 1, K))
    base = dict(dout_w=0, bias=0, bpart=0, db=0, p=0.0, k0=0, k1=0, step=0, stepp=0, row0=0)
    base.update(kw)
    native.hip().gnn_gat_rows(act, dout.data_ptr(), ldh, out.data_ptr(), q.data_ptr(), lse.data_ptr(),
                              s_dst.data_ptr(), dst_rows.data_ptr() if dst_rows is not None else 0, rstat.data_ptr(),
                              ds_dst.data_ptr(), dy.data_ptr() if dy is not None else 0,
                              dy.stride(0) if dy is not None else 0, n=n, K=K, Fh=Fh, wbf=wbf, st=st(), **base)
    torch.cuda.synchronize()
    assert torch.all(rstat[n:] == SENT)
    return rstat[:n], ds_dst


def run_cols(rpt, colt, Wh, s_src, rstat, dout, K, Fh, wbf, ldy=0):
    ns = rpt.numel() - 1
    HF = K * Fh
    dWh, dss = sent((ns + 1, HF)), sent((ns + 1, K))
    dy = sent((ns + 1, ldy), BF16) if ldy else None
    native.hip().gnn_gat_col(rpt.data_ptr(), colt.data_ptr(), Wh.data_ptr(), s_src.data_ptr(), rstat.data_ptr(),
                             dout.data_ptr(), 0 if ldy else dWh.data_ptr(), 0 if ldy else dss.data_ptr(),
                             dy.data_ptr() if ldy else 0, ldy, ns, K, Fh, st(), wbf)
    torch.cuda.synchronize()
    if ldy:
        assert torch.all(dy[ns:] == SENT) and torch.all(dy[:, HF + K:] == SENT), "dy outside [0, HF + K) was written"
        return dy[:ns, :HF], dy[:ns, HF:HF + K]
    assert torch.all(dWh[ns:] == SENT) and torch.all(dss[ns:] == SENT)
    return dWh[:ns], dss[:ns]


def ratio(got, ref, bound, what, worst):
    """Largest |got - ref| / bound; a zero bound demands equality."""
    err = np.abs(got - ref)
    assert np.all(err[bound == 0] == 0), what + ": nonzero where the bound is 0"
    r = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    worst[what] = max(worst.get(what, 0.0), r)
    return r


# ------------------------------------------------------------------ 1. variants
def test_the_cases_reach_every_compiled_variant():
    hip = native.hip()
    assert len(TABLE) == 22 and {c for _, _, c in SHAPES} == TABLE and FORMERLY_MISSING < TABLE
    for K, Fh, code in SHAPES:
        assert rule(K, Fh) and hip.gnn_gat_variant(K, Fh) == code == expected_variant(K, Fh), (K, Fh)
    assert {Fh for K, Fh, _ in SHAPES if K == 1} >= {24, 40, 176} and {3, 5} <= {K for K, _, _ in SHAPES}


# ------------------------------------------------------------------ 2. exact tier
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_bit_for_bit_on_equal_scores(case):
    K, Fh, wbf = case
    assert native.hip().gnn_gat_variant(K, Fh) == CODE[(K, Fh)]
    for mode in ("zero", "const"):
        c = exact_fwd_case(K, Fh, wbf, mode)
        g = c["g"]
        out, lse, q = run_fwd(g, to_dev(c["Wh"], wdt(wbf)), to_dev(c["s_src"]), to_dev(c["s_dst"]), K, Fh, wbf)
        out, lse, q = host(out), host(lse), host(q)
        bad = np.flatnonzero((out != c["out"]).any(1))
        assert bad.size == 0, "%s: out differs in rows %s (degrees %s)" % (mode, bad[:8], g["deg"][bad[:8]])
        empty = g["deg"] == 0
        assert np.all(out[empty] == 0) and np.all(lse[empty] == 0) and np.all(q[empty] == 0)
        assert np.all(np.abs(lse - c["lse"]) <= c["b_lse"]), mode + ": lse"
        assert np.all(q[c["pos"]] == 0), mode + ": q on the positive side"
        assert np.all(np.abs(q) <= 4 * U * np.abs(out) * (1 + 2.0 ** -7)), mode + ": q on the 0.2-slope side"
        # without q: the same out / lse
        out2, lse2, _ = run_fwd(g, to_dev(c["Wh"], wdt(wbf)), to_dev(c["s_src"]), to_dev(c["s_dst"]), K, Fh, wbf,
                                with_q=False)
        assert np.array_equal(host(out2), out) and np.array_equal(host(lse2), lse)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_row_half_bit_for_bit_on_dyadic_values(case):
    K, Fh, wbf = case
    HF = K * Fh
    c = exact_rows_case(K, Fh, wbf)
    n = c["out"].shape[0]
    ldy = (HF + 2 * K + 7) // 8 * 8 + 8
    dy = sent((n + 1, ldy), BF16)
    rstat, ds_dst = run_rows(to_dev(c["dout"], wdt(wbf)), to_dev(c["out"]), to_dev(c["q"], wdt(wbf)), to_dev(c["lse"]),
                             to_dev(c["s_dst"]), K, Fh, wbf, dy=dy)
    rs = host(rstat)
    assert np.array_equal(rs[:, :, 2], c["D"]), "D"
    assert np.array_equal(rs[:, :, 0], c["x"]) and np.array_equal(rs[:, :, 1], c["y"]) and np.all(rs[:, :, 3] == 0)
    assert np.array_equal(host(ds_dst[:n]), c["dsd"]) and torch.all(ds_dst[n:] == SENT)
    dyh = host(dy)
    assert np.array_equal(dyh[:n, HF + K:HF + 2 * K], bf16r(c["dsd"])), "dy column HF + K + k"
    dyh[:n, HF + K:HF + 2 * K] = SENT
    assert np.all(dyh == SENT), "dy outside column HF + K + k was written"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_column_half_bit_for_bit_with_unit_weights(case):
    K, Fh, wbf = case
    HF = K * Fh
    L = lanes_of(K, Fh)
    g = graph(L)
    # the true transpose (257 source rows, 55 destinations), and the degree list as the
    # transposed CSR (55 source rows of the exact lengths, 257 destinations)
    for rpt, colt, nd in ((g["rpt"], g["colt"], g["n"]), (g["rp"], g["col"], N_SRC)):
        c = exact_cols_case(K, Fh, wbf, rpt, colt, nd)
        args = (to_dev(rpt, torch.int32), to_dev(colt, torch.int32), to_dev(c["Wh"], wdt(wbf)), to_dev(c["s_src"]),
                to_dev(c["rstat"].reshape(nd, K * 4)), to_dev(c["dout"], wdt(wbf)), K, Fh, wbf)
        dWh, dss = run_cols(*args)
        assert np.array_equal(host(dWh), c["dWh"]), "dWh"
        assert np.array_equal(host(dss), c["dss"]), "ds_src"
        dWb, dsb = run_cols(*args, ldy=(HF + 2 * K + 7) // 8 * 8 + 8)
        assert np.array_equal(host(dWb), bf16r(c["dWh"])) and np.array_equal(host(dsb), bf16r(c["dss"])), "dy"


@pytest.mark.parametrize("K,HF,ldy", [(1, 32, 40), (3, 24, 32), (4, 32, 40), (4, 28, 36), (3, 20, 64), (1, 4, 8)])
def test_pack_grad_is_bf16_of_the_concatenation(K, HF, ldy):
    from cgnn_amd.gnn.gat_fused import pack_grad
    n = 37
    rng = np.random.default_rng(K + HF)
    dWh, dss, dsd = (f32(rng.standard_normal((n, w)) * 3) for w in (HF, K, K))
    dy = sent((n + 3, ldy), BF16)
    pack_grad(to_dev(dWh), to_dev(dss), to_dev(dsd), dy[:n])
    torch.cuda.synchronize()
    got = host(dy)
    exp = np.zeros((n, ldy))
    exp[:, :HF + 2 * K] = bf16r(np.concatenate([dWh, dss, dsd], 1))
    assert np.array_equal(got[:n], exp) and np.all(got[n:] == SENT)


# ------------------------------------------------------------------ 3. bounded tier
WORST = {}


def _patterns_of(K, Fh):
    if (K, Fh) in ALL_PATTERNS:
        return PATTERNS
    return (PATTERNS[[s[:2] for s in SHAPES].index((K, Fh)) % len(PATTERNS)],)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_and_backward_within_the_derived_bounds_of_fp64(case):
    K, Fh, wbf = case
    G = CODE[(K, Fh)] % 100
    worst = {}
    for pattern in _patterns_of(K, Fh):
        c = bounded_case(K, Fh, wbf, pattern)
        g, ref = c["g"], c["ref"]
        d = dev_graph(g)
        Wh, s_src, s_dst = to_dev(c["Wh"], wdt(wbf)), to_dev(c["s_src"]), to_dev(c["s_dst"])
        out, lse, q = run_fwd(g, Wh, s_src, s_dst, K, Fh, wbf)
        b_out, b_lse, b_q = forward_bounds(g, ref, K, wbf)
        oh, lh, qh = host(out), host(lse), host(q)
        assert np.all(np.isfinite(oh)) and np.all(np.isfinite(lh)) and np.all(np.isfinite(qh)), pattern
        r = [ratio(oh, ref["out"], b_out, "out", worst), ratio(lh, ref["lse"], b_lse, "lse", worst),
             ratio(qh, ref["q"], b_q, "q", worst)]
        # the row half, from the kernel's own stored out / q / lse
        dout = to_dev(c["dout"], wdt(wbf))
        rstat, ds_dst = run_rows(dout, out, q, lse, s_dst, K, Fh, wbf)
        rr = rows_ref(c["dout"], oh, qh, lh, c["s_dst"], K)
        rs = host(rstat)
        assert np.array_equal(rs[:, :, 0], rr["x"]) and np.array_equal(rs[:, :, 1], rr["y"])
        cd = (9 + math.log2(G)) * U
        r.append(ratio(rs[:, :, 2], rr["D"], cd * rr["aD"], "rstat.z", worst))
        dsd = host(ds_dst[:g["n"]])
        b_own = (11 + math.log2(G)) * U * 0.8 * rr["adq"]
        r.append(ratio(dsd, -0.8 * rr["dq"], b_own, "ds_dst", worst))
        # the identity ds_dst = -0.8 <dout, q> against the per-edge fp64 sum
        b_id = b_own + 0.8 * (np.abs(heads(c["dout"], K)) * heads(b_q, K)).sum(2).T
        per_edge, mag = edge_ds_dst(g, c, K)
        r.append(ratio(dsd, per_edge, b_id + 2.0 ** -40 * mag, "ds_dst (per edge)", worst))
        # the column half, from the kernel's own stored rstat
        cr = cols_ref(g["rpt"], g["colt"], c["Wh"], c["s_src"], rs, c["dout"], K, G)
        assert cr["margin"].min() > 8 * U                      # the slope side of fl(x + ss) is the reference's
        dWh, dss = run_cols(d["rpt"], d["colt"], Wh, s_src, rstat, dout, K, Fh, wbf)
        r.append(ratio(host(dWh), cr["dWh"], cr["b_dWh"], "dWh", worst))
        r.append(ratio(host(dss), cr["dss"], cr["b_dss"], "ds_src", worst))
        print("%s %s: error / bound  out %.3f lse %.3f q %.3f rstat.z %.3f ds_dst %.3f per-edge %.3f dWh %.3f "
              "ds_src %.3f" % (_id(case), pattern, *r))
    for k, v in worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("largest error / bound so far: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


# ------------------------------------------------------------------ 4. paths
def _wrapper_graph(g):
    from cgnn_amd.gnn.gat import GraphCSR
    d = dev_graph(g)
    G = GraphCSR(d["rp"], d["col"], g["n"], N_SRC)
    G._t = (d["rpt"], d["colt"])
    return G


@pytest.mark.parametrize("case", [(3, 16, 1), (3, 32, 0), (8, 32, 1), (5, 64, 1), (1, 280, 0)], ids=_id)
def test_dst_rows_gathers_s_dst_and_scatters_ds_dst(case):
    from cgnn_amd.gnn.gat_fused import _agg_fwd
    K, Fh, wbf = case
    HF = K * Fh
    c = bounded_case(K, Fh, wbf, "normal3")
    g = c["g"]
    n, tall = g["n"], g["n"] + 40
    rng = np.random.default_rng(5)
    idx = rng.permutation(tall)[:n].astype(np.int32)
    s_tall = f32(rng.standard_normal((tall, K)))
    s_tall[idx] = c["s_dst"]
    Wh, s_src = to_dev(c["Wh"], wdt(wbf)), to_dev(c["s_src"])
    plain = run_fwd(g, Wh, s_src, to_dev(c["s_dst"]), K, Fh, wbf)
    rows = to_dev(idx, torch.int32)
    via = run_fwd(g, Wh, s_src, to_dev(s_tall), K, Fh, wbf, dst_rows=rows)
    for a, b in zip(plain, via):
        assert torch.equal(a, b)
    qw = sent((n, HF), wdt(wbf))
    out_w, lse_w = _agg_fwd(Wh, s_src, to_dev(s_tall), _wrapper_graph(g), K, Fh, dst_rows=rows, q=qw)
    assert torch.equal(out_w, plain[0]) and torch.equal(lse_w, plain[1]) and torch.equal(qw, plain[2])
    # the row half: rstat in launch order, ds_dst / dy at dst_rows[i] only
    dout = to_dev(c["dout"], wdt(wbf))
    out, lse, q = plain
    rs0, ds0 = run_rows(dout, out, q, lse, to_dev(c["s_dst"]), K, Fh, wbf)
    ldy = (HF + 2 * K + 7) // 8 * 8
    dy = sent((tall, ldy), BF16)
    ds = sent((tall, K))
    rs1, _ = run_rows(dout, out, q, lse, to_dev(s_tall), K, Fh, wbf, dst_rows=rows, ds_rows=ds, dy=dy)
    assert torch.equal(rs0, rs1)
    exp = sent((tall, K))
    exp[rows.long()] = ds0[:n]
    assert torch.equal(ds, exp)
    expy = sent((tall, ldy), BF16)
    expy[rows.long(), HF + K:HF + 2 * K] = ds0[:n].to(BF16)
    assert torch.equal(dy, expy)


@pytest.mark.parametrize("case", [(3, 8, 1), (13, 8, 1), (8, 32, 1), (2, 256, 1)], ids=_id)
def test_agg_cols_row_range_is_the_slice_of_the_full_call(case):
    from cgnn_amd.gnn.gat_fused import _agg_cols
    K, Fh, wbf = case
    HF = K * Fh
    c = bounded_case(K, Fh, wbf, "straddle")
    g = c["g"]
    G = _wrapper_graph(g)
    Wh, s_src, s_dst, dout = to_dev(c["Wh"], BF16), to_dev(c["s_src"]), to_dev(c["s_dst"]), to_dev(c["dout"], BF16)
    out, lse, q = run_fwd(g, Wh, s_src, s_dst, K, Fh, 1)
    rstat, _ = run_rows(dout, out, q, lse, s_dst, K, Fh, 1)
    fW, fs = sent((N_SRC, HF)), sent((N_SRC, K))
    _agg_cols(Wh, s_src, rstat, dout, G, K, Fh, 0, N_SRC, dWh=fW, ds_src=fs)
    ldy = (HF + 2 * K + 7) // 8 * 8
    fy = sent((N_SRC, ldy), BF16)
    _agg_cols(Wh, s_src, rstat, dout, G, K, Fh, 0, N_SRC, dy=fy)
    torch.cuda.synchronize()
    assert torch.equal(fy[:, :HF + K], torch.cat([fW, fs], 1).to(BF16)) and torch.all(fy[:, HF + K:] == SENT)
    for lo, hi in ((0, 1), (1, 100), (100, 100), (100, 256), (256, 257), (31, 33)):
        pW, ps = sent((hi - lo + 1, HF)), sent((hi - lo + 1, K))
        _agg_cols(Wh, s_src, rstat, dout, G, K, Fh, lo, hi, dWh=pW, ds_src=ps)
        py = sent((N_SRC, ldy), BF16)
        _agg_cols(Wh, s_src, rstat, dout, G, K, Fh, lo, hi, dy=py)
        torch.cuda.synchronize()
        assert torch.equal(pW[:hi - lo], fW[lo:hi]) and torch.equal(ps[:hi - lo], fs[lo:hi]), (lo, hi)
        assert torch.all(pW[hi - lo:] == SENT) and torch.all(ps[hi - lo:] == SENT)
        ey = sent((N_SRC, ldy), BF16)
        ey[lo:hi] = fy[lo:hi]
        assert torch.equal(py, ey), (lo, hi)


@pytest.mark.parametrize("case", [(3, 16, 1), (5, 16, 0), (8, 32, 1), (21, 16, 0), (1, 280, 1)], ids=_id)
def test_a_rows_bits_do_not_depend_on_its_position_or_launch_mates(case):
    K, Fh, wbf = case
    c = bounded_case(K, Fh, wbf, "normal3")
    g = c["g"]
    gr = graph(c["L"], None, True)
    n = g["n"]
    Wh, s_src = to_dev(c["Wh"], wdt(wbf)), to_dev(c["s_src"])
    a = run_fwd(g, Wh, s_src, to_dev(c["s_dst"]), K, Fh, wbf)
    b = run_fwd(gr, Wh, s_src, to_dev(c["s_dst"][::-1].copy()), K, Fh, wbf)
    for x, y in zip(a, b):
        assert torch.equal(x, y.flip(0))
    a2 = run_fwd(g, Wh, s_src, to_dev(c["s_dst"]), K, Fh, wbf)
    assert all(torch.equal(x, y) for x, y in zip(a, a2))
    # the row half (the column half sums a source's destinations in their order, which the
    # renumbering reverses: its position independence is the row range test)
    dout = to_dev(c["dout"], wdt(wbf))
    out, lse, q = a
    r0, d0 = run_rows(dout, out, q, lse, to_dev(c["s_dst"]), K, Fh, wbf)
    r1, d1 = run_rows(*(t.flip(0).contiguous() for t in (dout, out, q, lse)), to_dev(c["s_dst"][::-1].copy()), K, Fh,
                      wbf)
    assert torch.equal(r0, r1.flip(0)) and torch.equal(d0[:n], d1[:n].flip(0))


def _elu(z):
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0)))


@pytest.mark.parametrize("K,Fh,row0,p,by_ptr,wbf", [(1, 32, 0, 0.0, False, 1), (3, 32, 7, 0.3, True, 1),
                                                   (16, 32, 70001, 0.5, False, 1), (3, 32, 70001, 0.5, True, 0),
                                                   (16, 32, 7, 0.3, False, 0), (1, 32, 7, 0.5, True, 0)])
def test_fused_activation_forward_and_backward(K, Fh, row0, p, by_ptr, wbf):
    """H = bf16(dropout(elu(out + bias))): z = fl(out + b), or fused with the final multiply of out
    (2 u (|out| + |b|) absolute; elu is 1-Lipschitz), expm1f (a few ulp: 4 u), the scale fl(1 / (1 - p))
    and its multiply (2 u): 8 u relative to the fp64 value of the kernel's own out, plus one bf16 ulp
    (2^-7).  Backward: dout = dH scale elu'(z), elu' by the fast exponential:
    (6 + 2 |z|) u, plus one bf16 ulp where dout is stored bf16."""
    from cgnn_amd.gnn import ops
    HF = K * Fh
    c = bounded_case(K, Fh, wbf, "straddle")
    g = c["g"]
    n = g["n"]
    rng = np.random.default_rng(row0 + K)
    bias = f32(rng.standard_normal(HF) * 0.5)
    key, step = (0x1234, 0x9876), 41
    stepp = torch.tensor([step], dtype=torch.int32, device=DEV)
    skw = dict(step=0, stepp=stepp.data_ptr()) if by_ptr else dict(step=step, stepp=0)
    ldh = HF + 8
    H = sent((n + 1, ldh), BF16)
    Wh, s_src, s_dst, bd = to_dev(c["Wh"], wdt(wbf)), to_dev(c["s_src"]), to_dev(c["s_dst"]), to_dev(bias)
    out, lse, q = run_fwd(g, Wh, s_src, s_dst, K, Fh, wbf, bias=bd.data_ptr(), H=H.data_ptr(), ldh=ldh, p=p,
                          k0=key[0], k1=key[1], row0=row0, **skw)
    plain = run_fwd(g, Wh, s_src, s_dst, K, Fh, wbf)
    assert torch.equal(out, plain[0]) and torch.equal(lse, plain[1]) and torch.equal(q, plain[2])
    assert torch.all(H[n:] == SENT) and torch.all(H[:, HF:] == SENT)
    keep = ops.dropout_keep_mask(n, HF, p, key, step, row0).numpy()
    z = host(out) + bias
    scale = 1.0 / (1.0 - p) if p > 0 else 1.0
    hv = host(H[:n, :HF])
    e = _elu(z) * scale
    nz = np.abs(e) > 1e-30
    assert np.array_equal((hv != 0)[nz], keep[nz]) and np.all(hv[~keep] == 0), "dropout pattern of H"
    tol = np.abs(e) * (2.0 ** -7 + 8 * U) + 2 * U * scale * (np.abs(host(out)) + np.abs(bias)[None, :])
    assert np.all(np.abs(hv - e)[keep] <= tol[keep]), "H"
    # backward
    dH = sent((n, ldh), BF16)
    dHv = bf16r(rng.standard_normal((n, HF)))
    dH[:, :HF] = to_dev(dHv, BF16)
    dout_w = sent((n + 1, HF), wdt(wbf))
    bpart = torch.empty(native.hip().gnn_gat_row_blocks(), HF, device=DEV)
    db = sent((HF + 3,))
    rstat, ds_dst = run_rows(dH, out, q, lse, s_dst, K, Fh, wbf, act=1, ldh=ldh, dout_w=dout_w.data_ptr(),
                             bias=bd.data_ptr(), bpart=bpart.data_ptr(), db=db.data_ptr(), p=p, k0=key[0], k1=key[1],
                             row0=row0, **skw)
    assert torch.all(dout_w[n:] == SENT) and torch.all(db[HF:] == SENT)
    dw = host(dout_w[:n])
    dref = dHv * scale * np.where(z > 0, 1.0, np.exp(np.minimum(z, 0)))
    nz = np.abs(dref) > 1e-30
    assert np.array_equal((dw != 0)[nz], keep[nz]) and np.all(dw[~keep] == 0), "dropout pattern of dout"
    tol = np.abs(dref) * ((6 + 2 * np.abs(z)) * U + (2.0 ** -7 if wbf else 0))
    assert np.all(np.abs(dw - dref)[keep] <= tol[keep])
    asum = np.abs(dw).sum(0)
    assert np.all(np.abs(host(db[:HF]) - dw.sum(0)) <= n * U * asum + (2.0 ** -8 * asum if wbf else 0)), "db"
    # the row half ran on the stored (rounded) dout
    G = expected_variant(K, Fh) % 100
    rr = rows_ref(dw, host(out), host(q), host(lse), c["s_dst"], K)
    rs = host(rstat)
    assert np.all(np.abs(rs[:, :, 2] - rr["D"]) <= (9 + math.log2(G)) * U * rr["aD"]), "rstat.z"
    assert np.all(np.abs(host(ds_dst[:n]) + 0.8 * rr["dq"]) <= (11 + math.log2(G)) * U * 0.8 * rr["adq"])


# ------------------------------------------------------------------ 5. row_ce
def ru8(x):
    return (x + 7) // 8 * 8


def row_ce_case(C, n, ldz, seed=0):
    rng = np.random.default_rng(C * 131 + n + seed)
    Z = f32(rng.standard_normal((n, C)) * 2)
    bias = f32(rng.standard_normal(C))
    y = rng.integers(0, C, n)
    y[0], y[-1] = 0, C - 1
    mask = rng.integers(0, 5, n)
    mask[:min(n, 3)] = 1
    z = Z + bias                                        # fp64 of fp32 values; the kernel rounds the sum once
    return dict(Z=Z, bias=bias, y=y.astype(np.int32), mask=mask.astype(np.uint8), z=f32(z))


def row_ce_ref(c, inv_count):
    z, y, mask = c["z"], c["y"], c["mask"]
    n, C = z.shape
    mx = z.max(1)
    lse = mx + np.log(np.exp(z - mx[:, None]).sum(1))
    arg = z.argmax(1)                                   # numpy: the first maximum
    ok = arg == y
    nll = lse - z[np.arange(n), y]
    tr = mask == 1
    stats = np.array([nll[tr].sum(), (ok & tr).sum(), (ok & (mask == 2)).sum(), (ok & (mask == 3)).sum()])
    d = np.exp(z - lse[:, None])
    d[np.arange(n), y] -= 1.0
    d = d * inv_count * tr[:, None]
    return stats, d, nll, np.abs(z).max(1)


CE_C = (1, 7, 63, 64, 65, 128, 129, 192, 193, 256)


@pytest.mark.parametrize("C", CE_C)
def test_row_ce_against_fp64(C):
    """z = fl(Z + b) is mirrored (one rounding); Zm = 2 max |z| >= max |z - mx|, u = 2^-24.
    lse = mx + log(s), s = sum exp(z - mx), fast exp / log (v_exp_f32 / v_log_f32 and a multiply):
    a term (2 + Zm) u relative, the sum of at most 4 slots and 6 butterfly steps 10 u, the log
    2 u |log2 s| ln2 + u |ln s| <= 17 u (s <= 256) plus the relative error of s, the add u |lse|:
    |lse - lse*| <= (Zm + 30 + |lse|) u with |lse| <= max |z| + ln C; the NLL adds u |nll|.
    p = exp(z - lse): argument rounding u |z - lse| <= (Zm + ln C) u, the error of lse, the exp 2 u:
    relative (2 Zm + max |z| + 2 ln C + 32) u; the subtraction of the one-hot and the multiply by
    inv_count u each: |dZ - dZ*| <= (2 Zm + max |z| + 2 ln C + 34) u inv (p + onehot).
    The sums over rows (NLL, db) are chains of at most n additions and the fixed-order colsum:
    (n + 8) u sum |terms| on top."""
    from cgnn_amd.gnn.gat_fused import row_ce
    waves = native.hip().gnn_gat_row_ce_waves()
    inv = 1.0 / 3
    for n in (1, 5, waves + 3):
        for ldz in (ru8(C), 64 * ((C + 63) // 64) + 8, 64 * ((C + 63) // 64) + 72):
            c = row_ce_case(C, n, ldz)
            stats, d, nll, zmax = row_ce_ref(c, float(np.float32(inv)))
            Zd = sent((n, ldz))
            Zd[:, :C] = to_dev(c["Z"])
            bias, y, mask = to_dev(c["bias"]), to_dev(c["y"], torch.int32), to_dev(c["mask"], torch.uint8)
            dZ, dZb, db = sent((n + 1, ldz)), sent((n + 1, ldz), BF16), sent((C + 2,))
            got = row_ce(Zd, bias, C, y, mask, inv, dZ=dZ[:n], dZb=dZb[:n], db=db)
            torch.cuda.synchronize()
            what = "C=%d n=%d ldz=%d" % (C, n, ldz)
            gs = host(got)
            assert np.array_equal(gs[1:], stats[1:]), what + ": counts"
            tr = c["mask"] == 1
            Zm, lnC = 2 * zmax, math.log(C)
            b_nll = ((Zm + 30 + zmax + lnC + np.abs(nll)) * U)[tr]
            assert abs(gs[0] - stats[0]) <= b_nll.sum() + (n + 8) * U * np.abs(nll[tr]).sum(), what + ": NLL"
            dz = host(dZ)
            assert np.all(dz[n:] == SENT) and np.all(dz[:n, C:] == 0) and np.all(dz[:n][~tr] == 0), what + ": zeros"
            onehot = np.zeros_like(d)
            onehot[np.arange(n), c["y"]] = inv
            b_d = ((2 * Zm + zmax + 2 * lnC + 34) * U)[:, None] * (np.abs(d + onehot * tr[:, None]) + onehot)
            assert np.all(np.abs(dz[:n, :C] - d) <= b_d), what + ": dZ"
            assert torch.equal(dZb[:n], dZ[:n].to(BF16)) and torch.all(dZb[n:] == SENT), what + ": dZb"
            dbh = host(db)
            assert np.all(dbh[C:] == SENT)
            assert np.all(np.abs(dbh[:C] - dz[:n, :C].sum(0)) <= (n + 8) * U * np.abs(dz[:n, :C]).sum(0)), what + ": db"
            # evaluation: no dZ -- identical statistics
            ev = row_ce(Zd, bias, C, y, mask, inv)
            assert torch.equal(ev, got), what + ": evaluation call"


def test_row_ce_argmax_ties_go_to_the_lowest_index():
    from cgnn_amd.gnn.gat_fused import row_ce
    C, ldz = 200, 200
    ties = [(3, 67), (67, 130), (3, 130), (3, 67, 130), (5, 6), (64, 128, 192), (199, 7), (0, 199)]
    n = len(ties)
    Z = np.zeros((n, ldz))
    Z[:, :] = np.random.default_rng(0).standard_normal((n, ldz)).astype(np.float32)
    for r, t in enumerate(ties):
        Z[r, list(t)] = 9.0
    for pick in (min, max):
        y = np.array([pick(t) for t in ties], dtype=np.int32)
        for m in (1, 2, 3):
            got = row_ce(to_dev(Z), to_dev(np.zeros(C)), C, to_dev(y, torch.int32),
                         to_dev(np.full(n, m), torch.uint8), 1.0)
            torch.cuda.synchronize()
            assert float(got[m]) == (n if pick is min else 0), (pick, m)
            assert sum(float(got[k]) for k in (1, 2, 3) if k != m) == 0
    got = row_ce(to_dev(Z), to_dev(np.zeros(C)), C, to_dev(y, torch.int32), to_dev(np.full(n, 4), torch.uint8), 1.0)
    assert torch.all(got == 0)                                # a mask above 3 counts nowhere


# ------------------------------------------------------------------ 6. rejections
def test_every_refusal_raises_and_writes_nothing():
    hip = native.hip()
    g = graph(8)
    d = dev_graph(g)
    n = g["n"]
    buf = [sent((n, 1024)) for _ in range(4)]
    bb = sent((n, 1024), BF16)
    z = torch.zeros(N_SRC, 1024, device=DEV)
    P = lambda t: t.data_ptr()

    def fwd(K, Fh, n=n, **kw):
        hip.gnn_gat_fwd(P(d["rp"]), P(d["col"]), P(z), P(z), P(z), P(buf[0]), P(buf[1]), n, K, Fh, st(), 0,
                        q=P(buf[2]), **kw)

    def rows(K, Fh, act=0, n=n, dy=0, ldy=0, **kw):
        base = dict(dout_w=0, bias=0, bpart=0, db=0, p=0.0, k0=0, k1=0, step=0, stepp=0, row0=0)
        base.update(kw)
        hip.gnn_gat_rows(act, P(z), 1024, P(z), P(z), P(z), P(z), 0, P(buf[0]), P(buf[1]), dy, ldy, n=n, K=K, Fh=Fh,
                         wbf=0, st=st(), **base)

    def cols(K, Fh, n=N_SRC, dy=0, ldy=0):
        hip.gnn_gat_col(P(d["rpt"]), P(d["colt"]), P(z), P(z), P(z), P(z), P(buf[0]), P(buf[1]), dy, ldy, n, K, Fh,
                        st(), 0)

    shapes = [(2, 12), (1, 12), (3, 24), (2, 48), (1, 520), (2, 264), (65, 8), (0, 8), (1, 0)]
    for K, Fh in shapes:
        assert hip.gnn_gat_variant(K, Fh) == -3 and not (K >= 1 and Fh >= 8 and rule(K, Fh))
        for f in (fwd, rows, cols):
            with pytest.raises(RuntimeError, match=r"\(code -3\)"):
                f(K, Fh)
    bad_h = [dict(K=3, Fh=8, H=P(bb), ldh=32, bias=P(z)), dict(K=1, Fh=32, H=P(bb), ldh=24, bias=P(z)),
             dict(K=1, Fh=32, H=P(bb), ldh=32, bias=0)]
    for kw in bad_h:
        with pytest.raises(RuntimeError, match=r"gnn_gat_fwd.*\(code -3\)"):
            fwd(**kw)
    full = dict(dout_w=P(buf[2]), bias=P(z), bpart=P(buf[3]))
    for miss in ("dout_w", "bias", "bpart"):
        with pytest.raises(RuntimeError, match=r"gnn_gat_rows.*\(code -3\)"):
            rows(1, 32, act=1, **{k: (0 if k == miss else v) for k, v in full.items()})
    with pytest.raises(RuntimeError, match=r"\(code -3\)"):
        rows(3, 8, act=1, **full)                                  # HF % 32
    with pytest.raises(RuntimeError, match=r"gnn_gat_col.*\(code -3\)"):
        cols(2, 32, dy=P(bb), ldy=64 + 3)
    # row_ce and pack_grad shape rules
    for C, ldz in ((0, 8), (257, 264), (40, 32), (-1, 8)):
        with pytest.raises(RuntimeError, match=r"gnn_gat_row_ce.*\(code -3\)"):
            hip.gnn_gat_row_ce(P(z), ldz, P(z), C, P(d["rp"]), P(d["rp"]), 1.0, P(buf[0]), P(bb), P(buf[1]), P(buf[2]),
                               P(buf[3]), 0, 4, st())
    for HF, K, ldy in ((32, 2, 38), (30, 1, 32), (32, 2, 32), (32, 4, 36)):
        with pytest.raises(RuntimeError, match=r"gnn_gat_pack_grad.*\(code -3\)"):
            hip.gnn_gat_pack_grad(P(z), P(z), P(z), HF, K, P(bb), ldy, 4, st())
    # n = 0: nothing launched, code 0
    fwd(2, 32, n=0)
    cols(2, 32, n=0)
    rows(2, 32, n=0)
    hip.gnn_gat_pack_grad(P(z), P(z), P(z), 32, 2, P(bb), 40, 0, st())
    torch.cuda.synchronize()
    assert all(bool(torch.all(b == SENT)) for b in buf) and bool(torch.all(bb == SENT))
    # after the refusals the launchers still work
    fwd(2, 32)
    torch.cuda.synchronize()
    assert bool(torch.all(buf[0].view(-1)[:n * 64] == 0))
    # every pair the rule allows is compiled: -1 cannot be reached through the launchers
    assert all(hip.gnn_gat_variant(K, Fh) > 0 for K in range(1, 65) for Fh in range(8, 513, 8) if rule(K, Fh))
