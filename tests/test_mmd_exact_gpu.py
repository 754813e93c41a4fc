"""Per-partial fp64 oracle tests of the four MMD kernels, at every compiled width.

Kernels (raw bindings ``hip.mmd`` / ``hip.mmd_mfma``): the vector kernel
``mmd_rbf_kernel<D,MODE>`` ("valu"), the 32-row matrix-core kernel ``mmd_mfma_kernel``
("m32"), the 16-row one ``mmd_mfma16_kernel`` ("m16", KD 128..256) and the dimension-
grouped ``mmd_mfma16g_kernel`` ("m16g", KD > 256).  Every ``loss_part[r, chunk, row_block]``
and every ``grad_part[chunk, r, :, :]`` is compared with an fp64 reference of exactly that
partial, computed here from the definition.

Data -- a clustered lattice on which the squared distance is exact
-------------------------------------------------------------------
Every coordinate is a multiple of 1/4.  A sample is a cluster centre plus a per-dimension
shift ``u[d]`` in {0, 1/4, 1/2} shared by all samples (period 3, so that dimensions 8, 16 or
32 apart are not interchangeable) plus one of three offsets on one of four pairs of
dimensions of its cluster.  Two samples of one cluster are at ``d2`` in ALLOWED_D2; two
samples of different clusters at ``d2 >= 22 500``, where ``exp(-0.005 d2) <= e^-112.5 ~
1.4e-49`` is below the smallest fp32 denormal: the device computes an exact 0 for every such
pair and the reference sets those pairs to 0 (their fp64 sum is below 1e-40).  Cluster 0
sits at the origin; the far centres are ``+-160 k`` on one axis (fewer than 6 active
dimensions, vector kernel only) or ``m`` times a sign pattern (rows of +-H8, tiled), ``m``
the smallest multiple of 1/4 that separates every pair.  ``|x|^2 <= 2^19``: every product
and partial sum of the Gram ``|x|^2 + |z|^2 - 2 x.z`` and of the norms is a multiple of 2^-4
below 2^24, exact in fp32 in any order, and every coordinate fits the f16 hi part (lo = 0),
so ``d2`` is exact in all four kernels.  The two parts and the two models draw from different
streams; a few pred samples coincide with true samples and with each other; in about half
of the cases the last one or two of the D rows are the caller's zero padding.

What the rows see differs between the two families, and is less than "every row its own
set of near columns":
* vector kernel: pred samples are spread over cluster 0 and the far clusters 1 .. nfar - 2,
  so rows of different clusters have disjoint near sets; 10 % of the true samples follow the
  same law, the rest sit in two clusters no pred sample visits (invisible to every row);
* matrix-core kernels: every pred sample is in cluster 0 (a row far from the origin would
  put ``|p| w(0) 2^-22`` of split error on a gradient of O(1): item 4 below), so all pred rows
  share one set of near columns -- every pred column and the ~10 % of true columns in
  cluster 0 -- and differ in their 12 (offset, dimension pair) classes, i.e. in the ``d2``
  values, from {0 .. 2.5}.  A column read from a wrong index still moves ``ks`` by O(0.1) to
  O(1) and the gradient by O(1) unless both samples are of one class; rows of far clusters
  are exercised by mode 2 only (rows from ``data``).
test_mmd_exact_cpu.py checks what holds: the (near set, d2) sequences of the 32 rows on the
two sides of every boundary differ, and all 32-column tiles of both parts and models differ.

Rules restated from the kernels' headers
----------------------------------------
``ks(d2) = sum_g exp(-g d2)``, ``w(d2) = sum_g g exp(-g d2)``, g in GAMMAS.  Columns are the
joint [pred; true] (mode 2: the true part only, rows from ``data`` too), cut in tiles of
256 (valu) or 32 (matrix cores) per part; chunk c holds tiles [c tpc, (c+1) tpc).

* ``loss_part[r, c, rb] = sum_{i in rb} sum_{tile in c} wgt sum_{j in tile} ks(d2_ij)``;
  ``wgt`` = -2 on the true part, +1 on the pred part, except in symmetric launches:
  - valu: mode 1 over all rows, and modes 0/3 with ``mirror=1``: per 256-row tile rt,
    pred tile < rt: 0, == rt: 1, > rt: 2 (mode 2 of the vector kernel is not symmetric);
  - m32: modes 1 and 2 over all rows, per 32-row wave tile wr: tile < wr 0, == 1, > 2;
  - m16: modes 1 and 2 over all rows, for a chunk of pred tiles only and (mode 2 or
    TX % tpc == 0): per 128-row block rb, tile < 4 rb: 0, < 4 (rb + 1): 1, else 2;
  - m16g: never.
  Mode 3 writes a zero loss partial.
* ``grad_part[c, r, d, i_local] = gscale sum_{j in c} s_j w(d2_ij) (z_jd - p_id)``,
  ``s_j`` = +1 pred / -1 true, row stride ``n_rows``; with ``mirror=1`` the pred tiles left
  of the row's own tile are left out of the chunk slots and arrive through
* mirror slot ``n_chunks + a``: rows of tiles b > a get ``gscale sum_{i in tile a} w_ic
  (p_i - p_c)``, rows of tiles <= a exact zeros.

Error bound (u = 2^-24; adding an exact 0 commits no rounding, so depths count near pairs)
-----------------------------------------------------------------------------------------
1. Exponentials (``rbf7_values``): ``exp2(d2 * (-g L2E))`` on an argument with three
   roundings (two constants' product, the multiply): relative ``eps0 = 2^-23 + ln2 |arg| 3u``
   (1-ulp v_exp_f32; exp2(0) = 1 exactly).  A power p by any multiplication chain carries
   ``p eps0 + (p - 1) u``; p = 1, 10 on a = e^-0.005 d2 and 1, 2, 4, 20, 200 on
   c = e^-0.25 d2.  The seven-term sums add 8u:
   ``dks = sum e_g eps_g + 8u ks``, ``dw = sum g e_g (eps_g + u) + 8u w``.
2. Loss partial: per lane and tile at most A packed adds (A = 128 valu, 8 m32, 4 m16) and
   the x + y add, one fma per tile into the lane's sum, 6 wave and 3 block levels (a level
   rounds only if two rows of the block have a term), ``depth_i`` their sum:
   ``|err| <= sum_i depth_i u sum|terms_i| + sum |wgt| dks``.
3. Vector gradient: one product and one add per near column, then (x + y) * gscale:
   ``|err| <= gscale (sum_j dw_ij |z_jd - p_id| + (2 n_i + 3) u sum_j w_ij |z_jd - p_id|)``.
4. Matrix-core gradient ``(G_i - p_i rs_i) gscale``: G sums (wh + wl) z over the near
   columns in fp32 (two non-zero passes, one rounding per product at most), ``rs`` the
   unsplit w.  The split leaves ``|w - wh - wl| <= 2^-22 |w|``, or 2^-25 absolute where
   the residual is an f16 subnormal; with ``S1 = sum_j |W_ij| |z_jd|``, ``S0 = sum_j |W_ij|``:
   ``|err| <= gscale (sum_j dw_ij |z_jd - p_id| + 2^-22 S1 + 2^-25 sum_j |z_jd|
   + (min(2 n_i, A t_i) + 2) u S1 + (min(n_i, 3 t_i) + 6) u |p_id| S0 + 3u (S1 + |p_id| S0))``
   (t_i column tiles with a near column; an MFMA adds its exact dot product to the accumulator
   with at most two roundings: A = 8 per tile for m32, 4 for m16)
   -- relative to ``sum|terms| = S1 + |p| S0``, not to ``sum |W| |z - p|``: hence small centres.
The asserted tolerance is ``min(bound, cap)``, cap = 2e-5 of the loss partial, 2e-4 of the
gradient partial's max|g|; test_mmd_exact_cpu.py asserts bound <= cap for every case.

Mode 3 runs the same gradient instruction sequence as mode 0 in all four kernels (the
loss flag only removes the ``tl += ks`` / ``lacc`` updates): gradients are compared bit
for bit.  Every launch runs twice (equal bits) into sentinel-filled buffers with slack.
"""
import functools
import math

import numpy as np
import pytest
import torch

from cgnn_amd.engine.reference import GAMMAS

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FAR = 22500.0
L2E = 1.4426950408889634
ALLOWED_D2 = tuple(0.25 * q for q in range(11))        # 0 .. 2.5
LOSS_CAP, GRAD_CAP = 2e-5, 2e-4
SENT = -777.25
SLACK = 97
GSCALE = 0.75
PRED_OFF = ((0.5, 0.5), (0.5, 0.0), (0.0, 0.5))          # no (0, 0): few coincident pairs (w(0) = 56.8)
SMALL_PRED_OFF = ((0.0, 0.0), (0.5, 0.0), (0.0, 0.5))    # N <= 3: pred 0 at the origin
TRUE_OFF = ((1.0, 0.0), (0.5, 0.5), (1.0, 1.0))
# N <= 3 (the last true sample is then a copy of pred 0): no partial whose terms cancel
SMALL_TRUE_OFF = {1: ((0.5, 0.0),), 2: ((1.0, 0.0),) * 2, 3: ((1.0, 0.0), (0.5, 0.5), (1.0, 0.0))}
POW = (("a", 1), ("a", 10), ("c", 1), ("c", 2), ("c", 4), ("c", 20), ("c", 200))
_H2 = np.array([[1, 1], [1, -1]])
_H8 = np.kron(np.kron(_H2, _H2), _H2)

VALU_D = (1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 32, 48, 64)
MFMA_D = (8, 12, 16, 20, 24, 32, 48, 64, 80, 96, 128, 160, 192, 224, 256,
          320, 384, 448, 512, 640, 768, 896, 1024, 1280)
MFMA_N = (1, 3, 31, 32, 33, 127, 128, 129, 257)
MFMA_FULL = (8, 64, 128, 256, 512)
RANGES = ((0, None), (37, 90), (-1, 1), (128, -128))      # resolved against N = 257


# ---------------------------------------------------------------------------- cases
class Case:
    pass


def cluster_dims(k, g, da):
    """The two dimensions that carry the offsets of group g (0..3) of cluster k."""
    a = (3 * k + 2 * g) % da
    b = (da - 1 - 5 * k - 3 * g) % da
    if b == a:
        b = (a + 1) % da
    return a, b


@functools.lru_cache(maxsize=None)
def make_case(D, N, pad, big, pred_far=True, seed=0, R=2):
    """Lattice case: P, T [R, D, N] fp64, cluster ids, the clusters' offset dimensions.
    ``big``: share of cluster 0; ``pred_far=False`` keeps every pred sample in cluster 0."""
    da = D - pad
    assert da >= 1
    if da < 6:
        nfar = 12
        cent = np.zeros((nfar + 1, D))
        for k in range(1, nfar + 1):
            cent[k, 0] = 160.0 * ((k + 1) // 2) * (1 if k % 2 else -1)
    else:
        nfar = 16
        S = np.array([[(1 if k < 8 else -1) * _H8[k % 8][d % 8] for d in range(da)] for k in range(16)], float)
        ham = min(int((S[a] != S[b]).sum()) for a in range(16) for b in range(a))
        m = math.ceil(4.0 * 154.0 / math.sqrt(min(da, 4 * ham))) / 4.0   # offsets move a sample by < 3
        cent = np.zeros((nfar + 1, D))
        cent[1:, :da] = m * S
    u = np.zeros(D)
    if N > 3:
        u[:da] = (np.arange(da) % 3) / 4.0
    c = Case()
    c.D, c.N, c.pad, c.da, c.R, c.nfar = D, N, pad, da, R, nfar
    c.dims = [[cluster_dims(k, g, da) for g in range(4)] for k in range(nfar + 1)]
    c.P = np.zeros((R, D, N))
    c.T = np.zeros((R, D, N))
    c.cidP = np.zeros((R, N), int)
    c.cidT = np.zeros((R, N), int)
    for r in range(R):
        for part, (X, cid, offs) in enumerate(((c.P, c.cidP, PRED_OFF if N > 3 else SMALL_PRED_OFF),
                                               (c.T, c.cidT, TRUE_OFF if N > 3 else SMALL_TRUE_OFF[N]))):
            rng = np.random.default_rng([seed, D, N, pad, r, part])
            if N <= 3:
                k = np.zeros(N, int)
                typ = np.arange(N) % 3
                grp = np.zeros(N, int)
            else:
                # pred: cluster 0 or one of the far clusters 1 .. nfar - 2; true: 10 % likewise,
                # the rest in the last two clusters, which no pred sample visits (so that the
                # -2 pred-true sum does not cancel the pred-pred sum of a loss partial)
                k = np.where(rng.random(N) < big, 0, rng.integers(1, nfar - 1, N))
                if not pred_far:
                    k[:] = 0
                if part == 1:
                    k = np.where(rng.random(N) < 0.1, k, rng.integers(nfar - 1, nfar + 1, N))
                k[0] = k[N - 1] = 0
                typ = rng.integers(0, 3, N)
                grp = rng.integers(0, 4, N)
            cid[r] = k
            for i in range(N):
                x = cent[k[i]] + u
                a, b = c.dims[k[i]][grp[i]]
                x[a] += offs[typ[i]][0]
                if da > 1:
                    x[b] += offs[typ[i]][1]
                X[r, :, i] = x
        if N >= 16:     # coincident samples: pred = pred, true = pred
            for dst, src in ((9, 4), (N - 3, 1)):
                c.P[r, :, dst] = c.P[r, :, src]
                c.cidP[r, dst] = c.cidP[r, src]
            for dst, src in ((5, 7), (N - 2, 3)):
                c.T[r, :, dst] = c.P[r, :, src]
                c.cidT[r, dst] = c.cidP[r, src]
        elif N >= 2:
            c.T[r, :, N - 1] = c.P[r, :, 0]
            c.cidT[r, N - 1] = c.cidP[r, 0]
    return c


def rbf_terms(d2, near):
    """ks, w and their device error bounds dks, dw (docstring, item 1); 0 off the near set."""
    ks = np.zeros_like(d2)
    w = np.zeros_like(d2)
    dks = np.zeros_like(d2)
    dw = np.zeros_like(d2)
    arg = {"a": 0.005 * L2E * d2, "c": 0.25 * L2E * d2}
    for g, (base, p) in zip(GAMMAS, POW):
        e = np.where(near, np.exp(-g * np.where(near, d2, 0.0)), 0.0)
        eps0 = np.where(d2 == 0, 0.0, 2.0 ** -23 + math.log(2.0) * arg[base] * 3 * U)
        eps = p * eps0 + (p - 1) * U
        ks += e
        w += g * e
        dks += e * eps
        dw += g * e * (eps + U)
    return ks, w, dks + 8 * U * ks, dw + 8 * U * w


class Terms:
    pass


@functools.lru_cache(maxsize=8)
def tile_terms(case, r, tw, tt):
    """Per (row, column tile) sums in fp64: everything a partial is assembled from."""
    N, D = case.N, case.D
    P = case.T[r] if tt else case.P[r]
    cp = case.cidT[r] if tt else case.cidP[r]
    Z = case.T[r] if tt else np.concatenate([case.P[r], case.T[r]], 1)
    cz = case.cidT[r] if tt else np.concatenate([case.cidP[r], case.cidT[r]])
    TX = (N + tw - 1) // tw
    ct = TX if tt else 2 * TX
    ncol = Z.shape[1]
    j = np.arange(ncol)
    tile_of = np.where(j < N, j // tw, TX + (j - N) // tw)
    s = np.where(j < N, 1.0, -1.0)
    d2 = (P * P).sum(0)[:, None] + (Z * Z).sum(0)[None, :] - 2.0 * (P.T @ Z)     # exact in fp64
    near = cp[:, None] == cz[None, :]
    ks, w, dks, dw = rbf_terms(d2, near)
    ind = np.zeros((ncol, ct))
    ind[j, tile_of] = 1.0
    t = Terms()
    t.d2, t.near, t.TX, t.ct, t.P = d2, near, TX, ct, P
    t.KS, t.dKS, t.CNT, t.S0 = ks @ ind, dks @ ind, near.astype(float) @ ind, w @ ind
    t.G = np.zeros((D, N, ct))
    t.S1 = np.zeros((D, N, ct))
    t.S1b = np.zeros((D, N, ct))
    for k in range(ct):
        cols = np.nonzero(tile_of == k)[0]
        A = w[:, cols] * s[cols]
        t.S1[:, :, k] = np.abs(Z[:, cols]) @ np.abs(A).T
        t.S1b[:, :, k] = np.abs(Z[:, cols]) @ near[:, cols].astype(float).T
    # sum s w (z - p), sum |w| |z - p| and sum dw |z - p|: within a cluster only its offset dimensions differ
    t.S = np.zeros((D, N, ct))
    t.dG = np.zeros((D, N, ct))
    for k in np.unique(cp):
        I = np.nonzero(cp == k)[0]
        J = np.nonzero(cz == k)[0]
        for d in {d for ab in case.dims[k] for d in ab}:
            df = Z[d, J][None, :] - P[d, I][:, None]
            ad = np.abs(df)
            t.G[d, I, :] = (w[np.ix_(I, J)] * s[J] * df) @ ind[J]     # no G - p rs cancellation in fp64
            t.S[d, I, :] = (w[np.ix_(I, J)] * ad) @ ind[J]
            t.dG[d, I, :] = (dw[np.ix_(I, J)] * ad) @ ind[J]
    return t


# ---------------------------------------------------------------------------- geometry
TILE = {"valu": 256, "m32": 32, "m16": 32, "m16g": 32}
ROWS = {"valu": 256, "m32": 128, "m16": 128, "m16g": 128}
LANE_ADDS = {"valu": 128, "m32": 8, "m16": 4, "m16g": 4}
# roundings of the gradient accumulator per column tile: two non-zero passes (wh z, wl z) of
# 2 (m32, K = 16) or 1 (m16, K = 32) instructions, each an exact dot product summed and added
# to the accumulator with at most two roundings
MMA_ROUNDS = {"m32": 8, "m16": 4, "m16g": 4}


def kernel_kind(D, wide):
    if D > 256:
        return "m16g"
    if D >= 128 and wide != 0:
        return "m16"
    return "m32"


def col_tiles(kind, N, mode):
    TX = (N + TILE[kind] - 1) // TILE[kind]
    return TX, (TX if mode == 2 else 2 * TX)


def default_geometry(kind, N):
    """(n_chunks, tpc) the callers pick (engine.batch.mmd_geometry / mmd_mfma_geometry)."""
    if kind == "valu":
        return 2 * ((N + 255) // 256), 1
    rb = (N + 127) // 128
    ct = 2 * ((N + 31) // 32)
    n_chunks = min(ct, max(1, math.ceil(8 / rb)))
    tpc = math.ceil(ct / n_chunks)
    return math.ceil(ct / tpc), tpc


def geometries(kind, N, mode, full=True):
    """Distinct (n_chunks, tpc) with n_chunks == ceil(column_tiles / tpc): the callers' one
    (for a mode-2 launch the callers pass it unchanged: the surplus chunks are empty),
    tpc = 1, one chunk, a chunk straddling pred | true with an odd number of pred tiles,
    and tpc = 3 (whole chunks left of a row block's diagonal at N = 257)."""
    TX, ct = col_tiles(kind, N, mode)
    out = [default_geometry(kind, N)]
    # the one-row range (N - 1, 1) at N = 257: the last pred tile holds column N - 1 alone, so a
    # chunk that is just this tile has the row itself as its only near column -- a true gradient
    # partial of exactly 0 (cap 0), which the matrix-core kernels' G - p rs only approaches.
    # Their row ranges keep the chunkings in which that tile shares its chunk with others
    cand = [1, ct, 3] if full or kind == "valu" else [ct, 3]
    cand += [t for t in (2, 4) if (full or kind == "valu") and mode != 2 and TX % t % 2 == 1]
    for tpc in cand:
        if 1 <= tpc <= ct:
            g = (math.ceil(ct / tpc), tpc)
            if g not in out:
                out.append(g)
    return out


def loss_weights(kind, mode, D, N, row_begin, n_rows, tpc, mirror):
    """wgt[i_local, tile] of the loss (docstring, the symmetric rules)."""
    TX, ct = col_tiles(kind, N, mode)
    i = row_begin + np.arange(n_rows)[:, None]
    tile = np.arange(ct)[None, :]
    pred = tile < TX
    wgt = np.where(pred, 1.0, -2.0) * np.ones((n_rows, 1))
    all_rows = row_begin == 0 and n_rows == N
    tri = None
    if kind == "valu":
        if all_rows and (mode == 1 or (mirror and mode in (0, 3) and D <= 8)):
            tri = np.where(tile < i // 256, 0.0, np.where(tile == i // 256, 1.0, 2.0))
    elif kind == "m32":
        if all_rows and mode in (1, 2):
            tri = np.where(tile < i // 32, 0.0, np.where(tile == i // 32, 1.0, 2.0))
    elif kind == "m16":
        if all_rows and mode in (1, 2) and (mode == 2 or TX % tpc == 0):
            rb = i // 128
            tri = np.where(tile < 4 * rb, 0.0, np.where(tile < 4 * (rb + 1), 1.0, 2.0))
    if tri is not None:
        wgt = np.where(pred, tri, wgt)
    return wgt


class Expect:
    pass


def expected(case, r, kind, mode, row_begin, n_rows, n_chunks, tpc, mirror=0):
    """fp64 partials, their derived bounds and caps for one launch of model r."""
    D, N = case.D, case.N
    t = tile_terms(case, r, TILE[kind], mode == 2)
    TX, ct = t.TX, t.ct
    rows = slice(row_begin, row_begin + n_rows)
    RB = ROWS[kind]
    n_rb = (n_rows + RB - 1) // RB
    e = Expect()
    e.n_rb = n_rb
    wgt = loss_weights(kind, mode, D, N, row_begin, n_rows, tpc, mirror)
    e.L = np.zeros((n_chunks, n_rb))
    e.Lb = np.zeros((n_chunks, n_rb))
    grad = mode in (0, 3)
    msym = kind == "valu" and mirror and grad and D <= 8
    n_mir = (N + 255) // 256 - 1 if msym else 0
    if grad:
        e.G = np.zeros((n_chunks + n_mir, D, n_rows))
        e.Gb = np.zeros((n_chunks + n_mir, D, n_rows))
    il = np.arange(n_rows)
    P = t.P[:, rows]

    def grad_slot(slot, inc):           # inc[i_local, tile]: the tiles summed for each row
        cnt = (t.CNT[rows] * inc).sum(1)
        e.G[slot] = GSCALE * (t.G[:, rows] * inc).sum(2)
        dG = (t.dG[:, rows] * inc).sum(2)
        if kind == "valu":
            e.Gb[slot] = GSCALE * (dG + (2 * cnt + 3) * U * (t.S[:, rows] * inc).sum(2))
        else:
            S1 = (t.S1[:, rows] * inc).sum(2)
            pS0 = np.abs(P) * (t.S0[rows] * inc).sum(1)
            S1b = (t.S1b[:, rows] * inc).sum(2)
            ntile = ((t.CNT[rows] > 0) * inc).sum(1)
            acc = np.minimum(2 * cnt, MMA_ROUNDS[kind] * ntile) + 2
            e.Gb[slot] = GSCALE * (dG + 2.0 ** -22 * S1 + 2.0 ** -25 * S1b
                                   + acc * U * S1 + (np.minimum(cnt, 3 * ntile) + 6) * U * pS0 + 3 * U * (S1 + pS0))

    for c in range(n_chunks):
        tl = np.arange(c * tpc, min(ct, (c + 1) * tpc))
        if mode != 3 and len(tl):
            wl = wgt[:, tl]
            terms = np.abs(wl) * t.KS[rows][:, tl]
            near = (t.CNT[rows][:, tl] * (wl != 0)).sum(1)
            nzrows = np.add.reduceat((near > 0).astype(float), np.arange(0, n_rows, RB))
            tree = np.minimum(9, np.maximum(np.repeat(nzrows, RB)[:n_rows] - 1, 0))
            depth = np.minimum(near, LANE_ADDS[kind] + 1) + np.minimum(near, len(tl)) + tree + 1
            val = (wl * t.KS[rows][:, tl]).sum(1)
            err = depth * U * terms.sum(1) + (np.abs(wl) * t.dKS[rows][:, tl]).sum(1)
            e.L[c] = np.add.reduceat(val, np.arange(0, n_rows, RB))
            e.Lb[c] = np.add.reduceat(err, np.arange(0, n_rows, RB))
        if grad:
            inc = np.zeros((n_rows, ct))
            inc[:, tl] = 1.0
            if msym:
                inc[(np.arange(ct)[None, :] < TX) & (np.arange(ct)[None, :] < (il // 256)[:, None])] = 0.0
            grad_slot(c, inc)
    for a in range(n_mir):
        inc = np.zeros((n_rows, ct))
        inc[il // 256 > a, a] = 1.0
        grad_slot(n_chunks + a, inc)
    e.Lcap = LOSS_CAP * np.abs(e.L)
    if grad:
        e.Gcap = GRAD_CAP * np.abs(e.G).max((1, 2), keepdims=True) * np.ones_like(e.G)
    return e


def resolve_range(rng, N):
    b, n = rng
    b = b if b >= 0 else N + b
    n = N - b if n is None else (n if n > 0 else N + n)
    return b, n


# ---------------------------------------------------------------------------- device side
FRACTIONS = {}


def _record(key, err, bound):
    m = bound > 0
    if m.any():
        FRACTIONS[key] = max(FRACTIONS.get(key, 0.0), float((err[m] / bound[m]).max()))


def _dev(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()


class Launch:
    """One case on the device: inputs uploaded once, any (mode, geometry) launched on them."""

    def __init__(self, case, kind, wide=-1):
        from cgnn_amd import native
        self.hip = native.hip()
        self.case, self.kind, self.wide = case, kind, wide
        self.X, self.Y = _dev(case.P), _dev(case.T)
        assert np.array_equal(self.X.cpu().numpy().astype(np.float64), case.P)
        self.xn, self.yn = _dev((case.P ** 2).sum(1)), _dev((case.T ** 2).sum(1))
        self.st = torch.cuda.current_stream().cuda_stream

    def run(self, mode, row_begin, n_rows, n_chunks, tpc, mirror=0):
        c = self.case
        RB = ROWS[self.kind]
        n_rb = (n_rows + RB - 1) // RB
        n_mir = (c.N + 255) // 256 - 1 if mirror else 0
        ng = (n_chunks + n_mir) * c.R * c.D * n_rows
        nl = c.R * n_chunks * n_rb
        outs = []
        for _ in range(2):
            gp = torch.full((ng + SLACK,), SENT, device="cuda")
            lp = torch.full((nl + SLACK,), SENT, device="cuda")
            if self.kind == "valu":
                self.hip.mmd(mode, c.D, self.X.data_ptr(), self.Y.data_ptr(), gp.data_ptr(), lp.data_ptr(),
                             c.N, c.R, n_rb, n_chunks, tpc, GSCALE, self.st, row_begin, n_rows, mirror)
            else:
                self.hip.mmd_mfma(mode, c.D, self.X.data_ptr(), self.Y.data_ptr(), self.xn.data_ptr(),
                                  self.yn.data_ptr(), gp.data_ptr(), lp.data_ptr(), c.N, c.R, n_chunks, tpc,
                                  GSCALE, self.st, row_begin, n_rows, self.wide)
            torch.cuda.synchronize()
            outs.append((gp.cpu().numpy(), lp.cpu().numpy()))
        (g0, l0), (g1, l1) = outs
        for a, b, name in ((g0, g1, "gradient"), (l0, l1, "loss")):
            d = np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0]
            assert d.size == 0, "%s partials not deterministic: %d differ, first at %s: %s vs %s" % (
                name, d.size, d[:8], a[d[:8]], b[d[:8]])
        assert np.all(g0[ng:] == SENT) and np.all(l0[nl:] == SENT), "slack overwritten"
        if mode in (1, 2):
            assert np.all(g0 == SENT), "evaluation wrote gradient partials"
        return (g0[:ng].reshape(n_chunks + n_mir, c.R, c.D, n_rows),
                l0[:nl].reshape(c.R, n_chunks, n_rb))


def _close(dev, ref, bound, cap, key, what):
    err = np.abs(dev.astype(np.float64) - ref)
    assert np.all(bound <= cap * (1 + 1e-12)), "%s: derived bound above its cap" % what
    _record(key, err, bound)
    bad = err > np.minimum(bound, cap)
    assert not bad.any(), "%s: %d outside the bound, worst err %.3e vs bound %.3e at %s" % (
        what, int(bad.sum()), err[bad].max(), bound[bad][err[bad].argmax()],
        tuple(int(v[0]) for v in np.nonzero(bad)))


def check_launch(L, mode, row_begin, n_rows, n_chunks, tpc, mirror=0, g_mode0=None):
    """Launch and compare every partial of both models; returns the gradient partials."""
    c, kind = L.case, L.kind
    gp, lp = L.run(mode, row_begin, n_rows, n_chunks, tpc, mirror)
    what = "%s D=%d N=%d mode=%d rows=(%d,%d) chunks=%d tpc=%d mirror=%d" % (
        kind, c.D, c.N, mode, row_begin, n_rows, n_chunks, tpc, mirror)
    for r in range(c.R):
        e = expected(c, r, kind, mode, row_begin, n_rows, n_chunks, tpc, mirror)
        if mode == 3:
            assert np.all(lp[r] == 0.0), what + ": mode 3 loss partial not zero"
        else:
            _close(lp[r], e.L, e.Lb, e.Lcap, kind + " loss", what + " loss r=%d" % r)
        if mode in (0, 3):
            _close(gp[:, r], e.G, e.Gb, e.Gcap, kind + " grad", what + " grad r=%d" % r)
            if c.pad:
                assert np.all(gp[:, r, c.D - c.pad:] == 0.0), what + ": gradient of a zero-padded dimension"
    if g_mode0 is not None:
        assert np.array_equal(gp.view(np.uint32), g_mode0.view(np.uint32)), what + ": mode 3 != mode 0 bits"
    return gp


def check_case(L, ranges=((0, None),), mirrors=(0,)):
    c = L.case
    for rng in ranges:
        b, n = resolve_range(rng, c.N)
        full = (b, n) == (0, c.N)
        for mode in ((0, 1, 2, 3) if full else (0, 1, 3)):
            if mode == 3:
                continue
            for n_chunks, tpc in geometries(L.kind, c.N, mode, full):
                for mirror in (mirrors if (full and mode == 0) else (0,)):
                    g0 = check_launch(L, mode, b, n, n_chunks, tpc, mirror)
                    if mode == 0:
                        check_launch(L, 3, b, n, n_chunks, tpc, mirror, g_mode0=g0)
    print("err/bound so far:", {k: "%.3f" % v for k, v in sorted(FRACTIONS.items())})


# ---------------------------------------------------------------------------- case lists
# The loss cap is relative to |partial|, and a partial is a difference (pred-pred minus twice
# pred-true, or a mirrored launch's self pair minus a few true columns): where the default draw
# leaves one partial near 0 the cap falls below any honest bound, so these cases take another
VALU_SEED = {(6, 257): 2, (64, 257): 1}


def valu_case(D, N, pad):
    return make_case(D, N, pad, valu_big(D, pad), True, VALU_SEED.get((D, N), 0))


def valu_cases():
    out = []
    for k, D in enumerate(VALU_D):
        pad = 0 if D == 1 else (k % 2) * (1 if D < 8 else 2)
        ns = [(1, 255), (2, 256)][k % 2]
        out += [(D, n, pad) for n in ns]
        if D <= 8 or D in (12, 64):
            out.append((D, 257, pad))
        if D in (1, 8, 12, 64):
            out.append((D, 513, pad))
    return out


def valu_big(D, pad):
    return 1.0 / 11 if D - pad < 6 else 1.0 / 15


def mfma_cases():
    """(D, N, pad, wide)"""
    out = []
    for k, D in enumerate(MFMA_D):
        pad = (k % 2) * 2
        wides = (0, 1) if 128 <= D <= 256 else (-1,)
        ns = MFMA_N if D in MFMA_FULL else ((1, 3, 31)[k % 3], 257 if D == 24 else 129)
        out += [(D, n, pad, w) for n in ns for w in wides]
    return out


MFMA_BIG = 0.3


def mfma_case(D, N, pad):
    return make_case(D, N, pad, MFMA_BIG, False)

VALU_RANGE_D = ((4, 1), (64, 0))
# narrow: 16, not 8 -- at D = 8 the derived bound of the one-row range in a single chunk
# (257 near columns over 18 tiles, one row's own max|g| as the yardstick) is 1.0 to 1.3 caps
MFMA_RANGE_D = ((16, 0, -1), (96, 2, -1), (128, 0, 1), (224, 2, 1), (224, 2, 0), (320, 0, -1), (1024, 2, -1))


@pytest.mark.parametrize("D,N,pad", valu_cases())
def test_vector_kernel_partials(D, N, pad):
    L = Launch(valu_case(D, N, pad), "valu")
    check_case(L, mirrors=(0, 1) if D <= 8 and N > 256 else (0,))
    if D <= 8 and N > 256:
        # all n_chunks + mirror slots sum to the unmirrored gradient
        c = L.case
        n_chunks, tpc = default_geometry("valu", N)
        g1, _ = L.run(0, 0, N, n_chunks, tpc, 1)
        g0, _ = L.run(0, 0, N, n_chunks, tpc, 0)
        for r in range(c.R):
            e0 = expected(c, r, "valu", 0, 0, N, n_chunks, tpc, 0)
            e1 = expected(c, r, "valu", 0, 0, N, n_chunks, tpc, 1)
            tol = e0.Gb.sum(0) + e1.Gb.sum(0) + 8 * U * (np.abs(e0.G).sum(0) + np.abs(e1.G).sum(0))
            diff = np.abs(g1[:, r].astype(np.float64).sum(0) - g0[:, r].astype(np.float64).sum(0))
            assert np.all(diff <= tol)


@pytest.mark.parametrize("D,N,pad,wide", mfma_cases())
def test_matrix_core_kernel_partials(D, N, pad, wide):
    check_case(Launch(mfma_case(D, N, pad), kernel_kind(D, wide), wide))


@pytest.mark.parametrize("D,pad", VALU_RANGE_D)
def test_vector_kernel_row_ranges(D, pad):
    check_case(Launch(valu_case(D, 257, pad), "valu"), ranges=RANGES)


@pytest.mark.parametrize("D,pad,wide", MFMA_RANGE_D)
def test_matrix_core_kernel_row_ranges(D, pad, wide):
    check_case(Launch(mfma_case(D, 257, pad), kernel_kind(D, wide), wide), ranges=RANGES)


def test_launchers_refuse_bad_arguments_and_write_nothing():
    c = mfma_case(8, 33, 0)
    L = Launch(c, "valu")
    gp = torch.full((4096,), SENT, device="cuda")
    lp = torch.full((64,), SENT, device="cuda")
    hip, st = L.hip, L.st

    def valu(D, rb, n, mirror=0, mode=0):
        hip.mmd(mode, D, L.X.data_ptr(), L.Y.data_ptr(), gp.data_ptr(), lp.data_ptr(), c.N, 1, 1, 2, 1, 1.0, st,
                rb, n, mirror)

    def mfma(D, rb, n):
        hip.mmd_mfma(0, D, L.X.data_ptr(), L.Y.data_ptr(), L.xn.data_ptr(), L.yn.data_ptr(), gp.data_ptr(),
                     lp.data_ptr(), c.N, 1, 2, 2, 1.0, st, rb, n, -1)

    for call, code in ((lambda: valu(5, 0, 33), -1), (lambda: valu(8, 30, 4), -2), (lambda: valu(8, 0, 0), -2),
                       (lambda: valu(8, 0, 33, mirror=1), -2), (lambda: valu(8, 1, 32, mirror=1), -2),
                       (lambda: valu(8, 0, 33, mirror=1, mode=1), -2),
                       (lambda: mfma(10, 0, 33), -1), (lambda: mfma(1100, 0, 33), -1),
                       (lambda: mfma(8, 30, 4), -2), (lambda: mfma(8, 0, 0), -2)):
        with pytest.raises(RuntimeError, match=r"code %d\)" % code):
            call()
    torch.cuda.synchronize()
    assert bool((gp == SENT).all()) and bool((lp == SENT).all())


@pytest.mark.parametrize("d,N,kernel,symmetric", [(3, 257, "valu", True), (3, 257, "valu", False),
                                                  (22, 129, "mfma", True), (126, 129, "mfma", True)])
def test_mmd_loss_end_to_end(d, N, kernel, symmetric):
    """ops.mmd_loss (true-true pass, training pass, loss_finalize, slot sum) on lattice data:
    loss and pred.grad against the fp64 sums of the same partial references."""
    from cgnn_amd.engine.batch import padded_dim
    from cgnn_amd.ops.mmd import mmd_loss
    D = padded_dim(d)
    c = mfma_case(D, N, D - d) if kernel == "mfma" else valu_case(D, N, D - d)
    kind = "valu" if kernel == "valu" else kernel_kind(D, -1)
    tkind = "valu" if D <= 64 else kind          # the kernel of the true-true pass
    pred = _dev(c.P[:, :d].transpose(0, 2, 1)).requires_grad_(True)
    true = _dev(c.T[:, :d].transpose(0, 2, 1))
    out = mmd_loss(pred, true, kernel=kernel, symmetric=symmetric)
    out.sum().backward()
    loss, grad = out.detach().cpu().numpy().astype(np.float64), pred.grad.cpu().numpy().astype(np.float64)
    mirror = int(kind == "valu" and symmetric)
    for r in range(c.R):
        n_chunks, tpc = default_geometry(kind, N)
        e = expected(c, r, kind, 0, 0, N, n_chunks, tpc, mirror)
        et = expected(c, r, tkind, 2, 0, N, *default_geometry(tkind, N))
        n2 = float(N * N)
        ref = (e.L.sum() + et.L.sum()) / n2
        mag = np.abs(e.L).sum() + np.abs(et.L).sum()
        tol = (e.Lb.sum() + et.Lb.sum() + (e.L.size + et.L.size + 16) * U * mag) / n2
        assert abs(loss[r] - ref) <= tol, (loss[r], ref, tol)
        scale = 4.0 / n2 / GSCALE
        gref = scale * e.G.sum(0)[:d].T
        gtol = scale * (e.Gb.sum(0) + (e.G.shape[0] + 2) * U * np.abs(e.G).sum(0))[:d].T
        assert np.all(np.abs(grad[r] - gref) <= gtol), float(np.abs(grad[r] - gref).max())
