"""The case builders, references and bounds of test_mmd_exact_gpu.py, checked without a GPU:
the lattice really makes d2 exact, the clusters are separated, the geometry helpers agree
with the engine's, the per-partial references add up to ``mmd_loss_dense`` and its fp64
autograd gradient, and every derived bound is below its cap."""
import numpy as np
import pytest
import torch

import test_mmd_exact_gpu as mx
from cgnn_amd.engine.batch import mmd_geometry, mmd_mfma_geometry
from cgnn_amd.engine.reference import mmd_loss_dense


def all_cases():
    """(case, kind, ranges, mirrors) of every GPU test."""
    out = []
    for D, N, pad in mx.valu_cases():
        out.append((mx.valu_case(D, N, pad), "valu", ((0, None),),
                    (0, 1) if D <= 8 and N > 256 else (0,)))
    for D, N, pad, wide in mx.mfma_cases():
        out.append((mx.mfma_case(D, N, pad), mx.kernel_kind(D, wide), ((0, None),), (0,)))
    for D, pad in mx.VALU_RANGE_D:
        out.append((mx.valu_case(D, 257, pad), "valu", mx.RANGES, (0,)))
    for D, pad, wide in mx.MFMA_RANGE_D:
        out.append((mx.mfma_case(D, 257, pad), mx.kernel_kind(D, wide), mx.RANGES, (0,)))
    return out


CASES = all_cases()
IDS = ["%s-D%d-N%d-p%d%s" % (k, c.D, c.N, c.pad, "-ranges" if len(rg) > 1 else "") for c, k, rg, _ in CASES]


def test_case_lists_cover_every_width_and_kernel():
    assert {c.D for c, k, _, _ in CASES if k == "valu"} == set(mx.VALU_D)
    assert {c.D for c, k, _, _ in CASES if k != "valu"} == set(mx.MFMA_D)
    assert {c.D for c, k, _, _ in CASES if k == "m16"} == {128, 160, 192, 224, 256}
    assert {c.D for c, k, _, _ in CASES if k == "m32"} >= {8, 96, 128, 160, 192, 224, 256}
    assert {c.N for c, k, _, _ in CASES if k == "valu"} == {1, 2, 255, 256, 257, 513}
    for D in mx.MFMA_FULL:
        assert {c.N for c, k, _, _ in CASES if k != "valu" and c.D == D} >= set(mx.MFMA_N)
    for D in mx.MFMA_D:
        ns = {c.N for c, k, _, _ in CASES if k != "valu" and c.D == D}
        assert any(n < 32 for n in ns) and any(n > 128 and n % 32 == 1 for n in ns)
    assert max(c.N for c, _, _, _ in CASES) <= 513


@pytest.mark.parametrize("case,kind", [(c, k) for c, k, _, _ in CASES], ids=IDS)
def test_lattice_is_exact_and_separated(case, kind):
    c = case
    for r in range(c.R):
        for X in (c.P[r], c.T[r]):
            assert np.array_equal(X * 4, np.round(X * 4))                    # multiples of 1/4
            assert np.all(X[c.D - c.pad:] == 0)
            hi = X.astype(np.float32).astype(np.float16)
            lo = (X.astype(np.float32) - hi.astype(np.float32)).astype(np.float16)
            assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), X)      # hi/lo round trip
            assert np.all(np.abs(lo.astype(np.float64)) >= 2.0 ** -14) or np.all(lo == 0)  # lo normal (here: 0)
            if kind != "valu":
                # sum |terms| of every norm and Gram, in units of the quantum 2^-4, stays below 2^24
                assert (X * X).sum(0).max() <= 2.0 ** 19
        Z = np.concatenate([c.P[r], c.T[r]], 1)
        if kind != "valu":
            assert (np.abs(c.P[r]).T @ np.abs(Z)).max() * 16 * 2 < 2.0 ** 24
        t = mx.tile_terms(c, r, mx.TILE[kind], False)
        assert np.array_equal(t.near, t.d2 < mx.FAR)
        assert np.all(t.d2[~t.near] >= mx.FAR)
        assert set(np.unique(t.d2[t.near])) <= set(mx.ALLOWED_D2)
        if c.N >= 16:
            assert (t.d2[:, c.N:] == 0).any() and (t.d2[:, :c.N] == 0).sum() > c.N   # coincident samples
    if c.N >= 31:
        assert not np.array_equal(c.P[0], c.P[1]) and not np.array_equal(c.P[0], c.T[0])


def _signature(t, i):
    j = np.nonzero(t.near[i])[0]
    return tuple(j), tuple(t.d2[i, j])


@pytest.mark.parametrize("case,kind", [(c, k) for c, k, _, _ in CASES if c.N >= 31], ids=[
    i for i, (c, _, _, _) in zip(IDS, CASES) if c.N >= 31])
def test_row_signatures_differ_across_boundaries(case, kind):
    """The rows on the two sides of every tile / row-block / chunk boundary (all multiples of
    32) see different near columns (coincident samples share theirs by construction); the
    column tiles of the joint, of both parts and both models, are pairwise different."""
    c = case
    tiles = []
    for r in range(c.R):
        t = mx.tile_terms(c, r, mx.TILE[kind], False)
        # the 32 rows before and after every boundary: different sequences of signatures
        for b in range(32, c.N - 31, 32):
            assert [_signature(t, i)[1] for i in range(b - 32, b)] != [_signature(t, i)[1] for i in range(b, b + 32)]
            assert _signature(t, b - 1)[0] != _signature(t, b)[0] or c.cidP[r, b - 1] == c.cidP[r, b]
        assert len({_signature(t, i) for i in range(c.N)}) >= 3
        Z = np.concatenate([c.P[r], c.T[r]], 1)
        for part in range(2):
            for c0 in range(0, c.N, 32):
                blk = Z[:, part * c.N + c0: part * c.N + min(c.N, c0 + 32)]
                if blk.shape[1] == 32:
                    tiles.append(blk.tobytes())
    assert len(set(tiles)) == len(tiles)


def test_geometry_helpers_agree_with_the_engine():
    for N in (1, 2, 3, 31, 32, 33, 127, 128, 129, 255, 256, 257, 513):
        rt, n_chunks, tpc = mmd_geometry(N)
        assert mx.default_geometry("valu", N) == (n_chunks, tpc) and rt == (N + 255) // 256
        rb, n_chunks, tpc = mmd_mfma_geometry(N)
        assert mx.default_geometry("m32", N) == (n_chunks, tpc) and rb == (N + 127) // 128
        for kind in ("valu", "m32"):
            for mode in (0, 2):
                TX, ct = mx.col_tiles(kind, N, mode)
                for g in mx.geometries(kind, N, mode)[1:]:
                    assert g[0] == -(-ct // g[1])
    # a chunk straddling pred | true with an odd number of pred tiles, and chunks wholly left of
    # a row block's diagonal, exist where the issue asks for them
    assert (5, 4) in mx.geometries("m32", 257, 0) and (9, 2) in mx.geometries("m32", 257, 0)
    assert (6, 3) in mx.geometries("m32", 257, 1) and (18, 1) in mx.geometries("m32", 257, 1)
    assert (3, 2) in mx.geometries("valu", 513, 0)


def _dense(case, r):
    p = torch.tensor(case.P[r].T.copy(), dtype=torch.float64, requires_grad=True)
    L = mmd_loss_dense(p, torch.tensor(case.T[r].T.copy(), dtype=torch.float64))
    (g,) = torch.autograd.grad(L, p)
    return float(L), g.numpy().T


@pytest.mark.parametrize("case,kind,mirrors", [(c, k, m) for c, k, rg, m in CASES if len(rg) == 1], ids=[
    i for i, (_, _, rg, _) in zip(IDS, CASES) if len(rg) == 1])
def test_partials_sum_to_the_dense_loss_and_gradient(case, kind, mirrors):
    c, N = case, case.N
    for r in range(c.R):
        Ld, gd = _dense(c, r)
        totals = []
        for mirror in mirrors:
            for n_chunks, tpc in mx.geometries(kind, N, 0):
                e = mx.expected(c, r, kind, 0, 0, N, n_chunks, tpc, mirror)
                for tmode_geom in mx.geometries(kind, N, 2):
                    et = mx.expected(c, r, kind, 2, 0, N, *tmode_geom)
                    totals.append((e.L.sum() + et.L.sum()) / N ** 2)
                np.testing.assert_allclose(4.0 / N ** 2 / mx.GSCALE * e.G.sum(0), gd, rtol=1e-12, atol=1e-12)
                # evaluation (symmetric weights where the kernel applies them): the same total
                e1 = mx.expected(c, r, kind, 1, 0, N, n_chunks, tpc)
                np.testing.assert_allclose(e1.L.sum(), e.L.sum(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(totals, Ld, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case,kind,ranges,mirrors", CASES, ids=IDS)
def test_derived_bounds_are_below_their_caps(case, kind, ranges, mirrors):
    c = case
    worst = [0.0, 0.0]
    for rng in ranges:
        b, n = mx.resolve_range(rng, c.N)
        full = (b, n) == (0, c.N)
        for mode in ((0, 1, 2) if full else (0, 1)):
            for n_chunks, tpc in mx.geometries(kind, c.N, mode, full):
                for mirror in (mirrors if full and mode == 0 else (0,)):
                    for r in range(c.R):
                        e = mx.expected(c, r, kind, mode, b, n, n_chunks, tpc, mirror)
                        what = (kind, c.D, c.N, mode, b, n, n_chunks, tpc, mirror, r)
                        m = e.Lb > 0
                        if m.any():
                            worst[0] = max(worst[0], float((e.Lb[m] / np.maximum(e.Lcap[m], 1e-300)).max()))
                        assert np.all(e.Lb <= e.Lcap), ("loss", what, worst)
                        if mode == 0:
                            m = e.Gb > 0
                            if m.any():
                                worst[1] = max(worst[1], float((e.Gb[m] / np.maximum(e.Gcap[m], 1e-300)).max()))
                            assert np.all(e.Gb <= e.Gcap), ("grad", what, worst)
    print("bound/cap worst (loss, grad):", worst)


def test_row_range_partials_are_rows_of_the_full_launch():
    c = mx.mfma_case(8, 257, 0)
    for kind in ("valu", "m32"):
        n_chunks, tpc = mx.default_geometry(kind, 257)
        full = mx.expected(c, 0, kind, 0, 0, 257, n_chunks, tpc)
        for rng in mx.RANGES[1:]:
            b, n = mx.resolve_range(rng, 257)
            e = mx.expected(c, 0, kind, 0, b, n, n_chunks, tpc)
            assert e.G.shape == (n_chunks, 8, n)
            np.testing.assert_array_equal(e.G, full.G[:, :, b:b + n])


def test_sparse_abs_terms_match_a_dense_evaluation():
    c = mx.mfma_case(12, 129, 2)
    t = mx.tile_terms(c, 1, 32, False)
    Z = np.concatenate([c.P[1], c.T[1]], 1)
    _, w, _, _ = mx.rbf_terms(t.d2, t.near)
    ad = np.abs(Z[:, None, :] - c.P[1][:, :, None])                 # [D, N, 2N]
    S = (w[None] * ad)
    for k in range(t.ct):
        cols = np.r_[32 * k:min(129, 32 * k + 32)] if k < t.TX else 129 + np.r_[32 * (k - t.TX):min(129, 32 * (k - t.TX) + 32)]
        np.testing.assert_allclose(t.S[:, :, k], S[:, :, cols].sum(2), rtol=1e-13, atol=1e-13)
