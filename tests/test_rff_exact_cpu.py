"""The Fourier-feature MMD oracle (tests/rff_oracle.py) and its committed cases, checked
without a GPU: the exact-argument tier is exact, the case tables reach the branches they name,
the reference is the model's definition (fp64 autograd, 1e-12), the generic tier's bounds sit
under their cap, the launcher's early returns, and eleven deliberate errors land outside the
asserted tolerance (twice the tolerance: the device may sit anywhere inside it).
"""
import math
import re

import numpy as np
import pytest

import rff_oracle as ox
from cgnn_amd import native
from cgnn_amd.utils import philox

U = ox.U
EXACT = ox.all_exact_cases()
UNIQUE = sorted({c[:4] for c in EXACT})


def test_case_tables_cover_the_shapes():
    default = [c for c in EXACT if not c[4] and not c[5]]
    assert {c[0] for c in default} >= set(ox.COMPILED_D) | {257, 300}
    assert {c[0] for c in EXACT if c[4]} == set(ox.VALU_D)
    assert {c[1] for c in default} >= set(ox.EX_N)
    assert {c[2] for c in default} >= set(ox.EX_K)
    wide = [c for c in EXACT if ox.form_of(c[0], 7 * c[2], c[4], c[5]) == "wide"]
    assert {c[0] for c in wide} == {1, 5, 31, 32, 33, 63, 64, 257, 300}
    assert {7 * c[2] for c in wide} == {7, 63, 70, 259} and {c[1] for c in wide} == {1, 33, 65}
    assert all(c[5] == (c[0] <= 256) for c in wide)
    padded = sum(1 for c in UNIQUE if c[3])
    assert 0.35 * len(UNIQUE) <= padded <= 0.65 * len(UNIQUE)
    for D in ox.COMPILED_D:                       # every tile count and both sides of the 128 / 256 blocks
        assert len({c[1] for c in ox.narrow_cases(D)}) == 4


def test_forms_and_gradient_chunks_follow_the_launcher():
    chunked = {c[:4] for c in ox.CHUNKED_CASES}
    for D, N, k, pad, fv, fw in EXACT:
        F = 7 * k
        form = ox.form_of(D, F, fv, fw)
        FC = ox.gradient_chunk(D, F)
        if (D, N, k, pad) in chunked:
            assert form == "mfma" and 32 <= FC < F and FC % 32 == 0
            assert tuple(min(FC, F - f0) for f0 in range(0, F, FC)) == ox.CHUNKS[(D, k)]
            assert (F % FC) % 32 != 0
        elif (D, N, k, pad) == ox.VALU_UNFORCED:
            assert form == "valu" and FC < F and not fv
        elif fw or D > 256:
            assert form == "wide"
        elif fv:
            assert form == "valu" and D <= 64
        else:
            assert form == "mfma" and FC == F
    assert ox.CHUNKS[(256, 37)] == (128, 128, 3) and ox.CHUNKS[(128, 46)] == (288, 34)
    assert [ox.gradient_chunk(D, 518) for D in (80, 96, 160, 192, 224)] == [480, 416, 224, 192, 160]


@pytest.mark.parametrize("D,N,k,pad", UNIQUE)
def test_exact_tier_is_exact(D, N, k, pad):
    c = ox.exact_case(D, N, k, pad)
    da = D - pad
    assert c.amax < 2.0 ** 18
    for r in range(c.R):
        W = c.W[r]
        assert np.array_equal(W[:, :D] * 8, np.round(W[:, :D] * 8)) and np.array_equal(W[:, D] * 64, np.round(W[:, D] * 64))
        assert W[:, D].min() >= 0 and W[:, D].max() < 2 * math.pi
        assert not W[:, da:D].any() and not c.P[r, da:].any() and not c.T[r, da:].any()
        th = []
        for X in (c.P[r], c.T[r]):
            assert np.array_equal(X * 8, np.round(X * 8))
            t64 = X.T @ W[:, :D].T + W[:, D]
            for order in ("fwd", "bwd", "pairs"):
                t32 = ox.theta_chain32(W, X, order)
                assert np.array_equal(t32.astype(np.float64), t64), order
            fr = ox.reduce32(t64)
            assert fr.min() >= 0.0 and fr.max() < 1.0
            # no two features and no two samples interchangeable
            assert np.unique(t64, axis=0).shape[0] == N and np.unique(W, axis=0).shape[0] == c.F
            assert N == 1 or np.unique(t64, axis=1).shape[1] == c.F      # one sample: two features may meet
            th.append(t64)
        big = np.abs(th[0][:, c.big]).max()
        assert big <= 2.0 ** 13 and (N < 31 or big >= 2.0 ** 8), big
        if N >= 8:
            assert np.array_equal(c.T[r, :, 1], c.P[r, :, 2]) and np.array_equal(c.T[r, :, N - 2], c.P[r, :, N - 1])
    assert not np.array_equal(c.W[0], c.W[1]) and not np.array_equal(c.P[0], c.P[1])


AUTOGRAD = [("exact",) + c for c in ((1, 33, 5, 0), (12, 65, 5, 2), (64, 31, 37, 0), (128, 33, 46, 2), (300, 33, 37, 2))]
AUTOGRAD += [("generic",) + c for c in ox.GENERIC_CASES[:2]]


@pytest.mark.parametrize("case", AUTOGRAD, ids=str)
def test_reference_is_the_models_definition(case):
    c = ox.exact_case(*case[1:]) if case[0] == "exact" else ox.generic_case(*case[1:])
    for r in range(c.R):
        e = ox.expected(c, r, "mfma", plain=True, coef_exact=True)
        loss, g = ox.reference_autograd(c, r)
        assert abs(e.loss.sum() - loss) <= 1e-12 * max(abs(loss), 1e-30)
        assert np.abs(e.grad - g).max() <= 1e-12 * np.abs(g).max()


def test_emulated_reduction_stays_within_its_derived_term():
    """cos of the fp32-reduced argument against cos(theta): within 2 u |theta| + pi u, and the
    large-argument features use a visible share of it (the emulation is not a no-op)."""
    worst = 0.0
    for D, N, k, pad in ((1, 257, 5, 0), (12, 65, 5, 2), (256, 129, 37, 0)):
        c = ox.exact_case(D, N, k, pad)
        for r in range(c.R):
            th = c.P[r].T @ c.W[r, :, :D].T + c.W[r, :, D]
            d = np.abs(np.cos(2 * math.pi * ox.reduce32(th)) - np.cos(th))
            lim = 2 * U * np.abs(th) + math.pi * U
            assert np.all(d <= lim)
            worst = max(worst, float((d / lim).max()))
    assert worst > 0.05


@pytest.mark.parametrize("D,N,k,scale", ox.GENERIC_CASES)
def test_generic_tier_bounds_are_under_their_cap(D, N, k, scale):
    c = ox.generic_case(D, N, k, scale)
    assert {int(b) for b in np.arange(c.F) // k} == set(range(7))
    for form in ("mfma", "valu", "wide"):
        for r in range(c.R):
            e = ox.expected(c, r, form)                     # composed: the widest tolerance asserted
            assert e.diff_tol.max() <= ox.GENERIC_CAP * np.abs(e.diff).max()
            assert e.grad_tol.max() <= ox.GENERIC_CAP * np.abs(e.grad).max()
            assert e.csum_tol.max() <= ox.GENERIC_CAP * N


def test_wide_scratch_floats():
    hip = native.hip()
    for (N, F, R), want in (((1, 7, 2), 42), ((33, 63, 2), 2 * 33 * 63 + 2 * 2 * 2 * 63), ((65, 259, 3), 3 * 65 * 259 + 3 * 2 * 3 * 259),
                            ((32, 70, 1), 32 * 70 + 2 * 70), ((257, 518, 2), 2 * 257 * 518 + 2 * 2 * 9 * 518)):
        assert hip.rff_wide_scratch_floats(N, F, R) == want == ox.wide_scratch_floats(N, F, R)


P = 64        # a non-null pointer; never dereferenced: both returns come before any HIP call


def _code(code, **kw):
    a = dict(mode=0, xhat=P, data=P, w=P, feat=P, loss=P, grad=P, N=33, D=12, F=35, R=2, k=5, norm=0.6, st=0)
    a.update(kw)
    with pytest.raises(RuntimeError) as err:
        native.hip().rff_fwd_bwd(**a)
    assert re.search(r"\(code %d\)" % code, str(err.value)), str(err.value)


def test_launcher_refuses_before_launching():
    for D in range(1, 257):
        if D not in ox.COMPILED_D:
            for mode in (0, 1):
                _code(-1, D=D, mode=mode)
            _code(-1, D=D, force_valu=1)
            _code(-1, D=D, scratch=0)
    _code(-1, D=0)
    _code(-2, D=257, scratch=0)
    _code(-2, D=300, scratch=0, mode=1)
    for D in (1, 5, 12, 64, 256):
        _code(-2, D=D, force_wide=1, scratch=0)
    _code(-2, D=12, force_wide=1, force_valu=1, scratch=0)


# ---------------------------------------------------------------------------- the oracle can fail
MUT_CASES = ((12, 33, 74, 2, 0, 0), (64, 65, 32, 2, 1, 0), (256, 129, 37, 0, 0, 0), (128, 33, 46, 2, 0, 0),
             (96, 65, 74, 0, 0, 0), (63, 33, 37, 0, 0, 1), (300, 65, 10, 0, 0, 0))
STAGE = {"tail_as_zero": "diff", "drop_last_sample": "diff", "drop_phase": "diff", "feature_shift": "diff",
         "swap_parts": "diff", "inv2pi": "diff", "sin_sign": "grad", "coef_half": "grad", "chunk_last": "grad",
         "loss_group": "loss"}


def test_mutation_cases_are_committed_cases():
    assert set(MUT_CASES) <= set(EXACT)
    assert set(STAGE) == set(ox.MUTATIONS)


@pytest.mark.parametrize("mut", ox.MUTATIONS)
def test_deliberate_errors_land_outside_the_tolerance(mut):
    caught = []
    for D, N, k, pad, fv, fw in MUT_CASES:
        c = ox.exact_case(D, N, k, pad)
        form = ox.form_of(D, c.F, fv, fw)
        if mut == "chunk_last" and not (form == "mfma" and ox.gradient_chunk(D, c.F) < c.F):
            continue
        if mut == "loss_group" and c.F <= 257:
            continue
        for r in range(c.R):
            clean = ox.expected(c, r, form)
            e0 = ox.expected(c, r, form, diff_dev=clean.diff)
            em = ox.expected(c, r, form, diff_dev=clean.diff, mut=mut)
            s = STAGE[mut]
            out = np.abs(getattr(em, s) - getattr(e0, s)) > 2 * getattr(e0, s + "_tol")
            caught.append(bool(out.any()))
            if s == "diff" and form == "wide":
                assert (np.abs(em.csum - e0.csum) > 2 * e0.csum_tol).any()
    assert caught and all(caught), (mut, caught)


# ---------------------------------------------------------------------------- rff_freqs
@pytest.mark.parametrize("D,d_true,k,step,off", ox.FREQ_CASES)
def test_freqs_reference_agrees_with_the_engine_oracle(D, d_true, k, step, off):
    from cgnn_amd.engine.reference import rff_frequencies
    F = 7 * k
    for key in ox.GENERIC_KEYS:
        W, rad = ox.freqs_reference(key, step + off, k, D, d_true)
        eng = rff_frequencies(key, step + off, k, d_true).numpy().T          # [F, d_true + 1]
        f = np.arange(F, dtype=np.uint32)[:, None]
        dd = np.arange(d_true, dtype=np.uint32)[None, :]
        g2 = 2.0 * np.repeat(np.asarray(ox.GAMMAS), k)[:, None]
        tol = g2 * ox.mirror_term(key, f, dd, step + off) + 2 * U * np.abs(eng[:, :d_true])   # gamma as fp32
        assert np.all(np.abs(W[:, :d_true] - eng[:, :d_true]) <= tol)
        assert not W[:, d_true:D].any()
        assert np.all(np.abs(W[:, D] - eng[:, d_true]) <= 2 * math.pi * 2.0 ** -25 + 2 * U * 2 * math.pi)
        # the gamma block of feature f is f // k: a reference with f // (k + 1) is far outside
        Wm, _ = ox.freqs_reference(key, step + off, k, D, d_true, mut="gamma_block")
        units = np.abs(Wm[:, :d_true] - W[:, :d_true]) / (U * np.maximum(rad[:, :d_true], 1e-300))
        assert units.max() > 1e3 * ox.FREQ_UNITS
        assert np.array_equal(Wm[:k], W[:k]) and not np.array_equal(Wm[k], W[k])
