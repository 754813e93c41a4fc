"""Kernel-level fp64 oracle tests of the Fourier-feature MMD kernels (rff_kernels.hip), through
the raw bindings ``hip.rff_freqs``, ``hip.rff_fwd_bwd`` and ``hip.rff_wide_scratch_floats``.

Every element a launch writes is compared with tests/rff_oracle.py, one stage at a time (theta
and the cos sums of the wide form's scratch image, diff, the loss partials and the gradient --
the last two from the DEVICE's diff), in two tiers: the exact-argument tier, on which theta is
exact in fp32 and the fp32 argument reduction is emulated, so that only the hardware cosine /
sine and the fp32 sums are left; and the generic tier, W from ``rff_freqs`` itself and Gaussian
samples, under the derived bound capped at 1e-2 of ``max |diff|`` / ``max |g|``.  Once per case
and model the composed stages are compared with fp64 autograd of
``engine.reference.rff_mmd_loss`` on the same W.  rff_oracle.py derives the bounds;
test_rff_exact_cpu.py checks the oracle and the case tables.

Every case runs in mode 0 and in mode 1 (loss only: equal bits of diff, loss partials and the
wide scratch; gradient buffer untouched).  Every output lies between guard bands in a buffer
prefilled with a NaN pattern: the exact set of written elements is asserted (all of diff, the
loss partials, chunk 0 of a two-chunk gradient buffer, exactly ``rff_wide_scratch_floats``
floats of scratch in the wide form and none of it otherwise).

Measured on an MI355X (``SEEN``, printed after every case; docs/KERNELS.md): the whole residual
of a diff element reaches 2.191 units of u per trig term, of a csum element 1.918; the
gradient's is inside its accumulation term everywhere.  TRIG_UNITS_SEEN in rff_oracle.py is the
former, one more unit is allowed.  ``rff_freqs``: 3.71 units of ``u * 2 gamma * radius``.
"""
import copy

import numpy as np
import pytest
import torch

import rff_oracle as ox
from cgnn_amd import native
from cgnn_amd.engine.batch import _keys_tensor

pytestmark = pytest.mark.gpu

U = ox.U
GUARD = 193
PATTERN = 0x7FC0BEEF                      # a quiet NaN with a payload no kernel produces
SEEN = {}


def _record(key, value):
    SEEN[key] = max(SEEN.get(key, 0.0), float(value))


class Guarded:
    """An fp32 output of ``shape`` between two guard bands, everything set to PATTERN."""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.flat = torch.full((self.n + 2 * GUARD,), PATTERN, dtype=torch.int32, device="cuda")
        self.shape = shape

    def ptr(self):
        return self.flat.data_ptr() + 4 * GUARD

    def read(self):
        """(values, written mask); asserts the guard bands."""
        bits = self.flat.cpu().numpy()
        assert np.all(bits[:GUARD] == PATTERN) and np.all(bits[GUARD + self.n:] == PATTERN), "guard band written"
        mid = bits[GUARD:GUARD + self.n].reshape(self.shape)
        return mid.view(np.float32), mid != PATTERN


def _dev(x):
    t = torch.tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()
    assert np.array_equal(t.cpu().numpy().astype(np.float64), x), "input not representable in fp32"
    return t


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Out:
    pass


def launch(case, mode, force_valu, force_wide):
    hip = native.hip()
    R, D, N, F, k = case.R, case.D, case.N, case.F, case.k
    X, Y, W = _dev(case.P), _dev(case.T), _dev(case.W)
    ns = hip.rff_wide_scratch_floats(N, F, R)
    assert ns == ox.wide_scratch_floats(N, F, R)
    diff, lp, grad, scr = Guarded(R, F), Guarded(R, (F + 255) // 256), Guarded(2, R, D, N), Guarded(ns)
    hip.rff_fwd_bwd(mode, X.data_ptr(), Y.data_ptr(), W.data_ptr(), diff.ptr(), lp.ptr(), grad.ptr(), N, D, F, R, k,
                    float(ox.norm_of(k)), _stream(), force_valu=force_valu, scratch=scr.ptr(), force_wide=force_wide)
    torch.cuda.synchronize()
    o = Out()
    o.diff, o.diff_w = diff.read()
    o.lp, o.lp_w = lp.read()
    o.grad, o.grad_w = grad.read()
    o.scr, o.scr_w = scr.read()
    return o


def _within(dev, ref, tol, what, key=None):
    err = np.abs(dev.astype(np.float64) - ref)
    if key:
        m = tol > 0
        if m.any():
            _record(key + " err/tol", (err[m] / tol[m]).max())
    bad = ~(err <= tol)
    assert not bad.any(), "%s: %d outside the tolerance, worst err %.3e vs %.3e at %s" % (
        what, int(bad.sum()), np.nanmax(err[bad]), tol[bad][np.nanargmax(err[bad])],
        tuple(int(v[0]) for v in np.nonzero(bad)))


def _units(dev, ref, tol0, weight, key):
    """Exact tier: the residual in units of u per trig term times the element's weight -- raw, and
    what is left of it above ``tol0``, the tolerance without a trig allowance."""
    err = np.abs(dev.astype(np.float64) - ref)
    m = weight > 0
    if m.any():
        _record(key + " raw", (err[m] / weight[m]).max())
        _record(key, (np.maximum(err - tol0, 0.0)[m] / weight[m]).max())


def check_case(case, force_valu=0, force_wide=0):
    R, D, N, F = case.R, case.D, case.N, case.F
    NT = (N + 31) // 32
    form = ox.form_of(D, F, force_valu, force_wide)
    what = "%s D=%d N=%d F=%d pad=%d %s" % (form, D, N, F, case.pad, "exact" if case.exact else "generic")
    o, o1 = launch(case, 0, force_valu, force_wide), launch(case, 1, force_valu, force_wide)
    # ---- write sets
    for x in (o, o1):
        assert x.diff_w.all() and x.lp_w.all(), what + ": diff / loss partial not fully written"
        assert x.scr_w.all() if form == "wide" else not x.scr_w.any(), what + ": scratch write set"
    assert o.grad_w[0].all() and not o.grad_w[1].any(), what + ": gradient write set (chunk 0 only)"
    assert not o1.grad_w.any(), what + ": mode 1 wrote the gradient buffer"
    for a, b, name in ((o.diff, o1.diff, "diff"), (o.lp, o1.lp, "loss partials"), (o.scr, o1.scr, "scratch")):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what + ": mode 1 %s != mode 0 bits" % name
    theta = o.scr[:R * N * F].reshape(R, N, F)
    csum = o.scr[R * N * F:].reshape(R, 2, NT, F)
    for r in range(R):
        w = what + " r=%d" % r
        refs = [(ox.expected(case, r, form, diff_dev=o.diff[r]), "")]
        if case.exact:
            refs.append((ox.expected(case, r, form, diff_dev=o.diff[r], plain=True), " (plain)"))
        for e, tag in refs:
            tier = ("exact " if case.exact else "generic ") + form + tag
            if form == "wide":
                if case.exact:
                    assert np.array_equal(theta[r].astype(np.float64), e.theta[0]), w + ": theta not bit-exact"
                else:
                    _within(theta[r], e.theta[0], e.dtheta_p, w + " theta", tier + " theta")
                _within(csum[r], e.csum, e.csum_tol, w + " csum" + tag, tier + " csum")
            _within(o.diff[r], e.diff, e.diff_tol, w + " diff" + tag, tier + " diff")
            _within(o.lp[r], e.loss, e.loss_tol, w + " loss partial" + tag, tier + " loss")
            _within(o.grad[0, r], e.grad, e.grad_tol, w + " grad" + tag, tier + " grad")
            assert not o.grad[0, r][e.grad_w == 0].any(), w + ": gradient where every frequency is zero"
            if not case.exact:
                assert e.diff_tol.max() <= ox.GENERIC_CAP * np.abs(e.diff).max(), w + ": diff bound above its cap"
                assert e.grad_tol.max() <= ox.GENERIC_CAP * np.abs(e.grad).max(), w + ": grad bound above its cap"
        if case.exact:
            e, z = refs[0][0], ox.expected(case, r, form, diff_dev=o.diff[r], units=0.0)
            if form == "wide":
                _units(csum[r], e.csum, z.csum_tol, e.csum_w, "trig units csum")
            _units(o.diff[r], e.diff, z.diff_tol, e.diff_w, "trig units diff")
            _units(o.grad[0, r], e.grad, z.grad_tol, e.grad_w, "trig units grad")
        if case.pad:
            assert not o.grad[0, r, D - case.pad:].any(), w + ": gradient of a zero-padded dimension"
        # the composed stages against autograd of the model's definition
        ec = ox.expected(case, r, form, plain=True)
        loss, g = ox.reference_autograd(case, r)
        lsum = o.lp[r].astype(np.float64).sum()
        assert abs(lsum - loss) <= ec.loss_tol.sum() + 2 * U * abs(loss), w + ": loss vs autograd"
        _within(o.grad[0, r], g, ec.grad_tol + 2 * U * np.abs(g), w + " grad vs autograd")
    print("seen so far:", {k: "%.3f" % v for k, v in sorted(SEEN.items())})


# ---------------------------------------------------------------------------- exact tier
@pytest.mark.parametrize("D", ox.COMPILED_D)
def test_default_path_every_compiled_width(D):
    for c in ox.narrow_cases(D):
        check_case(ox.exact_case(*c))


@pytest.mark.parametrize("D", ox.VALU_D)
def test_vector_kernels_every_compiled_width(D):
    for c in ox.valu_cases(D):
        check_case(ox.exact_case(*c), force_valu=1)


@pytest.mark.parametrize("D,N,k,pad", ox.CHUNKED_CASES)
def test_chunked_gradient(D, N, k, pad):
    assert ox.gradient_chunk(D, 7 * k) < 7 * k
    check_case(ox.exact_case(D, N, k, pad))


def test_vector_kernels_when_the_image_does_not_fit():
    D, N, k, pad = ox.VALU_UNFORCED
    assert ox.form_of(D, 7 * k) == "valu"
    check_case(ox.exact_case(D, N, k, pad))


@pytest.mark.parametrize("D,N,k,pad,force_wide", ox.WIDE_CASES)
def test_wide_form(D, N, k, pad, force_wide):
    check_case(ox.exact_case(D, N, k, pad), force_wide=force_wide)


# ---------------------------------------------------------------------------- rff_freqs
def _freqs(D, d_true, k, step, off, R=3):
    hip = native.hip()
    F = 7 * k
    W = Guarded(R, F, D + 1)
    keys = _keys_tensor(ox.GENERIC_KEYS[:R], "cuda")
    st = torch.tensor([step, 1000], dtype=torch.int32, device="cuda")
    hip.rff_freqs(W.ptr(), keys.data_ptr(), st.data_ptr(), off, k, D, 7, d_true, R, _stream())
    torch.cuda.synchronize()
    w, written = W.read()
    assert written.all(), "rff_freqs: not every element written"
    return w


@pytest.mark.parametrize("D,d_true,k,step,off", ox.FREQ_CASES)
def test_freqs_against_the_fp64_mirror(D, d_true, k, step, off):
    from cgnn_amd.engine.reference import rff_frequencies
    w = _freqs(D, d_true, k, step, off)
    F = 7 * k
    f = np.arange(F, dtype=np.uint32)[:, None]
    dd = np.arange(d_true, dtype=np.uint32)[None, :]
    for r, key in enumerate(ox.GENERIC_KEYS):
        ref, rad = ox.freqs_reference(key, step + off, k, D, d_true)
        err = np.abs(w[r, :, :d_true].astype(np.float64) - ref[:, :d_true])
        rd = rad[:, :d_true]
        assert not err[rd == 0].any()
        units = err[rd > 0] / (U * rd[rd > 0])
        _record("freq units", units.max())
        assert units.max() <= ox.FREQ_UNITS, "frequencies: %.3f units of u * 2 gamma * radius" % units.max()
        assert not w[r, :, d_true:D].any(), "padded columns not exact zeros"
        assert np.array_equal(w[r, :, D].view(np.uint32), ref[:, D].astype(np.float32).view(np.uint32)), "phase bits"
        # neighbouring gamma blocks: features k - 1 and k against the reference of their own block
        for fa in (k - 1, k):
            g2 = 2.0 * ox.GAMMAS32[fa // k]
            z, zr = ox.normal_reference(key, np.uint32(fa), dd[0], step + off, ox.philox.RNG_RFF_FREQ)
            assert np.all(np.abs(w[r, fa, :d_true] - g2 * z) <= ox.FREQ_UNITS * U * g2 * zr)
        eng = rff_frequencies(key, step + off, k, d_true).numpy().T
        g2 = 2.0 * np.repeat(np.asarray(ox.GAMMAS), k)[:, None]
        tol = ox.FREQ_UNITS * U * rd + g2 * ox.mirror_term(key, f, dd, step + off) + 2 * U * np.abs(eng[:, :d_true])
        assert np.all(np.abs(w[r, :, :d_true] - eng[:, :d_true]) <= tol), "engine oracle"
        assert np.all(np.abs(w[r, :, D] - eng[:, d_true]) <= 4 * U * 2 * np.pi)
    print("seen so far:", {k_: "%.3f" % v for k_, v in sorted(SEEN.items())})


def test_freqs_padding_and_step_offset():
    a = _freqs(12, 10, 5, 3, 2)
    b = _freqs(12, 10, 5, 5, 0)
    c = _freqs(12, 10, 5, 5, 1)
    d = _freqs(16, 10, 5, 5, 0)
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)
    assert np.array_equal(bits(a), bits(b)), "(step_base 3, off 2) != (5, 0)"
    assert not np.array_equal(bits(b[:, :, :10]), bits(c[:, :, :10])) and not np.array_equal(bits(b[:, :, 12]), bits(c[:, :, 12]))
    assert np.array_equal(bits(b[:, :, 12]), bits(d[:, :, 16])), "phase depends on the padding"
    assert np.array_equal(bits(b[:, :, :10]), bits(d[:, :, :10]))
    assert not np.array_equal(bits(b[0]), bits(b[1])) and not np.array_equal(bits(b[1]), bits(b[2]))


# ---------------------------------------------------------------------------- generic tier
@pytest.mark.parametrize("D,N,k,scale", ox.GENERIC_CASES)
def test_generic_tier(D, N, k, scale):
    base = ox.generic_case(D, N, k, scale)
    w = _freqs(D, D, k, base.step - 2, 2)
    case = copy.copy(base)
    case.W = w.astype(np.float64)
    # the device's draw is the mirror's, up to the normal's units
    assert np.abs(case.W - base.W).max() <= 1e-4 * np.abs(base.W).max()
    for fv, fw in ((0, 0), (1, 0), (0, 1)):
        check_case(case, force_valu=fv, force_wide=fw)
