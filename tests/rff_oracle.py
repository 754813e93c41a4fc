"""fp64 oracle, argument-reduction emulation, error bounds and committed cases of the
Fourier-feature MMD kernels (rff_kernels.hip).

Plain helper of tests/test_rff_exact_cpu.py and tests/test_rff_exact_gpu.py: numpy only, it
knows nothing of the device.

Layouts: ``W [R][F][D+1]`` (D frequencies, then the phase), ``x [R][D][N]``, ``diff [R][F]``,
``loss_part [R][ceil(F/256)]``, ``grad [1][R][D][N]``; wide-form scratch: ``theta [R][N][F]``
then ``csum [R][2][NT][F]``, NT = ceil(N/32).

Stages (each compared on its own; loss partials and the gradient from the DEVICE's diff)
-----------------------------------------------------------------------------------------
* ``theta[n,f] = sum_k W[f,k] x[k,n] + W[f,D]``
* ``csum[part,nt,f]``: sum over the 32 samples of tile nt of ``cos theta`` (wide form)
* ``diff[f] = norm (sum_n cos theta_pred - sum_n cos theta_true) / N``
* ``loss_part[b] = sum_{f in [256 b, 256 b + 256)} diff_f^2``
* ``grad[k,n] = sum_f (-coef diff_f sin theta_pred[n,f]) W[f,k]``, ``coef = 2 norm / N`` (fp32)

Two tiers
---------
Exact-argument tier (``exact_case``): frequencies and samples are multiples of 2^-3, phases
multiples of 2^-6 in [0, 2 pi); ``sum_k |w_k x_k| + phase < 2^18``, so every product and every
partial sum of theta is a multiple of 2^-6 below 2^18: exact in fp32 in any order, the device's
theta is the fp64 theta bit for bit.  Two features per case carry frequencies large enough for
``|theta|`` up to about 2^11 (what the gamma = 50 block produces).  What is left on the device:
(a) ``fract(theta * 0.15915494f)`` in fp32 -- emulated here (``reduce32``), the cosine / sine of
``2 pi fract`` then taken in fp64; (b) the hardware v_cos_f32 / v_sin_f32 -- TRIG_UNITS of u per
evaluation, measured (below); (c) the fp32 sums -- depth * u * sum|terms|, u = 2^-24:

* csum: a sum of n terms rounds at most n - 1 times (adding to an exact zero commits nothing),
  and at most 15 times in the lane and once across the wave halves: min(16, n - 1).
* diff: vector kernel N - 1 sequential adds; matrix-core kernel at most 16 per tile in the
  lane, the shuffle included, min(N - 1, 16 NT); wide form 16 per tile and NT in the reduce
  kernel; three more for the subtraction, the scaling by norm and the division, all relative
  to at most ``sum |cos pred| + sum |cos true|``.
* loss partial: the square, six wave levels, at most eight adds over the waves: 16 u sum diff^2.
* gradient: ``-coef diff_f`` and its product with the sine round once each, every feature adds
  one fused step to the accumulator (the matrix-core products are the bits of an fmaf chain;
  adding a masked exact zero commits nothing): ``(F + 3) u sum_f |coef diff_f sin w_fk|``, in
  all three forms and for every chunking of F.

Against the plain fp64 ``cos(theta)`` the reduction adds ``2 u |theta| + pi u`` per evaluation
(the constant 1/2pi and the product round once each: ``2 pi |theta / 2 pi| 2 u``; the
subtraction of the floor rounds to 2^-25 revolutions).

Generic tier (``generic_case``): W from ``rff_freqs`` itself (all seven gammas), Gaussian x;
theta within ``(D + 1) u (sum_k |w_k x_k| + |phase|)`` of fp64, a cosine within that plus the
reduction term plus the trig allowance.  The bound of a committed generic case is at most
GENERIC_CAP of ``max_f |diff_f|`` (gradient: of ``max |g|``) -- a condition on the cases,
asserted from the reference alone.

Trig allowance
--------------
The residual against the emulated reference on the exact tier in units of u per trig term
times the element's weight (diff: ``2 N * norm / N``; csum: samples of the tile; gradient:
``sum_f |coef diff_f w_fk|``), whole and less the derived term (c).  TRIG_UNITS_SEEN is the worst
whole residual of the shallow sums (diff, csum) on an MI355X; allowed: one unit more (a
different but equally valid instruction schedule).
"""
import functools
import math

import numpy as np

from cgnn_gen_oracle import U, fma32, normal_reference, u01_f32
from cgnn_amd.utils import philox

GAMMAS = (0.005, 0.05, 0.25, 0.5, 1.0, 5.0, 50.0)
GAMMAS32 = np.asarray(GAMMAS, np.float32).astype(np.float64)
COMPILED_D = (1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 32, 48, 64, 80, 96, 128, 160, 192, 224, 256)
VALU_D = tuple(d for d in COMPILED_D if d <= 64)
INV_2PI32 = np.float32(0.15915494309189535)
TWO_PI32 = np.float32(6.283185307179586)
RW_KC, RW_FC = 32, 64                     # the wide form's k-chunk (proj) and f-chunk (grad)
LDS_FLOATS = 160 * 1024 // 4              # the gradient kernel's W image: F (D + 2) floats
# Measured on an MI355X over every exact-tier case: the whole residual of a diff element is at
# most 2.191 units and of a csum element 1.918 (one-sample tiles, where (c) is zero); above the
# derived term (c) 0.336, 1.918 and, for the gradient, 0 remain (its whole residual reaches 11.53
# units at F = 518, all of it inside the (F + 3) u accumulation term).  The larger figure is taken.
TRIG_UNITS_SEEN = 2.191
TRIG_UNITS = TRIG_UNITS_SEEN + 1.0
# tests/test_cgnn_gen_exact_gpu.py: 3.57 units of u * radius seen, one allowed on top; the
# scaling by 2 gamma rounds once more
FREQ_UNITS = 3.57 + 1.0 + 1.0
GENERIC_CAP = 1e-2


# ---------------------------------------------------------------------------- launcher mirror
def gradient_chunk(D, F):
    """FC of rff_fb_d: all F features when [F][D + 2] floats fit in 160 KiB, else the largest
    multiple of 32 that does."""
    if F * (D + 2) <= LDS_FLOATS:
        return F
    return LDS_FLOATS // (D + 2) // 32 * 32


def form_of(D, F, force_valu=0, force_wide=0):
    """'wide', 'mfma' or 'valu': the kernels rff_launch_fwd_bwd picks."""
    if D > 256 or force_wide:
        return "wide"
    if D > 64 or (not force_valu and gradient_chunk(D, F) == F):
        return "mfma"
    return "valu"


def wide_scratch_floats(N, F, R):
    return R * N * F + R * 2 * ((N + 31) // 32) * F


# ---------------------------------------------------------------------------- fp32 pieces
def reduce32(theta, c=INV_2PI32):
    """``fract(theta * c)`` as cos_rev / sin_rev compute it: the fp32 product, then the fp32
    difference to its floor (exact in fp64, rounded once).  In revolutions, fp64."""
    u = (np.asarray(theta, np.float32) * np.float32(c)).astype(np.float64)
    return (u - np.floor(u)).astype(np.float32).astype(np.float64)


def theta_chain32(W, x, order):
    """theta [N, F] of one model by an fp32 chain started from the phase: 'fwd' (k ascending,
    the vector kernels), 'bwd' (k descending) or 'pairs' (two products summed, then added: a
    two-deep matrix-core step), everything rounded to fp32 after every operation."""
    F, D = W.shape[0], W.shape[1] - 1
    w = W.astype(np.float32)
    xs = x.astype(np.float32)
    acc = np.repeat(w[None, :, D], x.shape[1], 0)
    ks = list(range(D))
    if order == "bwd":
        ks.reverse()
    if order == "pairs":
        for k in range(0, D, 2):
            p = w[None, :, k].astype(np.float64) * xs[k][:, None]
            if k + 1 < D:
                p = (p + w[None, :, k + 1].astype(np.float64) * xs[k + 1][:, None])
            acc = (acc.astype(np.float64) + p.astype(np.float32)).astype(np.float32)
        return acc
    for k in ks:
        acc = fma32(w[None, :, k], xs[k][:, None], acc)
    return acc


# ---------------------------------------------------------------------------- cases
class Case:
    pass


def _unique_rows(draw, n):
    """n rows from ``draw(m)`` with no two equal."""
    a = draw(n)
    for _ in range(64):
        _, first = np.unique(a, axis=0, return_index=True)
        dup = np.setdiff1d(np.arange(n), first)
        if dup.size == 0:
            return a
        a[dup] = draw(dup.size)
    raise AssertionError("could not draw distinct rows")


@functools.lru_cache(maxsize=None)
def exact_case(D, N, k, pad=0, R=2, seed=0):
    """Exact-argument case: W [R, F, D + 1], P, T [R, D, N] in fp64 on the dyadic grids."""
    F = 7 * k
    da = D - pad
    assert da >= 1
    xm = 8 * (64 if da == 1 else 32 if da == 2 else 8 if da <= 4 else 2)   # max |x|, in eighths
    wm = 8 * (32 if da <= 2 else 2)
    big = sorted({F // 2, F - 1} if F > 1 else {0})
    lm = max(8 * 2, int(8 * 2048 / (xm / 8.0 * math.sqrt(da))))  # big-argument frequencies, in eighths
    c = Case()
    c.D, c.N, c.k, c.F, c.pad, c.da, c.R, c.exact, c.big = D, N, k, F, pad, da, R, True, big
    c.W = np.zeros((R, F, D + 1))
    c.P = np.zeros((R, D, N))
    c.T = np.zeros((R, D, N))
    for r in range(R):
        rng = np.random.default_rng([seed, D, N, k, pad, r, 91])

        def wrow(m):
            w = np.zeros((m, D + 1))
            w[:, :da] = rng.integers(-wm, wm + 1, (m, da)) / 8.0
            w[:, D] = rng.integers(0, 403, m) / 64.0             # 402 / 64 < 2 pi
            return w
        c.W[r] = _unique_rows(wrow, F)
        for f in big:
            c.W[r, f, :da] = rng.integers(-lm, lm + 1, da) / 8.0
        both = _unique_rows(lambda m: rng.integers(-xm, xm + 1, (m, da)) / 8.0, 2 * N)
        c.P[r, :da] = both[:N].T
        c.T[r, :da] = both[N:].T
        if N >= 8:                                               # pred samples that are true samples
            c.T[r, :, 1] = c.P[r, :, 2]
            c.T[r, :, N - 2] = c.P[r, :, N - 1]
    c.amax = max(float((np.abs(c.W[r, :, :D]) @ np.abs(X[r]) + np.abs(c.W[r, :, D:])).max())
                 for r in range(R) for X in (c.P, c.T))
    return c


def freqs_reference(key, step, k, D, d_true, mut=None):
    """rff_freqs_kernel of one model: (W [F, D + 1] fp64, radius [F, D + 1]).  The frequencies are
    ``2 gamma_{f // k}`` times normal_reference at counter (f, dd, step, RNG_RFF_FREQ), the phase
    is the device's fp32 ``6.2831855f * u01(word z)`` at counter word d_true, bit for bit."""
    F = 7 * k
    f = np.arange(F, dtype=np.uint32)
    W = np.zeros((F, D + 1))
    rad = np.zeros((F, D + 1))
    z, rd = normal_reference(key, f[:, None], np.arange(d_true, dtype=np.uint32)[None, :], step,
                             philox.RNG_RFF_FREQ)
    blk = np.minimum(f // ((k + 1) if mut == "gamma_block" else k), 6)
    g2 = 2.0 * GAMMAS32[blk][:, None]
    W[:, :d_true] = g2 * z
    rad[:, :d_true] = g2 * rd
    w2 = philox.philox4x32_10(f, d_true, step, philox.RNG_RFF_FREQ, key[0], key[1])[2]
    W[:, D] = (TWO_PI32 * u01_f32(w2).astype(np.float32)).astype(np.float32)
    return W, rad


def mirror_term(key, f, dd, step):
    """|normal_reference - philox.normal| allows: the fp64 mirror keeps the half of u01 that the
    device's fp32 expression rounds away (up to 2^-25 on either uniform): through the radius
    ``2^-25 / (u1 rad)``, through the angle ``2 pi 2^-25 rad``."""
    r0, _, _, _ = philox.philox4x32_10(f, dd, step, philox.RNG_RFF_FREQ, key[0], key[1])
    u1 = u01_f32(r0)
    rad = np.sqrt(-2.0 * np.log(u1))
    with np.errstate(divide="ignore"):
        return np.where(rad > 0, 2.0 ** -25 / (u1 * np.maximum(rad, 1e-300)), np.inf) + 2 * math.pi * 2.0 ** -25 * rad


GENERIC_KEYS = tuple(philox.model_key(23, "rffx", r) for r in range(3))


@functools.lru_cache(maxsize=None)
def generic_case(D, N, k, scale, R=3, seed=0, step=5):
    """Generic-tier case: Gaussian samples; W is the numpy mirror of rff_freqs here (the CPU
    checks), the GPU test replaces it with the device's draw."""
    c = Case()
    c.D, c.N, c.k, c.F, c.pad, c.da, c.R, c.exact, c.big = D, N, k, 7 * k, 0, D, R, False, []
    c.step, c.scale = step, scale
    rng = np.random.default_rng([seed, D, N, k, 17])
    c.P = (scale * rng.normal(0, 1, (R, D, N))).astype(np.float32).astype(np.float64)
    c.T = (scale * (1.5 * rng.normal(0, 1, (R, D, N)) + 1.0)).astype(np.float32).astype(np.float64)
    c.W = np.stack([freqs_reference(GENERIC_KEYS[r], step, k, D, D)[0] for r in range(R)])
    c.W = c.W.astype(np.float32).astype(np.float64)
    return c


# ---------------------------------------------------------------------------- reference
class Expect:
    pass


MUTATIONS = ("tail_as_zero", "drop_last_sample", "drop_phase", "feature_shift", "sin_sign", "coef_half",
             "swap_parts", "chunk_last", "loss_group", "inv2pi")


def norm_of(k):
    return np.float32(math.sqrt(2.0 / k))


def diff_depth(form, N):
    """Roundings of a feature's cos sum (n terms: at most n - 1) plus the three of the epilogue."""
    NT = (N + 31) // 32
    return min(N - 1, {"valu": N - 1, "mfma": 16 * NT, "wide": 16 + NT}[form]) + 3


def expected(case, r, form, diff_dev=None, plain=False, units=TRIG_UNITS, mut=None, coef_exact=False):
    """Every stage of model r in fp64 with its tolerance.  ``plain``: against cos / sin of theta
    itself, not of the emulated reduction (always so on the generic tier).  ``diff_dev``: the
    device's diff (loss partials and gradient follow from it); None composes the stages: the
    reference diff and its tolerance carried into both.  ``mut``: one deliberate error."""
    D, N, F, k = case.D, case.N, case.F, case.k
    NT = (N + 31) // 32
    W, P, T = case.W[r], case.P[r], case.T[r]
    if mut == "swap_parts":
        P, T = T, P
    norm = float(norm_of(k))
    coef = float(np.float32(2.0) * norm_of(k) / np.float32(N))       # the launcher's fp32 expression
    if coef_exact:
        coef = 2.0 * norm / N
    Wt = W
    if mut == "feature_shift":
        Wt = W[np.minimum(np.arange(F) + 1, F - 1)]
    ph = 0.0 if mut == "drop_phase" else Wt[:, D]
    plain = plain or not case.exact
    c32 = INV_2PI32
    if mut == "inv2pi":
        c32 = np.float32(np.nextafter(INV_2PI32, np.float32(1)) * np.float32(1 + 2.0 ** -12))
    e = Expect()
    e.theta, e.atheta, cs, ec = [], [], [], []
    for X in (P, T):
        th = X.T @ Wt[:, :D].T + ph                                   # [N, F]
        ath = np.abs(X).T @ np.abs(Wt[:, :D]).T + np.abs(Wt[:, D])
        dth = 0.0 if case.exact else (D + 1) * U * ath
        red = (2 * U * np.abs(th) + math.pi * U) if plain else 0.0
        e.theta.append(th)
        e.atheta.append(ath)
        ang = th if plain else 2 * math.pi * reduce32(th, c32)
        cs.append(np.cos(ang))
        ec.append(units * U + red + dth + np.zeros_like(th))
        if X is P:
            e.dtheta_p = dth + np.zeros_like(th)
            sn, es = np.sin(ang), ec[0]
    # csum [2, NT, F]
    edges = np.arange(0, N, 32)
    e.csum = np.stack([np.add.reduceat(c, edges, 0) for c in cs])
    if mut == "tail_as_zero" and N % 32:
        # the pred part only: counted in both parts it cancels in diff and shows in csum alone
        e.csum[0, -1] += (32 - N % 32) * np.cos(Wt[:, D] if plain else 2 * math.pi * reduce32(Wt[:, D], c32))
    if mut == "drop_last_sample":
        e.csum[0, -1] -= cs[0][N - 1]
    cnt = np.minimum(32, N - edges)[:, None]
    e.csum_tol = np.stack([np.minimum(16, cnt - 1) * U * np.add.reduceat(np.abs(c), edges, 0)
                           + np.add.reduceat(x, edges, 0) for c, x in zip(cs, ec)])
    e.csum_w = U * cnt[None] * np.ones((2, NT, F))
    # diff [F]
    mag = np.abs(cs[0]).sum(0) + np.abs(cs[1]).sum(0)
    e.diff = norm * (e.csum[0].sum(0) - e.csum[1].sum(0)) / N
    e.diff_tol = norm / N * (diff_depth(form, N) * U * mag + ec[0].sum(0) + ec[1].sum(0))
    e.diff_w = U * 2 * N * norm / N * np.ones(F)
    # loss partials and gradient, from the device's diff when given
    composed = diff_dev is None
    dd = e.diff if composed else np.asarray(diff_dev, np.float64)
    td = e.diff_tol if composed else np.zeros(F)
    sq = dd * dd
    grp = np.arange(0, F, 256)
    if mut == "loss_group" and F > 257:
        grp = np.concatenate([[0], np.arange(257, F, 256)])
    e.loss = np.add.reduceat(sq, grp)
    e.loss_tol = np.add.reduceat(16 * U * sq + 2 * np.abs(dd) * td + td * td, grp)
    keep = np.ones(F)
    if mut == "chunk_last":
        keep[gradient_chunk(D, F) - 1::gradient_chunk(D, F)] = 0.0
    gs = {"sin_sign": -1.0, "coef_half": 0.5}.get(mut, 1.0)
    S = -gs * coef * (dd * keep)[None, :] * sn                           # [N, F]
    aW = np.abs(W[:, :D])
    e.grad = (S @ W[:, :D]).T                                            # [D, N]
    e.grad_w = U * ((coef * np.abs(dd)) @ aW)[:, None] * np.ones((D, N))
    e.grad_tol = ((F + 3) * U * (np.abs(S) @ aW) + (coef * np.abs(dd)[None, :] * es) @ aW
                  + coef * (td[None, :] * np.abs(sn)) @ aW).T
    return e


def reference_autograd(case, r):
    """(loss, dloss/dpred [D, N]) of engine.reference.rff_mmd_loss on the case's W, fp64 autograd."""
    import torch
    from cgnn_amd.engine.reference import rff_mmd_loss
    pred = torch.tensor(case.P[r].T.copy(), dtype=torch.float64, requires_grad=True)
    true = torch.tensor(case.T[r].T.copy(), dtype=torch.float64)
    # the kernels take norm as an fp32 argument: sqrt(2 / k) rounded once
    s = (float(norm_of(case.k)) / math.sqrt(2.0 / case.k)) ** 2
    loss = s * rff_mmd_loss(pred, true, torch.tensor(case.W[r].T.copy(), dtype=torch.float64), case.k)
    (g,) = torch.autograd.grad(loss, pred)
    return float(loss.detach()), g.numpy().T


# ---------------------------------------------------------------------------- committed cases
EX_N = (1, 31, 32, 33, 64, 65, 127, 128, 129, 257)
EX_K = (1, 5, 32, 37, 74)


def _pad_of(i, D):
    return 0 if D == 1 else (i % 2) * (1 if D < 8 else 2)


def narrow_cases(D):
    """(D, N, k, pad) of the default path at a compiled D: four (N, k) that cycle through EX_N
    and EX_K over the widths, k lowered to the largest of EX_K whose image is staged whole."""
    i = COMPILED_D.index(D)
    out = []
    for j in range(4):
        N = EX_N[(4 * i + 3 * j) % 10]
        q = (i + j) % 5
        while gradient_chunk(D, 7 * EX_K[q]) != 7 * EX_K[q]:
            q -= 1
        out.append((D, N, EX_K[q], _pad_of(i + j, D)))
    return out


def valu_cases(D):
    i = COMPILED_D.index(D)
    return [(D, EX_N[(3 * i + 1 + 4 * j) % 10], EX_K[(i + 2 * j + 1) % 5], _pad_of(i + j + 1, D)) for j in range(3)]


# (D, N, k, pad): F (D + 2) floats exceed the image, the gradient stages FC < F features at a time
CHUNKED_CASES = ((256, 129, 37, 0), (128, 33, 46, 2), (80, 129, 74, 2), (96, 65, 74, 0), (160, 257, 74, 0),
                 (192, 33, 74, 2), (224, 128, 74, 0))
CHUNKS = {(256, 37): (128, 128, 3), (128, 46): (288, 34), (80, 74): (480, 38), (96, 74): (416, 102),
          (160, 74): (224, 224, 70), (192, 74): (192, 192, 134), (224, 74): (160, 160, 160, 38)}
VALU_UNFORCED = (64, 65, 89, 2)           # D <= 64 whose image does not fit: the vector kernels
# (D, N, k, pad, force_wide): F = 7, 63, 70, 259
WIDE_CASES = ((1, 33, 10, 0, 1), (1, 1, 1, 0, 1), (5, 65, 9, 1, 1), (5, 33, 37, 0, 1), (31, 1, 9, 0, 1),
              (31, 65, 10, 2, 1), (32, 33, 1, 0, 1), (32, 65, 37, 2, 1), (33, 65, 9, 0, 1), (33, 33, 10, 2, 1),
              (63, 33, 37, 0, 1), (63, 1, 10, 1, 1), (64, 65, 10, 0, 1), (64, 33, 9, 2, 1),
              (257, 33, 9, 0, 0), (257, 65, 37, 2, 0), (300, 65, 10, 0, 0), (300, 1, 1, 1, 0), (300, 33, 37, 2, 0))
# (D, N, k, scale): generic tier
GENERIC_CASES = ((2, 65, 5, 0.5), (2, 129, 37, 0.5), (12, 129, 5, 0.125), (12, 33, 37, 0.25), (32, 65, 5, 0.02))


def all_exact_cases():
    """(D, N, k, pad, force_valu, force_wide) of every exact-tier launch."""
    out = []
    for D in COMPILED_D:
        out += [c + (0, 0) for c in narrow_cases(D)]
    for D in VALU_D:
        out += [c + (1, 0) for c in valu_cases(D)]
    out += [c + (0, 0) for c in CHUNKED_CASES]
    out.append(VALU_UNFORCED + (0, 0))
    out += [c[:4] + (0, c[4]) for c in WIDE_CASES]
    return out


# (D, d_true, k, step_base, step_off): rff_freqs
FREQ_CASES = ((12, 10, 5, 3, 2), (12, 10, 5, 5, 0), (12, 10, 5, 5, 1), (16, 10, 5, 5, 0), (4, 4, 1, 0, 0),
              (2, 1, 3, 9, 0), (64, 64, 37, 1, 0), (31, 31, 2, 2, 0))
