"""Kernel-level fp64 oracle tests of the CGNN generator, Adam, init, noise and loss-finalize
kernels (cgnn_kernels.hip, cgnn_staged.hip) through the raw ``_hip`` launchers.

The oracle, the fp32 emulation, the bounds and the committed cases live in
tests/cgnn_gen_oracle.py; tests/test_cgnn_gen_exact_cpu.py proves on the CPU that the bounds
hold for an fp32 evaluation in the kernels' order, that seven deliberate errors break them,
and that no pre-activation of a committed backward input is near zero.

Launch hygiene: parameters come from ``engine.batch.param_buffer`` (PARAM_PAD floats past the
last model), ``gpart`` is [R][gen_bwd_blocks(N) | staged_tiles(N)][P], ``noise`` [R][NS][N],
``dxs`` [R][Dt][N] in every staged backward, and a forced placement is launched only when
its LDS (the launchers' formulas, mirrored in the helper and pinned against ``staged_plan`` on
the CPU) fits.  Every output sits between guard bands, filled with a NaN pattern: the tests
assert the exact write set.

Measured on an MI355X (largest error / bound per kernel: docs/KERNELS.md).  The device normal
is not bit-exact with a numpy evaluation: against ``normal_reference`` (fp64 log / sqrt / cos
of the device's own fp32 uniforms) the largest difference over all draws of this file was
3.57 units of ``u * radius`` (v_log_f32 / v_cos_f32 have absolute errors, so the unit is the
Box-Muller radius, not the draw), 2.52 for ``init_params``; the allowance is the former plus
one unit (one more for the scaling by init_std).  A draw from a wrong counter is off by
O(1), 10^7 units.  All 144 Adam updates were bitwise the numpy fp32 evaluation in the
kernel's order (powf and sqrtf agreed), so the test asserts equal bits.
"""
import numpy as np
import pytest
import torch

import cgnn_gen_oracle as ox
from cgnn_amd import native
from cgnn_amd.engine.batch import _keys_tensor, param_buffer
from cgnn_amd.engine.program import pack_schedules
from cgnn_amd.utils import philox

pytestmark = pytest.mark.gpu

U = ox.U
GUARD = 193
PATTERN = 0x7FC0BEEF                      # a quiet NaN with a payload no kernel produces
NORMAL_UNITS_SEEN = 3.57                  # largest seen over every draw of this file (MI355X)
NORMAL_UNITS = NORMAL_UNITS_SEEN + 1.0
FRACTIONS = {}


def _record(key, value):
    FRACTIONS[key] = max(FRACTIONS.get(key, 0.0), float(value))


def _ratio(key, err, bound):
    m = bound > 0
    if m.any():
        _record(key, (err[m] / bound[m]).max())


class Guarded:
    """An fp32 output of ``shape`` between two guard bands, everything set to PATTERN."""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.flat = torch.full((self.n + 2 * GUARD,), PATTERN, dtype=torch.int32, device="cuda")
        self.t = self.flat[GUARD:GUARD + self.n].view(torch.float32).view(*shape)
        self.shape = shape

    def ptr(self):
        return self.t.data_ptr()

    def read(self):
        """(values, written mask); asserts the guard bands."""
        bits = self.flat.cpu().numpy()
        assert np.all(bits[:GUARD] == PATTERN) and np.all(bits[GUARD + self.n:] == PATTERN), "guard band written"
        mid = bits[GUARD:GUARD + self.n].reshape(self.shape)
        return mid.view(np.float32), mid != PATTERN


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _params(theta):
    R, P = theta.shape
    buf = param_buffer(R, P, "cuda")
    buf.copy_(_dev(theta))
    return buf


def _stream():
    return torch.cuda.current_stream().cuda_stream


KEYS = [philox.model_key(17, "gx", r) for r in range(3)]


def _check_normals(dev, ref, rad, what):
    units = ox.normal_units(dev, ref, rad)
    _record("normal units", units.max())
    print("%s: device normal vs fp64 mirror, max %.3f units of u * radius" % (what, units.max()))
    assert units.max() <= NORMAL_UNITS, "%s: %.3f units at %s" % (
        what, units.max(), np.unravel_index(units.argmax(), units.shape))


# ---------------------------------------------------------------------------- forward
def _forward_case(progs, H, N, row0, step0, off, seed):
    """gen_fwd and gen_noise on one batch: noise against Philox, both noise buffers equal,
    every node against the oracle from the kernel's own inputs, write sets."""
    hip = native.hip()
    c = ox.make_case(progs, H, N, 1, seed)
    R, D, d, NS, P = c.R, c.D, c.d, c.NS, c.P
    assert hip.gen_fwd_lds(D, c.ps) <= ox.LDS_MAX
    theta = ox.forward_params(progs, P, seed)
    rng = np.random.default_rng([seed, H, N])
    data = np.zeros((R, D, N), np.float32)
    data[:, :d] = rng.standard_normal((R, d, N))
    prog, th, dat = _dev(c.prog), _params(theta), _dev(data)
    keys = _keys_tensor(KEYS[:R], "cuda")
    step = torch.tensor([step0, 99], dtype=torch.int32, device="cuda")
    xh, nz, xn, nz2 = Guarded(R, D, N), Guarded(R, NS, N), Guarded(R, N), Guarded(R, NS, N)
    hip.gen_fwd(prog.data_ptr(), c.ps, th.data_ptr(), P, dat.data_ptr(), xh.ptr(), nz.ptr(), NS, xn.ptr(),
                keys.data_ptr(), step.data_ptr(), off, N, D, H, R, _stream(), row0)
    hip.gen_noise(prog.data_ptr(), c.ps, keys.data_ptr(), step.data_ptr(), off, nz2.ptr(), NS, N, D, d, R, row0,
                  _stream())
    torch.cuda.synchronize()
    (x, xw), (z, zw), (nrm, nw), (z2, z2w) = xh.read(), nz.read(), xn.read(), nz2.read()
    what = "fwd H=%d N=%d" % (H, N)
    assert nw.all() and xw[:, :d].all() and not xw[:, d:].any(), what + ": xhat / xnorm write set"
    for r, p in enumerate(progs):
        rows, ref, rad = ox.noise_reference(p, KEYS[r], D, N, row0, step0 + off)
        want = np.zeros(NS, bool)
        want[rows] = True
        assert np.array_equal(zw[r].all(1), want) and np.array_equal(zw[r].any(1), want), what + ": noise write set"
        _check_normals(z[r, rows], ref, rad, what)
        # gen_noise: every variable row and every stream of the model; the same bits
        want2 = np.zeros(NS, bool)
        want2[:d] = True
        want2[D:D + p.n_conf] = True
        assert np.array_equal(z2w[r].all(1), want2) and np.array_equal(z2w[r].any(1), want2)
        assert np.array_equal(z[r, rows].view(np.uint32), z2[r, rows].view(np.uint32)), what + ": gen_noise bits"
        zin = np.where(zw[r], z[r], 0.0)
        val, bnd, obs, n2, n2b = ox.forward_oracle(p, H, theta[r], D, x[r], zin, data[r])
        err = np.abs(x[r, :d].astype(np.float64) - val)
        _ratio("gen_fwd", err, bnd)
        bad = err > bnd
        assert not bad.any(), "%s r=%d: node value outside the bound at (var, sample) %s: err %.3e" % (
            what, r, tuple(int(v[0]) for v in np.nonzero(bad)), err[bad].max())
        assert np.array_equal(x[r, :d][obs], data[r, :d][obs]), what + ": observed column"
        e2 = np.abs(nrm[r] - n2)
        _ratio("xnorm", e2, n2b)
        assert np.all(e2 <= n2b), what + ": xnorm"
    return c, x, z


@pytest.mark.parametrize("H", ox.COMPILED_H + (7, 25))
def test_per_sample_forward(H):
    for k, N in enumerate((1, 63, 64, 65, 257)):
        _forward_case(ox.per_sample_batch(H), H, N, row0=(0, 3, 1000)[k % 3], step0=5 * k, off=k % 2 * 2, seed=k)
    print("err/bound so far:", FRACTIONS)


@pytest.mark.parametrize("d", [70, 130])
def test_per_sample_forward_narrow_blocks(d):
    """D = 80 / 160: gen_fwd_block drops to 128 and to 64 samples per block."""
    hip = native.hip()
    assert hip.gen_fwd_lds(64, 0) // (4 * 64) == 256
    assert hip.gen_fwd_lds(80, 0) // (4 * 80) == 128 and hip.gen_fwd_lds(160, 0) // (4 * 160) == 64
    _forward_case([ox.wide(4, d, 3, seed=5), ox.wide(4, d, 2, seed=6)], 4, 150, row0=7, step0=1, off=1, seed=d)


# ---------------------------------------------------------------------------- backward
def _check_gpart(c, gp, gw, BS, key, what):
    K = ox.backward_K(BS, c.depth, c.max_in, c.H)
    for r, p in enumerate(c.progs):
        ref, maj, written = ox.backward_oracle(p, c.H, c.theta[r], c.D, c.xhat[r], c.noise[r], c.gradp[:, r], BS, c.P)
        assert written[:p.n_params].all() and not written[p.n_params:].any()
        assert gw[r, :, :p.n_params].all() and not gw[r, :, p.n_params:].any(), what + ": gpart write set"
        err = np.abs(np.where(gw[r], gp[r], 0.0).astype(np.float64) - ref)
        bound = K * U * maj
        _ratio(key, err, bound)
        bad = err > bound
        assert not bad.any(), "%s r=%d: %d outside the bound, first (block, param) %s: err %.3e bound %.3e" % (
            what, r, int(bad.sum()), tuple(int(v[0]) for v in np.nonzero(bad)), err[bad][0], bound[bad][0])


@pytest.mark.parametrize("H", ox.COMPILED_H)
def test_per_sample_backward(H):
    hip = native.hip()
    for kind, h, N, n_chunks in ox.per_sample_bwd_cases():
        if h != H:
            continue
        c = ox.per_sample_case(kind, H, N, n_chunks)
        assert hip.gen_bwd_lds(H, c.max_in, c.d, c.ps) <= ox.LDS_MAX
        G = hip.gen_bwd_blocks(N)
        prog, th = _dev(c.prog), _params(c.theta)
        xh, nz, gr = _dev(c.xhat), _dev(c.noise), _dev(c.gradp)
        gp = Guarded(c.R, G, c.P)
        hip.gen_bwd(prog.data_ptr(), c.ps, th.data_ptr(), c.P, xh.data_ptr(), nz.data_ptr(), c.NS, gr.data_ptr(),
                    n_chunks, c.R, N, c.D, c.d, H, c.max_in, gp.ptr(), _stream())
        torch.cuda.synchronize()
        g, gw = gp.read()
        _check_gpart(c, g, gw, 128, "gen_bwd", "bwd %s H=%d N=%d chunks=%d" % (kind, H, N, n_chunks))
    print("err/bound so far:", FRACTIONS)


# ---------------------------------------------------------------------------- staged
@pytest.mark.parametrize("kind,H,N,W", ox.staged_cases())
def test_staged_forward_and_backward(kind, H, N, W):
    hip = native.hip()
    c = ox.staged_case(kind, H, N, W)
    R, D, d, NS, P = c.R, c.D, c.d, c.NS, c.P
    sched, ss, _ = pack_schedules(c.progs)
    plan = hip.staged_plan(d, H, c.max_in, W)
    assert plan
    prog, sc, th = _dev(c.prog), _dev(sched), _params(c.theta)
    data = np.zeros((R, D, N), np.float32)
    dat, nz, gr = _dev(data), _dev(c.noise), _dev(c.gradp)
    what = "staged %s H=%d N=%d W=%d" % (kind, H, N, W)
    # forward: the plan's placement and every forced one that fits, bitwise the same
    outs = []
    for force in (-1, 0, 1):
        if force >= 0 and ox.staged_fwd_lds(d, W, H, c.max_in, force == 1) > ox.LDS_MAX:
            continue
        xh, xn = Guarded(R, D, N), Guarded(R, N)
        hip.gen_fwd_staged(prog.data_ptr(), c.ps, sc.data_ptr(), ss, th.data_ptr(), P, dat.data_ptr(), xh.ptr(),
                           nz.data_ptr(), NS, xn.ptr(), N, D, d, H, c.max_in, R, W, _stream(), force=force)
        torch.cuda.synchronize()
        (x, xw), (nrm, nw) = xh.read(), xn.read()
        assert nw.all() and xw[:, :d].all() and not xw[:, d:].any(), what + ": xhat / xnorm write set"
        outs.append((x[:, :d].copy(), nrm.copy()))
    assert len(outs) == 3
    for x, nrm in outs[1:]:
        assert np.array_equal(x.view(np.uint32), outs[0][0].view(np.uint32)), what + ": forward placements differ"
        assert np.array_equal(nrm.view(np.uint32), outs[0][1].view(np.uint32))
    x, nrm = outs[0]
    for r, p in enumerate(c.progs):
        xin = np.zeros((D, N), np.float32)
        xin[:d] = x[r]
        val, bnd, obs, n2, n2b = ox.forward_oracle(p, H, c.theta[r], D, xin, c.noise[r], data[r])
        err = np.abs(x[r].astype(np.float64) - val)
        _ratio("gen_fwd_staged", err, bnd)
        assert np.all(err <= bnd), what + ": forward node value r=%d" % r
        assert np.all(np.abs(nrm[r] - n2) <= n2b)
    # backward from the committed xhat: plan + every forced placement that fits
    T = hip.staged_tiles(N)
    xh = _dev(c.xhat)
    grads = []
    for force in (-1, 0, 1, 2):
        wb = plan[4] if force < 0 else W
        if force >= 0 and ox.staged_bwd_lds(d, wb, H, c.max_in, force >= 1, force == 2) > ox.LDS_MAX:
            continue
        gp = Guarded(R, T, P)
        dxs = torch.zeros(R, d, N, device="cuda")
        hip.gen_bwd_staged(prog.data_ptr(), c.ps, sc.data_ptr(), ss, th.data_ptr(), P, xh.data_ptr(), nz.data_ptr(),
                           NS, gr.data_ptr(), c.n_chunks, R, N, D, d, H, c.max_in, W, gp.ptr(), dxs.data_ptr(),
                           _stream(), force=force)
        torch.cuda.synchronize()
        grads.append(gp.read())
    assert len(grads) == 4
    _check_gpart(c, grads[0][0], grads[0][1], 64, "gen_bwd_staged", what)
    for g, gw in grads[1:]:
        assert np.array_equal(gw, grads[0][1])
        assert np.array_equal(g.view(np.uint32), grads[0][0].view(np.uint32)), what + ": backward placements differ"
    print("err/bound so far:", FRACTIONS)


# ---------------------------------------------------------------------------- Adam, init, finalize, advance
@pytest.mark.parametrize("P", [4, 1024, 1028])
def test_adam(P):
    hip = native.hip()
    lr, b1, b2, eps = 0.01, 0.9, 0.999, 1e-8
    prs = [P, P - 1, P - 3, P]                       # a mixed batch: every padding length
    R = len(prs)
    prog = np.zeros((R, 4), np.int32)
    prog[:, 1] = prs
    exact = 0
    for G in (1, 7, 8, 9):
        for t in (1, 2, 1000):
            rng = np.random.default_rng([P, G, t])
            params = rng.normal(0, 0.5, (R, P)).astype(np.float32)
            m = rng.normal(0, 1e-3, (R, P)).astype(np.float32)
            v = (rng.normal(0, 1e-3, (R, P)) ** 2).astype(np.float32)
            gpart = rng.normal(0, 1e-3, (R, G, P)).astype(np.float32)
            for r in range(R):
                gpart[r, :, prs[r]:] = np.nan         # never written by a backward: must not matter
            th, mm, vv, gp, pg = _params(params), _dev(m), _dev(v), _dev(gpart), _dev(prog)
            step = torch.tensor([77, t - 3], dtype=torch.int32, device="cuda")
            hip.adam(th.data_ptr(), mm.data_ptr(), vv.data_ptr(), gp.data_ptr(), G, pg.data_ptr(), 4,
                     P, step.data_ptr(), 2, lr, b1, b2, eps, R, _stream())
            torch.cuda.synchronize()
            pd, md, vd = th.cpu().numpy(), mm.cpu().numpy(), vv.cpu().numpy()
            for r in range(R):
                Pr = prs[r]
                pn, mn, vn, lr_t, stp = ox.adam_reference(params[r], m[r], v[r], gpart[r], Pr, t, lr, b1, b2, eps)
                what = "adam P=%d Pr=%d G=%d t=%d" % (P, Pr, G, t)
                for a, b, name in ((md[r], mn, "m"), (vd[r], vn, "v")):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what + ": %s bits" % name
                for a, b in ((pd[r], params[r]), (md[r], m[r]), (vd[r], v[r])):
                    assert np.array_equal(a[Pr:].view(np.uint32), b[Pr:].view(np.uint32)), what + ": padding touched"
                same = np.array_equal(pd[r].view(np.uint32), pn.view(np.uint32))
                exact += same
                assert same, what + ": params bits"
                p64, m64, v64, dp, dm, dv = ox.adam_oracle64(params[r].astype(np.float64), m[r].astype(np.float64),
                                                             v[r].astype(np.float64), gpart[r], Pr, t, lr, b1, b2, eps)
                e64 = np.abs(pd[r, :Pr] - p64[:Pr])
                _ratio("adam vs fp64", e64, dp[:Pr])
                assert np.all(e64 <= dp[:Pr]), what + ": params against fp64"
    print("adam P=%d: %d of %d updates bitwise the numpy fp32 evaluation" % (P, exact, 12 * R), FRACTIONS)


def test_init_params():
    hip = native.hip()
    progs = ox.per_sample_batch(7)
    c = ox.make_case(progs, 7, 1, 1)
    R, P = c.R, c.P
    std = 0.05
    th, mm, vv = Guarded(R, P), Guarded(R, P), Guarded(R, P)
    keys, pg = _keys_tensor(KEYS[:R], "cuda"), _dev(c.prog)
    hip.init_params(th.ptr(), mm.ptr(), vv.ptr(), pg.data_ptr(), c.ps, P, keys.data_ptr(), std, R, _stream())
    torch.cuda.synchronize()
    (p, pw), (m, mw), (v, vw) = th.read(), mm.read(), vv.read()
    assert pw.all() and mw.all() and vw.all() and not m.any() and not v.any()
    assert len({q.n_params for q in progs}) == 3
    for r, q in enumerate(progs):
        idx = np.arange(q.n_params, dtype=np.uint32)
        ref, rad = ox.normal_reference(KEYS[r], idx, 0, 0, philox.RNG_PARAM_INIT)
        # the scaling by init_std rounds once more: half a unit at most (|cos| <= 1)
        units = ox.normal_units(p[r, :q.n_params], np.float64(np.float32(std)) * ref, np.float64(np.float32(std)) * rad)
        _record("init units", units.max())
        print("init_params: max %.3f units" % units.max())
        assert units.max() <= NORMAL_UNITS + 1.0
        assert not p[r, q.n_params:].any()


@pytest.mark.parametrize("n_parts", [1, 255, 257])
def test_loss_finalize(n_parts):
    hip = native.hip()
    R, stride = 3, 5
    rng = np.random.default_rng(n_parts)
    lp = rng.normal(0, 1.0, (R, n_parts)).astype(np.float32)
    s64 = lp.astype(np.float64).sum(1)
    sabs = np.abs(lp.astype(np.float64)).sum(1)
    lpd = _dev(lp)
    for flags in (0, 1, 2):
        for tt0, inv in ((0.0, 0.25), (3.7, 1.0 / 49.0)):
            for st in (stride - 1, stride):
                tt, last, acc, hist = Guarded(R), Guarded(R), Guarded(R), Guarded(R, stride)
                tt.t.fill_(tt0)
                acc.t.fill_(1.5)
                step = torch.tensor([1234, st - 2], dtype=torch.int32, device="cuda")
                hip.loss_finalize(lpd.data_ptr(), n_parts, tt.ptr(), last.ptr(), acc.ptr(), inv, flags, hist.ptr(),
                                  stride, step.data_ptr(), 2, R, _stream())
                torch.cuda.synchronize()
                (t_, _), (l_, lw), (a_, _), (h_, hw) = tt.read(), last.read(), acc.read(), hist.read()
                what = "finalize n_parts=%d flags=%d st=%d" % (n_parts, flags, st)
                bound = n_parts * U * sabs
                if flags & 2:
                    err = np.abs(t_ - s64)
                    _ratio("loss_finalize", err, bound)
                    assert np.all(err <= bound), what
                    assert not lw.any() and not hw.any() and np.all(a_ == 1.5), what + ": write set"
                    continue
                assert np.all(t_ == np.float32(tt0)) and lw.all(), what
                L = (s64 + np.float64(np.float32(tt0))) * np.float64(np.float32(inv))
                # tt = 0 and inv = 1/4: the add and the scaling are exact, the bound is the sum's;
                # otherwise two more roundings of at most u each
                bl = bound * inv if tt0 == 0.0 else (bound + 2 * U * (sabs + tt0)) * inv
                err = np.abs(l_ - L)
                _ratio("loss_finalize", err, bl)
                assert np.all(err <= bl), what
                assert np.array_equal(a_, np.float32(1.5) + l_ if flags & 1 else np.full(R, 1.5, np.float32)), what
                want = np.zeros((R, stride), bool)
                if st < stride:
                    want[:, st] = True
                    assert np.array_equal(h_[:, st], l_), what + ": history value"
                assert np.array_equal(hw, want), what + ": history write set"


def test_advance_both_counters():
    hip = native.hip()
    step = torch.tensor([5, 7], dtype=torch.int32, device="cuda")
    for d_rng, d_opt, want in ((3, 0, [8, 7]), (0, 2, [8, 9]), (1, 1, [9, 10])):
        hip.advance(step.data_ptr(), d_rng, d_opt, _stream())
        torch.cuda.synchronize()
        assert step.cpu().tolist() == want
