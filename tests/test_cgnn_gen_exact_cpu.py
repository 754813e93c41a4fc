"""CPU half of the CGNN generator / Adam oracle suite (tests/cgnn_gen_oracle.py):

1. the fp64 oracle against ``ReferenceTrainer.generate`` and torch autograd (1e-12);
2. a numpy fp32 emulation in the kernels' summation order inside the derived bounds;
3. seven deliberate errors of that emulation outside them (the GPU tests could fail);
4. the ReLU-margin condition on exactly the inputs the GPU tests launch, no case left out;
5. the host-side selection codes of ``_hip`` that return before any HIP call.
"""
import re

import numpy as np
import pytest
import torch

import cgnn_gen_oracle as ox
from cgnn_amd import native
from cgnn_amd.engine.reference import ReferenceTrainer
from cgnn_amd.utils import philox

U = ox.U


def _autograd_case(prog, H, N, seed):
    rng = np.random.default_rng(seed)
    d = prog.n_vars
    data = rng.standard_normal((d, N))
    key = philox.model_key(seed, "ox")
    ref = ReferenceTrainer([prog], [data], [key], H)
    theta = torch.as_tensor(rng.normal(0, 0.6, prog.n_params)).requires_grad_(True)
    x = ref.generate(0, theta, step=3)                       # [d, N]
    gout = torch.as_tensor(rng.standard_normal((d, N)))
    (g,) = torch.autograd.grad((x * gout).sum(), theta)
    # the same noise the reference drew, as the kernels' noise buffer [NS, N]
    D = d
    noise = np.zeros((D + prog.n_conf, N))
    n = np.arange(N, dtype=np.uint32)
    for v in range(d):
        noise[v] = philox.normal(key[0], key[1], n, v, 3, philox.RNG_NODE_NOISE, dtype=np.float64)
    for c in range(prog.n_conf):
        noise[D + c] = philox.normal(key[0], key[1], n, c, 3, philox.RNG_CONF_NOISE, dtype=np.float64)
    return data, theta.detach().numpy(), x.detach().numpy(), gout.numpy(), g.numpy(), noise, D


@pytest.mark.parametrize("name", ["chain", "diamond", "pair", "confounded4"])
def test_oracle_matches_reference_and_autograd(name):
    H, N = 5, 37
    prog = getattr(ox, name)(H)
    data, theta, x, gout, g, noise, D = _autograd_case(prog, H, N, 5)
    val, bnd, obs, xn, xnb = ox.forward_oracle(prog, H, theta, D, x, noise, data)
    np.testing.assert_allclose(val, x, rtol=0, atol=1e-12)
    assert obs.sum() == (1 if name == "pair" else 0)
    # the oracle keeps the dtype it is given: fp64 inputs stay fp64 (astype is a no-op)
    out, maj, written = ox.backward_oracle(prog, H, theta, D, x, noise, gout[None], 16, prog.n_params)
    assert written.all()
    np.testing.assert_allclose(out.sum(0), g, rtol=0, atol=1e-12)
    assert np.all(np.abs(out) <= maj * (1 + 1e-12))


EMU = [("batch", 3, 65, 3), ("batch", 20, 129, 1), ("fan", 5, 65, 3), ("fan", 64, 129, 1), ("batch", 50, 1, 3)]


def _bwd_errs(c, BS, mut=None, r_only=None):
    """max over models of (|emulation - oracle| / bound) and whether any element is outside."""
    worst, outside = 0.0, False
    K = ox.backward_K(BS, c.depth, c.max_in, c.H)
    for r, p in enumerate(c.progs):
        ref, maj, written = ox.backward_oracle(p, c.H, c.theta[r], c.D, c.xhat[r], c.noise[r], c.gradp[:, r], BS, c.P)
        emu = ox.backward_emulate(p, c.H, c.theta[r], c.D, c.xhat[r], c.noise[r], c.gradp[:, r], BS, c.P, mut)
        err = np.abs(emu.astype(np.float64) - ref)
        bound = K * U * maj
        outside |= bool((err > bound).any())
        m = bound > 0
        worst = max(worst, float((err[m] / bound[m]).max()))
        assert np.all(emu[:, ~written] == 0)
    return worst, outside


@pytest.mark.parametrize("kind,H,N,n_chunks", EMU)
@pytest.mark.parametrize("BS", [128, 64])
def test_backward_emulation_within_bound(kind, H, N, n_chunks, BS):
    c = ox.per_sample_case(kind, H, N, n_chunks)
    worst, outside = _bwd_errs(c, BS)
    print("backward emulation err/bound: %.4f" % worst)
    assert not outside


@pytest.mark.parametrize("mut", ["drop_sample", "flip_mask", "b1_row", "conf_shift", "swap_parents", "omit_chunk"])
@pytest.mark.parametrize("BS", [128, 64])
def test_backward_mutations_outside_bound(mut, BS):
    c = ox.make_case(ox.per_sample_batch(6), 6, 65, 3, extra_noise_rows=1)
    assert _bwd_errs(c, BS)[1] is False
    assert _bwd_errs(c, BS, mut)[1] is True


@pytest.mark.parametrize("H", [1, 7, 20, 64])
def test_forward_emulation_and_mutations(H):
    N = 65
    progs = ox.per_sample_batch(H)
    c = ox.make_case(progs, H, N, 1, extra_noise_rows=1)
    theta = ox.forward_params(progs, c.P, 3)
    rng = np.random.default_rng(H)
    noise = rng.standard_normal(c.noise.shape).astype(np.float32)
    data = rng.standard_normal((c.R, c.D, N)).astype(np.float32)
    for r, p in enumerate(progs):
        for mut in (None, "swap_parents", "conf_shift"):
            x, nrm = ox.forward_emulate(p, H, theta[r], c.D, noise[r], data[r], mut)
            val, bnd, obs, xn, xnb = ox.forward_oracle(p, H, theta[r], c.D, x, noise[r], data[r])
            err = np.abs(x[:c.d].astype(np.float64) - val)
            applies = (mut == "swap_parents" and r != 2) or (mut == "conf_shift" and r == 2) or \
                      (mut == "swap_parents" and r == 2)
            if mut is None:
                assert np.all(err <= bnd) and np.all(err[obs] == 0)
                assert np.all(np.abs(nrm - xn) <= xnb)
            elif applies:
                assert (err > bnd).any(), (r, mut)


@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adam_emulation_and_beta2_mutation(t):
    rng = np.random.default_rng(t)
    P, Pr, G = 1028, 1025, 9
    params, m = rng.normal(0, 0.5, P).astype(np.float32), rng.normal(0, 1e-3, P).astype(np.float32)
    v = (rng.normal(0, 1e-3, P) ** 2).astype(np.float32)
    gpart = rng.normal(0, 1e-3, (G, P)).astype(np.float32)
    args = (params, m, v, gpart, Pr, t, 0.01, 0.9, 0.999, 1e-8)
    pn, mn, vn, lr_t, step = ox.adam_reference(*args)
    p64, m64, v64, dp, dm, dv = ox.adam_oracle64(params.astype(np.float64), m.astype(np.float64),
                                                 v.astype(np.float64), gpart, *args[4:])
    assert np.all(np.abs(pn - p64) <= dp) and np.all(np.abs(mn - m64) <= dm) and np.all(np.abs(vn - v64) <= dv)
    assert np.array_equal(pn[Pr:], params[Pr:]) and np.array_equal(mn[Pr:], m[Pr:])
    bad = ox.adam_reference(*args, mut="beta2_t-1")[0]
    assert (np.abs(bad - p64) > dp).any()


def test_relu_margin_of_every_committed_backward_input():
    """Exactly the inputs tests/test_cgnn_gen_exact_gpu.py launches, no case left out."""
    n = 0
    for kind, H, N, n_chunks in ox.per_sample_bwd_cases():
        c = ox.per_sample_case(kind, H, N, n_chunks)
        for r, p in enumerate(c.progs):
            assert ox.relu_margin_ok(p, H, c.theta[r], c.D, c.xhat[r], c.noise[r]), (kind, H, N, r)
            n += 1
    for kind, H, N, W in ox.staged_cases():
        c = ox.staged_case(kind, H, N, W)
        for r, p in enumerate(c.progs):
            assert ox.relu_margin_ok(p, H, c.theta[r], c.D, c.xhat[r], c.noise[r]), (kind, H, N, r)
            n += 1
    assert n > 300


def test_committed_cases_reach_every_branch():
    """Both reduction shapes at every H that has both, PPR on and off, both CW, every fwd_hc."""
    for H in ox.COMPILED_H:
        p = ox.fan(H)
        hp = ((H + 1) & ~1) // 2
        items = sorted({(nin + 1) * hp + 1 for _, kind, _, _, _, nin in p.node_records()})
        assert items[-1] > 64
        assert (items[0] <= 64) == (H < 64)
        if H < 48:
            assert 64 - hp < max(i for i in items if i <= 64) <= 64       # right at the threshold
    assert {ox.staged_fwd_hc(H) for H in ox.STAGED_H} == {32, 20, 16, 12, 10, 8, 6, 5, 4, 3, 2, 1}
    assert {ox.staged_cw(H) for _, H, _, _ in ox.staged_cases()} == {12, 16}
    mi = {k: ox.staged_case(k, 4, 1, 1).max_in for k in ("narrow", "big", "conf")}
    assert mi["narrow"] == 4 and mi["big"] >= 18 and mi["conf"] <= 17
    assert {W for _, _, _, W in ox.staged_cases() if _ != "x"} == {1, 2, 8}


# ---------------------------------------------------------------------------- host-side codes
def test_gen_bwd_variant_boundaries():
    hip = native.hip()
    # 24 / 25 variables: the per-sample kernels up to GEN_PER_SAMPLE_MAX_D, then the staged ones
    assert hip.gen_bwd_variant(20, 4, 24, 256) == 1
    assert hip.gen_bwd_variant(20, 4, 25, 256) == 2
    # an H the per-sample backward does not compile: staged whatever the size
    assert hip.gen_bwd_variant(7, 4, 5, 64) == 2
    # the per-sample LDS limit (160 KiB): bytes from the launcher's own query
    for H, max_in in ((20, 4), (64, 3)):
        d = 1
        while hip.gen_bwd_lds(H, max_in, d + 1, 0) <= ox.LDS_MAX:
            d += 1
        assert hip.gen_bwd_lds(H, max_in, d, 0) <= ox.LDS_MAX < hip.gen_bwd_lds(H, max_in, d + 1, 0)
        assert d > 24 and hip.gen_bwd_variant(H, max_in, d, 0) == 2     # staged wins above 24 when it fits
    he = lambda H: (H + 1) & ~1
    for H, max_in, d in ((1, 1, 1), (5, 7, 9), (64, 62, 24)):
        want = 4 * (128 * (he(H) + ((max_in + 2) | 1) + 2 * d) + 128 + (max_in + 1) * he(H))
        assert hip.gen_bwd_lds(H, max_in, d, 0) == want
    assert hip.gen_fwd_lds(64, 100) == 4 * (64 * 256 + 100)
    assert hip.gen_fwd_lds(65, 100) == 4 * (65 * 128 + 100)
    assert hip.gen_fwd_lds(128, 0) == 4 * 128 * 128 and hip.gen_fwd_lds(129, 0) == 4 * 129 * 64


def test_staged_plan_boundaries():
    hip = native.hip()
    assert hip.staged_plan(0, 20, 4, 4) == () and hip.staged_plan(34, 0, 4, 4) == ()
    assert hip.staged_plan(34, 20, 4, 0) == () and hip.staged_plan(34, 20, 4, 9) == ()
    assert hip.staged_plan(34, 20, 4, 4, -1) == ()
    for H, max_in, W in ((20, 4, 8), (16, 19, 2), (5, 4, 1), (36, 12, 4)):
        prev = None
        for d in range(1, 700):
            plan = hip.staged_plan(d, H, max_in, W)
            assert plan and plan[3] == W and plan[4] == min(W, 2)
            # forward: LDS state while it fits
            assert plan[0] == int(ox.staged_fwd_lds(d, W, H, max_in, False) > ox.LDS_MAX)
            # backward: the placement with the most resident waves (16 at most), ties keep LDS
            waves = [min(16, ox.LDS_MAX // ox.staged_bwd_lds(d, plan[4], H, max_in, pl >= 1, pl == 2) * plan[4])
                     if ox.staged_bwd_lds(d, plan[4], H, max_in, pl >= 1, pl == 2) <= ox.LDS_MAX else 0
                     for pl in range(3)]
            best = waves.index(max(waves))
            assert (plan[1], plan[2]) == (int(best >= 1), int(best == 2)), (H, max_in, W, d, plan, waves)
            prev = plan
        assert prev[1] == 1                                   # 699 variables: x in global memory
    assert hip.staged_plan(34, 20, 4000, 1) == ()              # absurd max_in: not even all-global
    assert hip.staged_tiles(1) == 1 and hip.staged_tiles(64) == 1 and hip.staged_tiles(65) == 2
    assert hip.gen_bwd_blocks(128) == 1 and hip.gen_bwd_blocks(129) == 2


P_ = 64         # a non-null pointer, never dereferenced: every row returns before any HIP call

REJECT = [
    # gen_bwd: prog ps params P xhat noise NS gradp nch R N D Dt H max_in gpart st
    ("gen_bwd H = 7", "gen_bwd", (P_, 64, P_, 64, P_, P_, 8, P_, 1, 1, 8, 8, 5, 7, 3, P_, 0), -1),
    ("gen_bwd H = 25", "gen_bwd", (P_, 64, P_, 64, P_, P_, 8, P_, 1, 1, 8, 8, 5, 25, 3, P_, 0), -1),
    ("gen_bwd LDS", "gen_bwd", (P_, 64, P_, 64, P_, P_, 512, P_, 1, 1, 8, 512, 400, 20, 3, P_, 0), -2),
    # gen_fwd: prog ps params P data xhat noise NS xnorm keys step off N D H R st row0
    ("gen_fwd LDS", "gen_fwd", (P_, 64, P_, 64, P_, P_, P_, 1024, 0, P_, P_, 0, 8, 1024, 20, 1, 0, 0), -2),
    # adam: params m v gpart G prog ps P step off lr b1 b2 eps R st
    ("adam P % 4", "adam", (P_, P_, P_, P_, 1, P_, 64, 1026, P_, 0, 0.01, 0.9, 0.999, 1e-8, 1, 0), -3),
    # gen_noise: prog ps keys step off noise NS N D Dt R row0 st
    ("gen_noise NS < D", "gen_noise", (P_, 64, P_, P_, 0, P_, 7, 8, 8, 5, 1, 0, 0), -2),
    ("gen_noise Dt > D", "gen_noise", (P_, 64, P_, P_, 0, P_, 8, 8, 8, 9, 1, 0, 0), -2),
    # gen_fwd_staged: prog ps sched ss params P data xhat noise NS xnorm N D Dt H max_in R W st force
    ("gen_fwd_staged W = 9", "gen_fwd_staged",
     (P_, 64, P_, 64, P_, 64, P_, P_, P_, 48, 0, 8, 48, 34, 20, 4, 1, 9, 0, -1), -2),
    ("gen_fwd_staged forced LDS", "gen_fwd_staged",
     (P_, 64, P_, 64, P_, 64, P_, P_, P_, 768, 0, 8, 768, 700, 20, 4, 1, 1, 0, 0), -2),
    # gen_bwd_staged: prog ps sched ss params P xhat noise NS gradp nch R N D Dt H max_in W gpart dxs st force
    ("gen_bwd_staged W = 0", "gen_bwd_staged",
     (P_, 64, P_, 64, P_, 64, P_, P_, 48, P_, 1, 1, 8, 48, 34, 20, 4, 0, P_, P_, 0, -1), -2),
    ("gen_bwd_staged forced LDS", "gen_bwd_staged",
     (P_, 64, P_, 64, P_, 64, P_, P_, 768, P_, 1, 1, 8, 768, 700, 20, 4, 1, P_, P_, 0, 0), -2),
    ("gen_bwd_staged forced x global does not fit either", "gen_bwd_staged",
     (P_, 64, P_, 64, P_, 64, P_, P_, 768, P_, 1, 1, 8, 768, 700, 20, 4, 1, P_, P_, 0, 1), -2),
    ("gen_bwd_staged global dL/dx without scratch", "gen_bwd_staged",
     (P_, 64, P_, 64, P_, 64, P_, P_, 768, P_, 1, 1, 8, 768, 700, 20, 4, 1, P_, 0, 0, 2), -2),
]


@pytest.mark.parametrize("name,args,code", [pytest.param(n, a, c, id=i) for i, n, a, c in REJECT])
def test_launcher_refuses_before_launching(name, args, code):
    assert ox.staged_bwd_lds(700, 1, 20, 4, True, False) > ox.LDS_MAX > ox.staged_bwd_lds(700, 1, 20, 4, True, True)
    with pytest.raises(RuntimeError) as err:
        getattr(native.hip(), name)(*args)
    assert re.search(r"\(code %d\)" % code, str(err.value)), str(err.value)


def test_normal_reference_is_the_mirror_up_to_the_uniform_rounding():
    """philox.normal keeps the half of u01 in fp64, the device rounds it away from 2^23 on."""
    key = philox.model_key(3, "nr")
    n = np.arange(4096, dtype=np.uint32)
    z, rad = ox.normal_reference(key, n, 2, 5, philox.RNG_NODE_NOISE)
    m = philox.normal(key[0], key[1], n, 2, 5, philox.RNG_NODE_NOISE, dtype=np.float64)
    # du <= 2^-25 on both uniforms: |dz| <= 2^-25 / (u1 rad) + 2 pi 2^-25 rad
    r0 = philox.philox4x32_10(n, 2, 5, philox.RNG_NODE_NOISE, key[0], key[1])[0]
    u1 = philox.u01(r0)
    assert np.all(np.abs(z - m) <= 2.0 ** -25 / (u1 * rad) + 2 * np.pi * 2.0 ** -25 * rad + 1e-15)
    assert np.abs(z - m).max() > 0
    x = np.array([0, 255, 256, 2 ** 31, 2 ** 32 - 1], np.uint32)
    assert np.all(ox.u01_f32(x) > 0) and ox.u01_f32(x)[-1] == 1.0 and ox.u01_f32(x)[0] == 2.0 ** -25
