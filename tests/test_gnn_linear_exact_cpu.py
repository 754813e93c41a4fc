"""The case builders and fp64 references of tests/test_gnn_linear_exact_gpu.py, run
without a GPU: every builder's exactness precondition (sum|terms| / quantum < 2^24, so a
mis-sized input range is caught here), the shape constraints of the launchers, and
self-checks of the references against independent implementations.  Sizes that depend on
the CU count assume 256 CUs."""
import numpy as np
import pytest
import torch

import test_gnn_linear_exact_gpu as lx

F64 = torch.float64
CUS = 256             # MI355X; the big cases are sized from the device on the GPU


def _bf16_rne(x32):
    """bf16 round-to-nearest-even of finite fp32 values by integer arithmetic."""
    u = x32.astype(np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).astype(np.float64)


def test_variant_codes_decode():
    assert lx.decode(-3) == -3 and lx.decode(-1) == -1
    assert lx.decode(1016008) == (lx.WS, 16, 8) and lx.decode(2004161) == (lx.SLAB, 4, 161)
    assert lx.decode(5017021) == (lx.WGT2, 17, 21) and lx.decode(4000000) == (lx.GEMM, 0, 0)


def test_fp16_rounding_helper_is_round_to_nearest_even():
    x = torch.tensor([2049.0, 2051.0, -2049.0, 1 + 2.0 ** -11, 0.0, 1000.25], dtype=F64)
    assert torch.equal(lx._f16r(x), torch.tensor([2048.0, 2052.0, -2048.0, 1.0, 0.0, 1000.0], dtype=F64))
    with pytest.raises(AssertionError):
        lx._f16r(torch.tensor([1 + 2.0 ** -30], dtype=F64))


def test_ym_bit_patterns_and_the_alive_mask():
    rng = np.random.default_rng(0)
    Ym = lx._ym(rng, 64, 40, 48, lx.NAN)
    bits = Ym[:, :40].contiguous().view(torch.int16).numpy().view(np.uint16)
    assert set(np.unique(bits)) == set(lx.YM_BITS)
    assert bool(torch.isnan(Ym[:, 40:].float()).all())
    a = lx.alive(Ym, 40)
    # positive sign and a set magnitude: the subnormal 0x0001 is alive, -0 and 0x8001 are not
    assert torch.equal(a, torch.from_numpy((bits & 0x8000 == 0) & (bits & 0x7fff != 0)))
    assert bool(a[torch.from_numpy(bits == 0x0001)].all()) and not bool(a[torch.from_numpy(bits == 0x8001)].any())
    assert not bool(a[torch.from_numpy(bits == 0x8000)].any()) and not bool(a[torch.from_numpy(bits == 0)].any())
    # bf16 subnormals flush in no comparison here: the float view agrees
    assert torch.equal(a, Ym[:, :40].double() > 0)


@pytest.mark.parametrize("name", sorted(lx.FWD))
def test_forward_cases_are_exact_and_well_formed(name):
    s = lx.FWD[name]
    c = lx.fwd_case(name)
    K1, K2, N, ldy = c["K1"], c["K2"], c["N"], c["ldy"]
    assert c["ld1"] % 8 == 0 and c["ld1"] >= K1 and ldy % 8 == 0 and (K2 == 0 or (K1 % 8 == 0 and c["ld2"] >= K2))
    assert bool((c["X1"][:, K1:] == lx.PAD).all())
    if c.get("tail"):
        nsplit, tk = c["tail"]
        assert nsplit % 4 == 0 and nsplit <= ldy and nsplit <= N and (N - nsplit) % tk == 0
        # the 16-bit padding the tail form must zero (tail_16_bf: the tight form, none)
        assert nsplit % 8 == 4 or ldy > nsplit or name == "tail_16_bf"
    else:
        assert N <= ldy
    if c["idx"] is not None:
        idx = c["idx"].numpy()
        assert len(np.unique(idx)) < len(idx) and bool((np.diff(idx) < 0).any()) and c["X1"].shape[0] > c["n"]
    if s["var"][0] == lx.WS:
        assert K1 % 8 == 0 and K2 % 8 == 0 and K1 + K2 <= 256 and max(N, ldy) <= 256 and not c.get("tail")
        assert (K1 + K2 + 15) // 16 <= s["var"][1] and 32 * s["var"][2] >= max(N, ldy)
    y16, planes, v, absum = lx.fwd_expected(c)            # asserts X W + b
    assert bool((absum >= v.abs() / c["rs"][:, None]).all())
    # against an independent path: numpy fp64, integer-arithmetic bf16
    pre = (c["X"].numpy() @ c["W"].numpy() + c["b"].numpy()) * c["rs"].numpy()[:, None]
    nsplit = c["tail"][0] if c.get("tail") else N
    if not c["fp16"]:
        assert np.array_equal(y16.numpy()[:, :nsplit], np.maximum(_bf16_rne(pre.astype(np.float32)), 0)[:, :nsplit])
    else:
        assert np.array_equal(y16.numpy()[:, :nsplit], np.maximum(pre.astype(np.float16).astype(np.float64), 0)[:, :nsplit])
    assert bool((y16[:, nsplit:] == 0).all())
    if planes is not None:
        P, tk = (N - nsplit) // c["tail"][1], c["tail"][1]
        assert planes.shape == (P, c["n"], tk)
        assert planes[1, 3, tk - 1] == max(pre[3, nsplit + tk + tk - 1], 0)
    if name in lx.DROP_CASES:
        cp = lx.fwd_case(name, posbias=True)
        for p in lx.PS_EXACT + (0.3,):
            keep = lx.keep_mask(cp["n"], N, p)
            out = lx.fwd_expected(cp, p, keep.double())
            assert bool((lx.fwd_expected(cp, p)[2] > 0).all()), "posbias leaves a non-positive pre-activation"
            if p != 0.3:
                assert torch.equal(out[0][:, :nsplit] != 0, keep[:, :nsplit])
                # the scale folded into W' and b' is exact: s * the unscaled output
                base = lx.fwd_expected(cp, 0.0)[2]
                assert torch.equal(out[2], lx.scale32(p) * base * keep)
            else:
                assert out[0] is None


def test_forward_tables_match_their_description():
    assert len(lx.FWD_TABLE) == 12 + 12 + 2 + 2
    assert {lx.table_key(s["var"], s["fp16"]) for s in lx.FWD.values()} == lx.FWD_TABLE
    assert lx.scale32(0.75) == 4.0 and lx.scale32(0.5) == 2.0
    for n in lx.ROW_COUNTS:
        lx.fwd_expected(lx.fwd_case("gemm_odd_h", n=n))
    # the periodic big cases: one period, every p they run
    for p in (0.0, 0.5):
        lx.fwd_expected(lx.fwd_case("ws_8_4_bf", n=lx.PERIOD, posbias=True), p)
    lx.fwd_expected(lx.fwd_case("slab_8_rag_bf", n=lx.PERIOD))


@pytest.mark.parametrize("nt", lx.WS_NTS)
def test_ws_row_counts_give_the_tiles_per_block(nt):
    for grid in (CUS, 3 * CUS):
        n = lx.ws_rows(grid, nt)
        tiles = (n + 31) // 32
        g = min(grid, tiles)
        per_block = [(tiles - 1 - b) // g + 1 for b in range(g)]
        assert n % 32 and per_block[0] == per_block[1] == nt and set(per_block[2:]) <= {nt - 1}
    assert {t % lx.WS_RING for t in lx.WS_NTS} == {0, 1, 2}


@pytest.mark.parametrize("name", sorted(lx.BWD))
def test_data_backward_cases_are_exact_and_well_formed(name):
    s = lx.BWD[name]
    c = lx.bwd_case(name)                                 # asserts dY W^T
    N, K1, K2 = c["N"], c["K1"], c["K2"]
    assert c["ldd"] % 8 == 0 and c["ldd"] >= N and (K2 == 0 or K1 % 8 == 0)
    if s["var"][0] == lx.WS:
        assert N % 8 == 0 and not s.get("f32") and K1 + K2 <= 32 * s["var"][2] and (N + 15) // 16 <= s["var"][1]
    a = lx.alive(c["Ym"], N)
    assert torch.equal(c["acc"], (c["dY"][:, :N] * a) @ c["W"].t())
    for ms in lx.MSCALES:
        for f32 in (False, True):
            d = lx.bwd_expected(c, ms, f32=f32)
            # ONE fp32 multiply by rs * mscale, then one bf16 rounding -- by numpy
            t = c["acc"].numpy().astype(np.float32) * (c["rs"].numpy().astype(np.float32) * np.float32(ms))[:, None]
            assert np.array_equal(d.numpy(), t.astype(np.float64) if f32 else _bf16_rne(t))
    # the order of the roundings matters at the inexact scale: bf16(g * mscale) first (the
    # CPU branch of gnn/linear.py) is a different function
    ms = lx.MSCALES[2]
    other = (lx._bf16r(lx._mul32(c["dY"][:, :N], ms)) * a) @ c["W"].t()
    assert not torch.equal(lx._bf16r(other) * c["rs"][:, None], lx.bwd_expected(c, ms))


def test_data_backward_tables_match_their_description():
    assert {lx.table_key(s["var"]) for s in lx.BWD.values()} == lx.BWD_TABLE and len(lx.BWD_TABLE) == 11
    halves = {(s["N"] // 8) & 1 for s in lx.BWD.values() if s["N"] % 8}
    assert halves == {0, 1}                               # the straddling chunk in either half
    for name in ("ws_4_4", "slab_16_f32"):
        lx.bwd_case(name, n=lx.PERIOD)


@pytest.mark.parametrize("name", sorted(lx.WGT))
def test_weight_backward_cases_are_exact_and_well_formed(name):
    c = lx.wgt_case(name)
    K1, K2, N = c["K1"], c["K2"], c["N"]
    KT, NB = c["ktnb"]
    kt = (K1 + K2 + 31) // 32
    assert kt <= KT and (K2 == 0 or K1 % 8 == 0) and (KT, NB) in lx.WGT_LIST
    a = lx.alive(c["Ym"], N)
    for mask in (True, False):
        for ms in lx.MSCALES:
            dW, db = lx.wgt_expected(c, ms, mask)         # asserts the sums
            g = _bf16_rne(c["dY"][:, :N].numpy().astype(np.float32) * np.float32(ms))
            if mask:
                g = g * a.numpy()
            assert np.array_equal(dW.numpy(), c["X"].numpy().T @ g) and np.array_equal(db.numpy(), g.sum(0))
    cn = lx.wgt_case(name, fill=lx.NAN)
    assert bool(torch.isfinite(lx.wgt_expected(cn, 2.0, True)[0]).all())


def test_weight_backward_tables_and_sizes():
    assert len(lx.WGT) == len(lx.WGT_LIST) == 18 and {s["ktnb"] for s in lx.WGT.values()} == set(lx.WGT_LIST)
    below = {((s["K1"] + s["K2"] + 31) // 32, s["ktnb"][0]) for s in lx.WGT.values()}
    assert {(3, 4), (6, 8), (7, 8), (10, 12), (13, 16)} <= below
    assert {((s["K1"] + s["K2"] + 1) * s["N"]) % 4 == 0 for s in lx.WGT.values()} == {True, False}
    base = lx.wgt_case("8_4", period=lx.PERIOD)
    for tpc in (1, 2, 3, 4, 5):
        n = lx.wgt_rows(CUS, tpc)
        tiles = (n + 31) // 32
        assert n % 32 and (tiles + CUS - 1) // CUS == tpc and tiles > CUS * (tpc - 1)
        lx.wgt_expected(base, 2.0, True, *divmod(n, lx.PERIOD))      # exact at the largest n too
    n = 32 * (CUS + 1) - 13
    lx.wgt_expected(base, 2.0, True, *divmod(n, lx.PERIOD))
    # the periodic total is the sum over the rows it stands for
    reps, last = divmod(2 * lx.PERIOD + 17, lx.PERIOD)
    dW, db = lx.wgt_expected(base, 1.0, False, reps, last)
    rows = torch.arange(2 * lx.PERIOD + 17) % lx.PERIOD
    assert torch.equal(dW, base["X"][rows].t() @ base["dY"][rows][:, :base["N"]])
    assert torch.equal(db, base["dY"][rows][:, :base["N"]].sum(0))
