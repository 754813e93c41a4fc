"""The case builders and fp64 references of tests/test_gnn_dense_exact_gpu.py, run
without a GPU: every builder's exactness precondition (sum|terms| / quantum < 2^24, so a
mis-sized input range is caught here) and self-checks of the reference helpers against
independent implementations."""
import numpy as np
import pytest
import torch

import test_gnn_dense_exact_gpu as dx
from cgnn_amd.gnn import ops

F64 = torch.float64
CUS = 256             # MI355X; the big cases are sized from the device's CU count on the GPU


def _bf16_rne_bits(x32):
    """bf16 round-to-nearest-even of finite fp32 values by integer arithmetic."""
    u = x32.astype(np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def test_bf16_rounding_helper_is_round_to_nearest_even():
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 257.0, 259.0, 0.0, 300.25], dtype=F64)
    exp = torch.tensor([1.0, 1 + 2.0 ** -6, -1.0, 256.0, 260.0, 0.0, 300.0], dtype=F64)
    assert torch.equal(dx._bf16r(ties), exp)
    rng = np.random.default_rng(0)
    x = (rng.integers(-2 ** 20, 2 ** 20, 4096) / 4.0).astype(np.float32)
    assert np.array_equal(dx._bf16r(torch.from_numpy(x).double()).numpy(), _bf16_rne_bits(x).astype(np.float64))
    with pytest.raises(AssertionError):
        dx._bf16r(torch.tensor([1 + 2.0 ** -30], dtype=F64))


def test_fp32_scale_and_multiply_helpers():
    assert dx.scale32(0.0) == 1.0 and dx.scale32(0.5) == 2.0
    s = dx.scale32(0.3)
    assert float(np.float32(s)) == s and abs(s * 0.7 - 1) < 2.0 ** -22
    x = torch.tensor([3.0, -0.75, 301.5], dtype=F64)
    got = dx._mul32(x, s).numpy()
    assert np.array_equal(got, (x.numpy().astype(np.float32) * np.float32(s)).astype(np.float64))
    assert not np.array_equal(got, x.numpy() * s)        # fp32 product, not the fp64 one


def test_exact_sum_precondition_rejects_missized_ranges():
    dx.assert_exact_sums(torch.tensor([2.0 ** 22 - 0.25]), 0.25, "ok")
    with pytest.raises(AssertionError):
        dx.assert_exact_sums(torch.tensor([2.0 ** 22]), 0.25, "too large")


@pytest.mark.parametrize("p", [0.5, 0.3])
@pytest.mark.parametrize("HD,n", [(128, 1), (256, 33), (128, 77)])
def test_keep_image_codec_round_trips(p, HD, n):
    keep = ops.dropout_keep_mask(n, HD, p, dx.KEY, dx.STEP, 64)
    img = dx.encode_keep_image(keep, HD)
    assert img.numel() == (n + 31) // 32 * (HD // 32) * 64
    assert torch.equal(dx.decode_keep_image(img, n, HD), keep)
    # one element by the documented formula: row 32 T + r, unit 32 t + 8 g + 4 uh + i
    r, t, g, uh, i = (n - 1) % 32, HD // 32 - 1, 2, 1, 3
    T = (n - 1) // 32
    hw = int(img[(T * (HD // 32) + t) * 64 + 32 * uh + r]) & 0xffff
    assert bool((hw >> (4 * g + i)) & 1) == bool(keep[32 * T + r, 32 * t + 8 * g + 4 * uh + i])


@pytest.mark.parametrize("F,ldx,C,ldc", dx.FWD_CASES)
def test_forward_cases_are_exact(F, ldx, C, ldc):
    assert ldx % 8 == 0 and ldx >= F and ldc % 8 == 0 and C <= ldc <= 64
    for HD in (256, 128):
        c = dx.fwd_case(dx.FWD_N, F, ldx, C, ldc, HD)          # asserts P1 + b1
        assert bool((c["AX"][:, F:] == dx.PAD).all())
        # the reference of H1 against an independent path: numpy fp64, integer-arithmetic bf16
        P1 = c["AX"][:, :F].numpy() @ c["W1"].numpy() + c["b1"].numpy()
        Hu = np.maximum(_bf16_rne_bits(P1.astype(np.float32)), 0).astype(np.float64)
        assert np.array_equal(c["Hu"].numpy(), Hu)
        for p in dx.PS:
            keep = dx.keep_mask(dx.FWD_N, HD, p, 0) if p > 0 else None
            H1, Z2, zraw, zabs = dx.fwd_expected(c, p, keep)   # asserts H1 W2 for p in {0, 1/2}
            assert (Z2 is None) == (p == 0.3)
            if Z2 is not None:
                assert bool((Z2[:, C:] == 0).all())
                zr, _ = dx.z2_from_h1(c, p, H1)                # the stored-H1 path reproduces it
                assert torch.equal(dx._bf16r(zr), Z2[:, :C])
            assert bool((zabs >= zraw.abs()).all())


def test_forward_big_case_is_exact_and_sized():
    n = dx.fwd_big_n(CUS)
    tiles, waves = (n + 31) // 32, 16 * CUS
    assert n % 32 and 2 * waves < tiles < 3 * waves            # 2 or 3 tiles per wave, partial last
    c = dx.fwd_big_case()
    for p in (0.0, 0.5):
        dx.fwd_expected(c, p, None)                            # every unit kept: bounds any mask
    for lo, hi in dx.big_mask_ranges(n, CUS):
        assert 0 <= lo < hi <= n
    assert dx.big_mask_ranges(n, CUS)[-1][1] == n


@pytest.mark.parametrize("n", dx.BWD_NS)
def test_dense_bwd_cases_are_exact(n):
    for HD in (128, 256):
        for C, ldc in dx.BWD_CLASSES:
            c = dx.bwd_case(n, C, ldc, HD)                     # asserts dY2 W2^T
            bits = c["H1"].view(torch.int16)
            assert bool(((bits == -32768) & ~c["alive"]).any()) or n == 1      # -0 is not alive
            assert torch.equal(c["alive"], (bits > 0))         # positive sign, non-zero magnitude
            for p in dx.PS:
                d = dx.bwd_expected(c, p)
                assert bool((d[~c["alive"]] == 0).all())
                if p == 0.5:
                    assert torch.equal(d, dx._bf16r(2 * c["dh"]) * c["alive"])


@pytest.mark.parametrize("ks", sorted(dx.FUSED_F))
def test_fused_bwd_cases_are_exact(ks):
    n = max(dx.FUSED_NS)                                       # the bounds grow with n
    for F in dx.FUSED_F[ks]:
        for ldx in sorted({dx.tight(F + 1), 128}):
            for C, ldc in dx.FUSED_CLASSES:
                c = dx.fused_case(n, F, ldx, C, ldc, 256)
                assert bool((c["AX"][:, F] == 1).all()) and bool((c["AX"][:, F + 1:] == 0).all())
                slabs3, total = dx.fused_expected(c, 0.0, None, 3)             # asserts gW1 / gW2
                slabs1, total1 = dx.fused_expected(c, 0.0, None, 1)
                assert torch.equal(slabs3.sum(0), slabs1[0])
                # the totals against the direct products
                Hk = c["Hu"]
                D = c["dhb"] * (Hk > 0)
                assert torch.equal(total[0], c["AX"][:, :F].t() @ D)
                assert torch.equal(total[1], D.sum(0))
                assert torch.equal(total[2], Hk.t() @ c["dY2"][:, :C])
                kf = dx.fused_width(F) - 64
                assert bool((slabs1[0][:, F + 1:kf] == 0).all()) and bool((slabs1[0][:, kf + C:] == 0).all())
                assert dx.fused_expected(c, 0.3, dx.keep_mask(n, 256, 0.3, 0), 3)[1] is None


def test_fused_bwd_table_matches_its_description():
    assert len(dx.FUSED_TABLE) == 10
    for ks, fs in dx.FUSED_F.items():
        assert all((F + 1 + 15) // 16 == ks for F in fs)
    assert {(C + 15) // 16 for C, _ in dx.FUSED_CLASSES} == {3, 4}
    assert dx.fused_width(100) == 192 and dx.fused_width(47) == 128 and dx.fused_width(127) == 192


def test_fused_bwd_big_case_is_exact_and_sized():
    n = dx.fused_big_n(CUS)
    tiles = (n + 31) // 32
    assert n % 32 and 3 * CUS < tiles < 4 * CUS                # 3 or 4 tiles per block, partial last
    c = dx.fused_case(n, 100, 104, 47, 48, 256)
    dx.fused_expected(c, 0.5, None, CUS)                       # every unit kept: bounds any mask
