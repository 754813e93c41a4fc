"""The case builders and fp64 references of tests/test_gat_exact_gpu.py, run without a GPU:
every builder's precondition (sum|terms| / quantum < 2^24, the distance of the raw scores from
the LeakyReLU kink, the score patterns), the agreement of the documented shape rule with the
library's host-side variant query, and self-checks of the references against fp64 autograd of
an independent dense formulation."""
import numpy as np
import pytest
import torch

import test_gat_exact_gpu as gx
from cgnn_amd import native

F64 = torch.float64


def test_rule_and_query_agree_for_every_shape():
    hip = native.hip()
    seen = set()
    for K in range(1, 65):
        for Fh in range(8, 513, 8):
            v = hip.gnn_gat_variant(K, Fh)
            if gx.rule(K, Fh):
                assert v == gx.expected_variant(K, Fh), (K, Fh, v)
                seen.add(v)
            else:
                assert v == -3, (K, Fh, v)
    assert seen == gx.TABLE and len(seen) == 22
    for K, Fh in ((1, 4), (1, 12), (2, 24), (0, 8), (-1, 8), (1, 0), (1, -8), (1, 520), (65, 8), (2 ** 20, 2 ** 20)):
        assert hip.gnn_gat_variant(K, Fh) == -3
    # the four pairs that used to be missing, by the examples of their shapes
    assert {hip.gnn_gat_variant(*s) for s in ((17, 8), (32, 8), (33, 8), (64, 8), (17, 16), (32, 16), (2, 256))} \
        == gx.FORMERLY_MISSING


def test_python_guards_are_the_rule():
    from cgnn_amd.gnn.gat_fused import FusedGAT
    for K in (1, 2, 3, 17, 33, 64):
        for Fh in (8, 16, 24, 32, 48, 256, 512):
            if (K * Fh) % 32 == 0:
                assert FusedGAT.supported(64, K, Fh, 7) == gx.rule(K, Fh), (K, Fh)


def test_shapes_table_and_graphs():
    assert {c for _, _, c in gx.SHAPES} == gx.TABLE
    assert all(gx.rule(K, Fh) and gx.expected_variant(K, Fh) == c for K, Fh, c in gx.SHAPES)
    for L in (8, 16, 32, 64):
        g = gx.graph(L)
        deg = set(g["deg"].tolist())
        assert {0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 5, 4099, 4096} <= deg
        assert g["col"].min() == 0 and g["col"].max() == gx.N_SRC - 1 and g["n"] != gx.N_SRC
        assert any(len(set(g["col"][a:b])) < b - a for a, b in zip(g["rp"][:-1], g["rp"][1:]))
        # the transposed CSR: the same edge multiset, destinations increasing, long rows
        rpt, colt = g["rpt"], g["colt"]
        srow = np.repeat(np.arange(gx.N_SRC), np.diff(rpt))
        assert sorted(zip(colt.tolist(), srow.tolist())) == sorted(zip(g["rows"].tolist(), g["col"].tolist()))
        assert all(np.all(np.diff(colt[a:b]) >= 0) for a, b in zip(rpt[:-1], rpt[1:]))
        assert np.diff(rpt).max() > 4 * 64 and np.diff(rpt).min() < 64
        gr = gx.graph(L, None, True)
        assert np.array_equal(gr["deg"], g["deg"][::-1])
        assert np.array_equal(gr["col"][:gr["rp"][1]], g["col"][g["rp"][-2]:])
        for order, sign in (("asc", 1), ("desc", -1)):
            go = gx.graph(L, order)
            assert np.array_equal(go["rp"], g["rp"])
            assert all(np.all(sign * np.diff(gx.RANK[go["col"][a:b]]) >= 0) for a, b in zip(go["rp"][:-1], go["rp"][1:]))
            assert all(sorted(go["col"][a:b]) == sorted(g["col"][a:b]) for a, b in zip(g["rp"][:-1], g["rp"][1:]))


def test_rounding_helpers():
    x = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.0, 3.0])
    assert np.array_equal(gx.bf16r(x), [1.0, 1 + 2.0 ** -6, -1.0, 0.0, 3.0])
    assert gx.f32(np.array([1 + 2.0 ** -30]))[0] == 1.0
    d = gx.dyadic(np.random.default_rng(0), (1000,), 8, 4)
    assert np.array_equal(d * 8, np.round(d * 8)) and d.min() == -4 and d.max() == 4


@pytest.mark.parametrize("case", gx.CASES, ids=gx._id)
def test_exact_builders_hold_their_budgets(case):
    K, Fh, wbf = case
    for mode in ("zero", "const"):
        c = gx.exact_fwd_case(K, Fh, wbf, mode)
        g = c["g"]
        assert np.all(c["out"][g["deg"] == 0] == 0) and np.all(c["lse"][g["deg"] == 0] == 0)
        one = np.flatnonzero(g["deg"] == 1)[0]
        assert np.array_equal(c["out"][one], c["Wh"][g["col"][g["rp"][one]]])
        assert c["pos"].any() and not c["pos"].all()
    r = gx.exact_rows_case(K, Fh, wbf)
    assert np.abs(r["D"]).max() > 1 and np.abs(r["dsd"]).max() > 1
    g = gx.graph(gx.lanes_of(K, Fh))
    for rpt, colt, nd in ((g["rpt"], g["colt"], g["n"]), (g["rp"], g["col"], gx.N_SRC)):
        c = gx.exact_cols_case(K, Fh, wbf, rpt, colt, nd)
        assert np.array_equal(gx.f32(c["dWh"]), c["dWh"]) and np.array_equal(gx.f32(c["dss"]), c["dss"])
        # leaky2(x) - y = 0 in fp32: fmaxf(x, 0.2f x) = x for x > 0
        x = c["rstat"][:, :, 0].astype(np.float32)
        assert np.all(np.maximum(x, np.float32(0.2) * x) == c["rstat"][:, :, 1].astype(np.float32))


@pytest.mark.parametrize("case", [c for c in gx.CASES if c[2] == 1], ids=gx._id)
def test_bounded_builders_hold_their_preconditions(case):
    K, Fh, wbf = case
    for pattern in gx._patterns_of(K, Fh):
        c = gx.bounded_case(K, Fh, wbf, pattern)
        b_out, b_lse, b_q = gx.forward_bounds(c["g"], c["ref"], K, wbf)
        assert np.all(b_out >= 0) and np.all(b_lse > 0) and np.all(b_q >= 0)
        # the bounds are far below the values they guard: a wrong element cannot hide
        big = np.abs(c["ref"]["out"]) > 0.1
        assert np.all(b_out[big] < 2e-2 * np.abs(c["ref"]["out"][big]) + 2e-3 * c["ref"]["aout"][big])
    assert {p for s in gx.SHAPES for p in gx._patterns_of(*s[:2])} == set(gx.PATTERNS)


def _dense_autograd(g, Wh, s_src, s_dst, dout, K):
    """An independent dense formulation in torch fp64 with autograd."""
    n, ns = g["n"], gx.N_SRC
    Cnt = torch.zeros(n, ns, dtype=F64)
    Cnt.index_put_((torch.from_numpy(g["rows"]).long(), torch.from_numpy(g["col"]).long()),
                   torch.ones(g["nnz"], dtype=F64), accumulate=True)
    W, a, b = (torch.from_numpy(t).clone().requires_grad_() for t in (Wh, s_src, s_dst))
    e = torch.nn.functional.leaky_relu(b[:, None, :] + a[None, :, :], 0.2)            # [n, ns, K]
    logw = torch.where(Cnt[:, :, None] > 0, e + torch.log(Cnt.clamp(min=1))[:, :, None], torch.full_like(e, -1e300))
    lse = torch.logsumexp(logw, 1)
    alpha = torch.exp(logw - lse[:, None, :]) * (Cnt[:, :, None] > 0)
    out = torch.einsum("ijk,jkf->ikf", alpha, W.view(ns, K, -1)).reshape(n, -1)
    gW, ga, gb = torch.autograd.grad(out, (W, a, b), torch.from_numpy(dout))
    return out.detach().numpy(), lse.detach().numpy(), gW.numpy(), ga.numpy(), gb.numpy()


@pytest.mark.parametrize("K,Fh,pattern", [(3, 8, "normal3"), (2, 32, "straddle"), (3, 32, "asc"), (1, 24, "minus120"),
                                          (2, 32, "plus120")])
def test_references_match_dense_fp64_autograd(K, Fh, pattern):
    c = gx.bounded_case(K, Fh, 0, pattern)
    g, ref = c["g"], c["ref"]
    out, lse, gW, ga, gb = _dense_autograd(g, c["Wh"], c["s_src"], c["s_dst"], c["dout"], K)
    has = g["deg"] > 0
    np.testing.assert_allclose(ref["out"], out, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(ref["lse"][has], lse[has], rtol=1e-12, atol=1e-12)
    assert np.all(ref["out"][~has] == 0) and np.all(ref["lse"][~has] == 0)
    # the LeakyReLU split: -0.8 <dout, q> is the per-edge sum is autograd's d s_dst
    rr = gx.rows_ref(c["dout"], ref["out"], ref["q"], ref["lse"], c["s_dst"], K)
    np.testing.assert_allclose(-0.8 * rr["dq"], gb, rtol=1e-9, atol=1e-11)
    per_edge, mag = gx.edge_ds_dst(g, c, K)
    assert np.all(np.abs(per_edge - gb) <= 2.0 ** -40 * mag + 1e-300)
    # the column half from exact statistics (x, y in log2 units, D)
    rstat = np.zeros((g["n"], K, 4))
    rstat[:, :, 0], rstat[:, :, 1], rstat[:, :, 2] = c["s_dst"] * gx.LOG2E, ref["lse"] * gx.LOG2E, rr["D"]
    G = gx.expected_variant(K, Fh) % 100
    cr = gx.cols_ref(g["rpt"], g["colt"], c["Wh"], c["s_src"], rstat, c["dout"], K, G)
    np.testing.assert_allclose(cr["dWh"], gW, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(cr["dss"], ga, rtol=1e-9, atol=1e-10)
    assert np.all(cr["b_dWh"] >= 0) and np.all(cr["b_dss"] >= 0)
    # sums of |terms| dominate the values
    assert np.all(ref["aout"] >= np.abs(ref["out"]) - 1e-12) and np.all(ref["aq"] >= np.abs(ref["q"]) - 1e-12)


@pytest.mark.parametrize("C", gx.CE_C)
def test_row_ce_reference_matches_torch_fp64(C):
    n = 40
    c = gx.row_ce_case(C, n, gx.ru8(C))
    inv = 0.25
    stats, d, nll, zmax = gx.row_ce_ref(c, inv)
    z = torch.from_numpy(c["z"]).clone().requires_grad_()
    y = torch.from_numpy(c["y"]).long()
    tr = torch.from_numpy(c["mask"] == 1)
    loss = torch.nn.functional.cross_entropy(z, y, reduction="none")
    (loss[tr].sum() * inv).backward()
    np.testing.assert_allclose(nll, loss.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(d, z.grad.numpy(), rtol=1e-10, atol=1e-14)
    assert stats[0] == pytest.approx(float(loss.detach()[tr].sum()), rel=1e-12)
    pred = z.detach().argmax(1)
    for m in (1, 2, 3):
        assert stats[m] == int(((pred == y) & torch.from_numpy(c["mask"] == m)).sum())
    assert set(np.unique(c["mask"])) <= {0, 1, 2, 3, 4} and c["y"][0] in (0, C - 1) and c["y"][-1] == C - 1
    assert np.array_equal(c["z"], gx.f32(c["Z"] + c["bias"]))
