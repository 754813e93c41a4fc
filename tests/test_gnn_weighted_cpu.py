"""Edge-weighted graph convolution on the CPU branches: ``ops.wspmm`` / ``ops.sddmm``,
``data.build_weighted_csr``, ``layers.WeightedGraph`` / ``weighted_aggregate`` and a GCN
trained on a weighted graph.

The op references are dense fp64 products built here.  Features are integers in [-3, 3],
edge values from {+-0.25, +-0.5, +-1, +-2, 0} and scales from {0.5, 1, 2}: every product
and partial sum is exact in fp32, so those comparisons are ``torch.equal``.
"""
import numpy as np
import pytest
import torch

from cgnn_amd.gnn import data, layers, ops
from cgnn_amd.gnn.layers import GCN, NormGraph, WeightedGraph, weighted_aggregate

F32, F64 = torch.float32, torch.float64
VALS = [-2.0, -1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0, 2.0]


def _csr(deg, n_src, rng):
    deg = np.asarray(deg, dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = rng.integers(0, n_src, int(rp[-1])).astype(np.int32)
    return torch.from_numpy(rp), torch.from_numpy(col)


def _dense(rp, col, val, n_src):
    """Dense fp64 matrix of the CSR (duplicate entries add)."""
    n = rp.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n), (rp[1:] - rp[:-1]).long())
    A = torch.zeros(n, n_src, dtype=F64)
    A.index_put_((rows, col.long()), val.double(), accumulate=True)
    return A, rows


def _case(seed=0, n_src=37):
    rng = np.random.default_rng(seed)
    deg = [0, 1, 2, 3, 5, 8, 9, 0, 17, 4, 1]
    rp, col = _csr(deg, n_src, rng)
    val = torch.from_numpy(rng.choice(VALS, col.numel())).float()
    rs = torch.from_numpy(rng.choice([0.5, 1.0, 2.0], len(deg))).float()
    cs = torch.from_numpy(rng.choice([0.5, 1.0, 2.0], n_src)).float()
    return rng, rp, col, val, rs, cs


@pytest.mark.parametrize("dt", [F32, torch.bfloat16, torch.float16, F64])
def test_wspmm_cpu_exact(dt):
    rng, rp, col, val, rs, cs = _case()
    n, n_src, F, ld = rp.numel() - 1, cs.numel(), 13, 16
    X = torch.zeros(n_src, ld, dtype=F64)
    X[:, :F] = torch.from_numpy(rng.integers(-3, 4, (n_src, F)).astype(np.float64))
    bias = torch.from_numpy(rng.integers(-2, 3, F).astype(np.float32))
    A, _ = _dense(rp, col, val, n_src)
    v = val.double() if dt == F64 else val
    for use_rs, use_cs, use_b, relu in [(0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 1, 0), (0, 1, 0, 1)]:
        ref = (A * cs.double()[None, :] if use_cs else A) @ X[:, :F]
        if use_rs:
            ref = ref * rs.double()[:, None]
        if use_b:
            ref = ref + bias.double()
        if relu:
            ref = ref.clamp_min(0)
        assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) < 4096
        full = torch.full((n + 2, ld), 7.0, dtype=dt)
        ops.wspmm(rp, col, v, X.to(dt), F, rscale=rs if use_rs else None, cscale=cs if use_cs else None,
                  bias=bias if use_b else None, relu=bool(relu), out=full[:n])
        exp = torch.zeros(n, ld, dtype=F64)
        exp[:, :F] = ref
        assert torch.equal(full[:n], exp.to(dt))
        assert torch.all(full[n:] == 7.0)
    # through an edge permutation: shuffled values, the same sums
    perm = torch.from_numpy(rng.permutation(col.numel())).to(torch.int32)
    shuffled = torch.empty_like(v)
    shuffled[perm.long()] = v
    a = ops.wspmm(rp, col, v, X.to(dt), F, rscale=rs, cscale=cs)
    b = ops.wspmm(rp, col, shuffled, X.to(dt), F, rscale=rs, cscale=cs, eperm=perm)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dt", [F32, torch.bfloat16, torch.float16, F64])
def test_sddmm_cpu_exact(dt):
    rng, rp, col, val, rs, cs = _case(1)
    n, n_src, F, ld = rp.numel() - 1, cs.numel(), 13, 16
    A = torch.full((n, ld), 5.0, dtype=F64)          # padding columns must not be read
    B = torch.full((n_src, ld), 5.0, dtype=F64)
    A[:, :F] = torch.from_numpy(rng.integers(-3, 4, (n, F)).astype(np.float64))
    B[:, :F] = torch.from_numpy(rng.integers(-3, 4, (n_src, F)).astype(np.float64))
    rows = torch.repeat_interleave(torch.arange(n), (rp[1:] - rp[:-1]).long())
    P = A[:, :F] @ B[:, :F].t()
    for use_s in (False, True):
        ref = P[rows, col.long()]
        if use_s:
            ref = ref * rs.double()[rows] * cs.double()[col.long()]
        out = torch.full((col.numel() + 3,), 7.0, dtype=F64 if dt == F64 else F32)
        ops.sddmm(rp, col, A.to(dt), B.to(dt), F, rscale=rs if use_s else None, cscale=cs if use_s else None,
                  out=out)
        assert torch.equal(out[:col.numel()].double(), ref)
        assert torch.all(out[col.numel():] == 7.0)
    with pytest.raises(TypeError):
        ops.sddmm(rp, col, A.float(), B.to(torch.bfloat16), F)


def _directed_graph(n, m, seed):
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    return rng, src, dst


def test_weighted_aggregate_gradcheck_fp64():
    n = 12
    rng, src, dst = _directed_graph(n, 40, 3)
    rp, col, val = data.build_weighted_csr(n, src, dst, rng.uniform(0.5, 1.5, 40))
    rs = torch.from_numpy(rng.uniform(0.5, 2.0, n))
    cs = torch.from_numpy(rng.uniform(0.5, 2.0, n))
    g = WeightedGraph(rp, col, val, rscale=rs, cscale=cs)
    x = torch.from_numpy(rng.standard_normal((n, 5))).requires_grad_()
    v = val.double().clone().requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b: weighted_aggregate(a, g, b), (x, v), eps=1e-6, atol=1e-7)
    # and the values: the dense product
    A, _ = _dense(rp, col, val, n)
    ref = (rs[:, None] * A * cs[None, :]) @ x.detach()
    got = weighted_aggregate(x.detach(), g, val.double())
    assert torch.allclose(got, ref, rtol=0, atol=1e-12)


def test_build_weighted_csr_rules():
    #        dst <- src
    src = [2, 0, 2, 1, 1, 3]
    dst = [0, 0, 0, 1, 2, 2]
    w = [1.0, 2.0, 0.5, 4.0, 3.0, 1.5]
    rp, col, val = data.build_weighted_csr(4, src, dst, w)
    assert rp.dtype == torch.int32 and col.dtype == torch.int32 and val.dtype == F32
    assert rp.tolist() == [0, 2, 3, 5, 5]                       # row 3: no in-edges
    assert col.tolist() == [0, 2, 1, 1, 3]                      # sorted by source inside a row
    assert val.tolist() == [2.0, 1.5, 4.0, 3.0, 1.5]            # 2 -> 0 twice: 1 + 0.5
    # directed: 1 -> 2 is there, 2 -> 1 is not
    A, _ = _dense(rp, col, val, 4)
    assert A[2, 1] == 3.0 and A[1, 2] == 0.0
    # self loops: nodes 0 and 1 have their own (kept at 2 and 4), the others get 0.25
    rp, col, val = data.build_weighted_csr(4, src, dst, w, self_loops=0.25)
    A, _ = _dense(rp, col, val, 4)
    assert torch.equal(torch.diagonal(A), torch.tensor([2.0, 4.0, 0.25, 0.25], dtype=F64))
    assert rp.tolist() == [0, 2, 3, 6, 7] and col.tolist() == [0, 2, 1, 1, 2, 3, 3]
    for i in range(4):
        c = col[rp[i]:rp[i + 1]].tolist()
        assert c == sorted(c)


def test_from_edges_sym_matches_build_csr_and_fp64_degrees():
    n = 50
    rng, src, dst = _directed_graph(n, 160, 4)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    s2, d2 = np.concatenate([src, dst]), np.concatenate([dst, src])     # a symmetric edge list
    # unit weights per DISTINCT edge: duplicates would sum
    key = np.unique(d2 * n + s2)
    d2, s2 = key // n, key % n
    g = WeightedGraph.from_edges(n, s2, d2, normalize="sym")
    rp, col = data.build_csr(n, src, dst)
    assert torch.equal(g.rowptr, rp) and torch.equal(g.col.to(col.dtype), col)
    deg = (rp[1:] - rp[:-1]).double()
    dinv = deg.pow(-0.5)
    rows = torch.repeat_interleave(torch.arange(n), (rp[1:] - rp[:-1]).long())
    assert g.val.dtype == F32
    assert torch.equal(g.val, (dinv[rows] * dinv[col.long()]).float())
    assert g.rscale is None and g.cscale is None


def test_from_edges_rw_rows_sum_to_one_and_zero_degree_rows():
    n = 30
    rng, src, dst = _directed_graph(n, 120, 5)
    w = rng.uniform(0.1, 3.0, 120)
    g = WeightedGraph.from_edges(n, src, dst, w, normalize="rw")
    rp = g.rowptr.long()
    for i in range(n):
        v = g.val[rp[i]:rp[i + 1]].double()
        k = v.numel()
        assert k >= 1                                       # the self loop
        # each entry is the exact quotient (|q| <= 1) rounded once to fp32: an error of at
        # most 2^-25 per entry, plus the fp64 quotients' own 2^-53 each
        assert abs(float(v.sum()) - 1.0) <= k * (2.0 ** -25 + 2.0 ** -52)
    # zero-degree rows: no self loops, node 7 has no in-edges; node 3's weights cancel
    src, dst, w = [0, 1, 0, 1], [2, 2, 3, 3], [1.0, 3.0, 1.0, -1.0]
    for mode in ("sym", "rw"):
        g = WeightedGraph.from_edges(8, src, dst, w, self_loops=None, normalize=mode)
        assert g.rowptr.tolist() == [0, 0, 0, 2, 4, 4, 4, 4, 4]
        assert torch.all(torch.isfinite(g.val))
        assert torch.all(g.val[2:] == 0)                    # row 3: d = 0 -> scale 0
    g = WeightedGraph.from_edges(8, src, dst, w, self_loops=None, normalize="rw")
    assert g.val[:2].tolist() == [0.25, 0.75]
    raw = WeightedGraph.from_edges(8, src, dst, w, self_loops=None, normalize=None)
    assert raw.val.tolist() == w


def test_from_norm_keeps_the_factored_form():
    gd = data.synthetic("cora", scale=0.05)
    ng = NormGraph.from_data(gd)
    wg = WeightedGraph.from_norm(ng)
    assert torch.all(wg.val == 1) and wg.rscale is ng.dinv and wg.cscale is ng.dinv
    x = torch.randn(gd.n, 16, generator=torch.Generator().manual_seed(0))
    a = layers.norm_aggregate(x, ng)
    b = weighted_aggregate(x, wg)
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


def test_transposed_is_cached_and_eperm_maps_to_forward_edges():
    rng, rp, col, val, rs, cs = _case(2)
    g = WeightedGraph(rp, col, val, n_src=cs.numel())
    t = g.transposed()
    assert g.transposed() is t
    rp_t, col_t, eperm = t
    assert rp_t.numel() == cs.numel() + 1 and eperm.dtype == torch.int32
    assert sorted(eperm.tolist()) == list(range(col.numel()))
    rows = torch.repeat_interleave(torch.arange(rp.numel() - 1), (rp[1:] - rp[:-1]).long())
    rows_t = torch.repeat_interleave(torch.arange(cs.numel()), (rp_t[1:] - rp_t[:-1]).long())
    # transposed edge k = (rows_t[k] <- col_t[k]) is forward edge eperm[k] = (col_t[k] <- rows_t[k])
    assert torch.equal(col[eperm.long()].long(), rows_t)
    assert torch.equal(rows[eperm.long()], col_t.long())
    # and the transposed aggregate is A^T x
    A, _ = _dense(rp, col, val, cs.numel())
    x = torch.from_numpy(rng.integers(-3, 4, (rp.numel() - 1, 8)).astype(np.float32))
    got = ops.wspmm(rp_t, col_t, val, x, 8, eperm=eperm)
    assert torch.equal(got.double(), A.t() @ x.double())


def test_gcn_trains_on_a_weighted_graph():
    n, C, F = 60, 3, 8
    rng = np.random.default_rng(7)
    y = np.arange(n) % C
    src, dst = [], []
    while len(src) < 400:                                    # planted communities, directed edges
        a, b = rng.integers(0, n, 2)
        if a != b and (y[a] == y[b] or rng.random() < 0.1):
            src.append(a)
            dst.append(b)
    w = rng.uniform(0.5, 2.0, len(src))
    g = WeightedGraph.from_edges(n, src, dst, w, normalize="rw")
    cent = rng.standard_normal((C, F))
    x = torch.from_numpy(cent[y] + 2.0 * rng.standard_normal((n, F))).float()
    yt = torch.from_numpy(y).long()
    model = GCN([F, 16, C], dropout=0.0, seed=1)
    opt = torch.optim.Adam(model.parameters(), lr=0.02)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(x, g), yt)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0], losses
    ew = g.val.clone().requires_grad_()
    loss = torch.nn.functional.cross_entropy(model(x, g, edge_weight=ew), yt)
    loss.backward()
    assert ew.grad is not None and ew.grad.dtype == F32 and ew.grad.shape == g.val.shape
    assert bool(torch.isfinite(ew.grad).all()) and float(ew.grad.abs().max()) > 0
    # the analytic edge gradient against autograd through the dense fp64 model
    rows = ops._row_ids(g.rowptr)
    ev = g.val.double().clone().requires_grad_()
    h = x.double()
    for k, conv in enumerate(model.convs):
        A = torch.zeros(n, n, dtype=F64).index_put((rows, g.col.long()), ev, accumulate=True)
        h = A @ (h @ conv.weight.double()) + conv.bias.double()
        if k == 0:
            h = h.relu()
    torch.nn.functional.cross_entropy(h, yt).backward()
    assert torch.allclose(ew.grad.double(), ev.grad, rtol=1e-4, atol=1e-6)
