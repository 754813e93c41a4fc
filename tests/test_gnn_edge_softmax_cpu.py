"""Edge softmax, ``edge_dot`` and ``AttentionConv`` without a GPU: the autograd functions under
``gradcheck`` in fp64, the edge-case rules of the CPU branch of ``ops.edge_softmax``, and a
one-head ``AttentionConv`` against a dense masked-softmax attention written here.  Every
reference is computed in this file from the CSR, never through ``ops``."""
import numpy as np
import pytest
import torch

from cgnn_amd.gnn import ops
from cgnn_amd.gnn.layers import AttentionConv, NormGraph, WeightedGraph, edge_dot, edge_softmax
from cgnn_amd.gnn.sage import Block
from cgnn_amd.utils import checks

F32, F64 = torch.float32, torch.float64
NAN, INF = float("nan"), float("inf")

# 6 destinations over 9 sources: an empty row, a single edge, a row that lists source 2 twice
RP = np.array([0, 3, 3, 4, 8, 10, 13], dtype=np.int32)
COL = np.array([1, 8, 0, 4, 2, 5, 2, 7, 3, 0, 6, 1, 5], dtype=np.int32)
N, N_SRC, NNZ = 6, 9, 13
ROWS = np.repeat(np.arange(N), np.diff(RP))


def _graphs():
    rp, col = torch.from_numpy(RP), torch.from_numpy(COL)
    sq = torch.from_numpy((COL % N).astype(np.int32))            # a square graph for the NormGraph
    return [("weighted", WeightedGraph(rp, col, torch.full((NNZ,), 7.0), n_src=N_SRC, rscale=torch.full((N,), 3.0)),
             COL, N_SRC),
            ("norm", NormGraph(rp, sq, torch.full((N,), 5.0)), sq.numpy(), N),
            ("block", Block(RP, COL, N_SRC, "cpu"), COL, N_SRC)]


def _softmax_ref(rp, s, scale):
    """[K, nnz] fp64 numpy: the definition, row by row; a row of -inf gives 0."""
    p = np.zeros_like(s)
    for k in range(s.shape[0]):
        for i in range(len(rp) - 1):
            e0, e1 = int(rp[i]), int(rp[i + 1])
            if e1 == e0:
                continue
            x = s[k, e0:e1]
            m = x.max()
            if m == -INF:
                continue
            with np.errstate(invalid="ignore"):
                ex = np.exp(scale * (x - m))
                p[k, e0:e1] = ex / ex.sum()
    return p


# ------------------------------------------------------------------ values of the CPU branch
@pytest.mark.parametrize("dt", [F32, F64])
def test_cpu_branch_matches_the_definition_and_leaves_the_gap_alone(dt):
    rng = np.random.default_rng(3)
    K, ld = 3, NNZ + 5
    s = np.full((K, ld), 77.0)
    s[:, :NNZ] = rng.standard_normal((K, NNZ)) * 3
    st = torch.from_numpy(s).to(dt)
    out = torch.full((K, ld), -9.0, dtype=dt)
    got = ops.edge_softmax(torch.from_numpy(RP), st, scale=0.5, out=out, nnz=NNZ)
    assert got is out and torch.all(out[:, NNZ:] == -9.0)
    ref = _softmax_ref(RP, st.double().numpy()[:, :NNZ], 0.5)
    np.testing.assert_allclose(out[:, :NNZ].double().numpy(), ref, rtol=1e-6 if dt == F32 else 1e-14)
    # the backward against the definition
    dp = rng.standard_normal((K, ld))
    dpt = torch.from_numpy(dp).to(dt)
    ds = ops.edge_softmax_bwd(torch.from_numpy(RP), out, dpt, scale=0.5, nnz=NNZ)
    p64, d64 = out.double().numpy()[:, :NNZ], dpt.double().numpy()[:, :NNZ]
    dot = np.zeros((K, N))
    for k in range(K):
        np.add.at(dot[k], ROWS, p64[k] * d64[k])
    np.testing.assert_allclose(ds[:, :NNZ].double().numpy(), 0.5 * p64 * (d64 - dot[:, ROWS]),
                               rtol=1e-5 if dt == F32 else 1e-13, atol=1e-7 if dt == F32 else 1e-15)
    # one head as a vector
    v = ops.edge_softmax(torch.from_numpy(RP), st[1, :NNZ].clone(), scale=0.5)
    assert torch.equal(v, out[1, :NNZ])
    # in place
    s2 = st.clone()
    assert ops.edge_softmax(torch.from_numpy(RP), s2, scale=0.5, out=s2, nnz=NNZ) is s2
    assert torch.equal(s2[:, :NNZ], out[:, :NNZ]) and torch.all(s2[:, NNZ:] == 77.0)


@pytest.mark.parametrize("dt", [F32, F64])
def test_edge_case_rules_on_the_cpu_branch(dt):
    rows = [[4.0], [1e30, 0.0, -1e30], [100.0, 100.0], [-INF, 1.0, -INF, 1.0], [-INF, -INF, -INF], [],
            [0.5, NAN, 2.0], [3.0, INF, -1.0], [1.0, 2.0, 3.0]]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    flat = torch.tensor([v for r in rows for v in r], dtype=dt)
    p = ops.edge_softmax(torch.from_numpy(rp), flat)
    seg = [p[rp[i]:rp[i + 1]] for i in range(len(rows))]
    assert seg[0].tolist() == [1.0]
    assert seg[1].tolist() == [1.0, 0.0, 0.0]
    assert seg[2].tolist() == [0.5, 0.5]
    assert seg[3].tolist() == [0.0, 0.5, 0.0, 0.5]
    assert seg[4].tolist() == [0.0, 0.0, 0.0]
    assert torch.isnan(seg[6]).all() and torch.isnan(seg[7]).all()
    # the NaN / +inf rows touch nothing else
    clean = flat.clone()
    clean[rp[6] + 1] = 0.0
    clean[rp[7] + 1] = 0.0
    q = ops.edge_softmax(torch.from_numpy(rp), clean)
    keep = torch.ones(flat.numel(), dtype=torch.bool)
    keep[rp[6]:rp[8]] = False
    assert torch.equal(p[keep], q[keep]) and not torch.isnan(q).any()
    assert abs(float(seg[8].sum()) - 1.0) < 1e-6


def test_validation_on_the_cpu_branch(monkeypatch):
    rp = torch.from_numpy(RP)
    with pytest.raises(ValueError):
        ops.edge_softmax(rp, torch.zeros(NNZ), out=torch.zeros(NNZ + 1))       # shapes differ
    with pytest.raises(ValueError):
        ops.edge_softmax(rp, torch.zeros(NNZ), lanes=3)
    with pytest.raises(ValueError):
        ops.edge_softmax(rp, torch.zeros(2, 2, NNZ))
    monkeypatch.setattr(checks, "ENABLED", True)
    with pytest.raises(ValueError, match="CGNN_CHECK"):
        ops.edge_softmax(rp, torch.zeros(2, NNZ - 1))                            # rowptr[-1] > ld
    with pytest.raises(ValueError, match="CGNN_CHECK"):
        ops.edge_softmax(rp, torch.zeros(NNZ), scale=0.0)
    with pytest.raises(ValueError, match="CGNN_CHECK"):
        ops.edge_softmax_bwd(rp, torch.zeros(NNZ), torch.zeros(NNZ), scale=INF)
    ops.edge_softmax(rp, torch.zeros(2, NNZ + 3), nnz=NNZ)


# ------------------------------------------------------------------ gradcheck
@pytest.mark.parametrize("K", [1, 3])
def test_gradcheck_edge_softmax(K):
    g = Block(RP, COL, N_SRC, "cpu")
    rng = np.random.default_rng(K)
    s = torch.from_numpy(rng.standard_normal((K, NNZ))).requires_grad_()
    assert torch.autograd.gradcheck(lambda x: edge_softmax(x, g, scale=0.5), (s,))
    if K == 1:
        v = torch.from_numpy(rng.standard_normal(NNZ)).requires_grad_()
        assert torch.autograd.gradcheck(lambda x: edge_softmax(x, g, scale=0.5), (v,))
    p = edge_softmax(s.detach(), g, scale=0.5)
    assert torch.allclose(p, torch.from_numpy(_softmax_ref(RP, s.detach().numpy(), 0.5)), rtol=1e-13, atol=0)


def test_gradcheck_edge_dot_both_operands_on_a_rectangular_graph():
    g = Block(RP, COL, N_SRC, "cpu")
    assert np.sum(COL[RP[3]:RP[4]] == 2) == 2                   # a source repeated in one row
    rng = np.random.default_rng(5)
    a = torch.from_numpy(rng.standard_normal((N, 5))).requires_grad_()
    b = torch.from_numpy(rng.standard_normal((N_SRC, 5))).requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b: edge_dot(a, b, g), (a, b))
    d = edge_dot(a, b, g).detach().numpy()
    ref = (a.detach().numpy()[ROWS] * b.detach().numpy()[COL]).sum(1)
    np.testing.assert_allclose(d, ref, rtol=1e-13)

    def heads(a, b):                                          # two heads into one [K, nnz] buffer
        buf = torch.full((2, NNZ), NAN, dtype=F64)
        o = edge_dot(a, b, g, out=buf[0])
        assert o.data_ptr() == buf.data_ptr()
        edge_dot(a * 2, b + 1, g, out=buf[1])
        return edge_softmax(buf, g, scale=0.5)

    assert torch.autograd.gradcheck(heads, (a, b))
    assert edge_dot(a.float(), b.float(), g).dtype == F32


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("root_weight", [True, False])
def test_gradcheck_attention_conv(concat, root_weight):
    rng = np.random.default_rng(11)
    for name, g, col, n_src in _graphs():
        m = AttentionConv(4, 2, 3, concat=concat, root_weight=root_weight,
                          generator=torch.Generator().manual_seed(1)).double()
        with torch.no_grad():
            for p in m.parameters():                          # non-zero biases
                p.add_(torch.from_numpy(rng.standard_normal(tuple(p.shape))) * 0.3)
        names = [k for k, _ in m.named_parameters()]
        assert len(names) == 6 + int(root_weight) + 1
        h = torch.from_numpy(rng.standard_normal((n_src, 4))).requires_grad_()

        def f(h, *params):
            return torch.func.functional_call(m, dict(zip(names, params)), (h, g))

        out = f(h, *m.parameters())
        assert out.shape == (N, 6 if concat else 3), name
        assert torch.autograd.gradcheck(f, (h, *m.parameters())), name


# ------------------------------------------------------------------ dense attention
def test_one_head_attention_conv_equals_dense_masked_attention():
    """heads = 1: out = softmax(mask(Q K^T / sqrt(d))) V + h_dst W_root + bias, with the mask's
    multiplicity (source 2 is listed twice in row 3: its term counts twice in numerator and
    denominator); the empty row keeps only the root term."""
    rng = np.random.default_rng(2)
    d = 5
    m = AttentionConv(4, 1, d, generator=torch.Generator().manual_seed(4)).double()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.from_numpy(rng.standard_normal(tuple(p.shape))) * 0.3)
    h = torch.from_numpy(rng.standard_normal((N_SRC, 4)))
    g = Block(RP, COL, N_SRC, "cpu")
    out, alpha = m(h, g, return_attention=True)
    assert alpha.shape == (1, NNZ) and alpha.dtype == F64
    hn = h.numpy()
    P = {k: v.detach().numpy() for k, v in m.named_parameters()}
    Q = hn[:N] @ P["w_q"][0] + P["b_q"][0]
    Kh = hn @ P["w_k"][0] + P["b_k"][0]
    V = hn @ P["w_v"][0] + P["b_v"][0]
    count = np.zeros((N, N_SRC))
    np.add.at(count, (ROWS, COL), 1.0)
    logits = Q @ Kh.T / np.sqrt(d)
    mx = np.where(count > 0, logits, -INF).max(1, keepdims=True)
    w = count * np.exp(np.where(count > 0, logits - np.where(mx > -INF, mx, 0.0), -INF))
    den = w.sum(1, keepdims=True)
    att = np.divide(w, den, out=np.zeros_like(w), where=den > 0)
    ref = att @ V + hn[:N] @ P["w_root"] + P["bias"]
    np.testing.assert_allclose(out.detach().numpy(), ref, rtol=1e-12, atol=1e-13)
    assert np.count_nonzero(att[1]) == 0 and count[3, 2] == 2


def test_attention_conv_storage_dtype_and_initialisation():
    m = AttentionConv(16, 4, 8, generator=torch.Generator().manual_seed(0))
    bound = (6.0 / (16 + 32)) ** 0.5
    for w in (m.w_q, m.w_k, m.w_v, m.w_root):
        assert 0.8 * bound < float(w.detach().abs().max()) <= bound
    assert m.w_q.shape == (4, 16, 8) and m.w_root.shape == (16, 32)
    assert all(float(b.detach().abs().max()) == 0 for b in (m.b_q, m.b_k, m.b_v, m.bias))
    g = Block(RP, COL, N_SRC, "cpu")
    out, alpha = m(torch.randn(N_SRC, 16, generator=torch.Generator().manual_seed(1)), g, return_attention=True)
    assert out.dtype == F32 and out.shape == (N, 32) and alpha.dtype == F32
    sums = torch.zeros(4, N).index_add_(1, torch.from_numpy(ROWS), alpha)
    assert torch.allclose(sums[:, [0, 2, 3, 4, 5]], torch.ones(4, 5), atol=1e-6) and torch.all(sums[:, 1] == 0)
    with pytest.raises(ValueError):
        m(torch.randn(N, 16), g)                                # fewer rows than sources
