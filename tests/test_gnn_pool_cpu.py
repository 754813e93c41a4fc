"""Max / min neighbour pooling without a GPU: the CPU branch of ``ops.pool`` / ``ops.pool_bwd``
against a loop reference written here (never through ``ops``), the autograd function under
``gradcheck``, the cached transposed-with-permutation of ``sage.Block``, ``SAGE(aggr=)`` and
the trainer rules, and the ``CGNN_CHECK`` validation."""
import numpy as np
import pytest
import torch

from cgnn_amd.gnn import ops
from cgnn_amd.gnn.layers import NormGraph, WeightedGraph, pool_aggregate
from cgnn_amd.gnn.sage import SAGE, Block, SAGETrainer, transpose_csr
from cgnn_amd.utils import checks

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64


# ------------------------------------------------------------------ the reference
def _pool_ref(rp, col, X, F, is_min):
    """The definition, as loops over fp64 numpy: CSR scan order, a candidate replaces the best
    only when strictly better or when it is NaN and the best is not; empty row: 0 / -1."""
    n = len(rp) - 1
    Y = np.zeros((n, F))
    A = np.full((n, F), -1, dtype=np.int64)
    for i in range(n):
        for f in range(F):
            for e in range(rp[i], rp[i + 1]):
                c = X[col[e], f]
                if e == rp[i]:
                    take = True
                else:
                    b = Y[i, f]
                    take = (c < b if is_min else c > b) or (np.isnan(c) and not np.isnan(b))
                if take:
                    Y[i, f], A[i, f] = c, e
    return Y, A


def _pool_bwd_ref(rp, col, A, dY, n_src, F):
    """dX[j, f] = sum over the edges e with col[e] == j of (A[i, f] == e) dY[i, f]."""
    dX = np.zeros((n_src, F))
    for i in range(len(rp) - 1):
        for e in range(rp[i], rp[i + 1]):
            dX[col[e]] += np.where(A[i, :F] == e, dY[i, :F], 0.0)
    return dX


def _same(got, exp):
    """Bitwise equality that lets a NaN equal a NaN."""
    got, exp = got.double(), exp.double()
    return bool(torch.equal(torch.isnan(got), torch.isnan(exp))
                and torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(exp, nan=0.0)))


def _toy(seed=0, n=23, n_src=31):
    """Rows of degree 0 .. 12 (two of them empty), one row repeating a source id, sources 0
    and n_src - 1 in use."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 13, n)
    deg[[0, 7]] = 0
    deg[3] = 5
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = rng.integers(0, n_src, int(rp[-1])).astype(np.int32)
    col[rp[3]:rp[4]] = col[rp[3]]
    col[rp[1]] = 0
    col[rp[2]] = n_src - 1
    return rp, col, rng


# ------------------------------------------------------------------ CPU branch
@pytest.mark.parametrize("dt", [F32, BF16, F16, F64])
@pytest.mark.parametrize("reduce", ["max", "min"])
def test_cpu_branch_equals_the_loop_reference(dt, reduce):
    rp, col, rng = _toy()
    n, n_src, F, ld = len(rp) - 1, 31, 11, 16
    rp_t, col_t = torch.from_numpy(rp), torch.from_numpy(col)
    for kind in ("normal", "ties", "nan"):
        X = torch.full((n_src, ld), 1e4, dtype=F64)               # the padding must not be read
        if kind == "ties":
            X[:, :F] = torch.from_numpy(rng.integers(-2, 3, (n_src, F)).astype(np.float64))
        else:
            X[:, :F] = torch.from_numpy(rng.standard_normal((n_src, F)))
        if kind == "nan":
            X[rng.integers(0, n_src, 9), rng.integers(0, F, 9)] = float("nan")
            X[5, 0] = float("inf")
            X[6, 1] = -float("inf")
        X = X.to(dt)
        Yr, Ar = _pool_ref(rp, col, X.double().numpy(), F, reduce == "min")
        out = torch.full((n + 2, ld), 7.0, dtype=dt)
        arg = torch.full((n + 2, ld), 7, dtype=torch.int32)
        Y, A = ops.pool(rp_t, col_t, X, F, reduce=reduce, out=out[:n], arg=arg[:n])
        assert Y.dtype == dt and A.dtype == torch.int32
        assert _same(Y[:, :F], torch.from_numpy(Yr)), (kind, dt)
        assert torch.equal(A[:, :F].long(), torch.from_numpy(Ar)), (kind, dt)
        assert torch.all(Y[:, F:] == 0) and torch.all(A[:, F:] == -1)
        assert torch.all(Y[[0, 7]] == 0) and torch.all(A[[0, 7]] == -1)          # empty rows
        assert torch.all(out[n:] == 7) and torch.all(arg[n:] == 7)
        Y2, none = ops.pool(rp_t, col_t, X, F, reduce=reduce, with_arg=False)
        assert none is None and _same(Y2, Y)
        # the gradient, from the reference's arg
        dY = torch.zeros(n, ld, dtype=F64)
        dY[:, :F] = torch.from_numpy(rng.integers(-3, 4, (n, F)).astype(np.float64))
        rpt, colt, eperm = transpose_csr(rp_t, col_t, n_src, with_perm=True)
        dXr = _pool_bwd_ref(rp, col, Ar, dY.numpy(), n_src, F)
        dX = ops.pool_bwd(rpt, colt, eperm, A, dY.to(dt), F)
        assert dX.dtype == dt and dX.shape == (n_src, ld)
        assert torch.equal(dX[:, :F].double(), torch.from_numpy(dXr)) and torch.all(dX[:, F:] == 0)
    with pytest.raises(ValueError):
        ops.pool(rp_t, col_t, X, F, reduce="sum")


def test_duplicate_source_in_a_row_is_counted_once():
    rp = torch.tensor([0, 3], dtype=torch.int32)
    col = torch.tensor([1, 1, 1], dtype=torch.int32)
    x = torch.tensor([[0.0] * 8, [2.0] * 8], requires_grad=True)
    g = WeightedGraph(rp, col, torch.ones(3), n_src=2)
    y = pool_aggregate(x, g)
    gy = torch.arange(1.0, 9.0)[None]
    y.backward(gy)
    assert torch.equal(y.detach(), torch.full((1, 8), 2.0))
    assert torch.equal(x.grad[1], gy[0]) and torch.all(x.grad[0] == 0)


# ------------------------------------------------------------------ autograd
@pytest.mark.parametrize("reduce", ["max", "min"])
def test_gradcheck_fp64(reduce):
    """Features are a random permutation of distinct values: no ties, so the gradient is
    defined (and gradcheck's perturbation, 1e-6, is far below the gaps of 0.01)."""
    rp, col, rng = _toy(3, n=9, n_src=12)
    F = 5
    vals = torch.from_numpy(rng.permutation(12 * F).astype(np.float64).reshape(12, F)) * 0.01
    graphs = [WeightedGraph(torch.from_numpy(rp), torch.from_numpy(col), torch.ones(len(col)), n_src=12),
              Block(rp, col, 12, "cpu")]
    for g in graphs:
        x = vals.clone().requires_grad_()
        assert torch.autograd.gradcheck(lambda t: pool_aggregate(t, g, reduce), (x,), eps=1e-6, atol=1e-7)


def test_normgraph_is_accepted_and_its_permutation_cached():
    from cgnn_amd.gnn import data
    gd = data.synthetic("cora", scale=0.05, device="cpu")
    ng = NormGraph.from_data(gd)
    x = torch.randn(gd.n, 12, generator=torch.Generator().manual_seed(0), dtype=F64).requires_grad_()
    y = pool_aggregate(x, ng, "max")
    Yr, Ar = _pool_ref(ng.rowptr.numpy(), ng.col.numpy(), x.detach().numpy(), 12, False)
    assert torch.equal(y.detach(), torch.from_numpy(Yr))
    gy = torch.randn(gd.n, 12, generator=torch.Generator().manual_seed(1), dtype=F64)
    y.backward(gy)
    t = ng.transposed_perm()
    assert ng.transposed_perm() is t
    # distinct values: one term per (row, feature) at most per edge, so the sums only differ
    # from the reference's by their order
    dXr = _pool_bwd_ref(ng.rowptr.numpy(), ng.col.numpy(), Ar, gy.numpy(), gd.n, 12)
    np.testing.assert_allclose(x.grad.numpy(), dXr, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ Block
def test_block_transposed_perm_is_cached_and_maps_to_forward_edges():
    rp, col, _ = _toy(5)
    b = Block(rp, col, 31, "cpu")
    plain = b.transposed()
    assert len(plain) == 2                                   # transposed() returns what it did
    rp_t, col_t, eperm = b.transposed_perm()
    assert b.transposed_perm()[2] is eperm and b.transposed() is plain
    assert torch.equal(rp_t, plain[0]) and torch.equal(col_t, plain[1])
    assert eperm.dtype == torch.int32 and sorted(eperm.tolist()) == list(range(len(col)))
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    for j in range(31):
        for t in range(int(rp_t[j]), int(rp_t[j + 1])):
            assert col[int(eperm[t])] == j and rows[int(eperm[t])] == int(col_t[t])


# ------------------------------------------------------------------ SAGE / trainer
def _blocks():
    rng = np.random.default_rng(9)
    sizes = [40, 22, 11, 5]                                  # sources of block 0 ... destinations of block 2
    out = []
    for ns, nd in zip(sizes[:-1], sizes[1:]):
        deg = rng.integers(0, 6, nd)
        rp = np.concatenate([[0], np.cumsum(deg)])
        out.append(Block(rp, rng.integers(0, ns, int(rp[-1])), ns, "cpu"))
    return out


def test_sage_mean_path_is_unchanged_and_pooling_differs():
    blocks = _blocks()
    x = torch.randn(40, 16, generator=torch.Generator().manual_seed(2))
    ref = SAGE(16, 8, 4, layers=3, dropout=0.0, seed=5)
    mean = SAGE(16, 8, 4, layers=3, dropout=0.0, seed=5, aggr="mean")
    mx = SAGE(16, 8, 4, layers=3, dropout=0.0, seed=5, aggr="max")
    assert ref.aggr == "mean" and mx.aggr == "max"
    for a, b in zip(ref.parameters(), mx.parameters()):
        assert torch.equal(a, b)
    y_ref, y_mean, y_max = ref(x, blocks), mean(x, blocks), mx(x, blocks)
    assert torch.equal(y_ref, y_mean)
    assert y_max.shape == y_ref.shape and not torch.equal(y_max, y_ref)
    y_max.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in mx.parameters())
    with pytest.raises(ValueError):
        SAGE(16, 8, 4, aggr="sum")


def test_trainer_rules_and_full_graph_training_with_max():
    from cgnn_amd.gnn import data
    g = data.synthetic("cora", scale=0.1, device="cpu", seed=0)
    with pytest.raises(ValueError, match="mean aggregator only"):
        SAGETrainer(g, aggr="max", fused=True)
    # 6 epochs: the count at which the "mean" trainer on the same data also ends below its
    # first loss (asserted here, so the choice is not tuned to the new aggregator)
    epochs = 6
    losses = {}
    for aggr in ("mean", "max"):
        tr = SAGETrainer(g, hidden=32, layers=2, dropout=0.0, lr=0.01, fanouts=None, seed=0, aggr=aggr,
                         fused=False if aggr == "mean" else None)
        assert tr.aggr == aggr and tr.fused is False and tr.model.aggr == aggr
        losses[aggr] = [tr.train_epoch() for _ in range(epochs)]
        assert all(np.isfinite(losses[aggr]))
    assert losses["mean"][-1] < losses["mean"][0]
    assert losses["max"][-1] < losses["max"][0], losses["max"]


# ------------------------------------------------------------------ checks
def test_checks_reject_bad_operands(monkeypatch):
    monkeypatch.setattr(checks, "ENABLED", True)
    rp, col, rng = _toy()
    n, n_src, F = len(rp) - 1, 31, 8
    rp_t, col_t = torch.from_numpy(rp), torch.from_numpy(col)
    X = torch.randn(n_src, F)
    Y, A = ops.pool(rp_t, col_t, X, F)                        # valid operands pass
    rpt, colt, eperm = transpose_csr(rp_t, col_t, n_src, with_perm=True)
    dY = torch.ones(n, F)
    ops.pool_bwd(rpt, colt, eperm, A, dY, F)
    bad = col_t.clone()
    bad[4] = n_src
    with pytest.raises(ValueError, match="CGNN_CHECK"):      # a column out of range
        ops.pool(rp_t, bad, X, F)
    with pytest.raises(ValueError, match="CGNN_CHECK"):      # arg of the wrong dtype (forward)
        ops.pool(rp_t, col_t, X, F, arg=torch.empty(n, F, dtype=torch.int64))
    with pytest.raises(ValueError, match="CGNN_CHECK"):      # a short eperm
        ops.pool_bwd(rpt, colt, eperm[:-1], A, dY, F)
    with pytest.raises(ValueError, match="CGNN_CHECK"):      # arg of the wrong dtype (backward)
        ops.pool_bwd(rpt, colt, eperm, A.long(), dY, F)
    with pytest.raises(ValueError, match="CGNN_CHECK"):      # eperm out of range
        ops.pool_bwd(rpt, colt, eperm + 1, A, dY, F)
    with pytest.raises(ValueError, match="CGNN_CHECK"):      # arg narrower than F
        ops.pool_bwd(rpt, colt, eperm, A, torch.ones(n, 16), 16)
