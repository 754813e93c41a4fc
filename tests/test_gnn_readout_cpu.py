"""Graph-level readout on CPU tensors: GraphBatch against a dense block-diagonal adjacency,
the CPU branches of ops.seg_reduce / ops.seg_bcast and the autograd functions of
gnn/readout.py against dense fp64 references, argument rejections, GlobalAttention."""
import numpy as np
import pytest
import torch

from cgnn_amd.gnn import ops
from cgnn_amd.gnn.layers import GINEConv, edge_aggregate, pool_aggregate
from cgnn_amd.gnn.readout import GlobalAttention, GraphBatch, graph_broadcast, graph_readout

F64 = torch.float64
R = ops.READOUT_CHUNK


# ------------------------------------------------------------------ GraphBatch
def _toy_graphs():
    """Five graphs: multi-edges, an empty graph (0 nodes), a graph without edges, and the
    three self loops (two in the fourth graph, one in the last) that the input holds itself."""
    return [
        (4, [0, 1, 1, 3, 0], [1, 2, 2, 0, 1]),            # 1 -> 2 twice, 0 -> 1 twice (apart in the input)
        (0, [], []),
        (3, [], []),
        (2, [1, 1, 0], [0, 1, 0]),                        # a self loop on node 1 and on node 0
        (5, [4, 3, 2, 1, 0], [0, 0, 0, 0, 0]),
    ]


def test_from_graphs_matches_the_dense_block_diagonal_adjacency():
    graphs = _toy_graphs()
    b = GraphBatch.from_graphs(graphs)
    sizes = [g[0] for g in graphs]
    n = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    A = np.zeros((n, n), dtype=np.int64)                     # A[dst, src] = multiplicity
    src_all, dst_all = [], []
    for k, (_, s, d) in enumerate(graphs):
        for a, c in zip(s, d):
            A[off[k] + c, off[k] + a] += 1
            src_all.append(off[k] + a)
            dst_all.append(off[k] + c)
    assert b.n == n and b.n_src == n and b.n_graphs == 5
    assert b.rowptr.dtype == torch.int32 and b.col.dtype == torch.int32 and b.eperm.dtype == torch.int64
    rp, col, ep = b.rowptr.numpy(), b.col.numpy(), b.eperm.numpy()
    assert rp[0] == 0 and rp[-1] == len(src_all) == col.size
    got = np.zeros_like(A)
    for i in range(n):
        for e in range(rp[i], rp[i + 1]):
            got[i, col[e]] += 1
    assert np.array_equal(got, A)
    # outside the diagonal blocks there is nothing; no self loop was added
    for k in range(5):
        blk = np.zeros_like(A, dtype=bool)
        blk[off[k]:off[k + 1], off[k]:off[k + 1]] = True
        assert A[blk].sum() == len(graphs[k][1])
    assert np.trace(got) == 3                                  # the three self loops of the input
    # eperm: CSR edge e is input edge eperm[e]; within a row the input order is kept
    src_all, dst_all = np.array(src_all), np.array(dst_all)
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert np.array_equal(dst_all[ep], rows) and np.array_equal(src_all[ep], col)
    assert sorted(ep.tolist()) == list(range(len(src_all)))
    for i in range(n):
        assert np.all(np.diff(ep[rp[i]:rp[i + 1]]) > 0)
    # graph tables
    assert b.gptr.tolist() == off.tolist() and b.gptr.dtype == torch.int32
    assert b.batch.tolist() == np.repeat(np.arange(5), sizes).tolist() and b.batch.dtype == torch.int32
    assert b.count.tolist() == sizes
    exp_inv = [np.float32(1.0 / s) if s else np.float32(0) for s in sizes]
    assert b.inv_count.dtype == torch.float32 and b.inv_count.tolist() == [float(v) for v in exp_inv]
    # the transpose is that of the CSR
    rp_t, col_t, ep_t = b.transposed_perm()
    assert b.transposed_perm() is b.transposed_perm()
    got_t = np.zeros_like(A)
    for j in range(n):
        for t in range(int(rp_t[j]), int(rp_t[j + 1])):
            got_t[int(col_t[t]), j] += 1
            assert col[int(ep_t[t])] == j
    assert np.array_equal(got_t, A)


def test_edge_rows_in_csr_order_through_eperm():
    """espmm over the batch with e_in[eperm] equals the dense sum of edge rows per destination."""
    graphs = _toy_graphs()
    b = GraphBatch.from_graphs(graphs)
    rng = np.random.default_rng(0)
    nnz = b.col.numel()
    e_in = torch.from_numpy(rng.standard_normal((nnz, 8)))
    off = np.concatenate([[0], np.cumsum([g[0] for g in graphs])])
    dst_all = np.concatenate([np.asarray(g[2], dtype=np.int64) + off[k] for k, g in enumerate(graphs)])
    ref = np.zeros((b.n, 8))
    np.add.at(ref, dst_all, e_in.numpy())
    y = edge_aggregate(None, e_in[b.eperm], b)
    np.testing.assert_allclose(y.numpy(), ref, rtol=1e-12, atol=1e-12)
    x = torch.from_numpy(rng.standard_normal((b.n, 8)))
    assert pool_aggregate(x, b).shape == (b.n, 8)              # anything pool_aggregate accepts


def test_chunk_tables():
    b = GraphBatch(torch.tensor([0, 70, 70, 80]), chunk=64)
    assert b.cptr.tolist() == [0, 64, 70, 80] and b.gchunk.tolist() == [0, 2, 2, 3]
    assert b.n_chunks == 3 and not b.single_pass and b.chunk == 64
    assert b.cptr.dtype == torch.int32 and b.gchunk.dtype == torch.int32
    # the default chunk is the exported constant
    lens = [R + 6, 0, 10, 2 * R, R, 1]
    gp = torch.tensor(np.concatenate([[0], np.cumsum(lens)]))
    b = GraphBatch.from_ptr(gp)
    assert b.chunk == R and b.gchunk.tolist() == [0, 2, 2, 3, 5, 6, 7]
    o = np.cumsum([0] + lens)
    assert b.cptr.tolist() == [0, R, o[1], o[3], o[3] + R, o[4], o[5], o[6]]
    assert b.col.numel() == 0 and b.rowptr.tolist() == [0] * (b.n + 1)
    assert GraphBatch.from_ptr(torch.tensor([0, R, R, R + 3])).single_pass
    assert not GraphBatch.from_ptr(torch.tensor([0, R + 1])).single_pass
    e = GraphBatch.from_ptr(torch.tensor([0]))
    assert e.n_graphs == 0 and e.n == 0 and e.single_pass and e.cptr.tolist() == [0] and e.gchunk.tolist() == [0]
    z = GraphBatch.from_graphs([(0, [], []), (0, [], [])])
    assert z.n_graphs == 2 and z.n == 0 and z.n_chunks == 0 and z.gchunk.tolist() == [0, 0, 0]
    c = b.to("cpu")
    assert c is not b and c.chunk == b.chunk and c.cptr.tolist() == b.cptr.tolist()


def test_graph_batch_rejections():
    with pytest.raises(ValueError):
        GraphBatch.from_graphs([(3, [0, 3], [1, 1])])          # a source id outside the graph
    with pytest.raises(ValueError):
        GraphBatch.from_graphs([(3, [0, -1], [1, 1])])
    with pytest.raises(ValueError):
        GraphBatch.from_graphs([(3, [0, 1], [1])])
    with pytest.raises(ValueError):
        GraphBatch.from_ptr(torch.tensor([0, 5, 3]))
    with pytest.raises(ValueError):
        GraphBatch.from_ptr(torch.tensor([1, 5]))
    with pytest.raises(ValueError):
        GraphBatch(torch.tensor([0, 5]), chunk=0)


# ------------------------------------------------------------------ the CPU branches
def _lens():
    return [0, 1, 2, 5, R - 1, R, R + 1, 2 * R + 3, 0, 7]


def _dense_reduce(X, lens, reduce):
    """fp64 [G, F] and the first-index arg, from numpy."""
    o = np.concatenate([[0], np.cumsum(lens)])
    Y = np.zeros((len(lens), X.shape[1]))
    A = np.full((len(lens), X.shape[1]), -1, dtype=np.int64)
    for g, m in enumerate(lens):
        if m == 0:
            continue
        v = X[o[g]:o[g + 1]]
        if reduce in ("sum", "mean"):
            Y[g] = v.sum(0) / (m if reduce == "mean" else 1)
        else:
            k = np.argmin(v, 0) if reduce == "min" else np.argmax(v, 0)
            Y[g] = v[k, np.arange(X.shape[1])]
            A[g] = o[g] + k
    return Y, A


@pytest.mark.parametrize("reduce", ["sum", "max", "min"])
def test_seg_reduce_cpu_branch_against_dense_fp64(reduce):
    lens = _lens()
    rng = np.random.default_rng(3)
    n, F, ld = sum(lens), 11, 16
    X = torch.full((n + 2, ld), 1e4, dtype=F64)
    X[:n, :F] = torch.from_numpy(rng.integers(-4, 5, (n, F)).astype(np.float64))      # ties
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    Yr, Ar = _dense_reduce(X[:n, :F].numpy(), lens, reduce)
    for dt in (F64, torch.float32, torch.bfloat16):
        Y, A = ops.seg_reduce(ptr, X.to(dt), F, reduce, with_arg=reduce != "sum")
        assert Y.dtype == dt and Y.shape == (len(lens), ld)
        assert torch.equal(Y[:, :F].double(), torch.from_numpy(Yr)) and torch.all(Y[:, F:] == 0)
        if reduce == "sum":
            assert A is None
        else:
            assert A.dtype == torch.int32 and torch.equal(A[:, :F].long(), torch.from_numpy(Ar))
            assert torch.all(A[:, F:] == -1) and torch.all(A[0] == -1)
    if reduce == "sum":
        rs = torch.tensor(rng.integers(1, 4, len(lens)).astype(np.float32))
        Y, _ = ops.seg_reduce(ptr, X, F, "sum", rscale=rs, out_dtype=F64)
        assert torch.equal(Y[:, :F], torch.from_numpy(Yr) * rs.double()[:, None])
        Y, _ = ops.seg_reduce(ptr, X.float(), F, "sum", out_dtype=torch.bfloat16)
        assert Y.dtype == torch.bfloat16 and torch.equal(Y[:, :F].double(), torch.from_numpy(Yr).bfloat16().double())
    else:
        # the second pass hands indices through: arg = arg_in[row]
        arg_in = torch.full((n, ld), -7, dtype=torch.int32)
        arg_in[:, :F] = torch.from_numpy(rng.integers(0, 1000, (n, F)).astype(np.int32))
        _, A2 = ops.seg_reduce(ptr, X, F, reduce, arg_in=arg_in, with_arg=True)
        exp = torch.where(torch.from_numpy(Ar) >= 0,
                          torch.gather(arg_in[:, :F].long(), 0, torch.from_numpy(Ar).clamp_min(0)), torch.tensor(-1))
        assert torch.equal(A2[:, :F].long(), exp) and torch.all(A2[:, F:] == -1)
        Y0, A0 = ops.seg_reduce(ptr, X, F, reduce)
        assert A0 is None and torch.equal(Y0[:, :F], torch.from_numpy(Yr))


def test_seg_reduce_cpu_nan_rule():
    nan, inf = float("nan"), float("inf")
    rows = [[1.0, nan, 3.0], [nan, 5.0], [-inf, -inf], [inf], [2.0, 2.0, 2.0]]
    lens = [len(r) for r in rows]
    X = torch.tensor([v for r in rows for v in r], dtype=F64)[:, None].expand(-1, 8).contiguous()
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    Y, A = ops.seg_reduce(ptr, X, 8, "max", with_arg=True)
    assert torch.isnan(Y[0, 0]) and int(A[0, 0]) == 1 and torch.isnan(Y[1, 0]) and int(A[1, 0]) == 3
    assert float(Y[2, 0]) == -inf and int(A[2, 0]) == 5 and int(A[4, 0]) == 8
    Y, A = ops.seg_reduce(ptr, X, 8, "min", with_arg=True)
    assert torch.isnan(Y[0, 0]) and int(A[0, 0]) == 1 and float(Y[3, 0]) == inf and int(A[3, 0]) == 7


def test_seg_bcast_cpu_branch_against_dense_fp64():
    lens = _lens()
    rng = np.random.default_rng(4)
    n, G, F, ld = sum(lens), len(lens), 11, 16
    seg = torch.from_numpy(np.repeat(np.arange(G), lens).astype(np.int32))
    U = torch.full((G, ld), 1e4, dtype=F64)
    U[:, :F] = torch.from_numpy(rng.standard_normal((G, F)))
    rs = torch.from_numpy(rng.standard_normal(G).astype(np.float32))
    out = ops.seg_bcast(seg, U, F)
    assert torch.equal(out[:, :F], U[seg.long(), :F]) and torch.all(out[:, F:] == 0) and out.shape == (n, ld)
    out = ops.seg_bcast(seg, U, F, rscale=rs)
    assert torch.equal(out[:, :F], U[seg.long(), :F] * rs.double()[seg.long(), None])
    arg = torch.full((G, ld), -1, dtype=torch.int32)
    o = np.concatenate([[0], np.cumsum(lens)])
    for g, m in enumerate(lens):
        if m:
            arg[g, :F] = torch.from_numpy(rng.integers(o[g], o[g + 1], F).astype(np.int32))
    out = ops.seg_bcast(seg, U, F, arg=arg)
    exp = torch.zeros(n, F, dtype=F64)
    for g in range(G):
        for f in range(F):
            if arg[g, f] >= 0:
                exp[int(arg[g, f]), f] = U[g, f]
    assert torch.equal(out[:, :F], exp) and torch.all(out[:, F:] == 0)
    assert ops.seg_bcast(seg, U.float(), F, out_dtype=torch.bfloat16).dtype == torch.bfloat16


@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
def test_graph_readout_two_level_equals_dense(reduce):
    """The chunked schedule (graphs longer than a chunk) and the single launch agree with the
    dense reference, values and gradient routing."""
    lens = _lens()
    rng = np.random.default_rng(5)
    n, F = sum(lens), 5
    xd = torch.from_numpy(rng.permutation(n * F).reshape(n, F).astype(np.float64))    # distinct values
    gp = torch.tensor(np.concatenate([[0], np.cumsum(lens)]))
    Yr, Ar = _dense_reduce(xd.numpy(), lens, reduce)
    gy = torch.from_numpy(rng.integers(-3, 4, (len(lens), F)).astype(np.float64))
    seg = np.repeat(np.arange(len(lens)), lens)
    if reduce in ("sum", "mean"):
        scale = np.array([1.0 / m if (m and reduce == "mean") else 1.0 for m in lens])
        dxr = gy.numpy()[seg] * scale[seg][:, None]
    else:
        dxr = np.zeros((n, F))
        for g in range(len(lens)):
            for f in range(F):
                if Ar[g, f] >= 0:
                    dxr[Ar[g, f], f] = gy[g, f]
    for chunk in (None, 4, 10 ** 6):
        b = GraphBatch(gp, chunk=chunk)
        assert b.single_pass == (chunk == 10 ** 6)
        x = xd.clone().requires_grad_()
        y = graph_readout(x, b, reduce)
        assert y.shape == (len(lens), F) and y.dtype == F64
        np.testing.assert_allclose(y.detach().numpy(), Yr, rtol=1e-7, atol=0)        # inv_count is fp32
        y.backward(gy)
        np.testing.assert_allclose(x.grad.numpy(), dxr, rtol=1e-7, atol=0)
        with torch.no_grad():
            assert torch.equal(graph_readout(xd, b, reduce), y.detach())              # without the index


@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
def test_gradcheck_graph_readout(reduce):
    lens = [3, 0, 1, 9, 4]
    rng = np.random.default_rng(6)
    n, F = sum(lens), 3
    x = torch.from_numpy(rng.permutation(n * F).reshape(n, F).astype(np.float64)).requires_grad_()   # distinct
    b = GraphBatch(torch.tensor(np.concatenate([[0], np.cumsum(lens)])), chunk=4)
    assert not b.single_pass
    assert torch.autograd.gradcheck(lambda t: graph_readout(t, b, reduce), (x,), eps=1e-4, atol=1e-6)


def test_gradcheck_graph_broadcast():
    lens = [3, 0, 1, 9, 4]
    rng = np.random.default_rng(7)
    u = torch.from_numpy(rng.standard_normal((len(lens), 3))).requires_grad_()
    b = GraphBatch(torch.tensor(np.concatenate([[0], np.cumsum(lens)])), chunk=4)
    scale = torch.tensor([0.5, 2.0, -1.0, 0.25, 3.0])
    assert torch.autograd.gradcheck(lambda t: graph_broadcast(t, b), (u,))
    assert torch.autograd.gradcheck(lambda t: graph_broadcast(t, b, scale), (u,))
    out = graph_broadcast(u.detach(), b, scale)
    assert torch.equal(out, u.detach()[b.batch.long()] * scale.double()[b.batch.long(), None])


# ------------------------------------------------------------------ rejections
def test_argument_rejections():
    b = GraphBatch.from_ptr(torch.tensor([0, 3, 5]))
    x = torch.zeros(5, 4)
    ptr = b.gptr
    with pytest.raises(ValueError):
        graph_readout(x, b, "prod")
    with pytest.raises(ValueError):
        graph_readout(torch.zeros(6, 4), b)
    with pytest.raises(ValueError):
        graph_readout(torch.zeros(5), b)
    with pytest.raises(ValueError):
        graph_broadcast(torch.zeros(3, 4), b)
    with pytest.raises(ValueError):
        graph_broadcast(torch.zeros(2, 4), b, scale=torch.ones(3))
    with pytest.raises(ValueError):
        graph_broadcast(torch.zeros(2, 4), b, scale=torch.ones(2, requires_grad=True))
    xp = torch.zeros(5, 8)
    with pytest.raises(ValueError):
        ops.seg_reduce(ptr, xp, 4, "mean")
    with pytest.raises(ValueError):
        ops.seg_reduce(ptr, xp, 4, "sum", with_arg=True)
    with pytest.raises(ValueError):
        ops.seg_reduce(ptr, xp, 4, "sum", arg_in=torch.zeros(5, 8, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.seg_reduce(ptr, xp, 4, "max", rscale=torch.ones(2))
    with pytest.raises(TypeError):
        ops.seg_reduce(ptr, xp, 4, "max", out=torch.zeros(2, 8, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.seg_bcast(b.batch, torch.zeros(2, 8), 4, rscale=torch.ones(2), arg=torch.zeros(2, 8, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.seg_bcast(b.batch, torch.zeros(0, 8), 4)


def test_checks_validate_the_segment_operands(monkeypatch):
    from cgnn_amd.utils import checks
    monkeypatch.setattr(checks, "ENABLED", True)
    xp = torch.zeros(5, 8)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    ops.seg_reduce(i32([0, 3, 5]), xp, 4)
    for bad in ([1, 3, 5], [0, 4, 3], [0, 3, 6]):               # start, monotone, end
        with pytest.raises(ValueError, match="CGNN_CHECK"):
            ops.seg_reduce(i32(bad), xp, 4)
    with pytest.raises(ValueError, match="CGNN_CHECK"):
        ops.seg_reduce(i32([0, 3, 5]), xp, 4, "max", arg=torch.zeros(2, 12, dtype=torch.int32))
    with pytest.raises(ValueError, match="CGNN_CHECK"):
        ops.seg_reduce(i32([0, 3, 5]), xp, 4, "max", arg=torch.zeros(1, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match="CGNN_CHECK"):
        ops.seg_reduce(i32([0, 3, 5]), xp, 4, "max", with_arg=True, arg_in=torch.zeros(4, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match="CGNN_CHECK"):
        ops.seg_reduce(i32([0, 3, 5]), xp, 4, rscale=torch.ones(1))
    u = torch.zeros(2, 8)
    ops.seg_bcast(i32([0, 0, 1]), u, 4)
    for bad in ([0, 2, 1], [-1, 0, 1]):
        with pytest.raises(ValueError, match="CGNN_CHECK"):
            ops.seg_bcast(i32(bad), u, 4)
    with pytest.raises(ValueError, match="CGNN_CHECK"):
        ops.seg_bcast(i32([0, 0, 1]), u, 4, arg=torch.zeros(2, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match="CGNN_CHECK"):
        ops.seg_bcast(i32([0, 0, 1]), u, 4, out=torch.zeros(2, 8))


# ------------------------------------------------------------------ GlobalAttention
def test_global_attention_shapes_and_semantics():
    lens = [3, 0, 1, 9, 4]
    rng = np.random.default_rng(8)
    n, F, H = sum(lens), 6, 4
    b = GraphBatch(torch.tensor(np.concatenate([[0], np.cumsum(lens)])), chunk=4)
    gen = torch.Generator().manual_seed(0)
    gate = torch.nn.Linear(F, 1).double()
    nn = torch.nn.Linear(F, H).double()
    with torch.no_grad():
        for p in list(gate.parameters()) + list(nn.parameters()):
            p.copy_(torch.randn(p.shape, generator=gen, dtype=F64))
    x = torch.from_numpy(rng.standard_normal((n, F))).requires_grad_()
    layer = GlobalAttention(gate, nn)
    out, alpha = layer(x, b, return_attention=True)
    assert out.shape == (len(lens), H) and alpha.shape == (n,)
    o = np.concatenate([[0], np.cumsum(lens)])
    ref = torch.zeros(len(lens), H, dtype=F64)
    for g, m in enumerate(lens):
        if m:
            xs = x.detach()[o[g]:o[g + 1]]
            a = torch.softmax(gate(xs)[:, 0], 0)
            assert torch.allclose(alpha[o[g]:o[g + 1]], a, rtol=1e-12, atol=1e-14)
            ref[g] = (a[:, None] * nn(xs)).sum(0)
    assert torch.allclose(out, ref.detach(), rtol=1e-12, atol=1e-13) and torch.all(out[1] == 0)
    assert torch.allclose(graph_readout(alpha[:, None], b, "sum")[[0, 2, 3, 4], 0], torch.ones(4, dtype=F64))
    assert torch.autograd.gradcheck(lambda t: layer(t, b), (x,))
    plain = GlobalAttention(gate)(x, b)
    assert plain.shape == (len(lens), F)
    with pytest.raises(ValueError):
        GlobalAttention(torch.nn.Linear(F, 2).double())(x, b)          # one gate column only


def test_gine_readout_linear_trains_on_the_cpu():
    """GINEConv -> graph_readout("mean") -> Linear on a GraphBatch with edge features."""
    rng = np.random.default_rng(9)
    graphs = []
    for _ in range(6):
        m = int(rng.integers(3, 12))
        k = int(rng.integers(m, 3 * m))
        graphs.append((m, rng.integers(0, m, k), rng.integers(0, m, k)))
    b = GraphBatch.from_graphs(graphs)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(b.n, 8, generator=gen)
    e = torch.randn(b.col.numel(), 3, generator=gen)[b.eperm]
    target = torch.randn(b.n_graphs, 2, generator=gen)
    torch.manual_seed(0)
    conv = GINEConv(torch.nn.Linear(8, 8), in_dim=8, edge_dim=3, generator=gen)
    head = torch.nn.Linear(8, 2)
    opt = torch.optim.Adam(list(conv.parameters()) + list(head.parameters()), lr=0.05)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = ((head(graph_readout(conv(x, b, e), b, "mean")) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0]
