"""Max / min pooling micro-benchmark: ``ops.pool`` (with and without the arg index) and
``ops.pool_bwd`` against ``ops.spmm`` and ``ops.wspmm`` on the same graph and features -- the
sum kernels gather exactly the bytes the pooling forward gathers -- and against the
``torch.scatter_reduce(..., "amax")`` formulation where its nnz x F temporary fits.
Default: the ogbn-arxiv shape, F = 128, bf16 (the graph and widths of tools/bench_wspmm.py).

The kernels alternate inside every round (so drift of the machine hits them alike); a round
times ``--inner`` back-to-back launches of each between device events; the figure is the
median over ``--rounds`` rounds, with the quartiles as the spread.  Prints one JSON line.

    python tools/bench_pool.py [--dataset ogbn-arxiv] [--F 128] [--rounds 50] [--inner 20]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="ogbn-arxiv")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--F", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scatter-max-bytes", type=float, default=8e9,
                    help="run the scatter_reduce formulation when its nnz x F temporaries fit in this")
    a = ap.parse_args()
    from cgnn_amd.gnn import ops
    from cgnn_amd.gnn.data import synthetic
    from cgnn_amd.gnn.sage import transpose_csr
    dev = torch.device("cuda", 0)
    g = synthetic(a.dataset, seed=0, device=dev, scale=a.scale)
    n, nnz, F = g.n, g.nnz, a.F
    ld = -(-F // 8) * 8
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.zeros(n, ld, device=dev)
    X[:, :F] = torch.randn(n, F, device=dev, generator=gen)
    X = X.to(torch.bfloat16)
    dY = torch.zeros(n, ld, device=dev)
    dY[:, :F] = torch.randn(n, F, device=dev, generator=gen)
    dY = dY.to(torch.bfloat16)
    val = torch.ones(nnz, device=dev)
    rp_t, col_t, eperm = transpose_csr(g.rowptr, g.col, n, with_perm=True)
    new = lambda dt=torch.bfloat16: torch.empty(n, ld, device=dev, dtype=dt)
    Ys, Yw, Yp, Yq, dX, A = new(), new(), new(), new(), new(), new(torch.int32)
    runs = {
        "spmm": lambda: ops.spmm(g.rowptr, g.col, X, F, out=Ys),
        "wspmm": lambda: ops.wspmm(g.rowptr, g.col, val, X, F, out=Yw),
        "pool_noarg": lambda: ops.pool(g.rowptr, g.col, X, F, out=Yq, with_arg=False),
        "pool": lambda: ops.pool(g.rowptr, g.col, X, F, out=Yp, arg=A),
        "pool_bwd": lambda: ops.pool_bwd(rp_t, col_t, eperm, A, dY, F, out=dX),
    }
    # the PyTorch formulation: an nnz x F gather, then an atomic scatter-max (no arg)
    scatter_bytes = nnz * F * 2 + nnz * F * 8
    if scatter_bytes <= a.scatter_max_bytes:
        rows = ops._row_ids(g.rowptr)
        index = rows[:, None].expand(nnz, F)
        col64 = g.col.long()
        Yt = torch.empty(n, F, device=dev, dtype=torch.bfloat16)

        def scatter():
            Yt.zero_()
            Yt.scatter_reduce_(0, index, X[col64, :F], "amax", include_self=False)
        runs["scatter_amax"] = scatter
    for _ in range(a.warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    same = bool(torch.equal(Yp, Yq))
    if "scatter_amax" in runs:
        same = same and bool(torch.equal(Yp[:, :F], Yt))
    times = {k: [] for k in runs}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for k, f in runs.items():
            ev0.record()
            for _ in range(a.inner):
                f()
            ev1.record()
            torch.cuda.synchronize()
            times[k].append(ev0.elapsed_time(ev1) / a.inner * 1e3)      # us per launch
    out = {"dataset": g.name, "n": n, "nnz": nnz, "F": F, "dtype": "bf16", "rounds": a.rounds, "inner": a.inner}
    for k, t in times.items():
        q = statistics.quantiles(t, n=4)
        out[k + "_us"] = round(statistics.median(t), 2)
        out[k + "_us_quartiles"] = [round(q[0], 2), round(q[2], 2)]
    for k in ("pool_noarg", "pool", "pool_bwd"):
        out[k + "_over_spmm"] = round(out[k + "_us"] / out["spmm_us"], 3)
        out[k + "_over_wspmm"] = round(out[k + "_us"] / out["wspmm_us"], 3)
    if "scatter_amax" in runs:
        out["scatter_amax_over_pool"] = round(out["scatter_amax_us"] / out["pool_us"], 2)
    # bytes the algorithm needs: the gathered rows (+ the arg and gradient rows of the backward)
    out["pool_gather_TBps"] = round(nnz * F * 2 / out["pool_noarg_us"] / 1e6, 3)
    out["pool_bwd_gather_TBps"] = round(nnz * F * (4 + 2) / out["pool_bwd_us"] / 1e6, 3)
    out["outputs_equal"] = same
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
