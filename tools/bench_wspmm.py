"""Edge-weighted SpMM / SDDMM micro-benchmark: ``ops.wspmm`` with unit values against
``ops.spmm(..., cscale=...)`` on the same graph (the cost of reading one fp32 value per
edge), with ``ops.sddmm`` beside them.  Default: the ogbn-arxiv shape, F = 128, bf16.

The three kernels alternate inside every round (so drift of the machine hits them alike);
a round times ``--inner`` back-to-back launches of each between device events; the figure
is the median over ``--rounds`` rounds, with the quartiles as the spread.  Prints one JSON
line.

    python tools/bench_wspmm.py [--dataset ogbn-arxiv] [--F 128] [--rounds 50] [--inner 20]
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
    a = ap.parse_args()
    from cgnn_amd.gnn import ops
    from cgnn_amd.gnn.data import synthetic
    dev = torch.device("cuda", 0)
    g = synthetic(a.dataset, seed=0, device=dev, scale=a.scale)
    n, nnz, F = g.n, g.nnz, a.F
    ld = -(-F // 8) * 8
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.zeros(n, ld, device=dev)
    X[:, :F] = torch.randn(n, F, device=dev, generator=gen)
    X = X.to(torch.bfloat16)
    A = torch.zeros(n, ld, device=dev)
    A[:, :F] = torch.randn(n, F, device=dev, generator=gen)
    A = A.to(torch.bfloat16)
    val = torch.ones(nnz, device=dev)
    Y0 = torch.empty(n, ld, device=dev, dtype=torch.bfloat16)
    Y1 = torch.empty(n, ld, device=dev, dtype=torch.bfloat16)
    D = torch.empty(nnz, device=dev)
    runs = {
        "spmm": lambda: ops.spmm(g.rowptr, g.col, X, F, rscale=g.dinv, cscale=g.dinv, out=Y0),
        "wspmm": lambda: ops.wspmm(g.rowptr, g.col, val, X, F, rscale=g.dinv, cscale=g.dinv, out=Y1),
        "sddmm": lambda: ops.sddmm(g.rowptr, g.col, A, X, F, rscale=g.dinv, cscale=g.dinv, out=D),
    }
    for _ in range(a.warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    # the two aggregates sum the same products in different orders: last-bit differences only
    diff = float((Y0.float() - Y1.float()).abs().max())
    scale = float(Y0.float().abs().max())
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
    out["wspmm_over_spmm"] = round(out["wspmm_us"] / out["spmm_us"], 3)
    out["wspmm_gather_TBps"] = round(nnz * F * 2 / out["wspmm_us"] / 1e6, 3)
    out["max_abs_diff_wspmm_spmm"] = diff
    out["max_abs_output"] = scale
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
