"""Edge-softmax micro-benchmark: ``ops.edge_softmax`` and ``ops.edge_softmax_bwd`` at K heads
against the PyTorch scatter composition on the same GPU and the same scores -- forward
``index_reduce(amax)``, ``exp``, ``index_add``, divide over a row-id vector; backward a product,
``index_add`` and two gathers -- and against the traffic floor of the forward, one read and
one write of K * nnz * 4 bytes.  Default: the ogbn-arxiv shape, K in {1, 4}.

The kernels alternate inside every round (so drift of the machine hits them alike); a round
times ``--inner`` back-to-back calls of each between device events; the figure is the median
over ``--rounds`` rounds, with the quartiles as the spread.  Prints one JSON line per K.

    python tools/bench_edge_softmax.py [--dataset ogbn-arxiv] [--heads 1 4] [--rounds 50] [--inner 20]
"""
import argparse
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="ogbn-arxiv")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--heads", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lanes", type=int, default=0, help="force the sub-group width (0: the launcher's choice)")
    a = ap.parse_args()
    from cgnn_amd.gnn import ops
    from cgnn_amd.gnn.data import synthetic
    warnings.filterwarnings("ignore", message="index_reduce")
    dev = torch.device("cuda", 0)
    g = synthetic(a.dataset, seed=0, device=dev, scale=a.scale)
    n, nnz = g.n, g.nnz
    rows = ops._row_ids(g.rowptr)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).long()
    gen = torch.Generator(device=dev).manual_seed(0)
    lanes = a.lanes or None
    scale = 0.125
    for K in a.heads:
        s = torch.randn(K, nnz, device=dev, generator=gen) * 3
        dp = torch.randn(K, nnz, device=dev, generator=gen)
        p, ds = torch.empty_like(s), torch.empty_like(s)
        pt, dst = torch.empty_like(s), torch.empty_like(s)
        m = torch.empty(K, n, device=dev)
        l = torch.empty(K, n, device=dev)

        def scatter_fwd():
            m.fill_(float("-inf")).index_reduce_(1, rows, s, "amax")
            ex = torch.exp(scale * (s - m[:, rows]))
            l.zero_().index_add_(1, rows, ex)
            torch.div(ex, l[:, rows], out=pt)

        def scatter_bwd():
            l.zero_().index_add_(1, rows, p * dp)
            torch.mul(p, dp - l[:, rows], out=dst).mul_(scale)

        runs = {
            "fwd": lambda: ops.edge_softmax(g.rowptr, s, scale=scale, out=p, lanes=lanes),
            "bwd": lambda: ops.edge_softmax_bwd(g.rowptr, p, dp, scale=scale, out=ds, lanes=lanes),
            "scatter_fwd": scatter_fwd,
            "scatter_bwd": scatter_bwd,
        }
        for _ in range(a.warmup):
            for f in runs.values():
                f()
        torch.cuda.synchronize()
        err_f = float(((p - pt).abs() / pt.clamp_min(1e-30)).max())
        err_b = float((ds - dst).abs().max())
        times = {k: [] for k in runs}
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.rounds):
            for k, f in runs.items():
                ev0.record()
                for _ in range(a.inner):
                    f()
                ev1.record()
                torch.cuda.synchronize()
                times[k].append(ev0.elapsed_time(ev1) / a.inner * 1e3)      # us per call
        out = {"dataset": g.name, "n": n, "nnz": nnz, "K": K, "lanes": a.lanes, "max_degree": int(deg.max()),
               "edges_in_rows_over_256": int(deg[deg > 256].sum()), "rounds": a.rounds, "inner": a.inner}
        for k, t in times.items():
            q = statistics.quantiles(t, n=4)
            out[k + "_us"] = round(statistics.median(t), 2)
            out[k + "_us_quartiles"] = [round(q[0], 2), round(q[2], 2)]
        out["scatter_fwd_over_fwd"] = round(out["scatter_fwd_us"] / out["fwd_us"], 2)
        out["scatter_bwd_over_bwd"] = round(out["scatter_bwd_us"] / out["bwd_us"], 2)
        # bytes the algorithm needs: the forward reads s and writes p; the backward reads p and
        # dp and writes ds (rowptr is K times smaller than the edge arrays' sum and not counted)
        out["fwd_floor_bytes"] = 2 * K * nnz * 4
        out["fwd_TBps_of_floor_bytes"] = round(2 * K * nnz * 4 / out["fwd_us"] / 1e6, 3)
        out["bwd_TBps_of_floor_bytes"] = round(3 * K * nnz * 4 / out["bwd_us"] / 1e6, 3)
        out["fwd_max_rel_diff_vs_scatter"] = err_f
        out["bwd_max_abs_diff_vs_scatter"] = err_b
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
