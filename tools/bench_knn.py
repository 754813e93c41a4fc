"""k-NN micro-benchmark: the search (``ops.knn_select`` + the device cumsum + ``ops.knn_fill``
with ``d2``, preallocated buffers, so without the host sync of ``knn_graph``) per sub-group
width and k, against two baselines on the same device in the same rounds:

    hip_radius   the radius search (``ops.radius_count`` + cumsum + ``ops.radius_fill``) at the
                 radius that gives the same mean degree: the price of selection over the
                 shared distance pass
    torch_topk   ``torch.cdist`` + ``torch.topk`` on the batch of equal graphs: what a user
                 would write without the kernels (it returns distance order and no CSR)

at three shapes, 3-D positions uniform in a unit cube per graph:

    small        1024 graphs of 64 points
    medium       64 graphs of 512 points
    cloud        one graph of 4096 points

The runs alternate inside every round (so drift of the machine hits them alike); a round
times ``--inner`` back-to-back calls of each between device events; the figure is the median
over ``--rounds`` rounds, with the quartiles as the spread.  Prints one JSON line per
(shape, k): the times of every allowed select width (``lanes >= k``; the fill runs at
``knn_graph``'s own width throughout), the automatic choice of ``knn_graph``, and both ratios
for the automatic choice.

    python tools/bench_knn.py [--shapes small,medium,cloud] [--k 8,16,32,64] [--lanes 8,16,32,64]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SHAPES = {"small": (1024, 64), "medium": (64, 512), "cloud": (1, 4096)}


def bench_shape(shape, k, widths, a):
    from cgnn_amd.gnn import ops
    from cgnn_amd.gnn.geometry import _auto_lanes, _knn_lanes
    from cgnn_amd.gnn.readout import GraphBatch
    dev = torch.device("cuda", 0)
    G, m = SHAPES[shape]
    b = GraphBatch(torch.arange(G + 1, dtype=torch.int64) * m).to(dev)
    n = b.n
    pos = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    auto, LF = _knn_lanes(k, m, n)
    widths = [L for L in widths if L >= k] or [auto]
    if auto not in widths:
        widths.append(auto)
    deg = torch.empty(n, dtype=torch.int32, device=dev)
    td = torch.empty(n, device=dev)
    tj = torch.empty(n, dtype=torch.int32, device=dev)
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    col = torch.empty(n * k, dtype=torch.int32, device=dev)
    d2 = torch.empty(n * k, device=dev)
    # the radius of the same mean degree, by bisection on the count pass (outside the timing)
    LR = _auto_lanes(m)
    want = min(k, m - 1)
    lo, hi = 0.0, 2.0
    for _ in range(30):
        r = 0.5 * (lo + hi)
        mean = float(ops.radius_count(pos, 3, r, b.gptr, b.batch, lanes=LR).float().mean())
        lo, hi = (r, hi) if mean < want else (lo, r)
    r = hi
    rdeg = ops.radius_count(pos, 3, r, b.gptr, b.batch, lanes=LR)
    rnnz = int(rdeg.sum())
    rrowptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    rcol = torch.empty(rnnz, dtype=torch.int32, device=dev)
    rd2 = torch.empty(rnnz, device=dev)
    res = {}

    def hip_knn(L):
        def run():
            ops.knn_select(pos, 3, k, b.gptr, b.batch, lanes=L, deg=deg, tau_d2=td, tau_j=tj)
            rowptr[1:] = torch.cumsum(deg, 0, dtype=torch.int32)
            ops.knn_fill(pos, 3, b.gptr, b.batch, rowptr, td, tj, lanes=LF, out=col, d2=d2)
        return run

    def hip_radius():
        ops.radius_count(pos, 3, r, b.gptr, b.batch, lanes=LR, out=rdeg)
        rrowptr[1:] = torch.cumsum(rdeg, 0, dtype=torch.int32)
        ops.radius_fill(pos, 3, r, b.gptr, b.batch, rrowptr, lanes=LR, out=rcol, d2=rd2)

    def torch_topk():
        p = pos.view(G, m, 3)
        d = torch.cdist(p, p)
        d.diagonal(dim1=1, dim2=2).fill_(float("inf"))
        res["topk"] = torch.topk(d, want, dim=2, largest=False)

    runs = {"hip_knn_%d" % L: hip_knn(L) for L in widths}
    runs["hip_radius"] = hip_radius
    runs["torch_topk"] = torch_topk
    for _ in range(a.warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    first = None
    same = True
    for L in widths:                                         # the CSR does not depend on the width
        runs["hip_knn_%d" % L]()
        got = (rowptr.clone(), col[:int(rowptr[-1])].clone())
        first = first or got
        same = same and torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])
    nnz = int(first[0][-1])
    # the baseline's edges: sorted by id they are the kernel's rows unless a near-tie of the
    # k-th place falls the other way in cdist's rounding (it goes through a matrix product);
    # the fraction of equal rows is reported, not trusted
    ids = (res["topk"].indices + (torch.arange(G, device=dev) * m)[:, None, None]).view(n, want).sort(1).values
    out = {"shape": shape, "graphs": G, "points_per_graph": m, "k": k, "edges": nnz, "auto_lanes": auto, "fill_lanes": LF,
           "radius": round(r, 5), "radius_edges": rnnz, "radius_lanes": LR, "rounds": a.rounds, "inner": a.inner,
           "every_width_gives_the_same_csr": bool(same),
           "torch_topk_rows_equal": float((ids == first[1].view(n, want)).all(1).float().mean()) if nnz == n * want
           else None}
    times = {q: [] for q in runs}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for q, f in runs.items():
            ev0.record()
            for _ in range(a.inner):
                f()
            ev1.record()
            torch.cuda.synchronize()
            times[q].append(ev0.elapsed_time(ev1) / a.inner * 1e3)      # us per call
    for q, t in times.items():
        qs = statistics.quantiles(t, n=4)
        out[q + "_us"] = round(statistics.median(t), 2)
        out[q + "_us_quartiles"] = [round(qs[0], 2), round(qs[2], 2)]
    mine = out["hip_knn_%d_us" % auto]
    out["knn_over_radius"] = round(mine / out["hip_radius_us"], 2)
    out["torch_over_knn"] = round(out["torch_topk_us"] / mine, 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,medium,cloud")
    ap.add_argument("--k", default="8,16,32,64")
    ap.add_argument("--lanes", default="8,16,32,64", help="comma-separated sub-group widths (those >= k are timed)")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn: no GPU; timings are taken on the device only")
    widths = [int(c) for c in a.lanes.split(",") if c]
    for shape in a.shapes.split(","):
        for k in (int(c) for c in a.k.split(",") if c):
            bench_shape(shape, k, widths, a)


if __name__ == "__main__":
    main()
