"""Radius-graph micro-benchmark: the neighbour search (``ops.radius_count`` + the device cumsum
+ ``ops.radius_fill``, with preallocated buffers, so without the host sync of ``radius_graph``)
and the backward of ``pair_distance`` (``ops.pair_d2_bwd``) against a PyTorch composition on the
device -- ``torch.cdist`` on the padded batch, a mask and ``nonzero`` for the search, two
``index_add_`` for the gradient -- at two shapes:

    molecular    2048 graphs of 10-40 points
    midsize      64 graphs of 1000 points

Positions are uniform in a cube whose side gives about ``--neighbours`` neighbours per point
inside ``r = 1``.  ``--lanes`` times the search for several sub-group widths (default: the
automatic choice of ``radius_graph`` alone).

The kernels alternate inside every round (so drift of the machine hits them alike); a round
times ``--inner`` back-to-back calls of each between device events; the figure is the median
over ``--rounds`` rounds, with the quartiles as the spread.  The PyTorch search ends in
``nonzero``, which synchronises with the host; the HIP search does not.  Prints one JSON line
per (shape, lanes).

    python tools/bench_radius.py [--shapes molecular,midsize] [--lanes 8,16,32,64] [--rounds 30] [--inner 10]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def graph_sizes(shape, seed=0):
    if shape == "molecular":
        gen = torch.Generator().manual_seed(seed)
        return torch.randint(10, 41, (2048,), generator=gen)
    if shape == "midsize":
        return torch.full((64,), 1000)
    raise ValueError("unknown shape %r" % shape)


def bench_shape(shape, lanes, a):
    from cgnn_amd.gnn import ops
    from cgnn_amd.gnn.geometry import _auto_lanes, radius_graph
    from cgnn_amd.gnn.readout import GraphBatch
    dev = torch.device("cuda", 0)
    sizes = graph_sizes(shape)
    gptr = torch.zeros(sizes.numel() + 1, dtype=torch.int64)
    gptr[1:] = torch.cumsum(sizes, 0)
    b = GraphBatch(gptr).to(dev)
    n, G, m = b.n, b.n_graphs, b.max_count
    r = 1.0
    # side of each graph's cube: n_g points with `neighbours` of them in a ball of radius r
    side = (sizes.double() * (4.0 / 3.0 * math.pi) / a.neighbours) ** (1.0 / 3.0)
    gen = torch.Generator().manual_seed(1)
    pos = (torch.rand(n, 3, generator=gen) * side[b.batch.cpu().long()].float()[:, None]).to(dev)
    L = _auto_lanes(m) if lanes is None else lanes
    g = radius_graph(pos, r, b, lanes=L)
    nnz = g.col.numel()
    rp_t, col_t, eperm_t = g.transposed_perm()
    gv = torch.randn(nnz, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    deg = torch.empty(n, dtype=torch.int32, device=dev)
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    d2 = torch.empty(nnz, device=dev)
    dpos = torch.empty_like(pos)
    # the padded batch of the PyTorch search
    slot = torch.arange(n, device=dev) - b.gptr.long()[b.batch.long()]
    rows64 = torch.repeat_interleave(torch.arange(n, device=dev), (g.rowptr[1:] - g.rowptr[:-1]).long())
    cols64 = g.col.long()
    res = {}

    def hip_search():
        ops.radius_count(pos, 3, r, b.gptr, b.batch, lanes=L, out=deg)
        rowptr[1:] = torch.cumsum(deg, 0, dtype=torch.int32)
        ops.radius_fill(pos, 3, r, b.gptr, b.batch, rowptr, lanes=L, out=col, d2=d2)

    def torch_search():
        pad = torch.full((G, m, 3), float("inf"), device=dev)
        pad[b.batch.long(), slot] = pos
        d = torch.cdist(pad, pad, compute_mode="donot_use_mm_for_euclid_dist")
        keep = d <= r                                        # inf - inf is NaN: padding drops out
        keep &= ~torch.eye(m, dtype=torch.bool, device=dev)
        gi, i, j = keep.nonzero(as_tuple=True)               # sorted by (graph, i, j)
        off = b.gptr.long()[gi]
        res["torch_rows"], res["torch_cols"] = off + i, off + j

    def hip_bwd():
        ops.pair_d2_bwd(g.rowptr, g.col, rp_t, col_t, eperm_t, pos, gv, 3, out=dpos)

    def torch_bwd():
        w = gv[:, None] * (pos[rows64] - pos[cols64])
        res["torch_dpos"] = 2 * torch.zeros_like(pos).index_add_(0, rows64, w).index_add_(0, cols64, -w)

    runs = {f.__name__: f for f in (hip_search, torch_search, hip_bwd, torch_bwd)}
    for _ in range(a.warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    ref = torch.zeros(n, 3, dtype=torch.float64, device=dev)
    w = gv.double()[:, None] * (pos.double()[rows64] - pos.double()[cols64])
    ref = 2 * ref.index_add_(0, rows64, w).index_add_(0, cols64, -w)
    scale = ref.abs().max()
    out = {"shape": shape, "graphs": G, "points": n, "max_points": m, "edges": nnz, "lanes": L,
           "auto_lanes": _auto_lanes(m), "rounds": a.rounds, "inner": a.inner,
           "hip_search_repeats": bool(torch.equal(col, g.col) and torch.equal(rowptr, g.rowptr)),
           # the baseline's own edge count: it is timed, not trusted (docs/PERF.md)
           "torch_edges": int(res["torch_rows"].numel()),
           "torch_search_equal": bool(torch.equal(res["torch_rows"], rows64) and torch.equal(res["torch_cols"], cols64)),
           "hip_bwd_max_err": float((dpos.double() - ref).abs().max() / scale),
           "torch_bwd_max_err": float((res["torch_dpos"].double() - ref).abs().max() / scale)}
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
    for k, t in times.items():
        q = statistics.quantiles(t, n=4)
        out[k + "_us"] = round(statistics.median(t), 2)
        out[k + "_us_quartiles"] = [round(q[0], 2), round(q[2], 2)]
    for k in ("search", "bwd"):
        out["torch_over_hip_" + k] = round(out["torch_%s_us" % k] / out["hip_%s_us" % k], 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="molecular,midsize")
    ap.add_argument("--lanes", default="", help="comma-separated sub-group widths (default: the automatic choice)")
    ap.add_argument("--neighbours", type=float, default=12.0)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_radius: no GPU; timings are taken on the device only")
    widths = [int(c) for c in a.lanes.split(",") if c] or [None]
    for shape in a.shapes.split(","):
        for L in widths:
            bench_shape(shape, L, a)


if __name__ == "__main__":
    main()
