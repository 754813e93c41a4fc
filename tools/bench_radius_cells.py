"""Cell-list radius search against the brute-force search, one point cloud per shape, with
``tools/bench_radius.py``'s method: the two searches alternate inside every round (so drift of
the machine hits them alike); a round times ``--inner`` back-to-back calls of each between
device events; the figure is the median over ``--rounds`` rounds, with the quartiles as the
spread.  Buffers are preallocated, so neither search synchronises with the host.

    cells   ops.cells_grid + cells_bin + cells_order + cells_count + the device cumsum +
            ops.cells_fill (search with stores, then the row pass): every step from the grid
            to the ordered rows
    brute   ops.radius_count + the device cumsum + ops.radius_fill

Positions are uniform in a cube whose side gives about ``--neighbours`` neighbours per point
inside ``r = 1``.  From ``--brute-once`` points on, the brute search is run once (after one
warm-up) instead of in rounds.  The steps of the cell path are then timed one by one in the
same way (``steps_us``).  Both CSRs are compared (``equal``).  Prints one JSON line per (points,
neighbours, lanes).

    python tools/bench_radius_cells.py [--points 4096,16384,65536,262144,1048576] [--neighbours 12,40]
                                       [--lanes 8,16] [--rounds 20] [--inner 5]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed(fns, rounds, inner):
    """{name: [us per call, one per round]} with the functions alternating inside a round."""
    times = {k: [] for k in fns}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for k, f in fns.items():
            ev0.record()
            for _ in range(inner):
                f()
            ev1.record()
            torch.cuda.synchronize()
            times[k].append(ev0.elapsed_time(ev1) / inner * 1e3)
    return times


def summary(t):
    if len(t) == 1:
        return round(t[0], 2), None
    q = statistics.quantiles(t, n=4)
    return round(statistics.median(t), 2), [round(q[0], 2), round(q[2], 2)]


def bench_shape(n, neighbours, lanes, a):
    from cgnn_amd import native
    from cgnn_amd.gnn import ops
    from cgnn_amd.gnn.geometry import _CELLS_MIN_POINTS, _auto_lanes
    dev = torch.device("cuda", 0)
    r, D, G = 1.0, 3, 1
    side = (n * (4.0 / 3.0 * math.pi) / neighbours) ** (1.0 / 3.0)
    pos = (torch.rand(n, 3, generator=torch.Generator().manual_seed(1)) * side).to(dev)
    gptr = torch.tensor([0, n], dtype=torch.int32, device=dev)
    seg = torch.zeros(n, dtype=torch.int32, device=dev)
    LB = _auto_lanes(n)
    # one pass with a read-back for the number of edges
    _, gn0, _, perm0, scell0, cptr0, spos0 = ops.cells_prepare(pos, D, r, gptr, seg)
    nnz = int(ops.cells_count(spos0, perm0, scell0, cptr0, gptr, seg, gn0, D, r, lanes=lanes).sum())
    del perm0, scell0, cptr0, spos0
    glo = torch.empty(G, 8, device=dev)
    gn = torch.empty(G, 4, dtype=torch.int32, device=dev)
    part = torch.empty(native.hip().gnn_cells_grid_floats(n), device=dev)
    cid = torch.empty(n, dtype=torch.int32, device=dev)
    deg = torch.empty(n, dtype=torch.int32, device=dev)
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    col, sj, bcol = (torch.empty(nnz, dtype=torch.int32, device=dev) for _ in range(3))
    d2, sd, bd2 = (torch.empty(nnz, device=dev) for _ in range(3))
    bdeg = torch.empty(n, dtype=torch.int32, device=dev)
    browptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    st = {}

    def grid():
        ops.cells_grid(pos, D, r, gptr, glo=glo, gn=gn, part=part)

    def bins():
        ops.cells_bin(pos, D, gptr, seg, glo, gn, out=cid)

    def order():
        st["perm"], st["scell"], st["cptr"], st["spos"] = ops.cells_order(pos, D, cid, G)

    def count():
        ops.cells_count(st["spos"], st["perm"], st["scell"], st["cptr"], gptr, seg, gn, D, r, lanes=lanes, out=deg)

    def cumsum():
        rowptr[1:] = torch.cumsum(deg, 0, dtype=torch.int32)

    def fill():
        ops.cells_fill(st["spos"], st["perm"], st["scell"], st["cptr"], gptr, seg, gn, D, r, rowptr, lanes=lanes,
                       out=col, d2=d2, scratch=(sj, sd))

    def rows():                                              # the second launch of cells_fill, alone
        native.hip().gnn_cells_rows(rowptr.data_ptr(), sj.data_ptr(), sd.data_ptr(), col.data_ptr(), d2.data_ptr(), n,
                                    nnz, 0, torch.cuda.current_stream().cuda_stream)

    steps = {f.__name__: f for f in (grid, bins, order, count, cumsum, fill, rows)}

    def cells():
        for k, f in steps.items():
            if k != "rows":
                f()

    def brute():
        ops.radius_count(pos, D, r, gptr, seg, lanes=LB, out=bdeg)
        browptr[1:] = torch.cumsum(bdeg, 0, dtype=torch.int32)
        ops.radius_fill(pos, D, r, gptr, seg, browptr, lanes=LB, out=bcol, d2=bd2)

    once = n >= a.brute_once
    for _ in range(a.warmup):
        cells()
    brute()
    torch.cuda.synchronize()
    out = {"points": n, "neighbours": neighbours, "edges": nnz, "edges_per_point": round(nnz / n, 2),
           "cells": gn[0].tolist(), "lanes": lanes or "default", "brute_lanes": LB, "rounds": a.rounds,
           "inner": a.inner, "brute_once": once, "cells_min_points": _CELLS_MIN_POINTS,
           "equal": bool(torch.equal(rowptr, browptr) and torch.equal(col, bcol)
                         and torch.equal(d2.view(torch.int32), bd2.view(torch.int32)))}
    if once:
        t = timed({"cells": cells}, a.rounds, a.inner)
        t.update(timed({"brute": brute}, 1, 1))
    else:
        t = timed({"cells": cells, "brute": brute}, a.rounds, a.inner)
    for k, v in t.items():
        out[k + "_us"], out[k + "_us_quartiles"] = summary(v)
    out["brute_over_cells"] = round(out["brute_us"] / out["cells_us"], 2)
    ts = timed(steps, a.rounds, a.inner)
    out["steps_us"] = {k: summary(v)[0] for k, v in ts.items()}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096,16384,65536,262144,1048576")
    ap.add_argument("--neighbours", default="12,40")
    ap.add_argument("--lanes", default="", help="comma-separated sub-group widths of the cell search (default: its own)")
    ap.add_argument("--brute-once", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_radius_cells: no GPU; timings are taken on the device only")
    widths = [int(c) for c in a.lanes.split(",") if c] or [None]
    for n in (int(c) for c in a.points.split(",")):
        for nb in (float(c) for c in a.neighbours.split(",")):
            for L in widths:
                bench_shape(n, nb, L, a)


if __name__ == "__main__":
    main()
