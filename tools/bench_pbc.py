"""Periodic radius-graph micro-benchmark: the search (``ops.radius_pbc_count`` + the device
cumsum + ``ops.radius_pbc_fill`` with ``shift`` and ``d2``, preallocated buffers, so without the
host sync of ``radius_graph``) per sub-group width, against two baselines that need no periodic
kernel, on the same device in the same rounds:

    hip_replicated   the non-periodic search (``ops.radius_count`` + cumsum + ``ops.radius_fill``)
                     over the explicitly replicated supercell -- every atom copied into every
                     image of the box, one graph of ``n_g * M`` points per cell: the rows of
                     the home atoms are the periodic rows (checked), the other rows are the
                     price of having no image loop
    torch_cdist      ``torch.cdist`` of the atoms against their replicated images and
                     ``nonzero`` of the mask: what a user would write without the kernels (it
                     ends in a host sync, as ``nonzero`` does)

at four shapes, 3-D positions uniform in a cubic cell, cutoff 1, ``n_g`` atoms per cell and ``M``
images (the cell edge sets M: 0.4 -> 7^3, 0.6 -> 5^3, 1.2 and 2.4 -> 3^3):

    tiny     2 atoms, 343 images          small    8 atoms, 125 images
    medium   64 atoms, 27 images          large    512 atoms, 27 images

over ``--rows`` atoms in all (the batch that fills the device).  The runs alternate inside
every round (so drift of the machine hits them alike); a round times ``--inner`` back-to-back
calls of each between device events; the figure is the median over ``--rounds`` rounds, with
the quartiles as the spread.  Prints one JSON line per shape: the times of every sub-group
width, the automatic choice of ``radius_graph``, and both ratios for the automatic choice.

    python tools/bench_pbc.py [--shapes tiny,small,medium,large] [--lanes 8,16,32,64] [--rows 16384]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

# atoms per cell, cell edge (cutoff 1), images per axis
SHAPES = {"tiny": (2, 0.4, 3), "small": (8, 0.6, 2), "medium": (64, 1.2, 1), "large": (512, 2.4, 1)}
R = 1.0


def bench_shape(shape, widths, a):
    from cgnn_amd.gnn import ops
    from cgnn_amd.gnn.geometry import _auto_lanes, image_ranges
    from cgnn_amd.gnn.readout import GraphBatch
    dev = torch.device("cuda", 0)
    m, edge, k = SHAPES[shape]
    G = max(1, a.rows // m)
    b = GraphBatch(torch.arange(G + 1, dtype=torch.int64) * m).to(dev)
    n = b.n
    cell3 = torch.eye(3) * edge
    nimg1 = image_ranges(cell3, True, R)
    assert nimg1.tolist() == [[k, k, k]], nimg1
    M = (2 * k + 1) ** 3
    pos = (torch.rand(n, 3, generator=torch.Generator().manual_seed(1)) * edge).to(dev)
    cell = cell3.reshape(1, 9).repeat(G, 1).to(dev)
    nimg = nimg1.repeat(G, 1).to(dev)
    auto = _auto_lanes(m * M)
    if auto not in widths:
        widths = widths + [auto]
    deg = torch.empty(n, dtype=torch.int32, device=dev)
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    ops.radius_pbc_count(pos, 3, R, b.gptr, b.batch, cell, nimg, lanes=auto, max_images=M, out=deg)
    nnz = int(deg.sum())
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    sh = torch.empty(nnz, dtype=torch.int32, device=dev)
    d2 = torch.empty(nnz, device=dev)

    # the replicated supercell: image s of atom j of cell g is point (g * m + j) * M + s_index
    S = torch.cartesian_prod(*[torch.arange(-k, k + 1)] * 3).float().to(dev) * edge          # [M, 3]
    rpos = (pos[:, None, :] + S[None, :, :]).reshape(n * M, 3).contiguous()
    rb = GraphBatch(torch.arange(G + 1, dtype=torch.int64) * (m * M)).to(dev)
    LR = _auto_lanes(m * M)
    rdeg = ops.radius_count(rpos, 3, R, rb.gptr, rb.batch, lanes=LR)
    rnnz = int(rdeg.sum(dtype=torch.int64))
    if rnnz >= 2 ** 31:
        raise SystemExit("bench_pbc: the replicated supercell has %d edges; lower --rows" % rnnz)
    rrowptr = torch.zeros(n * M + 1, dtype=torch.int32, device=dev)
    rcol = torch.empty(rnnz, dtype=torch.int32, device=dev)
    rd2 = torch.empty(rnnz, device=dev)
    home = M // 2                                             # the index of s = 0 in S
    res = {}

    def hip_pbc(L):
        def run():
            ops.radius_pbc_count(pos, 3, R, b.gptr, b.batch, cell, nimg, lanes=L, max_images=M, out=deg)
            rowptr[1:] = torch.cumsum(deg, 0, dtype=torch.int32)
            ops.radius_pbc_fill(pos, 3, R, b.gptr, b.batch, cell, nimg, rowptr, lanes=L, max_images=M, out=col,
                                shift=sh, d2=d2)
        return run

    def hip_replicated():
        ops.radius_count(rpos, 3, R, rb.gptr, rb.batch, lanes=LR, out=rdeg)
        rrowptr[1:] = torch.cumsum(rdeg, 0, dtype=torch.int32)
        ops.radius_fill(rpos, 3, R, rb.gptr, rb.batch, rrowptr, lanes=LR, out=rcol, d2=rd2)

    def torch_cdist():
        d = torch.cdist(pos.view(G, m, 3), rpos.view(G, m * M, 3))
        idx = torch.arange(m, device=dev)
        d[:, idx, idx * M + home] = float("inf")                # no self loop
        res["cdist"] = (d <= R).nonzero()

    runs = {"hip_pbc_%d" % L: hip_pbc(L) for L in widths}
    runs["hip_replicated"] = hip_replicated
    runs["torch_cdist"] = torch_cdist
    for _ in range(a.warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    first = None
    same = True
    for L in widths:                                         # the CSR does not depend on the width
        runs["hip_pbc_%d" % L]()
        got = (rowptr.clone(), col.clone(), sh.clone())
        first = first or got
        same = same and all(torch.equal(x, y) for x, y in zip(got, first))
    # the home rows of the replicated graph are the periodic rows: the same degrees
    rows_home = (torch.arange(n, device=dev) * M + home).long()
    home_deg_equal = bool(torch.equal(rdeg[rows_home], deg))
    out = {"shape": shape, "graphs": G, "atoms_per_cell": m, "images": M, "cell_edge": edge, "cutoff": R,
           "rows": n, "edges": nnz, "auto_lanes": auto, "replicated_points": n * M, "replicated_edges": rnnz,
           "replicated_lanes": LR, "rounds": a.rounds, "inner": a.inner,
           "every_width_gives_the_same_csr": bool(same), "replicated_home_rows_have_the_same_degrees": home_deg_equal,
           "torch_cdist_edges": int(res["cdist"].shape[0])}
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
    mine = out["hip_pbc_%d_us" % auto]
    out["fastest_lanes"] = min(widths, key=lambda L: out["hip_pbc_%d_us" % L])
    out["replicated_over_pbc"] = round(out["hip_replicated_us"] / mine, 2)
    out["torch_over_pbc"] = round(out["torch_cdist_us"] / mine, 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="tiny,small,medium,large")
    ap.add_argument("--lanes", default="8,16,32,64", help="comma-separated sub-group widths")
    ap.add_argument("--rows", type=int, default=16384, help="atoms in the batch, over all cells")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pbc: no GPU; timings are taken on the device only")
    widths = [int(c) for c in a.lanes.split(",") if c]
    for shape in a.shapes.split(","):
        bench_shape(shape, list(widths), a)


if __name__ == "__main__":
    main()
