"""Graph-readout micro-benchmark: the sum, the max (with its arg index) and the sum's backward
of ``gnn/readout.py`` (``ops.seg_reduce`` / ``ops.seg_bcast``, one launch or the two-level
schedule) against the same results formed with PyTorch's own ops on the device --
``index_add_``, ``scatter_reduce_(..., "amax")`` and indexing ``dY[batch]`` -- at two shapes:

    molecular    4096 graphs of 8-40 nodes, F = 128, bf16
    large        4 graphs of 250 000 nodes, F = 128, bf16

``--chunks`` times the two-level schedule for several chunk sizes (default: the exported
``ops.READOUT_CHUNK`` alone); a shape whose graphs all fit one chunk runs as a single launch
whatever the value.

The kernels alternate inside every round (so drift of the machine hits them alike); a round
times ``--inner`` back-to-back calls of each between device events; the figure is the median
over ``--rounds`` rounds, with the quartiles as the spread.  The kernels are pure streams, so
each HIP figure comes with the bandwidth it achieved on the bytes the result needs (the node
rows once, the graph rows once).  Prints one JSON line per (shape, chunk).

    python tools/bench_readout.py [--shapes molecular,large] [--chunks 64,256] [--rounds 50] [--inner 20]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def graph_sizes(shape, seed=0):
    if shape == "molecular":
        gen = torch.Generator().manual_seed(seed)
        return torch.randint(8, 41, (4096,), generator=gen)
    if shape == "large":
        return torch.full((4,), 250000)
    raise ValueError("unknown shape %r" % shape)


def bench_shape(shape, chunk, a):
    from cgnn_amd.gnn import ops
    from cgnn_amd.gnn.readout import GraphBatch, _reduce
    dev = torch.device("cuda", 0)
    sizes = graph_sizes(shape)
    gptr = torch.zeros(sizes.numel() + 1, dtype=torch.int64)
    gptr[1:] = torch.cumsum(sizes, 0)
    b = GraphBatch(gptr, chunk=chunk).to(dev)
    n, G, F = b.n, b.n_graphs, a.F
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(n, F, device=dev, generator=gen).to(torch.bfloat16)
    dY = torch.randn(G, F, device=dev, generator=gen).to(torch.bfloat16)
    batch64 = b.batch.long()
    index = batch64[:, None].expand(n, F)
    res = {}

    def hip_sum():
        res["hip_sum"] = _reduce(X, F, b, "sum")[0]

    def hip_max():
        res["hip_max"], res["hip_arg"] = _reduce(X, F, b, "max", with_arg=True)

    def hip_sum_bwd():
        res["hip_sum_bwd"] = ops.seg_bcast(b.batch, dY, F)

    def torch_sum():
        res["torch_sum"] = torch.zeros(G, F, dtype=X.dtype, device=dev).index_add_(0, batch64, X)

    def torch_max():
        res["torch_max"] = torch.zeros(G, F, dtype=X.dtype, device=dev).scatter_reduce_(0, index, X, "amax",
                                                                                      include_self=False)

    def torch_sum_bwd():
        res["torch_sum_bwd"] = dY[batch64]

    runs = {f.__name__: f for f in (hip_sum, torch_sum, hip_max, torch_max, hip_sum_bwd, torch_sum_bwd)}
    for _ in range(a.warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    ref = torch.zeros(G, F, dtype=torch.float64, device=dev).index_add_(0, batch64, X.double())
    out = {"shape": shape, "graphs": G, "nodes": n, "F": F, "dtype": "bf16", "chunk": b.chunk,
           "single_pass": b.single_pass, "chunks": b.n_chunks, "rounds": a.rounds, "inner": a.inner,
           "max_equal": bool(torch.equal(res["hip_max"], res["torch_max"])),
           "bwd_equal": bool(torch.equal(res["hip_sum_bwd"], res["torch_sum_bwd"])),
           "hip_sum_max_rel_err": float(((res["hip_sum"].double() - ref).abs() / ref.abs().clamp_min(1)).max()),
           "torch_sum_max_rel_err": float(((res["torch_sum"].double() - ref).abs() / ref.abs().clamp_min(1)).max())}
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
    for k in ("sum", "max", "sum_bwd"):
        out["torch_over_hip_" + k] = round(out["torch_%s_us" % k] / out["hip_%s_us" % k], 2)
    # bytes the result needs: every node row once and every graph row once (+ the arg of the max)
    stream = (n + G) * F * 2
    out["hip_sum_TBps"] = round(stream / out["hip_sum_us"] / 1e6, 3)
    out["hip_max_TBps"] = round((stream + G * F * 4) / out["hip_max_us"] / 1e6, 3)
    out["hip_sum_bwd_TBps"] = round(stream / out["hip_sum_bwd_us"] / 1e6, 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="molecular,large")
    ap.add_argument("--chunks", default="", help="comma-separated chunk sizes (default: ops.READOUT_CHUNK)")
    ap.add_argument("--F", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_readout: no GPU; timings are taken on the device only")
    chunks = [int(c) for c in a.chunks.split(",") if c] or [None]
    for shape in a.shapes.split(","):
        for k, chunk in enumerate(chunks):
            if k and int(graph_sizes(shape).max()) <= min(chunks):
                continue                                 # a single launch whatever the chunk
            bench_shape(shape, chunk, a)


if __name__ == "__main__":
    main()
