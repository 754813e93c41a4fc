"""Edge-feature aggregate micro-benchmark: ``ops.espmm`` (add + relu, mul), ``ops.egrad``
(dE alone, dE + dval), the transposed ``dx`` pass (the sum of the dE rows over the transposed
CSR), ``ops.wspmm`` with unit values (the same gather without an edge row) and the PyTorch
composition ``index_add_(relu(X[col] + E))`` on the same tensors.  Default: the ogbn-arxiv
shape, F = 128, bf16.

The kernels alternate inside every round (so drift of the machine hits them alike); a round
times ``--inner`` back-to-back launches of each between device events; the figure is the
median over ``--rounds`` rounds, with the quartiles as the spread.  Prints one JSON line.

    python tools/bench_espmm.py [--dataset ogbn-arxiv] [--F 128] [--rounds 50] [--inner 20]
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
    from cgnn_amd.gnn.sage import transpose_csr
    dev = torch.device("cuda", 0)
    g = synthetic(a.dataset, seed=0, device=dev, scale=a.scale)
    n, nnz, F = g.n, g.nnz, a.F
    ld = -(-F // 8) * 8
    gen = torch.Generator(device=dev).manual_seed(0)

    def rand(rows):
        t = torch.zeros(rows, ld, device=dev)
        t[:, :F] = torch.randn(rows, F, device=dev, generator=gen)
        return t.to(torch.bfloat16)

    X, E, G = rand(n), rand(nnz), rand(n)
    val = torch.ones(nnz, device=dev)
    rp_t, col_t, eperm = transpose_csr(g.rowptr, g.col, n, with_perm=True)
    rows = ops._row_ids(g.rowptr)
    colj = g.col.long()
    Y0, Y1, Y2, DX = (torch.empty(n, ld, device=dev, dtype=torch.bfloat16) for _ in range(4))
    DE = torch.empty(nnz, ld, device=dev, dtype=torch.bfloat16)
    DV = torch.empty(nnz, device=dev)
    Yc = torch.empty(n, ld, device=dev, dtype=torch.float32)

    def composition():
        Yc.zero_()
        Yc.index_add_(0, rows, torch.relu(X[colj] + E).float())

    runs = {
        "wspmm": lambda: ops.wspmm(g.rowptr, g.col, val, X, F, out=Y0),
        "espmm_add_relu": lambda: ops.espmm(g.rowptr, g.col, X, E, F, relu=True, out=Y1),
        "espmm_mul": lambda: ops.espmm(g.rowptr, g.col, X, E, F, op="mul", out=Y2),
        "egrad_dE": lambda: ops.egrad(g.rowptr, g.col, G, X, E, F, relu=True, dE=DE),
        "egrad_dE_dval": lambda: ops.egrad(g.rowptr, g.col, G, X, E, F, relu=True, dE=DE, dval=DV),
        "dx_pass": lambda: ops.espmm(rp_t, col_t, None, DE, F, eperm=eperm, out=DX),
        "torch_composition": composition,
    }
    for _ in range(a.warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    # the kernel and the composition sum the same terms (the composition rounds x + e to bf16
    # first and adds in any order): a bf16-sized difference
    diff = float((Y1.float() - Yc).abs().max())
    scale = float(Yc.abs().max())
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
    e_bytes = nnz * F * 2                                               # the streamed bytes of E
    out["E_bytes"] = e_bytes
    for k in ("espmm_add_relu", "espmm_mul", "egrad_dE", "egrad_dE_dval", "dx_pass"):
        out[k + "_over_wspmm"] = round(out[k + "_us"] / out["wspmm_us"], 3)
        out[k + "_E_TBps"] = round(e_bytes / out[k + "_us"] / 1e6, 3)
    out["torch_composition_over_espmm_add_relu"] = round(out["torch_composition_us"] / out["espmm_add_relu_us"], 2)
    out["max_abs_diff_espmm_composition"] = diff
    out["max_abs_output"] = scale
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
