"""The periodic geometry kernels on the GPU (gnn_geometry.hip: radius_pbc_kernel,
pair_d2_pbc_kernel, pair_d2_pbc_bwd_kernel) against numpy fp64 references computed here from
the contract -- never through the CPU branches of ``ops`` -- and a periodic SchNet end to end
against an fp64 evaluation of the same parameters.

Exactness.  Positions and cell entries are multiples of 1/4 of magnitude <= 8, image shifts
integers of magnitude <= 3.  An offset is then a multiple of 1/4 below 3 * 3 * 8 = 72 with
every partial sum of its fmas one too, an image ``p_j + off`` a multiple of 1/4 below 80, a
difference one below 88 and a squared distance a multiple of 1/16 below 3 * 88^2 < 2^15: 19
significant bits at most, exact in fp32 whatever the contraction.  Edge sets, order, shifts,
``d2`` and (with integer ``g``) every partial sum of the gradient are compared with
``torch.equal``; ``ref_pbc`` asserts the exactness of what it computes, and
test_gnn_pbc_cpu.py that of the offsets and images.
"""
import itertools

import numpy as np
import pytest
import torch

import test_gnn_geometry_gpu as gg
from cgnn_amd.gnn import ops
from cgnn_amd.gnn.geometry import image_ranges, pair_distance, radius_graph, wrap_positions
from cgnn_amd.gnn.readout import GraphBatch
from cgnn_amd.gnn.schnet import SchNet
from cgnn_amd.utils.hipgraph import StepGraph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -7               # sentinel of rows / tails a kernel must not write
BIG = 1.0e4             # fills the padding columns of pos: must never reach a result
JUNK = 7.75             # fills the cell entries outside the leading D x D block: never read
R = 1.25                # r * r = 1.5625 exactly; the offset (0.75, 1, 0) sits on the boundary
LANES = (8, 16, 32, 64)
U = 2.0 ** -24          # fp32 unit roundoff
NAN, INF = float("nan"), float("inf")

# empty graphs first, in the middle and last-but-one; the one-atom graph sees only its own images
SIZES = [0, 0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 0, 129]
NIMG = [(1, 1, 1), (0, 0, 0), (3, 3, 3), (3, 3, 3), (2, 1, 0), (0, 1, 1), (1, 1, 1), (1, 0, 0), (0, 0, 0),
        (0, 1, 1), (1, 1, 1), (3, 3, 3), (2, 1, 0)]
assert len(NIMG) == len(SIZES) and set(NIMG) == {(0, 0, 0), (1, 0, 0), (0, 1, 1), (1, 1, 1), (2, 1, 0), (3, 3, 3)}


def gptr_of(sizes):
    return gg.gptr_of(sizes)


def grid_cells(G, seed, nimg=None):
    """fp32 ``[G, 3, 3]`` on the 1/4 grid, |entry| <= 8: orthorhombic for even g, triclinic
    (lower triangular, sheared) for odd g.  A lattice vector is 2 to 4 long, but 1 to 1.5 along
    an axis with ``nimg`` 2 and 0.5 to 1 along one with 3, so that the far images hold edges."""
    rng = np.random.default_rng(seed)
    cells = np.zeros((G, 3, 3), dtype=np.float32)
    for g in range(G):
        for a in range(3):
            k = nimg[g][a] if nimg is not None else 1
            lo, hi = ((8, 17), (8, 17), (4, 7), (2, 5))[k]
            cells[g, a, a] = rng.integers(lo, hi) / 4
        if g % 2:
            for a, c in ((1, 0), (2, 0), (2, 1)):
                cells[g, a, c] = rng.integers(-4, 5) / 4
    assert np.all(cells * 4 == np.round(cells * 4)) and np.abs(cells).max() <= 8
    return cells


def cell_table(cells, D):
    """``[G, 9]`` as the kernels take it: the leading D x D block, JUNK elsewhere."""
    t = np.full(cells.shape, JUNK, dtype=np.float32)
    t[:, :D, :D] = cells[:, :D, :D]
    return t.reshape(-1, 9)


def grid_inputs(sizes, nimg, D, ldp, seed, special=True):
    """``(pos, cells)``: fp32 positions ``[n, ldp]`` on the 1/4 grid in [-2, 2] (padding columns
    BIG) and the cells of ``grid_cells``.  Planted in every graph of at least 8 points: a pair
    that is on the boundary only through an image of the first lattice vector (where that axis
    has images; directly on the boundary otherwise) and a coincident pair; with ``special`` one
    NaN and one inf coordinate in the graph of 129 points."""
    rng = np.random.default_rng(seed)
    cells = grid_cells(len(sizes), seed + 1, nimg)
    n = sum(sizes)
    pos = np.full((n, ldp), BIG, dtype=np.float32)
    off = 0
    for g, s in enumerate(sizes):
        p = rng.integers(-8, 9, size=(s, D)).astype(np.float32) / 4
        if s >= 8:
            step = np.array([0.75, 1.0, 0.0][:D] if D > 1 else [1.25], dtype=np.float32)
            # seen from p[0], source 1 is on the boundary in its image (-1, 0, 0); seen from
            # p[1], source 0 in its image (+1, 0, 0)
            p[1] = p[0] + step + (cells[g, 0, :D] if nimg[g][0] else 0)
            p[3] = p[2]                             # coincident
        if special and s == 129:
            p[50, 0] = NAN
            p[60, D - 1] = INF
        pos[off:off + s, :D] = p
        off += s
    finite = pos[:, :D][np.isfinite(pos[:, :D])]
    assert np.all(finite * 4 == np.round(finite * 4)) and np.abs(finite).max() <= 8
    return pos, cells


def image_box(ni):
    """int64 ``[M, D]``: the images in lexicographic order, the last axis fastest."""
    return np.array(list(itertools.product(*[range(-k, k + 1) for k in ni])), dtype=np.int64).reshape(-1, len(ni))


def pack(S):
    w = np.zeros(S.shape[0], dtype=np.int64)
    for a in range(S.shape[1]):
        w |= (S[:, a] & 0xFF) << (8 * a)
    return w


def ref_pbc(pos, D, r, sizes, cells, nimg, loop, check_exact=True):
    """(rowptr, col, shift, d2) by brute force over the image box per graph in fp64, in
    ascending (j, image)."""
    r2 = float(np.float32(r) * np.float32(r))
    rowptr, col, sh, d2 = [0], [], [], []
    off = 0
    with np.errstate(invalid="ignore"):
        for g, s in enumerate(sizes):
            p = pos[off:off + s, :D].astype(np.float64)
            S = image_box([min(max(k, 0), ops.PBC_NIMG_MAX) for k in nimg[g][:D]])
            home = int(np.nonzero((S == 0).all(1))[0][0])
            q = p[:, None, :] + (S.astype(np.float64) @ cells[g, :D, :D].astype(np.float64))[None, :, :]   # [j, m, D]
            packed = pack(S)
            for i in range(s):
                d = ((p[i] - q) ** 2).sum(2)        # [j, m]
                if check_exact:                     # every candidate's d2 is exact in fp32
                    fin = d[np.isfinite(d)]
                    assert fin.size == 0 or (fin.max() < 2 ** 15 and np.all(fin * 16 == np.round(fin * 16)))
                keep = d <= r2                      # False for NaN
                if not loop:
                    keep[i, home] = False
                js, ms = np.nonzero(keep)           # row-major: ascending (j, m)
                col.append(js + off)
                sh.append(packed[ms])
                d2.append(d[js, ms])
                rowptr.append(rowptr[-1] + js.size)
            off += s
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0)
    return (torch.tensor(rowptr, dtype=torch.int32), torch.tensor(cat(col), dtype=torch.int32),
            torch.tensor(cat(sh), dtype=torch.int32), torch.tensor(cat(d2), dtype=torch.float64).float())


def device_batch(sizes):
    gp = torch.tensor(gptr_of(sizes), dtype=torch.int32, device=DEV)
    seg = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes)).to(DEV)
    return gp, seg


def run_search(pos, D, r, sizes, cells, nimg, loop, lanes=None, tail=5):
    """(deg, rowptr, col, shift, d2) from the two passes with sentinel rows and tails, checked."""
    n = pos.shape[0]
    gp, seg = device_batch(sizes)
    p = torch.tensor(pos, device=DEV)
    ct = torch.tensor(cell_table(cells, D), device=DEV)
    ni = torch.tensor(nimg, dtype=torch.int32, device=DEV).reshape(-1, 3)
    deg = torch.full((n + tail,), SENT, dtype=torch.int32, device=DEV)
    ops.radius_pbc_count(p, D, r, gp, seg, ct, ni, loop=loop, lanes=lanes, max_images=343, out=deg)
    assert bool((deg[n:] == SENT).all()), "count wrote past its rows"
    rp = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    rp[1:] = torch.cumsum(deg[:n], 0, dtype=torch.int64)
    nnz = int(rp[-1])
    col = torch.full((nnz + tail,), SENT, dtype=torch.int32, device=DEV)
    sh = torch.full((nnz + tail,), SENT, dtype=torch.int32, device=DEV)
    d2 = torch.full((nnz + tail,), float(SENT), dtype=torch.float32, device=DEV)
    ops.radius_pbc_fill(p, D, r, gp, seg, ct, ni, rp.to(torch.int32), loop=loop, lanes=lanes, max_images=343,
                        out=col, shift=sh, d2=d2)
    assert bool((col[nnz:] == SENT).all()) and bool((d2[nnz:] == SENT).all()) and bool((sh[nnz:] == SENT).all()), \
        "fill wrote past nnz"
    return deg[:n].cpu(), rp.to(torch.int32).cpu(), col[:nnz].cpu(), sh[:nnz].cpu(), d2[:nnz].cpu()


_REF = {}


def reference(D, loop):
    """The shared inputs and reference of (D, loop): positions with ldp = 4 (the first D columns
    are those of every ldp), cells, and (rowptr, col, shift, d2)."""
    if (D, loop) not in _REF:
        pos, cells = grid_inputs(SIZES, NIMG, D, 4, seed=300 + D)
        _REF[(D, loop)] = (pos, cells) + ref_pbc(pos, D, R, SIZES, cells, NIMG, loop)
    return _REF[(D, loop)]


def with_ldp(pos, D, ldp):
    return np.ascontiguousarray(pos[:, :D]) if ldp == D else pos


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("D,ldp", [(1, 1), (1, 4), (2, 2), (2, 4), (3, 3), (3, 4)])
def test_periodic_radius_graph_exact_edge_sets(D, ldp, loop):
    pos, cells, rowptr, col, shift, d2 = reference(D, loop)
    on = d2 == np.float32(R) * np.float32(R)
    assert bool((on & (shift != 0)).any()), "no pair on the boundary through an image"
    assert bool(((d2 == 0) & (shift == 0)).any()), "no coincident pair"
    deg, rp, c, sh, dd = run_search(with_ldp(pos, D, ldp), D, R, SIZES, cells, NIMG, loop)
    assert torch.equal(rp, rowptr)
    assert torch.equal(deg, rowptr[1:] - rowptr[:-1])
    assert torch.equal(c, col)
    assert torch.equal(sh, shift)
    assert torch.equal(dd, d2)
    gp = gptr_of(SIZES)
    # the one-atom graph: its own images only, never its home image unless loop
    one = int(gp[SIZES.index(1)])
    assert int(rp[one + 1] - rp[one]) >= 4 and bool((c[rp[one]:rp[one + 1]] == one).all())
    assert int((sh[rp[one]:rp[one + 1]] == 0).sum()) == int(loop)
    # the NaN point has no edge at all; the inf point none either (inf - inf is NaN)
    off = int(gp[SIZES.index(129)])
    assert int(deg[off + 50]) == 0 and int(deg[off + 60]) == 0


@pytest.mark.parametrize("lanes", LANES)
def test_every_compiled_lanes_value_gives_the_same_csr(lanes):
    pos, cells, rowptr, col, shift, d2 = reference(3, False)
    _, rp, c, sh, dd = run_search(pos, 3, R, SIZES, cells, NIMG, False, lanes=lanes)
    assert torch.equal(rp, rowptr) and torch.equal(c, col) and torch.equal(sh, shift) and torch.equal(dd, d2)


def test_two_runs_give_the_same_csr():
    pos, cells, rowptr, col, shift, d2 = reference(3, False)
    a = run_search(pos, 3, R, SIZES, cells, NIMG, False)
    b = run_search(pos, 3, R, SIZES, cells, NIMG, False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_the_api_returns_the_reference_of_its_own_image_ranges():
    pos, cells, _, _, _, _ = reference(3, False)
    pbc = torch.tensor([[True, g % 3 != 0, g % 2 == 0] for g in range(len(SIZES))])
    nimg = image_ranges(torch.tensor(cells), pbc, R)
    assert 2 <= int(nimg.max()) <= ops.PBC_NIMG_MAX and int(nimg.min()) == 0
    rowptr, col, shift, d2 = ref_pbc(pos, 3, R, SIZES, cells, nimg.tolist(), False)
    p = torch.tensor(pos[:, :3], device=DEV)
    a = radius_graph(p, R, torch.tensor(gptr_of(SIZES), device=DEV), cell=torch.tensor(cells, device=DEV), pbc=pbc)
    b = radius_graph(p, R, GraphBatch(torch.tensor(gptr_of(SIZES))), cell=torch.tensor(cells), pbc=pbc)
    for g in (a, b):
        assert g.rowptr.device.type == "cuda" and g.shift.device.type == "cuda" and g.cell.device.type == "cuda"
        assert torch.equal(g.rowptr.cpu(), rowptr) and torch.equal(g.col.cpu(), col)
        assert torch.equal(g.shift.cpu(), shift) and torch.equal(g.d2.cpu(), d2)
        assert torch.equal(g.eperm.cpu(), torch.arange(col.numel()))
        assert g.cell.shape == (len(SIZES), 9) and torch.equal(g.cell.cpu().view(-1, 3, 3), torch.tensor(cells))
        assert torch.equal(ops.unpack_shift(shift, 3), g.shifts().cpu())
    back = a.to("cpu")
    assert torch.equal(back.shift, shift) and back.cell.device.type == "cpu"


def test_a_graph_keeps_its_rows_wherever_it_stands():
    sizes = [65, 9, 2, 33]
    nimg = [(1, 1, 1), (2, 1, 0), (3, 3, 3), (0, 1, 1)]
    pos, cells = grid_inputs(sizes, nimg, 3, 3, seed=7, special=False)
    gp = gptr_of(sizes)
    _, rp, col, sh, d2 = run_search(pos, 3, R, sizes, cells, nimg, False)
    perm = [2, 0, 3, 1]
    pos2 = np.concatenate([pos[gp[k]:gp[k + 1]] for k in perm])
    sizes2 = [sizes[k] for k in perm]
    gp2 = gptr_of(sizes2)
    _, rp2, col2, sh2, d22 = run_search(pos2, 3, R, sizes2, cells[perm], [nimg[k] for k in perm], False)
    for new, old in enumerate(perm):
        a0, a1 = int(rp[gp[old]]), int(rp[gp[old + 1]])
        b0, b1 = int(rp2[gp2[new]]), int(rp2[gp2[new + 1]])
        assert a1 - a0 == b1 - b0 and a1 > a0
        assert torch.equal(rp[gp[old]:gp[old + 1] + 1] - a0, rp2[gp2[new]:gp2[new + 1] + 1] - b0)
        assert torch.equal(col[a0:a1] - int(gp[old]), col2[b0:b1] - int(gp2[new]))
        assert torch.equal(sh[a0:a1], sh2[b0:b1])
        assert torch.equal(d2[a0:a1].view(torch.int32), d22[b0:b1].view(torch.int32))


@pytest.mark.parametrize("D,ldp", [(1, 4), (2, 2), (3, 3), (3, 4)])
def test_no_images_is_the_radius_search_bit_for_bit(D, ldp):
    pos, cells, _, _, _, _ = reference(D, False)
    pos = with_ldp(pos, D, ldp)
    zero = [(0, 0, 0)] * len(SIZES)
    for loop in (False, True):
        deg, rp, col, sh, d2 = run_search(pos, D, R, SIZES, cells, zero, loop)
        gp, seg = device_batch(SIZES)
        p = torch.tensor(pos, device=DEV)
        want = ops.radius_count(p, D, R, gp, seg, loop=loop)
        wcol, wd2 = ops.radius_fill(p, D, R, gp, seg, rp.to(DEV), loop=loop, with_d2=True)
        assert torch.equal(deg, want.cpu()) and torch.equal(col, wcol.cpu())
        assert torch.equal(d2.view(torch.int32), wd2.cpu().view(torch.int32))
        assert col.numel() > 100 and bool((sh == 0).all())


# ---------------------------------------------------------------- pair_d2_pbc

@pytest.mark.parametrize("D,ldp", [(1, 4), (2, 2), (3, 3), (3, 4)])
def test_pair_d2_pbc_reproduces_the_fill_pass_bit_for_bit(D, ldp):
    pos, cells, rowptr, col, shift, d2 = reference(D, False)
    p = torch.tensor(with_ldp(pos, D, ldp), device=DEV)
    ct = torch.tensor(cell_table(cells, D), device=DEV)
    _, seg = device_batch(SIZES)
    for lanes in (None,) + LANES:
        out = torch.full((col.numel() + 3,), float(SENT), device=DEV)
        ops.pair_d2_pbc(rowptr.to(DEV), col.to(DEV), shift.to(DEV), p, D, ct, seg, out=out, lanes=lanes,
                        nnz=col.numel())
        # NaN-free: the NaN / inf points have no edges
        assert torch.equal(out[:col.numel()].cpu().view(torch.int32), d2.view(torch.int32))
        assert bool((out[col.numel():] == SENT).all())


def shifted_multigraph(seed=3):
    """``(g, pos, cells, shifts)``: gg.multigraph(), a directed multigraph of three components
    (repeated edges, self loops), with an arbitrary int8 image per edge and cells of entries
    |c| <= 1 on the 1/4 grid: |off| <= 3 * 128, a difference below 400, d2 a multiple of 1/16
    below 3 * 400^2 < 2^19 -- 23 bits, exact in fp32."""
    g = gg.multigraph(seed)
    rng = np.random.default_rng(seed + 40)
    pos = gg.grid_positions([g.n], 3, 4, seed=11, special=False)
    cells = (rng.integers(-4, 5, (g.n_graphs, 3, 3)) / 4).astype(np.float32)
    shifts = rng.integers(-128, 128, (g.col.numel(), 3))
    shifts[:3] = [[-128, 127, 0], [127, -128, -1], [0, 0, 0]]
    return g, pos, cells, shifts


def test_pair_d2_pbc_on_a_directed_multigraph_with_arbitrary_shifts_equals_fp64():
    g, pos, cells, shifts = shifted_multigraph()
    rows = np.repeat(np.arange(g.n), np.diff(g.rowptr.numpy()))
    gid = g.batch.numpy()[rows]
    off = np.einsum("ea,eac->ec", shifts.astype(np.float64), cells[gid].astype(np.float64))
    diff = pos[rows, :3].astype(np.float64) - (pos[g.col.numpy(), :3].astype(np.float64) + off)
    d2 = (diff ** 2).sum(1)
    assert d2.max() < 2 ** 19 and np.all(d2 * 16 == np.round(d2 * 16)) and d2.max() > 1e4
    gd = g.to(DEV)
    got = ops.pair_d2_pbc(gd.rowptr, gd.col, torch.tensor(pack(shifts), dtype=torch.int32, device=DEV),
                          torch.tensor(pos, device=DEV), 3, torch.tensor(cells.reshape(-1, 9), device=DEV), gd.batch)
    assert torch.equal(got.cpu(), torch.tensor(d2).float())


# ---------------------------------------------------------------- pair_d2_pbc_bwd

def ref_bwd_pbc(pos, D, rowptr, col, shifts, cells, gid, g):
    """fp64 dpos from the definition; gid: the graph of each node."""
    n = pos.shape[0]
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    p = pos[:, :D].astype(np.float64)
    off = np.einsum("ea,eac->ec", shifts[:, :D].astype(np.float64), cells[gid[rows]][:, :D, :D].astype(np.float64))
    w = g[:, None].astype(np.float64) * (p[rows] - (p[col] + off))
    out = np.zeros((n, D))
    np.add.at(out, rows, w)
    np.add.at(out, col, -w)
    return 2 * out


def two_hub_graphs(n):
    """Two of gg.hub_graph side by side (different seeds), so that two cells are in play."""
    parts = []
    for seed in (1, 2):
        h = gg.hub_graph(n, seed=seed)
        parts.append((n, h.col.numpy(), np.repeat(np.arange(n), np.diff(h.rowptr.numpy()))))
    return GraphBatch.from_graphs(parts)


@pytest.mark.parametrize("D,ldp", [(1, 1), (2, 4), (3, 3), (3, 4)])
def test_pair_d2_pbc_bwd_exact(D, ldp):
    n = 160
    g = two_hub_graphs(n)
    deg_in = np.diff(g.rowptr.numpy())
    deg_out = np.bincount(g.col.numpy(), minlength=2 * n)
    assert deg_in.min() == 0 and deg_in.max() >= 300 and deg_out.max() >= 400 and (deg_in != deg_out).any()
    pos = gg.grid_positions([2 * n], D, ldp, seed=21 + D, special=False)
    cells = grid_cells(2, seed=5)
    rng = np.random.default_rng(9)
    gv = rng.integers(-2, 3, g.col.numel()).astype(np.float32)
    shifts = rng.integers(-3, 4, (g.col.numel(), 3))
    shifts[:, D:] = 0
    want = ref_bwd_pbc(pos, D, g.rowptr.numpy(), g.col.numpy(), shifts, cells, g.batch.numpy(), gv)
    # |g| <= 2, |difference| <= 16 + 72, multiples of 1/4: any partial sum of the at most
    # deg_in + deg_out <= 1024 terms is a multiple of 1/4 below 176 * 1024 < 2^18, exact in fp32
    assert (deg_in + deg_out).max() <= 1024 and np.abs(want).max() < 2 ** 19
    assert np.abs(want - gg.ref_bwd(pos, D, g.rowptr.numpy(), g.col.numpy(), gv)).max() > 1      # the shifts matter
    gd = g.to(DEV)
    rp_t, col_t, eperm_t = gd.transposed_perm()
    p = torch.tensor(pos, device=DEV)
    sh = torch.tensor(pack(shifts), dtype=torch.int32, device=DEV)
    ct = torch.tensor(cell_table(cells, D), device=DEV)
    for lanes in (None,) + LANES:
        out = torch.full((2 * n, ldp), float(SENT), device=DEV)
        ops.pair_d2_pbc_bwd(gd.rowptr, gd.col, sh, rp_t, col_t, eperm_t, p, torch.tensor(gv, device=DEV), D, ct,
                            gd.batch, out=out, lanes=lanes)
        assert torch.equal(out[:, :D].cpu(), torch.tensor(want).float()), "lanes %s" % lanes
        assert bool((out[:, D:] == 0).all()), "padding columns"
    iso = np.nonzero((deg_in == 0) & (deg_out == 0))[0]
    assert iso.size >= 5                                      # a node without edges gets 0
    assert bool((out[torch.tensor(iso, device=DEV)] == 0).all())


# ---------------------------------------------------------------- autograd

@pytest.mark.parametrize("squared", [True, False])
def test_pair_distance_autograd_against_fp64(squared):
    """The bounds of test_gnn_geometry_gpu.py::test_pair_distance_autograd_against_fp64, whose
    derivation counts the roundings from the difference ``p_i - q`` on: forward 6 u t
    (squared) / 4 u d, gradient 8 deg u S per node and coordinate.  They carry over when the
    image ``q = p_j + off`` itself is exact, so the inputs make it so: positions are multiples
    of 2^-16 below 8 and cell entries multiples of 1/4 below 4 with |s| <= 2, hence every
    offset and image is a multiple of 2^-16 below 32 -- 21 bits.  (For general inputs the image
    adds an absolute error of about u |q| to each coordinate, which no bound relative to the
    distance covers; that is a property of fp32 positions, not of the kernel.)  Largest
    observed fraction of the bounds on an MI355X: forward 0.42 (squared), 0.45 (distance);
    gradient 0.002 (squared), 0.003 (distance)."""
    torch.manual_seed(4)
    sizes = [30, 1, 64, 17]
    n, G = sum(sizes), len(sizes)
    cells = torch.tensor(grid_cells(G, seed=17))
    pos = torch.round(torch.randn(n, 3) * 1.2 * 2 ** 16) / 2 ** 16
    batch = GraphBatch(torch.tensor(gptr_of(sizes)))
    pos = wrap_positions(pos.double(), cells, True, batch).float()
    assert bool((pos.double() * 2 ** 16 == torch.round(pos.double() * 2 ** 16)).all()) and float(pos.abs().max()) < 8
    pos = pos.to(DEV)
    g = radius_graph(pos, 1.7, batch, cell=cells)
    nnz = g.col.numel()
    assert nnz > 200 and int(g.shifts().abs().max()) >= 1 and int((g.shift != 0).sum()) > 50
    wgt = torch.randn(nnz, device=DEV)
    p32 = pos.clone().requires_grad_(True)
    out = pair_distance(p32, g, squared=squared)
    (out * wgt).sum().backward()
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), (g.rowptr[1:] - g.rowptr[:-1]).long())
    cols = g.col.long()
    off = torch.einsum("ea,eac->ec", g.shifts().double(), cells.double().to(DEV)[g.batch.long()[rows]])
    p64 = pos.double().requires_grad_(True)
    t = ((p64[rows] - (p64[cols] + off)) ** 2).sum(1)
    ref = t if squared else torch.sqrt(t)
    (ref * wgt.double()).sum().backward()
    err = (out.detach().double() - ref.detach()).abs()
    bound = (6 if squared else 4) * U * ref.detach()
    print("forward: largest fraction of the bound %.3f" % float((err / bound).max()))
    assert bool((err <= bound).all())
    ge = wgt.double() if squared else wgt.double() / (2 * ref.detach())
    mag = ge.abs() * (p64.detach()[rows] - (p64.detach()[cols] + off)).abs().sum(1)
    s = torch.zeros(n, dtype=torch.float64, device=DEV).index_add_(0, rows, mag).index_add_(0, cols, mag)
    deg = torch.zeros(n, dtype=torch.float64, device=DEV).index_add_(0, rows, torch.ones_like(mag))
    deg = deg.index_add_(0, cols, torch.ones_like(mag))
    gbound = 8 * deg * U * 2 * s
    gerr = (p32.grad.double() - p64.grad).abs().max(1).values
    has = deg > 0
    print("gradient: largest fraction of the bound %.3f" % float((gerr[has] / gbound[has]).max()))
    assert bool((gerr <= gbound).all())
    assert bool((p32.grad[~has] == 0).all())


@pytest.mark.parametrize("squared", [True, False])
def test_pair_distance_autograd_on_generic_inputs_against_fp64(squared):
    """Generic fp32 positions and triclinic fp32 cells, where the image is rounded.  The
    reference is the fp64 evaluation of the same fp32 inputs; the bounds are those of the test
    above plus the image's own error, first order in u with 1 % for the higher orders.
    Image.  ``off[c]`` is a product and up to two fmas: three roundings, each relative to a
    partial sum of magnitude at most ``A[c] = sum_a |s_a| |C[a][c]|``; ``q[c] = fl(p_j[c] +
    off[c])`` adds one relative to ``|q[c]| <= |p_j[c]| + A[c]``.  So ``|dq[c]| <= eps[c] =
    1.01 u (|p_j[c]| + 4 A[c])``, and the same for ``p_k - off`` of an out-edge.
    Forward.  The difference inherits ``eps``; the square of a coordinate moves by ``2 |diff[c]|
    eps[c]``: ``|d2 - t| <= 6 u t + 2.02 sum_c |diff[c]| eps[c]``; for the distance, an absolute
    error E of d2 is E / (2 d) in d and ``sum_c |diff[c]| eps[c] <= d |eps|_2``:
    ``|d - sqrt t| <= 4 u d + 1.01 |eps|_2``.
    Gradient.  A term ``g_e (p_i - q)[c]`` moves by ``|g_e| eps[c]``; for the distance
    ``g_e = gd / (2 d)`` also inherits the relative error ``|eps|_2 / d`` of d, which times
    ``|diff[c]| <= d`` is ``|g_e| |eps|_2``.  Per node and coordinate, with the final factor 2:
    ``8 deg u S + 2.02 sum_e |g_e| (eps_e[c] + |eps_e|_2)``, S as above.  Largest observed
    fraction of the bounds on an MI355X: forward 0.53 (squared), 0.44 (distance); gradient
    0.004 (squared), 0.005 (distance)."""
    torch.manual_seed(14)
    rng = np.random.default_rng(14)
    sizes = [30, 1, 64, 17]
    n, G = sum(sizes), len(sizes)
    cells = torch.tensor(rng.normal(size=(G, 3, 3)) * 0.35 + np.eye(3) * 3.0, dtype=torch.float32)
    batch = GraphBatch(torch.tensor(gptr_of(sizes)))
    # one cell's worth of positions, moved away from the origin so that u |q| is several times
    # the rounding of a difference (neighbours stay neighbours; the list need not be complete)
    pos = (wrap_positions(torch.randn(n, 3) * 4, cells, True, batch) + 20.0).to(DEV)
    g = radius_graph(pos, 1.9, batch, cell=cells)
    nnz = g.col.numel()
    assert nnz > 200 and int((g.shift != 0).sum()) > 50
    wgt = torch.randn(nnz, device=DEV)
    p32 = pos.clone().requires_grad_(True)
    out = pair_distance(p32, g, squared=squared)
    (out * wgt).sum().backward()
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), (g.rowptr[1:] - g.rowptr[:-1]).long())
    cols = g.col.long()
    Ce = cells.double().to(DEV)[g.batch.long()[rows]]                       # [nnz, 3, 3]
    S = g.shifts().double()
    off = torch.einsum("ea,eac->ec", S, Ce)
    A = torch.einsum("ea,eac->ec", S.abs(), Ce.abs())
    p64 = pos.double().requires_grad_(True)
    diff = p64[rows] - (p64[cols] + off)
    t = (diff ** 2).sum(1)
    ref = t if squared else torch.sqrt(t)
    (ref * wgt.double()).sum().backward()
    diff, d = diff.detach(), torch.sqrt(t.detach())
    eps_in = 1.01 * U * (pos.double()[cols].abs() + 4 * A)                  # the image q of an in-edge
    eps_out = 1.01 * U * (pos.double()[rows].abs() + 4 * A)                 # p_k - off of an out-edge
    err = (out.detach().double() - ref.detach()).abs()
    if squared:
        bound = 6 * U * t.detach() + 2.02 * (diff.abs() * eps_in).sum(1)
    else:
        bound = 4 * U * d + 1.01 * eps_in.norm(dim=1)
    print("generic forward: largest fraction of the bound %.3f" % float((err / bound).max()))
    assert bool((err <= bound).all())
    ge = (wgt.double() if squared else wgt.double() / (2 * d)).abs()
    mag = ge * diff.abs().sum(1)
    s = torch.zeros(n, dtype=torch.float64, device=DEV).index_add_(0, rows, mag).index_add_(0, cols, mag)
    deg = torch.zeros(n, dtype=torch.float64, device=DEV).index_add_(0, rows, torch.ones_like(mag))
    deg = deg.index_add_(0, cols, torch.ones_like(mag))
    extra = torch.zeros(n, 3, dtype=torch.float64, device=DEV)
    extra = extra.index_add_(0, rows, ge[:, None] * (eps_in + eps_in.norm(dim=1, keepdim=True)))
    extra = extra.index_add_(0, cols, ge[:, None] * (eps_out + eps_in.norm(dim=1, keepdim=True)))
    gbound = (8 * deg * U * 2 * s)[:, None] + 2.02 * extra
    gerr = (p32.grad.double() - p64.grad).abs()
    has = deg > 0
    print("generic gradient: largest fraction of the bound %.3f" % float((gerr[has] / gbound[has]).max()))
    assert bool((gerr <= gbound).all())
    assert float(pos.abs().min()) > 16 and bool((p32.grad[~has] == 0).all())


# ---------------------------------------------------------------- capture

def test_the_four_periodic_ops_replay_under_step_graph():
    sizes = [12, 40, 0, 2, 33]
    nimg = [(1, 1, 1), (1, 0, 0), (3, 3, 3), (3, 3, 3), (0, 1, 1)]
    n = sum(sizes)
    gp, seg = device_batch(sizes)
    ni = torch.tensor(nimg, dtype=torch.int32, device=DEV)
    cap = 40000
    p = torch.zeros(n, 4, device=DEV)
    ct = torch.zeros(len(sizes), 9, device=DEV)
    gv = torch.zeros(cap, device=DEV)
    deg = torch.zeros(n, dtype=torch.int32, device=DEV)
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    col = torch.zeros(cap, dtype=torch.int32, device=DEV)
    sh = torch.zeros(cap, dtype=torch.int32, device=DEV)
    d2 = torch.zeros(cap, device=DEV)
    d2b = torch.zeros(cap, device=DEV)
    dpos = torch.zeros(n, 4, device=DEV)
    # a fixed periodic graph for the distances and the gradient: its transposed CSR is built
    # outside the capture
    bpos, bcells = grid_inputs(sizes, nimg, 3, 3, 1, special=False)
    bond = radius_graph(torch.tensor(bpos, device=DEV), R, gp, cell=torch.tensor(bcells))
    assert int((bond.shift != 0).sum()) > 0
    rp_t, col_t, eperm_t = bond.transposed_perm()

    def inputs(seed):
        pos, cells = grid_inputs(sizes, nimg, 3, 4, seed, special=False)
        p.copy_(torch.tensor(pos))
        ct.copy_(torch.tensor(cell_table(cells, 3)))
        gv.copy_(torch.randint(-2, 3, (cap,), generator=torch.Generator().manual_seed(seed)).float())

    def step():
        ops.radius_pbc_count(p, 3, R, gp, seg, ct, ni, max_images=343, out=deg)
        rowptr[1:] = torch.cumsum(deg, 0, dtype=torch.int32)
        ops.radius_pbc_fill(p, 3, R, gp, seg, ct, ni, rowptr, max_images=343, out=col, shift=sh, d2=d2)
        ops.pair_d2_pbc(bond.rowptr, bond.col, bond.shift, p, 3, ct, seg, out=d2b)
        ops.pair_d2_pbc_bwd(bond.rowptr, bond.col, bond.shift, rp_t, col_t, eperm_t, p, gv, 3, ct, seg, out=dpos,
                            nnz=bond.col.numel())

    bufs = (deg, rowptr, col, sh, d2, d2b, dpos)
    eager = []
    for seed in (31, 33):
        inputs(seed)
        for b in bufs:
            b.fill_(SENT)
        rowptr[0] = 0
        step()
        torch.cuda.synchronize()
        assert 0 < int(rowptr[-1]) < cap
        eager.append([b.clone() for b in bufs])
    assert not torch.equal(eager[0][2], eager[1][2]) and not torch.equal(eager[0][3], eager[1][3])
    inputs(35)
    sg = StepGraph(step, warmup=1, device=torch.device(DEV))
    sg()                                                   # eager warm-up
    for k, seed in enumerate((31, 33)):
        inputs(seed)
        for b in bufs:
            b.fill_(SENT)
        rowptr[0] = 0
        sg()
        assert sg.graph is not None
        torch.cuda.synchronize()
        for b, e in zip(bufs, eager[k]):
            assert torch.equal(b, e), "replay %d" % k


# ---------------------------------------------------------------- empty inputs, API errors

def test_empty_inputs():
    cell = torch.eye(3) * 2
    e = radius_graph(torch.zeros(0, 3, device=DEV), 1.0, cell=cell)
    assert e.n == 0 and e.col.numel() == 0 and e.shift.numel() == 0 and e.rowptr.tolist() == [0]
    assert e.cell.shape == (1, 9) and e.shifts().shape == (0, 3)
    e = radius_graph(torch.zeros(0, 2, device=DEV), 1.0, torch.zeros(4, dtype=torch.int64), cell=torch.eye(2))
    assert e.n_graphs == 3 and e.col.numel() == 0 and e.rowptr.tolist() == [0] and e.cell.shape == (3, 9)
    # a cutoff below every distance: no edge, although every axis has images
    pos = torch.tensor([[0.0, 0, 0], [1, 1, 1], [0.5, 1.5, 0.25]], device=DEV)
    g = radius_graph(pos, 0.25, torch.tensor([0, 2, 3]), cell=cell)
    assert g.col.numel() == 0 and g.shift.numel() == 0 and g.d2.numel() == 0 and g.rowptr.tolist() == [0] * 4
    assert radius_graph(pos, 0.0, torch.tensor([0, 2, 3]), cell=cell, loop=True).col.tolist() == [0, 1, 2]
    p = pos.clone().requires_grad_(True)
    d = pair_distance(p, g)
    assert d.shape == (0,)
    d.sum().backward()
    assert bool((p.grad == 0).all())


def test_radius_graph_cell_error_paths():
    pos = torch.rand(6, 3, device=DEV)
    cell = torch.eye(3) * 2
    with pytest.raises(NotImplementedError):
        radius_graph(pos, 1.0, cell=cell, max_num_neighbors=4)
    with pytest.raises(ValueError, match="singular"):
        radius_graph(pos, 1.0, cell=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="singular"):
        radius_graph(pos, 1.0, cell=torch.tensor([[1.0, 0, 0], [2, 0, 0], [0, 0, 1]]), pbc=(False, False, True))
    with pytest.raises(ValueError, match=r"cutoff 1 .* 0\.1 high"):
        radius_graph(pos, 1.0, cell=torch.eye(3) * 0.1)
    with pytest.raises(ValueError, match="finite"):
        radius_graph(pos, 1.0, cell=torch.eye(3) * float("nan"))
    with pytest.raises(ValueError, match="cell must be"):
        radius_graph(pos, 1.0, cell=torch.eye(2))
    with pytest.raises(ValueError, match="cell must be"):
        radius_graph(pos, 1.0, torch.tensor([0, 3, 6]), cell=torch.eye(3).expand(3, 3, 3))
    with pytest.raises(ValueError, match="pbc must be"):
        radius_graph(pos, 1.0, cell=cell, pbc=(True, False))
    with pytest.raises(TypeError):
        radius_graph(pos, 1.0, cell=cell, pbc=(1, 0, 1))
    with pytest.raises(TypeError):
        radius_graph(pos, 1.0, cell=torch.eye(3, dtype=torch.int64))
    # a singular cell without a periodic axis is no error: the plain radius graph
    a = radius_graph(pos, 0.5, cell=torch.zeros(3, 3), pbc=False)
    b = radius_graph(pos, 0.5)
    assert torch.equal(a.col, b.col) and torch.equal(a.rowptr, b.rowptr) and bool((a.shift == 0).all())


# ---------------------------------------------------------------- SchNet end to end

def periodic_edges(pos, cells, pbcs, gp, rc, extra=2):
    """``(rows, cols, offsets, margin)`` in fp64: every (i, j, s) with ``|p_i - p_j - s C| <= rc``
    over a box ``extra`` images wider than ``image_ranges`` asks for, in ascending (i, j, s),
    and the smallest distance of a pair to the cutoff."""
    rows, cols, offs, margin = [], [], [], np.inf
    for g in range(len(gp) - 1):
        p = pos[gp[g]:gp[g + 1]]
        ni = image_ranges(torch.tensor(cells[g]), torch.tensor(pbcs[g]), rc)[0].tolist()
        S = image_box([k + extra if per else 0 for k, per in zip(ni, pbcs[g])])
        off = S.astype(np.float64) @ cells[g]
        d = np.sqrt(((p[:, None, None, :] - p[None, :, None, :] - off[None, None, :, :]) ** 2).sum(3))     # [i, j, m]
        margin = min(margin, np.abs(d - rc).min())
        keep = d <= rc
        home = int(np.nonzero((S == 0).all(1))[0][0])
        keep[np.arange(len(p)), np.arange(len(p)), home] = False
        i, j, m = np.nonzero(keep)
        assert np.abs(S[m]).max(initial=0) <= max(ni)        # the wider box finds nothing new
        rows.append(i + gp[g])
        cols.append(j + gp[g])
        offs.append(off[m])
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(offs), margin


def schnet_formula_pbc(model, z, pos, rows, cols, offs, gid, G, dtype):
    """gg.schnet_formula with the edge offsets: the model in plain indexing and index_add, in
    ``dtype``, on the CPU: (E [G], F [n, 3])."""
    ssp = gg.ssp
    P = {k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items()}
    p = pos.detach().cpu().to(dtype).requires_grad_(True)
    rc = model.cutoff
    d = torch.sqrt(((p[rows] - (p[cols] + offs.to(dtype))) ** 2).sum(1))
    mu = P["smearing.offset"]
    delta = rc / (mu.numel() - 1)
    e = torch.exp(-0.5 / delta ** 2 * (d[:, None] - mu[None, :]) ** 2)
    c = torch.where(d < rc, 0.5 * (torch.cos(d * (np.pi / rc)) + 1), torch.zeros_like(d))
    x = P["embedding"][z.cpu()]
    for t in range(len(model.interactions)):
        k = "interactions.%d." % t
        h = x @ P[k + "conv.lin1.weight"]
        w = ssp(e @ P[k + "conv.filter1.weight"] + P[k + "conv.filter1.bias"]) @ P[k + "conv.filter2.weight"] \
            + P[k + "conv.filter2.bias"]
        m = c[:, None] * h[cols] * w
        agg = torch.zeros_like(h).index_add(0, rows, m)
        v = agg @ P[k + "conv.lin2.weight"] + P[k + "conv.lin2.bias"]
        x = x + ssp(v) @ P[k + "dense.weight"] + P[k + "dense.bias"]
    y = ssp(x @ P["out1.weight"] + P["out1.bias"]) @ P["out2.weight"] + P["out2.bias"]
    E = torch.zeros(G, dtype=dtype).index_add(0, gid, y[:, 0])
    F, = torch.autograd.grad(E.sum(), p)
    return E.detach(), -F


def test_periodic_schnet_energy_and_forces_end_to_end():
    """A crystal cell of 8 atoms in a triclinic cell, periodic in all directions, and a slab of
    6 atoms periodic in two, cutoff 3.2 above the two shortest lattice vectors of the crystal
    (3.1 and 3.13; half the shortest cell height is about 1.5), so that an atom meets several
    images of the same neighbour and of itself.  Energy and forces
    of the HIP path against fp64 over the explicit (row, col, offset) list; allowed: 4x the
    error of a plain PyTorch fp32 evaluation of the same formula against that fp64, the margin
    of test_gnn_geometry_gpu.py::test_schnet_energy_and_forces_end_to_end for the same reason
    (both are fp32 evaluations that differ in summation order and fused contractions only).
    Translating all atoms by a lattice vector and wrapping them again leaves E unchanged within
    the same bound.  Observed on an MI355X (368 edges, 32 of them from an atom to its own
    image): energy error 2.6e-7, 0.43x that of the PyTorch fp32 evaluation (6.1e-7); force
    error 5.4e-7, 0.84x (6.4e-7); energy error after the translation 7.4e-7, 1.22x."""
    rng = np.random.default_rng(12)
    sizes = [8, 6]
    rc = 3.2
    n, G = sum(sizes), len(sizes)
    gp = gptr_of(sizes)
    cells = np.array([[[3.1, 0.0, 0.0], [0.9, 3.0, 0.0], [0.6, -0.8, 3.3]],
                      [[3.4, 0.0, 0.0], [-0.7, 3.2, 0.0], [0.0, 0.0, 9.0]]]).astype(np.float32).astype(np.float64)
    pbcs = [[True, True, True], [True, True, False]]
    batch = GraphBatch(torch.tensor(gp))
    ct, pt = torch.tensor(cells), torch.tensor(pbcs)
    heights = 1 / np.linalg.norm(np.linalg.inv(cells[0]), axis=0)
    assert rc > 0.5 * heights.min()
    # seeded fractional positions, redrawn until no pair sits within 1e-3 of the cutoff
    for _ in range(100):
        frac = rng.random((n, 3))
        frac[sizes[0]:, 2] = 0.4 + 0.2 * frac[sizes[0]:, 2]                       # the slab: 1.8 thick
        pos = np.concatenate([frac[gp[k]:gp[k + 1]] @ cells[k] for k in range(G)])
        pos = wrap_positions(torch.tensor(pos.astype(np.float32)), ct, pt, batch).double().numpy()
        rows, cols, offs, margin = periodic_edges(pos, cells, pbcs, gp, rc)
        if margin >= 1e-3:
            break
    assert margin >= 1e-3
    rows, cols, offs = torch.tensor(rows), torch.tensor(cols), torch.tensor(offs)
    pair_count = np.unique(np.stack([rows.numpy(), cols.numpy()]), axis=1, return_counts=True)[1]
    assert rows.numel() > 250 and pair_count.max() >= 2 and bool((rows == cols).any())
    z = torch.tensor(rng.integers(1, 10, n))
    gid = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes))
    model = SchNet(hidden=32, n_filters=32, n_interactions=2, n_gaussians=16, cutoff=rc,
                   generator=torch.Generator().manual_seed(8)).to(DEV)
    post = torch.tensor(pos, dtype=torch.float32)
    bd = batch.to(DEV)
    g = model.neighbors(post.to(DEV), bd, cell=ct, pbc=pt)
    grow = torch.repeat_interleave(torch.arange(n), (g.rowptr[1:] - g.rowptr[:-1]).long().cpu())
    assert torch.equal(grow, rows) and torch.equal(g.col.cpu().long(), cols)
    goff = torch.einsum("ea,eac->ec", g.shifts().cpu().double(), ct[gid[grow]])
    assert float((goff - offs).abs().max()) < 1e-12
    E, F = model.energy_and_forces(z.to(DEV), post.to(DEV), bd, cell=ct, pbc=pt)
    E64, F64 = schnet_formula_pbc(model, z, post, rows, cols, offs, gid, G, torch.float64)
    E32, F32 = schnet_formula_pbc(model, z, post, rows, cols, offs, gid, G, torch.float32)
    assert float(F64.abs().max()) > 1e-3 and float(E64.abs().max()) > 1e-3
    eE, rE = (E.cpu().double() - E64).abs().max(), (E32.double() - E64).abs().max()
    eF, rF = (F.cpu().double() - F64).abs().max(), (F32.double() - F64).abs().max()
    print("periodic SchNet: energy error %.3e (PyTorch fp32 %.3e, ratio %.2f), force error %.3e (PyTorch fp32 "
          "%.3e, ratio %.2f)" % (eE, rE, eE / rE, eF, rF, eF / rF))
    assert eE <= 4 * rE and eF <= 4 * rF
    # all atoms moved by a lattice vector of their cell, then wrapped again
    moved = post + torch.tensor(np.stack([cells[0][0] - cells[0][2], 2 * cells[1][1]]), dtype=torch.float32)[gid]
    back = wrap_positions(moved.to(DEV), ct, pt, bd)
    E2, _ = model.energy_and_forces(z.to(DEV), back, bd, cell=ct, pbc=pt)
    eT = (E2.cpu().double() - E64).abs().max()
    print("periodic SchNet: energy error after a lattice translation %.3e (ratio %.2f)" % (eT, eT / rE))
    assert eT <= 4 * rE
