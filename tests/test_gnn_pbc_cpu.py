"""The periodic geometry path without a GPU: the CPU branches of ``ops.radius_pbc_count`` /
``radius_pbc_fill`` / ``pair_d2_pbc`` / ``pair_d2_pbc_bwd`` against the numpy fp64 brute force
over the image box of test_gnn_pbc_gpu.py (edge sets, order, shifts, ``d2``), ``image_ranges``
against a brute force over a box two images wider, ``wrap_positions``, the symmetry of the
edges, ``nimg = 0`` against the non-periodic ops, the autograd of ``pair_distance`` in fp64, and
the exact-lattice property the GPU tests rest on.
"""
import numpy as np
import pytest
import torch

import test_gnn_pbc_gpu as pg
from cgnn_amd.gnn import ops
from cgnn_amd.gnn.geometry import image_ranges, pair_distance, radius_graph, wrap_positions
from cgnn_amd.gnn.readout import GraphBatch
from cgnn_amd.gnn.schnet import SchNet

SIZES, NIMG, R = pg.SIZES, pg.NIMG, pg.R


def batch_of(sizes):
    gp = torch.tensor(pg.gptr_of(sizes), dtype=torch.int32)
    seg = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes))
    return gp, seg


def cpu_search(pos, D, r, sizes, cells, nimg, loop):
    gp, seg = batch_of(sizes)
    p = torch.as_tensor(pos)
    ct = torch.tensor(pg.cell_table(cells, D))
    ni = torch.tensor(nimg, dtype=torch.int32).reshape(-1, 3)
    deg = ops.radius_pbc_count(p, D, r, gp, seg, ct, ni, loop=loop)
    rp = torch.zeros(p.shape[0] + 1, dtype=torch.int32)
    rp[1:] = torch.cumsum(deg, 0)
    col, sh, d2 = ops.radius_pbc_fill(p, D, r, gp, seg, ct, ni, rp, loop=loop, with_d2=True)
    return rp, col, sh, d2


# ---------------------------------------------------------------- the exact lattice of the GPU tests

@pytest.mark.parametrize("D", [1, 2, 3])
def test_the_gpu_inputs_are_exact_in_fp32(D):
    """Every offset -- each partial sum of its fmas -- every image and every difference of the
    inputs of test_gnn_pbc_gpu.py is representable in fp32, and so is every d2 (``ref_pbc``
    asserts that one candidate by candidate)."""
    pos, cells, rowptr, col, shift, d2 = pg.reference(D, False)
    assert np.abs(cells).max() <= 8 and np.all(cells * 4 == np.round(cells * 4))
    fits = lambda x: bool(np.all(x.astype(np.float32).astype(np.float64) == x))
    off0 = 0
    for g, s in enumerate(SIZES):
        p = pos[off0:off0 + s, :D].astype(np.float64)
        p = p[np.isfinite(p).all(1)]
        S = pg.image_box(NIMG[g][:D]).astype(np.float64)
        assert np.abs(S).max() <= 3
        C = cells[g, :D, :D].astype(np.float64)
        part = S[:, 0:1] * C[0]
        assert fits(part)
        for a in range(1, D):
            part = S[:, a:a + 1] * C[a] + part
            assert fits(part)
        q = p[:, None, :] + part[None, :, :]
        assert fits(q) and np.abs(q).max(initial=0) <= 80
        diff = p[:, None, None, :] - q[None, :, :, :]
        assert fits(diff) and fits(diff * diff) and fits((diff * diff).cumsum(-1))
        off0 += s
    assert float(d2.max()) <= np.float32(R) * np.float32(R)


# ---------------------------------------------------------------- CPU branches against the brute force

@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_cpu_branch_equals_the_brute_force(D, loop):
    pos, cells, rowptr, col, shift, d2 = pg.reference(D, loop)
    for ldp in (D, 4):
        rp, c, sh, dd = cpu_search(pg.with_ldp(pos, D, ldp), D, R, SIZES, cells, NIMG, loop)
        assert torch.equal(rp, rowptr) and torch.equal(c, col) and torch.equal(sh, shift) and torch.equal(dd, d2)
    assert col.numel() > 1000 and int((shift != 0).sum()) > 100
    assert torch.equal(ops.unpack_shift(shift, 3)[:, D:], torch.zeros(col.numel(), 3 - D, dtype=torch.int32))


def test_cpu_branch_in_fp64_on_random_triclinic_input():
    rng = np.random.default_rng(5)
    sizes = [5, 0, 12, 1]
    nimg = [(2, 1, 1), (0, 0, 0), (1, 2, 1), (3, 2, 1)]
    cells = rng.normal(size=(4, 3, 3)) * 0.4 + np.eye(3) * 2.0
    pos = rng.normal(size=(sum(sizes), 3))
    want = pg.ref_pbc(pos, 3, 1.9, sizes, cells, nimg, False, check_exact=False)
    gp, seg = batch_of(sizes)
    ct, ni = torch.tensor(cells.reshape(-1, 9)), torch.tensor(nimg, dtype=torch.int32)
    deg = ops.radius_pbc_count(torch.tensor(pos), 3, 1.9, gp, seg, ct, ni)
    rp = torch.zeros(sum(sizes) + 1, dtype=torch.int32)
    rp[1:] = torch.cumsum(deg, 0)
    col, sh, d2 = ops.radius_pbc_fill(torch.tensor(pos), 3, 1.9, gp, seg, ct, ni, rp, with_d2=True)
    assert d2.dtype == torch.float64 and col.numel() > 200
    assert torch.equal(rp, want[0]) and torch.equal(col, want[1]) and torch.equal(sh, want[2])
    # fill's d2, pair_d2_pbc and the definition agree
    rows = np.repeat(np.arange(sum(sizes)), np.diff(rp.numpy()))
    S = ops.unpack_shift(sh, 3).numpy().astype(np.float64)
    diff = pos[rows] - (pos[col.numpy()] + np.einsum("ea,eac->ec", S, cells[seg.numpy()[rows]]))
    assert np.abs(d2.numpy() - (diff ** 2).sum(1)).max() < 1e-12
    again = ops.pair_d2_pbc(rp, col, sh, torch.tensor(pos), 3, ct, seg)
    assert float((again - d2).abs().max()) < 1e-12


def test_out_buffers_tails_and_a_short_rowptr():
    pos, cells, rowptr, col, shift, d2 = pg.reference(3, False)
    gp, seg = batch_of(SIZES)
    p, ct = torch.tensor(pos), torch.tensor(pg.cell_table(cells, 3))
    ni = torch.tensor(NIMG, dtype=torch.int32)
    nnz = col.numel()
    out = torch.full((nnz + 4,), -7, dtype=torch.int32)
    sh = torch.full((nnz + 4,), -7, dtype=torch.int32)
    dd = torch.full((nnz + 4,), -7.0)
    ops.radius_pbc_fill(p, 3, R, gp, seg, ct, ni, rowptr, out=out, shift=sh, d2=dd)
    assert torch.equal(out[:nnz], col) and torch.equal(sh[:nnz], shift) and torch.equal(dd[:nnz], d2)
    assert bool((out[nnz:] == -7).all()) and bool((sh[nnz:] == -7).all()) and bool((dd[nnz:] == -7).all())
    with pytest.raises(ValueError, match="nimg must be"):
        ops.radius_pbc_count(p, 3, R, gp, seg, ct, ni[:3])
    with pytest.raises(ValueError, match="cell must be"):
        ops.radius_pbc_count(p, 3, R, gp, seg, ct[:, :6], ni)
    with pytest.raises(ValueError, match="shift"):
        ops.pair_d2_pbc(rowptr, col, shift[:5], p, 3, ct, seg)


# ---------------------------------------------------------------- image_ranges

CELLS = {
    "cubic": np.eye(3) * 2.0,
    "orthorhombic": np.diag([1.5, 2.5, 4.0]),
    "triclinic": np.array([[2.0, 0.0, 0.0], [0.7, 2.2, 0.0], [-0.5, 0.6, 1.8]]),
    "sheared": np.array([[2.0, 0.0, 0.0], [1.6, 1.2, 0.0], [-1.1, 1.3, 1.1]]),       # heights well below the lengths
    "rotated": np.array([[1.2, 1.1, -0.4], [-1.3, 1.4, 0.9], [0.8, -0.2, 1.7]]),
}


@pytest.mark.parametrize("pbc", [(True, True, True), (True, False, True), (False, False, True), (False, True, False)])
@pytest.mark.parametrize("name", sorted(CELLS))
def test_image_ranges_miss_no_edge_of_wrapped_positions(name, pbc):
    C = CELLS[name].astype(np.float32).astype(np.float64)
    r = 1.6
    ni = image_ranges(torch.tensor(C), pbc, r)
    assert ni.shape == (1, 3) and ni.dtype == torch.int32
    heights = 1 / np.linalg.norm(np.linalg.inv(C), axis=0)
    for a in range(3):
        assert int(ni[0, a]) == (int(np.ceil(r / heights[a] * (1 + 2.0 ** -20))) if pbc[a] else 0)
    rng = np.random.default_rng(3)
    pos = rng.normal(size=(24, 3)) * 1.5
    pos = wrap_positions(torch.tensor(pos), torch.tensor(C), pbc).numpy()
    nimg = [tuple(ni[0].tolist())]
    wide = [tuple(k + 2 if per else 0 for k, per in zip(nimg[0], pbc))]
    a = pg.ref_pbc(pos, 3, r, [24], C[None], nimg, False, check_exact=False)
    b = pg.ref_pbc(pos, 3, r, [24], C[None], wide, False, check_exact=False)
    assert a[1].numel() > 30
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    if name == "sheared" and all(pbc):
        assert int(ni.max()) >= 3                   # the shear costs images: the ranges follow the heights


def test_image_ranges_shapes_batches_and_errors():
    C = torch.tensor(np.stack([CELLS["cubic"], CELLS["sheared"], CELLS["triclinic"]]))
    pbc = torch.tensor([[True, True, True], [False, True, False], [False, False, False]])
    ni = image_ranges(C, pbc, 1.0)
    assert ni.shape == (3, 3)
    assert ni[0].tolist() == [1, 1, 1] and ni[1, 0] == 0 and ni[1, 1] > 0 and ni[1, 2] == 0 and ni[2].tolist() == [0] * 3
    assert image_ranges(C, True, 1.0)[0].tolist() == [1, 1, 1]
    assert image_ranges(torch.eye(2) * 2, (True, False), 3.0).tolist() == [[2, 0, 0]]
    assert image_ranges(torch.eye(1) * 0.4, True, 1.0).tolist() == [[3, 0, 0]]
    assert image_ranges(torch.eye(3), True, 0.0).tolist() == [[0, 0, 0]]
    assert image_ranges(torch.eye(3), True, 1.0).tolist() == [[2, 2, 2]]       # the 2^-20 slack: never too few
    assert image_ranges(torch.zeros(3, 3), False, 1.0).tolist() == [[0, 0, 0]]  # nothing periodic: nothing to invert
    with pytest.raises(ValueError, match="singular"):
        image_ranges(torch.zeros(3, 3), (False, True, False), 1.0)
    with pytest.raises(ValueError, match="singular"):
        image_ranges(torch.tensor([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]]), True, 1.0)
    with pytest.raises(ValueError, match=r"cutoff 4 reaches 9 images along axis 1 of graph 0, whose cell is 0\.5 high"):
        image_ranges(torch.diag(torch.tensor([4.0, 0.5, 4.0])), True, 4.0)
    assert image_ranges(torch.diag(torch.tensor([4.0, 0.5, 4.0])), (True, False, True), 3.9).tolist() == [[1, 0, 1]]
    assert int(image_ranges(torch.eye(3), True, 6.9).max()) == ops.PBC_NIMG_MAX == 7
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            image_ranges(torch.eye(3), True, bad)


# ---------------------------------------------------------------- wrap_positions

def test_wrap_positions():
    rng = np.random.default_rng(8)
    sizes = [7, 0, 9]
    # the cells are those of the kernels, fp32: rounded here so that the check uses the same
    cells = torch.tensor(np.stack([CELLS["sheared"], CELLS["cubic"], CELLS["rotated"]])).float().double()
    pbc = torch.tensor([[True, True, True], [True, True, True], [True, False, True]])
    pos = torch.tensor(rng.normal(size=(16, 3)) * 6, requires_grad=True)
    gptr = torch.tensor(pg.gptr_of(sizes))
    w = wrap_positions(pos, cells, pbc, gptr)
    gid = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    inv = torch.linalg.inv(cells)[gid]
    frac = (w.detach()[:, None, :] @ inv)[:, 0, :]
    per = pbc[gid]
    assert bool((frac[per] >= -1e-12).all()) and bool((frac[per] < 1 + 1e-12).all())
    moved = ((w.detach() - pos.detach())[:, None, :] @ inv)[:, 0, :]
    assert float((moved - moved.round()).abs().max()) < 1e-12            # whole lattice vectors only
    assert bool((moved[~per].abs() < 1e-12).all())                         # none along an axis that is not periodic
    assert float(moved.abs().max()) >= 1
    w.sum().backward()
    assert torch.equal(pos.grad, torch.ones_like(pos))
    again = wrap_positions(w.detach(), cells, pbc, GraphBatch(gptr))
    assert float((again - w.detach()).abs().max()) < 1e-12
    one = wrap_positions(pos.detach()[:7], cells[0], True)
    assert torch.equal(one, w.detach()[:7])
    assert wrap_positions(torch.zeros(0, 3), cells[0], True).shape == (0, 3)


# ---------------------------------------------------------------- symmetry, nimg = 0

def test_every_edge_has_its_mirror():
    for D, loop in ((1, True), (2, False), (3, False)):
        pos, cells, rowptr, col, shift, d2 = pg.reference(D, loop)
        rows = torch.repeat_interleave(torch.arange(rowptr.numel() - 1), (rowptr[1:] - rowptr[:-1]).long())
        S = ops.unpack_shift(shift, 3)
        fwd = {(int(i), int(j)) + tuple(s) for i, j, s in zip(rows, col, S.tolist())}
        bwd = {(int(j), int(i)) + tuple(-k for k in s) for i, j, s in zip(rows, col, S.tolist())}
        assert len(fwd) == col.numel() and fwd == bwd
        assert any(i == j for i, j, *_ in fwd)      # an atom sees its own images


@pytest.mark.parametrize("D", [1, 2, 3])
def test_no_images_is_the_radius_search_bit_for_bit(D):
    pos, cells, _, _, _, _ = pg.reference(D, False)
    gp, seg = batch_of(SIZES)
    zero = [(0, 0, 0)] * len(SIZES)
    for loop in (False, True):
        rp, col, sh, d2 = cpu_search(pos, D, R, SIZES, cells, zero, loop)
        p = torch.tensor(pos)
        deg = ops.radius_count(p, D, R, gp, seg, loop=loop)
        wcol, wd2 = ops.radius_fill(p, D, R, gp, seg, rp, loop=loop, with_d2=True)
        assert torch.equal(rp[1:] - rp[:-1], deg) and torch.equal(col, wcol)
        assert torch.equal(d2.view(torch.int32), wd2.view(torch.int32)) and bool((sh == 0).all())
    g = radius_graph(torch.tensor(pos[:, :D]), R, torch.tensor(pg.gptr_of(SIZES)), cell=torch.tensor(cells), pbc=False)
    h = radius_graph(torch.tensor(pos[:, :D]), R, torch.tensor(pg.gptr_of(SIZES)))
    assert torch.equal(g.rowptr, h.rowptr) and torch.equal(g.col, h.col) and torch.equal(g.d2, h.d2)
    assert h.shift is None and h.cell is None and bool((g.shift == 0).all())
    # a non-periodic search over a periodic graph's batch does not inherit its shifts
    assert radius_graph(torch.tensor(pos[:, :D]), R, g).shift is None


# ---------------------------------------------------------------- pair ops, autograd, the API

def periodic_graph(dtype=torch.float64):
    rng = np.random.default_rng(2)
    sizes = [6, 1, 9]
    cells = torch.tensor(np.stack([CELLS["triclinic"], CELLS["cubic"] * 0.7, CELLS["rotated"]]))
    pbc = torch.tensor([[True, True, True], [True, True, True], [True, True, False]])
    batch = GraphBatch(torch.tensor(pg.gptr_of(sizes)))
    pos = wrap_positions(torch.tensor(rng.normal(size=(16, 3)) * 2), cells, pbc, batch).to(dtype)
    return pos, cells, pbc, batch, radius_graph(pos, 2.3, batch, cell=cells, pbc=pbc)


def test_pair_d2_pbc_bwd_cpu_equals_the_definition():
    pos, cells, pbc, batch, g = periodic_graph()
    rng = np.random.default_rng(4)
    gv = rng.normal(size=g.col.numel())
    want = pg.ref_bwd_pbc(pos.numpy(), 3, g.rowptr.numpy(), g.col.numpy(), g.shifts().numpy(),
                          cells.float().double().numpy(), g.batch.numpy(), gv)
    rp_t, col_t, eperm_t = g.transposed_perm()
    got = ops.pair_d2_pbc_bwd(g.rowptr, g.col, g.shift, rp_t, col_t, eperm_t, pos, torch.tensor(gv), 3, g.cell,
                              g.batch)
    assert np.abs(got.numpy() - want).max() < 1e-12 and np.abs(want).max() > 1
    fp32 = ops.pair_d2_pbc_bwd(g.rowptr, g.col, g.shift, rp_t, col_t, eperm_t, pos.float(),
                               torch.tensor(gv).float(), 3, g.cell, g.batch)
    assert fp32.dtype == torch.float32 and np.abs(fp32.numpy() - want).max() < 1e-4 * np.abs(want).max()


def test_pair_distance_autograd_on_a_periodic_graph_against_fp64():
    pos, cells, pbc, batch, g = periodic_graph()
    assert g.col.numel() > 100 and int((g.shift != 0).sum()) > 50 and g.d2.dtype == torch.float64
    rows = torch.repeat_interleave(torch.arange(16), (g.rowptr[1:] - g.rowptr[:-1]).long())
    assert bool((rows == g.col.long()).any())       # the one-atom graph: its own images
    off = torch.einsum("ea,eac->ec", g.shifts().double(), g.cell.view(-1, 3, 3).double()[g.batch.long()[rows]])
    wgt = torch.tensor(np.random.default_rng(1).normal(size=g.col.numel()))
    for squared in (True, False):
        p = pos.clone().requires_grad_(True)
        out = pair_distance(p, g, squared=squared)
        (out * wgt).sum().backward()
        q = pos.clone().requires_grad_(True)
        t = ((q[rows] - (q[g.col.long()] + off)) ** 2).sum(1)
        ref = t if squared else torch.sqrt(t)
        (ref * wgt).sum().backward()
        assert float((out.detach() - ref.detach()).abs().max()) < 1e-12
        assert float((p.grad - q.grad).abs().max()) < 1e-12 and float(q.grad.abs().max()) > 0.1
    assert float((pair_distance(pos, g, squared=True) - g.d2).abs().max()) < 1e-12


def test_graph_batch_carries_shift_and_cell():
    pos, cells, pbc, batch, g = periodic_graph(torch.float32)
    assert g.shift.dtype == torch.int32 and g.shift.shape == g.col.shape
    assert g.cell.dtype == torch.float32 and g.cell.shape == (3, 9)
    assert torch.equal(g.cell.view(3, 3, 3), cells.float())
    assert g.shifts().shape == (g.col.numel(), 3) and g.shifts().dtype == torch.int32
    assert torch.equal(ops._pack_shift(g.shifts()), g.shift)
    h = g.to("cpu")
    assert h is not g and torch.equal(h.shift, g.shift) and torch.equal(h.cell, g.cell)
    plain = GraphBatch(torch.tensor([0, 3]))
    assert plain.shift is None and plain.cell is None and plain.to("cpu").shift is None
    with pytest.raises(ValueError, match="not a periodic graph"):
        plain.shifts()
    with pytest.raises(NotImplementedError):
        radius_graph(pos, 1.0, batch, cell=cells, max_num_neighbors=3)


def test_schnet_takes_a_cell_on_the_cpu():
    pos, cells, pbc, batch, g = periodic_graph(torch.float32)
    z = torch.arange(16) % 5 + 1
    model = SchNet(hidden=16, n_filters=16, n_interactions=1, n_gaussians=8, cutoff=2.3,
                   generator=torch.Generator().manual_seed(1))
    nb = model.neighbors(pos, batch, cell=cells, pbc=pbc)
    assert torch.equal(nb.col, g.col) and torch.equal(nb.shift, g.shift)
    E, F = model.energy_and_forces(z, pos, batch, cell=cells, pbc=pbc)
    E2 = model(z, pos, graph=nb)
    assert E.shape == (3,) and F.shape == (16, 3) and torch.equal(E, E2.detach())
    free = model(z, pos, batch).detach()
    assert float((E - free).abs().max()) > 1e-4     # the images are felt
    # a lattice translation of one graph's atoms, wrapped back, changes nothing to rounding
    moved = pos.clone()
    moved[:6] += (cells[0][1] - 2 * cells[0][0]).float()
    E3, _ = model.energy_and_forces(z, wrap_positions(moved, cells, pbc, batch), batch, cell=cells, pbc=pbc)
    assert float((E3 - E).abs().max()) < 1e-4 * max(1.0, float(E.abs().max()))
