"""Return codes of the periodic geometry launchers (gnn_geometry.hip:
gnn_launch_radius_pbc_count, gnn_launch_radius_pbc_fill, gnn_launch_pair_d2_pbc,
gnn_launch_pair_d2_pbc_bwd), pinned without a GPU, in the form of
test_gnn_geometry_codes_cpu.py.

Every rejection and every zero-row return happens before the first HIP call: pointers are 0
or a dummy non-null integer that is never dereferenced.  The ORDER of the checks is API
(cgnn_api.h), the one of the non-periodic launchers: the compiled shape -- D in 1..3, lanes
in {0, 8, 16, 32, 64} -- (-1); ldp < D, nnz < 0 or an r that is negative or not finite (-3);
the zero-row return (n <= 0, and nnz == 0 in the pair kernels); the required pointers --
cell, nimg, seg_id and the fill's shift among them -- and G >= 1 (-3); the grid (-4).  The
max_images hint only chooses the width: no value of it is an error.  A row of the table is
(id, (binding, arguments), code), code ``None`` meaning that the call returns normally.  No row
reaches a launch.
"""
import re

import pytest

from cgnn_amd import native

P = 64                  # a non-null pointer; never dereferenced
OK = None
NAN, INF = float("nan"), float("inf")
HUGE = 2 ** 31 - 1      # rows: more blocks than a launch may have, for every lanes value


def count(n=5, G=2, D=3, ldp=3, r=1.0, loop=0, lanes=0, images=27, pos=P, gptr=P, seg=P, cell=P, nimg=P, deg=P):
    return "gnn_radius_pbc_count", (pos, gptr, seg, cell, nimg, deg, n, G, D, ldp, r, loop, lanes, images, 0)


def fill(n=5, G=2, D=3, ldp=3, r=1.0, loop=0, lanes=0, images=27, pos=P, gptr=P, seg=P, cell=P, nimg=P, rowptr=P,
         col=P, shift=P, d2=0):
    return "gnn_radius_pbc_fill", (pos, gptr, seg, cell, nimg, rowptr, col, shift, d2, n, G, D, ldp, r, loop, lanes,
                                   images, 0)


def pair(n=5, nnz=9, G=2, D=3, ldp=3, lanes=0, rowptr=P, col=P, shift=P, pos=P, cell=P, seg=P, d2=P):
    return "gnn_pair_d2_pbc", (rowptr, col, shift, pos, cell, seg, d2, n, nnz, G, D, ldp, lanes, 0)


def bwd(n=5, nnz=9, G=2, D=3, ldp=3, lanes=0, rowptr=P, col=P, shift=P, rowptr_t=P, col_t=P, eperm_t=P, pos=P,
        cell=P, seg=P, g=P, dpos=P):
    return "gnn_pair_d2_pbc_bwd", (rowptr, col, shift, rowptr_t, col_t, eperm_t, pos, cell, seg, g, dpos, n, nnz, G, D,
                                   ldp, lanes, 0)


NAMES = ("gnn_radius_pbc_count", "gnn_radius_pbc_fill", "gnn_pair_d2_pbc", "gnn_pair_d2_pbc_bwd")
BAD_LANES = (-8, 1, 4, 7, 12, 24, 48, 128)
GOOD_LANES = (0, 8, 16, 32, 64)

TABLE = []
for name, fn in (("count", count), ("fill", fill)):
    TABLE += [
        ("%s D = 0" % name, fn(D=0), -1),
        ("%s D = 4" % name, fn(D=4, ldp=4), -1),
        ("%s D = -1" % name, fn(D=-1), -1),
        ("%s D before ldp" % name, fn(D=4, ldp=3), -1),
        ("%s D before r" % name, fn(D=4, ldp=4, r=-1.0), -1),
        ("%s D before zero rows" % name, fn(D=0, n=0), -1),
        ("%s lanes before r" % name, fn(lanes=12, r=NAN), -1),
        ("%s lanes before zero rows" % name, fn(lanes=5, n=0), -1),
        ("%s lanes before null pointers" % name, fn(lanes=5, pos=0, cell=0, nimg=0), -1),
        ("%s ldp < D" % name, fn(D=3, ldp=2), -3),
        ("%s ldp = 0" % name, fn(D=1, ldp=0), -3),
        ("%s ldp < D with zero rows" % name, fn(D=2, ldp=1, n=0), -3),
        ("%s r < 0" % name, fn(r=-0.5), -3),
        ("%s r = nan" % name, fn(r=NAN), -3),
        ("%s r = inf" % name, fn(r=INF), -3),
        ("%s r = -inf" % name, fn(r=-INF), -3),
        ("%s r < 0 with zero rows" % name, fn(r=-1.0, n=0), -3),
        ("%s r before null pointers" % name, fn(r=NAN, pos=0, cell=0, nimg=0), -3),
        ("%s r = 0 is a radius" % name, fn(r=0.0, n=0), OK),
        ("%s zero rows before null pointers" % name, fn(n=0, pos=0, gptr=0, seg=0, cell=0, nimg=0), OK),
        ("%s negative rows, null pointers" % name, fn(n=-3, pos=0, gptr=0, seg=0, cell=0, nimg=0), OK),
        ("%s zero rows, no graphs" % name, fn(n=0, G=0), OK),
        ("%s null pos" % name, fn(pos=0), -3),
        ("%s null gptr" % name, fn(gptr=0), -3),
        ("%s null seg_id" % name, fn(seg=0), -3),
        ("%s null cell" % name, fn(cell=0), -3),
        ("%s null nimg" % name, fn(nimg=0), -3),
        ("%s no graphs" % name, fn(G=0), -3),
        ("%s null cell before the grid" % name, fn(n=HUGE, cell=0), -3),
        ("%s null nimg before the grid" % name, fn(n=HUGE, nimg=0), -3),
        ("%s grid" % name, fn(n=HUGE), -4),
    ] + [("%s lanes = %d" % (name, l), fn(lanes=l), -1) for l in BAD_LANES] + [
        ("%s lanes = %d, zero rows" % (name, l), fn(lanes=l, n=0), OK) for l in GOOD_LANES] + [
        ("%s lanes = %d grid" % (name, l), fn(lanes=l, n=HUGE), -4) for l in GOOD_LANES] + [
        ("%s max_images = %d is a hint, grid" % (name, m), fn(images=m, n=HUGE), -4)
        for m in (-5, 0, 1, 343, 3375, 10 ** 6)] + [
        ("%s max_images = %d is a hint, zero rows" % (name, m), fn(images=m, n=0), OK) for m in (-5, 0, 10 ** 6)] + [
        ("%s D = %d ldp = %d, zero rows" % (name, d, ld), fn(D=d, ldp=ld, n=0), OK)
        for d in (1, 2, 3) for ld in (d, 4, 8)]
TABLE += [
    ("count null deg", count(deg=0), -3),
    ("fill null rowptr", fill(rowptr=0), -3),
    ("fill null col", fill(col=0), -3),
    ("fill null shift", fill(shift=0), -3),
    ("fill null shift with d2", fill(shift=0, d2=P), -3),
    ("fill null shift before the grid", fill(n=HUGE, shift=0), -3),
    ("fill d2 is optional", fill(n=0, d2=P), OK),
    ("fill d2 is optional, grid", fill(n=HUGE, d2=0), -4),
]
for name, fn in (("pair", pair), ("bwd", bwd)):
    TABLE += [
        ("%s D = 0" % name, fn(D=0), -1),
        ("%s D = 4" % name, fn(D=4, ldp=4), -1),
        ("%s D before ldp" % name, fn(D=4, ldp=3), -1),
        ("%s D before zero rows" % name, fn(D=0, n=0), -1),
        ("%s D before no edges" % name, fn(D=5, ldp=8, nnz=0), -1),
        ("%s lanes before nnz < 0" % name, fn(lanes=12, nnz=-1), -1),
        ("%s lanes before null pointers" % name, fn(lanes=5, rowptr=0, shift=0, cell=0), -1),
        ("%s ldp < D" % name, fn(D=3, ldp=2), -3),
        ("%s ldp < D with zero rows" % name, fn(D=2, ldp=1, n=0), -3),
        ("%s ldp < D without edges" % name, fn(D=2, ldp=1, nnz=0), -3),
        ("%s nnz < 0" % name, fn(nnz=-1), -3),
        ("%s nnz < 0 with zero rows" % name, fn(nnz=-1, n=0), -3),
        ("%s zero rows before null pointers" % name, fn(n=0, rowptr=0, col=0, shift=0, pos=0, cell=0, seg=0), OK),
        ("%s negative rows, null pointers" % name, fn(n=-1, rowptr=0, col=0, shift=0, pos=0, cell=0, seg=0), OK),
        ("%s no edges before null pointers" % name, fn(nnz=0, rowptr=0, col=0, shift=0, pos=0, cell=0, seg=0), OK),
        ("%s no edges before no graphs" % name, fn(nnz=0, G=0), OK),
        ("%s null rowptr" % name, fn(rowptr=0), -3),
        ("%s null col" % name, fn(col=0), -3),
        ("%s null shift" % name, fn(shift=0), -3),
        ("%s null pos" % name, fn(pos=0), -3),
        ("%s null cell" % name, fn(cell=0), -3),
        ("%s null seg_id" % name, fn(seg=0), -3),
        ("%s no graphs" % name, fn(G=0), -3),
        ("%s null cell before the grid" % name, fn(n=HUGE, cell=0), -3),
        ("%s null shift before the grid" % name, fn(n=HUGE, shift=0), -3),
        ("%s grid" % name, fn(n=HUGE), -4),
    ] + [("%s lanes = %d" % (name, l), fn(lanes=l), -1) for l in BAD_LANES] + [
        ("%s lanes = %d, zero rows" % (name, l), fn(lanes=l, n=0), OK) for l in GOOD_LANES] + [
        ("%s lanes = %d grid" % (name, l), fn(lanes=l, n=HUGE), -4) for l in GOOD_LANES] + [
        ("%s D = %d ldp = %d, no edges" % (name, d, ld), fn(D=d, ldp=ld, nnz=0), OK)
        for d in (1, 2, 3) for ld in (d, 4, 8)]
TABLE += [
    ("pair null d2", pair(d2=0), -3),
    ("bwd null rowptr_t", bwd(rowptr_t=0), -3),
    ("bwd null col_t", bwd(col_t=0), -3),
    ("bwd null eperm_t", bwd(eperm_t=0), -3),
    ("bwd null g", bwd(g=0), -3),
    ("bwd null dpos", bwd(dpos=0), -3),
]


def test_the_table_names_the_four_launchers_and_every_case_once():
    ids = [t[0] for t in TABLE]
    assert len(set(ids)) == len(ids)
    assert {t[1][0] for t in TABLE} == set(NAMES)
    for name in NAMES:
        assert {t[2] for t in TABLE if t[1][0] == name} == {OK, -1, -3, -4}, name


@pytest.mark.parametrize("call,code", [pytest.param(c, code, id=i) for i, c, code in TABLE])
def test_launcher_code(call, code):
    name, args = call
    fn = getattr(native.hip(), name)
    if code is OK:
        fn(*args)
        return
    with pytest.raises(RuntimeError) as err:
        fn(*args)
    assert re.search(r"\(code %d\)" % code, str(err.value)), str(err.value)
