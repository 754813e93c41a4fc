"""Return codes of the cell-list launchers (gnn_cells.hip: gnn_launch_cells_grid,
gnn_launch_cells_bin, gnn_launch_cells_count, gnn_launch_cells_fill, gnn_launch_cells_rows),
pinned without a GPU, in the form of test_gnn_knn_codes_cpu.py.

Every rejection and every zero-row return happens before the first HIP call: pointers are 0
or a dummy non-null integer that is never dereferenced.  The ORDER of the checks is API
(cgnn_api.h): the compiled shape -- D in 1..3, lanes in {0, 8, 16, 32, 64} where the launcher
takes them -- (-1); ldp < D (the sorted positions: ldp != 4), a negative capacity, or an r that
is negative or not finite (-3); the zero-row return (n <= 0, and a capacity of 0 in fill and
rows); the required pointers and G >= 1 (-3); the grid (-4: more graphs than a launch has
blocks in cells_grid, more rows in count / fill / rows; cells_bin, one thread per point, has
no row count that overflows).  A row of the table is (id, (binding, arguments), code), code
``None`` meaning that the call returns normally.  No row reaches a launch.
"""
import re

import pytest

from cgnn_amd import native

P = 64                  # a non-null pointer; never dereferenced
OK = None
NAN, INF = float("nan"), float("inf")
HUGE = 2 ** 31 - 1      # rows: more blocks than a launch may have, for every lanes value


def grid(n=5, G=2, D=3, ldp=3, r=1.0, pos=P, gptr=P, part=P, glo=P, gn=P):
    return "gnn_cells_grid", (pos, gptr, part, glo, gn, n, G, D, ldp, r, 0)


def bins(n=5, G=2, D=3, ldp=3, pos=P, gptr=P, seg=P, glo=P, gn=P, cell_id=P):
    return "gnn_cells_bin", (pos, gptr, seg, glo, gn, cell_id, n, G, D, ldp, 0)


def count(n=5, G=2, D=3, ldp=4, r=1.0, loop=0, lanes=0, spos=P, perm=P, scell=P, cptr=P, gptr=P, seg=P, gn=P, deg=P):
    return "gnn_cells_count", (spos, perm, scell, cptr, gptr, seg, gn, deg, n, G, D, ldp, r, loop, lanes, 0)


def fill(n=5, G=2, D=3, ldp=4, r=1.0, loop=0, lanes=0, cap=7, spos=P, perm=P, scell=P, cptr=P, gptr=P, seg=P, gn=P,
         rowptr=P, sj=P, sd=P):
    return "gnn_cells_fill", (spos, perm, scell, cptr, gptr, seg, gn, rowptr, sj, sd, n, G, D, ldp, r, loop, lanes,
                              cap, 0)


def rows(n=5, cap=7, lanes=0, rowptr=P, sj=P, sd=P, col=P, d2=0):
    return "gnn_cells_rows", (rowptr, sj, sd, col, d2, n, cap, lanes, 0)


BAD_LANES = (-8, 1, 4, 7, 12, 24, 48, 128)
GOOD_LANES = (0, 8, 16, 32, 64)

TABLE = []
# the dimension and the row stride: the four launchers that take positions
for name, fn, ld in (("grid", grid, 3), ("bin", bins, 3), ("count", count, 4), ("fill", fill, 4)):
    TABLE += [
        ("%s D = 0" % name, fn(D=0), -1),
        ("%s D = 4" % name, fn(D=4, ldp=4), -1),
        ("%s D = -1" % name, fn(D=-1), -1),
        ("%s D before ldp" % name, fn(D=4, ldp=2), -1),
        ("%s D before zero rows" % name, fn(D=0, n=0), -1),
        ("%s ldp < D" % name, fn(D=3, ldp=2), -3),
        ("%s ldp < D with zero rows" % name, fn(D=2, ldp=1, n=0), -3),
        ("%s zero rows before null pointers" % name, fn(n=0, gptr=0, gn=0), OK),
        ("%s negative rows, null pointers" % name, fn(n=-3, gptr=0, gn=0), OK),
        ("%s zero rows, no graphs" % name, fn(n=0, G=0), OK),
        ("%s null gptr" % name, fn(gptr=0), -3),
        ("%s null gn" % name, fn(gn=0), -3),
        ("%s no graphs" % name, fn(G=0), -3),
    ] + [("%s D = %d, zero rows" % (name, d), fn(D=d, ldp=max(d, ld), n=0), OK) for d in (1, 2, 3)]
# the radius: the three launchers that take one
for name, fn in (("grid", grid), ("count", count), ("fill", fill)):
    TABLE += [
        ("%s D before r" % name, fn(D=4, ldp=4, r=-1.0), -1),
        ("%s r < 0" % name, fn(r=-0.5), -3),
        ("%s r = nan" % name, fn(r=NAN), -3),
        ("%s r = inf" % name, fn(r=INF), -3),
        ("%s r = -inf" % name, fn(r=-INF), -3),
        ("%s r < 0 with zero rows" % name, fn(r=-1.0, n=0), -3),
        ("%s r before null pointers" % name, fn(r=NAN, gptr=0), -3),
        ("%s r = 0 is a radius" % name, fn(r=0.0, n=0), OK),
        ("%s r = -0.0 is a radius" % name, fn(r=-0.0, n=0), OK),
    ]
# the sorted positions are [n, 4]
for name, fn in (("count", count), ("fill", fill)):
    TABLE += [
        ("%s ldp = 3" % name, fn(ldp=3), -3),
        ("%s ldp = 8" % name, fn(ldp=8), -3),
        ("%s ldp = 8 with zero rows" % name, fn(ldp=8, n=0), -3),
        ("%s lanes before ldp" % name, fn(lanes=12, ldp=3), -1),
        ("%s lanes before r" % name, fn(lanes=12, r=NAN), -1),
        ("%s null spos" % name, fn(spos=0), -3),
        ("%s null perm" % name, fn(perm=0), -3),
        ("%s null scell" % name, fn(scell=0), -3),
        ("%s null cptr" % name, fn(cptr=0), -3),
        ("%s null seg_id" % name, fn(seg=0), -3),
    ]
# the sub-group width: the three launchers that take one
for name, fn in (("count", count), ("fill", fill), ("rows", rows)):
    TABLE += [
        ("%s lanes before zero rows" % name, fn(lanes=5, n=0), -1),
        ("%s lanes before null pointers" % name, fn(lanes=5, rowptr=0) if name != "count" else fn(lanes=5, deg=0), -1),
        ("%s null pointer before the grid" % name, fn(n=HUGE, rowptr=0) if name != "count" else fn(n=HUGE, deg=0), -3),
        ("%s grid" % name, fn(n=HUGE, cap=HUGE) if name != "count" else fn(n=HUGE), -4),
    ] + [("%s lanes = %d" % (name, l), fn(lanes=l), -1) for l in BAD_LANES] + [
        ("%s lanes = %d, zero rows" % (name, l), fn(lanes=l, n=0), OK) for l in GOOD_LANES] + [
        ("%s lanes = %d grid" % (name, l), fn(lanes=l, n=HUGE, cap=HUGE) if name != "count" else fn(lanes=l, n=HUGE),
         -4) for l in GOOD_LANES]
# the capacity of the edge buffers: fill and rows
for name, fn in (("fill", fill), ("rows", rows)):
    TABLE += [
        ("%s cap < 0" % name, fn(cap=-1), -3),
        ("%s cap < 0 with zero rows" % name, fn(cap=-1, n=0), -3),
        ("%s cap < 0 before null pointers" % name, fn(cap=-1, rowptr=0), -3),
        ("%s lanes before cap" % name, fn(lanes=12, cap=-1), -1),
        ("%s no edges before null pointers" % name, fn(cap=0, rowptr=0, sj=0, sd=0), OK),
        ("%s null rowptr" % name, fn(rowptr=0), -3),
        ("%s null scratch ids" % name, fn(sj=0), -3),
        ("%s null scratch d2" % name, fn(sd=0), -3),
    ]
TABLE += [
    ("grid null pos", grid(pos=0), -3),
    ("grid null part", grid(part=0), -3),
    ("grid null glo", grid(glo=0), -3),
    ("grid null pointer before the grid", grid(G=2 ** 24, glo=0), -3),
    ("grid graphs", grid(G=2 ** 24), -4),
    ("grid graphs below the limit, zero rows", grid(G=2 ** 24 - 1, n=0), OK),
    ("bin null pos", bins(pos=0), -3),
    ("bin null seg_id", bins(seg=0), -3),
    ("bin null glo", bins(glo=0), -3),
    ("bin null cell_id", bins(cell_id=0), -3),
    ("count null deg", count(deg=0), -3),
    ("rows null col", rows(col=0), -3),
    ("rows null col with d2", rows(col=0, d2=P), -3),
    ("rows d2 is optional", rows(n=0, d2=P), OK),
    ("rows d2 goes on to the grid", rows(n=HUGE, cap=HUGE, d2=P), -4),
]

NAMES = {"gnn_cells_grid", "gnn_cells_bin", "gnn_cells_count", "gnn_cells_fill", "gnn_cells_rows"}


def test_the_table_names_the_five_launchers_and_every_case_once():
    ids = [t[0] for t in TABLE]
    assert len(set(ids)) == len(ids)
    assert {t[1][0] for t in TABLE} == NAMES
    for name in NAMES:
        codes = {t[2] for t in TABLE if t[1][0] == name}
        assert codes == ({OK, -1, -3} if name == "gnn_cells_bin" else {OK, -1, -3, -4}), name


def test_the_scratch_of_the_grid_is_eight_floats_per_chunk():
    f = native.hip().gnn_cells_grid_floats
    assert [f(n) for n in (-1, 0, 1, 1024, 1025, 2048, 2 ** 31 - 1)] == [0, 0, 8, 8, 16, 16, 8 * 2 ** 21]


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
