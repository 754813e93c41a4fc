"""Return codes of the k-NN launchers (gnn_geometry.hip: gnn_launch_knn_select,
gnn_launch_knn_fill), pinned without a GPU, in the form of test_gnn_geometry_codes_cpu.py.

Every rejection and every zero-row return happens before the first HIP call: pointers are 0
or a dummy non-null integer that is never dereferenced.  The ORDER of the checks is API
(cgnn_api.h): the compiled shape -- D in 1..3, k in 1..64 (select), lanes in {0, 8, 16, 32, 64}
and, in select, lanes >= k when given (a sub-group holds one key per lane) -- (-1); ldp < D or
an r that is negative or NaN (select; +inf is "no radius") (-3); the zero-row return
(n <= 0); the required pointers and G >= 1 (-3); the grid (-4).  A row of the table is
(id, (binding, arguments), code), code ``None`` meaning that the call returns normally.  No
row reaches a launch.
"""
import re

import pytest

from cgnn_amd import native

P = 64                  # a non-null pointer; never dereferenced
OK = None
NAN, INF = float("nan"), float("inf")
HUGE = 2 ** 31 - 1      # rows: more blocks than a launch may have, for every lanes value


def select(n=5, G=2, D=3, ldp=3, k=4, r=1.0, loop=0, lanes=0, pos=P, gptr=P, seg=P, deg=P, tau_d2=P, tau_j=P):
    return "gnn_knn_select", (pos, gptr, seg, deg, tau_d2, tau_j, n, G, D, ldp, k, r, loop, lanes, 0)


def fill(n=5, G=2, D=3, ldp=3, loop=0, lanes=0, pos=P, gptr=P, seg=P, rowptr=P, tau_d2=P, tau_j=P, col=P, d2=0):
    return "gnn_knn_fill", (pos, gptr, seg, rowptr, tau_d2, tau_j, col, d2, n, G, D, ldp, loop, lanes, 0)


BAD_LANES = (-8, 1, 4, 7, 12, 24, 48, 128)
GOOD_LANES = (0, 8, 16, 32, 64)

TABLE = []
for name, fn in (("select", select), ("fill", fill)):
    TABLE += [
        ("%s D = 0" % name, fn(D=0), -1),
        ("%s D = 4" % name, fn(D=4, ldp=4), -1),
        ("%s D = -1" % name, fn(D=-1), -1),
        ("%s D before ldp" % name, fn(D=4, ldp=3), -1),
        ("%s D before zero rows" % name, fn(D=0, n=0), -1),
        ("%s lanes before ldp" % name, fn(lanes=12, ldp=2), -1),
        ("%s lanes before zero rows" % name, fn(lanes=5, n=0), -1),
        ("%s lanes before null pointers" % name, fn(lanes=5, pos=0, gptr=0, seg=0), -1),
        ("%s ldp < D" % name, fn(D=3, ldp=2), -3),
        ("%s ldp = 0" % name, fn(D=1, ldp=0), -3),
        ("%s ldp < D with zero rows" % name, fn(D=2, ldp=1, n=0), -3),
        ("%s ldp before null pointers" % name, fn(ldp=2, pos=0, gptr=0, seg=0), -3),
        ("%s zero rows before null pointers" % name, fn(n=0, pos=0, gptr=0, seg=0), OK),
        ("%s negative rows, null pointers" % name, fn(n=-3, pos=0, gptr=0, seg=0), OK),
        ("%s zero rows, no graphs" % name, fn(n=0, G=0), OK),
        ("%s null pos" % name, fn(pos=0), -3),
        ("%s null gptr" % name, fn(gptr=0), -3),
        ("%s null seg_id" % name, fn(seg=0), -3),
        ("%s null tau_d2" % name, fn(tau_d2=0), -3),
        ("%s null tau_j" % name, fn(tau_j=0), -3),
        ("%s no graphs" % name, fn(G=0), -3),
        ("%s null pointer before the grid" % name, fn(n=HUGE, pos=0), -3),
        ("%s grid" % name, fn(n=HUGE), -4),
    ] + [("%s lanes = %d" % (name, l), fn(lanes=l), -1) for l in BAD_LANES] + [
        ("%s lanes = %d, zero rows" % (name, l), fn(lanes=l, n=0), OK) for l in GOOD_LANES] + [
        ("%s lanes = %d grid" % (name, l), fn(lanes=l, n=HUGE), -4) for l in GOOD_LANES] + [
        ("%s D = %d ldp = %d, zero rows" % (name, d, ld), fn(D=d, ldp=ld, n=0), OK)
        for d in (1, 2, 3) for ld in (d, 4, 8)]
TABLE += [
    ("select k = 0", select(k=0), -1),
    ("select k = -1", select(k=-1), -1),
    ("select k = 65", select(k=65), -1),
    ("select k = 65, lanes = 64", select(k=65, lanes=64), -1),
    ("select k before ldp", select(k=0, ldp=2), -1),
    ("select k before r", select(k=65, r=-1.0), -1),
    ("select k before zero rows", select(k=0, n=0), -1),
    ("select k before null pointers", select(k=0, pos=0, deg=0), -1),
    ("select D before r", select(D=4, ldp=4, r=-1.0), -1),
    ("select lanes before r", select(lanes=12, r=NAN), -1),
    ("select r < 0", select(r=-0.5), -3),
    ("select r = nan", select(r=NAN), -3),
    ("select r = -inf", select(r=-INF), -3),
    ("select r < 0 with zero rows", select(r=-1.0, n=0), -3),
    ("select r before null pointers", select(r=NAN, pos=0, gptr=0, seg=0), -3),
    ("select r = inf is no radius", select(r=INF, n=0), OK),
    ("select r = inf goes on to the pointers", select(r=INF, pos=0), -3),
    ("select r = inf goes on to the grid", select(r=INF, n=HUGE), -4),
    ("select r = 0 is a radius", select(r=0.0, n=0), OK),
    ("select r = -0.0 is a radius", select(r=-0.0, n=0), OK),
    ("select null deg", select(deg=0), -3),
    ("fill null rowptr", fill(rowptr=0), -3),
    ("fill null col", fill(col=0), -3),
    ("fill null col with d2", fill(col=0, d2=P), -3),
    ("fill d2 is optional", fill(n=0, d2=P), OK),
    ("fill d2 goes on to the grid", fill(n=HUGE, d2=P), -4),
]
# a sub-group holds one key per lane: a given lanes value must be at least k
TABLE += [("select k = %d lanes = %d" % (k, l), select(k=k, lanes=l, n=0), -1)
          for k, l in ((9, 8), (16, 8), (17, 16), (32, 16), (33, 32), (64, 32), (64, 8))]
TABLE += [("select k = %d lanes = %d, zero rows" % (k, l), select(k=k, lanes=l, n=0), OK)
          for k, l in ((1, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64), (1, 64), (64, 0))]
TABLE += [
    ("select lanes < k before r", select(k=9, lanes=8, r=-1.0), -1),
    ("select lanes < k before null pointers", select(k=33, lanes=32, pos=0), -1),
    ("select lanes = k grid", select(k=16, lanes=16, n=HUGE), -4),
    ("select k = 64 grid", select(k=64, n=HUGE), -4),
]


def test_the_table_names_the_two_launchers_and_every_case_once():
    ids = [t[0] for t in TABLE]
    assert len(set(ids)) == len(ids)
    assert {t[1][0] for t in TABLE} == {"gnn_knn_select", "gnn_knn_fill"}
    for name in ("gnn_knn_select", "gnn_knn_fill"):
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
