"""Return codes of the row-per-sub-group CSR launchers (gnn_wspmm.hip, gnn_pool.hip,
gnn_espmm.hip and spmm in gnn_sparse.hip), pinned without a GPU.

Every rejection and every zero-row return of these launchers happens before the first HIP
call, so the bindings can be called on a machine without a device: pointers are 0 or a dummy
non-null integer that is never dereferenced.  The codes and the ORDER of the checks are API
(cgnn_api.h): -3 a bad shape or a missing pointer, -5 an element type (pair) that is not
compiled, -1 an op that is not compiled.  A row of the table is (binding, arguments, code),
code ``None`` meaning that the call returns normally.  No row reaches a launch.
"""
import re

import pytest

from cgnn_amd import native

P = 64                  # a non-null pointer; never dereferenced
OK = None


def wspmm(n=5, F=16, ldx=16, ldy=16, xt=1, yt=1, relu=0, ptr=P):
    return "gnn_wspmm", (ptr,) * 9 + (n, F, ldx, ldy, xt, yt, relu, 0)


def sddmm(n=5, F=16, lda=16, ldb=16, t=1, ptr=P):
    return "gnn_sddmm", (ptr,) * 7 + (n, F, lda, ldb, t, 0)


def pool_fwd(n=5, F=16, ldx=16, ldy=16, ldarg=16, t=1, is_min=0, rowptr=P, x=P, y=P, arg=P):
    return "gnn_pool_fwd", (rowptr, P, x, y, arg, n, F, ldx, ldy, ldarg, t, is_min, 0)


def pool_bwd(n=5, F=16, ldarg=16, lddy=16, lddx=16, tdy=1, tdx=1, rowptr=P, arg=P, dy=P, dx=P):
    return "gnn_pool_bwd", (rowptr, P, P, arg, ldarg, dy, lddy, dx, lddx, n, F, tdy, tdx, 0)


def espmm(n=5, F=16, ldx=16, lde=16, ldy=16, t=1, op=0, relu=0, x=P, e=P, y=P, rowptr=P):
    return "gnn_espmm", (rowptr, rowptr, rowptr, rowptr, x, e, y, n, F, ldx, lde, ldy, t, op, relu, 0)


def egrad(n=5, F=16, lddy=16, ldx=16, lde=16, ldde=16, t=1, op=0, relu=0, dy=P, x=P, e=P, de=P, dval=P, rowptr=P):
    return "gnn_egrad", (rowptr, rowptr, rowptr, dy, x, e, de, dval, n, F, lddy, ldx, lde, ldde, t, op, relu, 0)


def spmm(n=5, F=16, ldx=16, ldy=16, xt=1, yt=1, cscale=0, ptr=P, short_rows=0):
    return "gnn_spmm", (ptr, ptr, ptr, ptr, 0, 0, n, F, ldx, ldy, xt, yt, 0, -1, 0, 0, 0, cscale, -1, short_rows)


# the (input, output) pairs wspmm and pool_bwd compile: the others of 0..2 x 0..2 are not
PAIRS = {(1, 1), (1, 0), (2, 2), (2, 0), (0, 0)}
NOT_PAIRS = sorted({(a, b) for a in range(3) for b in range(3)} - PAIRS) + [(3, 3), (-1, 0), (1, 3)]
# spmm compiles (0, 1) and (0, 2) as well, and only the same-type pairs with a column scale
SPMM_NOT_PAIRS = [(1, 2), (2, 1), (3, 3), (-1, 0), (0, 3)]
SPMM_NOT_PAIRS_CS = [(1, 0), (0, 1), (2, 0), (0, 2), (1, 2), (2, 1), (3, 3)]
BAD_TYPES = [3, -1]

TABLE = [
    # ---------------------------------------------------------------- wspmm
    ("wspmm ldx % 8", wspmm(F=12, ldx=12), -3),
    ("wspmm ldy % 8", wspmm(F=12, ldy=12), -3),
    ("wspmm F > ldx", wspmm(F=17, ldy=24), -3),
    ("wspmm F > ldy", wspmm(F=17, ldx=24), -3),
    ("wspmm F < 0", wspmm(F=-8), -3),
    ("wspmm ldx = 0", wspmm(F=0, ldx=0), -3),
    ("wspmm ldy = 0", wspmm(F=0, ldy=0), -3),
    ("wspmm ldy < 0", wspmm(F=-8, ldx=-8, ldy=-8), -3),
    ("wspmm F = 0 is a shape", wspmm(n=0, F=0), OK),
    ("wspmm stride before type", wspmm(ldx=12, xt=0, yt=1), -3),
    ("wspmm type before the zero-row return", wspmm(n=0, xt=0, yt=1), -5),
    ("wspmm stride with zero rows", wspmm(n=0, ldy=12), -3),
    ("wspmm zero rows, null pointers", wspmm(n=0, ptr=0), OK),
    ("wspmm negative rows, null pointers", wspmm(n=-1, ptr=0), OK),
    ("wspmm zero rows, two slabs", wspmm(n=0, F=1030, ldx=1032, ldy=1032, ptr=0), OK),
] + [("wspmm pair %r" % (p,), wspmm(xt=p[0], yt=p[1]), -5) for p in NOT_PAIRS] + [
    ("wspmm pair %r, zero rows" % (p,), wspmm(n=0, xt=p[0], yt=p[1], ptr=0), OK) for p in sorted(PAIRS)
] + [
    # ---------------------------------------------------------------- sddmm
    ("sddmm lda % 8", sddmm(F=12, lda=12), -3),
    ("sddmm ldb % 8", sddmm(F=12, ldb=12), -3),
    ("sddmm F > lda", sddmm(F=17, ldb=24), -3),
    ("sddmm F > ldb", sddmm(F=17, lda=24), -3),
    ("sddmm F = 0", sddmm(F=0), -3),
    ("sddmm F = 0, zero rows", sddmm(n=0, F=0), -3),
    ("sddmm F < 0", sddmm(F=-8), -3),
    ("sddmm lda = 0", sddmm(F=0, lda=0), -3),
    ("sddmm stride before type", sddmm(ldb=12, t=3), -3),
    ("sddmm type before the zero-row return", sddmm(n=0, t=3), -5),
    ("sddmm zero rows, null pointers", sddmm(n=0, ptr=0), OK),
    ("sddmm zero rows, three slabs", sddmm(n=0, F=1030, lda=1032, ldb=1032, ptr=0), OK),
] + [("sddmm type %d" % t, sddmm(t=t), -5) for t in BAD_TYPES] + [
    ("sddmm type %d, zero rows" % t, sddmm(n=0, t=t, ptr=0), OK) for t in range(3)
] + [
    # ---------------------------------------------------------------- pool_fwd
    ("pool_fwd ldx % 8", pool_fwd(F=12, ldx=12), -3),
    ("pool_fwd ldy % 8", pool_fwd(F=12, ldy=12), -3),
    ("pool_fwd ldarg % 8", pool_fwd(F=12, ldarg=12), -3),
    ("pool_fwd F > ldx", pool_fwd(F=17, ldy=24, ldarg=24), -3),
    ("pool_fwd F > ldy", pool_fwd(F=17, ldx=24, ldarg=24), -3),
    ("pool_fwd F > ldarg", pool_fwd(F=17, ldx=24, ldy=24), -3),
    ("pool_fwd F < 0", pool_fwd(F=-8), -3),
    ("pool_fwd ldx = 0", pool_fwd(F=0, ldx=0), -3),
    ("pool_fwd ldy = 0", pool_fwd(F=0, ldy=0), -3),
    ("pool_fwd ldarg = 0", pool_fwd(F=0, ldarg=0), -3),
    ("pool_fwd ldarg ignored without arg", pool_fwd(n=0, ldarg=12, arg=0), OK),
    ("pool_fwd ldarg = 0 without arg", pool_fwd(n=0, ldarg=0, arg=0), OK),
    ("pool_fwd stride before type", pool_fwd(ldx=12, t=3), -3),
    ("pool_fwd type before the zero-row return", pool_fwd(n=0, t=3), -5),
    ("pool_fwd type before the null pointers", pool_fwd(t=3, rowptr=0, x=0, y=0), -5),
    ("pool_fwd zero rows before the null pointers", pool_fwd(n=0, rowptr=0, x=0, y=0, arg=0), OK),
    ("pool_fwd negative rows, null pointers", pool_fwd(n=-1, rowptr=0, x=0, y=0, arg=0), OK),
    ("pool_fwd null rowptr", pool_fwd(rowptr=0), -3),
    ("pool_fwd null X", pool_fwd(x=0), -3),
    ("pool_fwd null Y", pool_fwd(y=0), -3),
    ("pool_fwd null Y, min", pool_fwd(y=0, is_min=1), -3),
    ("pool_fwd zero rows, arg wider than a slab", pool_fwd(n=0, F=8, ldx=8, ldy=8, ldarg=520), OK),
] + [("pool_fwd type %d" % t, pool_fwd(t=t), -5) for t in BAD_TYPES] + [
    ("pool_fwd type %d, zero rows" % t, pool_fwd(n=0, t=t), OK) for t in range(3)
] + [
    # ---------------------------------------------------------------- pool_bwd
    ("pool_bwd ldarg % 8", pool_bwd(F=12, ldarg=12), -3),
    ("pool_bwd lddy % 8", pool_bwd(F=12, lddy=12), -3),
    ("pool_bwd lddx % 8", pool_bwd(F=12, lddx=12), -3),
    ("pool_bwd F > ldarg", pool_bwd(F=17, lddy=24, lddx=24), -3),
    ("pool_bwd F > lddy", pool_bwd(F=17, ldarg=24, lddx=24), -3),
    ("pool_bwd F > lddx", pool_bwd(F=17, ldarg=24, lddy=24), -3),
    ("pool_bwd F < 0", pool_bwd(F=-8), -3),
    ("pool_bwd ldarg = 0", pool_bwd(F=0, ldarg=0), -3),
    ("pool_bwd lddy = 0", pool_bwd(F=0, lddy=0), -3),
    ("pool_bwd lddx = 0", pool_bwd(F=0, lddx=0), -3),
    ("pool_bwd stride before type", pool_bwd(lddx=12, tdy=0, tdx=1), -3),
    ("pool_bwd type before the zero-row return", pool_bwd(n=0, tdy=0, tdx=1), -5),
    ("pool_bwd type before the null pointers", pool_bwd(tdy=0, tdx=1, rowptr=0, arg=0, dy=0, dx=0), -5),
    ("pool_bwd zero rows before the null pointers", pool_bwd(n=0, rowptr=0, arg=0, dy=0, dx=0), OK),
    ("pool_bwd null rowptr", pool_bwd(rowptr=0), -3),
    ("pool_bwd null arg", pool_bwd(arg=0), -3),
    ("pool_bwd null dY", pool_bwd(dy=0), -3),
    ("pool_bwd null dX", pool_bwd(dx=0), -3),
    ("pool_bwd zero rows, three slabs", pool_bwd(n=0, F=1030, ldarg=1032, lddy=1032, lddx=1032), OK),
] + [("pool_bwd pair %r" % (p,), pool_bwd(tdy=p[0], tdx=p[1]), -5) for p in NOT_PAIRS] + [
    ("pool_bwd pair %r, zero rows" % (p,), pool_bwd(n=0, tdy=p[0], tdx=p[1]), OK) for p in sorted(PAIRS)
] + [
    # ---------------------------------------------------------------- espmm
    ("espmm ldx % 8", espmm(F=12, ldx=12), -3),
    ("espmm lde % 8", espmm(F=12, lde=12), -3),
    ("espmm ldy % 8", espmm(F=12, ldy=12), -3),
    ("espmm F > ldx", espmm(F=17, lde=24, ldy=24), -3),
    ("espmm F > lde", espmm(F=17, ldx=24, ldy=24), -3),
    ("espmm F > ldy", espmm(F=17, ldx=24, lde=24), -3),
    ("espmm F < 0", espmm(F=-8), -3),
    ("espmm ldx = 0", espmm(F=0, ldx=0), -3),
    ("espmm lde = 0", espmm(F=0, lde=0), -3),
    ("espmm ldy = 0", espmm(F=0, ldy=0), -3),
    ("espmm ldx ignored without X", espmm(n=0, ldx=12, x=0), OK),
    ("espmm ldx = 0 without X", espmm(n=0, ldx=0, x=0), OK),
    ("espmm null E", espmm(e=0), -3),
    ("espmm null Y", espmm(y=0), -3),
    ("espmm null E and Y with zero rows", espmm(n=0, e=0, y=0), -3),
    ("espmm relu with mul", espmm(op=1, relu=1), -3),
    ("espmm relu with mul, zero rows", espmm(n=0, op=1, relu=1), -3),
    ("espmm relu with mul, without X", espmm(op=1, relu=1, x=0), -3),
    ("espmm relu with mul before the type", espmm(op=1, relu=1, t=3), -3),
    ("espmm stride before type", espmm(lde=12, t=3), -3),
    ("espmm type before a bad op", espmm(t=3, op=2), -5),
    ("espmm bad op 2", espmm(op=2), -1),
    ("espmm bad op -1", espmm(op=-1), -1),
    ("espmm bad op with relu", espmm(op=2, relu=1), -1),
    ("espmm bad op without X", espmm(op=2, x=0), -1),
    ("espmm bad op before the zero-row return", espmm(n=0, op=2), -1),
    ("espmm type before the zero-row return", espmm(n=0, t=3), -5),
    ("espmm zero rows, null graph", espmm(n=0, rowptr=0, x=0), OK),
    ("espmm negative rows, null graph", espmm(n=-1, rowptr=0, x=0), OK),
    ("espmm zero rows, mul", espmm(n=0, op=1), OK),
    ("espmm zero rows, three slabs", espmm(n=0, F=1030, ldx=1032, lde=1032, ldy=1032), OK),
] + [("espmm type %d" % t, espmm(t=t), -5) for t in BAD_TYPES] + [
    ("espmm type %d, zero rows" % t, espmm(n=0, t=t), OK) for t in range(3)
] + [
    # ---------------------------------------------------------------- egrad
    ("egrad lddy % 8", egrad(F=12, lddy=12), -3),
    ("egrad ldx % 8", egrad(F=12, ldx=12), -3),
    ("egrad lde % 8", egrad(F=12, lde=12), -3),
    ("egrad ldde % 8", egrad(F=12, ldde=12), -3),
    ("egrad F > lddy", egrad(F=17, ldx=24, lde=24, ldde=24), -3),
    ("egrad F > ldx", egrad(F=17, lddy=24, lde=24, ldde=24), -3),
    ("egrad F > lde", egrad(F=17, lddy=24, ldx=24, ldde=24), -3),
    ("egrad F > ldde", egrad(F=17, lddy=24, ldx=24, lde=24), -3),
    ("egrad F < 0", egrad(F=-8), -3),
    ("egrad lddy = 0", egrad(F=0, lddy=0), -3),
    ("egrad ldx = 0", egrad(F=0, ldx=0), -3),
    ("egrad lde = 0", egrad(F=0, lde=0), -3),
    ("egrad ldde = 0", egrad(F=0, ldde=0), -3),
    ("egrad ldx ignored without X", egrad(n=0, ldx=12, x=0), OK),
    ("egrad ldde ignored without dE", egrad(n=0, ldde=12, de=0), OK),
    ("egrad ldde = 0 without dE", egrad(n=0, ldde=0, de=0), OK),
    ("egrad both outputs null", egrad(de=0, dval=0), -3),
    ("egrad both outputs null, zero rows", egrad(n=0, de=0, dval=0), -3),
    ("egrad dE alone", egrad(n=0, dval=0), OK),
    ("egrad dval alone", egrad(n=0, de=0), OK),
    ("egrad null dY", egrad(dy=0), -3),
    ("egrad null E", egrad(e=0), -3),
    ("egrad relu with mul", egrad(op=1, relu=1), -3),
    ("egrad relu with mul, without X", egrad(op=1, relu=1, x=0), -3),
    ("egrad relu with mul before the type", egrad(op=1, relu=1, t=3), -3),
    ("egrad stride before type", egrad(lde=12, t=3), -3),
    ("egrad type before a bad op", egrad(t=3, op=2), -5),
    ("egrad bad op 2", egrad(op=2), -1),
    ("egrad bad op -1", egrad(op=-1), -1),
    ("egrad bad op before the zero-row return", egrad(n=0, op=2), -1),
    ("egrad type before the zero-row return", egrad(n=0, t=3), -5),
    ("egrad zero rows, null graph", egrad(n=0, rowptr=0, x=0), OK),
    ("egrad zero rows, dE wider than a slab", egrad(n=0, F=8, lddy=8, ldx=8, lde=8, ldde=520), OK),
    ("egrad zero rows, three slabs", egrad(n=0, F=1030, lddy=1032, ldx=1032, lde=1032, ldde=1032), OK),
] + [("egrad type %d" % t, egrad(t=t), -5) for t in BAD_TYPES] + [
    ("egrad type %d, zero rows" % t, egrad(n=0, t=t), OK) for t in range(3)
] + [
    # ---------------------------------------------------------------- spmm
    # the oldest of these launchers: it rejects neither ld <= 0 nor F < 0, and its zero-row
    # return comes after the stride check but BEFORE the type check
    ("spmm ldx % 8", spmm(F=12, ldx=12), -3),
    ("spmm ldy % 8", spmm(F=12, ldy=12), -3),
    ("spmm F > ldx", spmm(F=17, ldy=24), -3),
    ("spmm F > ldy", spmm(F=17, ldx=24), -3),
    ("spmm stride before the zero-row return", spmm(n=0, ldy=12), -3),
    ("spmm stride before type", spmm(ldx=12, xt=1, yt=2), -3),
    ("spmm F < 0 passes the shape check", spmm(F=-8, xt=1, yt=2), -5),
    ("spmm F < 0, zero rows", spmm(n=0, F=-8), OK),
    ("spmm ld = 0 passes the shape check", spmm(F=0, ldx=0, ldy=0, xt=1, yt=2), -5),
    ("spmm ld = 0, zero rows", spmm(n=0, F=0, ldx=0, ldy=0), OK),
    ("spmm ld < 0 passes the shape check", spmm(F=-16, ldx=-8, ldy=-8, xt=1, yt=2), -5),
    ("spmm zero rows before the type", spmm(n=0, xt=1, yt=2), OK),
    ("spmm zero rows before the type, short rows", spmm(n=0, xt=3, yt=3, short_rows=1), OK),
    ("spmm negative rows, null pointers", spmm(n=-1, ptr=0), OK),
    ("spmm zero rows, null pointers", spmm(n=0, ptr=0), OK),
    ("spmm zero rows, three slabs", spmm(n=0, F=1030, ldx=1032, ldy=1032, ptr=0), OK),
    ("spmm bad pair, three slabs", spmm(F=1030, ldx=1032, ldy=1032, xt=1, yt=2), -5),
    ("spmm bad pair, short rows", spmm(xt=1, yt=2, short_rows=1), -5),
] + [("spmm pair %r" % (p,), spmm(xt=p[0], yt=p[1]), -5) for p in SPMM_NOT_PAIRS] + [
    ("spmm pair %r with a column scale" % (p,), spmm(xt=p[0], yt=p[1], cscale=P), -5) for p in SPMM_NOT_PAIRS_CS
]


def test_the_table_names_every_launcher_and_case_once():
    ids = [t[0] for t in TABLE]
    assert len(set(ids)) == len(ids)
    assert {t[1][0] for t in TABLE} == {"gnn_wspmm", "gnn_sddmm", "gnn_pool_fwd", "gnn_pool_bwd", "gnn_espmm",
                                        "gnn_egrad", "gnn_spmm"}


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
