"""Return codes of the graph-readout launchers (gnn_readout.hip: gnn_launch_seg_reduce,
gnn_launch_seg_bcast), pinned without a GPU, in the form of test_gnn_launch_codes_cpu.py.

Every rejection and every zero-row return happens before the first HIP call: pointers are 0
or a dummy non-null integer that is never dereferenced.  The ORDER of the checks is API
(cgnn_api.h): strides (-3), the element-type pair (-5), the zero-row return, the required
pointers (-3), the op code (-1).  A row of the table is (id, (binding, arguments), code), code
``None`` meaning that the call returns normally.  No row reaches a launch.
"""
import re

import pytest

from cgnn_amd import native

P = 64                  # a non-null pointer; never dereferenced
OK = None
SUM, MAX, MIN = 0, 1, 2


def reduce(S=5, F=16, ldx=16, ldy=16, lda_in=16, lda=16, tin=1, tout=1, op=SUM, ptr=P, x=P, y=P, rscale=0, arg_in=0,
           arg=0):
    return "gnn_seg_reduce", (ptr, x, y, rscale, arg_in, arg, S, F, ldx, ldy, lda_in, lda, tin, tout, op, 0)


def bcast(n=5, F=16, ldu=16, lda=16, ldo=16, tin=1, tout=1, seg=P, u=P, rscale=0, arg=0, out=P):
    return "gnn_seg_bcast", (seg, u, rscale, arg, out, n, F, ldu, lda, ldo, tin, tout, 0)


# the sum compiles wspmm's five pairs and fp32 -> bf16 / fp16; max / min the same-type pairs
SUM_PAIRS = {(1, 1), (1, 0), (2, 2), (2, 0), (0, 0), (0, 1), (0, 2)}
SUM_NOT_PAIRS = sorted({(a, b) for a in range(3) for b in range(3)} - SUM_PAIRS) + [(3, 3), (-1, 0), (1, 3)]
BEST_NOT_PAIRS = [(1, 0), (2, 0), (0, 1), (0, 2), (1, 2), (3, 3), (-1, -1)]
BCAST_PAIRS = {(1, 1), (1, 0), (2, 2), (2, 0), (0, 0)}
BCAST_NOT_PAIRS = sorted({(a, b) for a in range(3) for b in range(3)} - BCAST_PAIRS) + [(3, 3), (-1, 0), (1, 3)]

TABLE = [
    # ---------------------------------------------------------------- seg_reduce
    ("reduce ldx % 8", reduce(F=12, ldx=12), -3),
    ("reduce ldy % 8", reduce(F=12, ldy=12), -3),
    ("reduce ldarg % 8", reduce(F=12, lda=12, op=MAX, arg=P), -3),
    ("reduce ldarg_in % 8", reduce(F=12, lda_in=12, op=MAX, arg=P, arg_in=P), -3),
    ("reduce F > ldx", reduce(F=17, ldy=24), -3),
    ("reduce F > ldy", reduce(F=17, ldx=24), -3),
    ("reduce F > ldarg", reduce(F=17, ldx=24, ldy=24, op=MIN, arg=P), -3),
    ("reduce F > ldarg_in", reduce(F=17, ldx=24, ldy=24, lda=24, op=MIN, arg=P, arg_in=P), -3),
    ("reduce F < 0", reduce(F=-8), -3),
    ("reduce ldx = 0", reduce(F=0, ldx=0), -3),
    ("reduce ldy = 0", reduce(F=0, ldy=0), -3),
    ("reduce ldarg = 0", reduce(F=0, lda=0, op=MAX, arg=P), -3),
    ("reduce ldarg ignored without arg", reduce(S=0, lda=12, op=MAX), OK),
    ("reduce ldarg_in ignored without arg_in", reduce(S=0, lda_in=12, op=MAX, arg=P), OK),
    ("reduce F = 0 is a shape", reduce(S=0, F=0), OK),
    ("reduce stride before type", reduce(ldx=12, tin=1, tout=2), -3),
    ("reduce stride before a bad op", reduce(ldy=12, op=7), -3),
    ("reduce stride with zero rows", reduce(S=0, ldy=12), -3),
    ("reduce type before the zero-row return", reduce(S=0, tin=1, tout=2), -5),
    ("reduce type before the null pointers", reduce(tin=1, tout=2, ptr=0, x=0, y=0), -5),
    ("reduce type before a bad op", reduce(tin=1, tout=2, op=3), -5),
    ("reduce max type before the zero-row return", reduce(S=0, tin=1, tout=0, op=MAX), -5),
    ("reduce zero rows before the null pointers", reduce(S=0, ptr=0, x=0, y=0), OK),
    ("reduce negative rows, null pointers", reduce(S=-1, ptr=0, x=0, y=0), OK),
    ("reduce zero rows before a bad op", reduce(S=0, op=3), OK),
    ("reduce zero rows, max with arg", reduce(S=0, op=MAX, arg=P, arg_in=P), OK),
    ("reduce zero rows, three slabs", reduce(S=0, F=1030, ldx=1032, ldy=1032), OK),
    ("reduce zero rows, arg wider than a slab", reduce(S=0, F=8, ldx=8, ldy=8, lda=520, op=MIN, arg=P), OK),
    ("reduce null ptr", reduce(ptr=0), -3),
    ("reduce null Y", reduce(y=0), -3),
    ("reduce null Y, max", reduce(y=0, op=MAX), -3),
    ("reduce null ptr before a bad op", reduce(ptr=0, op=3), -3),
    ("reduce null Y before a bad op", reduce(y=0, op=-1), -3),
    ("reduce bad op 3", reduce(op=3), -1),
    ("reduce bad op -1", reduce(op=-1), -1),
    ("reduce bad op with arg", reduce(op=3, arg=P), -1),
    ("reduce bad op, fp32 to bf16", reduce(op=3, tin=0, tout=1), -1),
] + [("reduce sum pair %r" % (p,), reduce(tin=p[0], tout=p[1]), -5) for p in SUM_NOT_PAIRS] + [
    ("reduce sum pair %r, zero rows" % (p,), reduce(S=0, tin=p[0], tout=p[1]), OK) for p in sorted(SUM_PAIRS)
] + [("reduce max pair %r" % (p,), reduce(tin=p[0], tout=p[1], op=MAX), -5) for p in BEST_NOT_PAIRS] + [
    ("reduce min pair %r" % (p,), reduce(tin=p[0], tout=p[1], op=MIN), -5) for p in BEST_NOT_PAIRS
] + [("reduce op %d type %d, zero rows" % (op, t), reduce(S=0, tin=t, tout=t, op=op), OK)
     for op in (MAX, MIN) for t in range(3)] + [
    # ---------------------------------------------------------------- seg_bcast
    ("bcast ldu % 8", bcast(F=12, ldu=12), -3),
    ("bcast ldo % 8", bcast(F=12, ldo=12), -3),
    ("bcast ldarg % 8", bcast(F=12, lda=12, arg=P), -3),
    ("bcast F > ldu", bcast(F=17, ldo=24), -3),
    ("bcast F > ldo", bcast(F=17, ldu=24), -3),
    ("bcast F > ldarg", bcast(F=17, ldu=24, ldo=24, arg=P), -3),
    ("bcast F < 0", bcast(F=-8), -3),
    ("bcast ldu = 0", bcast(F=0, ldu=0), -3),
    ("bcast ldo = 0", bcast(F=0, ldo=0), -3),
    ("bcast ldarg = 0", bcast(F=0, lda=0, arg=P), -3),
    ("bcast ldarg ignored without arg", bcast(n=0, lda=12), OK),
    ("bcast F = 0 is a shape", bcast(n=0, F=0), OK),
    ("bcast stride before type", bcast(ldo=12, tin=0, tout=1), -3),
    ("bcast stride with zero rows", bcast(n=0, ldu=12), -3),
    ("bcast type before the zero-row return", bcast(n=0, tin=0, tout=1), -5),
    ("bcast type before the null pointers", bcast(tin=0, tout=1, seg=0, u=0, out=0), -5),
    ("bcast zero rows before the null pointers", bcast(n=0, seg=0, u=0, out=0), OK),
    ("bcast negative rows, null pointers", bcast(n=-1, seg=0, u=0, out=0), OK),
    ("bcast zero rows, three slabs", bcast(n=0, F=1030, ldu=1032, lda=1032, ldo=1032, arg=P), OK),
    ("bcast null seg_id", bcast(seg=0), -3),
    ("bcast null U", bcast(u=0), -3),
    ("bcast null out", bcast(out=0), -3),
    ("bcast null out with arg", bcast(out=0, arg=P), -3),
] + [("bcast pair %r" % (p,), bcast(tin=p[0], tout=p[1]), -5) for p in BCAST_NOT_PAIRS] + [
    ("bcast pair %r, zero rows" % (p,), bcast(n=0, tin=p[0], tout=p[1]), OK) for p in sorted(BCAST_PAIRS)
]


def test_the_table_names_both_launchers_and_every_case_once():
    ids = [t[0] for t in TABLE]
    assert len(set(ids)) == len(ids)
    assert {t[1][0] for t in TABLE} == {"gnn_seg_reduce", "gnn_seg_bcast"}


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
