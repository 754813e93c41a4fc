"""The oracle of tests/test_sampler_exact_gpu.py and its own checks, run without a GPU.

``ref_blocks`` is a NumPy model of the mini-batch sampling pipeline (gnn_sampler.hip:
``sample_neighbors_kernel`` and the ``sb_*`` kernels behind ``gnn_sample_blocks``).  It shares
no code with ``DeviceSampler``, ``sample_reference`` or ``transpose_csr``: rows with
``deg <= fanout`` are copied by index arithmetic, the Philox / Floyd twin runs over all the
other rows at once (one vector step per pick), new sources come from a boolean mark array,
the transposed CSR from a stable argsort.

What is checked here:

* the oracle equals ``sampler.sample_reference`` (the per-row Python twin) on small cases,
  and every field agrees with the dense 0/1 adjacency of the block;
* Floyd's algorithm itself, which an oracle that shares it cannot check: distinct positions
  in range, and inclusion counts within 4.5 standard deviations of uniform, for six
  (degree, fanout) pairs;
* ``gnn_sample_flag_bytes`` and ``gnn_sample_blocks_scratch`` against what the launcher
  indexes;
* every refusal of ``gnn_sample_blocks`` and ``gnn_sample_neighbors``, which happen before
  the first HIP call and so need no device (dummy pointers, never dereferenced).
"""
import re

import numpy as np
import pytest

from cgnn_amd import native
from cgnn_amd.gnn import sampler
from cgnn_amd.utils import philox
from cgnn_amd.utils.philox import model_key

SALT = 0x10000001             # salt * 16 + level wraps in 32 bits
SEED = 3
FLAG_BLK = 4096               # ids per flag block
SB = 1024                     # elements per scan block


# ---------------------------------------------------------------------------- graphs
def csr(rows, n=None):
    """CSR (int32 rowptr, col) of a list of neighbour lists."""
    n = len(rows) if n is None else n
    deg = np.zeros(n, dtype=np.int64)
    deg[:len(rows)] = [len(r) for r in rows]
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = np.asarray([c for r in rows for c in r], dtype=np.int32)
    return rowptr, col


def ring(n):
    """Every node v has the row [v - 1, v + 1] (mod n)."""
    v = np.arange(n, dtype=np.int64)
    col = np.stack([(v - 1) % n, (v + 1) % n], 1).reshape(-1).astype(np.int32)
    return (2 * np.arange(n + 1, dtype=np.int64)).astype(np.int32), col


def random_graph(n, degs, rng):
    """Row v has degs[v] columns drawn with replacement from [0, n): self-loops and
    repeated columns occur."""
    degs = np.asarray(degs, dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int32)
    return rowptr, rng.integers(0, n, int(rowptr[-1])).astype(np.int32)


# ---------------------------------------------------------------------------- the oracle
def floyd_positions(v, deg, fo, lsalt, k0, k1):
    """Floyd's ``fo`` distinct positions in [0, deg) for every row (v[r], deg[r] > fo), in the
    order they are drawn: an (R, fo) int64 array.  Step m draws t uniform in [0, j] for
    j = deg - fo + m from word m % 4 of Philox counter (v, lsalt, m // 4, RNG_SAMPLE) and
    keeps t, or j when t was drawn before."""
    v = np.asarray(v, dtype=np.int64)
    deg = np.asarray(deg, dtype=np.int64)
    assert v.shape == deg.shape and bool((deg > fo).all()) and fo >= 1
    R = v.size
    words = np.empty((R, 4 * ((fo + 3) // 4)), dtype=np.uint64)
    for c in range((fo + 3) // 4):
        w = philox.philox4x32_10(v.astype(np.uint32), np.uint32(lsalt), np.uint32(c), np.uint32(philox.RNG_SAMPLE),
                                 k0, k1)
        for q in range(4):
            words[:, 4 * c + q] = w[q]
    sel = np.empty((R, fo), dtype=np.int64)
    for m in range(fo):
        j = deg - fo + m
        t = ((words[:, m] * (j + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        dup = (sel[:, :m] == t[:, None]).any(1)
        sel[:, m] = np.where(dup, j, t)
    return sel


def ref_sample(rowptr, col, nodes, fo, lsalt, k0, k1):
    """One level's picks: (optr int32 [nd + 1], global picks int32 [total]); ``fo < 0``
    copies whole rows."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    nodes = np.asarray(nodes, dtype=np.int64)
    start = rowptr[nodes]
    deg = rowptr[nodes + 1] - start
    cnt = deg if fo < 0 else np.minimum(deg, fo)
    optr = np.concatenate([[0], np.cumsum(cnt)])
    total = int(optr[-1])
    # position within the row of every pick: 0, 1, .. for the copied rows
    pos = np.arange(total, dtype=np.int64) - np.repeat(optr[:-1], cnt)
    if fo >= 0:
        fl = np.nonzero(deg > fo)[0]
        if fl.size:
            sel = floyd_positions(nodes[fl], deg[fl], fo, lsalt, k0, k1)
            pos[(optr[fl][:, None] + np.arange(fo)[None, :]).reshape(-1)] = sel.reshape(-1)
    picks = np.asarray(col)[np.repeat(start, cnt) + pos]
    return optr.astype(np.int32), picks.astype(np.int32)


def level_salt(salt, level):
    return (int(salt) * 16 + level) & 0xFFFFFFFF


def ref_blocks(rowptr, col, seeds, fanouts, salt, seed, need_t):
    """Per level (seeds outwards) a dict: optr, inv_deg, picks (global), local, src, n_src,
    total and, where need_t[l], rp_t / col_t."""
    k0, k1 = model_key(seed, "neighbour-sampler")
    n = len(rowptr) - 1
    nodes = np.asarray(seeds, dtype=np.int64)
    out = []
    for l, fo in enumerate(fanouts):
        nd = nodes.size
        optr, picks = ref_sample(rowptr, col, nodes, fo, level_salt(salt, l), k0, k1)
        cnt = np.diff(optr)
        inv = np.zeros(nd, dtype=np.float32)
        inv[cnt > 0] = np.float32(1) / cnt[cnt > 0].astype(np.float32)
        mark = np.zeros(n, dtype=bool)
        mark[picks] = True
        mark[nodes] = False
        new = np.nonzero(mark)[0]
        src = np.concatenate([nodes, new])
        lid = np.full(n, -1, dtype=np.int64)
        lid[src] = np.arange(src.size)
        local = lid[picks]
        b = dict(optr=optr, inv_deg=inv, picks=picks, local=local.astype(np.int32), src=src.astype(np.int32),
                 n_src=int(src.size), total=int(optr[-1]))
        if need_t[l]:
            order = np.argsort(local, kind="stable")
            dst = np.repeat(np.arange(nd), cnt)
            b["col_t"] = dst[order].astype(np.int32)
            b["rp_t"] = np.concatenate([[0], np.cumsum(np.bincount(local, minlength=src.size))]).astype(np.int32)
        out.append(b)
        nodes = src
    return out


def slot_bounds(n, n_seeds_max, fanouts):
    """Upper bounds of a batch: per level (nd_max, smax = bound of its sources)."""
    nd, out = max(int(n_seeds_max), 1), []
    for fo in fanouts:
        out.append((nd, min(nd * (fo + 1), n)))
        nd = out[-1][1]
    return out


# ---------------------------------------------------------------------------- oracle checks
def small_cases():
    rng = np.random.default_rng(7)
    n = 90
    degs = rng.integers(0, 30, n)
    degs[[0, 17, 89]] = [0, 70, 1]
    g = random_graph(n, degs, rng)
    yield "random 5-3", g, rng.permutation(n)[:20], [5, 3]
    yield "random 16-17", g, rng.permutation(n)[:9], [16, 17]
    yield "random 64-1", g, np.asarray([17, 89, 0, 3]), [64, 1]
    yield "no seeds", g, np.zeros(0, dtype=np.int64), [4, 4]
    yield "all seeds descending", g, np.arange(n)[::-1], [2, 7]
    loops = csr([[0, 0, 1], [1], [], [2, 0, 2, 0, 3, 3, 3], [4]])
    yield "loops and multi-edges", loops, np.asarray([3, 0, 2]), [3, 2]


@pytest.mark.parametrize("name,g,seeds,fanouts", [pytest.param(*c, id=c[0]) for c in small_cases()])
def test_oracle_matches_the_python_twin_and_the_dense_adjacency(name, g, seeds, fanouts):
    rowptr, col = g
    n = len(rowptr) - 1
    got = ref_blocks(rowptr, col, seeds, fanouts, SALT, SEED, [True] * len(fanouts))
    twin = sampler.sample_reference(rowptr, col, seeds, fanouts, SALT, seed=SEED)
    nodes = np.asarray(seeds, dtype=np.int64)
    for l, (b, (rp, loc, src)) in enumerate(zip(got, twin)):
        fo, nd = fanouts[l], nodes.size
        assert np.array_equal(b["optr"], rp) and np.array_equal(b["local"], loc) and np.array_equal(b["src"], src)
        assert b["n_src"] == len(src) and b["total"] == rp[-1] == len(b["picks"])
        # sources: the destinations first, then the new ones, increasing and distinct
        assert np.array_equal(b["src"][:nd], nodes) and len(set(b["src"].tolist())) == b["n_src"] <= n
        new = b["src"][nd:]
        assert bool((np.diff(new) > 0).all())
        assert set(new.tolist()) == set(b["picks"].tolist()) - set(nodes.tolist())
        assert np.array_equal(b["src"][b["local"]], b["picks"])
        # dense adjacency (entry = multiplicity) of the block, and the rows of the graph
        A = np.zeros((nd, b["n_src"]), dtype=np.int64)
        for i in range(nd):
            row = col[rowptr[nodes[i]]:rowptr[nodes[i] + 1]].tolist()
            mine = b["picks"][b["optr"][i]:b["optr"][i + 1]].tolist()
            assert len(mine) == min(len(row), fo)
            if len(row) <= fo:
                assert mine == row
            else:                                   # a sub-multiset of the row
                assert all(mine.count(c) <= row.count(c) for c in set(mine))
            np.add.at(A[i], b["local"][b["optr"][i]:b["optr"][i + 1]], 1)
            want = np.float32(1) / np.float32(len(mine)) if mine else np.float32(0)
            assert b["inv_deg"][i] == want and b["inv_deg"].dtype == np.float32
        assert A.sum() == b["total"]
        # the transposed CSR is A^T with every bucket in increasing destination order
        T = np.zeros((b["n_src"], nd), dtype=np.int64)
        assert b["rp_t"][0] == 0 and b["rp_t"][-1] == b["total"] and len(b["rp_t"]) == b["n_src"] + 1
        for c in range(b["n_src"]):
            bucket = b["col_t"][b["rp_t"][c]:b["rp_t"][c + 1]]
            assert bool((np.diff(bucket) >= 0).all())
            np.add.at(T[c], bucket, 1)
        assert np.array_equal(T, A.T)
        nodes = b["src"].astype(np.int64)


def test_oracle_whole_row_copy_and_need_t_off():
    rowptr, col = csr([[1, 2, 2], [], [0]])
    k0, k1 = model_key(SEED, "neighbour-sampler")
    optr, picks = ref_sample(rowptr, col, [2, 0, 1], -1, 5, k0, k1)
    assert optr.tolist() == [0, 1, 4, 4] and picks.tolist() == [0, 1, 2, 2]
    b = ref_blocks(rowptr, col, [0], [1, 2], SALT, SEED, [False, True])
    assert "rp_t" not in b[0] and "rp_t" in b[1]
    assert level_salt(SALT, 1) == 0x11 and level_salt(SALT, 0) == 0x10


# Floyd's algorithm, checked alone: (deg, fanout, N).  The bound is a condition on the
# sampler, 4.5 standard deviations of a binomial count; the largest deviations measured are
# 2.62, 2.29, 2.29, 3.01, 2.43 and 0.85 sd.
FLOYD_CASES = [(12, 5, 4096), (23, 16, 4096), (24, 17, 4096), (80, 64, 2048), (65, 64, 2048), (3, 1, 4096)]


@pytest.mark.parametrize("deg,fo,N", FLOYD_CASES)
def test_floyd_positions_are_distinct_and_uniform(deg, fo, N):
    k0, k1 = model_key(3, "neighbour-sampler")
    lsalt = level_salt(11, 0)
    v = np.arange(N)
    sel = floyd_positions(v, np.full(N, deg), fo, lsalt, k0, k1)
    assert sel.shape == (N, fo) and sel.min() >= 0 and sel.max() < deg
    assert bool((np.diff(np.sort(sel, 1), axis=1) > 0).all())
    # the same positions from the per-row Python twin, through a graph whose column ids are
    # the positions (every 64th row: the twin is slow)
    sub = v[::64]
    rowptr = deg * np.arange(N + 1)
    twin = sampler.sample_reference(rowptr, np.tile(np.arange(deg), N), sub, [fo], 11, seed=3)
    rp, loc, src = twin[0]
    assert np.array_equal(rp, fo * np.arange(len(sub) + 1)) and np.array_equal(src[loc], sel[::64].reshape(-1))
    p = fo / deg
    sd = np.sqrt(N * p * (1 - p))
    dev = np.abs(np.bincount(sel.reshape(-1), minlength=deg) - N * p) / sd
    print("deg %d fanout %d N %d: largest deviation %.2f sd" % (deg, fo, N, dev.max()))
    assert dev.max() <= 4.5


# ---------------------------------------------------------------------------- buffer sizes
@pytest.mark.parametrize("n", [1, 4095, 4096, 4097])
def test_flag_bytes_are_whole_blocks_beyond_n(n):
    b = native.hip().gnn_sample_flag_bytes(n)
    assert b % FLAG_BLK == 0 and b > n and b - n <= FLAG_BLK
    assert b >= FLAG_BLK * ((n + FLAG_BLK - 1) // FLAG_BLK)      # every block the flag passes read


@pytest.mark.parametrize("n,batch,fanouts", [
    (1, 1, [1]), (5, 1, [64]), (4096, 1024, [15, 10, 5]), (4097, 1025, [1, 1]), (300000, 262145, [2]),
    (2449029, 1024, [15, 10, 5]), (1052673, 8, [2, 2]), (6000, 4099, [3, 2]), (50, 50, [64, 64]), (7, 1024, [3])])
def test_scratch_covers_what_the_launcher_indexes(n, batch, fanouts):
    bounds = slot_bounds(n, batch, fanouts)
    got = native.hip().gnn_sample_blocks_scratch(n, fanouts, [b[0] for b in bounds])
    nb = (n + FLAG_BLK - 1) // FLAG_BLK                              # one count per flag block
    # a scan of m values (m <= n: the ids are distinct) touches m + 0 values and ceil(m / SB)
    # block sums; the scans are over the destinations and, transposed, over the sources
    longest = max(max(min(nd, n), smax) for nd, smax in bounds)
    assert got >= nb + max(1, (longest + SB - 1) // SB) + longest
    # growing any bound never shrinks it
    assert native.hip().gnn_sample_blocks_scratch(n, fanouts, [b[0] + 1 for b in bounds]) >= got


# ---------------------------------------------------------------------------- refusals
P = 64                        # a non-null pointer; never dereferenced
OK = None


def blocks_call(n=100, n_seeds=4, fan=(5, 3), nd_max=(8, 48), ptr=P):
    L = len(fan)
    return "gnn_sample_blocks", (ptr, ptr, n, ptr, n_seeds, list(fan), list(nd_max)) + ([ptr] * L,) * 8 + (
        ptr, ptr, ptr, ptr, 1, 2, SALT, 0)


def neigh_call(n=5, fanout=5, ptr=P):
    return "gnn_sample_neighbors", (ptr, ptr, ptr, n, fanout, ptr, ptr, 1, 2, SALT, 0)


REFUSALS = [
    ("blocks fanout over 64 at level 1", blocks_call(fan=(5, 70)), -3),
    ("blocks fanout over 64 at level 0", blocks_call(fan=(65, 3)), -3),
    ("blocks fanout 0", blocks_call(fan=(0,), nd_max=(8,)), -3),
    ("blocks fanout 0 at the last level", blocks_call(fan=(5, 0)), -3),
    ("blocks fanout -1", blocks_call(fan=(-1,), nd_max=(8,)), -3),
    ("blocks no level", blocks_call(fan=(), nd_max=()), -3),
    ("blocks n = 0", blocks_call(n=0), -3),
    ("blocks n < 0", blocks_call(n=-5), -3),
    ("blocks n_seeds < 0", blocks_call(n_seeds=-1), -3),
    ("blocks n_seeds over nd_max[0]", blocks_call(n_seeds=9), -3),
    ("blocks nd_max[0] = 0", blocks_call(n_seeds=0, nd_max=(0, 48)), -3),
    ("blocks nd_max[1] = 0", blocks_call(nd_max=(8, 0)), -3),
    ("blocks nd_max < 0", blocks_call(nd_max=(8, -48)), -3),
    ("blocks null pointers, bad fanout", blocks_call(fan=(5, 70), ptr=0), -3),
    ("neighbors fanout 65", neigh_call(fanout=65), -3),
    ("neighbors fanout 65 before the zero-row return", neigh_call(n=0, fanout=65, ptr=0), -3),
    ("neighbors fanout 65, negative rows", neigh_call(n=-1, fanout=65, ptr=0), -3),
    ("neighbors zero rows", neigh_call(n=0, ptr=0), OK),
    ("neighbors zero rows, fanout 64", neigh_call(n=0, fanout=64, ptr=0), OK),
    ("neighbors zero rows, fanout 0", neigh_call(n=0, fanout=0, ptr=0), OK),
    ("neighbors zero rows, whole-row copy", neigh_call(n=0, fanout=-1, ptr=0), OK),
    ("neighbors negative rows", neigh_call(n=-3, ptr=0), OK),
]


def test_refusal_ids_are_unique():
    assert len({r[0] for r in REFUSALS}) == len(REFUSALS)


@pytest.mark.parametrize("call,code", [pytest.param(c, code, id=i) for i, c, code in REFUSALS])
def test_refusal_happens_before_any_hip_call(call, code):
    name, args = call
    fn = getattr(native.hip(), name)
    if code is OK:
        fn(*args)
        return
    with pytest.raises(RuntimeError) as err:
        fn(*args)
    assert re.search(r"\(code %d\)" % code, str(err.value)), str(err.value)


def test_per_level_lists_of_unequal_length_are_refused():
    name, args = blocks_call()
    args = list(args)
    args[7] = [P]                     # optr: one entry for two levels
    with pytest.raises(RuntimeError, match="differ in length"):
        native.hip().gnn_sample_blocks(*args)
