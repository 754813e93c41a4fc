"""The neighbour sampler and the mini-batch block pipeline (gnn_sampler.hip) against the NumPy
oracle of tests/test_sampler_exact_cpu.py, bit for bit.

Most cases drive the raw ``gnn_sample_blocks`` binding over buffers allocated here (``Rig``),
each with a sentinel tail, and compare EVERY output on its valid prefix: optr, inv_deg,
picks (in Floyd order), local, src, both counts per level, rp_t and col_t.  After every call
the flag bytes are zero over their padded length, every cnt_t is zero, what lies past a
valid prefix still holds the sentinel, and so do the tails past the documented bounds.  A few
cases go through ``PipelinedSampler`` (non-threaded, threaded) and ``DeviceSampler``.

The graphs are synthetic and as small as the path they reach allows: scan-block edges (1024
elements), more than 256 scan blocks, flag-block edges (4096 ids), more than 256 flag blocks,
both Floyd templates (fan-out <= 16, <= 64) below, at and above every degree threshold.
The default salt, 0x10000001, makes ``salt * 16 + level`` wrap in 32 bits.
"""
import numpy as np
import pytest
import torch

import test_sampler_exact_cpu as sx
from cgnn_amd import native
from cgnn_amd.gnn.sampler import DeviceSampler, PipelinedSampler
from cgnn_amd.utils.philox import model_key

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TAIL = 64                      # sentinel elements behind every buffer's documented bound
SENT = -0x5A5A5A5B             # no valid id, count or offset; as a float a large negative number
FSENT = 0xA5                   # behind the flag bytes
SALT, SEED = sx.SALT, sx.SEED


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


class Rig:
    """Device buffers of one slot at their documented bounds (as ``sampler._Slot`` sizes
    them) plus a sentinel tail each, and the shared flag / map / scratch state, which
    persists from one ``run`` to the next as it does in the pipelined sampler."""

    def __init__(self, g, fanouts, batch, need_t=None):
        rowptr, col = g
        self.n = len(rowptr) - 1
        self.rowptr, self.col = _dev(rowptr.astype(np.int32)), _dev(col.astype(np.int32))
        if self.col.numel() == 0:
            self.col = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.g = (np.asarray(rowptr), np.asarray(col))
        self.fanouts = [int(f) for f in fanouts]
        L = len(self.fanouts)
        self.need_t = [True] * L if need_t is None else list(need_t)
        self.bounds = sx.slot_bounds(self.n, batch, self.fanouts)
        self.nd_max = [b[0] for b in self.bounds]
        hip = native.hip()
        self.size = {}
        for l, (fo, (ndm, smax)) in enumerate(zip(self.fanouts, self.bounds)):
            pm = max(ndm * fo, 1)
            self.size[l] = dict(optr=ndm + 1, inv=ndm, picks=pm, local=pm, src=smax, rp_t=smax + 1, col_t=pm,
                                cnt_t=smax)
        self.fb = hip.gnn_sample_flag_bytes(self.n)
        self.flag = torch.zeros(self.fb + TAIL, dtype=torch.uint8, device=DEV)
        self.flag[self.fb:] = FSENT
        self.map = self._full(self.n + 1, 0)
        self.ns = hip.gnn_sample_blocks_scratch(self.n, self.fanouts, self.nd_max)
        self.bscratch = self._full(self.ns, 0)
        self.cnt_t = [self._full(self.size[l]["cnt_t"], 0) if self.need_t[l] else None for l in range(L)]
        self.out = None
        self.counts = None

    @staticmethod
    def _full(size, fill=SENT):
        t = torch.full((size + TAIL,), SENT, dtype=torch.int32, device=DEV)
        t[:size] = fill
        return t

    def fresh_outputs(self):
        L = len(self.fanouts)
        self.out = []
        for l in range(L):
            names = ["optr", "inv", "picks", "local", "src"] + (["rp_t", "col_t"] if self.need_t[l] else [])
            self.out.append({k: self._full(self.size[l][k]) for k in names})
        self.counts = self._full(2 * L)

    def call(self, seeds, salt=SALT, n_seeds=None, fanouts=None, nd_max=None, n=None, seed=SEED):
        """The raw binding on the current stream; ``seeds`` a device int32 tensor."""
        L = len(self.fanouts)
        p = lambda k: [self.out[l][k].data_ptr() if k in self.out[l] else 0 for l in range(L)]
        k0, k1 = model_key(seed, "neighbour-sampler")
        native.hip().gnn_sample_blocks(
            self.rowptr.data_ptr(), self.col.data_ptr(), self.n if n is None else n, seeds.data_ptr(),
            int(seeds.numel()) if n_seeds is None else n_seeds, self.fanouts if fanouts is None else fanouts,
            self.nd_max if nd_max is None else nd_max, p("optr"), p("inv"), p("picks"), p("local"), p("src"),
            p("rp_t"), p("col_t"), [t.data_ptr() if t is not None else 0 for t in self.cnt_t],
            self.counts.data_ptr(), self.flag.data_ptr(), self.map.data_ptr(), self.bscratch.data_ptr(), int(k0),
            int(k1), int(salt) & 0xFFFFFFFF, _stream())

    def run(self, seeds, salt=SALT, seed=SEED):
        """Sample ``seeds`` (NumPy ids) into fresh sentinel-filled outputs; returns the host
        copies after checking what the pipeline must leave behind."""
        self.fresh_outputs()
        sd = _dev(np.asarray(seeds, dtype=np.int32)) if len(seeds) else torch.zeros(1, dtype=torch.int32, device=DEV)
        self.call(sd, salt, n_seeds=len(seeds), seed=seed)
        torch.cuda.synchronize()
        self.check_state()
        host = [{k: t.cpu().numpy() for k, t in lv.items()} for lv in self.out]
        return host, self.counts.cpu().numpy()

    def check_state(self):
        flag = self.flag.cpu().numpy()
        assert not flag[:self.fb].any(), "flag bytes left set: %s" % np.nonzero(flag[:self.fb])[0][:8]
        assert (flag[self.fb:] == FSENT).all()
        for l, c in enumerate(self.cnt_t):
            if c is not None:
                c = c.cpu().numpy()
                assert not c[:-TAIL].any(), "cnt_t[%d] left non-zero" % l
                assert (c[-TAIL:] == SENT).all()
        assert bool((self.map[-TAIL:] == SENT).all()) and bool((self.bscratch[-TAIL:] == SENT).all())

    def untouched(self):
        return all(bool((t == SENT).all()) for lv in self.out for t in lv.values()) and bool(
            (self.counts == SENT).all())


def compare(rig, got, seeds, salt=SALT, seed=SEED):
    """Every output of one ``Rig.run`` against the oracle; returns the oracle's levels."""
    host, counts = got
    rowptr, col = rig.g
    ref = sx.ref_blocks(rowptr, col, seeds, rig.fanouts, salt, seed, rig.need_t)
    nd = len(seeds)
    want_counts = np.asarray([x for b in ref for x in (b["n_src"], b["total"])], dtype=np.int32)
    np.testing.assert_array_equal(counts[:-TAIL], want_counts, err_msg="counts")
    assert (counts[-TAIL:] == SENT).all()
    for l, (h, b) in enumerate(zip(host, ref)):
        ns, tot = b["n_src"], b["total"]
        assert nd <= rig.nd_max[l] and ns <= rig.bounds[l][1]
        pairs = [("optr", b["optr"], nd + 1), ("inv", b["inv_deg"].view(np.int32), nd), ("picks", b["picks"], tot),
                 ("local", b["local"], tot), ("src", b["src"], ns)]
        if rig.need_t[l]:
            pairs += [("rp_t", b["rp_t"], ns + 1), ("col_t", b["col_t"], tot)]
        else:
            assert "rp_t" not in h
        for name, want, m in pairs:
            assert len(want) == m
            np.testing.assert_array_equal(h[name][:m], want, err_msg="level %d %s" % (l, name))
            # nothing behind the valid prefix, nothing behind the documented bound
            assert (h[name][m:] == SENT).all(), "level %d %s written past its valid prefix" % (l, name)
            assert len(h[name]) == rig.size[l][name] + TAIL
        nd = ns
    return ref


def run_and_compare(g, seeds, fanouts, batch=None, need_t=None, salt=SALT):
    rig = Rig(g, fanouts, len(seeds) if batch is None else batch, need_t)
    return rig, compare(rig, rig.run(seeds, salt), seeds, salt)


# ---------------------------------------------------------------------------- scan edges
@pytest.fixture(scope="module")
def scan_graph():
    rng = np.random.default_rng(11)
    n = 6000
    degs = rng.choice([0, 1, 2, 3, 4, 6, 9], n, p=[.1, .2, .2, .2, .1, .1, .1])
    return sx.random_graph(n, degs, rng), rng.permutation(n)


@pytest.mark.parametrize("slack", [0, 37])
@pytest.mark.parametrize("n_seeds", [0, 1, 255, 256, 1023, 1024, 1025, 2048, 2049, 4099])
def test_seed_counts_at_the_scan_block_edges(scan_graph, n_seeds, slack):
    g, perm = scan_graph
    seeds = perm[:n_seeds]
    # slack: the grids cover a bound above the device-side counts
    rig, ref = run_and_compare(g, seeds, [3, 2], batch=n_seeds + slack)
    if n_seeds == 0:
        assert [b["n_src"] for b in ref] == [0, 0] and ref[0]["optr"].tolist() == [0] == ref[0]["rp_t"].tolist()


@pytest.mark.parametrize("target", [1024, 1025])
def test_source_counts_at_the_scan_block_edges(target):
    # 512 seeds with one new neighbour each (seed 0: one more for the odd target); the new nodes
    # point back at seeds, so level 1 has `target` destinations and adds no source: the
    # destination scan and the transposed scan of both levels run at the edge
    k = 512
    rows = [[k + i] for i in range(k)] + [[i, (i + 1) % k] for i in range(k)] + [[3]]
    if target == 1025:
        rows[0] = [k, 2 * k]
    g = sx.csr(rows)
    rig, ref = run_and_compare(g, np.arange(k), [2, 2])
    assert [b["n_src"] for b in ref] == [target, target]


@pytest.mark.parametrize("n_seeds", [262145, 264000])
def test_more_than_256_scan_blocks(n_seeds):
    # block 256 of the destination scan sums 256 predecessors; with 264000 seeds, and in the
    # transposed scan over ~300000 sources, blocks 257.. take a second turn of that loop
    n = 300000
    g = sx.ring(n)
    seeds = np.random.default_rng(2).permutation(n)[:n_seeds]
    rig, ref = run_and_compare(g, seeds, [2])
    assert ref[0]["n_src"] > 257 * 1024 and ref[0]["total"] == 2 * n_seeds


# ---------------------------------------------------------------------------- flag blocks
def _star_graph(n, targets, seed_pool, per_seed=16):
    """Seeds from ``seed_pool`` whose rows hold the ``targets`` (16 per seed); all other rows
    are empty.  Returns the graph and the seeds."""
    targets = list(targets)
    rows = [[] for _ in range(n)]
    seeds = []
    for i in range(0, len(targets), per_seed):
        s = seed_pool[len(seeds)]
        rows[s] = targets[i:i + per_seed]
        seeds.append(s)
    return sx.csr(rows), np.asarray(seeds)


def _flag_cases():
    for n in (5, 4095, 4096, 4097, 8192, 12300):
        t = {0, 15, 16, 4095, 4096, n - 1} | set(range(32, 48))       # a thread's 16 ids all set
        if n == 8192:
            t |= set(range(4096, 8192))                               # a whole block set
        if n == 12300:
            t -= set(range(4096, 8192))                               # none set between two with some
            t |= {8192, 12000}
        t = sorted(x for x in t if 0 <= x < n)
        ts = set(t)
        pool = [x for x in range(n) if x not in ts]
        if n == 5:
            t, pool = [0, 4], [2, 1]
        yield n, t, pool


@pytest.mark.parametrize("n,targets,pool", [pytest.param(*c, id="n%d" % c[0]) for c in _flag_cases()])
def test_new_sources_at_the_flag_block_edges(n, targets, pool):
    # seeds taken from the top of the pool: descending, far from their targets
    g, seeds = _star_graph(n, targets, pool[::-1])
    rig, ref = run_and_compare(g, seeds, [16, 3])
    assert ref[0]["src"][len(seeds):].tolist() == targets
    assert ref[1]["n_src"] == ref[0]["n_src"]                          # the new sources have empty rows


def test_more_than_256_flag_blocks():
    # 257 full flag blocks and one id: the last block sums 257 predecessors (a second turn of
    # the compaction's loop); new sources in blocks 0, 255, 256 and the last one
    n = 257 * 4096 + 1
    g = sx.ring(n)
    seeds = np.asarray([5, 255 * 4096 + 7, 256 * 4096 + 9, n - 2, 0, 255 * 4096])
    rig, ref = run_and_compare(g, seeds, [2, 2])
    new = ref[0]["src"][len(seeds):] // 4096
    assert {0, 255, 256, 257} <= set(new.tolist())
    assert (n - 1) in ref[0]["src"][len(seeds):]


# ---------------------------------------------------------------------------- fan-out, degree
def _degree_graph(fo, rng, n=6000, per=24):
    """Rows of degree 0, 1, fo - 1, fo, fo + 1, 2 fo (``per`` of each) and one of 5000 as the
    seeds, shuffled; the other rows have degrees up to 2 fo + 1 (the next level's)."""
    special = sorted({0, 1, max(fo - 1, 0), fo, fo + 1, 2 * fo})
    degs = rng.integers(0, 2 * fo + 2, n)
    seeds = rng.permutation(n)[:per * len(special) + 1]
    for i, d in enumerate(special):
        degs[seeds[per * i:per * (i + 1)]] = d
    degs[seeds[-1]] = 5000
    return sx.random_graph(n, degs, rng), rng.permutation(seeds)


@pytest.mark.parametrize("fo", [1, 2, 3, 4, 5, 15, 16, 17, 63, 64])
def test_fanouts_and_degrees_around_them(fo):
    g, seeds = _degree_graph(fo, np.random.default_rng(100 + fo))
    rig, ref = run_and_compare(g, seeds, [fo, fo])
    deg = np.diff(g[0])[seeds]
    assert (deg > fo).sum() >= (49 if fo > 1 else 25) and(np.diff(ref[0]["optr"]) == np.minimum(deg, fo)).all()


@pytest.mark.parametrize("fanouts", [[25, 64], [64, 1], [5, 17, 2], [16, 17]])
def test_mixed_fanouts_use_both_templates(fanouts):
    rng = np.random.default_rng(5)
    n = 3000
    g = sx.random_graph(n, rng.integers(0, 130, n), rng)
    run_and_compare(g, rng.permutation(n)[:40], fanouts)


@pytest.mark.parametrize("fo", [-1, 1, 16, 17, 64])
def test_sample_neighbors_alone(fo):
    rng = np.random.default_rng(9)
    n = 2000
    degs = rng.integers(0, 100, n)
    degs[[0, n - 1]] = [5000, 0]
    rowptr, col = sx.random_graph(n, degs, rng)
    nodes = np.concatenate([[0, n - 1], rng.permutation(np.arange(1, n - 1))[:700]])
    k0, k1 = model_key(SEED, "neighbour-sampler")
    lsalt = sx.level_salt(SALT, 3)
    optr, picks = sx.ref_sample(rowptr, col, nodes, fo, lsalt, k0, k1)
    if fo < 0:
        assert len(picks) == degs[nodes].sum()
    out = torch.full((len(picks) + TAIL,), SENT, dtype=torch.int32, device=DEV)
    drp, dcol, dn, dop = _dev(rowptr), _dev(col), _dev(nodes.astype(np.int32)), _dev(optr)
    native.hip().gnn_sample_neighbors(drp.data_ptr(), dcol.data_ptr(), dn.data_ptr(), len(nodes), fo, dop.data_ptr(),
                                      out.data_ptr(), int(k0), int(k1), lsalt, _stream())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    np.testing.assert_array_equal(out[:len(picks)], picks)
    assert (out[len(picks):] == SENT).all()


# ---------------------------------------------------------------------------- structure
def test_self_loops_repeated_columns_and_picked_destinations():
    rows = [[0, 0, 1], [1], [], [2, 0, 2, 0, 3, 3, 3], [4], [6, 6, 6, 6], [5, 0], [8, 8], [7, 7, 9], [9]]
    g = sx.csr(rows)
    for seeds in ([3, 0, 2], [9, 8, 7, 6, 5, 4, 3, 2, 1, 0], [5], [0, 9]):
        rig, ref = run_and_compare(g, np.asarray(seeds), [3, 2, 64])
    rig, ref = run_and_compare(g, np.asarray([3, 0, 2]), [3, 2])
    assert set(ref[0]["picks"].tolist()) & {3, 0, 2}                   # picks that are destinations


def test_a_level_that_adds_no_source():
    n = 50
    g = sx.csr([[c for c in range(n) if c != v] for v in range(n)])      # a clique, every node a seed
    rig, ref = run_and_compare(g, np.random.default_rng(1).permutation(n), [64, 7])
    assert [b["n_src"] for b in ref] == [n, n] and ref[0]["total"] == n * (n - 1)


def test_source_growth_capped_at_n():
    rng = np.random.default_rng(3)
    n = 300
    g = sx.random_graph(n, rng.integers(5, 40, n), rng)
    rig, ref = run_and_compare(g, rng.permutation(n)[:100], [10, 10, 10])
    assert rig.nd_max == [100, n, n] and ref[2]["n_src"] == n


@pytest.mark.parametrize("order", ["descending", "shuffled", "ends", "isolated between"])
def test_seed_orders_and_isolated_seeds(order):
    rng = np.random.default_rng(4)
    n = 1500
    degs = rng.integers(1, 20, n)
    iso = np.arange(7, n, 13)
    degs[iso] = 0
    g = sx.random_graph(n, degs, rng)
    seeds = {"descending": np.arange(n - 1, n - 400, -1), "shuffled": rng.permutation(n)[:333],
             "ends": np.asarray([n - 1, 0]), "isolated between": np.arange(0, 200)}[order]
    rig, ref = run_and_compare(g, seeds, [4, 17])
    if order == "isolated between":
        assert (ref[0]["inv_deg"][iso[iso < 200]] == 0).all()


# ---------------------------------------------------------------------------- transpose
def test_transposed_hub_bucket_empty_buckets_and_a_multi_edge():
    # 2049 destinations pick the hub: one bucket longer than a scan block; the seeds are
    # picked by nobody (2049 leading empty buckets); seed 5 picks the hub twice
    k, hub, n = 2049, 3000, 3001
    rows = [[hub] for _ in range(k)] + [[] for _ in range(n - k)]
    rows[5] = [hub, hub]
    rows[7] = [hub, 2500]
    rows[2500] = [0, 0, 3]
    rows[hub] = [hub, 1]
    g = sx.csr(rows)
    rig, ref = run_and_compare(g, np.arange(k), [2, 2])
    b = ref[0]
    assert b["rp_t"][:k + 1].tolist() == [0] * (k + 1) and b["src"][-1] == hub
    bucket = b["col_t"][b["rp_t"][-2]:b["rp_t"][-1]]
    assert len(bucket) == k + 1 and (bucket == 5).sum() == 2


@pytest.mark.parametrize("need_t", [(True, False), (False, True), (False, False), (True, True)])
def test_transposed_csr_on_and_off_per_level(need_t):
    rng = np.random.default_rng(6)
    n = 2500
    g = sx.random_graph(n, rng.integers(0, 12, n), rng)
    run_and_compare(g, rng.permutation(n)[:300], [5, 3], need_t=need_t)


# ---------------------------------------------------------------------------- independence
def test_a_nodes_picks_do_not_depend_on_its_batch_and_runs_repeat():
    rng = np.random.default_rng(8)
    n = 800
    g = sx.random_graph(n, rng.integers(0, 40, n), rng)
    common = rng.permutation(n)[:60]
    rest = np.setdiff1d(np.arange(n), common)
    a = np.concatenate([common, rest[:200]])
    b = rng.permutation(np.concatenate([rest[300:420], common]))
    big = Rig(g, [7, 17], 300)
    ra = compare(big, big.run(a), a)
    rb = compare(big, big.run(b), b)
    pa = {int(v): ra[0]["picks"][ra[0]["optr"][i]:ra[0]["optr"][i + 1]].tolist() for i, v in enumerate(a)}
    pb = {int(v): rb[0]["picks"][rb[0]["optr"][i]:rb[0]["optr"][i + 1]].tolist() for i, v in enumerate(b)}
    assert all(pa[int(v)] == pb[int(v)] for v in common) and list(a[:60]) != list(b[:60])
    # the same batch twice in the same slot, right after a larger one, and in a fresh slot
    small = b[:50]
    first = big.run(small)
    second = big.run(small)
    fresh = Rig(g, [7, 17], 300)
    third = fresh.run(small)
    compare(big, first, small)
    for other in (second, third):
        assert np.array_equal(first[1], other[1])
        for h0, h1 in zip(first[0], other[0]):
            assert all(np.array_equal(h0[k], h1[k]) for k in h0)
    # another salt or key: other picks
    assert not np.array_equal(big.run(small, salt=SALT + 1)[0][0]["picks"], first[0][0]["picks"])
    assert not np.array_equal(big.run(small, seed=SEED + 1)[0][0]["picks"], first[0][0]["picks"])


# ---------------------------------------------------------------------------- the wrappers
@pytest.fixture(scope="module")
def wrapper_case():
    rng = np.random.default_rng(12)
    n = 5000
    g = sx.random_graph(n, rng.integers(0, 100, n), rng)
    batches = [rng.permutation(n)[:m] for m in (48, 41, 48, 1, 33)]
    return g, batches


@pytest.mark.parametrize("slots,publish,threaded", [(2, False, False), (3, True, False), (3, True, True)])
@pytest.mark.parametrize("fanouts", [[25, 64], [5, 17, 3]])
def test_pipelined_sampler_matches_the_oracle(wrapper_case, fanouts, slots, publish, threaded):
    g, batches = wrapper_case
    ps = PipelinedSampler(_dev(g[0]), _dev(g[1]), fanouts, 48, seed=SEED, slots=slots, publish=publish,
                          threaded=threaded)
    L = len(fanouts)
    need_t = [l < L - 1 for l in range(L)]
    for k, seeds in enumerate(batches):
        salt = SALT + k
        sb = ps.enqueue(_dev(seeds.astype(np.int32)), salt)
        blocks, nodes = sb.resolve()
        torch.cuda.current_stream().wait_event(sb.slot.done)
        torch.cuda.synchronize()
        ref = sx.ref_blocks(g[0], g[1], seeds, fanouts, salt, SEED, need_t)
        sl = sb.slot
        want_counts = [x for b in ref for x in (b["n_src"], b["total"])]
        assert sl.counts_host.tolist() == want_counts and sl.counts.tolist() == want_counts
        assert np.array_equal(nodes.cpu().numpy(), ref[-1]["src"])
        for l, (blk, b) in enumerate(zip(blocks[::-1], ref)):
            assert blk.n_src == b["n_src"]
            assert np.array_equal(blk.rowptr.cpu().numpy(), b["optr"])
            assert np.array_equal(blk.col.cpu().numpy(), b["local"])
            assert np.array_equal(blk.gcol.cpu().numpy(), b["picks"])
            assert np.array_equal(blk.inv_deg.cpu().numpy().view(np.int32), b["inv_deg"].view(np.int32))
            assert np.array_equal(sl.src[l][:b["n_src"]].cpu().numpy(), b["src"])
            if need_t[l]:
                rp_t, col_t = blk.transposed()
                assert np.array_equal(rp_t.cpu().numpy(), b["rp_t"]) and np.array_equal(col_t.cpu().numpy(), b["col_t"])
                assert not bool(sl.cnt_t[l].any())
        assert not bool(ps.flag.any())
        ps.consumed(sb)


def test_device_sampler_matches_the_oracle(wrapper_case):
    g, batches = wrapper_case
    fanouts = [25, 64]
    ds = DeviceSampler(_dev(g[0]), _dev(g[1]), fanouts, seed=SEED)
    for k, seeds in enumerate(batches[:3]):
        blocks, nodes = ds.sample(_dev(seeds.astype(np.int32)), SALT + k)
        ref = sx.ref_blocks(g[0], g[1], seeds, fanouts, SALT + k, SEED, [False, False])
        assert np.array_equal(nodes.cpu().numpy(), ref[-1]["src"])
        for blk, b in zip(blocks[::-1], ref):
            assert blk.n_src == b["n_src"]
            assert np.array_equal(blk.rowptr.cpu().numpy(), b["optr"])
            assert np.array_equal(blk.col.cpu().numpy(), b["local"])
            assert np.array_equal(blk.inv_deg.cpu().numpy().view(np.int32), b["inv_deg"].view(np.int32))


# ---------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("what,kw", [
    ("fan-outs [5, 70]", dict(fanouts=[5, 70])), ("fan-out 0", dict(fanouts=[0, 3])),
    ("n = 0", dict(n=0)), ("n_seeds < 0", dict(n_seeds=-1)), ("n_seeds over nd_max[0]", dict(n_seeds=9)),
    ("nd_max[1] = 0", dict(nd_max=[8, 0]))])
def test_refused_calls_enqueue_nothing(what, kw):
    rng = np.random.default_rng(13)
    g = sx.random_graph(100, rng.integers(0, 9, 100), rng)
    rig = Rig(g, [5, 3], 8)
    rig.fresh_outputs()
    seeds = _dev(np.arange(8, dtype=np.int32))
    with pytest.raises(RuntimeError, match=r"\(code -3\)"):
        rig.call(seeds, **kw)
    torch.cuda.synchronize()
    assert rig.untouched()
    rig.check_state()
    # the same buffers then serve a valid call
    compare(rig, rig.run(np.arange(8)), np.arange(8))


def test_no_level_is_refused():
    with pytest.raises(RuntimeError, match=r"\(code -3\)"):
        native.hip().gnn_sample_blocks(64, 64, 10, 64, 0, [], [], [], [], [], [], [], [], [], [], 64, 64, 64, 64, 1, 2,
                                       3, _stream())


def test_zero_seeds_succeed():
    rng = np.random.default_rng(14)
    g = sx.random_graph(100, rng.integers(0, 9, 100), rng)
    rig = Rig(g, [5, 3], 8)
    host, counts = rig.run(np.zeros(0, dtype=np.int64))
    assert not counts[:4].any()
    assert host[0]["optr"][0] == 0 and host[0]["rp_t"][0] == 0 and host[1]["optr"][0] == 0 and host[1]["rp_t"][0] == 0
    compare(rig, (host, counts), np.zeros(0, dtype=np.int64))
