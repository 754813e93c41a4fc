"""The native step engine against a replay of its launch sequence through the raw launchers
(bit for bit), and the values it produces against fp64 (tests/engine_oracle.py).

Chain of equalities: chunked graph replay == eager chunks == one step per call == the raw
launchers in the documented order (``ShadowEngine``), each on every buffer of
``engine_oracle.COMPARED``, compared as bit patterns.  On top, the history, ``loss_last``,
``loss_acc``, ``tt`` and ``collect()`` against fp64 losses of the device's own ``xhat``
snapshots, and the first two Adam updates against ``adam_oracle64`` of the device's ``gpart``.

Every configuration runs once step by step (``stepwise``, cached) with a history and without;
the tests read that run.  Before every step ``lpart`` and ``loss_last`` of the trainer and of
the shadow are filled with a sentinel: a partial count that is too large reads it, and what a
step leaves unwritten is compared as unchanged.
"""
import functools

import numpy as np
import pytest
import torch

import cgnn_gen_oracle as ox
import engine_oracle as eo
from cgnn_amd import native
from cgnn_amd.engine.batch import DeviceTrainer

pytestmark = pytest.mark.gpu

IDS = tuple(eo.CONFIGS)
U = eo.U
RATIOS = {}


def _record(key, value):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(value))


def _trainer(cfg, hist_len, graph_chunk):
    tr = DeviceTrainer(cfg.programs(), cfg.datas(), cfg.keys(), eo.H, "cuda:0", **cfg.trainer_kwargs(hist_len, graph_chunk))
    assert tr.staged == (cfg.gen == "staged") and tr.mmd_kernel == cfg.loss, (tr.staged, tr.mmd_kernel)
    return tr


def _fill_unwritten(*objs):
    for o in objs:
        with torch.cuda.stream(o.stream):
            for name in eo.UNWRITTEN_CHECK:
                getattr(o, name).fill_(eo.SENT)


def _snap(o):
    o.stream.synchronize()
    return eo.snapshot(o)


class Run:
    pass


@functools.lru_cache(maxsize=None)
def stepwise(cid, hist):
    """DeviceTrainer.start(), 5 training and 3 evaluation steps, one per ``engine.run`` call,
    the shadow alongside: snapshots of both after start and after every step."""
    cfg = eo.CONFIGS[cid]
    hip = native.hip()
    cfg.check(hip)
    hist_len = eo.TRAIN_STEPS if hist else 0
    tr, sh = _trainer(cfg, hist_len, 0), eo.ShadowEngine(cfg, hist_len)
    run = Run()
    run.cfg, run.counts = cfg, (tr.engine.n_parts(), tr.engine.gen_blocks())
    run.shadow_counts = (sh.n_parts, sh.G)
    run.tol_counts = (sh.n_parts, sh.n_parts_tt, sh.mf_tpc if cfg.loss == "mfma" else sh.tpc,
                      (sh.mf_tpc if getattr(sh, "tt_mfma", False) else sh.tpc), getattr(sh, "tt_mfma", False))
    run.dev, run.shd, run.kinds, run.draw = [], [], [], []
    tr.start()
    sh.start()
    run.dev.append(_snap(tr))
    run.shd.append(_snap(sh))
    for t in range(eo.TRAIN_STEPS + eo.EVAL_STEPS):
        kind = 0 if t < eo.TRAIN_STEPS else 1
        _fill_unwritten(tr, sh)
        with torch.cuda.device(tr.device):
            tr.engine.run(kind, 1, 0, hist_len > 0)
        sh.run(kind, 1)
        run.dev.append(_snap(tr))
        run.shd.append(_snap(sh))
        run.kinds.append(kind)
        if kind == 1 and cfg.gen == "staged":
            run.draw.append(_draw_binding(sh, run.dev[-2]["step"], run.dev[-1]))
    tr._test_epochs = eo.EVAL_STEPS
    run.scores = tr.collect()
    # and one eager chunk of two steps of each kind: the engine's step offsets 0 and 1
    run.extra = []
    for kind in (0, 1):
        _fill_unwritten(tr, sh)
        with torch.cuda.device(tr.device):
            tr.engine.run(kind, 2, 0, hist_len > 0)
        sh.run(kind, 2)
        run.extra.append((_snap(tr), _snap(sh)))
    return run


def _draw_binding(sh, step_before, after):
    """``gen_fwd_staged_draw`` at the counter the step began with, with and without a noise
    buffer, into scratch outputs: (xhat equal, xnorm equal, stored noise equal) per variant."""
    hip, p = sh.hip, sh._p
    out = []
    step = torch.from_numpy(step_before.copy()).cuda()
    for with_noise in (True, False):
        xh, xn = torch.full_like(sh.xhat, eo.SENT), torch.full_like(sh.xnorm, eo.SENT)
        nz = torch.zeros_like(sh.noise) if with_noise else None
        xh[:, sh.d:] = 0.0                       # padding rows are the caller's zeros
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(sh.stream):
            hip.gen_fwd_staged_draw(p(sh.prog), sh.ps, p(sh.sched), sh.ss, p(sh.params), sh.P, p(sh.data), p(xh),
                                    p(nz), sh.NS, p(xn), sh.N, sh.D, sh.d, eo.H, sh.max_in, sh.R, sh.W, sh.st,
                                    keys=p(sh.keys), step=p(step), off=0, row0=0)
        sh.stream.synchronize()
        ok = [np.array_equal(xh.cpu().numpy().view(np.int32), after["xhat"]),
              np.array_equal(xn.cpu().numpy().view(np.int32), after["xnorm"])]
        if with_noise:
            rows = np.stack([eo.stored_noise_rows(q, sh.D, sh.NS) for q in sh.cfg.programs()])
            got, want = nz.cpu().numpy().view(np.int32), sh.noise.cpu().numpy().view(np.int32)
            ok.append(np.array_equal(got[rows], want[rows]) and not got[~rows].any())
        out.append(ok)
    return out


# ---------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("hist", [True, False], ids=["hist", "nohist"])
@pytest.mark.parametrize("cid", IDS)
def test_engine_equals_raw_launchers_bit_for_bit(cid, hist):
    """After start() and after each of the 5 + 3 steps every compared buffer of the trainer has
    the bits of the shadow's.  What a step does not write, found by reading the kernels and
    pinned here through the sentinel fill (equal to the shadow's, which writes the same set):
    a training step without a history (mode 3) writes exact +0 to its ``n_parts`` loss partials
    (all three MMD kernels store the untouched accumulator) and leaves ``loss_last``,
    ``loss_acc`` and ``hist`` alone -- ``loss_last`` must still read the sentinel; with a history
    it leaves ``loss_acc``; an evaluation step leaves ``hist``, ``gradp``, ``gpart``, ``params``,
    ``m``, ``v`` and, with the staged generator, ``noise`` (the engine passes no noise buffer;
    the shadow's gen_noise writes its own).  ``lpart`` past the partials the pass writes keeps
    the sentinel on both sides.  The history of the two extra training steps (counter 5, 6)
    falls past ``hist_stride`` = 5 and must leave ``hist`` as it was."""
    run = stepwise(cid, hist)
    cfg = run.cfg
    staged = cfg.gen == "staged"
    rows = np.stack([eo.stored_noise_rows(q, run.dev[0]["noise"].shape[1] - max(p.n_conf for p in cfg.programs()),
                                          run.dev[0]["noise"].shape[1]) for q in cfg.programs()])
    for t, (a, b) in enumerate(zip(run.dev, run.shd)):
        what = "%s hist=%s after %s" % (cid, hist, "start" if t == 0 else "step %d" % t)
        diff = eo.differing(a, b)
        if staged and t > 0 and "noise" in diff:
            if run.kinds[t - 1] == 0:              # the drawing forward stores the rows it consumes
                if np.array_equal(a["noise"][rows], b["noise"][rows]):
                    diff.remove("noise")
            elif np.array_equal(a["noise"], run.dev[t - 1]["noise"]):
                diff.remove("noise")
        assert diff == [], what + ": differ in " + ", ".join(diff)
        if t == 0:
            continue
        before = run.dev[t - 1]
        sent = np.float32(eo.SENT).view(np.int32)
        if run.kinds[t - 1] == 0:
            assert np.array_equal(a["loss_acc"], before["loss_acc"]), what
            if not hist:
                assert np.all(a["loss_last"] == sent), what + ": loss_last written without a history"
                if cfg.loss != "rff":
                    n = cfg.R * run.shadow_counts[0]
                    assert not a["lpart"].ravel()[:n].any(), what + ": mode 3 loss partials"
                    assert np.all(a["lpart"].ravel()[n:] == sent), what
        else:
            for name in ("hist", "gradp", "gpart", "params", "m", "v") + (("noise",) if staged else ()):
                assert np.array_equal(a[name], before[name]), what + ": evaluation wrote " + name
            assert a["step"].tolist() == [before["step"][0] + 1, before["step"][1]], what
    assert run.dev[-1]["step"].tolist() == [eo.TRAIN_STEPS + eo.EVAL_STEPS, eo.TRAIN_STEPS]
    # single-step calls only ever pass offset 0: a two-step eager chunk of each kind on top
    for kind, (a, b) in enumerate(run.extra):
        diff = eo.differing(a, b)
        if staged and "noise" in diff and (kind == 1 or np.array_equal(a["noise"][rows], b["noise"][rows])):
            diff.remove("noise")
        assert diff == [], "%s hist=%s two-step eager chunk of kind %d: differ in %s" % (cid, hist, kind, ", ".join(diff))
    assert np.array_equal(run.extra[0][0]["hist"], run.dev[-1]["hist"]), "history written past hist_stride"
    assert np.array_equal(run.extra[1][0]["noise"], run.extra[0][0]["noise"]) or not staged
    assert run.extra[1][0]["step"].tolist() == [eo.TRAIN_STEPS + eo.EVAL_STEPS + 4, eo.TRAIN_STEPS + 2]
    for k, res in enumerate(run.draw):
        assert all(res[0]) and all(res[1]), "%s eval step %d: gen_fwd_staged_draw binding %s" % (cid, k, res)
    assert len(run.draw) == (eo.EVAL_STEPS if staged else 0)


def _guarded_history(monkeypatch, R, hist_len, guard=16):
    """Make the next DeviceTrainer record its history into a view of a larger sentinel-filled
    buffer (the engine takes the pointer at construction): returns the flat buffer."""
    flat = torch.full((R * hist_len + guard,), eo.SENT, dtype=torch.float32, device="cuda:0")
    real = native.hip()

    class Proxy:
        def __getattr__(self, name):
            return getattr(real, name)

        def CgnnEngine(self, icfg, fcfg, ptrs, stream):
            ptrs = list(ptrs)
            assert ptrs[eo.HIST_SLOT] != 0 and icfg[eo.ICFG.index("hist_stride")] == hist_len
            ptrs[eo.HIST_SLOT] = flat.data_ptr()
            return real.CgnnEngine(icfg, fcfg, ptrs, stream)

    import cgnn_amd.engine.batch as eb
    monkeypatch.setattr(eb.native, "hip", lambda: Proxy())
    return flat


@pytest.mark.parametrize("cid", IDS)
def test_chunked_replay_equals_step_by_step(cid, monkeypatch):
    """train(5) + evaluate(3) as two replays of a captured two-step graph plus an eager
    remainder (graph_chunk = 2) and as eager chunks (graph_chunk = 0) end in the bits of the
    step-by-step run.  With a history of 3 < 5 steps the history holds the first three losses of
    the full history and nothing is written past it (sentinel behind the view)."""
    cfg = eo.CONFIGS[cid]
    full = stepwise(cid, True)
    want = full.dev[-1]
    for chunk in (2, 0):
        for hist_len in (eo.TRAIN_STEPS, 3):
            flat = _guarded_history(monkeypatch, cfg.R, hist_len)
            tr = _trainer(cfg, hist_len, chunk)
            monkeypatch.undo()
            tr.hist = flat[:cfg.R * hist_len].view(cfg.R, hist_len)
            tr.start()
            _fill_unwritten(tr)
            tr.train(eo.TRAIN_STEPS)
            tr.evaluate(eo.EVAL_STEPS)
            got = _snap(tr)
            what = "%s chunk=%d hist_len=%d" % (cid, chunk, hist_len)
            diff = [n for n in eo.differing(got, want) if n != "hist"]
            assert diff == [], what + ": differ in " + ", ".join(diff)
            assert np.array_equal(got["hist"], want["hist"][:, :hist_len]), what + ": history"
            tail = flat[cfg.R * hist_len:].cpu().numpy()
            assert np.all(tail == np.float32(eo.SENT)), what + ": written past the history"


@pytest.mark.parametrize("cid", IDS)
def test_engine_n_parts_and_gen_blocks(cid):
    run = stepwise(cid, True)
    assert run.counts == run.shadow_counts, (run.counts, run.shadow_counts)


# ---------------------------------------------------------------------------- fp64 tier
def _losses64(run, t):
    """(loss [R], tol [R], tt tol [R] | None) of the snapshot after step t."""
    cfg, s = run.cfg, run.dev[t]
    xh = eo.f32view(s, "xhat").astype(np.float64)
    D = xh.shape[1]
    data = np.zeros_like(xh)
    for r, x in enumerate(cfg.datas()):
        data[r, :cfg.d] = x
    if cfg.loss == "rff":
        L, tol = eo.rff_loss64(xh, data, eo.f32view(s, "rff_w").astype(np.float64), cfg.k)
        return L, tol, None
    L = np.array([eo.loss64(xh[r, :cfg.d], data[r, :cfg.d], cfg.N) for r in range(cfg.R)])
    tols = [eo.loss_tol(xh[r], data[r], cfg, run.tol_counts) for r in range(cfg.R)]
    return L, np.array([a for a, _ in tols]), np.array([b for _, b in tols])


@pytest.mark.parametrize("hist", [True, False], ids=["hist", "nohist"])
@pytest.mark.parametrize("cid", IDS)
def test_losses_against_fp64(cid, hist):
    """``hist[r, t]`` (training, when recorded), ``loss_last[r]`` (evaluation), ``tt[r]``,
    ``loss_acc`` and ``collect()`` against fp64 of the device's own ``xhat`` (Fourier: on the
    device's own ``rff_w``).  Tolerance: engine_oracle's docstring -- the per-pair bound of
    test_mmd_exact_gpu.py plus the rounding of ``d2`` off the lattice, the partial sums' depth,
    ``n_parts u sum|partials|`` for loss_finalize; rff_oracle's composed diff / loss-partial
    bounds for the Fourier loss.  It is at most 2e-4 of the loss in every case and step
    (asserted here on the device's samples, on the CPU from the reference alone).
    Largest error / tolerance seen on an MI355X: docs/KERNELS.md."""
    run = stepwise(cid, hist)
    cfg = run.cfg
    acc, acc_tol, acc_abs = np.zeros(cfg.R), np.zeros(cfg.R), np.zeros(cfg.R)
    tt_tol = _losses64(run, 1)[2]
    if tt_tol is not None:
        tt = np.array([eo.tt64(np.asarray(x, np.float64)) for x in cfg.datas()])
        e = np.abs(eo.f32view(run.dev[0], "tt").astype(np.float64) - tt)
        _record("tt", (e / tt_tol).max())
        assert np.all(e <= tt_tol), "%s: tt %s" % (cid, e / tt_tol)
    for t in range(1, len(run.dev)):
        kind = run.kinds[t - 1]
        if kind == 0 and not hist:
            continue
        L, tol, tt_tol = _losses64(run, t)
        assert np.all(tol <= eo.REL_CAP * np.abs(L)), "%s step %d: tolerance %s over 2e-4 of the loss %s" % (cid, t, tol, L)
        got = eo.f32view(run.dev[t], "hist")[:, t - 1] if kind == 0 else eo.f32view(run.dev[t], "loss_last")
        err = np.abs(got.astype(np.float64) - L)
        print("%s step %d: loss %s err/tol %s tol/loss %.2e" % (cid, t, L, err / tol, (tol / L).max()))
        _record("loss", (err / tol).max())
        assert np.all(err <= tol), "%s step %d: loss %s against fp64 %s, tolerance %s" % (cid, t, got, L, tol)
        if kind == 1:
            acc, acc_tol, acc_abs = acc + L, acc_tol + tol, acc_abs + np.abs(L)
    fin = eo.f32view(run.dev[-1], "loss_acc").astype(np.float64)
    tol = acc_tol + eo.EVAL_STEPS * U * acc_abs
    _record("loss_acc", (np.abs(fin - acc) / tol).max())
    assert np.all(np.abs(fin - acc) <= tol), "%s: loss_acc" % cid
    assert np.all(np.abs(run.scores - acc / eo.EVAL_STEPS) <= (tol + U * acc_abs) / eo.EVAL_STEPS), "%s: collect()" % cid
    assert np.array_equal(run.dev[-1]["tt"], run.dev[0]["tt"])
    print("largest error / tolerance so far:", RATIOS)


@pytest.mark.parametrize("cid", IDS)
def test_first_update_against_fp64_adam(cid):
    """params, m, v after training steps 1 and 2 against fp64 TF1 Adam of the device's own
    ``gpart`` at t = 1 and t = 2 (``adam_oracle64``, its ``lr_t_rel`` bound): the optimiser
    counter ``step[1]`` feeds the update it belongs to."""
    run = stepwise(cid, True)
    cfg = run.cfg
    for t in (1, 2):
        a, b = run.dev[t - 1], run.dev[t]
        assert b["step"].tolist() == [t, t]
        gp = eo.f32view(b, "gpart")
        for r, q in enumerate(cfg.programs()):
            Pr = q.n_params
            g = np.where(np.arange(gp.shape[2]) < Pr, gp[r], 0.0).astype(np.float32)
            old = [eo.f32view(a, n)[r].astype(np.float64) for n in ("params", "m", "v")]
            p64, m64, v64, dp, dm, dv = ox.adam_oracle64(old[0], old[1], old[2], g, Pr, t, cfg.lr, eo.BETA1, eo.BETA2, eo.EPS)
            for name, ref, bound in (("params", p64, dp), ("m", m64, dm), ("v", v64, dv)):
                err = np.abs(eo.f32view(b, name)[r].astype(np.float64) - ref)
                ok = bound > 0
                if ok.any():
                    _record("adam " + name, (err[ok] / bound[ok]).max())
                assert np.all(err <= bound), "%s t=%d r=%d: %s, worst err/bound %.3g at %d" % (
                    cid, t, r, name, (err[ok] / bound[ok]).max() if ok.any() else np.inf, int(np.argmax(err - bound)))
            assert np.any(eo.f32view(b, "params")[r, :Pr] != eo.f32view(a, "params")[r, :Pr])
    print("adam error / bound:", {k: v for k, v in RATIOS.items() if k.startswith("adam")})


# ---------------------------------------------------------------------------- sensitivity
def _chunked_shadow(cfg, hist_len, mut):
    sh = eo.ShadowEngine(cfg, hist_len, mut=mut)
    sh.start()
    _fill_unwritten(sh)
    sh.run(0, eo.TRAIN_STEPS)
    mid = _snap(sh)
    sh.run(1, eo.EVAL_STEPS)
    return mid, _snap(sh)


@pytest.mark.parametrize("cid", eo.MUTATION_CONFIGS)
def test_shadow_mutations_are_detected(cid):
    """Each deliberate error of the shadow (all inside allocated memory: counts only shrink)
    changes a compared buffer after the training chunk or after the evaluation chunk.  The
    unmutated shadow, run as one chunk of 5 and one of 3, ends in the bits of the step-by-step
    engine.  ``mode0_for_3`` (no history) changes the loss partials the step leaves behind and
    nothing else."""
    cfg = eo.CONFIGS[cid]
    applied = []
    for hist_len in (eo.TRAIN_STEPS, 0):
        mid0, end0 = _chunked_shadow(cfg, hist_len, None)
        assert eo.differing(end0, stepwise(cid, hist_len > 0).dev[-1]) == []
        for mut in eo.MUTATIONS:
            if not eo.mutation_applies(mut, cfg) or (mut == "mode0_for_3") != (hist_len == 0):
                continue
            mid, end = _chunked_shadow(cfg, hist_len, mut)
            changed = sorted(set(eo.differing(mid, mid0)) | set(eo.differing(end, end0)))
            print(cid, mut, "changes", changed)
            assert changed, "%s: mutation %s went unnoticed" % (cid, mut)
            if mut == "mode0_for_3":
                assert changed == ["lpart"] and eo.differing(end, end0) == [], changed
            applied.append(mut)
    assert set(applied) == {m for m in eo.MUTATIONS if eo.mutation_applies(m, cfg)}
