"""Host-side half of the engine step oracle (tests/engine_oracle.py): the committed
configurations reach the branches they exist for, the fp64 tier's tolerance is at most 2e-4 of
the loss from the reference alone, the fp64 losses are ``ReferenceTrainer``'s, and the
positional icfg / fcfg / ptrs lists ``DeviceTrainer`` builds are in the order
``cgnn_engine_create`` reads."""
import os
import re

import numpy as np
import pytest
import torch

import cgnn_amd
import engine_oracle as eo
import rff_oracle as rx
from cgnn_amd.engine import batch as eb

CSRC = os.path.join(os.path.dirname(os.path.abspath(cgnn_amd.__file__)), "csrc", "kernels")
IDS = tuple(eo.CONFIGS)


def _hip():
    try:
        from cgnn_amd import native
        return native.hip()
    except Exception as e:                                   # no built extension on this machine
        pytest.skip("the _hip module cannot be imported: %s" % e)


def test_the_table_of_configurations():
    assert IDS == ("valu1", "valu_mirror", "conf", "mfma_vtt", "mfma_mtt", "staged_small", "staged_dxs",
                   "rff_narrow", "rff_wide")
    shape = {c.id: (c.d, c.N, c.k) for c in eo.CONFIGS.values()}
    assert shape["valu1"] == (2, 65, 0) and shape["valu_mirror"] == (5, 257, 0) and shape["conf"] == (5, 64, 0)
    assert shape["mfma_vtt"] == (10, 130, 0) and shape["mfma_mtt"] == (70, 150, 0)
    assert shape["staged_small"] == (24, 65, 0) and shape["rff_narrow"] == (5, 65, 5) and shape["rff_wide"][::2] == (40, 10)
    assert eb.padded_dim(10) == 12 and eb.padded_dim(70) == 80 and eb.padded_dim(40) == 48 > eb.WIDE_RFF_D
    assert set(eo.MUTATION_CONFIGS) <= set(IDS)


@pytest.mark.parametrize("cid", IDS)
def test_configuration_preconditions(cid):
    eo.CONFIGS[cid].check(_hip())


def test_every_mutation_runs_somewhere():
    assert len(eo.MUTATIONS) == 9
    for mut in eo.MUTATIONS:
        assert any(eo.mutation_applies(mut, eo.CONFIGS[c]) for c in eo.MUTATION_CONFIGS), mut


def _reference_steps(cfg):
    """(generated samples [R, d, N] fp64, rng step, ReferenceTrainer's own losses [R]) before each
    of the 5 + 3 steps of the schedule, on the CPU reference."""
    ref = eo.reference_trainer(cfg)
    for t in range(eo.TRAIN_STEPS + eo.EVAL_STEPS):
        with torch.no_grad():
            xs = np.stack([ref.generate(r, ref.params[r]).numpy() for r in range(cfg.R)])
            own = np.array([float(ref.loss(r, ref.params[r])) for r in range(cfg.R)])
        yield xs, ref.rng_step, own
        if t < eo.TRAIN_STEPS:
            ref.train(1)
        else:
            ref.rng_step += 1


@pytest.mark.parametrize("cid", IDS)
def test_tolerance_is_within_2e_4_of_the_loss_and_losses_are_the_reference(cid):
    """On the committed data with fp64-generated samples, at every step of the schedule: the
    derived tolerance of the fp64 tier is at most 2e-4 of the loss, and ``loss64`` /
    ``rff_loss64`` agree with ``ReferenceTrainer.loss`` to 1e-12 (the Fourier one after the
    fp32 rounding of ``norm``, which the kernels take as an argument)."""
    hip = _hip()
    cfg = eo.CONFIGS[cid]
    D = eb.padded_dim(cfg.d)
    data = np.stack([np.asarray(x, np.float64) for x in cfg.datas()])
    assert np.all(np.abs(data.mean(2)) < 1e-6 * max(cfg.scale, 1e-3)) and len({x.tobytes() for x in data}) == cfg.R
    assert len(set(cfg.keys())) == cfg.R
    worst = 0.0
    for xs, step, own in _reference_steps(cfg):
        if cfg.loss == "rff":
            pad = lambda a: np.concatenate([a, np.zeros((cfg.R, D - cfg.d, cfg.N))], 1)
            W = np.stack([rx.freqs_reference(cfg.keys()[r], step, cfg.k, D, cfg.d)[0] for r in range(cfg.R)])
            L, tol = eo.rff_loss64(pad(xs), pad(data), W, cfg.k)
            # ReferenceTrainer draws the frequencies from the fp64 Philox mirror, whose uniforms keep
            # a half the device rounds away: compare on the same W instead
            from cgnn_amd.engine.reference import rff_mmd_loss
            for r in range(cfg.R):
                ref = float(rff_mmd_loss(torch.as_tensor(xs[r].T.copy()), torch.as_tensor(data[r].T.copy()),
                                         torch.as_tensor(np.concatenate([W[r][:, :cfg.d], W[r][:, D:]], 1).T.copy()),
                                         cfg.k))
                assert abs(L[r] / eo.rff_norm_ratio(cfg.k) - ref) <= 1e-12 * max(1.0, abs(ref))
        else:
            cnt = eo.shadow_counts_host(cfg, hip)
            L = np.array([eo.loss64(xs[r], data[r], cfg.N) for r in range(cfg.R)])
            tol = np.array([eo.loss_tol(xs[r], data[r], cfg, cnt)[0] for r in range(cfg.R)])
            assert np.all(np.abs(L - own) <= 1e-12 * np.maximum(1.0, np.abs(own)))
        assert np.all(L > 0) and np.all(tol > 0)
        worst = max(worst, float((tol / L).max()))
    print("%s: largest tolerance / loss over the schedule %.3e" % (cid, worst))
    assert worst <= eo.REL_CAP


def test_rff_loss64_is_the_reference_trainers_loss_on_its_own_frequencies():
    """With ``rff_frequencies`` (the fp64 mirror ReferenceTrainer uses) as W, rff_loss64 is
    ``ReferenceTrainer.loss`` to 1e-12."""
    from cgnn_amd.engine.reference import rff_frequencies
    cfg = eo.CONFIGS["rff_narrow"]
    ref = eo.reference_trainer(cfg)
    data = np.stack([np.asarray(x, np.float64) for x in cfg.datas()])
    with torch.no_grad():
        xs = np.stack([ref.generate(r, ref.params[r]).numpy() for r in range(cfg.R)])
        own = np.array([float(ref.loss(r, ref.params[r])) for r in range(cfg.R)])
    W = np.stack([rff_frequencies(cfg.keys()[r], 0, cfg.k, cfg.d).numpy().T for r in range(cfg.R)])   # [F, d + 1]
    L, _ = eo.rff_loss64(xs, data, W, cfg.k)
    assert np.all(np.abs(L / eo.rff_norm_ratio(cfg.k) - own) <= 1e-12 * np.maximum(1.0, np.abs(own)))


# ---------------------------------------------------------------------------- positional ABI
def _code(path):
    with open(path) as f:
        return f.read()


def test_engine_create_reads_the_order_device_trainer_builds():
    """icfg / fcfg / ptrs: the table of engine_oracle against (a) the assignments of
    ``cgnn_engine_create``, (b) the fields ``EngineConfig`` / ``EngineBuffers`` declare, (c) the
    lists ``DeviceTrainer.__init__`` builds, and the sizes against the ``PyEngine`` check."""
    src = _code(os.path.join(CSRC, "cgnn_engine.hip"))
    body = src[src.index('extern "C" void* cgnn_engine_create'):src.index('extern "C" void cgnn_engine_destroy')]
    for prefix, arr, names in (("c", "icfg", eo.ICFG), ("c", "fcfg", eo.FCFG), ("b", "ptrs", eo.PTRS)):
        read = re.findall(r"\b%s\.(\w+)\s*=\s*(?:\([^)]*\)\s*)?%s\[(\d+)\]" % (prefix, arr), body)
        assert [int(k) for _, k in read] == list(range(len(names))), arr
        assert tuple(n for n, _ in read) == names, arr
    cfg_fields = re.findall(r"\b(\w+)\s*=\s*[-\w.]+f?\s*[,;]", src[src.index("struct EngineConfig"):src.index("struct EngineBuffers")])
    assert set(cfg_fields) == set(eo.ICFG) | set(eo.FCFG)
    buf_fields = re.findall(r"\*\s*(\w+)\s*=\s*nullptr", src[src.index("struct EngineBuffers"):src.index("class Engine")])
    assert set(buf_fields) == set(eo.PTRS)
    assert (len(eo.ICFG), len(eo.FCFG), len(eo.PTRS)) == (21, 5, 23)
    bind = _code(os.path.join(CSRC, "bindings.cpp"))
    m = re.search(r"icfg\.size\(\) < (\d+) \|\| fcfg\.size\(\) < (\d+) \|\| ptrs\.size\(\) < (\d+)", bind)
    assert m and tuple(int(x) for x in m.groups()) == (21, 5, 23)
    # DeviceTrainer's lists, by the names it uses for the same things
    py = _code(os.path.join(os.path.dirname(eb.__file__), "batch.py"))
    alias = {"self.H": "H", "stride": "prog_stride", "self.hist_len": "hist_stride", "self.rff_k": "rff_k", "d": "d_true",
             "self.NS": "NS", 'int(self.mmd_kernel == "mfma")': "mfma", "self.mirror": "mirror",
             "int(self.staged)": "staged", "sstride": "sched_stride", "self.stage_w": "stage_w",
             "float(learning_rate)": "lr", "0.9": "beta1", "0.999": "beta2", "1e-8": "eps", "float(init_std)": "init_std"}

    def items(name):
        text = re.search(r"\b%s = \[(.*?)\]\n" % name, py, re.S).group(1)
        return tuple(alias.get(x.strip(), x.strip()) for x in re.split(r",\s*(?![^()]*\))", text.replace("\n", " ")))
    assert items("icfg") == eo.ICFG
    assert items("fcfg") == eo.FCFG
    first = re.search(r"ptrs = \[t\.data_ptr\(\) for t in \((.*?)\)\]", py, re.S).group(1)
    names = [x.strip().replace("self.", "") for x in first.replace("\n", " ").split(",")]
    assert re.search(r"ptrs\.append\(self\.hist\.data_ptr\(\) if self\.hist_len else 0\)", py)
    names.append("loss_hist")
    rest = re.search(r"ptrs \+= \[(.*?)\]\n", py, re.S).group(1)
    names += re.findall(r"self\.(\w+)\.data_ptr\(\)", rest)
    assert tuple(names) == eo.PTRS
    assert eo.PTRS[eo.HIST_SLOT] == "loss_hist" and eo.HIST_SLOT == 13
