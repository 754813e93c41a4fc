"""Step-level oracle of the native CGNN engine (cgnn_engine.hip, engine/batch.py).

Shared helper of tests/test_engine_step_exact_cpu.py and tests/test_engine_step_exact_gpu.py;
importing it needs no GPU.

``ShadowEngine`` transcribes the launch sequence documented at the top of cgnn_engine.hip

    init       : init_params
    tt         : mmd(mode 2) | mmd_mfma(mode 2) -> loss_finalize(flags 2)       (exact loss only)
    train step : gen_fwd -> loss(train) -> [loss_finalize(flags 0)] -> gen_bwd -> adam
    eval step  : gen_fwd -> loss(eval)  -> loss_finalize(flags 1)
    chunk      : steps with off = 0 .. n - 1, then advance(n, n | 0)

into calls of the raw ``_hip`` launchers -- each of which has a kernel-level oracle of its own
-- on its own copy of every buffer, eagerly, on its own stream, with its own step counter.  The
counts the engine derives in C++ are derived here a second time, from the header comment of
cgnn_engine.hip and docs/KERNELS.md:

* loss partials of a step: Fourier ``ceil(7k / 256)``; matrix core ``mf_chunks * row_blocks``;
  vector ``n_chunks * row_tiles``.  The true-true pass runs on the vector kernel wherever it
  has a variant for D (``mmd_supported_d``), on the matrix cores (mode 2) only above that, and
  has the partial count of the kernel that ran it.
* gradient slots the generator backward sums: Fourier 1, matrix core ``mf_chunks``, vector
  ``n_chunks + mirror``.
* training mode 0 when a history is recorded, else 3 (no loss); the Fourier kernel has no
  mode 3.  ``gscale = 4 / N^2`` in training, 0 otherwise.
* ``loss_finalize`` scale: 1 for the Fourier loss, ``1 / N^2`` for the exact one.
* generator blocks of ``gpart``: ``staged_tiles(N)`` | ``gen_bwd_blocks(N)``.

The staged generator of the shadow is ``gen_noise`` + ``gen_fwd_staged`` (the engine's forward
draws the noise itself); so in a staged evaluation step the shadow's ``noise`` changes and the
engine's does not.

fp64 tier
---------
``loss64`` / ``rff_loss64`` evaluate the loss of an ``xhat`` snapshot in fp64, ``loss_tol`` /
``rff_loss_tol`` the error the device may have against it (u = 2^-24):

Exact loss, ``L = inv (sum_pp ks - 2 sum_pt ks + tt)``, ``tt = sum_tt ks``, ``inv = 1 / N^2``.
1. Per pair the bound of tests/test_mmd_exact_gpu.py, item 1 (``rbf_terms``): ``dks``.
2. That file's inputs sit on a lattice where ``d2`` is exact.  Here it is not: a pair adds
   ``w(d2) dd2 exp(50 dd2)``, ``w = sum_g g exp(-g d2)``, with
   - vector kernel: ``d2 = sum_k (z_k - p_k)^2``, every difference and square within u, D fused
     adds: ``dd2 = (D + 3) u d2``;
   - matrix cores: ``|x|^2 + |z|^2 - 2 x.z``.  ``xnorm`` within ``2 (d + 1) u |x|^2`` (the generator
     oracle's bound), ``ynorm`` (a torch fp32 sum) within ``(D + 1) u |z|^2``; each operand
     ``hi + lo`` in f16 leaves at most ``2^-22 |x_k| + 2^-25`` (a subnormal lo), three passes drop
     ``lo lo``: ``3 * 2^-22 sum|x_k z_k| + 2^-25 (|x|_1 + |z|_1)``; ``3 KD / 16`` accumulating MFMAs
     of at most two roundings each, three for the combination.  With ``2 |x.z| <= |x|^2 + |z|^2``:
     ``dd2 = (2 (d + 1) + D + 1 + 3 + 12 + 6 KD / 16 + 1) u (|x|^2 + |z|^2) + 2^-24 (|x|_1 + |z|_1)``.
3. Summation (that file's item 2): a term passes at most ``A`` adds in its lane and tile
   (vector: the ``ceil(min(256, N) / 2)`` real column pairs of a tile, padded columns add exact
   zeros; 8 matrix core), one for the pair of packed halves, one per tile of the chunk,
   6 wave and 3 block levels: ``(A + 1 + tpc + 9) u sum|terms|``.
4. ``loss_finalize`` (tests/test_cgnn_gen_exact_gpu.py): ``n_parts u sum|partials|`` for the
   step and for the true-true pass each, two roundings for ``(s + tt) inv``, two for ``inv``
   itself (``(float)N (float)N`` is exact below 2^12, the division and the product round).
``loss_acc`` adds one rounding per evaluation step, ``collect()`` one for the division.

Fourier loss: ``rff_oracle.expected`` on the device's own ``rff_w`` (generic tier, stages
composed: the diff tolerance carried into the loss partials; zero padding dimensions commit no
rounding and are left out of its ``(D + 1) u`` term), plus ``(n_parts + 2) u sum``.

Condition on the committed cases: the tolerance is at most 2e-4 of the loss (what
``test_mmd_loss_and_grad_match_oracle`` allows) at every one of the 5 + 3 steps.  The CPU test
asserts it from ``ReferenceTrainer`` alone.  It fixes the scales: the exact-loss cases hold at
unit scale; the Fourier bound grows with ``(D + 1) u sum_k |w_k x_k|`` of the gamma = 50 block
(rff_oracle's generic tier), so the Fourier cases draw data -- and initial parameters -- of a
small scale (``Config.scale``, ``Config.init_std``), and the wide one a learning rate that keeps
the generated samples at that scale over the five steps (Adam moves a parameter by about lr a
step whatever the gradient's size).  ``mfma_mtt`` halves the data scale: the Gram form's
``dd2`` is relative to ``|x|^2 + |z|^2`` = 140 at d = 70, not to ``d2``, and on the diagonal
of the true-true block (d2 = 0, w = 56.8) that alone is 8.6e-4 of the loss at unit scale.
"""
import functools
import math

import numpy as np

import cgnn_gen_oracle as ox
import rff_oracle as rx
from cgnn_amd.engine import batch as eb
from cgnn_amd.engine.program import compile_program, pack_programs
from cgnn_amd.engine.reference import GAMMAS, ReferenceTrainer, mmd_loss_dense
from cgnn_amd.utils import philox

U = 2.0 ** -24
REL_CAP = 2e-4
TRAIN_STEPS, EVAL_STEPS = 5, 3
SENT = -777.25                       # fill of the buffers a step may leave unwritten
LR, BETA1, BETA2, EPS = 0.01, 0.9, 0.999, 1e-8
H = 8

# the order cgnn_engine_create reads (EngineConfig / EngineBuffers field comments)
ICFG = ("R", "N", "D", "H", "P", "prog_stride", "max_in", "row_tiles", "n_chunks", "tpc", "hist_stride", "rff_k",
        "d_true", "NS", "mfma", "mf_chunks", "mf_tpc", "mirror", "staged", "sched_stride", "stage_w")
FCFG = ("lr", "beta1", "beta2", "eps", "init_std")
PTRS = ("prog", "params", "m", "v", "data", "xhat", "noise", "gradp", "lpart", "gpart", "tt", "loss_last",
        "loss_acc", "loss_hist", "step", "keys", "rff_w", "rff_diff", "xnorm", "ynorm", "dxs", "sched",
        "rff_scratch")
HIST_SLOT = PTRS.index("loss_hist")

# buffers compared bit for bit after every step (names of DeviceTrainer and ShadowEngine alike)
COMPARED = ("params", "m", "v", "xhat", "xnorm", "noise", "gradp", "lpart", "gpart", "tt", "loss_last", "loss_acc",
            "hist", "step", "rff_w", "rff_diff")
# a training step without a history (mode 3) writes exact zeros to its loss partials and leaves
# these untouched; with a history only loss_acc; an evaluation step leaves hist
UNWRITTEN_CHECK = ("lpart", "loss_last")

MUTATIONS = ("adam_no_off", "gen_fwd_no_off", "advance_n_0", "n_parts_minus_1", "n_parts_tt_in_step", "no_mirror",
             "mode0_for_3", "rff_exact_inv", "eval_flag0")


# ---------------------------------------------------------------------------- configurations
def _pairs(h):
    return [compile_program(["X", "Y"], {"Y": ["X"]}, h, observed=["X"]),
            compile_program(["X", "Y"], {"X": ["Y"]}, h, observed=["Y"]),
            compile_program(["X", "Y"], {"Y": ["X"]}, h)]


def _wide3(d):
    return lambda h: [ox.wide(h, d, 3, seed=1), ox.wide(h, d, 2, seed=2), ox.wide(h, d, 3, seed=3)]


def smallest_dx_global(hip, max_in=4, W=2):
    """Smallest variable count whose staged plan keeps dL/dx in global memory (the plan depends
    on H only through the backward chunk width, 12 or 16 units: H is taken as committed)."""
    for d in range(2, 512):
        plan = hip.staged_plan(d, H, max_in, W)
        if plan and plan[2]:
            return d
    raise AssertionError("no dx_global plan below 512 variables")


class Config:
    def __init__(self, id, progs, d, N, gen, loss, k=0, scale=1.0, init_std=0.05, lr=LR, kw=None):
        self.id, self._progs, self.d, self.N, self.gen, self.loss, self.k = id, progs, d, N, gen, loss, k
        self.scale, self.init_std, self.lr, self.kw = scale, init_std, lr, dict(kw or {})
        self.R = 3

    @functools.lru_cache(maxsize=None)
    def programs(self):
        ps = self._progs(H)
        assert len(ps) == self.R and all(p.n_vars == self.d for p in ps)
        return ps

    @functools.lru_cache(maxsize=None)
    def datas(self):
        """[d, N] per model: distinct Gaussian draws, centred per variable, of scale ``scale``."""
        out = []
        for r in range(self.R):
            rng = np.random.default_rng([41, self.d, self.N, r])
            x = rng.standard_normal((self.d, self.N)) * (1.0 + 0.25 * r)
            x -= x.mean(1, keepdims=True)
            out.append((self.scale * x).astype(np.float32))
        return out

    def keys(self):
        return [philox.model_key(29, self.id, r) for r in range(self.R)]

    def trainer_kwargs(self, hist_len, graph_chunk):
        kw = dict(learning_rate=self.lr, init_std=self.init_std, use_fast_mmd=self.loss == "rff", nb_vectors=self.k or 100,
                  record_history=hist_len, graph_chunk=graph_chunk)
        kw.update(self.kw)
        return kw

    def check(self, hip):
        """The preconditions of the branch this case exists for, from the host-side helpers."""
        ps = self.programs()
        d, N, D = self.d, self.N, eb.padded_dim(self.d)
        _, stride, P, max_in = pack_programs(ps)
        assert min(p.n_params for p in ps) < P, "mixed n_params"
        assert len({p.prog.tobytes() for p in ps}) == self.R, "distinct graphs"
        fam = hip.gen_bwd_variant(H, max_in, d, stride)
        if self.gen == "per-sample":
            assert fam == 1 and hip.gen_fwd_lds(D, stride) <= 160 * 1024
        elif self.kw.get("generator") == "staged":
            assert fam == 1 and hip.gen_staged_supported(H, max_in, d), "staged only because it is forced"
        else:
            assert fam == 2
        rt, nc, tpc = eb.mmd_geometry(N)
        rb, mfc, mft = eb.mmd_mfma_geometry(N)
        assert rb == hip.mmd_mfma_row_blocks(N)
        if self.loss == "valu":
            assert hip.mmd_supported_d(D) and D <= eb.MAX_VALU_D
            assert self.kw.get("mmd_kernel") == "valu" or not hip.mmd_mfma_supported(D)
        elif self.loss == "mfma":
            assert hip.mmd_mfma_supported(D)
        c = self.id
        if c == "valu1":
            assert rt == 1 and eb.mmd_mirror_slots(D, N) == 0
        if c == "valu_mirror":
            assert eb.mmd_mirror_slots(D, N) > 0 and eb.mmd_mirror_slots(D, N - 1) == 0, "smallest N with a mirror slot"
        if c == "conf":
            assert max(p.n_conf for p in ps) > 0
        if c == "mfma_vtt":
            assert hip.mmd_supported_d(D) and mfc * rb != nc * rt, "tt on the vector kernel, counts differ"
        if c == "mfma_mtt":
            assert not hip.mmd_supported_d(D), "tt in mode 2 of the matrix-core kernel"
        if c == "staged_dxs":
            W = eb.staged_setup(ps, H, max_in, d, stride)[2]
            assert d == smallest_dx_global(hip, max_in, W), "smallest d with dL/dx in global memory"
        if c == "staged_small":
            assert not eb.staged_setup(ps, H, max_in, d, stride)[3]
        if self.loss == "rff":
            F = 7 * self.k
            assert (F + 255) // 256 >= 1
            assert (D > eb.WIDE_RFF_D) == (c == "rff_wide")


CONFIGS = {c.id: c for c in (
    Config("valu1", _pairs, 2, 65, "per-sample", "valu"),
    Config("valu_mirror", lambda h: [ox.diamond(h), ox.observed5(h), ox.chain(h, 5)], 5, 257, "per-sample", "valu"),
    Config("conf", ox.per_sample_batch, 5, 64, "per-sample", "valu"),
    Config("mfma_vtt", _wide3(10), 10, 130, "per-sample", "mfma"),
    Config("mfma_mtt", _wide3(70), 70, 150, "staged", "mfma", scale=0.5),
    Config("staged_small", _wide3(24), 24, 65, "staged", "valu", kw=dict(generator="staged", mmd_kernel="valu")),
    Config("staged_dxs", _wide3(34), 34, 65, "staged", "mfma"),
    Config("rff_narrow", lambda h: [ox.diamond(h), ox.observed5(h), ox.chain(h, 5)], 5, 65, "per-sample", "rff",
           k=5, scale=0.02, init_std=0.02),
    Config("rff_wide", _wide3(40), 40, 65, "staged", "rff", k=10, scale=0.003, init_std=0.001, lr=1e-4),
)}
MUTATION_CONFIGS = ("valu_mirror", "mfma_vtt", "rff_narrow")


def mutation_applies(mut, cfg):
    return {"n_parts_tt_in_step": cfg.id == "mfma_vtt", "no_mirror": cfg.id == "valu_mirror",
            "mode0_for_3": cfg.loss != "rff", "rff_exact_inv": cfg.loss == "rff"}.get(mut, True)


# ---------------------------------------------------------------------------- the shadow
class ShadowEngine:
    """The engine's launch sequence through the raw launchers.  ``mut``: one of MUTATIONS."""

    def __init__(self, cfg, hist_len, device="cuda", mut=None):
        import torch
        from cgnn_amd import native
        assert mut is None or mut in MUTATIONS
        hip = self.hip = native.hip()
        self.cfg, self.mut, self.hist_len = cfg, mut, int(hist_len)
        progs, datas = cfg.programs(), cfg.datas()
        R, N, d = cfg.R, cfg.N, cfg.d
        D = eb.padded_dim(d)
        self.R, self.N, self.d, self.D = R, N, d, D
        prog, self.ps, self.P, self.max_in = pack_programs(progs)
        self.staged = cfg.gen == "staged"
        if self.staged:
            sched, self.ss, self.W, dxg = eb.staged_setup(progs, H, self.max_in, d, self.ps)
        else:
            sched, self.ss, self.W, dxg = np.zeros((1, 4), np.int32), 4, 8, False
        self.NS = D + max(int(p.n_conf) for p in progs)
        self.row_tiles, self.n_chunks, self.tpc = eb.mmd_geometry(N)
        self.rb, self.mf_chunks, self.mf_tpc = eb.mmd_mfma_geometry(N)
        self.k = cfg.k if cfg.loss == "rff" else 0
        F = self.F = 7 * self.k
        self.mirror = eb.mmd_mirror_slots(D, N) if cfg.loss == "valu" else 0
        valu_parts, mfma_parts = self.n_chunks * self.row_tiles, self.mf_chunks * self.rb
        if cfg.loss == "rff":
            self.n_parts, self.n_parts_tt, self.grad_chunks, self.scale = (F + 255) // 256, 0, 1, 1.0
        else:
            self.scale = float(np.float32(1.0) / (np.float32(N) * np.float32(N)))
            if cfg.loss == "mfma":
                self.tt_mfma = not hip.mmd_supported_d(D)
                self.n_parts, self.grad_chunks = mfma_parts, self.mf_chunks
                self.n_parts_tt = mfma_parts if self.tt_mfma else valu_parts
            else:
                self.tt_mfma = False
                self.n_parts = self.n_parts_tt = valu_parts
                self.grad_chunks = self.n_chunks + self.mirror
        self.G = hip.staged_tiles(N) if self.staged else hip.gen_bwd_blocks(N)
        f32 = dict(dtype=torch.float32, device=device)
        self.prog = torch.from_numpy(prog).to(device)
        data = np.zeros((R, D, N), np.float32)
        for r, x in enumerate(datas):
            data[r, :d] = x
        self.data = torch.from_numpy(data).to(device)
        self.keys = eb._keys_tensor(cfg.keys(), device)
        self.params = eb.param_buffer(R, self.P, device)
        self.m, self.v = torch.zeros(R, self.P, **f32), torch.zeros(R, self.P, **f32)
        self.xhat, self.noise = torch.zeros(R, D, N, **f32), torch.zeros(R, self.NS, N, **f32)
        self.gradp = torch.zeros(max(self.n_chunks + self.mirror, self.mf_chunks, 1), R, D, N, **f32)
        self.lpart = torch.zeros(R, max(valu_parts, mfma_parts, (F + 255) // 256 if F else 0), **f32)
        self.gpart = torch.zeros(R, self.G, self.P, **f32)
        self.sched = torch.from_numpy(sched).to(device)
        self.tt, self.loss_last, self.loss_acc = (torch.zeros(R, **f32) for _ in range(3))
        self.hist = torch.zeros(R, max(self.hist_len, 1), **f32)
        self.step = torch.zeros(2, dtype=torch.int32, device=device)
        self.rff_w, self.rff_diff = torch.zeros(R, max(F, 1), D + 1, **f32), torch.zeros(R, max(F, 1), **f32)
        self.rff_scratch = (torch.zeros(hip.rff_wide_scratch_floats(N, F, R), **f32)
                            if self.k and D > eb.WIDE_RFF_D else None)
        self.xnorm = torch.zeros(R, N, **f32)
        self.ynorm = (self.data * self.data).sum(1).contiguous()
        self.dxs = torch.zeros(R, d, N, **f32) if dxg else None
        self.stream = torch.cuda.Stream(device)
        self.st = self.stream.cuda_stream
        self._torch = torch

    @staticmethod
    def _p(t):
        return t.data_ptr() if t is not None else 0

    def start(self):
        hip, p, st = self.hip, self._p, self.st
        self.step.zero_()
        self.loss_acc.zero_()
        self.stream.wait_stream(self._torch.cuda.current_stream())
        hip.init_params(p(self.params), p(self.m), p(self.v), p(self.prog), self.ps, self.P, p(self.keys),
                        self.cfg.init_std, self.R, st)
        if self.k:
            return
        if self.tt_mfma:
            hip.mmd_mfma(2, self.D, p(self.xhat), p(self.data), p(self.xnorm), p(self.ynorm), p(self.gradp),
                         p(self.lpart), self.N, self.R, self.mf_chunks, self.mf_tpc, 0.0, st)
        else:
            hip.mmd(2, self.D, p(self.xhat), p(self.data), p(self.gradp), p(self.lpart), self.N, self.R,
                    self.row_tiles, self.n_chunks, self.tpc, 0.0, st)
        hip.loss_finalize(p(self.lpart), self.n_parts_tt, p(self.tt), p(self.loss_last), p(self.loss_acc),
                          self.scale, 2, 0, 0, p(self.step), 0, self.R, st)

    def _gen_fwd(self, off):
        hip, p, st = self.hip, self._p, self.st
        if self.staged:
            hip.gen_noise(p(self.prog), self.ps, p(self.keys), p(self.step), off, p(self.noise), self.NS, self.N,
                          self.D, self.d, self.R, 0, st)
            hip.gen_fwd_staged(p(self.prog), self.ps, p(self.sched), self.ss, p(self.params), self.P, p(self.data),
                               p(self.xhat), p(self.noise), self.NS, p(self.xnorm), self.N, self.D, self.d, H,
                               self.max_in, self.R, self.W, st)
        else:
            hip.gen_fwd(p(self.prog), self.ps, p(self.params), self.P, p(self.data), p(self.xhat), p(self.noise),
                        self.NS, p(self.xnorm), p(self.keys), p(self.step), 0 if self.mut == "gen_fwd_no_off" else off,
                        self.N, self.D, H, self.R, st)

    def _loss(self, off, train, need_loss):
        hip, p, st = self.hip, self._p, self.st
        N = self.N
        if self.k:
            hip.rff_freqs(p(self.rff_w), p(self.keys), p(self.step), off, self.k, self.D, 7, self.d, self.R, st)
            hip.rff_fwd_bwd(0 if train else 1, p(self.xhat), p(self.data), p(self.rff_w), p(self.rff_diff),
                            p(self.lpart), p(self.gradp), N, self.D, self.F, self.R, self.k,
                            float(np.sqrt(np.float32(2.0) / np.float32(self.k))), st, 0, p(self.rff_scratch),
                            int(self.rff_scratch is not None))
            return
        mode = (0 if need_loss or self.mut == "mode0_for_3" else 3) if train else 1
        gscale = 4.0 * self.scale if train else 0.0
        if self.cfg.loss == "mfma":
            hip.mmd_mfma(mode, self.D, p(self.xhat), p(self.data), p(self.xnorm), p(self.ynorm), p(self.gradp),
                         p(self.lpart), N, self.R, self.mf_chunks, self.mf_tpc, gscale, st)
        else:
            hip.mmd(mode, self.D, p(self.xhat), p(self.data), p(self.gradp), p(self.lpart), N, self.R, self.row_tiles,
                    self.n_chunks, self.tpc, gscale, st, mirror=1 if train and self.mirror > 0 else 0)

    def _finalize(self, off, flags, hist):
        hip, p = self.hip, self._p
        n = self.n_parts
        if self.mut == "n_parts_minus_1":
            n -= 1
        if self.mut == "n_parts_tt_in_step":
            n = self.n_parts_tt
        inv = (float(np.float32(1.0) / (np.float32(self.N) * np.float32(self.N))) if self.mut == "rff_exact_inv"
               else self.scale)
        hip.loss_finalize(p(self.lpart), n, p(self.tt), p(self.loss_last), p(self.loss_acc), inv, flags,
                          p(self.hist) if hist else 0, self.hist_len if hist else 0, p(self.step), off, self.R,
                          self.st)

    def _train_step(self, off, hist):
        hip, p, st = self.hip, self._p, self.st
        self._gen_fwd(off)
        self._loss(off, True, hist)
        if hist:
            self._finalize(off, 0, True)
        nch = self.grad_chunks - (self.mirror if self.mut == "no_mirror" else 0)
        if self.staged:
            hip.gen_bwd_staged(p(self.prog), self.ps, p(self.sched), self.ss, p(self.params), self.P, p(self.xhat),
                               p(self.noise), self.NS, p(self.gradp), nch, self.R, self.N, self.D, self.d, H,
                               self.max_in, self.W, p(self.gpart), p(self.dxs), st)
        else:
            hip.gen_bwd(p(self.prog), self.ps, p(self.params), self.P, p(self.xhat), p(self.noise), self.NS,
                        p(self.gradp), nch, self.R, self.N, self.D, self.d, H, self.max_in, p(self.gpart), st)
        hip.adam(p(self.params), p(self.m), p(self.v), p(self.gpart), self.G, p(self.prog), self.ps, self.P,
                 p(self.step), 0 if self.mut == "adam_no_off" else off, self.cfg.lr, BETA1, BETA2, EPS, self.R, st)

    def _eval_step(self, off):
        self._gen_fwd(off)
        self._loss(off, False, True)
        self._finalize(off, 0 if self.mut == "eval_flag0" else 1, False)

    def run(self, kind, steps):
        """One eager chunk of ``steps`` steps (0 train, 1 eval) and its advance node."""
        hist = self.hist_len > 0
        for k in range(steps):
            if kind == 0:
                self._train_step(k, hist)
            else:
                self._eval_step(k)
        d_opt = steps if kind == 0 and self.mut != "advance_n_0" else 0
        self.hip.advance(self._p(self.step), steps, d_opt, self.st)

    def sync(self):
        self.stream.synchronize()


def snapshot(obj):
    """Host copies (int32 bit patterns) of every compared buffer of a trainer or a shadow."""
    out = {}
    for name in COMPARED:
        t = getattr(obj, name)
        if name == "hist":
            t = t[:, :obj.hist_len]
        if name == "params":
            t = t.contiguous()
        a = t.detach().cpu().numpy()
        out[name] = a.view(np.int32).copy() if a.dtype == np.float32 else a.copy()
    return out


def differing(a, b):
    """Names of the buffers of two snapshots that are not the same bits."""
    return [n for n in COMPARED if a[n].shape != b[n].shape or not np.array_equal(a[n], b[n])]


def f32view(snap, name):
    return snap[name].view(np.float32)


def stored_noise_rows(prog, D, NS):
    """Rows of ``noise`` a drawing forward stores: generated variables and the streams they use."""
    rows = np.zeros(NS, bool)
    for var, kind, pars, confs, poff, nin in prog.node_records():
        if kind != 1:
            rows[var] = True
            rows[[D + c for c in confs]] = True
    return rows


# ---------------------------------------------------------------------------- fp64 losses
def _d2(x, z):
    return np.maximum((x * x).sum(0)[:, None] + (z * z).sum(0)[None, :] - 2.0 * (x.T @ z), 0.0)


def loss64(xhat, data, N):
    """Exact multi-bandwidth MMD^2 of one model's snapshot ([d, N] each), fp64."""
    import torch
    pred = torch.as_tensor(np.asarray(xhat, np.float64)[:, :N].T.copy())
    true = torch.as_tensor(np.asarray(data, np.float64)[:, :N].T.copy())
    return float(mmd_loss_dense(pred, true))


def tt64(data):
    y = np.asarray(data, np.float64)
    return float(sum(np.exp(-g * _d2(y, y)).sum() for g in GAMMAS))


def _block_tol(x, z, kernel, d, D):
    """(sum ks, pair error) of one block of the loss on ``kernel`` ('valu' | 'mfma')."""
    from test_mmd_exact_gpu import rbf_terms
    d2 = _d2(x, z)
    ks, w, dks, dw = rbf_terms(d2, np.ones_like(d2, bool))
    if kernel == "valu":
        dd2 = (D + 3) * U * d2
    else:
        KD = (D + 15) // 16 * 16
        c = 2 * (d + 1) + (D + 1) + 3 + 12 + 6 * KD // 16 + 1
        n2 = (x * x).sum(0)[:, None] + (z * z).sum(0)[None, :]
        n1 = np.abs(x).sum(0)[:, None] + np.abs(z).sum(0)[None, :]
        dd2 = c * U * n2 + 2.0 ** -24 * n1
    return ks.sum(), (dks + w * dd2 * np.exp(50.0 * dd2)).sum()


def loss_tol(xhat, data, cfg, shadow_counts):
    """(tolerance of the step's loss, tolerance of tt) of one model; ``shadow_counts`` =
    (n_parts, n_parts_tt, tpc of the step, tpc of the tt pass, tt on the matrix cores)."""
    n_parts, n_parts_tt, tpc, tpc_tt, tt_mfma = shadow_counts
    d, D, N = cfg.d, eb.padded_dim(cfg.d), cfg.N
    x, y = np.asarray(xhat, np.float64)[:d], np.asarray(data, np.float64)[:d]
    spp, epp = _block_tol(x, x, cfg.loss, d, D)
    spt, ept = _block_tol(x, y, cfg.loss, d, D)
    stt, ett = _block_tol(y, y, "mfma" if tt_mfma else "valu", d, D)
    A_valu = (min(256, N) + 1) // 2
    A = A_valu if cfg.loss == "valu" else 8
    A_tt = 8 if tt_mfma else A_valu
    s_step = spp + 2 * spt
    tol_step = epp + 2 * ept + (A + 1 + tpc + 9 + n_parts) * U * s_step
    tol_tt = ett + (A_tt + 1 + tpc_tt + 9 + n_parts_tt) * U * stt
    inv = 1.0 / (N * N)
    L = inv * (spp - 2 * spt + stt)
    return inv * (tol_step + tol_tt + 2 * U * (s_step + stt)) + 3 * U * abs(L), tol_tt


def _rff_case(xhat, data, W, k):
    c = rx.Case()
    c.R, c.D, c.N = xhat.shape
    c.k, c.F, c.exact, c.pad, c.da, c.big = k, 7 * k, False, 0, c.D, []
    c.P, c.T, c.W = np.asarray(xhat, np.float64), np.asarray(data, np.float64), np.asarray(W, np.float64)
    return c


def rff_loss64(xhat, data, W, k):
    """(loss [R], tolerance [R]) of the Fourier loss of snapshots [R, D, N] on the frequencies
    ``W [R, F, D + 1]`` (the device's own ``rff_w``); ``norm = sqrt(2 / k)`` as the fp32 the
    kernels take."""
    D = xhat.shape[1]
    form = rx.form_of(D, 7 * k, force_wide=int(D > eb.WIDE_RFF_D))
    # the padded dimensions are exact zeros in x and W: they commit no rounding to theta, so the
    # (D + 1) u term of rff_oracle counts the live dimensions only
    live = np.flatnonzero(np.abs(np.asarray(W)[:, :, :D]).sum((0, 1)) + np.abs(xhat).sum((0, 2)) + np.abs(data).sum((0, 2)))
    keep = np.concatenate([live, [D]])
    c = _rff_case(np.asarray(xhat)[:, live], np.asarray(data)[:, live], np.asarray(W)[:, :, keep], k)
    loss, tol = np.zeros(c.R), np.zeros(c.R)
    for r in range(c.R):
        e = rx.expected(c, r, form, plain=True)
        loss[r] = e.loss.sum()
        tol[r] = e.loss_tol.sum() + (len(e.loss) + 2) * U * np.abs(e.loss).sum()
    return loss, tol


def rff_norm_ratio(k):
    """(fp32 sqrt(2 / k))^2 over 2 / k: rff_loss64 over engine.reference.rff_mmd_loss."""
    return (float(rx.norm_of(k)) / math.sqrt(2.0 / k)) ** 2


def shadow_counts_host(cfg, hip):
    """loss_tol's count tuple from the host-side helpers alone (the CPU test)."""
    N, D = cfg.N, eb.padded_dim(cfg.d)
    rt, nc, tpc = eb.mmd_geometry(N)
    rb, mfc, mft = eb.mmd_mfma_geometry(N)
    if cfg.loss == "mfma":
        tt_mfma = not hip.mmd_supported_d(D)
        return mfc * rb, mfc * rb if tt_mfma else nc * rt, mft, mft if tt_mfma else tpc, tt_mfma
    return nc * rt, nc * rt, tpc, tpc, False


def reference_trainer(cfg):
    return ReferenceTrainer(cfg.programs(), cfg.datas(), cfg.keys(), H, learning_rate=cfg.lr, init_std=cfg.init_std,
                            use_fast_mmd=cfg.loss == "rff", nb_vectors=cfg.k or 100)
