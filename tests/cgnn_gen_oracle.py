"""fp64 oracle, fp32 emulation and error bounds of the CGNN generator / Adam kernels.

Plain helper of tests/test_cgnn_gen_exact_cpu.py and tests/test_cgnn_gen_exact_gpu.py: it
interprets a ``Program`` in numpy and knows nothing of the device.

Layouts (cgnn_kernels.hip): a generated node owns ``W1[nin][H], b1[H], W2[H], b2`` at its
``param_off``; its inputs are ``[parents..., own noise, confounder streams...]``; ``gpart``
has the same layout per (model, sample block).

Bounds (u = 2^-24)
------------------
* forward, one node from the kernel's own inputs: ``2 (nin + H + 2) u S`` with
  ``S = |b2| + sum_q |W2_q| (|b1_q| + sum_j |W1_jq x_j|)`` -- nin + 1 fused multiply-adds per
  unit, H + 1 for the output, each within u of the running magnitude, doubled for the
  rounding of the stored inputs; ``xnorm``: ``2 (d + 1) u sum_v x_v^2``.
* backward: the same backprop on absolute values with the fp64 ReLU masks kept (a running
  majorant A of every sum the kernel forms: ``dL/dx`` through ``|W1| |W2|``, ``dW2`` through
  ``|b1| + sum_j |W1_j| |x_j|`` because the kernels form it as ``sum_j W1ext_j Gm_j``), times
  ``K u``, ``K = block_samples + depth (max_in + H + 4)``: one rounding per sample of the
  block sum, and per level of the DAG the H + 1 roundings of a ``dL/dparent`` push, the
  n_chunks adds and the max_in + 1 terms of the ``dW2`` contraction.
* ReLU masks: every pre-activation of the committed backward inputs is an odd multiple of
  2^-7 by construction (``backward_inputs``), far outside ``64 u sum|terms|`` of zero and
  exact in fp32, so fp32 and fp64 masks agree; ``relu_margin_ok`` checks exactly that.
* Adam: fp32 numpy in the kernel's order (contraction off); ``lr_t`` apart, see
  ``adam_reference``.
"""
import numpy as np

from cgnn_amd.engine.program import compile_program
from cgnn_amd.utils import philox

U = 2.0 ** -24
COMPILED_H = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 30, 32, 40, 48, 50, 64)
LDS_MAX = 160 * 1024


# ---------------------------------------------------------------------------- programs
def diamond(H):
    n = list("abcde")
    return compile_program(n, {"b": ["a"], "c": ["a"], "d": ["b", "c"], "e": ["d"]}, H)


def chain(H, d=4):
    n = ["v%d" % k for k in range(d)]
    return compile_program(n, {n[k]: [n[k - 1]] for k in range(1, d)}, H)


def pair(H):
    return compile_program(["X", "Y"], {"Y": ["X"]}, H, observed=["X"])


def observed5(H):
    """Five variables, the cause observed: X -> Y, (Y, X) -> Z (parents swapped on purpose), U -> V."""
    n = ["X", "Y", "Z", "U", "V"]
    return compile_program(n, {"Y": ["X"], "Z": ["Y", "X"], "V": ["U"]}, H, observed=["X"])


def confounded5(H):
    """Five variables, three confounder streams, every stream used (NS = D + 3 > D)."""
    n = list("abcde")
    return compile_program(n, {"b": ["a"], "c": ["a", "b"], "e": ["c"]}, H,
                           confounders={"a": [0, 1], "b": [0, 2], "c": [1], "d": [2, 1], "e": [2]}, n_conf=3)


def confounded4(H):
    n = list("abcd")
    return compile_program(n, {"b": ["a"], "c": ["b"], "d": ["a", "c"]}, H,
                           confounders={"a": [0], "b": [0, 1], "c": [1], "d": [1, 0]}, n_conf=2)


def split_max_in(H):
    """Largest node input count whose reduction takes the two-wave split (n_items <= 64)."""
    hp = ((H + 1) & ~1) // 2
    return 63 // hp - 1


def fan(H):
    """Roots and two children whose input counts sit on both sides of n_items = 64 for H
    (H = 64: the split is unreachable, one two-input child)."""
    m = max(split_max_in(H), 1)
    roots = ["r%d" % k for k in range(m)]
    par = {"B": roots}                           # nin = m + 1: loops over the block
    nodes = roots + ["B"]
    if m >= 2:
        par["A"] = roots[:m - 1]                 # nin = m: split
        nodes.append("A")
    return compile_program(nodes, par, H)


def wide(H, d=34, max_par=3, seed=0, big=0, conf=False):
    """Random DAG of d variables for the level-scheduled kernels; ``big``: one node with that
    many parents; ``conf``: four confounder streams on the first eight nodes."""
    rng = np.random.default_rng([seed, d, max_par, big])
    n = ["v%d" % k for k in range(d)]
    par = {}
    for k in range(1, d):
        m = int(rng.integers(0, min(k, max_par) + 1))
        par[n[k]] = [n[i] for i in rng.choice(k, m, replace=False)]
    if big:
        par[n[d - 2]] = [n[i] for i in rng.permutation(d - 2)[:big]]
    cf = {n[k]: [k % 4, (k + 1) % 4][:1 + k % 2] for k in range(8)} if conf else None
    return compile_program(n, par, H, confounders=cf, n_conf=4 if conf else 0)


def depth_of(prog):
    lv = {}
    for var, kind, pars, confs, poff, nin in prog.node_records():
        lv[var] = 0 if kind == 1 or not pars else 1 + max(lv[p] for p in pars)
    return 1 + max(lv.values())


# ---------------------------------------------------------------------------- inputs
def forward_params(progs, P, seed):
    rng = np.random.default_rng([seed, 11])
    th = np.zeros((len(progs), P), np.float32)
    for r, p in enumerate(progs):
        th[r, :p.n_params] = rng.normal(0, 0.6, p.n_params)
    return th


def backward_inputs(progs, H, P, D, NS, N, n_slots, seed):
    """params [R, P], xhat [R, D, N], noise [R, NS, N], gradp [n_slots, R, D, N], all fp32.
    W1, xhat and noise are multiples of 1/8 and b1 an odd multiple of 1/128: every
    pre-activation is an odd multiple of 1/128, computed exactly in fp32.  W2, b2 and the
    incoming gradients are continuous."""
    R = len(progs)
    rng = np.random.default_rng([seed, H, N, 7])
    th = np.zeros((R, P), np.float32)
    for r, p in enumerate(progs):
        for var, kind, pars, confs, poff, nin in p.node_records():
            if kind == 1:
                continue
            th[r, poff:poff + nin * H] = rng.integers(-8, 9, nin * H) / 8.0
            th[r, poff + nin * H:poff + (nin + 1) * H] = (2 * rng.integers(-24, 24, H) + 1) / 128.0
            th[r, poff + (nin + 1) * H:poff + (nin + 2) * H + 1] = rng.normal(0, 0.7, H + 1)
    xhat = (rng.integers(-16, 17, (R, D, N)) / 8.0).astype(np.float32)
    noise = (rng.integers(-16, 17, (R, NS, N)) / 8.0).astype(np.float32)
    gradp = (rng.normal(0, 1e-3, (n_slots, R, D, N))).astype(np.float32)
    return th, xhat, noise, gradp


# ---------------------------------------------------------------------------- fp32 helpers
def f32(x):
    return np.asarray(x, np.float32)


def fma32(a, b, c):
    """fmaf on fp32 arrays (one rounding; the double product is exact)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def node_inputs(D, var, pars, confs, xhat, noise, mut=None):
    """[nin, N] input rows of a node: parents from xhat, own noise, confounder streams."""
    pars = list(pars)
    if mut == "swap_parents" and len(pars) >= 2:
        pars[0], pars[1] = pars[1], pars[0]
    cf = [D + c + (1 if mut == "conf_shift" else 0) for c in confs]
    rows = [xhat[p] for p in pars] + [noise[var]] + [noise[c] for c in cf]
    return np.stack(rows, 0)


def unpack(theta, poff, nin, H):
    W1 = theta[poff:poff + nin * H].reshape(nin, H)
    b1 = theta[poff + nin * H:poff + (nin + 1) * H]
    W2 = theta[poff + (nin + 1) * H:poff + (nin + 2) * H]
    return W1, b1, W2, theta[poff + (nin + 2) * H]


# ---------------------------------------------------------------------------- forward
def forward_oracle(prog, H, theta, D, xhat, noise, data):
    """Every node from the kernel's own inputs (its parents in ``xhat``, its ``noise``), fp64:
    (value [d, N], bound [d, N], observed mask [d]); plus xnorm and its bound."""
    d, N = prog.n_vars, xhat.shape[1]
    th = theta.astype(np.float64)
    X, Z = xhat.astype(np.float64), noise.astype(np.float64)
    val, bnd, obs = np.zeros((d, N)), np.zeros((d, N)), np.zeros(d, bool)
    for var, kind, pars, confs, poff, nin in prog.node_records():
        if kind == 1:
            val[var], obs[var] = data[var], True
            continue
        W1, b1, W2, b2 = unpack(th, poff, nin, H)
        inp = node_inputs(D, var, pars, confs, X, Z)                       # [nin, N]
        pre = b1[:, None] + W1.T @ inp
        val[var] = W2 @ np.maximum(pre, 0.0) + b2
        S = abs(b2) + np.abs(W2) @ (np.abs(b1)[:, None] + np.abs(W1).T @ np.abs(inp))
        bnd[var] = 2 * (nin + H + 2) * U * S
    order = [rec[0] for rec in prog.node_records()]
    xn = (X[order] ** 2).sum(0)
    return val, bnd, obs, xn, 2 * (d + 1) * U * xn


def forward_emulate(prog, H, theta, D, noise, data, mut=None):
    """gen_fwd_kernel in fp32, in its order (own noise + bias, parents, confounders; W2 chain)."""
    d, N = prog.n_vars, noise.shape[1]
    x = np.zeros((D, N), np.float32)
    for var, kind, pars, confs, poff, nin in prog.node_records():
        if kind == 1:
            x[var] = data[var]
            continue
        W1, b1, W2, b2 = unpack(theta, poff, nin, H)
        inp = node_inputs(D, var, pars, confs, x, noise, mut)
        npar = len(pars)
        out = np.full(N, b2, np.float32)
        for q in range(H):
            a = fma32(W1[npar, q], inp[npar], b1[q])
            for j in list(range(npar)) + list(range(npar + 1, nin)):
                a = fma32(W1[j, q], inp[j], a)
            out = fma32(W2[q], np.maximum(a, np.float32(0)), out)
        x[var] = out
    nrm = np.zeros(N, np.float32)
    for rec in prog.node_records():
        nrm = fma32(x[rec[0]], x[rec[0]], nrm)
    return x, nrm


# ---------------------------------------------------------------------------- backward
def relu_margin_ok(prog, H, theta, D, xhat, noise):
    """No pre-activation within 64 u sum|terms| of zero (fp64), for exactly these inputs."""
    th, X, Z = theta.astype(np.float64), xhat.astype(np.float64), noise.astype(np.float64)
    for var, kind, pars, confs, poff, nin in prog.node_records():
        if kind == 1:
            continue
        W1, b1, W2, b2 = unpack(th, poff, nin, H)
        inp = node_inputs(D, var, pars, confs, X, Z)
        pre = b1[:, None] + W1.T @ inp
        mag = np.abs(b1)[:, None] + np.abs(W1).T @ np.abs(inp)
        if not np.all(np.abs(pre) > 64 * U * mag):
            return False
    return True


def backward_oracle(prog, H, theta, D, xhat, noise, gradp, BS, P):
    """fp64 backprop per block of BS samples from the kernel's inputs (gradp [n_chunks, D, N]):
    (gpart [G, P], majorant [G, P], written [P])."""
    d, N = prog.n_vars, xhat.shape[1]
    G = (N + BS - 1) // BS
    th, X, Z = theta.astype(np.float64), xhat.astype(np.float64), noise.astype(np.float64)
    g = gradp.astype(np.float64).sum(0)[:d].copy()
    ga = np.abs(gradp.astype(np.float64)).sum(0)[:d].copy()
    out, maj, written = np.zeros((G, P)), np.zeros((G, P)), np.zeros(P, bool)
    edges = np.arange(0, N, BS)
    blk = lambda a: np.add.reduceat(a, edges, axis=-1)                     # [..., G]
    for var, kind, pars, confs, poff, nin in reversed(list(prog.node_records())):
        if kind == 1:
            continue
        W1, b1, W2, b2 = unpack(th, poff, nin, H)
        inp = node_inputs(D, var, pars, confs, X, Z)
        pre = b1[:, None] + W1.T @ inp                                     # [H, N]
        apre = np.abs(b1)[:, None] + np.abs(W1).T @ np.abs(inp)
        mask = pre > 0
        mg, mga = mask * g[var], mask * ga[var]                            # [H, N]
        ext = np.concatenate([inp, np.ones((1, N))], 0)                    # [nin + 1, N]
        n1 = (nin + 1) * H
        for b in range(G):
            s = slice(b * BS, min(N, (b + 1) * BS))
            out[b, poff:poff + n1] = ((ext[:, s] @ mg[:, s].T) * W2).ravel()
            maj[b, poff:poff + n1] = ((np.abs(ext[:, s]) @ mga[:, s].T) * np.abs(W2)).ravel()
        out[:, poff + n1:poff + n1 + H] = blk(np.maximum(pre, 0) * g[var]).T
        maj[:, poff + n1:poff + n1 + H] = blk(mask * apre * ga[var]).T
        out[:, poff + n1 + H] = blk(g[var])
        maj[:, poff + n1 + H] = blk(ga[var])
        written[poff:poff + n1 + H + 1] = True
        for j, p in enumerate(pars):
            g[p] += (W1[j] * W2) @ mg
            ga[p] += (np.abs(W1[j]) * np.abs(W2)) @ mga
    return out, maj, written


def backward_K(BS, depth, max_in, H):
    return BS + depth * (max_in + H + 4)


def _seqsum(a, z, split):
    """sum_s a[..., s] z[..., s] in fp32 the way gen_bwd_kernel's item() does: two fma chains
    over even / odd samples, per wave half when ``split``; a, z padded to the block."""
    def chain(a, z):
        acc0 = np.zeros(a.shape[:-1], np.float32)
        acc1 = np.zeros(a.shape[:-1], np.float32)
        for s in range(0, a.shape[-1], 2):
            acc0 = fma32(a[..., s], z[..., s], acc0)
            acc1 = fma32(a[..., s + 1], z[..., s + 1], acc1)
        return f32(acc0 + acc1)
    if split:
        return f32(chain(a[..., :64], z[..., :64]) + chain(a[..., 64:], z[..., 64:]))
    return chain(a, z)


def backward_emulate(prog, H, theta, D, xhat, noise, gradp, BS, P, mut=None):
    """The kernels' backward in fp32: chunk sum in order, per-unit fma chains, the block
    reduction in gen_bwd_kernel's item order (BS = 128; a 64-sample tile sums as one chain
    pair), dW2 from the Gm rows.  ``mut`` names one deliberate error (CPU mutation tests)."""
    d, N = prog.n_vars, xhat.shape[1]
    G = (N + BS - 1) // BS
    NP = G * BS
    pad = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (NP - N,), np.float32)], -1)
    chunks = gradp[:-1] if mut == "omit_chunk" else gradp
    g = np.zeros((d, N), np.float32)
    for c in range(chunks.shape[0]):
        g = f32(g + chunks[c, :d])
    g = pad(g)
    X, Z = pad(f32(xhat)), pad(f32(noise))
    out = np.zeros((G, P), np.float32)
    first = True
    for var, kind, pars, confs, poff, nin in reversed(list(prog.node_records())):
        if kind == 1:
            continue
        W1, b1, W2, b2 = unpack(f32(theta), poff, nin, H)
        inp = node_inputs(D, var, pars, confs, X, Z, mut)
        inp[:, N:] = 0
        pre = np.repeat(b1[:, None], NP, 1)
        for j in range(nin):
            pre = fma32(W1[j][:, None], inp[j][None, :], pre)
        mask = pre > 0
        if mut == "flip_mask" and first:
            mask[0, 0] = ~mask[0, 0]
        mg = f32(mask * g[var])
        for j, p in enumerate(pars):
            s = np.zeros(NP, np.float32)
            for q in range(H):
                s = fma32(f32(W1[j, q] * W2[q]), mg[q], s)
            g[p] = f32(g[p] + s)
        ext = np.concatenate([inp, np.ones((1, NP), np.float32), g[var][None]], 0)   # rows nin: 1, nin + 1: g
        mgr = mg.copy()
        gr = ext[nin + 1].copy()
        if mut == "drop_sample" and first:
            mgr[:, min(3, N - 1)] = 0
            gr[min(3, N - 1)] = 0
        HP = ((H + 1) & ~1) // 2
        split = BS == 128 and (nin + 1) * HP + 1 <= 64
        n1 = (nin + 1) * H
        for b in range(G):
            s = slice(b * BS, (b + 1) * BS)
            Gm = _seqsum(ext[:nin + 1, None, s], mgr[None, :, s], split)              # [nin + 1, H]
            out[b, poff:poff + n1] = f32(W2[None, :] * Gm).ravel()
            W1e = np.concatenate([W1, b1[None]], 0)
            if mut == "b1_row":
                W1e[0] = b1
            acc = np.zeros(H, np.float32)
            for j in range(nin + 1):
                acc = fma32(W1e[j], Gm[j], acc)
            out[b, poff + n1:poff + n1 + H] = acc
            out[b, poff + n1 + H] = _seqsum(np.ones(BS, np.float32)[None], gr[None, s], split)[0]
        first = False
    return out


# ---------------------------------------------------------------------------- noise / init
def u01_f32(x):
    """The device's ``u01`` as it is computed, in fp32: ``(float)(x >> 8) + 0.5f`` rounds to
    even from 2^23 on (the fp64 mirror in utils/philox.py keeps the half), so the device's
    uniform is up to 2^-25 off the mirror's -- which moves a draw with u1 near 1 (a small
    Box-Muller radius) by far more than the transcendentals do."""
    h = (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32) + np.float32(0.5)
    return (h * np.float32(1.0 / 16777216.0)).astype(np.float64)


def normal_reference(key, a, b, step, purpose):
    """(draw, radius) in fp64 from the device's fp32 uniforms: the integer part and the
    uniforms are bit-exact, only log2 / sqrt / cos are left to differ."""
    r0, r1, _, _ = philox.philox4x32_10(a, b, step, purpose, key[0], key[1])
    rad = np.sqrt(-2.0 * np.log(u01_f32(r0)))
    return rad * np.cos(2.0 * np.pi * u01_f32(r1)), rad


def noise_reference(prog, key, D, N, row0, step):
    """(rows, values [len(rows), N], radius [len(rows), N]) of every stream a forward of
    ``prog`` draws: its generated variables and the confounder ids it uses."""
    n = (np.arange(N, dtype=np.int64) + row0).astype(np.uint32)
    rows, vals, rads = [], [], []
    used = set()
    for var, kind, pars, confs, poff, nin in prog.node_records():
        if kind == 1:
            continue
        z, rad = normal_reference(key, n, var, step, philox.RNG_NODE_NOISE)
        rows.append(var), vals.append(z), rads.append(rad)
        for c in confs:
            if c not in used:
                used.add(c)
                z, rad = normal_reference(key, n, c, step, philox.RNG_CONF_NOISE)
                rows.append(D + c), vals.append(z), rads.append(rad)
    return np.array(rows), np.stack(vals), np.stack(rads)


def normal_units(dev, ref, rad):
    """|device - reference| in units of u * radius: the device's log2 and cosine (in
    revolutions) are hardware approximations with an absolute error, so the error of a draw
    scales with its Box-Muller radius, not with the draw.  A zero radius (u1 rounded to 1)
    must give an exact zero."""
    err = np.abs(dev.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(rad > 0, err / (U * rad), np.where(err > 0, np.inf, 0.0))


# ---------------------------------------------------------------------------- Adam
def adam_reference(params, m, v, gpart, Pr, t, lr, b1, b2, eps, mut=None):
    """adam_tf1_kernel on [P] params/m/v and gpart [G, P] in numpy fp32, in its order with no
    contraction; padding [Pr, P) untouched.  Returns (params, m, v, lr_t, step) where
    ``params_new = params - step`` on [0, Pr) and ``step = lr_t m / (sqrt(v) + eps)``."""
    one = np.float32(1)
    b1, b2, lr, eps = np.float32(b1), np.float32(b2), np.float32(lr), np.float32(eps)
    g = np.zeros(params.shape, np.float32)
    for k in range(gpart.shape[0]):
        g = f32(g + gpart[k])
    tt = t - 1 if mut == "beta2_t-1" else t
    p2 = np.float32(np.float64(b2) ** tt)
    p1 = np.float32(np.float64(b1) ** t)
    lr_t = f32(f32(lr * np.sqrt(f32(one - p2))) / f32(one - p1))
    mn = f32(f32(b1 * m) + f32(f32(one - b1) * g))
    vn = f32(f32(b2 * v) + f32(f32(f32(one - b2) * g) * g))
    live = np.arange(params.size) < Pr
    with np.errstate(invalid="ignore"):
        step = f32(f32(lr_t * mn) / f32(np.sqrt(vn) + eps))
        pn = np.where(live, f32(params - step), params)
    return pn, np.where(live, mn, m), np.where(live, vn, v), lr_t, step


def adam_oracle64(params, m, v, gpart, Pr, t, lr, b1, b2, eps):
    """fp64 TF1 Adam over the fixed-order slab sum: (params, m, v, bounds of each)."""
    f = np.float64
    b1, b2, lr, eps = f(np.float32(b1)), f(np.float32(b2)), f(np.float32(lr)), f(np.float32(eps))
    G = gpart.shape[0]
    g = gpart.astype(f).sum(0)
    ga = np.abs(gpart.astype(f)).sum(0)
    lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    mn = b1 * m + (1 - b1) * g
    vn = b2 * v + (1 - b2) * g * g
    dm = (G + 3) * U * (b1 * np.abs(m) + (1 - b1) * ga)
    dv = (2 * G + 4) * U * (b2 * np.abs(v) + (1 - b2) * ga * ga)
    step = lr_t * mn / (np.sqrt(vn) + eps)
    # relative: lr_t (lr_t_rel: the cancellation in 1 - beta^t at small t is fp32's own), m as
    # above, sqrt(v) half of v's relative error, four more roundings; where v ~ 0 eps dominates
    den = np.sqrt(vn) + eps
    dstep = np.abs(step) * (lr_t_rel(t, b1, b2) + 4 * U) + lr_t * dm / den + lr_t * np.abs(mn) * (0.5 * dv / np.maximum(np.sqrt(vn), 1e-300)) / den ** 2
    live = np.arange(params.size) < Pr
    pn = np.where(live, params - step, params)
    dp = np.where(live, dstep + U * np.abs(pn), 0.0)
    return pn, np.where(live, mn, m), np.where(live, vn, v), dp, np.where(live, dm, 0), np.where(live, dv, 0)


def lr_t_rel(t, b1, b2):
    """Relative error of the fp32 ``lr sqrt(1 - b2^t) / (1 - b1^t)``: each power within 3 u
    (powf 2 ulp and the subtraction), amplified by the cancellation against 1, half of it
    through the square root; sqrtf, the product and the division 4 u more."""
    p1, p2 = b1 ** t, b2 ** t
    return 4 * U + 0.5 * 3 * U * (1 + p2) / (1 - p2) + 3 * U * (1 + p1) / (1 - p1)


# ---------------------------------------------------------------------------- LDS mirrors
def staged_cw(H):
    return 12 if (H + 11) // 12 == (H + 15) // 16 else 16


def staged_bwd_lds(Dt, W, H, max_in, xg, dg):
    """cgnn_staged.hip bwd_lds: bytes of a backward block of W waves."""
    cw = staged_cw(H)
    si = (max_in + 2) | 1
    slab = 64 * (si + 1) + 64 * (cw + 2) + (max_in + 2) * 16 + (0 if max_in <= 17 else max_in * 64)
    return 4 * ((0 if xg else Dt * 64) + (0 if dg else Dt * 64) + W * slab)


def staged_fwd_hc(H):
    for c in (32, 20, 16, 12, 10, 8, 6, 5, 4, 3, 2, 1):
        if H % c == 0:
            return c


def staged_fwd_lds(Dt, W, H, max_in, xg):
    hcs = (staged_fwd_hc(H) + 3) & ~3
    return 4 * ((0 if xg else Dt * 64) + W * (max_in + 2) * hcs)


# ---------------------------------------------------------------------------- committed cases
BWD_N = (1, 63, 64, 65, 128, 129, 257)
STAGED_H = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 32, 36)       # every fwd_hc value, CW 12 and 16
STAGED_N = (1, 64, 65, 150)
STAGED_W = (1, 2, 8)


class Case:
    pass


def make_case(progs, H, N, n_chunks, seed=0, extra_noise_rows=0):
    """Packed batch + committed backward inputs of a list of programs (one variable count)."""
    from cgnn_amd.engine.batch import padded_dim
    from cgnn_amd.engine.program import pack_programs
    c = Case()
    c.progs, c.H, c.N, c.n_chunks, c.R = progs, H, N, n_chunks, len(progs)
    c.d = progs[0].n_vars
    assert all(p.n_vars == c.d for p in progs)
    c.D = padded_dim(c.d)
    c.prog, c.ps, c.P, c.max_in = pack_programs(progs)
    c.NS = c.D + max(p.n_conf for p in progs) + extra_noise_rows
    c.depth = max(depth_of(p) for p in progs)
    c.theta, c.xhat, c.noise, c.gradp = backward_inputs(progs, H, c.P, c.D, c.NS, N, n_chunks, seed)
    return c


def per_sample_batch(H):
    return [diamond(H), observed5(H), confounded5(H)]


def per_sample_bwd_cases():
    """(kind, H, N, n_chunks): every compiled H at every N of BWD_N on the three-program
    batch (n_chunks alternating 1 / 3), and the fan program of H (node input counts on both
    sides of n_items = 64) at one and at two blocks."""
    out = []
    for i, H in enumerate(COMPILED_H):
        for k, N in enumerate(BWD_N):
            out.append(("batch", H, N, 1 + 2 * ((i + k) % 2)))
        out.append(("fan", H, 65, 3))
        out.append(("fan", H, 129, 1))
    return out


def per_sample_case(kind, H, N, n_chunks):
    progs = per_sample_batch(H) if kind == "batch" else [fan(H)] * 2
    return make_case(progs, H, N, n_chunks)


def staged_programs(kind, H):
    if kind == "narrow":
        return [wide(H, 34, 3, seed=1), wide(H, 34, 2, seed=2)]          # max_in 4
    if kind == "big":
        return [wide(H, 34, 3, seed=3, big=18), wide(H, 34, 3, seed=1)]   # max_in 19: PPR false
    return [wide(H, 34, 3, seed=4, conf=True), wide(H, 34, 3, seed=1)]    # confounders


def staged_cases():
    """(kind, H, N, W): every STAGED_H x N / W cycling on the narrow batch, the 19-input batch
    at both CW and every W, the confounder batch once."""
    out = []
    for i, H in enumerate(STAGED_H):
        out.append(("narrow", H, STAGED_N[i % 4], STAGED_W[i % 3]))
    out += [("big", 20, 65, 1), ("big", 16, 150, 2), ("big", 5, 64, 8), ("conf", 20, 150, 2), ("conf", 7, 65, 8)]
    return out


def staged_case(kind, H, N, W):
    return make_case(staged_programs(kind, H), H, N, 2)
