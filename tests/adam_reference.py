"""A float64 Adam step on given gradients, and error measures in units of u = 2^-24, for the tests of the clip + Adam tail (needs no GPU).

Shared by tests/test_optimizer_tail_host.py (the yardstick: torch's own float32 step against its float64 step) and tests/test_gpu_optimizer_tail.py
(the kernels of csrc/st_misc.h against the float64 step).  The reference is torch.optim.Adam(foreach=False) on CPU tensors, its state preloaded with
(step - 1, exp_avg, exp_avg_sq), after the gradient took grad_scale and the L1 clip of its first n_clip elements (nn_proc.py:299-302:
coef = min(1, 1 / (norm + 1e-6))) -- everything in the dtype asked for.

make_state() spreads the per-element scale over nine decades (Adam is scale-free per element, a kernel's rounding is not), mixes exact zeros into
every array and plants the quads the kernel treats apart: g = m = v = 0 (its structural-zero skip), g = 0 with live moments (must still move) and
quads with one live lane.  Nothing is subnormal: (1 - b2) * g^2 stays above 1e-37 for the clip coefficients the tests reach.

The measures divide by the SCALE of a quantity, never by the quantity: 0.9 m + 0.1 g can cancel, so an error relative to the new moment or to the
update itself says nothing.

Yardstick (tests/test_optimizer_tail_host.py::test_yardstick_stays_below_its_ceiling: steps {1, 2, 10, 1000, 100000} x two (b1, b2, eps) x
grad_scale {1, 0.25}, n = 65536, n_clip = n / 2, lr = 1e-3), worst over the sweep, torch 2.x CPU float32 against float64, in units of u:
    m 1.13    v 4.56    g 1.28    update 4.03
(torch 2.10, make_state(65536, seed 11)).  YARDSTICK_CEILING below is what the host test holds them to.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
MEASURES = ("m", "v", "g", "update")
# what the yardstick may reach before the host test fails: the recorded values plus about a sixth (another torch version may sum the norm in
# another order, which moves the coefficient by an ulp); the GPU bounds are 4 x the yardstick measured in the test itself, not 4 x these
YARDSTICK_CEILING = {"m": 1.3, "v": 5.3, "g": 1.5, "update": 4.7}

QUAD_ZERO, QUAD_G_ZERO, QUAD_ONE_LANE = 1, 2, 3


def quad_kinds(n, seed):
    """The planted kind of every aligned quad (0 = none): about 3 % each, and one of each in quads 1, 2, 3 wherever there are 8 quads or more."""
    rng = np.random.default_rng(seed + 7919)
    nq = n // 4
    r = rng.random(nq)
    kind = np.zeros(nq, np.int8)
    kind[r < 0.03] = QUAD_ZERO
    kind[(r >= 0.03) & (r < 0.06)] = QUAD_G_ZERO
    kind[(r >= 0.06) & (r < 0.09)] = QUAD_ONE_LANE
    if nq >= 8:
        kind[1:4] = (QUAD_ZERO, QUAD_G_ZERO, QUAD_ONE_LANE)
    return kind


def make_state(n, seed):
    """float32 torch tensors p, g, m, v of n elements (n % 4 == 0)."""
    assert n % 4 == 0 and n > 0
    rng = np.random.default_rng(seed)
    s = 10.0 ** rng.uniform(-10.0, -1.0, n)
    g = np.where(rng.random(n) < 0.5, -1.0, 1.0) * s * 10.0 ** rng.uniform(-2.0, 0.5, n)
    m = s * rng.uniform(-1.0, 1.0, n)
    v = s * s * rng.uniform(0.25, 4.0, n)
    p = 0.1 * rng.standard_normal(n)
    g[rng.random(n) < 0.05] = 0.0
    p[rng.random(n) < 0.05] = 0.0
    z = rng.random(n) < 0.05
    m[z] = 0.0; v[z] = 0.0
    kind = np.repeat(quad_kinds(n, seed), 4)
    lane = np.arange(n) % 4
    live = np.repeat(rng.integers(0, 4, n // 4), 4)
    dead = (kind == QUAD_ZERO) | ((kind == QUAD_ONE_LANE) & (lane != live))
    g[dead | (kind == QUAD_G_ZERO)] = 0.0
    m[dead] = 0.0; v[dead] = 0.0
    fix = (kind == QUAD_G_ZERO) & (m == 0.0)          # these quads keep live moments in every lane
    m[fix] = 0.5 * s[fix]; v[fix] = s[fix] ** 2
    fix = (kind == QUAD_ONE_LANE) & (lane == live) & (g == 0.0)
    g[fix] = s[fix]
    return tuple(torch.from_numpy(a.astype(np.float32)) for a in (p, g, m, v))


def clip(g, n_clip, grad_scale):
    """In place, in g's dtype: g *= grad_scale; norm = sum |g[:n_clip]|; g[:n_clip] *= min(1, 1 / (norm + 1e-6)).  Returns (norm, coef) as 0-d tensors."""
    g.mul_(grad_scale)
    norm = g[:n_clip].abs().sum()
    coef = torch.clamp(1.0 / (norm + 1e-6), max=1.0)
    g[:n_clip].mul_(coef)
    return norm, coef


def adam_ref(p, g, m, v, step, lr, b1, b2, eps, n_clip, grad_scale, dtype):
    """One step in `dtype` from copies of the inputs: returns the new (p, g, m, v, norm, coef), tensors of `dtype` and two Python floats."""
    p, g, m, v = (t.detach().to(dtype).clone() for t in (p, g, m, v))
    norm, coef = clip(g, int(n_clip), grad_scale)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    p.grad = g
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m, "exp_avg_sq": v}
    opt.step()
    assert float(opt.state[p]["step"]) == step
    return p.detach(), g, m, v, float(norm), float(coef)


def adam_trajectory(p, grads, lr, b1, b2, eps, n_clip, grad_scale, dtype):
    """len(grads) consecutive steps of ONE free-running optimizer from m = v = 0 (its own step counter: 1, 2, ...): returns (p, m, v,
    [(norm, coef)], the largest |clipped g| every element saw)."""
    p = p.detach().to(dtype).clone()
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    clips, gmax = [], torch.zeros_like(p)
    for g in grads:
        g = g.detach().to(dtype).clone()
        norm, coef = clip(g, int(n_clip), grad_scale)
        clips.append((float(norm), float(coef)))
        gmax = torch.maximum(gmax, g.abs())
        p.grad = g
        opt.step()
    st = opt.state[p]
    assert float(st["step"]) == len(grads)
    return p.detach(), st["exp_avg"], st["exp_avg_sq"], clips, gmax


def _f64(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def _ratio(num, den):
    """num / den where a zero scale admits no error at all: 0 / 0 = 0, x / 0 = inf."""
    out = np.zeros_like(num)
    nz = den > 0
    out[nz] = num[nz] / den[nz]
    out[~nz & (num > 0)] = np.inf
    return out


def measures(got, ref, old, step, lr, b1, b2, eps):
    """The four errors of got = (p, g, m, v) against ref = the float64 step's (p, g, m, v), from old = the inputs (p, g, m, v), worst element each, in
    units of u = 2^-24:
      m       |d| / max(|m_old|, |g_ref|)
      v       |d| / v_ref                                   (v_ref == 0: any difference counts as inf)
      g       |d| / |g_ref|
      update  max(|(p - p_old) - (p_ref - p_old)| - ulp32(p_ref) / 2, 0) / S,   S = (lr / bc1) max(|m_old|, |g_ref|) / (sqrt(v_ref) / sqrt(bc2) + eps)
    A non-finite value in `got` gives inf."""
    gp, gg, gm, gv = (_f64(t) for t in got)
    rp, rg, rm, rv = (_f64(t) for t in ref)
    op, _, om, _ = (_f64(t) for t in old)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    scale_m = np.maximum(np.abs(om), np.abs(rg))
    half_ulp = 0.5 * np.spacing(np.abs(rp).astype(np.float32)).astype(np.float64)
    S = (lr / bc1) * scale_m / (np.sqrt(rv) / math.sqrt(bc2) + eps)
    upd = np.maximum(np.abs((gp - op) - (rp - op)) - half_ulp, 0.0)
    out = {"m": _ratio(np.abs(gm - rm), scale_m), "v": _ratio(np.abs(gv - rv), rv), "g": _ratio(np.abs(gg - rg), np.abs(rg)), "update": _ratio(upd, S)}
    res = {}
    for k, (e, a) in zip(MEASURES, ((out["m"], gm), (out["v"], gv), (out["g"], gg), (out["update"], gp))):
        res[k] = float("inf") if not np.isfinite(a).all() else float(e.max()) / U
    return res


def yardstick(p, g, m, v, step, lr, b1, b2, eps, n_clip, grad_scale, ref=None):
    """The four measures of the reference's own float32 step against its float64 step on the same inputs (ref: that float64 step, if the caller has it)."""
    ref = adam_ref(p, g, m, v, step, lr, b1, b2, eps, n_clip, grad_scale, torch.float64) if ref is None else ref
    own = adam_ref(p, g, m, v, step, lr, b1, b2, eps, n_clip, grad_scale, torch.float32)
    return measures(own[:4], ref[:4], (p, g, m, v), step, lr, b1, b2, eps)


SWEEP_STEPS = (1, 2, 10, 1000, 100000)
SWEEP_HYPER = ((0.9, 0.999, 1e-8), (0.85, 0.99, 1e-6))
SWEEP_SCALES = (1.0, 0.25)
SWEEP_N, SWEEP_LR, SWEEP_SEED = 65536, 1e-3, 11


def sweep_cases():
    return [(st, h, gs) for st in SWEEP_STEPS for h in SWEEP_HYPER for gs in SWEEP_SCALES]
