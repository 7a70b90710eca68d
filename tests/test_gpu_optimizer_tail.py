"""The clip + Adam tail on GIVEN gradients against a float64 Adam (tests/adam_reference.py): st_clip_adam, st_finalize_scalars, st_dp_clip_adam and the
head of the captured step.  Needs a GPU.

Through the whole train step the tail is only ever seen from m = v = 0 with nearly the same gradient every step, where the update is lr * sign(g)
whatever the bias corrections, the betas or the place of eps are, and behind 1e-12 of upstream gradient noise that m / (sqrt(v) + eps) turns into a
fraction of lr.  Here the kernel gets g, m, v and p, so there is no upstream noise and it is held to a few units of u = 2^-24:

  * one step: the four measures of adam_reference.measures, each within 4 x the yardstick of the SAME case (torch's float32 step against its float64
    step, computed in the test).  The factor 4 is for the roundings the kernel legitimately takes and torch's float32 path does not: contracted fma,
    the reciprocal form of the coefficient, (w2 g) g against w2 (g g).
  * hyper-parameters reach the library as C floats, so the reference takes float32(lr), float32(b1), ... as its exact inputs: 0.999f differs from
    0.999 by 1.3e-8, which pow(., 1000) turns into 60 u of sqrt(bc2).
  * sums (st_finalize_scalars, the norm of st_dp_clip_adam) are held to the derived bound of their summation order, (ceil(n / 256) + 12) u sum |x|.

Worst seen on an MI355X over every st_clip_adam and st_dp_clip_adam case, units of u (the bound is 4 x the yardstick of the case; in brackets the
largest yardstick of any case, then the largest ratio of a case's figure to its own yardstick):
    m 1.05 (1.05, x 1.04)    v 5.19 (6.21, x 1.12)    g 1.81 (2.87, x 1.12)    update 3.74 (3.96, x 1.52)
The kernel takes torch's own order of operations, so most cases land on the yardstick's very figure.  Trajectory, 50 steps: p 1.3e-7 absolute, m 0.53,
v 8.4 against torch float32's 1.3e-7, 0.61, 8.4.  The norm of st_dp_clip_adam over 4.2 M elements: 0.8 u of the float64 sum at the worst (bound 33 u).
With bc2_sqrt replaced by 1, with eps moved under the root, and with the clipped range one quad too long, 47, 51 and 35 of the 61 cases fail.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from oracle import st_oracle as O
from signaltrain_amd import _lib
from tests import adam_reference as A
from tests import dims_table as DT
from tests import gpu_checks as G

pytestmark = pytest.mark.gpu

DEV = G.DEV
U = A.U
FACTOR = 4.0
SENTINEL = np.array([-11.0, -12.0, -13.0, -14.0, -15.0, 3.0, 41.0, -17.0], np.float32)      # what a scalar nobody wrote still holds
f32 = lambda x: float(np.float32(x))
bits = lambda t: (t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))).view(torch.int32)
same_bits = lambda a, b: bool(torch.equal(bits(a), bits(b)))


@functools.lru_cache(maxsize=2)
def _state(n, seed):
    return A.make_state(n, seed)


def state_of(n, seed):
    """Fresh copies: the cached tensors are never written."""
    return tuple(t.clone() for t in _state(n, seed))


def hyper32(lr, b1, b2, eps):
    return f32(lr), f32(b1), f32(b2), f32(eps)


class Device:
    """p, g, m, v and the eight scalars on the device; step() is one st_clip_adam on them."""

    def __init__(self, state, scalars):
        self.lib = _lib.load()
        self.t = [t.to(DEV).contiguous() for t in state]
        self.s = torch.from_numpy(np.asarray(scalars, np.float32).copy()).to(DEV)
        self.n = int(state[0].numel())

    def step(self, n_stft, gs, lr, b1, b2, eps, step):
        P, Gr, M, V = self.t
        _lib.check(self.lib.st_clip_adam(_lib.ptr(P), _lib.ptr(Gr), _lib.ptr(M), _lib.ptr(V), self.n, int(n_stft), _lib.ptr(self.s),
                                         float(gs), float(lr), float(b1), float(b2), float(eps), int(step), G.stream()), "st_clip_adam")
        torch.cuda.synchronize()

    def read(self):
        return tuple(t.cpu() for t in self.t), self.s.cpu().numpy()


def quads(t):
    return (t.numpy() if torch.is_tensor(t) else t).reshape(-1, 4)


def check_planted_quads(state, got, lr):
    """g = m = v = 0 quads: p keeps its bits, the moments stay zero.  g = 0 quads with live moments: they move (a skip keyed on g alone would not); how
    far is the measures' business, and a parameter whose update is below half its ulp may stay, so of p only the bulk is asked to move."""
    p, g, m, v = state
    zq = (quads(g) == 0).all(1) & (quads(m) == 0).all(1) & (quads(v) == 0).all(1)
    if zq.any():
        z = torch.from_numpy(np.repeat(zq, 4))
        assert same_bits(got[0][z], p[z]) and not got[2][z].any() and not got[3][z].any() and not got[1][z].any()
    live = (quads(g) == 0).all(1) & (quads(m) != 0).all(1)
    if live.any():
        l_ = torch.from_numpy(np.repeat(live, 4))
        assert (got[2][l_] != m[l_]).all() and (got[3][l_] != v[l_]).all()
        assert lr == 0 or (got[0][l_] != p[l_]).float().mean() > 0.9
    return int(zq.sum()), int(live.sum())


def run_case(state, n_stft, gs, lr, b1, b2, eps, step, label, bound=True):
    """One st_clip_adam with scalars[3], scalars[4] from the float64 reference: asserts the four measures against 4 x the case's yardstick (bound = False:
    the caller does, over several states), that the scalars are only read, and the planted quads.  Returns (got, ref, measured, yardstick)."""
    lr, b1, b2, eps = hyper32(lr, b1, b2, eps)
    ref = A.adam_ref(*state, step, lr, b1, b2, eps, n_stft, gs, torch.float64)
    yard = A.yardstick(*state, step, lr, b1, b2, eps, n_stft, gs, ref=ref)
    g2 = ref[1][ref[1] != 0] ** 2
    assert g2.numel() == 0 or (1.0 - b2) * float(g2.min()) > 1e-37, "the case reaches the subnormals: the relative measures would not hold"
    scal = SENTINEL.copy(); scal[3] = np.float32(ref[4]); scal[4] = np.float32(ref[5])
    dev = Device(state, scal)
    dev.step(n_stft, gs, lr, b1, b2, eps, step)
    got, s_out = dev.read()
    e = A.measures(got, ref[:4], state, step, lr, b1, b2, eps)
    if bound:
        print(f"{label}: " + "  ".join(f"{k} {e[k]:.2f} (yardstick {yard[k]:.2f})" for k in A.MEASURES) + f"  norm {ref[4]:.4g} coef {ref[5]:.4g}")
    assert same_bits(s_out, scal), "st_clip_adam wrote the scalars it only reads"
    for k in A.MEASURES:
        assert not bound or e[k] <= FACTOR * yard[k], (label, k, e, yard)
    check_planted_quads(state, got, lr)
    return got, ref, e, yard


# ---------------------------------------------------------------------------------------------- st_clip_adam: hyper-parameters
@pytest.mark.parametrize("gs", A.SWEEP_SCALES)
@pytest.mark.parametrize("hyper", A.SWEEP_HYPER, ids=["b.9_.999_e1e-8", "b.85_.99_e1e-6"])
@pytest.mark.parametrize("step", A.SWEEP_STEPS)
def test_clip_adam_one_step_over_steps_and_betas(step, hyper, gs):
    """From a preloaded state with m and v of the gradient's own scale: bc1, bc2, w1, w2 and eps all show (from m = v = 0 they cancel)."""
    n = A.SWEEP_N
    state = state_of(n, A.SWEEP_SEED)
    _, ref, _, _ = run_case(state, n // 2, gs, A.SWEEP_LR, *hyper, step, f"step {step} {hyper} gs {gs}")
    assert ref[5] < 1.0                                             # the clip is active in this sweep


def test_clip_adam_lr_zero_keeps_the_parameters():
    n = 1028
    state = state_of(n, 5)
    got, ref, e, _ = run_case(state, 512, 1.0, 0.0, 0.9, 0.999, 1e-8, 3, "lr 0")
    assert same_bits(got[0], state[0])
    live = state[1] != 0
    moved = lambda k: (got[k][live] != state[k][live]).float().mean().item()
    assert moved(2) > 0.99 and moved(3) > 0.99                                                         # the moments still advance


# ---------------------------------------------------------------------------------------------- st_clip_adam: sizes and the clipped range
CAP = 2048 * 256 * 4          # floats one grid-stride trip of the capped grid covers
SIZES = [4, 1020, 1028, CAP, CAP + 4, 3 * CAP + 1028]          # one thread / ragged last block / the 2048-block cap exactly / one quad into trip two / several trips


def _ranges():
    out = []
    for n in SIZES:
        cand = [0, 4, n - 4, n] + ([CAP + 516] if n > CAP + 520 else [])
        for c in sorted(set(cand)):
            out.append(pytest.param(n, c, id=f"n{n}-clip{c}"))
    return out


def plant_boundary(state, n_stft):
    """Known live values in the quads on either side of n_stft (and a norm above 1, so that the coefficient is well below 1)."""
    p, g, m, v = state
    n = g.numel()
    pat = torch.tensor([3.6, -3.2, 2.8, -2.4], dtype=torch.float32)          # sum |.| = 12: above 1 under grad_scale 0.25 too
    for q0 in (n_stft - 4, n_stft):
        if 0 <= q0 and q0 + 4 <= n:
            g[q0:q0 + 4] = pat; m[q0:q0 + 4] = -0.5 * pat; v[q0:q0 + 4] = 0.37 * pat * pat


def check_boundary(state, got, ref, n_stft, gs):
    n_total = state[1].numel()
    g_old, g_new, coef = state[1].double(), got[1].double(), ref[5]
    if n_stft >= 4:                                  # the last clipped quad took the coefficient ...
        assert coef < 0.5
        q = slice(n_stft - 4, n_stft)
        want = g_old[q] * gs * coef
        assert ((g_new[q] - want).abs() <= 2 * U * want.abs()).all(), (g_new[q], want)
    if n_stft + 4 <= n_total:                        # ... the first quad behind it did not: grad_scale alone, a power of two, exactly
        q = slice(n_stft, n_stft + 4)
        assert torch.equal(g_new[q], g_old[q] * gs), (g_new[q], g_old[q] * gs)


@pytest.mark.parametrize("n_total, n_stft", _ranges())
def test_clip_adam_sizes_and_clip_boundary(n_total, n_stft):
    gs = 0.25 if n_total in (1028, CAP + 4) else 1.0
    args = (n_stft, gs, 1e-3, 0.9, 0.999, 1e-8, 10, f"n {n_total} clip {n_stft} gs {gs}")
    if n_total > 4:
        state = state_of(n_total, 20 + SIZES.index(n_total))
        plant_boundary(state, n_stft)
        got, ref, _, _ = run_case(state, *args)
        check_boundary(state, got, ref, n_stft, gs)
        return
    # one quad: four samples say nothing about a worst case, for the yardstick or for the kernel, so the case is 256 one-quad states (every second one
    # with the planted boundary values) and the worst over all of them is held to 4 x the yardstick's worst over the same states
    worst, yard = {k: 0.0 for k in A.MEASURES}, {k: 0.0 for k in A.MEASURES}
    for seed in range(256):
        state = A.make_state(4, 1000 + seed)
        if seed % 2:
            plant_boundary(state, n_stft)
        got, ref, e, y = run_case(state, *args, bound=False)
        if seed % 2:
            check_boundary(state, got, ref, n_stft, gs)
        worst = {k: max(worst[k], e[k]) for k in worst}; yard = {k: max(yard[k], y[k]) for k in yard}
    print(f"{args[-1]}, 256 states: " + "  ".join(f"{k} {worst[k]:.2f} (yardstick {yard[k]:.2f})" for k in A.MEASURES))
    for k in A.MEASURES:
        assert worst[k] <= FACTOR * yard[k], (k, worst, yard)


@pytest.mark.parametrize("gs", [1.0, 0.25])
def test_clip_adam_inactive_clip_scales_exactly_once(gs):
    """norm < 1, so coef == 1: with grad_scale 1 the gradient buffer comes back bit-identical (the kernel does not even write it), with grad_scale 0.25
    every element, clipped range or not, is scaled exactly once."""
    n, n_stft = 1028, 512
    state = list(state_of(n, 6))
    norm = float(state[1][:n_stft].double().abs().sum())
    state[1] = state[1] * 2.0 ** math.floor(math.log2(0.4 / norm))          # exact: a power of two
    got, ref, _, _ = run_case(tuple(state), n_stft, gs, 1e-3, 0.9, 0.999, 1e-8, 4, f"coef 1, gs {gs}")
    assert ref[5] == 1.0 and 0.0 < ref[4] < 1.0
    assert same_bits(got[1], state[1] * gs)


# ---------------------------------------------------------------------------------------------- st_clip_adam: the overflow skip
def test_clip_adam_skips_on_a_non_finite_norm():
    n = 1028
    state = state_of(n, 7)
    scal = SENTINEL.copy(); scal[4] = 1.0
    args = (512, 1.0, *hyper32(1e-3, 0.9, 0.999, 1e-8), 5)
    dev = Device(state, scal)
    for k, bad in enumerate((np.inf, np.nan)):
        dev.s[3] = float(bad)
        before = dev.s.cpu()
        dev.step(*args)
        got, s_out = dev.read()
        for a, b in zip(got, state):
            assert same_bits(a, b), f"norm {bad}: the step was not skipped"
        assert s_out[5] == SENTINEL[5] + k + 1
        keep = [0, 1, 2, 3, 4, 6, 7]
        assert same_bits(torch.from_numpy(s_out)[keep], before[keep])
    dev.s[3] = 3.0e38                                 # finite, however large: the step runs
    dev.step(*args)
    got, s_out = dev.read()
    live = state[1] != 0
    assert (got[2][live] != state[2][live]).float().mean() > 0.99 and not same_bits(got[0], state[0])
    assert s_out[5] == SENTINEL[5] + 2
    ref = A.adam_ref(*state, 5, *hyper32(1e-3, 0.9, 0.999, 1e-8), 0, 1.0, torch.float64)          # coef 1 at grad_scale 1: the plain step
    e = A.measures(got, ref[:4], state, 5, *hyper32(1e-3, 0.9, 0.999, 1e-8))
    yard = A.yardstick(*state, 5, *hyper32(1e-3, 0.9, 0.999, 1e-8), 0, 1.0, ref=ref)
    assert all(e[k] <= FACTOR * yard[k] for k in A.MEASURES), (e, yard)


# ---------------------------------------------------------------------------------------------- st_clip_adam: 50 consecutive steps
def test_clip_adam_trajectory_from_zero_moments():
    """step = 1 .. 50 from m = v = 0 with a fresh gradient per step, against ONE free-running float64 torch.optim.Adam (its own step counter): the
    step -> bc1, bc2 sequence.  Bound: 4 x what torch's free-running float32 Adam deviates by on the same gradients, measure by measure -- p absolutely
    (every update is of size lr), m by the largest clipped gradient the element saw, v relatively."""
    n, n_clip, steps, gs = 2052, 1024, 50, 1.0
    lr, b1, b2, eps = hyper32(1e-3, 0.9, 0.999, 1e-8)
    rng = np.random.default_rng(77)
    s = 10.0 ** rng.uniform(-8.0, -1.0, n)
    grads = []
    for _ in range(steps):
        g = s * rng.standard_normal(n)
        g[rng.random(n) < 0.05] = 0.0
        grads.append(torch.from_numpy(g.astype(np.float32)))
    p0 = torch.from_numpy((0.1 * rng.standard_normal(n)).astype(np.float32))
    p64, m64, v64, clips, gmax = A.adam_trajectory(p0, grads, lr, b1, b2, eps, n_clip, gs, torch.float64)
    p32, m32, v32, _, _ = A.adam_trajectory(p0, grads, lr, b1, b2, eps, n_clip, gs, torch.float32)
    assert all(c < 1.0 for _, c in clips)

    def deviation(p, m, v):
        p, m, v = p.double(), m.double(), v.double()
        assert not (v[v64 == 0] != 0).any()
        nz = v64 > 0
        return {"p": float((p - p64).abs().max()), "m": float(((m - m64).abs()[gmax > 0] / gmax[gmax > 0]).max()) / U,
                "v": float(((v - v64).abs()[nz] / v64[nz]).max()) / U}
    yard = deviation(p32, m32, v32)
    zero = torch.zeros(n)
    dev = Device((p0, grads[0], zero, zero), SENTINEL)
    for t, g in enumerate(grads):
        dev.t[1].copy_(g)
        dev.s[3] = f32(clips[t][0]); dev.s[4] = f32(clips[t][1])
        dev.step(n_clip, gs, lr, b1, b2, eps, t + 1)
    (p, _, m, v), _ = dev.read()
    e = deviation(p, m, v)
    print(f"trajectory, 50 steps: device {e}  torch float32 {yard}")
    assert float((p64 - p0.double()).abs().max()) > 2 * lr           # it did travel
    for k in e:
        assert e[k] <= FACTOR * yard[k], (k, e, yard)


# ---------------------------------------------------------------------------------------------- st_finalize_scalars
def sum_bound(n, abs_sum):
    """256 serial accumulators of ceil(n / 256) terms each, then the block tree: first-order bound of that summation order."""
    return (math.ceil(n / 256) + 12) * U * abs_sum


def _partial_counts(d):
    lib = _lib.load()
    n = (lib.st_ola_loss_partials(C.byref(d)), lib.st_ae_fwd_partials(C.byref(d)), lib.st_norm_partials(C.byref(d)))
    assert all(k > 0 for k in n), n
    return n


FIN_CASES = [pytest.param(None, 1, id="scale1-B1"), pytest.param(None, 3, id="scale1-B3"), pytest.param(None, 1024, id="scale1-B1024"),
             pytest.param("n256", 3, id="n256-B3")]


@pytest.mark.parametrize("offset", [4, 1], ids=["aligned16", "off-by-one-float"])
@pytest.mark.parametrize("row, B", FIN_CASES)
def test_finalize_scalars_against_float64_sums(row, B, offset):
    lib = _lib.load()
    geo = O.geometry(1, 4, "lean") if row is None else DT.geo_of(row)
    d = G.dims_of(geo, B, 4)
    n_loss, n_reg, n_norm = _partial_counts(d)
    print(f"partials: loss {n_loss} reg {n_reg} norm {n_norm}")
    if row is None and B == 1024:
        assert n_loss == 8192 and n_loss // 4 > 768 + 256          # the four-deep unrolled loop runs, and more than once for some threads
    if row is None and B == 3:
        assert n_loss // 4 <= 768                                   # the single loop alone
    if row is not None:
        assert any(k % 4 for k in (n_loss, n_reg, n_norm)), "no count with a scalar tail: pick another geometry"
    rng = np.random.default_rng(1000 * B + offset)
    wide = lambda k: 10.0 ** rng.uniform(-6.0, 0.0, k)
    host = {"loss": wide(n_loss), "reg": wide(n_reg) * np.where(rng.random(n_reg) < 0.5, -1.0, 1.0), "a": wide(n_norm), "s": wide(n_norm)}
    reg_scale = (2e-5 / 10) / (B * geo["OT"] * geo["F"])            # gpu_checks' reg_coef at loss scale 1
    for target in (0.5, 1.0, 1e3):
        for inv_world in (1.0, 0.25):
            k = target / ((host["a"].sum() + host["s"].sum()) * inv_world)
            h32 = {key: (val * (k if key in ("a", "s") else 1.0)).astype(np.float32) for key, val in host.items()}
            bufs = {}
            for key, val in h32.items():                            # 16-byte aligned at offset 4 floats (the float4 path), not at offset 1 (psum's scalar branch)
                big = torch.zeros(val.size + 8, device=DEV)
                view = big[offset:offset + val.size]
                view.copy_(torch.from_numpy(val))
                assert (view.data_ptr() % 16 == 0) == (offset == 4)
                bufs[key] = view
            scal = torch.from_numpy(SENTINEL.copy()).to(DEV)
            _lib.check(lib.st_finalize_scalars(C.byref(d), _lib.ptr(bufs["loss"]), _lib.ptr(bufs["reg"]), _lib.ptr(bufs["a"]), _lib.ptr(bufs["s"]),
                                               inv_world, _lib.ptr(scal), G.stream()), "st_finalize_scalars")
            torch.cuda.synchronize()
            s = scal.cpu().numpy()
            h = {key: val.astype(np.float64) for key, val in h32.items()}
            by = B * geo["y"]
            want1, want2, want3 = h["loss"].sum() / by, h["reg"].sum() * reg_scale, (h["a"].sum() + h["s"].sum()) * inv_world
            assert abs(s[1] - want1) <= sum_bound(n_loss, h["loss"].sum() / by), (s[1], want1)
            assert abs(s[2] - want2) <= sum_bound(n_reg, np.abs(h["reg"]).sum() * reg_scale), (s[2], want2)
            assert abs(s[3] - want3) <= sum_bound(2 * n_norm, want3), (s[3], want3)
            assert abs(float(s[0]) - (float(s[1]) + float(s[2]))) <= float(np.spacing(max(abs(s[0]), abs(s[1])))), s[:3]      # one rounding or two (a contracted fma)
            coef = np.float32(min(np.float32(1.0), np.float32(1.0) / (s[3] + np.float32(1e-6))))
            assert abs(float(s[4]) - float(coef)) <= 4 * float(np.spacing(coef)), (s[4], coef)
            assert abs(float(s[3]) - target) < 1e-4 * target
            assert (s[4] == 1.0) if target == 0.5 else (s[4] < 1.0)
            assert same_bits(s[5:], SENTINEL[5:])
    # what is not given is not written
    scal = torch.from_numpy(SENTINEL.copy()).to(DEV)
    _lib.check(lib.st_finalize_scalars(C.byref(d), _lib.ptr(bufs["loss"]), _lib.ptr(bufs["reg"]), None, None, 1.0, _lib.ptr(scal), G.stream()), "no norms")
    torch.cuda.synchronize()
    s2 = scal.cpu().numpy()
    assert same_bits(s2[3:], SENTINEL[3:]) and same_bits(s2[:3], s[:3])
    scal = torch.from_numpy(SENTINEL.copy()).to(DEV)
    _lib.check(lib.st_finalize_scalars(C.byref(d), None, _lib.ptr(bufs["reg"]), _lib.ptr(bufs["a"]), _lib.ptr(bufs["s"]), 0.25, _lib.ptr(scal), G.stream()), "no loss")
    torch.cuda.synchronize()
    s3 = scal.cpu().numpy()
    assert same_bits(s3[:3], SENTINEL[:3]) and same_bits(s3[3:5], s[3:5]) and same_bits(s3[5:], SENTINEL[5:])


# ---------------------------------------------------------------------------------------------- st_dp_clip_adam
@pytest.fixture(scope="module")
def engine_case():
    geo, X, Y, KN, P = G.make_case(B=3, seed=2)
    return geo, G.t(X), G.t(Y), G.t(KN), P


@pytest.mark.parametrize("clip_all", [False, True], ids=["clip-stft", "clip-all"])
@pytest.mark.parametrize("gs", [1.0, 0.5])
def test_dp_clip_adam_on_given_gradients(engine_case, gs, clip_all):
    """StepEngine.clip_adam (st_dp_clip_adam: l1_partial_kernel + the fused finalize inside clip_adam_kernel) on make_state's gradients: the norm it forms,
    the step it takes, and the loss scalars it republishes from the workspace."""
    from signaltrain_amd.engine import StepEngine
    geo, x, y, kn, P = engine_case
    d = G.dims_of(geo, 3, 4)
    eng = StepEngine(d, DEV, clip_all=clip_all)
    eng.load_state_dict(P)
    eng.loss_backward(x, kn, y)
    torch.cuda.synchronize()
    published = eng.scalars.cpu()
    assert published[0] > 0 and published[1] > 0
    n, step = eng.layout.total, 10
    state = state_of(n, 31)
    for buf, src in zip((eng.params, eng.grads, eng.m, eng.v), state):
        buf.copy_(src)
    eng.step_count = step - 1
    lr, b1, b2, eps = hyper32(1e-3, 0.9, 0.999, 1e-8)
    n_clip = n if clip_all else eng.layout.n_stft
    eng.clip_adam(lr, gs, betas=(b1, b2), eps=eps)
    torch.cuda.synchronize()
    s = eng.scalars.cpu().numpy()
    got = tuple(t.cpu() for t in (eng.params, eng.grads, eng.m, eng.v))
    ref = A.adam_ref(*state, step, lr, b1, b2, eps, n_clip, gs, torch.float64)
    yard = A.yardstick(*state, step, lr, b1, b2, eps, n_clip, gs, ref=ref)
    n_part = _lib.load().st_norm_partials(C.byref(d))
    per_thread = math.ceil(n_clip / (4 * 256 * n_part))
    bound = (per_thread + 12) * U * ref[4] + sum_bound(n_part, ref[4])
    print(f"dp clip_adam gs {gs} clip_all {clip_all}: norm {s[3]:.9g} ref {ref[4]:.9g} err {abs(float(s[3]) - ref[4]) / ref[4] / U:.2f} u (bound {bound / ref[4] / U:.0f} u)")
    assert abs(float(s[3]) - ref[4]) <= bound
    coef = np.float32(min(np.float32(1.0), np.float32(1.0) / (s[3] + np.float32(1e-6))))
    assert abs(float(s[4]) - float(coef)) <= 4 * float(np.spacing(coef)) and s[4] < 1.0
    e = A.measures(got, ref[:4], state, step, lr, b1, b2, eps)
    print("  " + "  ".join(f"{k} {e[k]:.2f} (yardstick {yard[k]:.2f})" for k in A.MEASURES))
    for k in A.MEASURES:
        assert e[k] <= FACTOR * yard[k], (k, e, yard)
    check_planted_quads(state, got, lr)
    assert same_bits(s[:3], published[:3]), (s[:3], published[:3])          # the same partials, summed in the same order
    assert same_bits(s[5:], published[5:])


# ---------------------------------------------------------------------------------------------- the head of the captured step
def test_graph_head_clamps_at_the_end_of_the_lr_table(engine_case):
    """step_tick_kernel with a table SHORTER than the run: iteration it runs with lr_table[min(max(it - 1, 0), n - 1)]."""
    geo, x, y, kn, P = engine_case
    d = G.dims_of(geo, 3, 4)
    table = [1e-3, 3e-4]
    e1 = G.new_engine(d); e1.load_state_dict(P)
    e2 = G.new_engine(d); e2.load_state_dict(P)
    e2.graph_capture(3, table)
    try:
        for it in range(5):
            xi, yi = torch.roll(x, 23 * it, 1).contiguous(), torch.roll(y, 23 * it, 1).contiguous()
            lr = table[min(max(it - 1, 0), 1)]
            e1.train_step(xi, kn, yi, lr)
            e2.graph_step(xi, kn, yi)
            torch.cuda.synchronize()
            s = e2.scalars.cpu().numpy()
            assert s[6] == it + 1
            assert s[7] == np.float32(lr), (it, s[7], lr)
            assert torch.equal(e1.scalars[:5], e2.scalars[:5]), it
            assert (e1.params - e2.params).abs().max().item() <= 1e-7, it
    finally:
        e2.graph_destroy()
