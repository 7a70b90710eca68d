"""The clip + Adam tail without a GPU: what st_clip_adam refuses before it launches anything, and the yardstick the GPU tests of the tail
(tests/test_gpu_optimizer_tail.py) are scaled by."""
import ctypes as C

import numpy as np
import pytest
import torch

from signaltrain_amd import _lib
from tests import adam_reference as A


# ---------------------------------------------------------------------------------------------- st_clip_adam's argument checks
def _call(lib, ptrs, n_total, n_stft, step):
    """st_clip_adam on dummy HOST addresses: every case below is refused before any device access, so nothing is ever read through them."""
    rc = lib.st_clip_adam(*[C.c_void_p(a) if a else None for a in ptrs[:4]], n_total, n_stft, C.c_void_p(ptrs[4]) if ptrs[4] else None,
                          1.0, 1e-3, 0.9, 0.999, 1e-8, step, None)
    return rc, lib.st_last_error()


@pytest.fixture(scope="module")
def dummies():
    keep = [(C.c_float * 8)() for _ in range(5)]
    yield [C.addressof(b) for b in keep]


@pytest.mark.parametrize("n_total, n_stft, step, cause", [
    (0, 0, 1, b"n_total must be positive"),            # was a zero-block launch
    (-4, -8, 1, b"n_total must be positive"),
    (8, -4, 1, b"n_stft must not be negative"),
    (6, 4, 1, b"multiples of 4"),
    (8, 2, 1, b"multiples of 4"),
    (8, 12, 1, b"n_stft exceeds n_total"),
    (8, 4, 0, b"step must be at least 1"),
    (8, 4, -3, b"step must be at least 1"),
])
def test_clip_adam_refuses_bad_sizes(dummies, n_total, n_stft, step, cause):
    lib = _lib.load()
    rc, msg = _call(lib, dummies, n_total, n_stft, step)
    assert rc != 0 and msg.startswith(b"st_clip_adam") and cause in msg, (rc, msg)


@pytest.mark.parametrize("which", range(5), ids=["params", "grads", "m", "v", "scalars"])
def test_clip_adam_refuses_each_null_pointer(dummies, which):
    lib = _lib.load()
    ptrs = list(dummies); ptrs[which] = 0
    rc, msg = _call(lib, ptrs, 8, 4, 1)
    assert rc != 0 and b"st_clip_adam: null pointer" in msg, (rc, msg)


# ---------------------------------------------------------------------------------------------- the reference itself
def test_make_state_plants_what_it_promises():
    n = 65536
    p, g, m, v = (t.numpy() for t in A.make_state(n, A.SWEEP_SEED))
    assert all(a.dtype == np.float32 and a.shape == (n,) for a in (p, g, m, v))
    q = lambda a: a.reshape(-1, 4)
    zero_quads = (q(g) == 0).all(1) & (q(m) == 0).all(1) & (q(v) == 0).all(1)
    g0_live = (q(g) == 0).all(1) & (q(m) != 0).all(1) & (q(v) > 0).all(1)
    one_lane = ((q(g) != 0).sum(1) == 1) & ((q(m) != 0).sum(1) <= 1)
    assert zero_quads.sum() >= 100 and g0_live.sum() >= 100 and one_lane.sum() >= 100
    assert zero_quads[1] and g0_live[2] and one_lane[3]
    for a in (g, p, m):
        assert 0.03 < (a == 0).mean() < 0.25
    assert ((m == 0) == (v == 0)).all() and (v >= 0).all()
    tiny = np.finfo(np.float32).tiny
    for a in (g, m, v):
        assert np.abs(a[a != 0]).min() > 1e3 * tiny            # nothing near the subnormals
    # (1 - b2) g^2 > 1e-37 under the strongest clip the GPU tests reach: a clipped gradient is g / sum |g| whatever grad_scale is, and the largest
    # case sums 6292484 elements
    gmin, gmean = float(np.abs(g[g != 0]).min()), float(np.abs(g).astype(np.float64).mean())
    assert 0.001 * (gmin / (6292484 * gmean)) ** 2 > 1e-37


def test_adam_ref_is_the_textbook_step():
    """adam_ref (torch's optimizer with a preloaded state) against the four lines of the algorithm written out in float64."""
    n, step, lr, b1, b2, eps, gs, n_clip = 1024, 7, 3e-4, 0.85, 0.99, 1e-6, 0.25, 512
    p, g, m, v = (t.double() for t in A.make_state(n, 3))
    g = g * 4096.0                                                            # a norm above 1: the clip is active
    rp, rg, rm, rv, norm, coef = A.adam_ref(p, g, m, v, step, lr, b1, b2, eps, n_clip, gs, torch.float64)
    g2 = g * gs
    assert norm == pytest.approx(float(g2[:n_clip].abs().sum()), rel=1e-14) and coef == pytest.approx(1.0 / (norm + 1e-6), rel=1e-14) and coef < 1
    g2[:n_clip] *= coef
    m2 = b1 * m + (1 - b1) * g2
    v2 = b2 * v + (1 - b2) * g2 * g2
    p2 = p - lr / (1 - b1 ** step) * m2 / (v2.sqrt() / (1 - b2 ** step) ** 0.5 + eps)
    for a, b in ((rg, g2), (rm, m2), (rv, v2), (rp, p2)):
        assert torch.allclose(a, b, rtol=1e-12, atol=0.0)
    e = A.measures((rp, rg, rm, rv), (rp, rg, rm, rv), (p, g, m, v), step, lr, b1, b2, eps)
    assert e == {k: 0.0 for k in A.MEASURES}
    bad_v = rv.clone(); bad_v[1::2] *= 1.0 + 2.0 ** -20                          # 16 u on v
    e = A.measures((rp, rg, rm, bad_v), (rp, rg, rm, rv), (p, g, m, v), step, lr, b1, b2, eps)
    assert 15.9 < e["v"] < 16.1 and e["m"] == 0.0


def test_yardstick_stays_below_its_ceiling():
    """The reference's own float32 step against its float64 step (never the code under test): a change of recipe or of torch version that moves the
    yardstick shows here, on the CPU, and not as a GPU bound that silently widened."""
    p, g, m, v = A.make_state(A.SWEEP_N, A.SWEEP_SEED)
    worst = {k: 0.0 for k in A.MEASURES}
    for step, (b1, b2, eps), gs in A.sweep_cases():
        y = A.yardstick(p, g, m, v, step, A.SWEEP_LR, b1, b2, eps, A.SWEEP_N // 2, gs)
        worst = {k: max(worst[k], y[k]) for k in worst}
    print("yardstick, units of 2^-24:", {k: round(x, 2) for k, x in worst.items()})
    for k in A.MEASURES:
        assert 0.0 < worst[k] <= A.YARDSTICK_CEILING[k], (k, worst)
