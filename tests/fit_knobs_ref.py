"""The reference of the device knob fit (st_fit_knobs): objective and gradient from oracle/st_oracle.py, a float64 Adam + clamp replay, and the case table
the host and GPU tests share.  Needs no GPU.

Objective: J(knobs) = (1 / n_out) sum_{i < n_out} logcosh(y_hat_i - target_i), n_out = n - (L - y): the windows are host_audio.sliding_window's (below L: the one
zero-padded window), the target of a window its last y samples, and the output positions of the last window that lie behind the recording's end carry neither
loss nor gradient.  The oracle's model_loss_bwd knows no mask, so those positions get y_true = out itself (dy = -tanh(0) / (nwin y) = 0 there), its L1 term is
switched off for the call, and its d_knobs -- the gradient of the mean over nwin * y samples -- is rescaled by nwin * y / n_out."""
import math

import numpy as np

from oracle import host_audio
from oracle import st_oracle as O
from tests.dims_table import geo_of, seeds_of

K = 4
# the rows the GPU file compares against this reference; None is the default geometry (T - OT == 16)
ROWS = ["n256", "h256", "ragged", "tiny", "n32", None]
HOPS = 7                # nine windows: batches of four end in a single window whose tail lies behind the recording's end
KN = np.array([0.1, -0.3, 0.25, -0.45], np.float32)
TOL_GRAD = {"f32": 2e-4, "f32x3": 2e-4, "bf16": 6e-2, "bf16_all": 6e-2, "f16": 6e-2, "f16_all": 6e-2}      # tests/test_gpu_knob_grad_fused.py TOL
# signal seed per row where it is not 3: the first of 3, 4, 5, ... at which the float32 oracle agrees with the float64 one to a quarter of the fp32 tolerances
# (tests/test_fit_knobs_host.py::test_cases_are_well_conditioned asserts it; the rule of tests/dims_table.py).  Every row qualifies at 3.
SIGNAL_SEED = {}


def geo_for(row):
    return O.geometry(1, 4, "lean") if row is None else geo_of(row)


def length(geo, hops=HOPS):
    """Not a whole number of hops: hops + 2 windows."""
    return geo["L"] + hops * geo["y"] + 777 % geo["y"]


def signal(n, seed=3):
    rng = np.random.default_rng(seed)
    return (0.4 * np.sin(np.arange(n) * 0.013) + 0.05 * rng.standard_normal(n)).astype(np.float32)


def target_of(sig, seed=11):
    """A processed version that is no output of the model: a soft-clipped, slightly delayed copy plus a little noise (residuals of order 0.1)."""
    rng = np.random.default_rng(seed)
    t = np.tanh(1.7 * np.roll(sig.astype(np.float64), 3)) * 0.6 + 0.01 * rng.standard_normal(sig.size)
    return t.astype(np.float32)


def pair(row, hops=HOPS):
    geo = geo_for(row)
    sig = signal(length(geo, hops), SIGNAL_SEED.get(row, 3))
    return sig, target_of(sig)


def windows(sig, geo):
    """audio.sliding_window with overlap L - y; below one window, the one zero-padded window."""
    L, y = geo["L"], geo["y"]
    if sig.size < L:
        return np.pad(sig, (0, L - sig.size))[None, :]
    return np.ascontiguousarray(host_audio.sliding_window(sig, L, overlap=L - y))


def objective(sig, tgt, kn_rows, P, geo, dtype=np.float64, want_grad=True):
    """(J, d J / d knobs per window [nwin, K], out [n_out]) in `dtype` arithmetic (the rounding modes of the oracle, if any are set, apply).
    The gradient of ONE knob row is the sum over the windows."""
    L, y = geo["L"], geo["y"]
    n = sig.size
    n_out = n - (L - y)
    assert n_out > 0
    xw = windows(sig, geo).astype(dtype)
    tw = windows(tgt, geo)[:, L - y:].astype(dtype)
    nwin = xw.shape[0]
    kn = np.asarray(kn_rows, dtype)
    kn = np.tile(kn.reshape(1, -1), (nwin, 1)) if kn.size == kn.shape[-1] else kn.reshape(nwin, -1)
    Pd = {k: v.astype(dtype) for k, v in P.items()}
    out = O.model_fwd(xw, kn, Pd, geo)[0]
    valid = (np.arange(nwin * y) < n_out).reshape(nwin, y)
    J = float(np.sum(O.logcosh(out.astype(np.float64) - tw.astype(np.float64))[valid]) / n_out)
    if not want_grad:
        return J, None, out.reshape(-1)[:n_out]
    y_true = np.where(valid, tw, out).astype(dtype)
    lam = O.L1_LAMBDA
    try:
        O.L1_LAMBDA = 0.0
        _, _, c = O.model_loss_bwd(xw, kn, y_true, Pd, geo)
    finally:
        O.L1_LAMBDA = lam
    g = c["d_knobs"].astype(np.float64) * (nwin * y / n_out)
    return J, g, out.reshape(-1)[:n_out]


def adam_replay(k0, grads, first_step=1, lr=0.05, b1=0.9, b2=0.999, eps=1e-8, m=None, v=None):
    """torch.optim.Adam's update (bias-corrected, denom = sqrt(v) / sqrt(1 - b2^t) + eps) and the clamp to [-0.5, 0.5], in float64, on a given gradient
    history [steps, ...].  Returns (knobs, m, v)."""
    p = np.asarray(k0, np.float64).copy()
    m = np.zeros_like(p) if m is None else np.asarray(m, np.float64).copy()
    v = np.zeros_like(p) if v is None else np.asarray(v, np.float64).copy()
    for s, g in enumerate(np.asarray(grads, np.float64)):
        t = first_step + s
        g = g.reshape(p.shape)
        m = m + (1.0 - b1) * (g - m)
        v = b2 * v + (1.0 - b2) * g * g
        denom = np.sqrt(v) / math.sqrt(1.0 - b2 ** t) + eps
        p = p - (lr / (1.0 - b1 ** t)) * m / denom
        p = np.clip(p, -0.5, 0.5)
    return p, m, v


_CASES = {}


def case(row):
    """(geo, P) of a row, parameters seeded as the fused sweep seeds them; made once, never modified."""
    from tests import gpu_checks as G                        # make_case only (numpy); no GPU touched
    if row not in _CASES:
        geo, _, _, _, P = G.make_case(1, seeds_of(row)[1], K=K, geo=None if row is None else geo_of(row))
        _CASES[row] = (geo, P)
    return _CASES[row]
