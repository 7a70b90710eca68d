"""Round 10: the fused fp32 step builds the autoencoders' LDS weight images (forward and data-gradient fragment images of both nets, zero padding included, and the
frequency-weight table) ONCE per step in prep_kernel; ae_fwd_kernel and the kept-activation ae_bwd_kernel copy them linearly instead of rebuilding them in every
workgroup.  Same values at the same LDS positions, same arithmetic behind them: every result is the in-kernel build's (st_set_tuning(8202)) bit for bit.

Tolerances: none -- every comparison is torch.equal / ==.  The shapes are the smallest at which each run-time-sized part of the image takes another form:
IN = T of layer 1 (25: not a multiple of 4; 11: odd, under one 16-wide tile; 32: the full padded width), OUT = OT of layer 9 (9, 6, 16), IN = 16 + K of layer 5
(K = 0, 2, 4) and FP, the length of the table (528 at the default geometry, 32 at n32).  The images lie in the h4 / d a4 exchange areas of the autoencoder workspace
(1024 floats per 16-row group, unused on this path): the forward's part needs 20 groups at the default geometry, the backward's 38 -- so the batches at the small
geometries are the smallest at which both kernels take the ready-made images (t32_ot16: 9 groups per window, B = 5; n32: 2 per window, B = 19), and B = 1 at the
default geometry (33 groups) is the case where only the forward does."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IN_KERNEL, READY = 8202, 8201      # st_set_tuning: kept activations with the images built inside the kernels / the shipped default


def _inputs(row, B, K):
    """Seeded inputs of B windows at the default geometry (row None) or a tests/dims_table.py row: an 8-window case tiled and rescaled per window."""
    from tests import gpu_checks as G
    from tests import dims_table as DT
    nb = min(B, 8)
    geo, X, Y, KN, P = G.make_case(nb, 23, K=K, geo=None if row is None else DT.geo_of(row))
    rng = np.random.default_rng(11)
    reps = (B + nb - 1) // nb
    X = (np.tile(X, (reps, 1))[:B] * rng.uniform(0.4, 1.0, (B, 1))).astype(np.float32)
    Y = (np.tile(Y, (reps, 1))[:B] * rng.uniform(0.4, 1.0, (B, 1))).astype(np.float32)
    KN = (rng.random((B, K)) - 0.5).astype(np.float32)
    return geo, X, Y, KN, P


def _engine(row, B, K):
    from tests import gpu_checks as G
    from signaltrain_amd.engine import StepEngine
    geo, X, Y, KN, P = _inputs(row, B, K)
    eng = StepEngine(G.dims_of(geo, B, K), G.DEV); eng.load_state_dict(P)
    return eng, G.t(X), G.t(KN), G.t(Y)


def _with_code(code, fn):
    from signaltrain_amd import _lib
    lib = _lib.load()
    if code is None:
        return fn()
    try:
        _lib.check(lib.st_set_tuning(code), "st_set_tuning")
        return fn()
    finally:
        _lib.check(lib.st_set_tuning(READY), "st_set_tuning")


def _train(row, B, K, code=None, poison=False):
    """Loss + the 40 gradient tensors of one batch, then the parameters after two optimizer steps.  poison: the whole workspace holds NaN bit patterns before each call."""
    import torch

    def run():
        eng, x, kn, y = _engine(row, B, K)
        nan_fill = (lambda: eng.ws.fill_(0xFF)) if poison else (lambda: None)      # 0xFFFFFFFF: a NaN in every float (and every 16-bit half)
        nan_fill(); eng.loss_backward(x, kn, y); torch.cuda.synchronize()
        g = {k: v.clone() for k, v in eng.layout.views(eng.grads).items()}; loss = float(eng.scalars[0])
        nan_fill(); eng.train_step(x, kn, y, 1e-3)
        nan_fill(); eng.train_step(x, kn, y, 1e-3); torch.cuda.synchronize()
        return g, loss, eng.params.clone()
    return _with_code(code, run)


@functools.lru_cache(maxsize=None)
def _ready_b3():
    """The image path at B = 3, default geometry: shared by the equality, padding and repeatability cases (never modified)."""
    return _train(None, 3, 4)


def _assert_same(a, b):
    import torch
    (ga, la, pa), (gb, lb, pb) = a, b
    assert len(ga) == 40 and la == lb, (la, lb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    assert torch.equal(pa, pb)


@pytest.mark.parametrize("row,B,K", [
    (None, 3, 4),            # fewer groups than waves, a partial group per window
    (None, 64, 4),
    (None, 130, 4),          # ragged last round
    (None, 1, 4),            # 33 groups: ready-made images in the forward, the backward builds its own
    ("h512", 3, 4),          # T = 11, OT = 6: layer-1 rows of 11 floats (no multiple of 4), one partly filled 16-wide tile in both run-time-sized layers
    ("t32_ot16", 5, 4),      # T = 32, OT = 16: both at their padded width, no padding column left in layers 1 and 9
    ("n32", 19, 4),          # F = 17: a 32-entry frequency-weight table, two groups per window
    (None, 3, 0),            # the model without knobs: layer 5 has IN = 16
    (None, 3, 2),            # IN = 18
])
def test_ready_made_images_give_the_in_kernel_build_bit_for_bit(row, B, K):
    """Loss, all 40 gradient tensors and the parameters after two optimizer steps: the default path (images from prep_kernel) against st_set_tuning(8202)."""
    ready = _ready_b3() if (row, B, K) == (None, 3, 4) else _train(row, B, K)
    _assert_same(ready, _train(row, B, K, code=IN_KERNEL))


def test_every_float_of_the_images_is_written():
    """The workspace is the caller's and holds nothing from one call to the next: with NaN bit patterns in every byte of it before each call the step is what it
    is on a zeroed workspace -- the zero padding of the images (and of everything else the step reads) is written, not inherited."""
    import torch
    g, loss, p = _train(None, 3, 4, poison=True)
    assert np.isfinite(loss) and bool(torch.isfinite(p).all()) and all(bool(torch.isfinite(v).all()) for v in g.values())
    _assert_same((g, loss, p), _ready_b3())


def test_forward_only_and_evaluation_use_the_same_images():
    """st_model_fwd without saved state and st_eval_step run prep_kernel + ae_fwd_kernel too: y_hat, |STFT| in and out and the eight evaluation scalars are the
    in-kernel build's bits."""
    import torch

    def run():
        eng, x, kn, y = _engine(None, 3, 4)
        y_hat, mag, mag_hat = eng.forward(x, kn, save_for_backward=False)
        eng.eval_reset(0.25)
        y_eval = eng.eval_step(x, kn, y, want_y_hat=True)
        return y_hat.clone(), mag.clone(), mag_hat.clone(), y_eval.clone(), eng.eval_read()
    a, b = _with_code(None, run), _with_code(IN_KERNEL, run)
    for u, v in zip(a[:4], b[:4]):
        assert torch.equal(u, v)
    assert a[4] == b[4] and all(np.isfinite(a[4])), (a[4], b[4])


def test_image_path_repeats_bit_for_bit():
    _assert_same(_train(None, 3, 4), _ready_b3())
