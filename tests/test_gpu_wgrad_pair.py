"""The fp32 step runs both 128 x 128-tile weight-gradient GEMMs as ONE launch (csrc/st_gemm_tn.h: gemm_tn128_pair_kernel; event-profile names wgrad_pair /
wgrad_pair_reduce) against one launch per GEMM, which st_set_tuning(9582) selects.  Every workgroup runs its analysis slice and then its synthesis slice on
the same accumulators with the same k-tile loop; the products of every output element are summed in the same order, the slabs are summed by the same block
function in the same order: every result is the same bits.

Tolerances: none -- every comparison is numpy.array_equal / ==.  Batches: 3 (one k-slice per GEMM, one or two k-tiles), 8 (two analysis slices against one
synthesis slice: slots with a single entry), 64 (wave-uniform addresses, short slices), 130 (ragged last k-tiles, per-row addresses); n512 is the other geometry
of tests/dims_table.py on this kernel (4 x 4 tiles, two per basis half).  The workspace holds NaN bit patterns before every call, so every slab element and
Nyquist partial the reduce reads was written by this call's launch."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PER_GEMM = 9582      # st_set_tuning: the pipelined loop, one launch per GEMM (the schedule before the pair launch)
K = 4
LR = 1e-3
PAIR_NAMES = ("wgrad_pair", "wgrad_pair_reduce")
GEMM_NAMES = ("synthesis_wgrad", "analysis_wgrad", "analysis_wgrad_reduce")


def _inputs(row, B):
    from tests import gpu_checks as G
    from tests import dims_table as DT
    nb = min(B, 8)
    geo, X, Y, KN, P = G.make_case(nb, 29, K=K, geo=None if row is None else DT.geo_of(row))
    rng = np.random.default_rng(13)
    reps = (B + nb - 1) // nb
    X = (np.tile(X, (reps, 1))[:B] * rng.uniform(0.4, 1.0, (B, 1))).astype(np.float32)
    Y = (np.tile(Y, (reps, 1))[:B] * rng.uniform(0.4, 1.0, (B, 1))).astype(np.float32)
    KN = (rng.random((B, K)) - 0.5).astype(np.float32)
    return geo, X, Y, KN, P


def _engine(row, B):
    from tests import gpu_checks as G
    from signaltrain_amd.engine import StepEngine
    geo, X, Y, KN, P = _inputs(row, B)
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
        _lib.check(lib.st_reset_tuning(), "st_reset_tuning")


def _train(row, B, code=None):
    """Loss and the 40 gradient tensors after the first of two st_train_steps, the parameters after the second; NaN bit patterns in the workspace before each call."""
    import torch

    def run():
        eng, x, kn, y = _engine(row, B)
        eng.ws.fill_(0xFF); eng.train_step(x, kn, y, LR); torch.cuda.synchronize()
        g = {k: v.cpu().numpy().copy() for k, v in eng.layout.views(eng.grads).items()}; loss = float(eng.scalars[0])
        eng.ws.fill_(0xFF); eng.train_step(x, kn, y, LR); torch.cuda.synchronize()
        g.update({k + "@2": v.cpu().numpy().copy() for k, v in eng.layout.views(eng.grads).items()})      # ... and the gradients of the second step
        return g, (loss, float(eng.scalars[0])), eng.params.cpu().numpy().copy()
    return _with_code(code, run)


@functools.lru_cache(maxsize=None)
def _pair_b64():
    """The pair launch at B = 64, default geometry: shared by the equality, repeatability and graph cases (never modified)."""
    return _train(None, 64)


def _assert_same(a, b):
    (ga, la, pa), (gb, lb, pb) = a, b
    assert len(ga) == 80 and all(np.isfinite(la)) and la == lb, (la, lb)
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    assert np.isfinite(pa).all() and np.array_equal(pa, pb)
    assert any(bool((v != 0).any()) for v in ga.values())


@pytest.mark.parametrize("row,B", [(None, 3), (None, 8), (None, 64), (None, 130), ("n512", 8)])
def test_pair_launch_gives_the_per_gemm_launches_bit_for_bit(row, B):
    pair = _pair_b64() if (row, B) == (None, 64) else _train(row, B)
    _assert_same(pair, _train(row, B, code=PER_GEMM))


def test_pair_launch_repeats_bit_for_bit():
    _assert_same(_train(None, 64), _pair_b64())


def test_graph_replay_gives_the_eager_step():
    import torch
    eng, x, kn, y = _engine(None, 64)
    try:
        eng.graph_capture(64, [LR, LR, LR])
        eng.ws.fill_(0xFF); eng.graph_step(x, kn, y); torch.cuda.synchronize()
        g = {k: v.cpu().numpy().copy() for k, v in eng.layout.views(eng.grads).items()}; loss = float(eng.scalars[0])
        eng.ws.fill_(0xFF); eng.graph_step(x, kn, y); torch.cuda.synchronize()
        g.update({k + "@2": v.cpu().numpy().copy() for k, v in eng.layout.views(eng.grads).items()})
        loss2, p = float(eng.scalars[0]), eng.params.cpu().numpy().copy()
    finally:
        eng.graph_destroy()
    _assert_same((g, (loss, loss2), p), _pair_b64())


def test_loss_backward_gives_the_same_gradients_under_both_schedules():
    import torch

    def run():
        eng, x, kn, y = _engine(None, 64)
        eng.ws.fill_(0xFF); eng.loss_backward(x, kn, y); torch.cuda.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in eng.layout.views(eng.grads).items()}, [float(v) for v in eng.scalars[:5]]
    (ga, sa), (gb, sb) = _with_code(None, run), _with_code(PER_GEMM, run)
    assert sa == sb and all(np.isfinite(sa)), (sa, sb)
    assert len(ga) == 40
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k


def _profile_names(code):
    import torch

    def run():
        eng, x, kn, y = _engine(None, 8)
        lib = eng.lib
        assert lib.st_profile_enable(1) == 0
        try:
            eng.train_step(x, kn, y, LR); torch.cuda.synchronize()
            buf = C.create_string_buffer(1 << 14)
            assert lib.st_profile_report(buf, len(buf)) == 0
        finally:
            lib.st_profile_enable(0)
        return [ln.split()[0] for ln in buf.value.decode().splitlines() if ln.strip()]
    return _with_code(code, run)


def test_event_profile_names_the_schedule():
    names = _profile_names(None)
    assert all(n in names for n in PAIR_NAMES) and not any(n in names for n in GEMM_NAMES), names
    assert "post_ae" in names and "synthesis_dgrad" in names and "clip_adam" in names, names
    names = _profile_names(PER_GEMM)
    assert all(n in names for n in GEMM_NAMES) and not any(n in names for n in PAIR_NAMES), names
