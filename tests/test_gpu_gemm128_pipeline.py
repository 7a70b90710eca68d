"""Round 7: the pipelined k-tile loop of the 128 x 128-tile fp32 weight-gradient kernel (st_gemm_tn.h: gemm_tn128_kernel) against its round-3 loop,
which st_set_tuning(9580) selects.  The pipelined loop moves the barrier, the LDS stores, the global loads and the first fragment reads of the next
k-tile among the MFMAs, and (frame-major rows with a batch that is a multiple of the k-tile depth) addresses a k-tile from wave-uniform frame /
window indices; none of that changes which products are summed or in which order, so every result is the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _case(B, K=4):
    from tests import gpu_checks as G
    geo, X, Y, KN, P = G.make_case(8, 31, K=K)            # the default geometry (8192-sample windows, 1024-tap bases)
    rng = np.random.default_rng(17)
    reps = (B + 7) // 8
    X = (np.tile(X, (reps, 1))[:B] * rng.uniform(0.4, 1.0, (B, 1))).astype(np.float32)
    Y = (np.tile(Y, (reps, 1))[:B] * rng.uniform(0.4, 1.0, (B, 1))).astype(np.float32)
    KN = (rng.random((B, K)) - 0.5).astype(np.float32)
    return geo, G.t(X), G.t(KN), G.t(Y), P


def _run(geo, B, K, x, kn, y, P):
    import torch
    from tests import gpu_checks as G
    from signaltrain_amd.engine import StepEngine
    d = G.dims_of(geo, B, K)
    eng = StepEngine(d, G.DEV); eng.load_state_dict(P)
    eng.loss_backward(x, kn, y); torch.cuda.synchronize()
    g = {k: v.clone() for k, v in eng.layout.views(eng.grads).items()}; l = float(eng.scalars[0])
    eng.train_step(x, kn, y, 1e-3); eng.train_step(x, kn, y, 1e-3); torch.cuda.synchronize()
    return g, l, eng.params.clone()


# 256: the benchmark's batch (wave-uniform addresses, 44 / 14 k-tiles per slice); 130: not a multiple of 32 (per-row addresses, slices whose last
# k-tile runs past the range); 3: one or two k-tiles per slice and empty slices; 64: a multiple of 32 with short slices (wave-uniform addresses, 1-2 k-tiles)
@pytest.mark.parametrize("B", [256, 130, 3, 64])
def test_pipelined_weight_gradient_gemm_is_the_round3_loop_bit_for_bit(B):
    import torch
    from signaltrain_amd import _lib
    lib = _lib.load()
    K = 4
    geo, x, kn, y, P = _case(B, K)
    g_new, l_new, p_new = _run(geo, B, K, x, kn, y, P)
    g_rep, l_rep, p_rep = _run(geo, B, K, x, kn, y, P)
    try:
        _lib.check(lib.st_set_tuning(9580), "st_set_tuning")
        g_old, l_old, p_old = _run(geo, B, K, x, kn, y, P)
    finally:
        _lib.check(lib.st_set_tuning(9581), "st_set_tuning")
    assert np.isfinite(l_new) and l_new != 0.0
    assert any(bool((v != 0).any()) for v in g_new.values())
    # two runs of the new form repeat
    assert l_new == l_rep
    for k in g_new:
        assert torch.equal(g_new[k], g_rep[k]), ("repeat", k)
    assert torch.equal(p_new, p_rep)
    # new form == old form
    assert l_new == l_old, (l_new, l_old)
    for k in g_new:
        assert torch.equal(g_new[k], g_old[k]), k
    assert torch.equal(p_new, p_old)


def test_tuning_code_9580_selects_the_round3_loop_and_reset_restores():
    import ctypes as C
    from signaltrain_amd import _lib
    lib = _lib.load()
    n = lib.st_get_tuning(None, 0)
    cur, dflt = (C.c_int * n)(), (C.c_int * n)()
    lib.st_tuning_defaults(dflt, n)
    try:
        assert lib.st_set_tuning(9580) == 0
        lib.st_get_tuning(cur, n)
        changed = [i for i in range(n) if cur[i] != dflt[i]]
        assert len(changed) == 1 and cur[changed[0]] == 2 and dflt[changed[0]] == 1      # the TN kernel's switch
        assert lib.st_set_tuning(9581) == 0
        lib.st_get_tuning(cur, n)
        assert list(cur) == list(dflt)
    finally:
        lib.st_reset_tuning()
