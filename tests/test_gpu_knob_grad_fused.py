"""st_model_bwd_knobs on the device: d loss / d knobs out of the ONE backward pass of the batch (the autoencoder backward kernels write the per-group column
sums of d a5, one small launch sums a window's groups and applies W5) against the oracle's d_knobs, beside the exact per-window route under the same bound;
the parameter gradients bitwise those of st_model_bwd; st_model.knob_grad_route = "fused" against the reference's autograd (golden G12 / G4); predict.fit_knobs."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = {"f32": 2e-4, "bf16_all": 6e-2, "f16_all": 6e-2}      # tests/test_gpu_parity.py::test_knob_gradient_against_oracle, tests/test_gpu_model_api.py::test_knob_gradient_all_three_outputs

# (scale, shrink, K, B, dtype, g_mag_hat given): each the smallest case that reaches a distinct kernel instantiation or loop state
CASES = [
    (1, 4, 4, 3, "f32", True),          # kept-activation fp32 kernel, VAR 1 (an upstream d / d mag_hat arrives)
    (1, 4, 4, 3, "f32", False),         # VAR 2: T - OT = 16
    (1, 2, 7, 2, "f32", False),         # VAR 0, seven knobs
    (1, 4, 3, 17, "f32", False),        # 561 groups > 128 workgroups x 4 waves: second trip of the persistent group loop, the in-place prefetch live
    (1, 4, 4, 3, "bf16_all", False),    # split decoder kernel, GM false
    (1, 4, 4, 3, "f16_all", True),      # split decoder kernel, GM true
    (1, 4, 4, 33, "bf16_all", False),   # 1089 groups > 128 x 8 waves: second trip of the split kernel's loop
    (2, 4, 4, 3, "f32", False),         # wide path, INNER kernel
    (2, 4, 4, 17, "f32", False),        # wide path, second trip
    (2, 4, 4, 4, "bf16_all", False),    # wide path, 16-bit layers
]


class _arith:
    """The arithmetic of a case on both sides: the engine's compute dtype and the oracle's matching operand rounding (tests/gpu_checks.mixed_mode, without a
    loss scale: the upstream gradients are handed over as they are)."""

    def __init__(self, dtype):
        from tests import gpu_checks as G
        self.ctx = None if dtype == "f32" else G.mixed_mode(2, half="bf16" if dtype == "bf16_all" else "f16", loss_scale=0.0, clip_all=False)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def _oracle_case(scale, shrink, K, B, with_l1):
    """Inputs, parameters and the oracle's d_knobs with the training loss's own upstream gradients: dy always, the L1 term's d / d mag_hat only where the case
    hands it over (without it the reference is the oracle's d_knobs of the log-cosh term alone: its L1 weight set to zero for the call)."""
    from oracle import st_oracle as O
    from tests import gpu_checks as G
    geo, X, Y, KN, P = G.make_case(B=B, seed=31, scale=scale, shrink=shrink, K=K)
    lam = O.L1_LAMBDA
    try:
        if not with_l1:
            O.L1_LAMBDA = 0.0
        _, _, c = O.model_loss_bwd(X, KN, Y, P, geo)
    finally:
        O.L1_LAMBDA = lam
    F = geo["F"]
    w = O.freq_weights(F, np.float32)
    g_mh = None
    if with_l1:
        g_mh = (np.float32(O.L1_LAMBDA / 10) / np.float32(B * geo["OT"] * F) * np.sign(c["mag_hat"]) * w).astype(np.float32)      # the L1 term of calc_loss (loss_functions.py:36)
    return geo, X, KN, P, c["dy"], g_mh, c["d_knobs"].astype(np.float64)


@pytest.mark.parametrize("scale,shrink,K,B,dtype,with_l1", CASES)
def test_fused_knob_gradient_against_oracle(scale, shrink, K, B, dtype, with_l1):
    """backward_with_knob_grad's g_knobs against the oracle's d_knobs at the project's tolerance for this quantity (2e-4 of max|ref| in fp32, 6e-2 with 16-bit
    layers) -- and the exact per-window route under the same bound in the same test, so that a miss tells kernel from oracle."""
    from tests import gpu_checks as G
    with _arith(dtype):
        geo, X, KN, P, dy, g_mh, ref = _oracle_case(scale, shrink, K, B, with_l1)
        d = G.dims_of(geo, B, K)
        eng = G.new_engine(d); eng.load_state_dict(P)
        assert eng.compute_dtype == dtype and eng.knob_grad_fused_supported(B)
        x, kn, gy = G.t(X), G.t(KN), G.t(dy)
        gm = None if g_mh is None else G.t(g_mh)
        eng.forward(x, kn, save_for_backward=True)
        grads, gk = eng.backward_with_knob_grad(x, kn, gy, gm)
        fused = gk.cpu().numpy().astype(np.float64)
        slow = eng.knob_grad(x, kn, gy, gm).cpu().numpy().astype(np.float64)
    assert fused.shape == slow.shape == ref.shape == (B, K)
    sc = np.abs(ref).max()
    ef, es = np.abs(fused - ref).max() / sc, np.abs(slow - ref).max() / sc
    print(f"knob grad vs oracle, scale {scale} shrink {shrink} K {K} B {B} {dtype} l1 {with_l1}: fused {ef:.3e}  per-window {es:.3e}  fused vs per-window {np.abs(fused - slow).max() / sc:.3e}  tol {TOL[dtype]:.0e}")
    assert np.all(np.isfinite(fused))
    assert es <= TOL[dtype], ("per-window route", es, slow, ref)
    assert ef <= TOL[dtype], ("fused route", ef, fused, ref)


@pytest.mark.parametrize("scale,dtype,with_l1", [(1, "f32", False), (1, "f32", True), (1, "bf16_all", False), (2, "f32", False), (2, "f16_all", False)])
def test_same_state_parameter_gradients_are_bitwise_those_of_backward(scale, dtype, with_l1):
    """After ONE forward(save_for_backward=True): backward() and backward_with_knob_grad() leave eng.grads bitwise equal (the flag only adds stores), a second
    backward_with_knob_grad() repeats g_knobs bit for bit (fixed summation order, scratch never cleared), and a backward() after it still works without a new
    forward (the saved state is still the batch's)."""
    from tests import gpu_checks as G
    B, K = 4, 4
    with _arith(dtype):
        geo, X, KN, P, dy, g_mh, _ = _oracle_case(scale, 4, K, B, with_l1)
        eng = G.new_engine(G.dims_of(geo, B, K)); eng.load_state_dict(P)
        x, kn, gy = G.t(X), G.t(KN), G.t(dy)
        gm = None if g_mh is None else G.t(g_mh)
        eng.forward(x, kn, save_for_backward=True)
        gen = eng.generation
        g0 = eng.backward(x, kn, gy, gm).clone()
        g1, k1 = eng.backward_with_knob_grad(x, kn, gy, gm); g1 = g1.clone()
        eng._knob_groups.fill_(float("nan"))              # whatever the scratch held: every element read is written first
        g2, k2 = eng.backward_with_knob_grad(x, kn, gy, gm); g2 = g2.clone()
        g3 = eng.backward(x, kn, gy, gm).clone()
        assert eng.generation == gen
    assert torch.isfinite(k1).all() and float(k1.abs().max()) > 0
    assert torch.equal(g1, g0) and torch.equal(g2, g0) and torch.equal(g3, g0)
    assert torch.equal(k2, k1)


def _golden_model(golden_dir):
    from tests.test_gpu_model_api import _golden_model as gm
    return gm(golden_dir)


@pytest.mark.parametrize("dtype", ["f32", "bf16_all"])
def test_window_independence(golden_dir, dtype):
    """The form of test_knob_gradient_all_three_outputs on the fused route: upstream gradients of ALL outputs, B = 3 with distinct windows, against float64
    torch-CPU autograd of the reference op sequence -- and although the whole batch goes through one pass, window 1's gradient is BITWISE unchanged when
    windows 0 and 2 change (a window's groups are its own, summed in a fixed order), while window 0's does change."""
    from oracle import torch_cpu_step as TC
    m, g, P, geo = _golden_model(golden_dir)
    m.set_compute_dtype(dtype)
    m.knob_grad_route = "fused"
    rng = np.random.default_rng(21)
    B = 3
    x = (0.3 * rng.standard_normal((B, geo["L"]))).astype(np.float32)
    kn = (rng.random((B, 4)) - 0.5).astype(np.float32)
    p1 = rng.standard_normal((B, geo["y"])).astype(np.float32)
    p2 = (0.1 * rng.standard_normal((B, geo["T"], geo["F"]))).astype(np.float32)
    p3 = (0.1 * rng.standard_normal((B, geo["OT"], geo["F"]))).astype(np.float32)
    P64 = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in P.items()}
    k64 = torch.tensor(kn, dtype=torch.float64, requires_grad=True)
    y, mg, mh = TC.forward(P64, torch.tensor(x, dtype=torch.float64), k64)
    ((y * torch.tensor(p1, dtype=torch.float64)).sum() + (mg * torch.tensor(p2, dtype=torch.float64)).sum()
     + (mh * torch.tensor(p3, dtype=torch.float64)).sum()).backward()
    ref = k64.grad.numpy()

    def run(xx):
        kg = torch.from_numpy(kn).cuda().requires_grad_(True)
        yg, mgg, mhg = m.forward(torch.from_numpy(xx).cuda(), kg)
        ((yg * torch.from_numpy(p1).cuda()).sum() + (mgg * torch.from_numpy(p2).cuda()).sum() + (mhg * torch.from_numpy(p3).cuda()).sum()).backward()
        return kg.grad.detach().cpu().numpy().astype(np.float64)
    got = run(x)
    tol = TOL[dtype]
    print(f"fused knob grad, all three outputs, {dtype}: {np.abs(got - ref).max() / np.abs(ref).max():.3e} (tol {tol:.0e})")
    assert np.abs(got - ref).max() <= tol * np.abs(ref).max(), (got, ref)
    x2 = x.copy(); x2[0] *= -0.5; x2[2] = x2[2][::-1]
    got2 = run(x2)
    assert np.array_equal(got2[1], got[1]) and not np.array_equal(got2[0], got[0])


def _g12_run(m, g, route_check=None):
    from signaltrain_amd import loss_functions
    x, yt = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["y"]).cuda()
    kn = torch.from_numpy(g["knobs"]).cuda().requires_grad_(True)
    m.zero_grad()
    y, mag, mag_hat = m.forward(x, kn)
    if route_check is not None:
        route_check(x, kn)
    sbf = torch.exp((7. / 513) * torch.arange(0., 513, device="cuda")).expand_as(mag_hat).float()
    loss_functions.calc_loss(y, yt, mag_hat, scale_by_freq=sbf).backward()
    return kn.grad.detach().cpu().numpy().astype(np.float64), {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in m.named_parameters()}


def _check_g12_g4(got, grads, golden_dir):
    from tests.golden_util import ae_keys
    g4 = np.load(os.path.join(golden_dir, "g4_backward.npz")); g12 = np.load(os.path.join(golden_dir, "g12_knob_grad.npz"))
    ref = g12["d_knobs"]
    assert got.shape == ref.shape == (2, 4)
    e = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"fused route vs golden G12: {e:.3e}")
    assert e <= 2e-4, (got, ref)
    for k in ae_keys():
        assert np.abs(grads[k] - g4["g_" + k]).max() <= 2e-4 * np.abs(g4["g_" + k]).max() + 1e-12, k


def test_st_model_fused_route_matches_reference_autograd(golden_dir):
    """st_model.knob_grad_route = "fused": kn.grad against the REFERENCE's own autograd (golden G12) and the parameter gradients of the same backward() against
    golden G4, as test_knob_gradient_matches_reference_autograd checks the exact route -- with ONE backward_with_knob_grad call, no per-window pass and no
    second forward.  Then the stale generation stamp: another forward in between makes the backward rebuild its state first (one more forward), same gradients."""
    m, g, P, geo = _golden_model(golden_dir)
    assert m.knob_grad_route == "exact"                  # the default every other test runs under
    with pytest.raises(ValueError):
        m.knob_grad_route = "quick"
    m.knob_grad_route = "fused"
    eng = m.engine(torch.from_numpy(g["x"]).cuda())
    calls = {"forward": 0, "fused": 0, "exact": 0}
    fwd, fused, exact = eng.forward, eng.backward_with_knob_grad, eng.knob_grad

    def count(name, fn):
        def wrapped(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapped
    eng.forward, eng.backward_with_knob_grad, eng.knob_grad = count("forward", fwd), count("fused", fused), count("exact", exact)
    got, grads = _g12_run(m, g)
    assert m.mpaec._engine is eng
    assert calls == {"forward": 1, "fused": 1, "exact": 0}, calls
    _check_g12_g4(got, grads, golden_dir)
    # a validation batch between forward and backward: the stamp is stale, the state is rebuilt
    calls.update(forward=0, fused=0, exact=0)
    got, grads = _g12_run(m, g, route_check=lambda x, kn: eng.forward(torch.flip(x.detach(), dims=(1,)).contiguous(), kn.detach()))
    assert calls == {"forward": 3, "fused": 1, "exact": 0}, calls
    _check_g12_g4(got, grads, golden_dir)


def test_st_model_fused_route_falls_back_where_unsupported(golden_dir):
    """A batch the library does not run in one pass (here: the diagnostic switch that makes the fp32 backward recompute its activations) takes the exact route."""
    from signaltrain_amd import _lib
    m, g, P, geo = _golden_model(golden_dir)
    m.knob_grad_route = "fused"
    eng = m.engine(torch.from_numpy(g["x"]).cuda())
    lib = _lib.load()
    try:
        _lib.check(lib.st_set_tuning(8200), "st_set_tuning")
        assert not eng.knob_grad_fused_supported(2)
        with pytest.raises(RuntimeError, match="g_ae_save"):
            x, kn = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["knobs"]).cuda()
            eng.forward(x, kn, save_for_backward=True)
            eng.backward_with_knob_grad(x, kn, torch.zeros(2, geo["y"], device="cuda"))
        got, grads = _g12_run(m, g)
    finally:
        lib.st_reset_tuning()
    _check_g12_g4(got, grads, golden_dir)


def test_knobless_model_returns_an_empty_gradient():
    from tests import gpu_checks as G
    geo, X, Y, KN, P = G.make_case(B=2, seed=3, K=0)
    eng = G.new_engine(G.dims_of(geo, 2, 0)); eng.load_state_dict(P)
    assert not eng.knob_grad_fused_supported(2)
    x, kn = G.t(X), torch.empty(2, 0, device=G.DEV)
    gy = torch.full((2, geo["y"]), 1e-3, device=G.DEV)
    eng.forward(x, kn, save_for_backward=True)
    g0 = eng.backward(x, kn, gy).clone()
    g1, gk = eng.backward_with_knob_grad(x, kn, gy)
    assert gk.shape == (2, 0) and torch.equal(g1, g0)


def test_fit_knobs_recovers_the_models_own_settings(golden_dir):
    """predict.fit_knobs on the golden model: 3 windows of seeded noise, the target is the model's own predict_long output at a seeded k* != 0 (so the loss at
    k* is zero and the loss at the start vector, zeros, is not), 50 Adam steps from zeros.  The loss goes down, the result stays in [-0.5, 0.5], and the first
    step's gradient is the window sum of backward_with_knob_grad's output for g_y_hat = tanh(y_hat - target) / n."""
    from signaltrain_amd import predict
    m, g, P, geo = _golden_model(golden_dir)
    chunk, out = m.in_chunk_size, m.out_chunk_size
    rng = np.random.default_rng(5)
    nwin = 3
    n = chunk + (nwin - 1) * out
    signal = (0.3 * rng.standard_normal(n)).astype(np.float32)
    k_star = (rng.random(4) - 0.5).astype(np.float32)
    assert np.abs(k_star).min() > 0
    pred = predict.predict_long(signal, k_star, m, chunk, out)
    assert pred.shape == (n - (chunk - out),)
    target = np.zeros(n, np.float32); target[chunk - out:] = pred
    hist_g = []
    k_fit, hist = predict.fit_knobs(signal, target, m, chunk, out, steps=50, lr=0.05, grad_history=hist_g)
    print(f"fit_knobs: loss {hist[0]:.4e} -> {hist[-1]:.4e}; k* {k_star}, fitted {k_fit}, |k - k*| {np.abs(k_fit - k_star)} (max {np.abs(k_fit - k_star).max():.3e})")
    assert len(hist) == 50 and k_fit.shape == (4,) and np.all(np.isfinite(hist))
    assert hist[-1] < hist[0]
    assert np.all(np.abs(k_fit) <= 0.5)
    # the first step's gradient, by hand
    eng = m.engine(torch.zeros(nwin, chunk, device="cuda"))
    x = torch.from_numpy(np.stack([signal[w * out:w * out + chunk] for w in range(nwin)])).cuda()
    t = torch.from_numpy(np.stack([target[w * out + chunk - out:w * out + chunk] for w in range(nwin)])).cuda()
    kn = torch.zeros(nwin, 4, device="cuda")
    y_hat = eng.forward(x, kn, save_for_backward=True)[0]
    gk = eng.backward_with_knob_grad(x, kn, torch.tanh(y_hat - t) / float(nwin * out))[1]
    want = gk.sum(0).cpu().numpy()
    assert np.abs(want).max() > 0
    np.testing.assert_allclose(hist_g[0], want, rtol=1e-6, atol=0)
