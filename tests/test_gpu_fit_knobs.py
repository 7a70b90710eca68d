"""GPU: the knob fit on the device -- st_fit_knobs / StepEngine.fit_knobs / predict.fit_knobs(route="device").

The recording and its target stay in HBM; one C call enqueues every batch of every optimiser step: the forward of st_predict_long with the code h4 kept, the
overlap-add with the loss side, the synthesis data-gradient GEMM, the knob-only autoencoder backward, the per-window reduce and the Adam tail.  Checked
against the float64 reference of tests/fit_knobs_ref.py (conditioning asserted on the CPU by tests/test_fit_knobs_host.py), against the existing route on
the same windows materialised on the host, and for chaining, repeatability, formats, the Adam tail and everything it must leave alone."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from oracle import st_oracle as O
from signaltrain_amd import _lib
from tests import fit_knobs_ref as R
from tests import gpu_checks as G
from tests.test_gpu_predict_long import LEVELS

pytestmark = pytest.mark.gpu

K = R.K
B = 4                   # nine windows in batches of four: the last batch is one window whose tail lies behind the recording's end
KNOB_NW = 12            # waves per workgroup of ae_knob_bwd_kernel (AE_KNOB_NW, csrc/st_api.hip); its grid is at most half the CUs per net
_REF = {}


def engine(row, batch=B):
    geo, P = R.case(row)
    eng = G.new_engine(G.dims_of(geo, batch, K)); eng.load_state_dict(P)
    return eng, geo, P


def knob_rows(nwin):
    """One distinct, seeded row per window, inside (-0.45, 0.45)."""
    return (0.9 * (np.random.default_rng(17).random((nwin, K)) - 0.5)).astype(np.float32)


def reference(row, per_window):
    """(J, gradient) of the float64 reference at R.KN (one row: the window sum) or at knob_rows (one row per window); computed once per case, never modified."""
    key = (row, per_window)
    if key not in _REF:
        geo, P = R.case(row)
        sig, tgt = R.pair(row)
        nwin = R.windows(sig, geo).shape[0]
        J, g, _ = R.objective(sig, tgt, knob_rows(nwin) if per_window else R.KN, P, geo)
        _REF[key] = (J, g if per_window else g.sum(0, keepdims=True))
    return _REF[key]


def one_step(eng, sig, tgt, kn, batch=B, **kw):
    """steps = 1, lr = 0: the loss and the gradient at kn, the knobs untouched."""
    k, loss, grads, _ = eng.fit_knobs(G.t(sig) if isinstance(sig, np.ndarray) else sig, G.t(tgt) if isinstance(tgt, np.ndarray) else tgt,
                                      G.t(kn), steps=1, lr=0.0, batch=batch, want_grads=True, **kw)
    return float(loss[0]), G.n(grads[0]), k


@pytest.mark.parametrize("per_window", [False, True], ids=["one_row", "row_per_window"])
@pytest.mark.parametrize("row", R.ROWS)
def test_fp32_gradient_and_loss_against_the_float64_reference(row, per_window):
    """steps = 1, lr = 0, fp32: grad_hist[0] within 2e-4 of max|ref| of the reference gradient (the project's knob-gradient bound), loss_hist[0] within
    gpu_checks.TOL relative of the reference J; for one knob row (the sum over the windows) and for one row per window (each window's own gradient)."""
    eng, geo, P = engine(row)
    sig, tgt = R.pair(row)
    nwin = R.windows(sig, geo).shape[0]
    assert nwin == 9
    kn = knob_rows(nwin) if per_window else R.KN
    J, g = reference(row, per_window)
    loss, grad, k = one_step(eng, sig, tgt, kn)
    assert grad.shape == g.shape and torch.equal(k.reshape(-1), G.t(kn).reshape(-1))      # lr = 0: the knobs stay
    eg = float(np.abs(grad - g).max() / np.abs(g).max())
    eJ = abs(loss - J) / abs(J)
    print(f"fit_knobs vs float64 reference [{row or 'default'} {'per window' if per_window else 'one row'}]: grad {eg:.2e} (tol {R.TOL_GRAD['f32']:.0e})  J {eJ:.2e} (tol {G.TOL:.0e})")
    assert eg <= R.TOL_GRAD["f32"], (row, eg, grad, g)
    assert eJ <= G.TOL, (row, eJ, loss, J)


def second_trip_batch(geo):
    """The smallest batch whose group count exceeds grid x waves of ae_knob_bwd_kernel: its persistent loop takes a second trip."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_pass = max(cus // 2, 1) * KNOB_NW
    gpw = int(_lib.load().st_kp(geo["F"])) // 32
    return per_pass // gpw + 1


def test_second_trip_of_the_persistent_loop():
    """Default geometry, one batch of the smallest size at which B * 33 groups exceed (CUs / 2) x 12 waves (B = 47 on 256 CUs): the prefetch of the next
    group is live.  Same reference, same bounds."""
    geo, P = R.case(None)
    nb = second_trip_batch(geo)
    eng, _, _ = engine(None, nb)
    n = geo["L"] + (nb - 1) * geo["y"] - 5 * 4 - 1          # nb windows, the last one cut short
    sig = R.signal(n, seed=9); tgt = R.target_of(sig)
    assert R.windows(sig, geo).shape[0] == nb
    J, g, _ = R.objective(sig, tgt, R.KN, P, geo)
    g = g.sum(0, keepdims=True)
    loss, grad, _ = one_step(eng, sig, tgt, R.KN, batch=nb)
    eg, eJ = float(np.abs(grad - g).max() / np.abs(g).max()), abs(loss - J) / abs(J)
    print(f"fit_knobs second trip: B={nb} groups={nb * (int(_lib.load().st_kp(geo['F'])) // 32)} grad {eg:.2e} J {eJ:.2e}")
    assert eg <= R.TOL_GRAD["f32"] and eJ <= G.TOL, (nb, eg, eJ)


@pytest.mark.parametrize("row", ["n256", None])
@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_16bit_layers_against_the_mixed_mode_oracle(half, row):
    """bf16_all / f16_all against the oracle under mixed_mode(2, loss_scale=0, clip_all=False): 6e-2 of max|ref| (tests/test_gpu_knob_grad_fused.py TOL)."""
    with G.mixed_mode(2, half=half, loss_scale=0.0, clip_all=False):
        eng, geo, P = engine(row)
        sig, tgt = R.pair(row)
        J, g, _ = R.objective(sig, tgt, R.KN, P, geo, dtype=np.float32)
        loss, grad, _ = one_step(eng, sig, tgt, R.KN)
    g = g.sum(0, keepdims=True)
    eg, eJ = float(np.abs(grad - g).max() / np.abs(g).max()), abs(loss - J) / abs(J)
    print(f"fit_knobs vs mixed-mode oracle [{half}_all {row or 'default'}]: grad {eg:.2e} J {eJ:.2e}")
    assert np.all(np.isfinite(grad)) and eg <= R.TOL_GRAD[half + "_all"] and eJ <= 6e-2, (half, row, eg, eJ)


@pytest.mark.parametrize("row", ["n256", None])
@pytest.mark.parametrize("level", list(LEVELS))
def test_every_level_against_the_existing_route(level, row):
    """All six levels against forward(save_for_backward=True) + backward_with_knob_grad(g_y = tanh(y_hat - t) / n_out, the tail masked) on the same windows
    materialised on the host: 2e-4 (f32, f32x3) / 6e-2 (the 16-bit levels) of max|ref|.  The deviation seen is printed."""
    with LEVELS[level]():
        eng, geo, P = engine(row)
        sig, tgt = R.pair(row)
        L, y = geo["L"], geo["y"]
        n_out = sig.size - (L - y)
        xw = R.windows(sig, geo); tw = R.windows(tgt, geo)[:, L - y:]
        nwin = xw.shape[0]
        valid = G.t((np.arange(nwin * y) < n_out).reshape(nwin, y).astype(np.float32))
        ref = torch.zeros(K, dtype=torch.float64, device=G.DEV)
        for b0 in range(0, nwin, B):
            xb, tb = G.t(xw[b0:b0 + B]), G.t(tw[b0:b0 + B])
            kb = G.t(np.tile(R.KN, (xb.shape[0], 1)))
            y_hat = eng.forward(xb, kb, save_for_backward=True)[0]
            g_y = (torch.tanh(y_hat - tb) * valid[b0:b0 + B] / float(n_out)).contiguous()
            ref += eng.backward_with_knob_grad(xb, kb, g_y)[1].double().sum(0)
        ref = ref.cpu().numpy()
        _, grad, _ = one_step(eng, sig, tgt, R.KN)
    e = float(np.abs(grad[0] - ref).max() / np.abs(ref).max())
    print(f"fit_knobs vs backward_with_knob_grad [{level} {row or 'default'}]: {e:.2e} (tol {R.TOL_GRAD[level]:.0e})")
    assert e <= R.TOL_GRAD[level], (level, row, e, grad, ref)


def test_long_recording_keeps_its_gradient_on_fp16():
    """n256 / f16_all, n_out > 2^17: the seeded signal tiled with a period of eight hops.  tanh / n_out is below 7.6e-6 here and shrinks with the length; applied
    ahead of the 16-bit operand of the data-gradient GEMM it would lose the gradient to fp16's subnormal range, applied behind W5 it does not.  Reference: the
    mixed-mode oracle on the distinct windows (one period and the ragged end), each window's unscaled gradient counted as often as the window occurs and the sum
    scaled by 1 / n_out the same way.  Bound: 6e-2 of max|ref|."""
    with G.mixed_mode(2, half="f16", loss_scale=0.0, clip_all=False):
        nb = 64
        eng, geo, P = engine("n256", nb)
        L, y = geo["L"], geo["y"]
        period = 8
        reps = (1 << 17) // (period * y) + 2
        base = R.signal(period * y, seed=21)
        sig = np.tile(base, reps)[:period * y * reps - 100]
        tgt = R.target_of(sig, seed=23)
        tgt = np.tile(tgt[period * y:2 * period * y], reps)[:sig.size]          # periodic as well
        n_out = sig.size - (L - y)
        assert n_out > (1 << 17)
        xw = R.windows(sig, geo); tw = R.windows(tgt, geo)[:, L - y:]
        nwin = xw.shape[0]
        valid = (np.arange(nwin * y) < n_out).reshape(nwin, y)
        both = np.concatenate([xw, tw, valid.astype(np.float32)], axis=1)
        uniq, inverse, counts = np.unique(both, axis=0, return_inverse=True, return_counts=True)
        assert uniq.shape[0] <= period + (L // y) + 2, uniq.shape
        ux, ut, uv = uniq[:, :L], uniq[:, L:L + y], uniq[:, L + y:] > 0
        nu = ux.shape[0]
        kn = np.tile(R.KN, (nu, 1))
        out = O.model_fwd(ux, kn, P, geo)[0]
        lam = O.L1_LAMBDA
        try:
            O.L1_LAMBDA = 0.0
            _, _, c = O.model_loss_bwd(ux, kn, np.where(uv, ut, out).astype(np.float32), P, geo)
        finally:
            O.L1_LAMBDA = lam
        ref = (c["d_knobs"].astype(np.float64) * counts[:, None]).sum(0) * (nu * y / n_out)
        _, grad, _ = one_step(eng, sig, tgt, R.KN, batch=nb)
    e = float(np.abs(grad[0] - ref).max() / np.abs(ref).max())
    print(f"fit_knobs long recording [f16_all n256]: n_out={n_out} windows={nwin} distinct={nu} grad {grad[0]} ref {ref} dev {e:.2e}")
    assert np.abs(ref).max() > 0 and e <= R.TOL_GRAD["f16_all"], (e, grad, ref)


@pytest.mark.parametrize("per_window", [False, True], ids=["one_row", "row_per_window"])
@pytest.mark.parametrize("level", ["f32", "bf16_all"])
def test_chained_single_steps_are_one_call_bit_for_bit(level, per_window):
    with LEVELS[level]():
        eng, geo, P = engine("n256")
        sig, tgt = (G.t(a) for a in R.pair("n256"))
        k0 = G.t(knob_rows(9) if per_window else R.KN)
        kA, lA, gA, (mA, vA, nA) = eng.fit_knobs(sig, tgt, k0, steps=3, batch=B, want_grads=True)
        k, st, ls, gs = k0, None, [], []
        for _ in range(3):
            k, l, g, st = eng.fit_knobs(sig, tgt, k, steps=1, batch=B, want_grads=True, state=st)
            ls.append(l); gs.append(g)
    assert nA == st[2] == 4
    assert torch.equal(kA, k) and torch.equal(mA, st[0]) and torch.equal(vA, st[1])
    assert torch.equal(lA, torch.cat(ls)) and torch.equal(gA, torch.cat(gs))
    assert not torch.equal(kA, k0) and float(lA[2]) != float(lA[0])


@pytest.mark.parametrize("level", ["f32", "f16_all"])
def test_repeated_call_repeats_its_bits_whatever_the_workspace_held(level):
    """Two identical calls, the workspace filled with NaN in between: every element read is written first, every reduction has a fixed order."""
    with LEVELS[level]():
        eng, geo, P = engine(None)
        sig, tgt = (G.t(a) for a in R.pair(None))
        a = eng.fit_knobs(sig, tgt, G.t(R.KN), steps=2, batch=B, want_grads=True)
        eng._fit_ws.view(torch.float32).fill_(float("nan"))
        b = eng.fit_knobs(sig, tgt, G.t(R.KN), steps=2, batch=B, want_grads=True)
    for x, y in zip(a[:3] + a[3][:2], b[:3] + b[3][:2]):
        assert torch.isfinite(x).all() and torch.equal(x, y)


def test_int16_pair_and_its_float32_image_give_equal_bits():
    eng, geo, P = engine("n256")
    sig, tgt = R.pair("n256")
    s16 = np.round(sig * 20000).astype(np.int16); t16 = np.round(tgt * 20000).astype(np.int16)
    sf = (s16.astype(np.float64) / 32767.0).astype(np.float32); tf = (t16.astype(np.float64) / 32767.0).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).to(G.DEV)
    a = eng.fit_knobs(dev(s16), dev(t16), G.t(R.KN), steps=2, batch=B, want_grads=True)
    b = eng.fit_knobs(dev(sf), dev(tf), G.t(R.KN), steps=2, batch=B, want_grads=True)
    c = eng.fit_knobs(dev(s16), dev(tf), G.t(R.KN), steps=2, batch=B, want_grads=True)          # mixed: the int16 one converted on the device
    # views 8 bytes off a 16-byte boundary, through the wrapper: float32 (realigned by a copy) and int16 (8-byte aligned: taken as it is)
    pad_f = torch.zeros(sf.size + 2, dtype=torch.float32, device=G.DEV); pad_f[2:] = dev(sf)
    pad_s = torch.zeros(s16.size + 4, dtype=torch.int16, device=G.DEV); pad_s[4:] = dev(s16)
    assert pad_f[2:].data_ptr() % 16 == 8 and pad_s[4:].data_ptr() % 16 == 8
    d = eng.fit_knobs(pad_f[2:], dev(tf), G.t(R.KN), steps=2, batch=B, want_grads=True)
    e = eng.fit_knobs(pad_s[4:], dev(t16), G.t(R.KN), steps=2, batch=B, want_grads=True)
    for other in (b, c, d, e):
        for x, y in zip(a[:3], other[:3]):
            assert torch.equal(x, y)
    assert float(a[1][0]) > 0


@pytest.mark.parametrize("per_window", [False, True], ids=["one_row", "row_per_window"])
def test_adam_tail_against_the_float64_replay(per_window):
    """The knobs after 10 steps against the float64 replay of Adam + clamp on the returned grad_hist.  Bound: 4 x the deviation torch's own float32 CPU Adam
    (foreach=False) shows from that replay on the same history -- the rule of tests/adam_reference.py -- or one unit u = 2^-24 of the knob scale 0.5 where that
    is smaller.  The start vector puts one knob at 0.499 with a gradient that pushes it out: the clamp acts."""
    eng, geo, P = engine("n256")
    sig, tgt = (G.t(a) for a in R.pair("n256"))
    k0 = (knob_rows(9) if per_window else R.KN.copy()).astype(np.float32).reshape(-1, K)
    probe = one_step(eng, sig, tgt, k0 if per_window else R.KN)[1]          # [rows, K]
    j = int(np.argmax(np.abs(probe).min(0)))
    k0[:, j] = -0.499 * np.sign(probe[:, j])                 # Adam moves against the gradient: outwards
    k0 = k0.reshape((9, K) if per_window else (K,))
    k, loss, grads, (m, v, nxt) = eng.fit_knobs(sig, tgt, G.t(k0), steps=10, lr=0.05, batch=B, want_grads=True)
    gh = G.n(grads).reshape((10,) + k0.shape)
    want, wm, wv = R.adam_replay(k0, gh)
    p = torch.tensor(k0, requires_grad=True)
    opt = torch.optim.Adam([p], lr=0.05, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    for g in gh:
        p.grad = torch.tensor(g.astype(np.float32))
        opt.step()
        with torch.no_grad():
            p.clamp_(-0.5, 0.5)
    yard = float(np.abs(p.detach().numpy().astype(np.float64) - want).max())
    u = 0.5 * 2.0 ** -24
    bound = max(4 * yard, u)
    dev = float(np.abs(G.n(k).reshape(k0.shape) - want).max())
    print(f"fit_knobs Adam tail [{'per window' if per_window else 'one row'}]: device {dev:.3e}  torch float32 {yard:.3e}  u {u:.3e}  bound {bound:.3e}")
    assert nxt == 11 and np.abs(want).max() == 0.5 and np.array_equal(np.abs(G.n(k).reshape(k0.shape)) == 0.5, np.abs(want) == 0.5)
    assert dev <= bound, (dev, yard, bound)
    # the moments: the C ABI takes the betas as float32, so 1 - beta differs from the replay's by up to 2^-24 * beta / (1 - beta) relative -- 5.4e-7 for
    # beta1 = 0.9, 6e-5 for beta2 = 0.999 -- and that factor scales every term of the moment; ten float32 roundings (6e-8 each) come on top: 1e-5 and 1e-4
    assert np.abs(G.n(m).reshape(k0.shape) - wm).max() <= 1e-5 * np.abs(wm).max() and np.abs(G.n(v).reshape(k0.shape) - wv).max() <= 1e-4 * np.abs(wv).max()


def test_leaves_everything_else_alone():
    """eng.params, eng.grads, eng.ws and the predict workspace keep their contents; nothing is written behind loss_hist + steps or behind grad_hist's end."""
    eng, geo, P = engine("n256")
    sig, tgt = (G.t(a) for a in R.pair("n256"))
    eng.predict_long(sig, G.t(R.KN), batch=B)                 # allocates the predict workspace
    eng.grads.normal_(); eng.ws.random_(0, 255)
    before = [t.clone() for t in (eng.params, eng.grads, eng.ws, eng._predict_ws)]
    gen = eng.generation
    eng.fit_knobs(sig, tgt, G.t(R.KN), steps=2, batch=B, want_grads=True)
    torch.cuda.synchronize()
    for a, b in zip(before, (eng.params, eng.grads, eng.ws, eng._predict_ws)):
        assert torch.equal(a, b)
    assert eng.generation == gen
    # the C call itself, with guard elements behind both histories
    lib = _lib.load()
    steps, rows = 2, 9
    d = eng.dims.with_batch(B)
    kn = G.t(knob_rows(rows)); m = torch.zeros_like(kn); v = torch.zeros_like(kn)
    loss = torch.full((steps + 4,), -7.0, dtype=torch.float64, device=G.DEV)
    grad = torch.full((steps * rows * K + 16,), -7.0, dtype=torch.float32, device=G.DEV)
    rc = lib.st_fit_knobs(C.byref(d), _lib.ptr(eng.params), _lib.PCM_F32, C.c_void_p(sig.data_ptr()), C.c_void_p(tgt.data_ptr()), sig.numel(),
                          _lib.ptr(kn), rows, _lib.ptr(m), _lib.ptr(v), 1, steps, 0.05, 0.9, 0.999, 1e-8,
                          C.c_void_p(loss.data_ptr()), _lib.ptr(grad), _lib.ptr(eng._fit_ws), G.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.st_last_error()
    assert bool((loss[steps:] == -7.0).all()) and bool((loss[:steps] > 0).all())
    assert bool((grad[steps * rows * K:] == -7.0).all()) and bool((grad[:steps * rows * K] != -7.0).all())


def _golden_model(golden_dir):
    from tests.test_gpu_model_api import _golden_model as gm
    return gm(golden_dir)


def test_device_route_on_the_golden_model(golden_dir):
    """The form of test_fit_knobs_recovers_the_models_own_settings on route="device": 3 windows, the target is the model's own prediction at a seeded k*, 50
    steps from zeros.  The loss falls, the result stays in [-0.5, 0.5], and the first step's gradient agrees with the batched route's within the 2e-4 bound
    (n = L + 2 y: the two objectives coincide)."""
    from signaltrain_amd import predict
    m, g, P, geo = _golden_model(golden_dir)
    chunk, out = m.in_chunk_size, m.out_chunk_size
    rng = np.random.default_rng(5)
    n = chunk + 2 * out
    signal = (0.3 * rng.standard_normal(n)).astype(np.float32)
    k_star = (rng.random(4) - 0.5).astype(np.float32)
    pred = predict.predict_long(signal, k_star, m, chunk, out)
    target = np.zeros(n, np.float32); target[chunk - out:] = pred
    hg_dev, hg_bat = [], []
    k_fit, hist = predict.fit_knobs(signal, target, m, chunk, out, steps=50, lr=0.05, grad_history=hg_dev, route="device")
    predict.fit_knobs(signal, target, m, chunk, out, steps=1, lr=0.05, grad_history=hg_bat)
    e = float(np.abs(hg_dev[0] - hg_bat[0]).max() / np.abs(hg_bat[0]).max())
    print(f"fit_knobs(route='device'): loss {hist[0]:.4e} -> {hist[-1]:.4e}; k* {k_star}, fitted {k_fit}; first gradient vs batched route {e:.2e}")
    assert len(hist) == 50 and len(hg_dev) == 50 and k_fit.shape == (4,) and k_fit.dtype == np.float32 and np.all(np.isfinite(hist))
    assert hist[-1] < hist[0] and np.all(np.abs(k_fit) <= 0.5)
    assert e <= R.TOL_GRAD["f32"], e
    # one row per window: init [nwin, K]
    k_rows, hist_rows = predict.fit_knobs(signal, target, m, chunk, out, steps=3, lr=0.05, init=np.zeros((3, 4), np.float32), route="device")
    assert k_rows.shape == (3, 4) and len(hist_rows) == 3 and abs(hist_rows[0] - hist[0]) <= 1e-12 + 1e-6 * hist[0]


def test_wide_geometry_falls_back_to_the_batched_route():
    from signaltrain_amd import nn_proc, predict
    nn_proc._QUIET = True
    torch.manual_seed(3)
    m = nn_proc.st_model(scale_factor=2, shrink_factor=4, num_knobs=4).to(G.DEV)
    chunk, out = m.in_chunk_size, m.out_chunk_size
    rng = np.random.default_rng(8)
    signal = (0.3 * rng.standard_normal(chunk + out)).astype(np.float32)
    target = np.tanh(signal).astype(np.float32)
    predict._warned_fit_unsupported = False
    with pytest.warns(RuntimeWarning, match="st_fit_knobs_supported"):
        k_dev, h_dev = predict.fit_knobs(signal, target, m, chunk, out, steps=2, route="device")
    with warnings.catch_warnings():
        warnings.simplefilter("error")                        # warns once
        k_dev2, h_dev2 = predict.fit_knobs(signal, target, m, chunk, out, steps=2, route="device")
    k_bat, h_bat = predict.fit_knobs(signal, target, m, chunk, out, steps=2)
    assert np.array_equal(k_dev, k_bat) and h_dev == h_bat and np.array_equal(k_dev2, k_bat) and h_dev2 == h_bat
