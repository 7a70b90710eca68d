"""GPU: whole-signal inference in one device call -- st_predict_long / StepEngine.predict_long / predict.predict_long(route="device").

The recording stays in HBM; the library reads the overlapping windows out of it, runs the validation forward batch by batch and writes the prediction to its
place.  Checked against the float64 oracle run window by window on the host (audio.sliding_window), against st_eval_step on the same windows materialised,
across batch sizes, sample formats and knob layouts, and for everything it must leave alone."""
import contextlib
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from oracle import host_audio
from oracle import st_oracle as O
from signaltrain_amd import _lib
from tests import gpu_checks as G
from tests.dims_table import geo_of, seeds_of

pytestmark = pytest.mark.gpu

K = 4
LEVELS = {
    "f32": contextlib.nullcontext, "f32x3": G.split_mode,
    "bf16": lambda: G.mixed_mode(1, half="bf16"), "bf16_all": lambda: G.mixed_mode(2, half="bf16"),
    "f16": lambda: G.mixed_mode(1, half="f16"), "f16_all": lambda: G.mixed_mode(2, half="f16"),
}
_CASES = {}


def case(row):
    """(geo, P) of a dims-table row (None: the default geometry), seeded as the fused sweep seeds it; made once, never modified."""
    if row not in _CASES:
        geo, _, _, _, P = G.make_case(1, seeds_of(row)[1], K=K, geo=None if row is None else geo_of(row))
        _CASES[row] = (geo, P)
    return _CASES[row]


def signal(n, seed=3):
    rng = np.random.default_rng(seed)
    return (0.4 * np.sin(np.arange(n) * 0.013) + 0.05 * rng.standard_normal(n)).astype(np.float32)


def length(geo, hops=7):
    """Not a whole number of hops: hops + 2 windows, i.e. three batches of four with a last batch of one at hops = 7."""
    return geo["L"] + hops * geo["y"] + 777 % geo["y"]


def lengths(L, y):
    return [1, L - y, L - y + 1, L - 1, L, L + 1, L + y - 1, L + y, L + 3 * y + 777 % y]


def windows(sig, geo):
    """The windows the reference forms on the host: audio.sliding_window with overlap L - y; below one window, the one zero-padded window."""
    L, y = geo["L"], geo["y"]
    if sig.size < L:
        return np.pad(sig, (0, L - sig.size))[None, :]
    return np.ascontiguousarray(host_audio.sliding_window(sig, L, overlap=L - y))


def oracle(sig, kn_rows, P, geo):
    """float64 oracle window by window; kn_rows [K] or [nwin, K]."""
    f = np.float64
    xw = windows(sig, geo).astype(f)
    kn = np.asarray(kn_rows, f)
    kn = np.tile(kn, (xw.shape[0], 1)) if kn.ndim == 1 else kn
    out = O.model_fwd(xw, kn, {k: v.astype(f) for k, v in P.items()}, geo)[0].reshape(-1)
    return out[:max(sig.size - (geo["L"] - geo["y"]), 0)]


def engine(row, B):
    geo, P = case(row)
    eng = G.new_engine(G.dims_of(geo, B, K)); eng.load_state_dict(P)
    return eng, geo, P


KN = np.array([0.1, -0.3, 0.25, -0.45], np.float32)


@pytest.mark.parametrize("row", ["n256", "h256", "ragged", "tiny", None])
def test_fp32_against_the_float64_oracle(row):
    """fp32, every overlap-add form (h256: four overlapping frames), an all-padding last frame (ragged), L < N (tiny) and the default geometry: within
    gpu_checks.TOL = 1e-4 of max|ref| of the oracle run window by window -- the bar of test_predict_long_matches_windowed_oracle.  Nine windows in batches
    of four: the last batch is a single window whose tail lies behind the end of the signal."""
    eng, geo, P = engine(row, 4)
    n = length(geo)
    sig = signal(n)
    y = eng.predict_long(G.t(sig), G.t(KN))
    ref = oracle(sig, KN, P, geo)
    assert y.dtype == torch.float32 and y.is_cuda and tuple(y.shape) == (n - (geo["L"] - geo["y"]),) == ref.shape
    e = float(np.abs(G.n(y) - ref).max() / np.abs(ref).max())
    print(f"predict_long vs float64 oracle [{row or 'default'}]: n={n} rel={e:.2e}")
    assert e <= G.TOL, (row, e)


def test_ragged_lengths():
    """Every length around the window and hop boundaries at n256: the length is the reference's, the values the oracle's, and a signal no longer than the
    first window's lookback gives an empty result."""
    eng, geo, P = engine("n256", 3)
    L, y = geo["L"], geo["y"]
    full = signal(L + 4 * y)
    for n in lengths(L, y):
        sig = full[:n].copy()
        got = eng.predict_long(G.t(sig), G.t(KN))
        assert tuple(got.shape) == (max(n - (L - y), 0),), n
        if n <= L - y:
            assert got.numel() == 0
            continue
        ref = oracle(sig, KN, P, geo)
        e = float(np.abs(G.n(got) - ref).max() / np.abs(ref).max())
        print(f"predict_long ragged length n={n}: {got.numel()} samples rel={e:.2e}")
        assert e <= G.TOL, (n, e)


@pytest.mark.parametrize("row", ["n384", None])
@pytest.mark.parametrize("level", list(LEVELS))
def test_same_forward_as_validation(level, row):
    """Every arithmetic level: the device route against eval_step(want_y_hat=True) on the same windows materialised on the host, batch for batch (3, 3, 1
    windows) -- the same GEMM, autoencoder and summation order, asserted to 1e-6 of max|ref| (the bound test_eval_step_is_the_training_forward holds for "same
    kernels").  Whether the two were bit-equal is printed."""
    with LEVELS[level]():
        B = 3
        eng, geo, P = engine(row, B)
        n = length(geo, hops=5)
        sig = signal(n, seed=5)
        got = eng.predict_long(G.t(sig), G.t(KN), batch=B)
        xw = windows(sig, geo)
        assert xw.shape[0] == 7
        ref = []
        for b0 in range(0, xw.shape[0], B):
            xb = xw[b0:b0 + B]
            y_hat = eng.eval_step(G.t(xb), G.t(np.tile(KN, (xb.shape[0], 1))), G.t(np.zeros((xb.shape[0], geo["y"]), np.float32)), want_y_hat=True)
            ref.append(y_hat.reshape(-1))
        ref = torch.cat(ref)[:got.numel()]
        bits = bool(torch.equal(got, ref))
        r = G.n(ref)
        e = float(np.abs(G.n(got) - r).max() / np.abs(r).max())
        print(f"predict_long vs eval_step [{level} {row or 'default'}]: bit-equal={bits} rel={e:.2e}")
        assert e <= 1e-6, (level, row, e)


@pytest.mark.parametrize("level", ["f32", "bf16_all"])
def test_batch_independence(level):
    """2, 5 or all windows per batch: the same prediction to 1e-6 of max|y| (test_full_size_batch_properties' forward bound)."""
    with LEVELS[level]():
        eng, geo, P = engine("n256", 16)
        sig = G.t(signal(length(geo), seed=6))
        ys = {b: G.n(eng.predict_long(sig, G.t(KN), batch=b)) for b in (2, 5, 16)}
        sc = np.abs(ys[16]).max()
        for b in (2, 5):
            e = float(np.abs(ys[b] - ys[16]).max() / sc)
            print(f"predict_long batch {b} vs one batch [{level}]: rel={e:.2e}")
            assert e <= 1e-6, (level, b, e)


@pytest.mark.parametrize("level", ["f32", "bf16_all"])
def test_int16_signal_equals_its_float_image(level):
    """ST_PCM_S16: the int16 recording gives, bit for bit, what the float32 route gives on (float)((double)s / 32767.0)."""
    with LEVELS[level]():
        eng, geo, P = engine("n256", 4)
        n = length(geo)
        s16 = np.clip(np.round(signal(n, seed=7) * 32767.0 * 2.5), -32768, 32767).astype(np.int16)      # peaks of 1.1: clipped at both ends
        assert s16.min() == -32768 and s16.max() == 32767                       # both ends of the format occur
        img = (s16.astype(np.float64) / 32767.0).astype(np.float32)
        a = eng.predict_long(torch.from_numpy(s16).to(G.DEV), G.t(KN))
        b = eng.predict_long(G.t(img), G.t(KN))
        assert a.dtype == torch.float32 and a.shape == b.shape and torch.equal(a, b)
        assert float(b.abs().max()) > 0.1


def test_int16_view_at_8_mod_16_is_read_in_place():
    """An int16 recording that starts four samples (8 bytes) behind a 16-byte boundary is taken as it is -- the library reads int16 recordings as aligned
    quads of four samples (pcm_align in st_api.hip) -- and gives the bits of an aligned clone of the same samples: predict_long, and encode_long + decode_long."""
    eng, geo, P = engine("tiny", 3)
    L, y = geo["L"], geo["y"]
    n = L + 3 * y + 777 % y
    assert int(eng.lib.st_predict_windows(C.byref(eng.dims), n)) == 5
    buf = torch.zeros(n + 8, dtype=torch.int16, device=G.DEV)
    view = buf[4:4 + n]
    view.copy_(torch.from_numpy(np.round(signal(n, seed=11) * 30000).astype(np.int16)).to(G.DEV))
    clone = view.clone()
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 and clone.data_ptr() % 16 == 0
    kn = G.t(KN)
    want = eng.predict_long(clone, kn)
    assert want.numel() == n - (L - y) and float(want.abs().max()) > 0
    assert torch.equal(eng.predict_long(view, kn), want)
    code = eng.encode_long(view)
    assert code.signal.data_ptr() == view.data_ptr()              # not copied
    assert torch.equal(eng.decode_long(code, kn), eng.decode_long(eng.encode_long(clone), kn))


def test_knob_automation():
    """One knob row per window (two settings alternating) against the oracle with the same per-window knobs at 1e-4; one row equals that row repeated
    over the windows bit for bit."""
    eng, geo, P = engine("n256", 4)
    n = length(geo)
    sig = signal(n, seed=8)
    nwin = int(eng.lib.st_predict_windows(C.byref(eng.dims), n))
    assert nwin == 9
    rows = np.stack([KN if w % 2 == 0 else -KN[::-1] for w in range(nwin)]).astype(np.float32)
    got = eng.predict_long(G.t(sig), G.t(rows))
    ref = oracle(sig, rows, P, geo)
    e = float(np.abs(G.n(got) - ref).max() / np.abs(ref).max())
    one = oracle(sig, KN, P, geo)
    print(f"predict_long knob automation: rel={e:.2e} (against the one-setting oracle: {float(np.abs(G.n(got) - one).max() / np.abs(one).max()):.2e})")
    assert e <= G.TOL
    assert np.abs(ref - one).max() > 100 * G.TOL * np.abs(one).max()            # the second setting is audible: the rows were really taken per window
    a = eng.predict_long(G.t(sig), G.t(KN))
    for shape in ((1, K), (nwin, K)):
        b = eng.predict_long(G.t(sig), G.t(np.broadcast_to(KN, shape).copy()))
        assert torch.equal(a, b), shape
    with pytest.raises(ValueError, match="rows"):
        eng.predict_long(G.t(sig), G.t(rows[:nwin - 1]))


def test_guards():
    """Nothing outside out[0, n_out) is written (n_out is not a multiple of four: the last quad is clipped), nothing at or past signal + n is read (NaN
    there), and parameters, moments and gradients are bit-unchanged while generation moves by one."""
    eng, geo, P = engine("n256", 4)
    n = length(geo)
    n_out = n - (geo["L"] - geo["y"])
    assert n_out % 4 != 0 and n % 4 != 0
    sig = signal(n, seed=9)
    for name in ("grads", "m", "v"):
        getattr(eng, name).copy_(torch.randn_like(eng.params))
    before = {k: getattr(eng, k).clone() for k in ("params", "grads", "m", "v", "scalars")}
    gen = eng.generation
    plain = eng.predict_long(G.t(sig), G.t(KN))
    assert eng.generation == gen + 1
    PAD, POISON = 64, 12345.0
    buf = torch.full((PAD + n_out + PAD,), POISON, dtype=torch.float32, device=G.DEV)
    got = eng.predict_long(G.t(sig), G.t(KN), out=buf[PAD:PAD + n_out + 8])
    assert got.data_ptr() == buf[PAD:].data_ptr() and got.numel() == n_out and torch.equal(got, plain)
    assert bool((buf[:PAD] == POISON).all()) and bool((buf[PAD + n_out:] == POISON).all())
    for dtype, host in ((torch.float32, sig), (torch.int16, np.round(sig * 20000).astype(np.int16))):
        clean = eng.predict_long(torch.from_numpy(host).to(G.DEV), G.t(KN))
        if dtype == torch.float32:
            sbuf = torch.full((PAD + n + PAD,), float("nan"), dtype=dtype, device=G.DEV)
        else:
            sbuf = torch.full((PAD + n + PAD,), 32767, dtype=dtype, device=G.DEV)      # int16 has no NaN: full scale where zeros are due
        sbuf[PAD:PAD + n] = torch.from_numpy(host).to(G.DEV)
        emb = eng.predict_long(sbuf[PAD:PAD + n], G.t(KN))
        assert bool(torch.isfinite(emb).all()) and torch.equal(emb, clean), dtype
    for k, v in before.items():
        assert torch.equal(getattr(eng, k), v), k


def test_training_trajectory_is_untouched():
    """A train step before and one after a prediction: the trajectory of the two train steps alone, bit for bit."""
    geo, P = case("n256")
    _, X, Y, KNB, _ = G.make_case(3, 21, K=K, geo=geo_of("n256"))
    a = G.new_engine(G.dims_of(geo, 3, K)); a.load_state_dict(P)
    b = G.new_engine(G.dims_of(geo, 3, K)); b.load_state_dict(P)
    sig = G.t(signal(length(geo), seed=10))
    for i in range(2):
        a.train_step(G.t(X), G.t(KNB), G.t(Y), 1e-3)
        b.train_step(G.t(X), G.t(KNB), G.t(Y), 1e-3)
        if i == 0:
            a.predict_long(sig, G.t(KN))
    for k in ("params", "m", "v", "grads", "scalars"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.step_count == b.step_count == 2


def _model(scale=1):
    from signaltrain_amd import nn_proc
    nn_proc._QUIET = True
    geo = O.geometry(scale, 4)
    P = G.make_case(1, 1, K=K, scale=scale)[4]
    m = nn_proc.st_model(scale_factor=scale, shrink_factor=4, num_knobs=K)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    return m.to(G.DEV), P, geo


def test_python_route():
    """predict.predict_long(route="device") against route="batched" in fp32: each is within 1e-4 of the oracle, so they agree within 2e-4 of max|ref|; same
    shape and dtype; a device tensor as the signal and one knob row per window are taken."""
    from signaltrain_amd.predict import predict_long
    m, P, geo = _model()
    L, y = geo["L"], geo["y"]
    n = L + 4 * y + 777
    sig = signal(n, seed=11)
    batched = predict_long(sig, KN, m, L, y, batch_size=3)
    device = predict_long(sig, KN, m, L, y, batch_size=3, route="device")
    ref = oracle(sig, KN, P, geo)
    assert isinstance(device, np.ndarray) and device.dtype == batched.dtype == np.float32 and device.shape == batched.shape == (n - (L - y),)
    sc = np.abs(ref).max()
    print(f"predict_long routes: device-batched={np.abs(device - batched).max() / sc:.2e} device-oracle={np.abs(device - ref).max() / sc:.2e} "
          f"batched-oracle={np.abs(batched - ref).max() / sc:.2e}")
    assert np.abs(device - batched).max() <= 2e-4 * sc and np.abs(device - ref).max() <= 1e-4 * sc
    resident = predict_long(torch.from_numpy(sig).to(G.DEV), KN, m, L, y, batch_size=3, route="device")
    assert isinstance(resident, np.ndarray) and np.array_equal(resident, device)
    nwin = 6
    rows = np.stack([KN if w % 2 == 0 else -KN[::-1] for w in range(nwin)]).astype(np.float32)
    auto = predict_long(sig, rows, m, L, y, batch_size=4, route="device")
    ref2 = oracle(sig, rows, P, geo)
    assert auto.shape == device.shape and np.abs(auto - ref2).max() <= 1e-4 * np.abs(ref2).max()
    comp = predict_long(sig, KN, m, L, y, batch_size=3, route="device", compand=True)
    comp_b = predict_long(sig, KN, m, L, y, batch_size=3, compand=True)
    assert comp.shape == comp_b.shape and np.abs(comp - comp_b).max() <= 2e-4 * np.abs(comp_b).max()


def test_unsupported_geometry_falls_back_with_one_warning():
    """The 65536-sample window runs the wide autoencoder path, which st_predict_long does not take: route="device" warns once and returns what the batched
    route returns."""
    from signaltrain_amd import predict
    m, P, geo = _model(scale=8)
    L, y = geo["L"], geo["y"]
    d = _lib.geometry(8, 4, K, 1)
    if _lib.load().st_predict_supported(C.byref(d)):
        pytest.skip("every geometry is supported: there is no fallback to exercise")
    sig = signal(L + y + 5, seed=12)
    predict._warned_unsupported = False
    with pytest.warns(RuntimeWarning, match="batched route"):
        a = predict.predict_long(sig, KN, m, L, y, batch_size=2, route="device")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b = predict.predict_long(sig, KN, m, L, y, batch_size=2, route="device")          # the second time: no warning
    c = predict.predict_long(sig, KN, m, L, y, batch_size=2)
    assert np.array_equal(a, c) and np.array_equal(b, c)
