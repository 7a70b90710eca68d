"""GPU: the LowPass and Denoise effects on the device -- st_lowpass (the third-order Butterworth low-pass as a scan over the filter's modes,
csrc/st_filter.h) against scipy's float64 lfilter, st_denoise_input, the two effects in the fused feed st_synth_effect (csrc/st_feed.h: the clean
window is ST_FX_COMP4C's bit for bit, per-window reproducibility, the noise's law), and datasets / one training step on their minibatches."""
import ctypes as C
import numpy as np
import pytest
import torch
from scipy.signal import butter, lfilter

pytestmark = pytest.mark.gpu
SR = 44100.0
BOUND = 1e-5           # of max(1e-3, max |ref|): the bound between a device effect and its host reference elsewhere in the suite


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _signals(L, seed=0):
    rng = np.random.default_rng(seed)
    n = np.arange(L)
    box = np.full(L, 0.1, dtype=np.float32); box[L // 5:L // 2] = 0.8; box[L // 2:] = 0.2
    imp = np.zeros(L, dtype=np.float32); imp[0] = 1.0
    return {"white": (2.0 * rng.random(L) - 1.0).astype(np.float32), "box": box,
            "sine30": (0.7 * np.sin(2 * np.pi * 30.0 * n / SR)).astype(np.float32), "impulse": imp}


def _lowpass(x, fc, ysz):
    """st_lowpass on device tensors x [B, L], cutoffs fc [B] (Hz)"""
    from signaltrain_amd import _lib
    x = x.contiguous(); kw = fc.to(torch.float32).reshape(-1, 1).contiguous()
    y = torch.empty(x.shape[0], ysz, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().st_lowpass(_lib.ptr(x), _lib.ptr(kw), SR, x.shape[0], x.shape[1], ysz, _lib.ptr(y), _stream()), "st_lowpass")
    return y


def _ref(x, fc, ysz):
    b, a = butter(3, float(np.float32(fc)) / (SR / 2))
    return lfilter(b, a, x.astype(np.float64))[-ysz:]


def _ratio(y, ref):
    return float(np.abs(y.astype(np.float64) - ref).max() / max(1e-3, np.abs(ref).max()))


@pytest.mark.parametrize("L,ysz", [(2048, 2048), (8192, 2048), (8192, 4100), (2060, 2060), (1000, 4)])
def test_lowpass_matches_lfilter(L, ysz):
    """One chunk and the whole window; the carry across four chunks; an output that starts mid-chunk; a ragged last run and chunk; a window
    shorter than a chunk.  Three rows per launch, each with its own cutoff."""
    sig = _signals(L, seed=L)
    worst = 0.0
    for name, x in sig.items():
        X = torch.from_numpy(np.stack([x, x, x])).cuda()
        for fcs in ((10.0, 10.5, 100.0), (2000.0, 10.0, 10.5)):
            y = _lowpass(X, torch.tensor(fcs, device="cuda"), ysz).cpu().numpy()
            for b, fc in enumerate(fcs):
                r = _ratio(y[b], _ref(x, fc, ysz))
                worst = max(worst, r)
                assert r <= BOUND, (L, ysz, name, fc, r)
    print(f"st_lowpass vs lfilter, L={L} ysz={ysz}: worst ratio {worst:.3g}")


def test_lowpass_bad_cutoffs_give_nan_rows_only():
    L, ysz = 8192, 2048
    x = _signals(L, seed=5)["white"]
    fcs = (100.0, 0.0, 33.0, SR / 2, 2000.0, float("nan"), -4.0, 700.0, SR / 4)        # sr / 4: the real pole at the origin, a valid cutoff
    y = _lowpass(torch.from_numpy(np.stack([x] * len(fcs))).cuda(), torch.tensor(fcs, device="cuda"), ysz).cpu().numpy()
    for b, fc in enumerate(fcs):
        if 0.0 < fc < SR / 2:
            assert _ratio(y[b], _ref(x, fc, ysz)) <= BOUND, fc
        else:
            assert np.isnan(y[b]).all(), fc


def test_lowpass_effect_go_device():
    from signaltrain_amd import audio
    fx = audio.LowPass()
    x = _signals(8192, seed=6)["white"]
    kn = torch.tensor([[-0.5], [0.1], [0.5]], device="cuda")
    X = torch.from_numpy(np.stack([x] * 3)).cuda()
    y = fx.go_device(X, kn, 2048)
    kw = audio._knobs_wc_device(fx.knob_ranges, kn, "cuda")
    assert torch.equal(y, _lowpass(X, kw[:, 0], 2048)) and kw[:, 0].tolist() == [10.0, kw[1, 0].item(), 2000.0]
    for b in range(3):
        ref = audio.lowpass(x, float(kw[b, 0]), SR)[-2048:]
        assert _ratio(y[b].cpu().numpy(), ref.astype(np.float64)) <= BOUND


# ---- the fused feed
def _feed(fx, K, rng, B, augment, first=1000, seed=77, L=8192, ysz=2048, chooser=-1, scratch=False):
    from signaltrain_amd import _lib
    lib = _lib.load()
    x = torch.empty(B, L, device="cuda"); y = torch.empty(B, ysz, device="cuda"); kn = torch.empty(B, K, device="cuda")
    lo = (C.c_float * 4)(*[float(v) for v in rng[:, 0]]); hi = (C.c_float * 4)(*[float(v) for v in rng[:, 1]])
    scr = torch.empty(int(lib.st_synth_effect_scratch_floats(fx, B, L)), device="cuda") if scratch else None
    _lib.check(lib.st_synth_effect(fx, seed, first, B, L, ysz, K, SR, lo, hi, augment, chooser, None, _lib.ptr(x), _lib.ptr(y), _lib.ptr(kn),
                                   _lib.ptr(scr), _stream()), "st_synth_effect")
    return x, y, kn


@pytest.fixture(scope="module", params=[0, 1], ids=["plain", "augment"])
def feeds(request):
    """(clean x of ST_FX_COMP4C, the LOWPASS batch, the DENOISE batch) for windows [1000, 1008) of stream 77"""
    from signaltrain_amd import _lib, audio
    aug = request.param
    c4 = _feed(_lib.FX_COMP4C, 4, audio.Compressor_4c().feed_ranges(), 8, aug)
    lp = _feed(_lib.FX_LOWPASS, 1, audio.LowPass().feed_ranges(), 8, aug)
    dn = _feed(_lib.FX_DENOISE, 1, audio.Denoise().feed_ranges(), 8, aug)
    torch.cuda.synchronize()
    return aug, c4, lp, dn


def test_feed_clean_window_is_comp4c_s(feeds):
    aug, c4, lp, dn = feeds
    assert torch.equal(lp[0], c4[0])
    assert torch.equal(lp[2], c4[2][:, :1]) and torch.equal(dn[2], c4[2][:, :1])         # the first knob draw is the same, too
    for kn in (lp[2], dn[2]):
        assert kn.shape == (8, 1) and float(kn.min()) >= -0.5 and float(kn.max()) <= 0.5
    assert bool(torch.isfinite(lp[1]).all()) and bool(torch.isfinite(dn[0]).all())


def test_feed_is_a_function_of_the_window_index(feeds):
    from signaltrain_amd import _lib, audio
    aug, c4, lp, dn = feeds
    for fx, rng, whole in ((_lib.FX_LOWPASS, audio.LowPass().feed_ranges(), lp), (_lib.FX_DENOISE, audio.Denoise().feed_ranges(), dn)):
        parts = [_feed(fx, 1, rng, 4, aug, first=1000), _feed(fx, 1, rng, 4, aug, first=1004)]
        for i in range(3):
            assert torch.equal(whole[i], torch.cat([p[i] for p in parts])), (fx, i)


def test_feed_lowpass_target(feeds):
    from signaltrain_amd import audio
    aug, c4, (x, y, kn), dn = feeds
    fx = audio.LowPass()
    kw = audio._knobs_wc_device(fx.knob_ranges, kn, "cuda")
    assert torch.equal(y, _lowpass(x, kw[:, 0], 2048))
    assert not torch.equal(y, x[:, -2048:])
    xh, yh, kwh = x.cpu().numpy(), y.cpu().numpy(), kw.cpu().numpy()
    worst = 0.0
    for b in range(8):
        ref = audio.lowpass(xh[b], float(kwh[b, 0]), SR)[-2048:].astype(np.float64)
        r = _ratio(yh[b], ref); worst = max(worst, r)
        assert r <= BOUND, (b, r)
    print(f"feed low-pass vs audio.lowpass: worst ratio {worst:.3g}")


def test_feed_denoise_pair_and_noise_law(feeds):
    from signaltrain_amd import _lib, audio
    aug, (clean, _, _), lp, (x, y, kn) = feeds
    assert torch.equal(y, clean[:, -2048:])                                             # the target is the clean window's tail
    s = audio._knobs_wc_device(audio.Denoise().knob_ranges, kn, "cuda")
    lib = _lib.load()

    def noisy(src):
        out = torch.empty_like(src)
        _lib.check(lib.st_denoise_input(77, 1000, _lib.ptr(src), _lib.ptr(s), 8, 8192, _lib.ptr(out), _stream()), "st_denoise_input")
        return out
    xn = noisy(clean)
    assert torch.equal(x, xn)
    alias = clean.clone()
    _lib.check(lib.st_denoise_input(77, 1000, _lib.ptr(alias), _lib.ptr(s), 8, 8192, _lib.ptr(alias), _stream()), "st_denoise_input")
    assert torch.equal(alias, xn)                                                       # x_noisy may alias x
    noise = noisy(torch.zeros_like(clean))                                              # 0 + n: the noise itself
    assert bool((noise.abs() <= s).all())
    assert bool(((x.double() - clean.double() - noise.double()).abs() <= 2.0 ** -24 * x.abs().double()).all())      # x = fl(clean + noise): one rounding
    d = (x.double() - clean.double()).abs()                                             # one float32 rounding of the sum on top
    assert bool((d <= s.double() + 2.0 ** -24 * (clean.abs().double() + s.double())).all())
    keep = s[:, 0] >= 1e-3
    assert int((~keep).sum()) < 4
    u = (noise[keep].double() / s[keep].double()).cpu().numpy()
    N = u.size
    assert abs(u.mean()) <= 4 / np.sqrt(N)
    assert abs(u.var() - 1 / 3) <= 0.05 / 3
    uc = u - u.mean(axis=1, keepdims=True)
    rho = float((uc[:, 1:] * uc[:, :-1]).sum() / (uc * uc).sum())
    assert abs(rho) < 4 / np.sqrt(N)
    assert not np.array_equal(u[0], u[1])
    print(f"denoise noise: N={N} mean {u.mean():.3g} var {u.var():.4f} lag-1 {rho:.3g}")


def test_feed_lowpass_pink_noise_at_the_long_window():
    """Forced chooser 1 (sine + 1/f + white noise) at L = 16384: the 1/f noise comes from the library's four-step transform through `scratch`."""
    from signaltrain_amd import _lib, audio
    fx = audio.LowPass()
    lib = _lib.load()
    assert lib.st_synth_effect_scratch_floats(_lib.FX_LOWPASS, 4, 16384) > 0
    x, y, kn = _feed(_lib.FX_LOWPASS, 1, fx.feed_ranges(), 4, 1, L=16384, ysz=4096, chooser=1, scratch=True)
    c4 = _feed(_lib.FX_COMP4C, 4, audio.Compressor_4c().feed_ranges(), 4, 1, L=16384, ysz=4096, chooser=1, scratch=True)
    assert torch.equal(x, c4[0]) and bool(torch.isfinite(x).all()) and float(x.abs().amax(1).min()) > 0.05
    kw = audio._knobs_wc_device(fx.knob_ranges, kn, "cuda")
    assert torch.equal(y, _lowpass(x, kw[:, 0], 4096))
    xh, yh = x.cpu().numpy(), y.cpu().numpy()
    for b in range(4):
        assert _ratio(yh[b], _ref(xh[b], float(kw[b, 0]), 4096)) <= BOUND, b


@pytest.mark.parametrize("cls", ["LowPass", "Denoise"])
def test_dataset_batches_and_one_training_step(cls):
    from signaltrain_amd import audio, datasets, nn_proc
    nn_proc._QUIET = True
    np.random.seed(3); torch.manual_seed(3)
    ds = datasets.SynthAudioDataSet(8192, getattr(audio, cls)(), y_size=2048)
    x, y, kn = ds.batch_device(4)
    assert ds._feed_count == 4                                                           # the fused branch
    assert x.is_cuda and x.shape == (4, 8192) and y.shape == (4, 2048) and kn.shape == (4, 1) and x.dtype == y.dtype == kn.dtype == torch.float32
    if cls == "Denoise":
        assert not torch.equal(y, x[:, -2048:])
        # the non-fused branch takes the effect's second return value as the input, too
        g = torch.Generator(device="cuda"); g.manual_seed(1)
        ds2 = datasets.SynthAudioDataSet(8192, audio.Denoise(), y_size=2048, augment=False)
        x2, y2, k2 = ds2.batch_device(4, generator=g)
        s2 = audio._knobs_wc_device(ds2.effect.knob_ranges, k2, "cuda")
        d2 = (x2[:, -2048:] - y2).abs()
        assert ds2._feed_count == 0 and bool((d2 <= s2 * (1 + 1e-6) + 1e-6).all()) and float(d2.max()) > 0
        g.manual_seed(1); np.random.seed(99)                                             # the whole batch, noise included, follows the generator
        x3, y3, k3 = datasets.SynthAudioDataSet(8192, audio.Denoise(), y_size=2048, augment=False).batch_device(4, generator=g)
        assert torch.equal(x3, x2) and torch.equal(y3, y2) and torch.equal(k3, k2)
    model = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=1, sr=44100).to("cuda")
    eng = model.engine(torch.zeros(4, 8192, device="cuda"))
    loss = float(eng.train_step(x, kn, y, 1e-4)[0])
    assert np.isfinite(loss) and loss > 0


@pytest.mark.parametrize("cls", ["LowPass", "Denoise"])
def test_train_on_the_device_feed(tmp_path, monkeypatch, cls):
    """train.train takes the fused feed and the recycled validation set for both effects without special cases."""
    import os
    from signaltrain_amd import audio, datasets, misc, nn_proc, train
    nn_proc._QUIET = True
    made = []
    fused = datasets.SynthAudioDataSet.batch_device

    def counting(self, B, *a, **kw):
        out = fused(self, B, *a, **kw); made.append((B, self._feed_count)); return out
    monkeypatch.setattr(datasets.SynthAudioDataSet, "batch_device", counting)
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0); np.random.seed(0)
    fx = getattr(audio, cls)()
    train.train(effect=fx, epochs=1, n_data_points=512, batch_size=128, device=torch.device("cuda:0"), device_feed=True, lr_max=2e-4)
    assert made and all(c > 0 for _, c in made) and sum(B for B, _ in made) == 512 + 128      # every window came out of the fused feed
    lines = [l.split() for l in open("vl_avg_out.dat").read().strip().splitlines()]
    assert len(lines) == 1 and np.isfinite(float(lines[0][-1]))
    sd, rv = misc.load_checkpoint("modelcheckpoint.tar", device="cpu")
    assert rv["effect_name"] == fx.name and list(rv["knob_names"]) == fx.knob_names and np.array_equal(rv["knob_ranges"], fx.knob_ranges)
    assert all(torch.isfinite(v).all() for v in sd.values())
