"""GPU: the compressor family on the device -- st_compressor (the envelope compressor of audio.py:349-371 as a parallel scan, csrc/st_misc.h)
against golden G15 and the host restatement, and the fused feed st_synth_effect (csrc/st_feed.h) for the comp / comp_t / comp_one effects:
targets, knob shapes, per-window reproducibility, the two forms of the effect, the fixed settings of comp_t, and a short training run of each
new knob count."""
import ctypes as C
import os
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SR = 44100.0


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _compressor(x, kw, ysz):
    """st_compressor on device tensors x [B, L], world knobs kw [B, 3]"""
    from signaltrain_amd import _lib
    x = x.contiguous(); kw = kw.to(torch.float32).contiguous()
    y = torch.empty(x.shape[0], ysz, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().st_compressor(_lib.ptr(x), _lib.ptr(kw), SR, x.shape[0], x.shape[1], ysz, _lib.ptr(y), _stream()), "st_compressor")
    return y


def test_device_compressor_matches_reference_golden(golden_dir):
    from signaltrain_amd import audio
    g = np.load(os.path.join(golden_dir, "g15_compressor_family.npz"))
    x = torch.from_numpy(g["comp_x"]).cuda()
    ref = g["comp_y"]
    for y in (audio.Compressor().go_device(x, torch.from_numpy(g["comp_kn"]).float().cuda()), _compressor(x, torch.from_numpy(g["comp_kw"]).cuda(), 8192)):
        y = y.cpu().numpy().astype(np.float64)
        for i in range(len(ref)):
            assert np.abs(y[i] - ref[i]).max() <= 2e-6 * max(1.0, np.abs(ref[i]).max()), i    # float32 knobs (1 ms is not a float32 value), float32 y
        assert np.abs(y[4, :2048]).max() == 0.0
    for pre, fx in (("thresh", audio.Comp_Just_Thresh()), ("one", audio.Compressor_4c_OneSetting())):
        y = fx.go_device(x[torch.from_numpy(g[pre + "_idx"]).cuda()], torch.from_numpy(g[pre + "_kn"]).cuda()).cpu().numpy()
        assert np.abs(y - g[pre + "_y"]).max() <= 2e-6 * max(1.0, np.abs(g[pre + "_y"]).max()), pre


@pytest.mark.parametrize("L,ysz", [(8192, 2048), (20000, 20000), (65536, 16256)])
def test_device_compressor_matches_host_restatement(L, ysz):
    """Random batches (as test_device_compressor_matches_reference_golden of the comp_4c effect): several levels, a silent stretch, Beta knobs;
    L = 20000 is not a whole number of the scan's chunks."""
    from signaltrain_amd import audio
    rng = np.random.default_rng(L)
    B = 5
    X = (rng.standard_normal((B, L)) * np.linspace(0.02, 0.9, B)[:, None]).astype(np.float32)
    X[1, 100:900] = 0.0
    X[3, :1500] = 0.0                                   # starts in digital silence
    KN = (rng.beta(0.8, 0.8, size=(B, 3)) - 0.5).astype(np.float32)
    fx = audio.Compressor()
    kw = audio._knobs_wc_device(fx.knob_ranges, torch.from_numpy(KN).cuda(), "cuda")
    yd = _compressor(torch.from_numpy(X).cuda(), kw, ysz).cpu().numpy()
    kwh = kw.cpu().numpy().astype(np.float64)            # the same float32 world knobs on the host
    for b in range(B):
        ref = audio.compressor(X[b], *kwh[b], sr=SR)[-ysz:]
        assert np.abs(yd[b] - ref).max() <= 1e-6 * max(1e-3, np.abs(ref).max()), (L, b)
    assert np.array_equal(yd, fx.go_device(torch.from_numpy(X).cuda(), torch.from_numpy(KN).cuda(), ysz).cpu().numpy())


def test_device_compressor_threshold_above_envelope_and_ratio_one():
    rng = np.random.default_rng(9)
    X = torch.from_numpy((0.5 * rng.standard_normal((3, 20000))).astype(np.float32)).clamp(-0.9, 0.9).cuda()
    X[1, :5000] = 0.0
    hi = torch.tensor([[0.0, 4.0, 1e-3], [0.0, 2.0, 4e-2], [-0.5, 5.0, 0.01]], device="cuda")       # |x| < 0.9: the envelope stays below -0.9 dB
    y = _compressor(X, hi, 20000)
    assert torch.equal(y, X)                                                                          # gain exactly 1, bit for bit
    one = torch.tensor([[-40.0, 1.0, 1e-3], [-60.0, 1.0, 4e-2], [-20.0, 1.0, 0.01]], device="cuda")
    y1 = _compressor(X, one, 20000)
    assert float((y1 - X).abs().max()) <= 1e-6 * float(X.abs().max())


FEED = [("comp", "Compressor", 3), ("comp_t", "Comp_Just_Thresh", 1), ("comp_one", "Compressor_4c_OneSetting", 4)]


def _ds(cls, L=8192, ysz=2048, seed=11, augment=True):
    from signaltrain_amd import audio, datasets
    np.random.seed(seed)
    return datasets.SynthAudioDataSet(L, getattr(audio, cls)(), y_size=ysz, augment=augment)


@pytest.mark.parametrize("key,cls,K", FEED)
def test_feed_targets_knobs_and_batching(key, cls, K):
    ds = _ds(cls)
    x, y, kn = ds.batch_device(96)
    assert x.shape == (96, 8192) and y.shape == (96, 2048) and kn.shape == (96, K) and x.dtype == y.dtype == kn.dtype == torch.float32
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all())
    assert float(kn.min()) >= -0.5 and float(kn.max()) <= 0.5 and float(kn.std()) > 0.2
    y2 = ds.effect.go_device(x, kn, 2048)                            # the unfused path on the same windows and knobs
    assert float((y - y2).abs().max()) <= 1e-6 * float(y2.abs().max()), key
    assert float(x.abs().amax(1).min()) > 0.05
    assert not torch.equal(y, x[:, -2048:])                          # the effect did something
    # a function of (seed, window index) only
    a, b = _ds(cls, seed=5), _ds(cls, seed=5)
    xa, ya, ka = a.batch_device(8)
    parts = [b.batch_device(3), b.batch_device(5)]
    for i, t in enumerate((xa, ya, ka)):
        assert torch.equal(t, torch.cat([p[i] for p in parts])), (key, i)


def _feed_direct(fx, K, B, L, ysz, scratch, seed=77, first=1000):
    from signaltrain_amd import _lib
    lib = _lib.load()
    x = torch.empty(B, L, device="cuda"); y = torch.empty(B, ysz, device="cuda"); kn = torch.empty(B, K, device="cuda")
    rng = fx.feed_ranges()
    lo = (C.c_float * 4)(*[float(v) for v in rng[:, 0]]); hi = (C.c_float * 4)(*[float(v) for v in rng[:, 1]])
    scr = torch.empty(int(lib.st_synth_effect_scratch_floats(fx.feed_fx, B, L)), device="cuda") if scratch else None
    _lib.check(lib.st_synth_effect(fx.feed_fx, seed, first, B, L, ysz, K, SR, lo, hi, 1, -1, None, _lib.ptr(x), _lib.ptr(y), _lib.ptr(kn),
                                   _lib.ptr(scr), _stream()), "st_synth_effect")
    return x, y, kn


@pytest.mark.parametrize("key,cls,K", FEED)
def test_feed_split_and_in_kernel_forms_agree(key, cls, K):
    from signaltrain_amd import audio
    fx = getattr(audio, cls)()
    s = _feed_direct(fx, K, 64, 8192, 2048, scratch=True)
    k = _feed_direct(fx, K, 64, 8192, 2048, scratch=False)
    for i in range(3):
        assert torch.equal(s[i], k[i]), (key, i)


def test_feed_comp_t_settings_are_fixed():
    """comp_t = the 4-control compressor with only the threshold drawn: its target is st_compressor_4c at (threshold, 3, 0.05 s, 1 s)."""
    from signaltrain_amd import audio, _lib
    fx = audio.Comp_Just_Thresh()
    x, y, kn = _feed_direct(fx, 1, 64, 8192, 2048, scratch=True)
    thr = -50.0 + (kn + 0.5) * 40.0
    kw = torch.cat([thr, torch.tensor([[3.0, 0.05, 1.0]], device="cuda").expand(64, 3)], 1).contiguous()
    y4 = torch.empty_like(y)
    _lib.check(_lib.load().st_compressor_4c(_lib.ptr(x), _lib.ptr(kw), SR, 64, 8192, 2048, _lib.ptr(y4), _stream()), "st_compressor_4c")
    assert float((y - y4).abs().max()) <= 1e-6 * float(y4.abs().max())
    kw[:, 1] = 5.0                                                     # another ratio gives another target
    _lib.check(_lib.load().st_compressor_4c(_lib.ptr(x), _lib.ptr(kw), SR, 64, 8192, 2048, _lib.ptr(y4), _stream()), "st_compressor_4c")
    assert float((y - y4).abs().max()) > 1e-3 * float(y4.abs().max())


def test_feed_comp_at_the_long_window():
    """The envelope compressor's feed at the 65536-sample window (the library's own 1/f-noise transform through the scratch, split form)."""
    ds = _ds("Compressor", L=65536, ysz=16256, seed=3)
    x, y, kn = ds.batch_device(8)
    assert getattr(ds, "_dev_gen", None) is None and kn.shape == (8, 3)
    y2 = ds.effect.go_device(x, kn, 16256)
    assert float((y - y2).abs().max()) <= 1e-6 * float(y2.abs().max())


@pytest.mark.parametrize("cls,K", [("Compressor", 3), ("Comp_Just_Thresh", 1)])
def test_train_with_the_new_effects(tmp_path, cls, K):
    from signaltrain_amd import audio, misc, nn_proc, train
    nn_proc._QUIET = True
    cwd = os.getcwd(); os.chdir(tmp_path)
    try:
        torch.manual_seed(0); np.random.seed(0)
        fx = getattr(audio, cls)()
        train.train(effect=fx, epochs=2, n_data_points=2048, batch_size=256, device=torch.device("cuda:0"), device_feed=True, lr_max=2e-4)
        lines = [l.split() for l in open("vl_avg_out.dat").read().strip().splitlines()]
        assert len(lines) == 2 and all(np.isfinite(float(l[-1])) for l in lines)
        sd, rv = misc.load_checkpoint("modelcheckpoint.tar", device="cpu")
        assert rv["effect_name"] == fx.name and list(rv["knob_names"]) == fx.knob_names
        assert np.asarray(rv["knob_ranges"]).shape == (K, 2) and np.array_equal(rv["knob_ranges"], fx.knob_ranges)
        assert all(torch.isfinite(v).all() for v in sd.values())
        m = nn_proc.st_model(scale_factor=rv["scale_factor"], shrink_factor=rv["shrink_factor"], num_knobs=K, sr=rv["sr"])
        m.load_state_dict(sd)
    finally:
        os.chdir(cwd)
