"""CPU: the twelve signal families of audio.synth_input_sample on the host side of the feed -- the float64 restatement of the families beyond the
compressor's set against golden G17 (the reference itself), the batched generators of audio_device.py against the restatements
(distributional: another generator than numpy's), the host replica of the feed's second draw sequence (datasets.synth_feed_draw), the refusals
of st_synth_effect_families (no launch: runs without a GPU) and the `choosers` plumbing of the datasets."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import host_audio as H
from signaltrain_amd import audio, audio_device as AD, datasets
from tests import signal_families_ref as R

SR = 44100.0
L = 1024
N_HOST, N_OTHER = 160, 640          # windows per family: the host sample the margin comes from, and the (larger) sample compared with it
T64 = R.time_values(L, SR)
T32 = T64.astype(np.float32)


def test_restatement_reproduces_the_reference():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "g17_signal_families.npz"))
    assert g["y"].dtype == np.float32 and list(g["families"]) == list(R.FAMILIES)
    t = g["t_f32"].astype(np.float64)
    assert np.array_equal(t, R.time_values(len(t), float(g["sr"])))
    for i, s in enumerate(g["seeds"]):
        for j, c in enumerate(g["families"]):
            y, _ = R.synth_input_sample(t, int(c), np.random.RandomState(int(s)))
            ref = g["y"][i, j].astype(np.float64)
            # G17 is the reference's float64 output rounded once to float32 for storage: half a float32 ulp, and float64 round-off on top
            assert np.all(np.abs(y - ref) <= 2.0 ** -24 * np.abs(ref) + 1e-13), (int(s), int(c), np.abs(y - ref).max())


def test_env_db_is_the_integer_formula():
    for n in (64, 256, 1000, 4096, 8192, 16384, 65536):
        k = np.arange(n)
        assert np.array_equal(-30 + (30 * k) // (n - 1), R.env_dB(n)), n


# ---------------------------------------------------------------------------------------------- the batched generators, by family
def _host_sample(c, n, seed):
    if c in R.FAMILIES:
        rng = np.random.RandomState(seed)
        return np.stack([R.synth_input_sample(T64, c, rng)[0] for _ in range(n)])
    np.random.seed(seed)
    return np.stack([H.synth_input_sample(T32, c) for _ in range(n)])


def _stats(x):
    """per-window peak and mean |x| -> the three statistics compared"""
    x = np.asarray(x, dtype=np.float64)
    return np.abs(x).max(1), np.abs(x).mean(1)


def _three(peak, mabs):
    return np.array([np.quantile(peak, 0.05), np.quantile(peak, 0.95), mabs.mean()])


def _margin(peak, mabs, seed=0, rounds=200):
    """five bootstrap standard errors of each statistic over the sample"""
    rng = np.random.default_rng(seed)
    n = len(peak)
    boot = np.stack([_three(peak[i], mabs[i]) for i in (rng.integers(0, n, n) for _ in range(rounds))])
    return 5.0 * boot.std(0)


@pytest.fixture(scope="module")
def host_samples():
    return {c: _stats(_host_sample(c, N_HOST, 100 + c)) for c in range(12)}


@pytest.mark.parametrize("c", range(12))
def test_margin_holds_between_two_host_samples(host_samples, c):
    """The margin is only worth relying on if an independent host sample of the other sample's size passes it"""
    ref, other = host_samples[c], _stats(_host_sample(c, N_OTHER, 900 + c))
    d, m = np.abs(_three(*other) - _three(*ref)), _margin(*ref)
    print(f"family {c}: host vs host  |difference| {d}  margin {m}")
    assert np.all(d <= m), (c, d, m)


@pytest.mark.parametrize("c", range(12))
def test_batched_generators_make_every_family(host_samples, c):
    g = torch.Generator(device="cpu"); g.manual_seed(40 + c)
    x, pick = AD.synth_input_batch(N_OTHER, L, SR, g, "cpu", chooser=c)
    assert x.shape == (N_OTHER, L) and x.dtype == torch.float32 and bool((pick == c).all()) and bool(torch.isfinite(x).all())
    ref = host_samples[c]
    d, m = np.abs(_three(*_stats(x.numpy())) - _three(*ref)), _margin(*ref)
    print(f"family {c}: batched vs host  |difference| {d}  margin {m}")
    assert np.all(d <= m), (c, d, m)


def test_default_set_keeps_its_draw_sequence():
    """The families beyond the compressor's set draw nothing unless one of them can come out"""
    def run(**kw):
        g = torch.Generator(device="cpu"); g.manual_seed(9)
        x, pick = AD.synth_input_batch(16, L, SR, g, "cpu", **kw)
        return x, pick, torch.rand(4, generator=g)
    a, b = run(), run(choosers=AD.COMPRESSOR_CHOOSERS)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    wide = run(choosers=tuple(range(12)))
    assert not torch.equal(wide[2], a[2])
    with pytest.raises(NotImplementedError, match="superposition"):
        run(chooser=12)


def test_custom_set_is_drawn_uniformly():
    g = torch.Generator(device="cpu"); g.manual_seed(21)
    fams, n = (1, 3, 5, 6, 7), 5000
    _, pick = AD.synth_input_batch(n, 64, SR, g, "cpu", choosers=fams)
    cnt = np.array([int((pick == f).sum()) for f in fams])
    assert cnt.sum() == n and np.all(np.abs(cnt - n / 5) <= 5 * np.sqrt(n * 0.2 * 0.8)), cnt


# ---------------------------------------------------------------------------------------------- the host replica of the second draw sequence
def test_synth_feed_draw_is_a_function_of_seed_and_window():
    w = np.array([0, 1, 2, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 17], dtype=np.uint64)
    fams = (0, 1, 3, 4, 6, 10, 2, 7, 9)
    whole = datasets.synth_feed_draw(7, w, 8192, SR, choosers=fams)
    for i, wi in enumerate(w):
        one = datasets.synth_feed_draw(7, int(wi), 8192, SR, choosers=fams)
        again = datasets.synth_feed_draw(7, int(wi), 8192, SR, choosers=sorted(fams))
        for k, v in whole.items():
            assert np.array_equal(v[i], one[k]) and np.array_equal(one[k], again[k]), (k, int(wi))
    other = datasets.synth_feed_draw(8, w, 8192, SR, choosers=fams)
    assert not np.array_equal(other["step_freq"], whole["step_freq"]) and len(set(whole["step_freq"].tolist())) == len(w)
    # the set moves the family only; the window length moves what is measured in samples or seconds
    full = datasets.synth_feed_draw(7, w, 8192, SR, choosers=range(12))
    assert all(np.array_equal(full[k], whole[k]) for k in whole if k != "family")
    short = datasets.synth_feed_draw(7, w, 256, SR, choosers=fams)
    for k in ("family", "tri_height", "tri_amp", "spike_amp", "spike_height", "step_freq", "sweep_f_low", "sweep_f_high", "sweep_amp_too", "sweep_amp",
              "white10", "pink10", "pink11"):
        assert np.array_equal(short[k], whole[k]), k
    assert np.all(short["spike_loc"] < 256) and np.all(short["spike_loc"] >= 0)
    assert np.all(datasets.synth_feed_draw(7, w, 8192, SR)["family"] == -1)        # the compressor's set: the first sequence's choice


def test_synth_feed_draw_laws():
    n = 20000
    fams = (1, 3, 5, 6, 7)
    d = datasets.synth_feed_draw(3, np.arange(n), 8192, SR, choosers=fams)
    cnt = np.array([int((d["family"] == f).sum()) for f in fams])
    assert cnt.sum() == n and np.all(np.abs(cnt - n / 5) <= 5 * np.sqrt(n * 0.2 * 0.8)), cnt
    tl = float(d["tl"][0])
    assert tl == float(np.float32(8191) / np.float32(SR))
    assert 0.4 <= np.abs(d["tri_height"]).min() and np.abs(d["tri_height"]).max() <= 0.8 and 0.45 < (d["tri_height"] > 0).mean() < 0.55
    assert d["tri_width"].max() <= tl / 4 and np.all(d["tri_t0"] >= 2 * d["tri_width"]) and d["tri_t0"].max() <= 0.9 * tl * (1 + 1e-6)
    assert 0.02 <= d["tri_amp"].min() and d["tri_amp"].max() <= 0.12 and d["spike_amp"].max() <= 0.1
    assert 400 <= d["step_freq"].min() and d["step_freq"].max() <= 5000 and abs(d["step_freq"].mean() - 2700) < 5 * 4600 / np.sqrt(12 * n)
    assert d["sweep_f_low"].min() == 20 and d["sweep_f_low"].max() == 999 and d["sweep_f_high"].min() >= 1000 and d["sweep_f_high"].max() <= 19999
    assert abs(d["sweep_amp_too"].mean() - 1 / 3) <= 5 * np.sqrt(2 / 9 / n)
    assert d["sweep_amp"].max() <= 0.9 and d["white10"].max() <= 0.2 and d["pink10"].max() <= 0.2 and 0.2 <= d["pink11"].min() and d["pink11"].max() <= 0.8
    assert d["spike_loc"].shape == (n, 50) and d["spike_loc"].min() == 0 and d["spike_loc"].max() == 8192 - 3 and np.abs(d["spike_height"]).max() <= 0.7
    # the spike index of the reference, int(int(u L - 2) + t[-1]), on the replica's own uniform draws
    u = (d["spike_height"][0].astype(np.float64) / 0.7 + 1) / 2                # not the position draws: only the formula is checked here
    for L_, t_last in ((8192, tl), (65536, 65535 / SR)):
        for v in list(u[:8]) + [0.0, 1e-5, 2.5 / L_, 1 - 2.0 ** -24]:
            want = R.spike_loc(v, L_, t_last)
            got = int(np.trunc(np.trunc(v * L_ - 2.0) + t_last))
            assert want == got and -1 <= want <= L_ - 2
    s = datasets.synth_feed_stream(3, 5, 13, np.arange(4096))
    assert s.dtype == np.float32 and 0 <= s.min() and s.max() < 1 and abs(s.mean() - 0.5) < 5 / np.sqrt(12 * 4096)
    assert not np.array_equal(s, datasets.synth_feed_stream(3, 5, 17, np.arange(4096)))


# ---------------------------------------------------------------------------------------------- the C entry's refusals
def test_families_entry_refuses_before_any_launch():
    from signaltrain_amd import _lib
    lib = _lib.load()
    lo = (C.c_float * 4)(-30.0, 1.0, 1e-3, 1e-3); hi = (C.c_float * 4)(0.0, 5.0, 4e-2, 4e-2)
    x = C.c_void_p(64)                                                         # never dereferenced: every call below is refused

    def call(mask, chooser, fx=_lib.FX_COMP4C, K=4, ptr=x):
        return lib.st_synth_effect_families(fx, mask, 1, 0, 4, 8192, 2048, K, 44100.0, lo, hi, 0, chooser, None, ptr, ptr, ptr, None, None)
    assert _lib.FAMILIES_COMPRESSOR == 0xD7 == _lib.family_mask(None) == _lib.family_mask(AD.COMPRESSOR_CHOOSERS) and _lib.family_mask(range(12)) == _lib.FAMILIES_ALL == 0xFFF
    for mask, chooser, word in ((0, -1, b"empty"), (0x1000, -1, b"past family 11"), (0xFFF | 1 << 31, 3, b"past family 11"),
                                (0xFFF, 12, b"superposition"), (0xFFF, 13, b"superposition"), (0xD7, 99, b"superposition"),
                                (0xFFF, -2, b"forced family -2"), (0xFFF, 101, b"superposition")):
        assert call(mask, chooser) == -1, (mask, chooser)
        err = lib.st_last_error()
        assert word in err and b"st_synth_effect_families" in err, (mask, chooser, err)
    # what st_synth_effect refuses, under the new entry's name
    assert call(0xFFF, 3, fx=9) == -1 and b"st_synth_effect_families: effect 9" in lib.st_last_error()
    assert call(0xFFF, 3, fx=_lib.FX_LOWPASS, K=4) == -1 and b"st_synth_effect_families: ST_FX_LOWPASS takes 1 knob" in lib.st_last_error()
    for chooser in (-1, 3, 5, 8, 9, 10, 11, 0, 7, 100):                       # every family passes the family rules: the null pointer is what stops these
        assert call(0xFFF, chooser, ptr=None) == -1 and b"st_synth_effect_families: null pointer" in lib.st_last_error(), chooser
    # st_synth_effect and st_synth_comp4c keep their rule and their words
    for fn, head in ((lambda ch: lib.st_synth_effect(_lib.FX_COMP4C, 1, 0, 4, 8192, 2048, 4, 44100.0, lo, hi, 0, ch, None, x, x, x, None, None), b"st_synth_effect"),
                     (lambda ch: lib.st_synth_comp4c(1, 0, 4, 8192, 2048, 4, 44100.0, lo, hi, 0, ch, None, x, x, x, None, None), b"st_synth_effect")):
        for ch in (3, 5, 8, 9, 10, 11, 12):
            assert fn(ch) == -1
            assert lib.st_last_error() == head + b": signal family %d is not built (the compressor's set is 0,1,2,4,6,7)" % ch


# ---------------------------------------------------------------------------------------------- datasets
def test_dataset_choosers_plumbing(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)            # the CPU-device form of the generators, with or without a GPU
    fx = audio.Compressor_4c()
    np.random.seed(6)
    ds = datasets.SynthAudioDataSet(1024, fx, datapoints=8, y_size=256, item_chunk=8)
    assert ds.choosers == datasets.COMPRESSOR_CHOOSERS == AD.COMPRESSOR_CHOOSERS
    ds11 = datasets.SynthAudioDataSet(1024, fx, datapoints=8, y_size=256, item_chunk=8, choosers=[11, 11], augment=False)
    assert ds11.choosers == (11,)
    pink_only = np.stack([ds11[i][0] for i in range(8)])
    even = np.abs(pink_only[:, 1:512] - pink_only[:, :512:-1]).max()           # 1/f noise of a real spectrum is an even sequence: no other family is
    assert pink_only.shape == (8, 1024) and even < 1e-5 and 0.2 - 1e-6 <= np.abs(pink_only).max(1).min() and np.abs(pink_only).max() <= 0.8 + 1e-6
    x, y, k = ds11[0]
    assert x.dtype == np.float32 and y.shape == (256,) and k.shape == (4,)
    # the dataset's argument wins, then the effect's attribute, then the compressor's set
    assert audio.Effect.feed_choosers is None

    class Swept(audio.Compressor_4c):
        feed_choosers = (9, 8)
    assert datasets.SynthAudioDataSet(1024, Swept(), datapoints=8, y_size=256).choosers == (8, 9)
    assert datasets.SynthAudioDataSet(1024, Swept(), datapoints=8, y_size=256, choosers=[3]).choosers == (3,)
    rec = datasets.SynthAudioDataSet(1024, Swept(), datapoints=6, y_size=256, recycle=True, item_chunk=4)
    peaks = np.abs(rec.x).max(1)
    assert rec.x.shape == (6, 1024) and np.all((peaks >= 0.6 - 1e-6) & (peaks <= 0.9 + 1e-6))      # both families are normish'd
    for bad in ([], [12], [-1], [0, 100]):
        with pytest.raises(ValueError, match="0..11"):
            datasets.SynthAudioDataSet(1024, fx, datapoints=8, y_size=256, choosers=bad)
    import inspect
    from signaltrain_amd import train
    assert inspect.signature(train.train).parameters["choosers"].default is None
    assert inspect.signature(datasets.DeviceRecycledDataSet.__init__).parameters["choosers"].default is None
