"""GPU: all twelve signal families of audio.synth_input_sample in the fused feed (st_synth_effect_families, csrc/st_feed.h).

With the compressor's mask the new entry is st_synth_effect, bit for bit.  The families the compressor's set leaves out -- 3 triangle + 1/f noise,
5 spikes + normal noise, 8 ampexpstepup, 9 sweep, 10 box + white + 1/f noise, 11 scaled 1/f noise -- are REPLAYED: their parameters come from the
host replica of the feed's second draw sequence (datasets.synth_feed_draw, exact), their values from the float64 restatement of the reference
(tests/signal_families_ref.py, pinned by golden G17).  Polarity and normish gain belong to the first sequence, which has no host replica: both
signs are tried and normalised families are compared at unit peak.

Yardstick for values (the project's optimizer-tail precedent): 4 x the deviation of a float32 numpy evaluation of the same formula and
parameters from the float64 one, computed here per window, plus 1e-8 for the noise of audio.py:333.  Sums of replayed parts are compared to
ULPS float32 ulp of the window's peak (each of the few terms of such a sum is rounded once)."""
import ctypes as C
import numpy as np
import pytest
import torch

from tests import signal_families_ref as R

pytestmark = pytest.mark.gpu
SR = 44100.0
SEED, FIRST = 91, 5000
COMPRESSOR, ALL = 0xD7, 0xFFF
ULPS = 8
F32 = np.float32


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _effect(name):
    from signaltrain_amd import audio
    return getattr(audio, name)()


def _feed(fx, B, L, ysz, mask=ALL, chooser=-1, augment=1, scratch=False, first=FIRST, seed=SEED, entry="families"):
    """(x, y, knobs) of windows [first, first + B) of stream `seed` for the Effect object fx"""
    from signaltrain_amd import _lib
    lib = _lib.load()
    K, rng = len(fx.knob_ranges), fx.feed_ranges()
    x = torch.empty(B, L, device="cuda"); y = torch.empty(B, ysz, device="cuda"); kn = torch.empty(B, K, device="cuda")
    lo = (C.c_float * 4)(*[float(v) for v in rng[:, 0]]); hi = (C.c_float * 4)(*[float(v) for v in rng[:, 1]])
    scr = torch.empty(int(lib.st_synth_effect_scratch_floats(fx.feed_fx, B, L)), device="cuda") if scratch else None
    tail = (seed, first, B, L, ysz, K, SR, lo, hi, augment, chooser, None, _lib.ptr(x), _lib.ptr(y), _lib.ptr(kn), _lib.ptr(scr), _stream())
    if entry == "families":
        _lib.check(lib.st_synth_effect_families(fx.feed_fx, mask, *tail), "st_synth_effect_families")
    else:
        _lib.check(lib.st_synth_effect(fx.feed_fx, *tail), "st_synth_effect")
    return x, y, kn


_windows = {}


def _clean(family, L, B=8):
    """The clean windows [FIRST, FIRST + B) of one forced family (float64 host array): made once and shared"""
    k = (family, L, B)
    if k not in _windows:
        scratch = L > 8192
        x, _, _ = _feed(_effect("Compressor_4c"), B, L, L // 4, chooser=family, augment=0, scratch=scratch)
        _windows[k] = x.cpu().numpy().astype(np.float64)
    return _windows[k]


def _draw(b, L):
    from signaltrain_amd import datasets
    return datasets.synth_feed_draw(SEED, FIRST + b, L, SR, choosers=range(12))


def _stream_u(b, s, L):
    from signaltrain_amd import datasets
    return datasets.synth_feed_stream(SEED, FIRST + b, s, np.arange(L))


def _best_sign(x, ref):
    """(error, sign) of the polarity that brings ref closer to x"""
    ep, em = np.abs(x - ref).max(), np.abs(x + ref).max()
    return (ep, 1.0) if ep <= em else (em, -1.0)


# ---------------------------------------------------------------------------------------------- the compressor's mask
@pytest.mark.parametrize("cls", ["Compressor_4c", "Compressor", "LowPass", "Denoise"])
def test_compressor_mask_is_st_synth_effect(cls):
    fx = _effect(cls)
    for L, ysz, B in ((8192, 2048, 16), (256, 64, 5)):
        for scratch in (False, True):
            for augment in (0, 1):
                a = _feed(fx, B, L, ysz, mask=COMPRESSOR, augment=augment, scratch=scratch)
                b = _feed(fx, B, L, ysz, augment=augment, scratch=scratch, entry="effect")
                for i in range(3):
                    assert torch.equal(a[i], b[i]), (cls, L, scratch, augment, i)
    a = _feed(fx, 4, 16384, 4096, mask=COMPRESSOR, scratch=True)             # the long window's noise through the scratch
    b = _feed(fx, 4, 16384, 4096, scratch=True, entry="effect")
    for i in range(3):
        assert torch.equal(a[i], b[i]), (cls, 16384, i)
    # a forced family of the compressor's set is the same window whatever the mask holds
    a = _feed(fx, 4, 8192, 2048, mask=0x28, chooser=7)
    b = _feed(fx, 4, 8192, 2048, chooser=7, entry="effect")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ---------------------------------------------------------------------------------------------- replay
@pytest.mark.parametrize("L", [256, 8192])
def test_replay_step_family_8(L):
    X, t = _clean(8, L), R.time_values(L)
    edB = R.env_dB(L)
    bounds = np.flatnonzero(np.diff(edB) != 0)
    bounds = np.concatenate([bounds, bounds + 1])                              # the last sample of a level and the first of the next
    worst, covered = 0.0, 0
    for b in range(X.shape[0]):
        d = _draw(b, L)
        r64, r32 = R.step_from(t, d["step_freq"]), R.step_from(t, d["step_freq"], dtype=F32).astype(np.float64)
        u64, u32 = r64 / np.abs(r64).max(), r32 / np.abs(r32).max()
        peak = np.abs(X[b]).max()
        assert 0.6 - 1e-6 <= peak <= 0.9 + 1e-6, (b, peak)
        yard = 4 * np.abs(u32 - u64).max() + 2e-8 / peak
        err, sgn = _best_sign(X[b] / peak, u64)
        print(f"family 8 L={L} window {b}: freq {d['step_freq']:.1f} peak {peak:.4f} error {err:.3g} yardstick {yard:.3g}")
        assert err <= yard, (b, err, yard)
        worst = max(worst, err / yard)
        # the steps: wherever the tone is not near a zero the level read off the window is the integer dB of floor(linspace(-30, 0, L)) exactly
        s = np.sin(float(d["step_freq"]) * t)
        ok = np.abs(s) > 0.05
        lev = 10 * np.log10(np.abs(X[b][ok]) / peak * np.abs(r64).max() / np.abs(s[ok]))
        assert np.array_equal(np.rint(lev), edB[ok]), b
        covered += int(ok[bounds].sum())
    assert covered >= 0.8 * X.shape[0] * len(bounds)
    print(f"family 8 L={L}: worst error / yardstick {worst:.3g}")


@pytest.mark.parametrize("L", [256, 8192])
def test_replay_sweep_family_9(L):
    X, t = _clean(9, L, B=12), R.time_values(L)
    worst, too = 0.0, 0
    for b in range(X.shape[0]):
        d = _draw(b, L)
        p = (d["sweep_f_low"], d["sweep_f_high"], d["sweep_amp"], bool(d["sweep_amp_too"]))
        assert 20 <= p[0] < 1000 <= p[1] < 20000
        too += p[3]
        r64, r32 = R.sweep_from(t, *p), R.sweep_from(t, *p, dtype=F32).astype(np.float64)
        u64, u32 = r64 / np.abs(r64).max(), r32 / np.abs(r32).max()
        peak = np.abs(X[b]).max()
        assert 0.6 - 1e-6 <= peak <= 0.9 + 1e-6, (b, peak)
        yard = 4 * np.abs(u32 - u64).max() + 2e-8 / peak
        err, _ = _best_sign(X[b] / peak, u64)
        print(f"family 9 L={L} window {b}: {p[0]}-{p[1]} Hz amp_too {p[3]} peak {peak:.4f} error {err:.3g} yardstick {yard:.3g}")
        assert err <= yard, (b, err, yard)
        worst = max(worst, err / yard)
    assert 0 < too < X.shape[0]                                                # both forms of the sweep are among the windows
    print(f"family 9 L={L}: worst error / yardstick {worst:.3g}")


@pytest.mark.parametrize("L", [256, 8192])
def test_replay_spikes_family_5(L):
    X = _clean(5, L)
    worst, overlaps = 0.0, 0
    for b in range(X.shape[0]):
        d = _draw(b, L)
        loc, h, amp = d["spike_loc"], d["spike_height"], d["spike_amp"]
        assert loc.shape == (50,) and loc.min() >= 0 and loc.max() < L and np.abs(h).max() <= 0.7
        u1, u2 = _stream_u(b, 13, L), _stream_u(b, 17, L)
        sp = R.spikes_from(L, loc, h)
        r64 = sp + float(amp) * R.normal_from(u1, u2)
        r32 = (R.spikes_from(L, loc, h, dtype=F32) + F32(amp) * R.normal_from(u1, u2, dtype=F32)).astype(np.float64)
        yard = 4 * np.abs(r32 - r64).max() + 1e-8
        err, sgn = _best_sign(X[b], r64)
        print(f"family 5 L={L} window {b}: noise {amp:.4f} error {err:.3g} yardstick {yard:.3g}")
        assert err <= yard, (b, err, yard)
        worst = max(worst, err / yard)
        assert np.abs(X[b]).max() <= 0.7 + 0.1 * np.sqrt(2 * 24 * np.log(2)) + 1e-6
        # positions and order: without the replayed noise exactly the samples the spikes were written to are left, with the value of the LAST write
        bare = sgn * X[b] - float(amp) * R.normal_from(u1, u2)
        assert np.array_equal(np.abs(bare) > 2 * yard, np.abs(sp) > 2 * yard), b
        touched = np.zeros(L, dtype=int)
        for l in loc:
            touched[[l, (l + 1) % L, (l - 1) % L]] += 1
        overlaps += int((touched > 1).sum())
    assert overlaps > 0                                                        # some sample was written twice: the order mattered
    print(f"family 5 L={L}: worst error / yardstick {worst:.3g}, {overlaps} samples written more than once")


# ---------------------------------------------------------------------------------------------- the 1/f part
def _ulp_tol(x):
    return ULPS * 2.0 ** -24 * max(1.0, float(np.abs(x).max())) + 1e-8


@pytest.mark.parametrize("L", [256, 8192, 16384])
def test_pink_part_families_3_and_11(L):
    """window - replayed deterministic part == replayed amount x the same window's chooser = 100 noise"""
    pink, t = _clean(100, L), R.time_values(L)
    assert np.allclose(np.abs(pink).max(axis=1), 1.0, atol=1e-6)
    X11, X3 = _clean(11, L), _clean(3, L)
    for b in range(pink.shape[0]):
        d = _draw(b, L)
        assert 0.2 <= d["pink11"] <= 0.8 and 0.02 <= d["tri_amp"] <= 0.12
        err, _ = _best_sign(X11[b], float(d["pink11"]) * pink[b])
        tol = _ulp_tol(X11[b])
        print(f"family 11 L={L} window {b}: amount {d['pink11']:.4f} error {err:.3g} bound {tol:.3g}")
        assert err <= tol, (b, err, tol)
        p = (d["tri_height"], d["tri_width"], d["tri_t0"])
        assert 0.4 <= abs(p[0]) <= 0.8 and 0 <= p[1] <= d["tl"] / 4 and p[2] <= 0.9 * d["tl"] * (1 + 1e-6)
        r64, r32 = R.triangle_from(t, *p), R.triangle_from(t, *p, dtype=F32).astype(np.float64)
        yard = 4 * np.abs(r32 - r64).max() + _ulp_tol(X3[b])
        err, _ = _best_sign(X3[b], r64 + float(d["tri_amp"]) * pink[b])
        print(f"family 3 L={L} window {b}: height {p[0]:.3f} width {p[1]:.4f} t0 {p[2]:.4f} amount {d['tri_amp']:.4f} error {err:.3g} yardstick {yard:.3g}")
        assert err <= yard, (b, err, yard)
        peak = np.abs(X3[b]).max()                                             # not normalised: the triangle's apex under its noise
        assert np.abs(r64).max() - d["tri_amp"] - 1e-6 <= peak <= abs(p[0]) + d["tri_amp"] + 1e-6


@pytest.mark.parametrize("L", [256, 8192, 16384])
def test_family_10_is_a_box_under_replayed_noise(L):
    pink, X = _clean(100, L), _clean(10, L)
    for b in range(X.shape[0]):
        d = _draw(b, L)
        assert 0 <= d["white10"] <= 0.2 and 0 <= d["pink10"] <= 0.2
        noise = float(d["white10"]) * (2.0 * _stream_u(b, 3, L).astype(np.float64) - 1.0) + float(d["pink10"]) * pink[b]
        tol = _ulp_tol(X[b])
        found = False
        for sgn in (1.0, -1.0):
            box = sgn * X[b] - noise
            cuts = np.flatnonzero(np.abs(np.diff(box)) > 2 * tol) + 1
            if len(cuts) > 3:
                continue
            segs = np.split(box, cuts)
            if any(np.ptp(s) > 2 * tol for s in segs):
                continue
            lv = [float(np.median(s)) for s in segs]
            # box (audio.py:106-122): h_bgn in [0, 0.15] up to i_up - 2, ONE sample of h_end, h_mid in [0.6, 0.95] on [i_up, i_dn), h_end in [0.1, 0.3]
            if not (0.1 - tol <= lv[-1] <= 0.3 + tol):
                continue
            mids = [v for v, s in zip(lv, segs) if v > 0.5]
            assert len(mids) == 1 and 0.6 - tol <= mids[0] <= 0.95 + tol, (b, lv)
            for v, s in zip(lv, segs):
                assert v > 0.5 or -tol <= v <= 0.3 + tol, (b, lv)
                assert v > 0.5 or abs(v - lv[-1]) <= 2 * tol or (s is segs[0] and v <= 0.15 + tol), (b, lv)
            found = True
            print(f"family 10 L={L} window {b}: plateaus {[round(v, 4) for v in lv]} at {cuts.tolist()} white {d['white10']:.4f} 1/f {d['pink10']:.4f}")
            break
        assert found, b


# ---------------------------------------------------------------------------------------------- targets, reproducibility, sets
@pytest.mark.parametrize("family", [3, 5, 8, 9, 10, 11])
def test_target_is_the_effect_of_the_generated_window(family):
    from signaltrain_amd import _lib, audio
    L, ysz, B = 8192, 2048, 6
    clean = None
    for cls in ("Compressor_4c", "Compressor", "LowPass", "Denoise"):
        fx = _effect(cls)
        for scratch in ((False, True) if cls.startswith("Compressor") else (False,)):
            x, y, kn = _feed(fx, B, L, ysz, chooser=family, scratch=scratch)
            assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all()) and float(kn.min()) >= -0.5 and float(kn.max()) <= 0.5
            if cls == "Compressor_4c" and clean is None:
                clean = x
            if cls == "Denoise":
                assert torch.equal(y, clean[:, -ysz:])
                s = audio._knobs_wc_device(fx.knob_ranges, kn, "cuda")
                xn = torch.empty_like(clean)
                _lib.check(_lib.load().st_denoise_input(SEED, FIRST, _lib.ptr(clean), _lib.ptr(s), B, L, _lib.ptr(xn), _stream()), "st_denoise_input")
                assert torch.equal(x, xn)
                continue
            assert torch.equal(x, clean), (cls, scratch)                       # the clean window does not depend on the effect or its form
            y2 = fx.go_device(x, kn, ysz)                                      # the stand-alone effect kernel on the same windows
            if cls == "LowPass":
                assert torch.equal(y, y2) and not torch.equal(y, x[:, -ysz:])
            else:                                                              # (a quiet window may pass a compressor untouched: no such check there)
                assert float((y - y2).abs().max()) <= 1e-6 * float(y2.abs().max()), (cls, scratch)


def test_custom_set_windows_are_a_function_of_the_index_only():
    fx, mask = _effect("LowPass"), 0b101100101000                              # {3, 5, 8, 9, 11}
    whole = _feed(fx, 24, 8192, 2048, mask=mask)
    parts = [_feed(fx, 7, 8192, 2048, mask=mask), _feed(fx, 17, 8192, 2048, mask=mask, first=FIRST + 7)]
    for i in range(3):
        assert torch.equal(whole[i], torch.cat([p[i] for p in parts])), i
    other = _feed(fx, 24, 8192, 2048, mask=mask, seed=SEED + 1)
    assert not torch.equal(whole[0], other[0])
    long_ = _feed(fx, 6, 16384, 4096, mask=mask, scratch=True)                 # the long window: the noise passes know the set's families
    parts = [_feed(fx, 2, 16384, 4096, mask=mask, scratch=True), _feed(fx, 4, 16384, 4096, mask=mask, scratch=True, first=FIRST + 2)]
    for i in range(3):
        assert torch.equal(long_[i], torch.cat([p[i] for p in parts])), i
    assert bool(torch.isfinite(long_[0]).all())


@pytest.mark.parametrize("L", [256, 16384])
def test_custom_set_draws_only_its_members(L):
    """Window b of a set is the forced window of the family synth_feed_draw names for it -- every member comes up, nothing else does"""
    from signaltrain_amd import datasets
    fams, B = (3, 4, 9, 10, 11), 32
    fx = _effect("Compressor_4c")
    scratch = L > 8192
    x, y, kn = _feed(fx, B, L, L // 4, mask=sum(1 << f for f in fams), scratch=scratch)
    drawn = datasets.synth_feed_draw(SEED, FIRST + np.arange(B), L, SR, choosers=fams)["family"]
    assert set(drawn.tolist()) == set(fams)
    forced = {f: _feed(fx, B, L, L // 4, chooser=f, scratch=scratch) for f in fams}
    for b in range(B):
        for i, t in enumerate((x, y, kn)):
            assert torch.equal(t[b], forced[int(drawn[b])][i][b]), (b, int(drawn[b]), i)
        others = [f for f in fams if f != int(drawn[b])]
        assert all(not torch.equal(x[b], forced[f][0][b]) for f in others), b


def test_dataset_and_train_take_choosers(tmp_path, monkeypatch):
    from signaltrain_amd import audio, datasets, nn_proc, train
    nn_proc._QUIET = True
    np.random.seed(4)
    ds = datasets.SynthAudioDataSet(8192, audio.LowPass(), y_size=2048, choosers=[9, 8, 11, 5, 3])
    assert ds.choosers == (3, 5, 8, 9, 11)
    x, y, kn = ds.batch_device(16)
    drawn = datasets.synth_feed_draw(ds._feed_seed, np.arange(16), 8192, 44100, choosers=ds.choosers)["family"]
    x9, _, _ = datasets.SynthAudioDataSet(8192, audio.LowPass(), y_size=2048, choosers=[9]).batch_device(1)
    assert ds._feed_count == 16 and bool(torch.isfinite(x).all()) and set(drawn.tolist()) <= set(ds.choosers)
    b9 = int(np.flatnonzero(drawn == 9)[0])
    peak = float(x[b9].abs().max())
    assert 0.6 - 1e-6 <= peak <= 0.9 + 1e-6 and x9.shape == (1, 8192)
    rec = datasets.DeviceRecycledDataSet(8192, audio.LowPass(), datapoints=8, y_size=2048, choosers=[11], gen_batch=8)
    assert rec.choosers == (11,) and rec.x.shape == (8, 8192)
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0); np.random.seed(0)
    seen = []
    init = datasets.SynthAudioDataSet.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw); seen.append(self.choosers)
    monkeypatch.setattr(datasets.SynthAudioDataSet, "__init__", spy)
    train.train(effect=audio.LowPass(), epochs=1, n_data_points=256, batch_size=64, device=torch.device("cuda:0"), device_feed=True, lr_max=2e-4,
                choosers=[0, 1, 3, 4, 6, 10, 2, 7, 9])
    assert seen and all(c == (0, 1, 2, 3, 4, 6, 7, 9, 10) for c in seen)
    lines = [l.split() for l in open("vl_avg_out.dat").read().strip().splitlines()]
    assert len(lines) == 1 and np.isfinite(float(lines[0][-1]))
