"""CPU: the LowPass and Denoise effects (signaltrain/audio.py:610-625, :558-571) on the host -- audio.lowpass against scipy's butter + lfilter,
the effects' knobs and the (target, input) pair of Denoise, the modal scan of csrc/st_filter.h restated in numpy against lfilter, the closed-form
poles against butter's denominator, the refusals of the new entry points (no launch: runs without a GPU) and the Dataset items of Denoise."""
import ctypes as C
import numpy as np
import pytest
from scipy.signal import butter, lfilter

from signaltrain_amd import _lib, audio

SR = 44100.0
CUTOFFS = (10.0, 10.5, 33.0, 100.0, 700.0, 2000.0)


def _signals(L, seed=0):
    rng = np.random.default_rng(seed)
    n = np.arange(L)
    box = np.full(L, 0.1, dtype=np.float32); box[L // 5:L // 2] = 0.8; box[L // 2:] = 0.2
    imp = np.zeros(L, dtype=np.float32); imp[0] = 1.0
    return {"white": (2.0 * rng.random(L) - 1.0).astype(np.float32), "box": box,
            "sine30": (0.7 * np.sin(2 * np.pi * 30.0 * n / SR)).astype(np.float32), "impulse": imp}


def modal_design(fc, sr):
    """Poles, residues and direct term of the parallel form (csrc/st_filter.h), float64 / complex128."""
    K = np.tan(np.pi * fc / sr)
    s = np.array([-1.0, np.exp(2j * np.pi / 3), np.exp(-2j * np.pi / 3)])
    p = (1 + K * s) / (1 - K * s)
    b0 = K ** 3 / ((1 + K) * (1 + K + K * K))
    r = np.array([b0 * (1 + 1 / p[k]) ** 3 / np.prod([1 - p[j] / p[k] for j in range(3) if j != k]) for k in range(3)])
    d = (-b0 / np.prod(p)).real
    return p, r, d


def _mode_scan(x, p, R=8, T=256, W=64):
    """s[n] = p s[n-1] + x[n] from s[-1] = 0 the way the device runs it: chunks of T runs of R samples; per run the map s -> p^m s + v from a zero
    start, a doubling (Hillis-Steele) combine of the maps over each wave of W runs, the waves' maps composed in order, the chunk's carry, and
    every run replayed from its incoming state.  Ragged last run / chunk: absent samples leave the map untouched."""
    L = len(x); CH = R * T
    out = np.empty(L, dtype=np.complex128)
    carry = 0j
    for c0 in range(0, L, CH):
        n = min(CH, L - c0)
        xc = np.zeros(CH); xc[:n] = x[c0:c0 + n]
        xr = xc.reshape(T, R); valid = (np.arange(CH) < n).reshape(T, R)
        A = np.ones(T, dtype=np.complex128); B = np.zeros(T, dtype=np.complex128)
        for k in range(R):
            A = np.where(valid[:, k], A * p, A); B = np.where(valid[:, k], p * B + xr[:, k], B)
        A = A.reshape(T // W, W); B = B.reshape(T // W, W)
        o = 1
        while o < W:
            Ao = np.ones_like(A); Bo = np.zeros_like(B)
            Ao[:, o:] = A[:, :-o]; Bo[:, o:] = B[:, :-o]                        # lanes below o combine with the identity
            B = A * Bo + B; A = A * Ao
            o *= 2
        Ae = np.ones_like(A); Be = np.zeros_like(B)
        Ae[:, 1:] = A[:, :-1]; Be[:, 1:] = B[:, :-1]                            # exclusive: the map of the lanes below
        s_in = np.empty((T // W, W), dtype=np.complex128)
        sw = carry
        for w in range(T // W):
            s_in[w] = Ae[w] * sw + Be[w]
            sw = A[w, W - 1] * sw + B[w, W - 1]
        s = s_in.reshape(T)
        S = np.empty((T, R), dtype=np.complex128)
        for k in range(R):
            s = np.where(valid[:, k], p * s + xr[:, k], s); S[:, k] = s
        carry = s[T - 1]
        out[c0:c0 + n] = S.reshape(CH)[:n]
    return out


def modal_lowpass(x, fc, sr):
    """y = d x + r_0 s0 + 2 Re(r_1 s1) with the real mode's terms regrouped as the kernel has them: (d + r_0) x[n] + (r_0 p_0) s0[n-1],
    d + r_0 = b0 - 2 Re(r_1) and r_0 p_0 = b0 (1 + p_0)^3 / |p_0 - p_1|^2 (no 1 / p_0: finite at fc = sr / 4, where p_0 = 0)."""
    p, r, d = modal_design(fc, sr)
    K = np.tan(np.pi * fc / sr)
    b0 = K ** 3 / ((1 + K) * (1 + K + K * K))
    g, q0 = b0 - 2.0 * r[1].real, b0 * (1 + p[0].real) ** 3 / abs(p[0] - p[1]) ** 2
    x = np.asarray(x, dtype=np.float64)
    s0 = _mode_scan(x, p[0].real + 0j).real
    s1 = _mode_scan(x, p[1])
    s0_prev = np.concatenate([[0.0], s0[:-1]])
    return g * x + q0 * s0_prev + 2.0 * (r[1] * s1).real


def test_host_lowpass_is_butter_plus_lfilter():
    x = _signals(4096, seed=1)["white"]
    for fc in (10.0, 333.0, 2000.0):
        b, a = butter(3, fc / (SR / 2))
        ref = lfilter(b, a, x).astype(np.float32)
        y = audio.lowpass(x, fc, SR)
        assert y.dtype == np.float32 and np.array_equal(y, ref)
        yy, xx = audio.LowPass().go_wc(x, [fc])
        assert np.array_equal(yy, ref) and xx is x


def test_effect_declarations():
    lp, dn = audio.LowPass(), audio.Denoise()
    assert lp.name == "LowPass" and lp.knob_names == ["cutoff"] and np.array_equal(lp.knob_ranges, [[10, 2000]])
    assert lp.knobs_wc(np.array([-0.5])) == [10.0] and lp.knobs_wc(np.array([0.5])) == [2000.0]
    assert lp.feed_fx == _lib.FX_LOWPASS == 2 and not lp.is_inverse
    assert dn.name == "Denoise" and dn.knob_names == ["strength"] and np.array_equal(dn.knob_ranges, [[0.0, 0.5]])
    assert dn.feed_fx == _lib.FX_DENOISE == 3 and dn.is_inverse
    assert lp.feed_ranges().shape == dn.feed_ranges().shape == (4, 2)


def test_denoise_returns_clean_target_and_bounded_noise():
    np.random.seed(4)
    x = _signals(4096, seed=2)["sine30"]
    fx = audio.Denoise()
    for k in (-0.5, -0.1, 0.3, 0.5):
        strength = fx.knobs_wc(np.array([k]))[0]
        y, xn = fx.go(x, np.array([k]))
        assert y is x and xn.dtype == np.float32 and xn.shape == x.shape
        err = np.abs(xn.astype(np.float64) - x.astype(np.float64))
        assert err.max() <= strength + 2.0 ** -24 * (np.abs(x).max() + strength) * 2        # the noise's and the sum's float32 roundings
        if strength > 0:
            assert err.max() > 0.5 * strength
        else:
            assert np.array_equal(xn, x)


def test_modal_scan_restatement_matches_lfilter():
    """Self-contained by design (runs no library code): the device algorithm in numpy float64 against scipy's sequential float64 lfilter: 1e-5 of max(1e-3, max |ref|) (the bound between a device
    effect and its host reference elsewhere in the suite).  Measured worst ratio: 3e-7 (lfilter itself is 7.5e-8 away from a long-double run at
    10 Hz: the direct-form coefficients are ill-conditioned there)."""
    L, ysz = 8192, 2048
    sig = _signals(L)
    worst = 0.0
    for fc in CUTOFFS:
        b, a = butter(3, fc / (SR / 2))
        for name, x in sig.items():
            ref = lfilter(b, a, x.astype(np.float64))[-ysz:]
            y = modal_lowpass(x, fc, SR)[-ysz:]
            ratio = np.abs(y - ref).max() / max(1e-3, np.abs(ref).max())
            worst = max(worst, ratio)
            assert ratio <= 1e-5, (fc, name, ratio)
    print(f"modal scan vs lfilter: worst ratio {worst:.3g}")


def test_closed_form_poles_are_butters():
    """Self-contained by design: the closed-form design st_filter.h uses, restated above, against scipy's butter."""
    for fc in CUTOFFS + (5000.0, 15000.0):
        p, r, d = modal_design(fc, SR)
        b, a = butter(3, fc / (SR / 2))
        assert np.abs(np.poly(p).real - a).max() <= 1e-13 and np.abs(np.poly(p).imag).max() <= 1e-13, fc
        # ... and the parallel form is the same transfer function: its impulse response is lfilter's
        imp = np.zeros(64); imp[0] = 1.0
        n = np.arange(64)
        h = (r[:, None] * p[:, None] ** n[None, :]).sum(0).real + d * imp
        href = lfilter(b, a, imp)
        assert np.abs(h - href).max() <= 1e-9 * max(np.abs(href).max(), 1e-3), fc


def _feed_call(fx, K, lo0, hi0, x=None):
    lib = _lib.load()
    lo = (C.c_float * 4)(lo0, 0, 0, 0); hi = (C.c_float * 4)(hi0, 0, 0, 0)
    return lib.st_synth_effect(fx, 1, 0, 4, 8192, 2048, K, SR, lo, hi, 0, -1, None, x, x, x, None, None)


def test_feed_refuses_bad_knob_counts_and_ranges_without_a_gpu():
    lib = _lib.load()
    assert _feed_call(_lib.FX_LOWPASS, 2, 10, 2000) == -1 and b"K=2" in lib.st_last_error() and b"ST_FX_LOWPASS" in lib.st_last_error()
    assert _feed_call(_lib.FX_DENOISE, 4, 0, 0.5) == -1 and b"K=4" in lib.st_last_error() and b"ST_FX_DENOISE" in lib.st_last_error()
    for lo0, hi0 in ((10, 22050), (10, 30000), (0, 2000), (-5, 2000), (300, 200)):
        assert _feed_call(_lib.FX_LOWPASS, 1, lo0, hi0) == -1 and b"0 < lo <= hi < sr / 2" in lib.st_last_error(), (lo0, hi0, lib.st_last_error())
    for lo0, hi0 in ((-0.1, 0.5), (0.3, 0.2)):
        assert _feed_call(_lib.FX_DENOISE, 1, lo0, hi0) == -1 and b"0 <= lo <= hi" in lib.st_last_error(), (lo0, hi0)
    # valid ids, counts and ranges get as far as the pointers
    assert _feed_call(_lib.FX_LOWPASS, 1, 10, 2000) == -1 and b"null" in lib.st_last_error()
    assert _feed_call(_lib.FX_DENOISE, 1, 0, 0.5) == -1 and b"null" in lib.st_last_error()
    # no second-launch form: the scratch is only the long windows' noise
    assert lib.st_synth_effect_scratch_floats(_lib.FX_LOWPASS, 4, 8192) == lib.st_synth_effect_scratch_floats(_lib.FX_DENOISE, 4, 8192) == 0
    for fx in (_lib.FX_LOWPASS, _lib.FX_DENOISE):
        assert lib.st_synth_effect_scratch_floats(fx, 4, 16384) == lib.st_synth_effect_scratch_floats(_lib.FX_COMP4C, 4, 16384) - 4 * (16384 + 4) > 0


def test_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float32)
    p = C.c_void_p(buf.ctypes.data)                  # never dereferenced: every call below is refused before any launch
    for args, what in (((None, p, SR, 1, 16, 16, p, None), b"null"), ((p, None, SR, 1, 16, 16, p, None), b"null"), ((p, p, SR, 1, 16, 16, None, None), b"null"),
                       ((p, p, SR, 1, 16, 20, p, None), b"ysz"), ((p, p, SR, 1, 18, 16, p, None), b"multiple of 4"), ((p, p, SR, 0, 16, 16, p, None), b"bad sizes")):
        assert lib.st_lowpass(*args) == -1 and b"st_lowpass" in lib.st_last_error() and what in lib.st_last_error(), (args, lib.st_last_error())
    for args, what in (((1, 0, None, p, 1, 16, p, None), b"null"), ((1, 0, p, None, 1, 16, p, None), b"null"), ((1, 0, p, p, 1, 16, None, None), b"null"),
                       ((1, 0, p, p, 1, 18, p, None), b"multiple of 4"), ((1, 0, p, p, 0, 16, p, None), b"bad sizes")):
        assert lib.st_denoise_input(*args) == -1 and b"st_denoise_input" in lib.st_last_error() and what in lib.st_last_error(), (args, lib.st_last_error())


def test_dataset_items_of_denoise_through_the_host_path(monkeypatch):
    """The host item path takes the effect's second return value as the item's input: the target is the clean window's tail, the input the noisy
    window.  The clean windows are those of a one-knob compressor dataset built from the same seeds (the same generator draws)."""
    import torch
    from signaltrain_amd import datasets
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    items = {}
    for name, fx in (("dn", audio.Denoise()), ("ct", audio.Comp_Just_Thresh())):
        np.random.seed(21)
        ds = datasets.SynthAudioDataSet(8192, fx, y_size=2048, item_chunk=4)
        items[name] = [ds[i] for i in range(4)]
    assert len(items["dn"][0]) == 3
    n_noisy = 0
    for (x, y, k), (xc, _, kc) in zip(items["dn"], items["ct"]):
        assert x.shape == (8192,) and y.shape == (2048,) and k.shape == (1,) and x.dtype == y.dtype == np.float32
        assert np.array_equal(k, kc) and np.array_equal(y, xc[-2048:])                  # the target is the clean signal's tail
        strength = audio.Denoise().knobs_wc(k)[0]
        err = np.abs(x.astype(np.float64) - xc.astype(np.float64))
        assert err.max() <= strength + 2.0 ** -24 * (np.abs(xc).max() + strength) * 2
        n_noisy += bool(err.max() > 0.5 * strength > 0)
    assert n_noisy >= 2
