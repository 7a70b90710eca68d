"""Effects and audio files -- the parts of signaltrain/audio.py the training driver needs: the Effect classes (:449-537, knob names / ranges,
normalised <-> world knob coordinates), the compressor target effects (compressor_4controls :380-426: on the GPU through st_compressor_4c /
st_synth_effect, on the host through the gcc-built helper for file datasets; compressor :349-371: st_compressor / st_synth_effect, and a
numpy / scipy restatement on the host), LowPass (:610-625: st_lowpass / st_synth_effect, scipy on the host) and Denoise (:558-571: the noisy signal
is the input, st_denoise_input / st_synth_effect), Echo (:539-547 over echo() :430-443: st_echo / st_synth_effect, a float32 numpy restatement on
the host) and DeCompressor_4c (:573-583: the compressed signal is the input, st_compressor_4c / st_synth_effect), wav reading / writing (:207-262) and file-defined effects
(:624-670).  The synthetic test signals themselves are generated on the GPU (csrc/st_feed.h, audio_device.py); their numpy restatement lives
on the checker side (oracle/host_audio.py)."""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_AUD = None


def _audio_lib():
    global _AUD
    if _AUD is None:
        path = os.path.join(_HERE, "libst_audio.so")
        if os.path.isfile(path):
            lib = C.CDLL(path)
            lib.st_compressor_4controls.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_double] * 5
            lib.st_compressor_4controls.restype = None
            _AUD = lib
        else:
            _AUD = False
    return _AUD


def compressor_4controls(x, thresh=-24.0, ratio=2.0, attackTime=0.01, releaseTime=0.01, sr=44100.0):
    """audio.py:380-426.  Uses the gcc-built helper when present, else a numpy/python loop."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    lib = _audio_lib()
    if lib:
        y = np.empty_like(x)
        lib.st_compressor_4controls(x.ctypes.data, y.ctypes.data, x.size, float(thresh), float(ratio),
                                    float(attackTime), float(releaseTime), float(sr))
        return y
    N = len(x)
    alphaA = np.exp(-np.log(9) / (sr * attackTime)); alphaR = np.exp(-np.log(9) / (sr * releaseTime))
    x_dB = np.maximum(20 * np.log10(np.abs(x) + 1e-8), -96).astype(np.float32)
    gc = np.zeros(N, dtype=np.float32)
    i = x_dB > thresh
    gc[i] = thresh + (x_dB[i] - thresh) / ratio - x_dB[i]
    lin = np.zeros(N, dtype=np.float32)
    prev = 0.0
    g = gc.tolist()
    out = [0.0] * N
    for n in range(1, N):
        prev = float(np.float32((1 - alphaA) * g[n] + alphaA * prev if g[n] < prev else (1 - alphaR) * g[n] + alphaR * prev))
        out[n] = prev
    lin = np.power(10.0, np.asarray(out, dtype=np.float32) / 20)
    return (lin * x).astype(np.float32)


def compressor(x, thresh=-24.0, ratio=2.0, attackrel=0.045, sr=44100.0):
    """audio.py:349-371 (the `comp` effect): the dB signal 20 log10(|x| + 1e-6) in float32, smoothed by the first-order Butterworth low-pass
    at 1 / (attackrel sr) of Nyquist in float64 -- written out from the bilinear transform, k = tan(pi Wn / 2): b0 = b1 = k / (1 + k), pole
    (1 - k) / (1 + k) -- started from its steady state at the first sample (e[0] = d[0]); the static curve on the smoothed envelope, the gain
    applied in float64 and the result rounded to float32 (the training target's type).  The device form is st_compressor."""
    from scipy.signal import lfilter
    x = np.asarray(x, dtype=np.float32)
    d = np.float32(20.0) * np.log10(np.abs(x) + np.float32(1e-6))
    k = np.tan(np.pi / (2.0 * float(attackrel) * float(sr)))
    b0, p = k / (1.0 + k), (1.0 - k) / (1.0 + k)
    e = lfilter([b0, b0], [1.0, -p], d.astype(np.float64), zi=[(1.0 - b0) * float(d[0])])[0] if len(d) else np.zeros(0)
    out = np.where(e > thresh, thresh + (e - thresh) / ratio, e)
    return (x * np.power(10.0, (out - e) / 20)).astype(np.float32)


def lowpass(x, cutoff, sr=44100.0, order=3):
    """audio.py:618-625 (the `lowpass` effect): scipy's Butterworth low-pass at cutoff / (sr / 2) of Nyquist run by lfilter from a zero state, as
    the reference calls them, in float64; the result rounded to float32 (the training target's type).  The device form is st_lowpass."""
    from scipy.signal import butter, lfilter
    b, a = butter(order, float(cutoff) / (0.5 * float(sr)), btype='low', analog=False)
    return lfilter(b, a, np.asarray(x, dtype=np.float32)).astype(np.float32)


def echo(x, delay_samples=1487, ratio=0.6, echoes=1):
    """audio.py:430-443 (the `echo` effect) on a float32 window: np.round(echoes) copies of x are added to it, copy i delayed by i * delay_samples and
    scaled by ratio ** i; a fractional delay is a two-tap interpolation between the neighbouring whole delays.  The delay length and the power are
    Python floats (float64); the window stays float32 and every product and sum is rounded on its own, which is what the reference's expression
    gives under numpy 2 (Python-float weights on a float32 array) -- bit for bit, tests/golden/g18_echo_decomp.npz.  A delay below one sample is
    refused (the reference raises on its empty slice there).  The device form is st_echo."""
    x = np.asarray(x, dtype=np.float32)
    delay = float(delay_samples)
    if not (1.0 <= delay < np.inf):
        raise ValueError(f"echo: delay_samples = {delay_samples!r}: a finite delay of at least one sample is required")
    L = len(x)
    y = x.copy()
    for i in range(1, int(np.round(echoes)) + 1):
        dl = i * delay
        D = int(np.floor(dl)); diff = dl - D
        a = np.zeros(L, dtype=np.float32); b = np.zeros(L, dtype=np.float32)      # x shifted by D and D + 1 samples, zeros in front
        if D < L: a[D:] = x[:L - D]
        if D + 1 < L: b[D + 1:] = x[:L - D - 1]
        xd = np.float32(1 - diff) * a + np.float32(diff) * b
        y = y + np.float32(pow(float(ratio), i)) * xd
    return y


def _device_effect(fn, effect, x, kw, y_size):
    """y [B, y_size] of the library's effect `fn` (st_compressor_4c / st_compressor) on device tensors x [B, L] with world-coordinate knobs kw [B, K]."""
    import ctypes as C
    import torch
    from . import _lib
    x = x.to(torch.float32).contiguous(); B, L = x.shape
    kw = kw.to(torch.float32).contiguous()
    y_size = L if y_size is None else int(y_size)
    y = torch.empty(B, y_size, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):             # the library launches on the current device
        _lib.check(getattr(_lib.load(), fn)(_lib.ptr(x), _lib.ptr(kw), float(effect.sr), B, L, y_size, _lib.ptr(y),
                                            C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)), fn)
    return y


class Effect:
    """audio.py:449-480.  feed_fx: the st_synth_effect id (_lib.FX_*) of the library's fused device feed for this effect, None if there is none;
    feed_ranges(): the four (low, high) knob rows that feed takes (knobs past len(knob_ranges) are fixed at their low end);
    makes_input: the effect makes the item's input itself (Denoise) -- its go_device returns (y, x_new) and takes seed=, the noise stream;
    feed_choosers: the signal families (audio.synth_input_sample's 0..11) a synthetic dataset of this effect draws from when it is given none;
    None = the compressor's set {0,1,2,4,6,7} (datasets.py:317).
    Of the reference's eleven effects two are not built: PitchShifter (:549-556) is a call into librosa, which this project does not depend on, and
    TimeAlign (:585-607) ignores its input and synthesises a hard-coded 4096-sample window, so it fits none of the window sizes train.train uses."""
    feed_fx = None
    makes_input = False
    feed_choosers = None

    def __init__(self, sr=44100.0, dtype=np.float32):
        self.name = 'Generic Effect'; self.knob_names = ['knob']
        self.knob_ranges = np.array([[0, 1]], dtype=dtype); self.sr = sr; self.is_inverse = False

    def feed_ranges(self):
        r = np.asarray(self.knob_ranges, dtype=np.float64)
        return np.concatenate([r, np.zeros((4 - len(r), 2))]) if len(r) < 4 else r

    def knobs_wc(self, knobs_nn):
        return (self.knob_ranges[:, 0] + (knobs_nn + 0.5) * (self.knob_ranges[:, 1] - self.knob_ranges[:, 0])).tolist()

    def info(self):
        print(f'Effect: {self.name}.  Knobs:')
        for n, r in zip(self.knob_names, self.knob_ranges):
            print(f'                            {n}: {r[0]} to {r[1]}')

    def go_wc(self, x, knobs_wc):
        raise Exception("This effect's go_wc() is undefined")

    def go(self, x, knobs_nn, **kwargs):
        return self.go_wc(x, self.knobs_wc(knobs_nn), **kwargs)


class Compressor(Effect):
    """audio.py:484-491: the envelope compressor (`comp`): threshold, ratio and one attack / release time."""
    feed_fx = 1                                   # _lib.FX_COMP

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.name = 'Compressor'
        self.knob_names = ['threshold', 'ratio', 'attackreleaseTime']
        self.knob_ranges = np.array([[-30, 0], [1, 5], [1e-3, 4e-2]])

    def go_wc(self, x, knobs_w):
        return compressor(x, thresh=knobs_w[0], ratio=knobs_w[1], attackrel=knobs_w[2], sr=self.sr), x

    def go_device(self, x, knobs_nn, y_size=None):
        """Batched effect on the GPU (st_compressor): x [B,L] and knobs_nn [B,3] in [-.5,.5] as device tensors -> y [B,y_size]
        (the last y_size samples).  No CPU fallback."""
        if x.device.type != "cuda":
            raise RuntimeError("Compressor.go_device needs ROCm device tensors")
        return _device_effect("st_compressor", self, x, _knobs_wc_device(self.knob_ranges, knobs_nn, x.device), y_size)


def _knobs_wc_device(knob_ranges, knobs_nn, device):
    """Effect.knobs_wc (audio.py:455) on a [B, K] device tensor, float32."""
    import torch
    lo = torch.as_tensor(np.asarray(knob_ranges)[:, 0], dtype=torch.float32, device=device)
    hi = torch.as_tensor(np.asarray(knob_ranges)[:, 1], dtype=torch.float32, device=device)
    return (lo + (knobs_nn.to(torch.float32) + 0.5) * (hi - lo)).contiguous()


class Compressor_4c(Effect):
    """audio.py:493-500."""
    feed_fx = 0                                   # _lib.FX_COMP4C

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.name = 'Compressor_4c'
        self.knob_names = ['threshold', 'ratio', 'attackTime', 'releaseTime']
        self.knob_ranges = np.array([[-30, 0], [1, 5], [1e-3, 4e-2], [1e-3, 4e-2]])

    def go_wc(self, x, knobs_w):
        return compressor_4controls(x, thresh=knobs_w[0], ratio=knobs_w[1], attackTime=knobs_w[2],
                                    releaseTime=knobs_w[3], sr=self.sr), x

    def go_device(self, x, knobs_nn, y_size=None):
        """Batched effect on the GPU (st_compressor_4c): x [B,L] and knobs_nn [B,4] in [-.5,.5] as device tensors ->
        y [B,y_size] (the last y_size samples, datasets.py:327-330).  No CPU fallback."""
        if x.device.type != "cuda":
            raise RuntimeError("Compressor_4c.go_device needs ROCm device tensors")
        return _device_effect("st_compressor_4c", self, x, _knobs_wc_device(self.knob_ranges, knobs_nn, x.device), y_size)


class LowPass(Effect):
    """audio.py:610-625: a third-order Butterworth low-pass with the cutoff (Hz) as its knob."""
    feed_fx = 2                                   # _lib.FX_LOWPASS

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.name = 'LowPass'
        self.knob_names = ['cutoff']
        self.knob_ranges = np.array([[10, 2000]])

    def go_wc(self, x, knobs_w, order=3):
        return lowpass(x, knobs_w[0], sr=self.sr, order=order), x

    def go_device(self, x, knobs_nn, y_size=None):
        """Batched effect on the GPU (st_lowpass): x [B,L] and knobs_nn [B,1] in [-.5,.5] as device tensors -> y [B,y_size]
        (the last y_size samples).  No CPU fallback."""
        if x.device.type != "cuda":
            raise RuntimeError("LowPass.go_device needs ROCm device tensors")
        return _device_effect("st_lowpass", self, x, _knobs_wc_device(self.knob_ranges, knobs_nn, x.device), y_size)


class Denoise(Effect):
    """audio.py:558-571: uniform noise of amplitude `strength` is added to the signal and the pair is swapped -- the clean signal is the target,
    the noisy one the input (is_inverse), so the model learns to remove noise by a tunable amount.  go / go_wc / go_device return
    (target, input) like every effect; here the input is NOT the x that came in."""
    feed_fx = 3                                   # _lib.FX_DENOISE
    makes_input = True

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.name = 'Denoise'
        self.knob_names = ['strength']
        self.knob_ranges = np.array([[0.0, 0.5]])
        self.is_inverse = True

    def go_wc(self, x, knobs_w):
        return x, x + (knobs_w[0] * (2 * np.random.random(x.shape[0]) - 1)).astype(x.dtype, copy=False)

    def go_device(self, x, knobs_nn, y_size=None, seed=None, first_window=0):
        """(y, x_noisy) on the GPU: y [B,y_size] = the last y_size samples of the clean x [B,L], x_noisy [B,L] = x plus the noise of
        st_denoise_input at strength knobs_wc(knobs_nn [B,1]), rows = windows first_window ... of the noise stream `seed` (None: drawn from
        numpy's global generator, so it follows np.random.seed of the run).  No CPU fallback."""
        import torch
        from . import _lib
        if x.device.type != "cuda":
            raise RuntimeError("Denoise.go_device needs ROCm device tensors")
        x = x.to(torch.float32).contiguous(); B, L = x.shape
        kw = _knobs_wc_device(self.knob_ranges, knobs_nn, x.device)
        seed = int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)
        xn = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().st_denoise_input(seed, int(first_window), _lib.ptr(x), _lib.ptr(kw), B, L, _lib.ptr(xn),
                                                    C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)), "st_denoise_input")
        return x[:, L - (L if y_size is None else int(y_size)):].contiguous(), xn


class Echo(Effect):
    """audio.py:539-547: echoes of the signal -- delay in samples, attenuation ratio per echo and the number of echoes (a switch: it is rounded, and
    so is the delay).  Its signal families are the reference's set "for echo" (datasets.py:320)."""
    feed_fx = 4                                   # _lib.FX_ECHO
    feed_choosers = (1, 3, 5, 6, 7)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.name = 'Echo'
        self.knob_names = ['delay_samples', 'ratio', 'echoes']
        self.knob_ranges = np.array([[400, 400], [0.4, 1.0], [2, 2]])

    def go_wc(self, x, knobs_w):
        return echo(x, delay_samples=int(np.round(knobs_w[0])), ratio=knobs_w[1], echoes=int(np.round(knobs_w[2]))), x

    def go_device(self, x, knobs_nn, y_size=None):
        """Batched effect on the GPU (st_echo): x [B,L] and knobs_nn [B,3] in [-.5,.5] as device tensors -> y [B,y_size] (the last y_size
        samples); the delay and the echo count are rounded (half to even) as go_wc rounds them.  No CPU fallback."""
        if x.device.type != "cuda":
            raise RuntimeError("Echo.go_device needs ROCm device tensors")
        kw = _knobs_wc_device(self.knob_ranges, knobs_nn, x.device)
        kw[:, 0] = kw[:, 0].round(); kw[:, 2] = kw[:, 2].round()
        return _device_effect("st_echo", self, x, kw, y_size)


class DeCompressor_4c(Effect):
    """audio.py:573-583: the inverse problem of Compressor_4c, with its knobs -- the compressed signal is the input and the clean one the target
    (is_inverse).  go / go_wc / go_device return (target, input) like every effect; the input is NOT the x that came in (makes_input)."""
    feed_fx = 5                                   # _lib.FX_DECOMP4C
    makes_input = True

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        sub_effect = Compressor_4c(**kwargs)
        self.name = 'DeCompressor_4c'
        self.knob_names = sub_effect.knob_names
        self.knob_ranges = sub_effect.knob_ranges
        self.is_inverse = True

    def go_wc(self, x, knobs_w):
        return x, compressor_4controls(x, thresh=knobs_w[0], ratio=knobs_w[1], attackTime=knobs_w[2], releaseTime=knobs_w[3], sr=self.sr)

    def go_device(self, x, knobs_nn, y_size=None, seed=None):
        """(y, x_compressed) on the GPU: y [B,y_size] = the last y_size samples of the clean x [B,L], x_compressed [B,L] = st_compressor_4c of the
        whole window at knobs_wc(knobs_nn [B,4]).  seed is what every makes_input effect is handed (Denoise's noise stream) and is not used.
        No CPU fallback."""
        if x.device.type != "cuda":
            raise RuntimeError("DeCompressor_4c.go_device needs ROCm device tensors")
        B, L = x.shape
        xc = _device_effect("st_compressor_4c", self, x, _knobs_wc_device(self.knob_ranges, knobs_nn, x.device), L)
        return x[:, L - (L if y_size is None else int(y_size)):].to(xc.dtype).contiguous(), xc


class Compressor_4c_Large(Compressor_4c):
    """audio.py:503-510."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.name = 'Compressor_4c_Large'
        self.knob_ranges = np.array([[-50, 0], [1.5, 10], [1e-3, 1], [1e-3, 1]])


class Comp_Just_Thresh(Effect):
    """audio.py:513-526: compressor_4controls with the threshold as its only knob; ratio 3, attack 50 ms, release 1 s fixed (the reference's
    comparison effect for the LA2A)."""
    feed_fx = 0                                   # _lib.FX_COMP4C with K = 1

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.name = 'Comp_Just_Thresh'
        self.knob_names = ['threshold']
        self.knob_ranges = np.array([[-50, -10]])
        self.ratio, self.attack, self.release = 3.0, .05, 1.0

    def feed_ranges(self):
        fixed = [self.ratio, self.attack, self.release]
        return np.array([list(self.knob_ranges[0])] + [[v, v] for v in fixed], dtype=np.float64)

    def go_wc(self, x, knobs_w):
        return compressor_4controls(x, thresh=knobs_w[0], ratio=self.ratio, attackTime=self.attack, releaseTime=self.release, sr=self.sr), x

    def go_device(self, x, knobs_nn, y_size=None):
        """st_compressor_4c with world knobs (threshold, 3, 0.05, 1): x [B,L], knobs_nn [B,1] device tensors -> y [B,y_size]."""
        import torch
        if x.device.type != "cuda":
            raise RuntimeError("Comp_Just_Thresh.go_device needs ROCm device tensors")
        thr = _knobs_wc_device(self.knob_ranges, knobs_nn, x.device)
        fixed = torch.tensor([self.ratio, self.attack, self.release], dtype=torch.float32, device=x.device).expand(thr.shape[0], 3)
        return _device_effect("st_compressor_4c", self, x, torch.cat([thr, fixed], 1), y_size)


class Compressor_4c_OneSetting(Compressor_4c):
    """audio.py:529-536: compressor_4controls locked in one setting (degenerate ranges; the threshold's is written high to low)."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.name = 'Compressor_4c_OneSetting'
        self.knob_ranges = np.array([[-25.001, -25.], [4, 4.001], [5e-3, 5.001e-3], [2e-2, 2.001e-2]])


def int2knobs(idx, knob_ranges, settings_per):
    """audio.py:677-712: setting `idx` of the grid of `settings_per` equally spaced values per knob, as world-coordinate floats.  The knobs are the
    digits of idx in base settings_per, the LAST knob varying fastest, and digit d of knob k stands for lo_k + (hi_k - lo_k) / (settings_per - 1) * d.
      int2knobs(12345, [[-.5, .5]] * 4, 12) -> [0.13636..., -0.40909..., 0.22727..., 0.31818...]
      int2knobs(100, [[1, 6]] * 3, 6) -> [3.0, 5.0, 5.0]        int2knobs(1234, [[0, 9]] * 4, 10) -> [1.0, 2.0, 3.0, 4.0]"""
    sp, nk, idx = int(settings_per), len(knob_ranges), int(idx)
    assert idx < sp ** nk, f"idx ({idx}) must be less than the number of grid points ({sp ** nk})"
    digits = []
    for _ in range(nk):
        idx, d = divmod(idx, sp)
        digits.append(d)
    return [float(r[0] + (r[1] - r[0]) / (sp - 1) * d) for r, d in zip(knob_ranges, reversed(digits))]


# ------------------------------------------------------------------------------------------------ wav files + file-defined effects
def mu_compand(y, mu=32):
    """audio.py:339-340: mu-law companding (run_train.py --compand, datasets.py:218-220, utils/predict_long.py:38-40)."""
    return np.sign(y) * np.log(1 + mu * np.abs(y)) / np.log(1 + mu)


def mu_decompand(y, mu=32):
    """audio.py:343-344."""
    return np.sign(y) / mu * ((1 + mu) ** np.abs(y) - 1)


def read_audio_file(filename, sr=44100, mono=True, norm=False, dtype=np.float32, info=None, **_ignored):
    """audio.py:207-255: a wav file as float in [-1, 1] (int16 / 32767), first channel if `mono`.  A file at another sample rate is resampled to
    `sr` with a polyphase filter (scipy.signal.resample_poly; the reference calls librosa.resample there -- another low-pass design, so such
    files agree with the reference's to the filters' pass-band ripple, not bit for bit).  info: an optional dict that receives what the
    returned samples are -- "int16" (the file holds 16-bit PCM) and "exact" (they are still s / 32767 of it: neither resampled nor normalised)."""
    from scipy.io import wavfile
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        read_sr, signal = wavfile.read(filename)
    if mono and signal.ndim > 1:
        signal = signal[:, 0]
    was_int16 = signal.dtype == np.int16
    if info is not None:
        info["int16"], info["exact"] = bool(was_int16), bool(was_int16 and read_sr == int(sr) and not norm)
    if was_int16:
        signal = np.array(signal / 32767.0, dtype=dtype)
    signal = signal.astype(dtype, copy=False)
    if read_sr != int(sr):
        from math import gcd
        from scipy.signal import resample_poly
        g = gcd(int(sr), int(read_sr))
        print(f"read_audio_file: {filename}: resampling {read_sr} Hz -> {int(sr)} Hz")
        signal = resample_poly(signal.astype(np.float64), int(sr) // g, int(read_sr) // g, axis=0).astype(dtype)
    if norm:
        m = np.max(np.abs(signal))
        signal = signal / m if m > 0 else signal
    return signal, sr


def write_audio_file(filename, data, sr=44100):
    """audio.py:258-262."""
    from scipy.io import wavfile
    wavfile.write(filename, sr, data)


class FileEffect(Effect):
    """audio.py:624-670: an effect that exists only as recordings -- <path>/Train, <path>/Val with input_* / target_* pairs and
    <path>/effect_info.ini ([effect] name, knob_names, knob_ranges [, inverse]); e.g. the LA2A of BASELINE configs[3]."""

    def __init__(self, path, sr=44100):
        super().__init__(sr=sr)
        import ast
        import configparser
        import glob
        if path is None or not glob.glob(path + "/Train/target*") or not glob.glob(path + "/Val/target*") or not glob.glob(path + "/effect_info.ini"):
            raise FileNotFoundError(f"FileEffect: no Train/ + Val/ target files or effect_info.ini under {path}")
        cfg = configparser.ConfigParser(); cfg.read(path + "/effect_info.ini")
        self.name = cfg["effect"]["name"].strip("'\"") + "(files)"
        self.knob_names = list(ast.literal_eval(cfg.get("effect", "knob_names")))       # literal_eval instead of the reference's eval
        self.knob_ranges = np.array(ast.literal_eval(cfg.get("effect", "knob_ranges")), dtype=np.float64)
        if cfg["effect"].get("inverse"):
            self.is_inverse = True; self.name = "De-" + self.name

    def go_wc(self, x, knobs_w):
        return None                      # there is no plugin to call: the targets are recordings
