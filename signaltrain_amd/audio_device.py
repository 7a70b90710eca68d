"""Device-side synthetic test signals for the comp_4c task -- SURVEY.md 8(f)-1, the rest of the GPU data feed.

signaltrain/audio.py:85-196 and :296-334 (`synth_input_sample` and the generators it calls: all twelve signal families; the default
set is the compressor's, {0, 1, 2, 4, 6, 7}, datasets.py:317, whose draw sequence is what it always was) restated as BATCHED device computations: every window of a minibatch draws its own
chooser, tone count, amplitudes, frequencies, onsets ... from a device `torch.Generator` (no host RNG, no host loop), the
waveforms are evaluated elementwise over [B, L] and normalised per window exactly as `normish` / `pinknoise` do.  The 1/f noise
keeps the reference's construction -- an inverse real FFT of a REAL spectrum `(2 u - 1) / sqrt(k + 1)` (so it is an even
sequence, like the reference's) -- through `torch.fft.irfft` (rocFFT): the feed is not the hot path (SURVEY.md 8, rows
"next"), the one sequential, expensive part of it -- the compressor -- is the hand-written HIP kernel `st_compressor_4c`.

Parity is distributional (the draws come from a different generator than numpy's): tests compare amplitude ranges, onset
statistics and spectra with the host generators of signaltrain_amd/audio.py; the effect itself is pinned by golden G9.
"""
import math

import torch

COMPRESSOR_CHOOSERS = (0, 1, 2, 4, 6, 7)        # datasets.py:317


def _u(gen, *shape, device):
    return torch.rand(*shape, generator=gen, device=device, dtype=torch.float32)


def _sign(gen, *shape, device):
    return torch.where(_u(gen, *shape, device=device) < 0.5, -1.0, 1.0)


def _normish(y, gen, lo=0.6, hi=0.9):
    """audio.py:78-81: y / max|y| * U(lo, hi), per window."""
    B = y.shape[0]
    peak = y.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)
    return y / peak * ((hi - lo) * _u(gen, B, 1, device=y.device) + lo)


def pinknoise(B, N, gen, device):
    """audio.py:85-94: irfft of a real spectrum (2u-1)/sqrt(k+1), k = 0..N/2, normalised to unit peak."""
    nf = N // 2 + 1
    spec = (2.0 * _u(gen, B, nf, device=device) - 1.0) / torch.sqrt(torch.arange(nf, device=device, dtype=torch.float32) + 1.0)
    y = torch.fft.irfft(spec.to(torch.complex64), n=N, dim=1)
    return y / y.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)


def randsine(t, B, gen, amp_range=(0.2, 0.9), freq_range=(5.0, 150.0)):
    """audio.py:96-104: one or two cosines with random amplitude / frequency / onset, then normish."""
    dev, tl = t.device, float(t[-1])
    n_tones = torch.randint(1, 3, (B, 1), generator=gen, device=dev)
    y = torch.zeros(B, t.shape[0], device=dev)
    for i in range(2):
        amp = amp_range[0] + (amp_range[1] - amp_range[0]) * _u(gen, B, 1, device=dev)
        freq = freq_range[0] + (freq_range[1] - freq_range[0]) * _u(gen, B, 1, device=dev)
        t0 = _u(gen, B, 1, device=dev) * tl
        y = y + torch.where(n_tones > i, amp, torch.zeros_like(amp)) * torch.cos(freq * (t[None, :] - t0))
    return _normish(y, gen)


def box(t, B, gen):
    """audio.py:106-124 with delta = 0: three plateaus; sample i_up - 1 keeps the end height (the reference's slice bounds)."""
    dev, n = t.device, t.shape[0]
    h0, h1, h2 = 0.15 * _u(gen, B, 1, device=dev), 0.35 * _u(gen, B, 1, device=dev) + 0.6, 0.2 * _u(gen, B, 1, device=dev) + 0.1
    i_up = (0.3 * _u(gen, B, 1, device=dev) * n).floor()
    i_dn = torch.minimum(i_up + ((0.3 + 0.35 * _u(gen, B, 1, device=dev)) * n).floor(), torch.full_like(i_up, n - 1))
    i = torch.arange(n, device=dev, dtype=torch.float32)[None, :]
    x = h2.expand(B, n).clone()
    x = torch.where(i < i_up - 1, h0, x)
    x = torch.where((i >= i_up) & (i < i_dn), h1, x)
    return x


def expdecay(t, B, gen):
    """audio.py:126-136: plateau, then an exponential decay from a random onset."""
    dev, tl = t.device, float(t[-1])
    t0 = 0.35 * _u(gen, B, 1, device=dev) * tl
    hi, lo = 0.35 * _u(gen, B, 1, device=dev) + 0.6, 0.1 * _u(gen, B, 1, device=dev) + 0.1
    decay = 12.0 * _u(gen, B, 1, device=dev)
    tt = t[None, :]
    return torch.where(tt < t0, lo, torch.exp(-decay * (tt - t0)) * hi)


def pluck(t, B, gen, freq_range=(50.0, 6400.0)):
    """audio.py:138-148: one to three sines with random sign / phase under an exponential decay, then normish."""
    dev, tl = t.device, float(t[-1])
    n_tones = torch.randint(1, 4, (B, 1), generator=gen, device=dev)
    y = torch.zeros(B, t.shape[0], device=dev)
    for i in range(3):
        amp0 = (0.45 * _u(gen, B, 1, device=dev) + 0.5) * _sign(gen, B, 1, device=dev)
        t0 = (2.0 * _u(gen, B, 1, device=dev) - 1.0) * 0.3 * tl
        freq = freq_range[0] + (freq_range[1] - freq_range[0]) * _u(gen, B, 1, device=dev)
        y = y + torch.where(n_tones > i, amp0, torch.zeros_like(amp0)) * torch.sin(freq * (t[None, :] - t0))
    return _normish(y * expdecay(t, B, gen), gen)


def triangle(t, B, gen, pink):
    """audio.py:188-196: ramp up, then down, zero outside, plus 1/f noise; not normalised."""
    dev, tl = t.device, float(t[-1])
    height = (0.4 * _u(gen, B, 1, device=dev) + 0.4) * _sign(gen, B, 1, device=dev)
    width = _u(gen, B, 1, device=dev) / 4 * tl
    t0 = 2 * width + 0.4 * _u(gen, B, 1, device=dev) * tl
    tt = t[None, :]
    x = height * (1 - (tt - t0).abs() / width.clamp_min(1e-30))
    x = torch.where((tt < t0 - width) | (tt > t0 + width), torch.zeros_like(x), x)
    return x + (0.1 * _u(gen, B, 1, device=dev) + 0.02) * pink


def spikes(t, B, gen, n_spikes=50):
    """audio.py:175-186: fifty three-sample spikes, each written over what is there (index int(int(u n - 2) + t[-1]), -1 wraps), plus normal noise."""
    dev, n, tl = t.device, t.shape[0], float(t[-1])
    x = torch.zeros(B, n, device=dev)
    for _ in range(n_spikes):
        loc = torch.trunc(torch.trunc(_u(gen, B, 1, device=dev).double() * n - 2) + tl).long()
        h = (2 * _u(gen, B, 1, device=dev) - 1) * 0.7
        x.scatter_(1, loc % n, h); x.scatter_(1, (loc + 1) % n, h / 2); x.scatter_(1, (loc - 1) % n, h / 2)
    return x + 0.1 * _u(gen, B, 1, device=dev) * torch.randn(B, n, generator=gen, device=dev)


def ampexpstepup(t, B, gen, start_dB=-30, freq_range=(400.0, 5000.0)):
    """audio.py:149-161: a tone under an envelope that rises in integer dB steps (env = 10^(dB / 10), as the reference has it), then normish."""
    dev, n = t.device, t.shape[0]
    i = torch.arange(n, device=dev, dtype=torch.int64)
    env_dB = start_dB + torch.div(-start_dB * i, max(n - 1, 1), rounding_mode="floor")      # == floor(linspace(start_dB, 0, n))
    freq = freq_range[0] + (freq_range[1] - freq_range[0]) * _u(gen, B, 1, device=dev)
    y = torch.pow(10.0, env_dB.double() / 10)[None, :] * torch.sin(freq.double() * t.double()[None, :])
    return _normish(y.float(), gen)


def sweep(t, B, gen):
    """audio.py:164-173 with the draws of :323-325: exponential sweep f_low -> f_high (the constant in front is 20, not f_low), for one window
    in three with the amplitude rising too, then normish."""
    dev, tl = t.device, float(t[-1])
    f_low = torch.randint(20, 1000, (B, 1), generator=gen, device=dev).double()
    f_high = torch.randint(1000, 20000, (B, 1), generator=gen, device=dev).double()
    amp_too = torch.randint(0, 3, (B, 1), generator=gen, device=dev) == 2
    lnfr = torch.log(f_high / f_low)
    amp = 0.9 * _u(gen, B, 1, device=dev).double()
    g = torch.exp(t.double()[None, :] / tl * lnfr)
    y = amp * torch.sin(20 * 2 * math.pi * tl / lnfr * (g - 1))
    return _normish(torch.where(amp_too, y * g, y).float(), gen)


EXTENDED_CHOOSERS = (3, 5, 8, 9, 10, 11)


def synth_input_batch(B, chunk_size, sr, gen, device, choosers=COMPRESSOR_CHOOSERS, chooser=None):
    """B windows of audio.synth_input_sample (audio.py:296-334): x [B, chunk_size] float32 on `device`, and the chooser drawn
    for each window, uniformly over `choosers` (families 0..11; the superposition is not built).  chooser: force one signal family
    for every window (tests).  The families beyond the compressor's set draw only when one of them can come out."""
    asked = tuple(choosers) if chooser is None else (int(chooser),)
    if not asked or any(int(k) != k or not 0 <= k <= 11 for k in asked):
        raise NotImplementedError(f"audio_device.synth_input_batch: signal families are 0..11 (the superposition, 12 and up, is not built), not {asked}")
    t = torch.arange(chunk_size, device=device, dtype=torch.float32) / float(sr)
    n = chunk_size
    if chooser is None:
        pick = torch.tensor(choosers, device=device)[torch.randint(0, len(choosers), (B,), generator=gen, device=device)]
    else:
        pick = torch.full((B,), int(chooser), device=device)
    c = pick[:, None]
    sine, plk, bx = randsine(t, B, gen), pluck(t, B, gen), box(t, B, gen)
    pink = pinknoise(B, n, gen, device)
    white = 2.0 * _u(gen, B, n, device=device) - 1.0
    y = torch.where(c == 0, sine, torch.zeros_like(sine))
    y = torch.where(c == 1, sine + 0.2 * _u(gen, B, 1, device=device) * pink + 0.2 * _u(gen, B, 1, device=device) * white, y)
    y = torch.where(c == 2, plk, y)
    y = torch.where(c == 4, bx, y)
    y = torch.where(c == 6, bx * white, y)
    y = torch.where(c == 7, plk + (0.3 * _u(gen, B, 1, device=device) + 0.1) * pink, y)
    if any(k in EXTENDED_CHOOSERS for k in asked):
        y = torch.where(c == 3, triangle(t, B, gen, pink), y)
        y = torch.where(c == 5, spikes(t, B, gen), y)
        y = torch.where(c == 8, ampexpstepup(t, B, gen), y)
        y = torch.where(c == 9, sweep(t, B, gen), y)
        y = torch.where(c == 10, bx + 0.2 * _u(gen, B, 1, device=device) * white + 0.2 * _u(gen, B, 1, device=device) * pink, y)
        y = torch.where(c == 11, (0.6 * _u(gen, B, 1, device=device) + 0.2) * pink, y)
    # audio.py:333: random polarity + 1e-8 of uniform noise (keeps log10 away from exact zeros downstream)
    return y * _sign(gen, B, 1, device=device) + _u(gen, B, n, device=device) * 1e-8, pick


def random_ends(B, K, gen, device):
    """audio.py:20-21: Beta(0.8, 0.8) -- emphasises the ends of the knob range -- as a ratio of Gamma draws."""
    conc = torch.full((B, K), 0.8, device=device)
    # torch has no generator-aware Beta: Gamma(a) by Marsaglia-Tsang on a + 1 with the u^(1/a) boost, from this generator's draws
    def gamma(a):
        d = a + 1.0 - 1.0 / 3.0
        cc = 1.0 / torch.sqrt(9.0 * d)
        out = torch.zeros_like(a); todo = torch.ones_like(a, dtype=torch.bool)
        for _ in range(16):
            z = torch.randn(a.shape, generator=gen, device=device)
            v = (1.0 + cc * z) ** 3
            u = _u(gen, *a.shape, device=device)
            ok = (v > 0) & (torch.log(u.clamp_min(1e-30)) < 0.5 * z * z + d - d * v + d * torch.log(v.clamp_min(1e-30)))
            take = todo & ok
            out = torch.where(take, d * v, out); todo = todo & ~take
            if not bool(todo.any()):
                break
        return out * _u(gen, *a.shape, device=device).clamp_min(1e-30) ** (1.0 / a)
    x, y = gamma(conc), gamma(conc)
    return x / (x + y)
