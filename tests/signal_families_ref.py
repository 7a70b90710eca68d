"""Restatement of the reference's test signals beyond the compressor's set (signaltrain/audio.py:149-196 and :296-334): families 3 (triangle +
1/f noise), 5 (spikes + normal noise), 8 (ampexpstepup from -30 dB), 9 (sweep), 10 (box + white + 1/f noise) and 11 (scaled 1/f noise).

Two forms.  `*_from(t, parameters...)` evaluates one generator from explicit parameters in the arithmetic `dtype` (float64: the reference's own;
float32: the same formula with every step rounded to float32 -- the yardstick of the GPU tests).  `synth_input_sample(t, chooser, rng)` draws
the parameters from numpy's legacy generator in the reference's order and so reproduces the reference for np.random.seed(s): golden G17
(tests/golden/g17_signal_families.npz, captured by tools/capture_golden_families.py) pins it.
t: the window's time values; the feed's are float32(n) / sr -- `time_values` -- and the float64 form takes them widened."""
import numpy as np

N_SPIKES = 50
FAMILIES = (3, 5, 8, 9, 10, 11)


def time_values(L, sr=44100.0):
    return (np.arange(L, dtype=np.float32) / np.float32(sr)).astype(np.float64)


def normish(y, u, dtype=np.float64):
    """audio.py:75-81 with the draw u"""
    f = dtype
    return y / np.max(np.abs(y)) * ((f(0.9) - f(0.6)) * f(u) + f(0.6))


def pinknoise_from(spec_u):
    """audio.py:85-94 from the N // 2 + 1 uniform draws of its spectrum"""
    noise = 2 * np.asarray(spec_u, dtype=np.float64) - 1
    s = np.sqrt(np.arange(len(noise)) + 1.)
    y = (np.fft.irfft(noise / s)).real
    return y / np.max(np.abs(y))


def triangle_from(t, height, width, t0, dtype=np.float64):
    """audio.py:188-194 without its noise"""
    f = dtype
    t, height, width, t0 = np.asarray(t).astype(f), f(height), f(width), f(t0)
    x = height * (f(1) - np.abs(t - t0) / width)
    x[np.where(t < (t0 - width))] = 0
    x[np.where(t > (t0 + width))] = 0
    return x


def spike_loc(u, n, t_last):
    """audio.py:178: int(int(u n - 2) + t[-1]) -- two truncations toward zero"""
    return int(int(u * n - 2) + 1 * t_last)


def spikes_from(n, loc, height, dtype=np.float64):
    """audio.py:176-182 without the noise: the spikes written in order, later ones over earlier ones; negative indices wrap as numpy's do"""
    x = np.zeros(n, dtype=dtype)
    for l, h in zip(loc, height):
        h = dtype(h)
        x[l] = h
        x[(l + 1) % n] = h / 2
        x[l - 1] = h / 2
    return x


def normal_from(u1, u2, dtype=np.float64):
    """Box-Muller as the feed forms it: sqrt(-2 ln(1 - u1)) cos(2 pi u2)"""
    f = dtype
    u1, u2 = np.asarray(u1).astype(f), np.asarray(u2).astype(f)
    return np.sqrt(f(-2) * np.log(f(1) - u1)) * np.cos(f(2 * np.pi) * u2)


def env_dB(n, start_dB=-30):
    return np.floor(np.linspace(start_dB, 0, num=n))


def step_from(t, freq, start_dB=-30, dtype=np.float64):
    """audio.py:156-160 before normish: env = 10^(env_dB / 10) (sic)"""
    f = dtype
    t = np.asarray(t).astype(f)
    env = np.power(f(10.0), env_dB(len(t), start_dB).astype(f) / f(10))
    return env * np.sin(f(freq) * t)


def sweep_from(t, f_low, f_high, amp, amp_too, dtype=np.float64):
    """audio.py:167-172 before normish: the constant in front is 20 whatever f_low is"""
    f = dtype
    t = np.asarray(t).astype(f)
    tmax = t[-1]
    lnfr = f(np.log(int(f_high) / int(f_low)))
    y = f(amp) * np.sin(f(20) * f(2) * f(np.pi) * tmax / lnfr * (np.exp(t / tmax * lnfr) - f(1)))
    if amp_too:
        y = y * np.exp(lnfr * t / tmax)
    return y


def box_from(t, h_bgn, h_mid, h_end, u_up, u_dn):
    """audio.py:106-122 with delta = 0"""
    maxi = len(t)
    i_up = int(0.3 * u_up * maxi)
    i_dn = min(i_up + int((0.3 + 0.35 * u_dn) * maxi), maxi - 1)
    x = h_end * np.ones(t.shape[0]).astype(t.dtype, copy=False)
    x[0:i_up - 1] = h_bgn
    x[i_up:i_dn] = h_mid
    return x


def synth_input_sample(t, chooser, rng):
    """audio.synth_input_sample(t, chooser) for families 3, 5, 8, 9, 10, 11 with its draws taken from `rng` (np.random.RandomState) in the
    reference's order.  Returns (y, parts): parts holds the drawn parameters and noise arrays."""
    t = np.asarray(t, dtype=np.float64)
    n, tl = t.shape[0], t[-1]
    p = {}

    def pink():
        p["spec_u"] = rng.random_sample(n // 2 + 1)
        return pinknoise_from(p["spec_u"])
    if chooser == 3:
        p["height"] = (0.4 * rng.rand() + 0.4) * rng.choice([-1, 1])
        p["width"] = rng.rand() / 4 * tl
        p["t0"] = 2 * p["width"] + 0.4 * rng.rand() * tl
        x = triangle_from(t, p["height"], p["width"], p["t0"])
        p["amp_n"] = 0.1 * rng.rand() + 0.02
        y = x + p["amp_n"] * pink()
    elif chooser == 5:
        p["loc"], p["spike_height"] = [], []
        for _ in range(N_SPIKES):
            p["loc"].append(spike_loc(rng.rand(), n, tl))
            p["spike_height"].append((2 * rng.rand() - 1) * 0.7)
        x = spikes_from(n, p["loc"], p["spike_height"])
        p["amp_n"] = 0.1 * rng.rand()
        p["normal"] = rng.normal(size=n)
        y = x + p["amp_n"] * p["normal"]
    elif chooser == 8:
        p["freq"] = 400 + (5000 - 400) * rng.rand()
        y = normish(step_from(t, p["freq"]), rng.rand())
    elif chooser == 9:
        p["f_low"], p["f_high"] = rng.randint(20, 1000), rng.randint(1000, 20000)
        p["amp_too"] = bool(rng.choice([False, False, True]))
        p["amp"] = 0.9 * rng.rand()
        y = normish(sweep_from(t, p["f_low"], p["f_high"], p["amp"], p["amp_too"]), rng.rand())
    elif chooser == 10:
        h = (0.15 * rng.rand(), 0.35 * rng.rand() + 0.6, 0.2 * rng.rand() + 0.1)
        bx = box_from(t, *h, rng.rand(), rng.rand())
        p["amp_w"] = 0.2 * rng.rand()
        p["white"] = 2 * rng.rand(n) - 1
        white = p["amp_w"] * p["white"]
        p["amp_n"] = 0.2 * rng.rand()
        y = bx + white + p["amp_n"] * pink()
    elif chooser == 11:
        p["amp_n"] = 0.6 * rng.rand() + 0.2
        y = p["amp_n"] * pink()
    else:
        raise ValueError(f"signal_families_ref restates families {FAMILIES}, not {chooser}")
    p["polarity"] = rng.choice([-1, 1])
    return y * p["polarity"] + rng.rand(len(y)) * 1e-8, p
