#!/usr/bin/env python3
"""Golden G18 from the *imported reference* (build container only): the Echo and DeCompressor_4c effects.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_echo.py
Writes (small, committed):

  tests/golden/g18_echo_decomp.npz
        x [4, 4096] float32: the windows `signals` = white noise, an impulse at 0, a box, a 30 Hz sine.
        audio.echo(x[s], delay_samples=d, ratio=r, echoes=e) (audio.py:430-443) for every window and every (d, r, e) of the grid
        delays [9] x ratios [4] x echoes [5] (Python floats / ints, as Effect.knobs_wc hands them over):
          echo_sha256 [4, 9, 4, 5, 32] uint8   SHA-256 of the float32 result's bytes -- the whole grid, 720 results of 16 KB each, bit for bit;
          echo_y_ib   [2, 9, 4, 5, 4096]       the results themselves for the impulse and the box (they compress to almost nothing);
          echo_y_wn   [9, 4096]                ... and for the white noise at ratio float32(0.76), 3 echoes, every delay.
        Echo().go(x[0], knobs) at echo_knobs_nn [3, 3]: echo_go_y [3, 4096], echo_go_knobs_wc [3, 3] (float64, Effect.knobs_wc).
        DeCompressor_4c().go(x[s], knobs) at decomp_knobs_nn [3, 4] on windows decomp_sig [3]: decomp_go_input [3, 4096] (the second return
        value; the first is x itself), decomp_go_knobs_wc [3, 4].
        Both effects' name, knob_names, knob_ranges and is_inverse.
"""
import hashlib, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _ref_import import import_reference                       # noqa: E402

A = import_reference().audio
L, SR = 4096, 44100.0
rng = np.random.default_rng(18)
n = np.arange(L)
box = np.full(L, 0.1, dtype=np.float32); box[L // 5:L // 2] = 0.8; box[L // 2:] = 0.2
imp = np.zeros(L, dtype=np.float32); imp[0] = 1.0
X = np.stack([(2.0 * rng.random(L) - 1.0).astype(np.float32), imp, box, (0.7 * np.sin(2 * np.pi * 30.0 * n / SR)).astype(np.float32)])
SIGNALS = ["white", "impulse", "box", "sine30"]
DELAYS = [1, 1.5, 333.3, 400, 1487, 2047.5, L - 1, L, 5000.25]
RATIOS = [0.4, float(np.float32(0.76)), 1.0, -0.5]
ECHOES = [0, 1, 2, 3, 8]

sha = np.zeros((4, len(DELAYS), len(RATIOS), len(ECHOES), 32), dtype=np.uint8)
y_ib = np.zeros((2, len(DELAYS), len(RATIOS), len(ECHOES), L), dtype=np.float32)
y_wn = np.zeros((len(DELAYS), L), dtype=np.float32)
for s in range(4):
    for i, d in enumerate(DELAYS):
        for j, r in enumerate(RATIOS):
            for k, e in enumerate(ECHOES):
                y = A.echo(X[s], delay_samples=d, ratio=r, echoes=e)
                assert y.dtype == np.float32 and y.shape == (L,)
                sha[s, i, j, k] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(y).tobytes()).digest(), dtype=np.uint8)
                if s in (1, 2):
                    y_ib[s - 1, i, j, k] = y
                if s == 0 and j == 1 and e == 3:
                    y_wn[i] = y

fx = A.Echo()
echo_kn = np.array([[-0.5, -0.5, -0.5], [0.1, 0.1, 0.2], [0.5, 0.5, 0.5]])
echo_go = np.stack([fx.go(X[0], kn)[0] for kn in echo_kn])
assert echo_go.dtype == np.float32
echo_kw = np.array([fx.knobs_wc(kn) for kn in echo_kn], dtype=np.float64)

dc = A.DeCompressor_4c()
dc_kn = np.array([[-0.5, 0.5, -0.5, 0.5], [0.0, 0.1, -0.2, 0.3], [-0.3, 0.5, 0.5, -0.5]])
dc_sig = np.array([0, 3, 2])
pairs = [dc.go(X[s], kn) for s, kn in zip(dc_sig, dc_kn)]
assert all(p[0] is X[s] or np.array_equal(p[0], X[s]) for p, s in zip(pairs, dc_sig))
dc_in = np.stack([p[1] for p in pairs]).astype(np.float32)
dc_kw = np.array([dc.knobs_wc(kn) for kn in dc_kn], dtype=np.float64)

path = os.path.join(OUT, "g18_echo_decomp.npz")
np.savez_compressed(
    path, x=X, signals=np.array(SIGNALS), delays=np.array(DELAYS, dtype=np.float64), ratios=np.array(RATIOS, dtype=np.float64), echoes=np.array(ECHOES),
    echo_sha256=sha, echo_y_ib=y_ib, echo_y_wn=y_wn, sr=np.float64(SR),
    echo_knobs_nn=echo_kn, echo_go_y=echo_go, echo_go_knobs_wc=echo_kw,
    decomp_knobs_nn=dc_kn, decomp_sig=dc_sig, decomp_go_input=dc_in, decomp_go_knobs_wc=dc_kw,
    echo_name=np.array(fx.name), echo_knob_names=np.array(fx.knob_names), echo_knob_ranges=np.asarray(fx.knob_ranges, dtype=np.float64), echo_is_inverse=np.array(bool(fx.is_inverse)),
    decomp_name=np.array(dc.name), decomp_knob_names=np.array(dc.knob_names), decomp_knob_ranges=np.asarray(dc.knob_ranges, dtype=np.float64),
    decomp_is_inverse=np.array(bool(dc.is_inverse)))
print(f"{path}: {os.path.getsize(path)} bytes")
