#!/usr/bin/env python3
"""Round-7 golden vectors from the *imported reference* (build container only); complements capture_golden{,_r2,...,_r6}.py.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_r7.py
Writes (small, committed):

  tests/golden/g15_compressor_family.npz   the three compressor effects of the reference's run_train.py keys comp / comp_t / comp_one:
        comp_x [6, 8192] float32, comp_kn [6, 3] (normalised knobs), comp_kw [6, 3] (the reference's knobs_wc of them), comp_y [6, 8192] float64:
            Compressor().go(x, knobs) (audio.py:349-371, :484-491) -- the reference's float64 output.  Windows: attack / release at both ends of
            the range (1 ms, 40 ms), ratio 1 (identity curve), threshold 0 dB on a window peaking above 1, a window that starts in digital silence
            (d[0] = -120 dB) and a mid-range setting.
        thresh_idx [2], thresh_kn [2, 1], thresh_y [2, 8192]: Comp_Just_Thresh().go on comp_x[thresh_idx] (audio.py:513-526);
        one_idx [2], one_kn [2, 4], one_y [2, 8192]: Compressor_4c_OneSetting().go on comp_x[one_idx] (audio.py:529-536);
        <prefix>_name, <prefix>_knob_names, <prefix>_knob_ranges for prefixes comp / thresh / one: the metadata checkpoints carry.
The reference's compressor_4controls runs with numba's @jit stubbed to the identity (tools/_ref_import.py), as for golden G9.
"""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _ref_import import import_reference                       # noqa: E402

A = import_reference().audio
L, SR = 8192, 44100.0
rng = np.random.default_rng(15)
t = np.arange(L) / SR


def bursts(levels, f0):
    """a tone whose level steps through `levels` (equal parts of the window), plus a little noise"""
    lev = np.repeat(np.asarray(levels, dtype=np.float64), -(-L // len(levels)))[:L]
    return lev * np.sin(2 * np.pi * f0 * t) + 0.01 * rng.standard_normal(L)


X = np.stack([
    bursts([0.05, 0.9, 0.1, 0.7], 220.0),          # 0: attack / release 1 ms
    bursts([0.8, 0.05, 0.6, 0.02], 330.0),         # 1: 40 ms
    bursts([0.3, 0.9, 0.05, 0.5], 440.0),          # 2: ratio 1
    bursts([0.4, 3.0, 0.7, 2.0], 150.0),           # 3: threshold 0 dB, peak above 1 (the envelope crosses it)
    bursts([0.0, 0.8, 0.3, 0.9], 500.0),           # 4: digital silence first (zeroed below)
    bursts([0.2, 0.6, 0.9, 0.1], 275.0),           # 5: mid-range
]).astype(np.float32)
X[4, :L // 4] = 0.0
assert np.abs(X[3]).max() > 1.0
KN = np.array([[0.1, 0.3, -0.5],                   # (threshold, ratio, attack / release) in [-0.5, 0.5]
               [0.2, -0.1, 0.5],
               [-0.2, -0.5, -0.2],
               [0.5, 0.25, 0.0],
               [-0.1, 0.4, -0.3],
               [0.0, 0.0, 0.0]])

fx = A.Compressor()
KW = np.array([fx.knobs_wc(k) for k in KN])
assert np.isclose(KW[0, 2], 1e-3) and np.isclose(KW[1, 2], 4e-2) and KW[2, 1] == 1.0 and KW[3, 0] == 0.0
Y = np.stack([np.asarray(fx.go(X[i], KN[i])[0], dtype=np.float64) for i in range(len(X))])
assert not np.array_equal(Y[3], X[3].astype(np.float64))
assert np.abs(Y[4, :L // 4]).max() == 0.0 and not np.array_equal(Y[0], X[0].astype(np.float64))

ft, fo = A.Comp_Just_Thresh(), A.Compressor_4c_OneSetting()
T_IDX, T_KN = np.array([0, 5]), np.array([[-0.3], [0.4]], dtype=np.float32)
O_IDX, O_KN = np.array([1, 3]), np.array([[0.2, -0.4, 0.1, 0.5], [-0.5, 0.3, -0.2, 0.0]], dtype=np.float32)
TY = np.stack([np.asarray(ft.go(X[i], k)[0], dtype=np.float64) for i, k in zip(T_IDX, T_KN)])
OY = np.stack([np.asarray(fo.go(X[i], k)[0], dtype=np.float64) for i, k in zip(O_IDX, O_KN)])

meta = {}
for pre, e in (("comp", fx), ("thresh", ft), ("one", fo)):
    meta[pre + "_name"] = np.array(e.name)
    meta[pre + "_knob_names"] = np.array(e.knob_names)
    meta[pre + "_knob_ranges"] = np.asarray(e.knob_ranges, dtype=np.float64)
path = os.path.join(OUT, "g15_compressor_family.npz")
np.savez_compressed(path, comp_x=X, comp_kn=KN, comp_kw=KW, comp_y=Y, thresh_idx=T_IDX, thresh_kn=T_KN, thresh_y=TY,
                    one_idx=O_IDX, one_kn=O_KN, one_y=OY, sr=np.float64(SR), **meta)
print(f"{path}: {os.path.getsize(path)} bytes")
