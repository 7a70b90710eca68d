#!/usr/bin/env python3
"""Golden G17 from the *imported reference* (build container only): the signal families the compressor's set leaves out.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_families.py
Writes (small, committed):

  tests/golden/g17_signal_families.npz   audio.synth_input_sample(t, chooser=c) (audio.py:296-334) for c in families = [3, 5, 8, 9, 10, 11] after
        np.random.seed(s), s in seeds = [17, 1717]:  y [2, 6, 1024] float32 (the reference's float64 output, rounded once for storage), and t_f32 [1024],
        the time values float32(n) / 44100.  The reference receives them WIDENED to float64, so its arithmetic is float64 under either numpy
        promotion rule (with a float32 t, numpy 1.x and 2.x promote `python float * float32 array` differently).
tests/signal_families_ref.py restates these families and must reproduce y from np.random.RandomState(s).
"""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _ref_import import import_reference                       # noqa: E402

A = import_reference().audio
L, SR = 1024, 44100.0
FAMILIES, SEEDS = [3, 5, 8, 9, 10, 11], [17, 1717]
t32 = np.arange(L, dtype=np.float32) / np.float32(SR)
t = t32.astype(np.float64)

Y = np.zeros((len(SEEDS), len(FAMILIES), L), dtype=np.float32)
for i, s in enumerate(SEEDS):
    for j, c in enumerate(FAMILIES):
        np.random.seed(s)
        y = A.synth_input_sample(t, chooser=c)
        assert y.dtype == np.float64 and y.shape == (L,) and np.isfinite(y).all()
        Y[i, j] = y.astype(np.float32)
path = os.path.join(OUT, "g17_signal_families.npz")
np.savez_compressed(path, y=Y, t_f32=t32, families=np.array(FAMILIES), seeds=np.array(SEEDS), sr=np.float64(SR))
print(f"{path}: {os.path.getsize(path)} bytes")
