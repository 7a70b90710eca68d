#!/usr/bin/env python3
"""Generator time per signal family (the fused feed with a fixed chooser: the compressor's set, then families 3, 5, 8, 9, 10, 11), B windows of L samples: where the feed's GPU time goes; then the drawn
stream (chooser -1) of every effect with a fused feed -- the compressors, LowPass and Denoise -- per call and per 256-window minibatch.
    python tools/feed_family_times.py [L] [B]      (GPU box)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from signaltrain_amd import datasets, audio, _lib
L = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
B = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
lib = _lib.load()
ds = datasets.SynthAudioDataSet(L, audio.Compressor_4c(), datapoints=B, y_size=L // 4)
def timed(ds, ch):
    for _ in range(2): ds.batch_device(B, "cuda:0", chooser=ch)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10): ds.batch_device(B, "cuda:0", chooser=ch)
    e1.record(); torch.cuda.synchronize()
    return e0, e1
for ch in (-1, 0, 1, 2, 4, 6, 7, 3, 5, 8, 9, 10, 11):
    e0, e1 = timed(ds, ch)
    print(f"L={L} B={B} chooser {ch:3d}: {e0.elapsed_time(e1) / 10 * 1e3:8.1f} us per call (all launches of the call, back to back: the lane-per-window smoothing stage is a constant ~290 us at L = 8192 / ~2.3 ms at 65536 of it)")
for name, fx in (("ST_FX_COMP4C", audio.Compressor_4c()), ("ST_FX_COMP", audio.Compressor()), ("ST_FX_LOWPASS", audio.LowPass()), ("ST_FX_DENOISE", audio.Denoise())):
    e0, e1 = timed(datasets.SynthAudioDataSet(L, fx, datapoints=B, y_size=L // 4), -1)
    us = e0.elapsed_time(e1) / 10 * 1e3
    print(f"L={L} B={B} {name:14s}: {us:8.1f} us per call = {us * 256 / B:7.1f} us per 256-window minibatch")
