#!/usr/bin/env python3
"""GPU: rate of the device-side data feed of one effect (csrc/st_feed.h: st_synth_effect = generator kernel + for the compressors the lane-per-window
stage), windows per second, and the kernels' own times (library event profiling).  --effect comp_4c|comp|lowpass|denoise|echo|decomp_4c (default
comp_4c); --choosers 0,1,3,...: the signal families drawn (default: the effect's own set, else the compressor's); --sizes L:ysz:B,...: the cases."""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from signaltrain_amd import audio, datasets, _lib
EFFECTS = {"comp_4c": audio.Compressor_4c, "comp": audio.Compressor, "lowpass": audio.LowPass, "denoise": audio.Denoise, "echo": audio.Echo,
           "decomp_4c": audio.DeCompressor_4c}
ap = argparse.ArgumentParser()
ap.add_argument("--effect", default="comp_4c", choices=sorted(EFFECTS))
ap.add_argument("--choosers", default=None, type=lambda s: [int(v) for v in s.split(",")])
ap.add_argument("--sizes", default="8192:2048:256,8192:2048:2048,65536:16256:64,65536:16256:2048", type=lambda s: [tuple(int(v) for v in c.split(":")) for c in s.split(",")])
args = ap.parse_args()
lib = _lib.load()
for L, ysz, B in args.sizes:
    ds = datasets.SynthAudioDataSet(L, EFFECTS[args.effect](), y_size=ysz, choosers=args.choosers)
    for _ in range(3): ds.batch_device(B)
    torch.cuda.synchronize(); t0 = time.time(); n = 20
    for _ in range(n): ds.batch_device(B)
    torch.cuda.synchronize(); dt = (time.time() - t0) / n
    lib.st_profile_enable(1)
    for _ in range(5): ds.batch_device(B)
    torch.cuda.synchronize()
    buf = C.create_string_buffer(1 << 14); lib.st_profile_report(buf, len(buf)); lib.st_profile_enable(0)
    ks = "  ".join(f"{l.split()[0]} {float(l.split()[1]) / int(l.split()[2]) * 1e3:.0f} us" for l in buf.value.decode().strip().splitlines())
    tag = "" if args.effect == "comp_4c" else f"effect={args.effect} "
    print(f"{tag}L={L} B={B} families={','.join(str(c) for c in ds.choosers)}: {dt*1e3:.3f} ms/batch = {B/dt:.0f} windows/s generated on the device   [{ks}]")
