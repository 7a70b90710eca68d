#!/usr/bin/env python3
"""Real-time factor of long-file inference (utils/predict_long.py:30-79) over a long synthetic signal, both routes of predict.predict_long
side by side in one run:
  batched   device-side framing (a strided view of the padded signal), st_model_fwd per batch of windows, the cropped concatenation;
  device    st_predict_long: one C call that reads the windows out of the signal and writes the prediction to its place.
Per line (window, compute dtype, windows per batch):
  end to end   numpy in, numpy out: INCLUDING the host->device copy of the signal and the device->host copy of the prediction (both routes);
  resident     the signal already in HBM as float32, the prediction left there: StepEngine.predict_long, and for the batched route its loop over the
               strided view of the padded signal (predict._batched_windows) without the upload and the copy back;
  s16          the same with the signal as 16-bit PCM in HBM.
Every figure is the median of 3 timed runs (the routes alternate) with the spread [min .. max]; seconds of 44.1 kHz audio per second of wall time.
    python tools/predict_rtf.py [minutes of audio, default 10] [--out FILE, default profiles/predict_long_device_rtf.txt]      (GPU box)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from signaltrain_amd import nn_proc, predict
nn_proc._QUIET = True
args = sys.argv[1:]
OUT = os.path.join(ROOT, "profiles", "predict_long_device_rtf.txt")
if "--out" in args:
    i = args.index("--out"); OUT = args[i + 1]; del args[i:i + 2]
MIN = float(args[0]) if args else 10.0
SR, REPS = 44100, 3
rng = np.random.default_rng(0)
n = int(MIN * 60 * SR)
sig = (0.3 * np.sin(2 * np.pi * 220.0 * np.arange(n) / SR) * (0.5 + 0.5 * np.sin(2 * np.pi * 0.5 * np.arange(n) / SR)) + 0.01 * rng.standard_normal(n)).astype(np.float32)
kn = np.array([0.1, -0.2, 0.3, 0.0], np.float32)
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def fig(ts):
    """median [min .. max] of the timed runs, in ms"""
    return f"{np.median(ts) * 1e3:7.1f} ms [{min(ts) * 1e3:6.1f} .. {max(ts) * 1e3:6.1f}]"


say(f"# long-file inference, {MIN:g} min of 44.1 kHz audio ({n} samples), median of {REPS} [min .. max], {torch.cuda.get_device_name(0)}")
for scale in (1, 8):
    for dt in ("f32", "bf16_all"):
        torch.manual_seed(0)
        m = nn_proc.st_model(scale_factor=scale, shrink_factor=4, num_knobs=4).to("cuda:0")
        m.set_compute_dtype(dt)
        L, y = m.in_chunk_size, m.out_chunk_size
        nwin = (n - L + y - 1) // y + 1
        for bs in ((200, 1024) if scale == 1 else (64, 200)):       # 200 = the reference's default (predict_long.py:30)
            eng = m.engine(torch.empty((), device="cuda:0").expand(bs, L))
            on_device = eng.predict_supported()
            routes = {"batched": lambda: predict.predict_long(sig, kn, m, L, y, sr=SR, batch_size=bs)}
            if on_device:
                routes["device"] = lambda: predict.predict_long(sig, kn, m, L, y, sr=SR, batch_size=bs, route="device")
            for fn in routes.values():                               # warm-up at the timed shapes (workspaces, first launches)
                ref = fn()
            assert np.isfinite(ref).all() and len(ref) == n - (L - y)
            t = {k: [] for k in routes}
            for _ in range(REPS):
                for k, fn in routes.items():
                    t[k].append(timed(fn)[0])
            head = f"window {L:6d} -> {y:5d}  {dt:9s} batch {bs:5d} ({nwin} windows)"
            say(f"{head}  batched end to end {fig(t['batched'])} = {MIN * 60 / np.median(t['batched']):7.0f} x real time ({nwin / np.median(t['batched']) / 1e3:7.1f} k windows/s)")
            xw = predict._windows(sig, L, y, torch.device("cuda:0"))
            predict._batched_windows(xw, kn, m, y, bs)
            tb = [timed(lambda: predict._batched_windows(xw, kn, m, y, bs))[0] for _ in range(REPS)]
            say(f"{'':{len(head)}}  batched resident   {fig(tb)} = {MIN * 60 / np.median(tb):7.0f} x real time ({nwin / np.median(tb) / 1e3:7.1f} k windows/s)")
            del xw
            if not on_device:
                say(f"{'':{len(head)}}  device   not run: st_predict_supported refuses this geometry (route='device' takes the batched route)")
                continue
            say(f"{'':{len(head)}}  device  end to end {fig(t['device'])} = {MIN * 60 / np.median(t['device']):7.0f} x real time ({nwin / np.median(t['device']) / 1e3:7.1f} k windows/s)"
                f"  batched / device = {np.median(t['batched']) / np.median(t['device']):.2f}")
            sig_f = torch.from_numpy(sig).cuda()
            sig_s = torch.from_numpy(np.round(sig * 32767.0).astype(np.int16)).cuda()
            knd = torch.from_numpy(kn).cuda()
            out = torch.empty(n - (L - y), dtype=torch.float32, device="cuda:0")
            for name, s in (("resident", sig_f), ("s16     ", sig_s)):
                eng.predict_long(s, knd, out=out, batch=bs)
                ts = [timed(lambda: eng.predict_long(s, knd, out=out, batch=bs))[0] for _ in range(REPS)]
                assert bool(torch.isfinite(out).all())
                say(f"{'':{len(head)}}  device  {name}   {fig(ts)} = {MIN * 60 / np.median(ts):7.0f} x real time ({nwin / np.median(ts) / 1e3:7.1f} k windows/s)"
                    f"  batched resident / device = {np.median(tb) / np.median(ts):.2f}")
            del sig_f, sig_s, out
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
