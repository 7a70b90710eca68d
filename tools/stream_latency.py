#!/usr/bin/env python3
"""Latency of a predict session (StepEngine.open_stream / PredictStream.push) beside the way the same thing is done without it, at scale 1, f32 and bf16_all.
Pushes: one push of m = y samples per channel (one window per channel) at C = 1, 2, 8, 64 channels, blocks already in HBM, wall time from the call to the
  device having finished; median of REPS pushes after a warm-up, with [min .. max], beside the block's duration y / 44100 s.
    session   PredictStream.push of a [C, y] block;
    rolling   built only from entries that exist without the session: a rolling [L] tensor per channel (torch.cat of its tail and the new block) and one
              StepEngine.predict_long call on it per block and channel.
Files: StepEngine.predict_channels on 60 s x 2 and x 8 channels against one predict_long call per channel; median of 3.
    python tools/stream_latency.py [--out FILE, default profiles/predict_stream_device.txt]      (GPU box)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from signaltrain_amd import nn_proc
nn_proc._QUIET = True
args = sys.argv[1:]
OUT = os.path.join(ROOT, "profiles", "predict_stream_device.txt")
if "--out" in args:
    i = args.index("--out"); OUT = args[i + 1]; del args[i:i + 2]
SR, REPS, WARM, FILE_REPS, FILE_S = 44100, 30, 5, 3, 60
DEV = "cuda:0"
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def fig(ts, unit=1e6, name="us", prec=1):
    return f"{np.median(ts) * unit:8.{prec}f} {name} [{min(ts) * unit:8.{prec}f} .. {max(ts) * unit:8.{prec}f}]"


def tone(C, n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    return np.stack([0.3 * np.sin(2 * np.pi * 110.0 * (c + 2) * t) + 0.01 * rng.standard_normal(n) for c in range(C)]).astype(np.float32)


say(f"# predict session, window 8192 -> 2048 at 44.1 kHz, {torch.cuda.get_device_name(0)}")
say(f"# pushes: one block of y = 2048 samples per channel ({2048 / SR * 1e3:.1f} ms of audio), median of {REPS} pushes [min .. max] after {WARM}")
kn = torch.tensor([0.1, -0.2, 0.3, 0.0], device=DEV)
for dt in ("f32", "bf16_all"):
    torch.manual_seed(0)
    m = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=4).to(DEV)
    m.set_compute_dtype(dt)
    L, y = m.in_chunk_size, m.out_chunk_size
    for C in (1, 2, 8, 64):
        eng = m.engine(torch.empty((), device=DEV).expand(max(C, 1), L))
        sig = torch.from_numpy(tone(C, L + (WARM + REPS) * y, seed=C)).to(DEV)
        st = eng.open_stream(C, batch=C)
        st.push(sig[:, :L].contiguous(), kn)
        blocks = [sig[:, L + i * y:L + (i + 1) * y].contiguous() for i in range(WARM + REPS)]
        last = None
        ts = []
        for i, b in enumerate(blocks):
            t, last = timed(lambda: st.push(b, kn))
            if i >= WARM:
                ts.append(t)
        assert tuple(last.shape) == (C, y) and bool(torch.isfinite(last).all())
        roll = [sig[c, :L].clone() for c in range(C)]
        tr = []

        def rolling(b):
            out = []
            for c in range(C):
                roll[c] = torch.cat((roll[c][y:], b[c]))
                out.append(eng.predict_long(roll[c], kn, batch=1))
            return out
        for i, b in enumerate(blocks):
            t, ref = timed(lambda: rolling(b))
            if i >= WARM:
                tr.append(t)
        e = float((torch.stack(ref) - last).abs().max() / last.abs().max())
        assert e <= 1e-5, e                                   # the two ways computed the same last block
        say(f"{dt:9s} C = {C:3d}  session {fig(ts)}   rolling {fig(tr)}   rolling / session = {np.median(tr) / np.median(ts):5.2f}   "
            f"block = {y / SR * 1e6:.0f} us: session takes {np.median(ts) / (y / SR) * 100:.2f} % of it")
say(f"# files: {FILE_S} s x C channels resident in HBM, median of {FILE_REPS} [min .. max]")
for dt in ("f32", "bf16_all"):
    torch.manual_seed(0)
    m = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=4).to(DEV)
    m.set_compute_dtype(dt)
    L, y = m.in_chunk_size, m.out_chunk_size
    bs = 1024
    eng = m.engine(torch.empty((), device=DEV).expand(bs, L))
    for C in (2, 8):
        n = FILE_S * SR
        sig = torch.from_numpy(tone(C, n, seed=100 + C)).to(DEV)
        out = torch.empty(C, (n - (L - y) + 3) // 4 * 4, dtype=torch.float32, device=DEV)
        got = eng.predict_channels(sig, kn, out=out)
        tc = [timed(lambda: eng.predict_channels(sig, kn, out=out))[0] for _ in range(FILE_REPS)]
        per = lambda: [eng.predict_long(sig[c], kn, batch=bs) for c in range(C)]
        ref = torch.stack(per())
        tp = [timed(per)[0] for _ in range(FILE_REPS)]
        e = float((ref - got).abs().max() / ref.abs().max())
        assert e <= 1e-5, e
        say(f"{dt:9s} C = {C:3d}  predict_channels {fig(tc, 1e3, 'ms', 2)} = {C * FILE_S / np.median(tc):8.0f} channel-seconds / s   "
            f"predict_long per channel {fig(tp, 1e3, 'ms', 2)}   per channel / channels = {np.median(tp) / np.median(tc):5.2f}")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
