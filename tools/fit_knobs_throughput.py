#!/usr/bin/env python3
"""Time per optimiser step of predict.fit_knobs, both routes side by side in one run on the same model and recording:
  batched   the host loop: unfold + contiguous per batch, StepEngine.forward(save_for_backward=True), the log-cosh loss and tanh in torch,
            backward_with_knob_grad, one host synchronisation per step;
  device    st_fit_knobs: one C call that enqueues every batch of every step, the knob-only autoencoder backward, the loss, the window sum, Adam and the clamp
            on the device.
Seeded recording, 60 s at 44.1 kHz, the default geometry, 256 windows per batch, 20 steps, at f32 and bf16_all.  Warm-up first, then the routes alternate;
every figure is the median of 3 timed runs with the spread [min .. max], numpy in, numpy out (uploads and the copy back included on both routes).
Then, untimed, the library's own per-kernel times (st_profile_report: events on the stream inside the process) of ONE step of the device route, and of one
forward + backward_with_knob_grad of the batched route at the same batch, with ae_knob_bwd beside the autoencoder backward it replaces.
    python tools/fit_knobs_throughput.py [seconds of audio, default 60] [--out FILE, default profiles/fit_knobs_device.txt]      (GPU box)"""
import ctypes as C
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from signaltrain_amd import _lib, nn_proc, predict
nn_proc._QUIET = True
args = sys.argv[1:]
OUT = os.path.join(ROOT, "profiles", "fit_knobs_device.txt")
if "--out" in args:
    i = args.index("--out"); OUT = args[i + 1]; del args[i:i + 2]
SEC = float(args[0]) if args else 60.0
SR, REPS, STEPS, BS = 44100, 3, 20, 256
rng = np.random.default_rng(0)
n = int(SEC * SR)
sig = (0.3 * np.sin(2 * np.pi * 220.0 * np.arange(n) / SR) * (0.5 + 0.5 * np.sin(2 * np.pi * 0.5 * np.arange(n) / SR)) + 0.01 * rng.standard_normal(n)).astype(np.float32)
tgt = (0.6 * np.tanh(1.7 * sig)).astype(np.float32)
lines = []
lib = _lib.load()


def say(s):
    print(s, flush=True); lines.append(s)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def fig(ts, per):
    """median [min .. max] of the timed runs, in ms per optimiser step"""
    return f"{np.median(ts) / per * 1e3:8.2f} ms [{min(ts) / per * 1e3:7.2f} .. {max(ts) / per * 1e3:7.2f}]"


def profiled(fn):
    """{kernel: (total us, launches)} of one untimed pass under the library's event profiling"""
    torch.cuda.synchronize()
    _lib.check(lib.st_profile_enable(1), "st_profile_enable")
    try:
        fn(); torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 14)
        _lib.check(lib.st_profile_report(buf, len(buf)), "st_profile_report")
    finally:
        lib.st_profile_enable(0)
    out = {}
    for ln in buf.value.decode().splitlines():
        name, ms, cnt = ln.rsplit(" ", 2)
        out[name] = (float(ms) * 1e3, int(cnt))
    return out


say(f"# knob fit, {SEC:g} s of 44.1 kHz audio ({n} samples), {STEPS} Adam steps, {BS} windows per batch, median of {REPS} [min .. max], {torch.cuda.get_device_name(0)}")
for dt in ("f32", "bf16_all"):
    torch.manual_seed(0)
    m = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=4).to("cuda:0")
    m.set_compute_dtype(dt)
    L, y = m.in_chunk_size, m.out_chunk_size
    nwin = (n - L + y - 1) // y + 1
    routes = {"batched": lambda: predict.fit_knobs(sig, tgt, m, L, y, steps=STEPS, batch_size=BS),
              "device": lambda: predict.fit_knobs(sig, tgt, m, L, y, steps=STEPS, batch_size=BS, route="device")}
    res = {k: fn() for k, fn in routes.items()}                      # warm-up at the timed shapes (workspaces, first launches)
    assert all(np.isfinite(r[1]).all() and len(r[1]) == STEPS for r in res.values())
    t = {k: [] for k in routes}
    for _ in range(REPS):
        for k, fn in routes.items():
            t[k].append(timed(fn)[0])
    head = f"window {L} -> {y}  {dt:9s} ({nwin} windows, {-(-nwin // BS)} batches)"
    mb, md = np.median(t["batched"]) / STEPS, np.median(t["device"]) / STEPS
    spread = max(max(v) - min(v) for v in t.values()) / STEPS
    say(f"{head}  batched {fig(t['batched'], STEPS)} per step")
    say(f"{'':{len(head)}}  device  {fig(t['device'], STEPS)} per step   batched / device = {mb / md:.2f}   gain {1e3 * (mb - md):.2f} ms per step, "
        f"largest spread {1e3 * spread:.2f} ms: {'beyond' if mb - md > spread else 'WITHIN'} the spread")
    say(f"{'':{len(head)}}  first loss batched {res['batched'][1][0]:.6e} / device {res['device'][1][0]:.6e}  (the batched route counts the zero-padded tail of the last window)")
    # ---- the kernel split of one step of the device route
    eng = m.engine(torch.empty((), device="cuda:0").expand(BS, L))
    sd, td, kd = torch.from_numpy(sig).cuda(), torch.from_numpy(tgt).cuda(), torch.zeros(4, device="cuda:0")
    eng.fit_knobs(sd, td, kd, steps=1, batch=BS)
    p = profiled(lambda: eng.fit_knobs(sd, td, kd, steps=1, batch=BS))
    tot = sum(v[0] for v in p.values())
    say(f"  one device step, per kernel (us over all {-(-nwin // BS)} batches; launches): total {tot:.0f} us")
    for name, (us, cnt) in sorted(p.items(), key=lambda kv: -kv[1][0]):
        say(f"    {name:22s} {us:9.1f} us  {cnt:3d} launches  {100 * us / tot:5.1f} %")
    # ---- the autoencoder backward of the batched route at the same batch, beside ae_knob_bwd of one full batch
    xw = predict._windows(sig, L, y, torch.device("cuda:0"))[:BS].contiguous()
    kb = torch.zeros(BS, 4, device="cuda:0")
    g_y = torch.tanh(eng.forward(xw, kb, save_for_backward=True)[0] - 0.1) / float(BS * y)

    def old():
        eng.forward(xw, kb, save_for_backward=True)
        eng.backward_with_knob_grad(xw, kb, g_y)
    old()
    q = profiled(old)
    ae_old = {k: v for k, v in q.items() if k.startswith("ae_bwd") or k == "ae_grad_reduce"}
    one = profiled(lambda: eng.fit_knobs(sd[:L + (BS - 1) * y], td[:L + (BS - 1) * y], kd, steps=1, batch=BS))
    knob = one.get("ae_knob_bwd", (float("nan"), 0))[0]
    old_us = sum(v[0] for v in ae_old.values())
    say(f"  autoencoder backward at B = {BS}: ae_knob_bwd {knob:.1f} us  against  " + " + ".join(f"{k} {v[0]:.1f}" for k, v in ae_old.items()) +
        f" = {old_us:.1f} us of backward_with_knob_grad  ({old_us / knob:.2f} x)")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
