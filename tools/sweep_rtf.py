#!/usr/bin/env python3
"""Knob sweeps and knob fits from a recording encoded once (st_encode_long / st_decode_long / st_fit_knobs_coded) beside the routes that run the whole forward
per setting and per step (st_predict_long, st_fit_knobs), in one run on the same machine:
  sweep   S = 1, 4, 16 settings: S calls of StepEngine.predict_long against one encode_long + one decode_long of S settings (and the decode alone, the code
          already there), resident float32 and 16-bit PCM;
  fit     per Adam step: fit_knobs on the recording against fit_knobs on its code, the encode's one-off cost beside it;
  split   the kernels of one decoded batch (st_profile_report): decoder kernel, frames GEMM, overlap-add, with the decoder kernel's achieved HBM rate beside
          the bytes it must move -- the batch's code in, the spectra AA out.
Levels f32 and bf16_all, the default geometry, 256 windows per batch.  Every figure is the median of 3 timed runs (the routes alternate; each run repeats its
route ITER times so that it lasts tens of milliseconds) with the spread [min .. max].
    python tools/sweep_rtf.py [seconds of audio, default 60] [--out FILE, default profiles/predict_sweep_device.txt]      (GPU box)"""
import ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from signaltrain_amd import _lib, nn_proc
nn_proc._QUIET = True
args = sys.argv[1:]
OUT = os.path.join(ROOT, "profiles", "predict_sweep_device.txt")
if "--out" in args:
    i = args.index("--out"); OUT = args[i + 1]; del args[i:i + 2]
SEC = float(args[0]) if args else 60.0
SR, REPS, ITER, STEPS, BS = 44100, 3, 20, 20, 256
rng = np.random.default_rng(0)
n = int(SEC * SR)
sig = (0.3 * np.sin(2 * np.pi * 220.0 * np.arange(n) / SR) * (0.5 + 0.5 * np.sin(2 * np.pi * 0.5 * np.arange(n) / SR)) + 0.01 * rng.standard_normal(n)).astype(np.float32)
tgt = (0.6 * np.tanh(1.7 * sig)).astype(np.float32)
lines = []
lib = _lib.load()


def say(s):
    print(s, flush=True); lines.append(s)


def timed(fn, iters=1):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def fig(ts, per=1):
    """median [min .. max] of the timed runs, in ms"""
    return f"{np.median(ts) / per * 1e3:8.3f} ms [{min(ts) / per * 1e3:7.3f} .. {max(ts) / per * 1e3:7.3f}]"


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


def race(routes, iters):
    """{route: [seconds per call]} of REPS alternating timed runs, every route warmed up at the timed shapes first"""
    for fn in routes.values():
        fn()
    t = {k: [] for k in routes}
    for _ in range(REPS):
        for k, fn in routes.items():
            t[k].append(timed(fn, iters))
    return t


say(f"# encode once / decode per setting, {SEC:g} s of 44.1 kHz audio ({n} samples), {BS} windows per batch, median of {REPS} [min .. max], {torch.cuda.get_device_name(0)}")
for dt in ("f32", "bf16_all"):
    torch.manual_seed(0)
    m = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=4).to("cuda:0")
    m.set_compute_dtype(dt)
    L, y = m.in_chunk_size, m.out_chunk_size
    nwin = (n - L + y - 1) // y + 1
    n_out = n - (L - y)
    eng = m.engine(torch.empty((), device="cuda:0").expand(BS, L))
    assert eng.decode_supported()
    d = eng.dims
    KP, F, OT = int(lib.st_kp(d.F)), d.F, d.OT
    pools = {"f32": torch.from_numpy(sig).cuda(), "s16": torch.from_numpy(np.round(sig * 32767.0).astype(np.int16)).cuda()}
    say(f"window {L} -> {y}  {dt}  ({nwin} windows, {-(-nwin // BS)} batches, code {int(lib.st_code_bytes(C.byref(d), n)) / 2 ** 20:.1f} MiB)")
    for fmt, s in pools.items():
        te = race({"encode": lambda: eng.encode_long(s, batch=BS)}, ITER)["encode"]
        say(f"  {fmt}  encode_long (one-off)                 {fig(te)}")
        code = eng.encode_long(s, batch=BS)
        for S in (1, 4, 16):
            kn = torch.from_numpy((rng.random((S, 4)) - 0.5).astype(np.float32)).cuda()
            out_p = torch.empty(S, (n_out + 3) // 4 * 4, dtype=torch.float32, device="cuda:0")
            out_d = torch.empty_like(out_p)

            def predict_loop():
                for i in range(S):
                    eng.predict_long(s, kn[i], out=out_p[i], batch=BS)
            t = race({"predict": predict_loop,
                      "encode+decode": lambda: eng.decode_long(eng.encode_long(s, batch=BS), kn, out=out_d, batch=BS),
                      "decode": lambda: eng.decode_long(code, kn, out=out_d, batch=BS)}, max(ITER // S, 2))
            dev = float((out_d[:, :n_out] - out_p[:, :n_out]).abs().max() / out_p[:, :n_out].abs().max())
            mp, me, md = (np.median(t[k]) / S for k in ("predict", "encode+decode", "decode"))
            spread = max(max(v) - min(v) for v in t.values()) / S
            say(f"  {fmt}  S = {S:2d}  per setting: st_predict_long {fig(t['predict'], S)}   encode + decode {fig(t['encode+decode'], S)}   decode alone {fig(t['decode'], S)}")
            say(f"            predict / (encode + decode) = {mp / me:.2f}   predict / decode = {mp / md:.2f}   gain {1e3 * (mp - me):.3f} ms per setting, largest spread "
                f"{1e3 * spread:.3f} ms: {'beyond' if mp - me > spread else 'WITHIN'} the spread   max|decode - predict| / max|predict| = {dev:.1e}")
    # ---- the fit, per Adam step
    sd, td, k0 = pools["f32"], torch.from_numpy(tgt).cuda(), torch.zeros(4, device="cuda:0")
    code = eng.encode_long(sd, batch=BS)
    t = race({"plain": lambda: eng.fit_knobs(sd, td, k0, steps=STEPS, batch=BS), "coded": lambda: eng.fit_knobs(code, td, k0, steps=STEPS, batch=BS)}, 1)
    a, b = eng.fit_knobs(sd, td, k0, steps=STEPS, batch=BS), eng.fit_knobs(code, td, k0, steps=STEPS, batch=BS)
    mp, mc = np.median(t["plain"]) / STEPS, np.median(t["coded"]) / STEPS
    spread = max(max(v) - min(v) for v in t.values()) / STEPS
    say(f"  fit, {STEPS} Adam steps, per step: st_fit_knobs {fig(t['plain'], STEPS)}   st_fit_knobs_coded {fig(t['coded'], STEPS)}   plain / coded = {mp / mc:.2f}   gain "
        f"{1e3 * (mp - mc):.3f} ms per step, largest spread {1e3 * spread:.3f} ms: {'beyond' if mp - mc > spread else 'WITHIN'} the spread")
    say(f"       last loss plain {float(a[1][-1]):.6e} / coded {float(b[1][-1]):.6e}   max|knobs coded - plain| = {float((a[0] - b[0]).abs().max()):.1e}   (the encode, once: see above)")
    # ---- the kernel split of one decoded batch
    nb = min(BS, nwin)
    one = sd[:L + (nb - 1) * y]
    c1 = eng.encode_long(one, batch=BS)
    k1 = torch.zeros(1, 4, device="cuda:0")
    eng.decode_long(c1, k1, batch=BS)
    p = profiled(lambda: eng.decode_long(c1, k1, batch=BS))
    tot = sum(v[0] for v in p.values())
    say(f"  one decoded batch of {nb} windows, one setting, per kernel: total {tot:.1f} us")
    for name, (us, cnt) in sorted(p.items(), key=lambda kv: -kv[1][0]):
        say(f"    {name:22s} {us:9.1f} us  {cnt:3d} launches  {100 * us / tot:5.1f} %")
    code_in = nb * (KP // 2) * (32 + 2 * OT) * 4
    aa_out = nb * OT * KP * (2 if dt != "f32" else 4)
    us = p.get("ae_dec_fwd", (float("nan"), 0))[0]
    say(f"    ae_dec_fwd must move {code_in / 1e6:.1f} MB of code in + {aa_out / 1e6:.1f} MB of AA out = {(code_in + aa_out) / 1e6:.1f} MB: {(code_in + aa_out) / us / 1e6:.2f} TB/s achieved")
    q = profiled(lambda: eng.predict_long(one, k1[0], batch=BS))
    say(f"  st_predict_long on the same batch: total {sum(v[0] for v in q.values()):.1f} us  (" + ", ".join(f"{k} {v[0]:.1f}" for k, v in sorted(q.items(), key=lambda kv: -kv[1][0])) + ")")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
