#!/usr/bin/env python3
"""Rendering a folder of recordings through an effect: ONE st_render_pool call beside what the library offered before it -- one existing effect entry
(st_compressor_4c, st_compressor, st_lowpass, st_echo, st_denoise_input) per file, B = 1, on an aligned copy of the file.  The loop is the yardstick; its
copies, outputs and knob rows are made before the clock starts.
    pool 1   256 clips of 1.5 s: the launch-bound case (and, for the 4-control compressor, 256 one-thread chains one after the other);
    pool 2   8 files of 60 s: few long files -- the sequential chain keeps 8 lanes busy.
Float32 pool, 44.1 kHz.  Both forms are timed in the same process, alternating, after one warm-up each: device events around the calls, the second event
synchronised; median of REPS [min .. max]; spread = max - min.  The render's bits are compared with the loop's once per case.
    python tools/render_pool_throughput.py [--out FILE, default profiles/render_pool_device.txt] [--once]      (GPU box)
--once: one st_render_pool call per case and nothing else (the run a kernel trace is taken of); writes no file.
A section of FILE that starts with the line "# resource summary" is kept as it is."""
import ctypes as C, datetime, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from signaltrain_amd import _lib
args = sys.argv[1:]
OUT = os.path.join(ROOT, "profiles", "render_pool_device.txt")
if "--out" in args:
    i = args.index("--out"); OUT = args[i + 1]; del args[i:i + 2]
ONCE = "--once" in args
SR, REPS = 44100.0, 7
POOLS = (("256 x 1.5 s", 256, 1.5), ("8 x 60 s", 8, 60.0))
FX = (("comp_4c", _lib.FX_COMP4C, "st_compressor_4c", 4), ("comp", _lib.FX_COMP, "st_compressor", 3), ("lowpass", _lib.FX_LOWPASS, "st_lowpass", 1),
      ("echo", _lib.FX_ECHO, "st_echo", 3), ("denoise", _lib.FX_DENOISE, "st_denoise_input", 1), ("decomp_4c", _lib.FX_DECOMP4C, "st_compressor_4c", 4))
LL = C.POINTER(C.c_longlong)
lib = _lib.load()
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def fig(ts):
    return f"{np.median(ts):10.3f} ms [{min(ts):10.3f} .. {max(ts):10.3f}]"


def knobs(fx, nfiles, rng):
    kw = np.zeros((nfiles, 4), np.float32)
    u = rng.random((nfiles, 4))
    if fx in (_lib.FX_COMP4C, _lib.FX_DECOMP4C, _lib.FX_COMP):
        kw[:] = np.array([-30.0, 1.0, 1e-3, 1e-3]) + u * np.array([30.0, 4.0, 3.9e-2, 3.9e-2])
    elif fx == _lib.FX_LOWPASS:
        kw[:, 0] = 10.0 + 1990.0 * u[:, 0]
    elif fx == _lib.FX_DENOISE:
        kw[:, 0] = 0.5 * u[:, 0]
    else:
        kw[:, :3] = np.stack([np.full(nfiles, 400.0), 0.4 + 0.6 * u[:, 1], np.full(nfiles, 2.0)], axis=1)
    return kw


say(f"# render a folder of recordings through an effect, float32 pool at 44.1 kHz, {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}")
say(f"# render = one st_render_pool call; loop = one effect entry per file (B = 1, aligned copies made beforehand); device events, alternating, median of {REPS} "
    f"[min .. max] after one warm-up each; spread = max - min of the loop")
verdicts = []
for name, nfiles, seconds in POOLS:
    n = int(seconds * SR)
    rng = np.random.default_rng(nfiles)
    t = np.arange(n) / SR
    files = [(0.4 * np.sin(2 * np.pi * (80.0 + 3.0 * f) * t) * (0.3 + 0.7 * (np.sin(2 * np.pi * 3 * t) > 0)) + 0.02 * rng.standard_normal(n)).astype(np.float32) for f in range(nfiles)]
    lens = np.full(nfiles, n, np.int64)
    off = np.arange(nfiles, dtype=np.int64) * n
    pool = torch.from_numpy(np.concatenate(files)).cuda()
    off_d, len_d = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    out = torch.empty(nfiles * n, device="cuda")
    npad = -(-n // 4) * 4
    xs = torch.zeros(nfiles, npad, device="cuda"); xs[:, :n] = pool.view(nfiles, n)
    ys = torch.empty(nfiles, npad, device="cuda")
    for label, fx, entry, K in FX:
        kw = knobs(fx, nfiles, rng)
        kw_d = torch.from_numpy(kw).cuda()
        rows = torch.from_numpy(np.ascontiguousarray(kw[:, :K])).cuda()
        scr = torch.empty(int(lib.st_render_pool_scratch_floats(fx, lens.ctypes.data_as(LL), nfiles)), device="cuda")

        def render():
            _lib.check(lib.st_render_pool(fx, SR, _lib.PCM_F32, _lib.ptr(pool), _lib.ptr(off_d), _lib.ptr(len_d), nfiles, n, nfiles * n, _lib.ptr(kw_d), 5, 0, _lib.ptr(out),
                                          _lib.ptr(scr) if scr.numel() else None, stream()), "st_render_pool")

        Lf = npad if fx in (_lib.FX_LOWPASS, _lib.FX_DENOISE) else n      # the multiple each entry demands
        ptrs = [(C.c_void_p(xs[f].data_ptr()), C.c_void_p(rows[f].data_ptr()), C.c_void_p(ys[f].data_ptr())) for f in range(nfiles)]

        def loop():
            s = stream()
            for f, (xp, kp, yp) in enumerate(ptrs):
                if fx == _lib.FX_DENOISE:
                    rc = lib.st_denoise_input(5, f, xp, kp, 1, Lf, yp, s)
                else:
                    rc = getattr(lib, entry)(xp, kp, SR, 1, Lf, Lf, yp, s)
                if rc:
                    _lib.check(rc, entry)
        if ONCE:
            render(); torch.cuda.synchronize()
            continue
        render(); loop(); torch.cuda.synchronize()
        same = torch.equal(out.view(nfiles, n).view(torch.int32), ys[:, :n].contiguous().view(torch.int32))
        tr, tl = [], []
        for _ in range(REPS):
            tr.append(timed(render)); tl.append(timed(loop))
        spread = max(tl) - min(tl)
        ok = np.median(tr) < np.median(tl) if nfiles > 64 else np.median(tr) <= np.median(tl) + spread
        verdicts.append(ok)
        say(f"pool {name:11s} {label:9s} render {fig(tr)} = {nfiles * seconds / (np.median(tr) * 1e-3):10.0f} audio-seconds / s   loop {fig(tl)}   loop / render = "
            f"{np.median(tl) / np.median(tr):7.2f}   loop spread {spread:8.3f} ms   bits {'equal' if same else 'DIFFER'}   {'ok' if ok else 'SLOWER'}")
if not ONCE:
    say("# requirement (render faster on the 256 clips; on the 8 long files not slower than the loop by more than the loop's spread): "
        + ("met in every row" if all(verdicts) else "NOT met in the rows marked SLOWER"))
    kept = []
    if os.path.isfile(OUT):
        old = open(OUT).read().splitlines()
        if "# resource summary" in old:
            kept = old[old.index("# resource summary"):]
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines + kept) + "\n")
