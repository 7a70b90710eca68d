#!/usr/bin/env python3
"""Cost of the live feed's pre-roll (st_live_feed_stream, csrc/st_feed_stream.h) on one GPU, written to profiles/stream_feed_throughput.txt:
 1. per effect, us per call of 2048 windows at L = 8192, ysz = 2048 (DeviceLiveLoader's chunk) from the int16 pool at synth_prob 0, for preroll in
    {0, L, 4 L, 16 L}, beside st_live_feed alternating in the same process, with the library's own per-kernel times (st_profile_report) of each.
    Device events around blocks of calls, a warm-up, every block's time printed;
 2. windows/s of train.train's loop at bf16_all, B = 256, comp_4c through DeviceLiveLoader at preroll 0 and 4 L.
Usage: tools/stream_feed_throughput.py [BLOCKS [CALLS [LOOP_STEPS [OUT]]]]"""
import contextlib, ctypes as C, io, os, re, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from signaltrain_amd import _lib, audio, datasets, nn_proc, train
nn_proc._QUIET = True
BLOCKS = max(3, int(sys.argv[1])) if len(sys.argv) > 1 else 5
CALLS = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 20
LOOP_STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 400
DST = os.path.abspath(sys.argv[4]) if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "stream_feed_throughput.txt")      # main() changes the directory
G, L, YSZ, SR = 2048, 8192, 2048, 44100.0
PREROLLS = [0, L, 4 * L, 16 * L]
EFFECTS = ["Compressor_4c", "Compressor", "LowPass", "Denoise", "Echo", "DeCompressor_4c"]
OUT = []


def say(*a):
    line = " ".join(str(v) for v in a); print(line, flush=True); OUT.append(line)


def make_inputs(root, nfiles, seconds, seed, sr=44100, nval=2):
    """Train/ and Val/ folders of int16 wav inputs, noise-like audio from `seed`, odd lengths."""
    rng = np.random.default_rng(seed)
    for sub, cnt in (("Train", nfiles), ("Val", nval)):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
        for i in range(cnt):
            n = int(seconds * sr) + 2 * int(rng.integers(0, 500)) + 1
            audio.write_audio_file(os.path.join(root, sub, f"rec_{i:03d}.wav"), rng.integers(-20000, 20000, size=n, dtype=np.int16), sr)
    return root


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) / n * 1e3                    # us per call


def kernel_times(fn, n=8):
    """us per call of every kernel of `fn`'s launches, by the library's own event profile"""
    lib = _lib.load()
    fn(); torch.cuda.synchronize()
    _lib.check(lib.st_profile_enable(1))
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    buf = C.create_string_buffer(4096)
    _lib.check(lib.st_profile_report(buf, 4096)); _lib.check(lib.st_profile_enable(0))
    rows = [l.split() for l in buf.value.decode().splitlines()]
    return ", ".join(f"{r[0]} {float(r[1]) * 1e3 / int(r[2]):.0f}" for r in rows)


def per_effect(root):
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with contextlib.redirect_stdout(io.StringIO()):
        src = datasets.AudioInputDataSet(L, audio.Compressor_4c(), path=root + "/Train/", datapoints=G, y_size=YSZ)
    t = src.feed_tables()
    pool = torch.from_numpy(datasets._feed_pool(src.x, "s16", "tool")).to(dev)
    off, ln = torch.from_numpy(t["off"]).to(dev), torch.from_numpy(t["len"]).to(dev)
    say(f"\n== st_live_feed_stream, {G} windows per call, L = {L}, ysz = {YSZ}, synth_prob 0, int16 pool; {len(src.x)} files, {t['pool_samples']} samples; "
        f"us per call, {BLOCKS} blocks of {CALLS} calls")
    x, y = torch.empty(G, L, device=dev), torch.empty(G, YSZ, device=dev)
    cnt = [0]
    for name in EFFECTS:
        fx = getattr(audio, name)()
        K, rng = len(fx.knob_names), fx.feed_ranges()
        lo = (C.c_float * 4)(*[float(v) for v in rng[:, 0]]); hi = (C.c_float * 4)(*[float(v) for v in rng[:, 1]])
        kn = torch.empty(G, K, device=dev)
        scr = torch.empty(max(max(int(lib.st_live_feed_stream_scratch_floats(fx.feed_fx, G, L, p, 0.0)) for p in PREROLLS), 1), device=dev)

        def live():
            _lib.check(lib.st_live_feed(fx.feed_fx, _lib.FAMILIES_COMPRESSOR, 0.0, 7, cnt[0], G, L, YSZ, K, SR, lo, hi, 1, _lib.PCM_S16, _lib.ptr(pool),
                                        _lib.ptr(off), _lib.ptr(ln), len(src.x), t["min_len"], t["pool_samples"], _lib.ptr(x), _lib.ptr(y), _lib.ptr(kn), None, _lib.ptr(scr),
                                        stream()), "st_live_feed")
            cnt[0] += G

        def streamed(p):
            _lib.check(lib.st_live_feed_stream(fx.feed_fx, _lib.FAMILIES_COMPRESSOR, 0.0, p, 7, cnt[0], G, L, YSZ, K, SR, lo, hi, 1, _lib.PCM_S16, _lib.ptr(pool),
                                               _lib.ptr(off), _lib.ptr(ln), len(src.x), t["min_len"], t["pool_samples"], _lib.ptr(x), _lib.ptr(y), _lib.ptr(kn), None,
                                               _lib.ptr(scr), stream()), "st_live_feed_stream")
            cnt[0] += G
        who = [("st_live_feed", live)] + [(f"stream preroll {p:6d}", (lambda p=p: streamed(p))) for p in PREROLLS]
        for _, fn in who:
            timed(fn, 3)                                   # warm-up: code objects, allocator
        times = {n: [] for n, _ in who}
        for blk in range(BLOCKS):
            for n, fn in who:                              # alternate the contenders inside every block
                times[n].append(timed(fn, CALLS))
        say(f"\n{name} (K = {K}):")
        for n, fn in who:
            v = times[n]; med = float(np.median(v))
            say(f"  {n:24s} " + " ".join(f"{u:8.1f}" for u in v) + f"   median {med:8.1f} us = {G / med * 1e6:12.0f} windows/s")
        for n, fn in who:
            say(f"    kernels of {n} (us per call): {kernel_times(fn)}")
        base = float(np.median(times["st_live_feed"]))
        say("  against st_live_feed: " + ", ".join(f"preroll {p}: {float(np.median(times[f'stream preroll {p:6d}'])) / base:.2f} x" for p in PREROLLS)
            + f"   ((preroll + L) / L = {', '.join(str((p + L) // L) for p in PREROLLS)})")


def loop_rate(root, preroll, B=256):
    buf = io.StringIO()
    torch.manual_seed(0); np.random.seed(0)
    with contextlib.redirect_stdout(buf):
        train.train(effect=audio.Compressor_4c(), epochs=3, n_data_points=B * LOOP_STEPS, batch_size=B, device=torch.device("cuda:0"),
                    input_path=root, preroll=preroll, device_feed=True, compute_dtype="bf16_all", device_eval=True)
    m = re.search(r"\((\d+) train windows/s incl\. the data feed; last epoch (\d+)\)", buf.getvalue())
    for f in ("modelcheckpoint.tar", "vl_avg_out.dat", "val_err_mae.dat"):
        if os.path.exists(f): os.remove(f)
    return int(m.group(1)), int(m.group(2))


def main():
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    work = tempfile.mkdtemp()
    os.chdir(work)
    say(f"stream_feed_throughput: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d')}")
    root = make_inputs(os.path.join(work, "rec16"), 16, 20.0, seed=1)
    per_effect(root)
    if LOOP_STEPS > 0:
        say(f"\n== train.train loop, comp_4c, bf16_all, B = 256, 3 epochs of {LOOP_STEPS} steps through DeviceLiveLoader (windows/s over all epochs incl. the data feed; last epoch):")
        for rep in range(2):
            for p in (0, 4 * L):                           # alternate
                r = loop_rate(root, p)
                say(f"  run {rep + 1}: preroll {p:6d} {r[0]:8d} windows/s   last epoch {r[1]:8d}")
    os.makedirs(os.path.dirname(DST), exist_ok=True)
    with open(DST, "w") as f:
        f.write("\n".join(OUT) + "\n")
    print("written:", DST)


if __name__ == "__main__":
    main()
