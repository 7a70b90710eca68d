#!/usr/bin/env python3
"""Scoring and fitting many knob settings from a recording's code (st_score_knobs_coded / st_fit_knobs_multi_coded) beside the routes the library had before them,
in one run, in one process, on the same inputs:
  score   S = 4, 16, 64 candidates: StepEngine.score_knobs against decode_long into an [S, n_out] buffer followed by a torch log-cosh mean over it, with the
          peak extra device memory of either side (torch's allocator: outputs and temporaries; the engine's workspaces exist before the measurement);
  fit     per Adam step per start: one fit_knobs_multi call of S starts against S sequential fit_knobs(code, ...) calls;
  stack   on the short clip, the same calls at three batch sizes: B = nwin (not stacked: every launch covers nwin rows), B = 2 nwin (the threshold of
          st_knob_multi_plan: two settings per batch) and B = 256 (as many settings as fit) -- the rows the stacking rule rests on;
  split   the kernels of one stacked batch of the fit and of the score (st_profile_report).
Levels f32 and bf16_all, the default geometry, a 60 s recording and a 2 s clip.  Every figure is the median of 3 timed runs (the routes alternate, every route
warmed up at the timed shapes first) with the spread [min .. max].
    python tools/knob_search_throughput.py [--out FILE, default profiles/knob_search_device.txt] [--quick]      (GPU box)"""
import ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from signaltrain_amd import _lib, nn_proc
nn_proc._QUIET = True
args = sys.argv[1:]
OUT = os.path.join(ROOT, "profiles", "knob_search_device.txt")
if "--out" in args:
    i = args.index("--out"); OUT = args[i + 1]; del args[i:i + 2]
QUICK = "--quick" in args          # a rehearsal at toy sizes: its figures mean nothing
SR, REPS, STEPS, BS = 44100, 3, 10, 256
LONG_S, SHORT_S = (3.0, 0.5) if QUICK else (60.0, 2.0)
SETTINGS = (4, 16) if QUICK else (4, 16, 64)
LN2 = 0.6931471805599453
rng = np.random.default_rng(0)
lines = []
lib = _lib.load()
if not torch.cuda.is_available():
    sys.exit("knob_search_throughput: needs a GPU (no figure is taken without one)")


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


def race(routes, iters):
    """{route: [seconds per call]} of REPS alternating timed runs, every route warmed up at the timed shapes first"""
    for fn in routes.values():
        fn()
    t = {k: [] for k in routes}
    for _ in range(REPS):
        for k, fn in routes.items():
            t[k].append(timed(fn, iters))
    return t


def peak_extra(fn):
    """bytes torch's allocator held at the peak of fn() beyond what it held before (warm: the engine's workspaces are allocated)"""
    fn(); torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn(); torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return peak


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


def recording(seconds):
    n = int(seconds * SR)
    sig = (0.3 * np.sin(2 * np.pi * 220.0 * np.arange(n) / SR) * (0.5 + 0.5 * np.sin(2 * np.pi * 0.5 * np.arange(n) / SR)) + 0.01 * rng.standard_normal(n)).astype(np.float32)
    return torch.from_numpy(sig).cuda(), torch.from_numpy((0.6 * np.tanh(1.7 * sig)).astype(np.float32)).cuda()


def plan_text(eng, n, S, B):
    d = eng.dims.with_batch(B)
    cnt = lib.st_knob_multi_plan(C.byref(d), n, S, None, 0)
    buf = (C.c_int * 4)()
    lib.st_knob_multi_plan(C.byref(d), n, S, buf, 1)
    return f"{cnt} batches of {buf[1]} windows x {buf[3]} settings"


def old_score(eng, code, tgt_out, kn, B):
    """the route before st_score_knobs_coded: every setting's output, then a torch log-cosh mean over it"""
    a = (eng.decode_long(code, kn, batch=B) - tgt_out).abs_()
    return (a + torch.log1p(torch.exp(-2.0 * a)) - LN2).mean(dim=1, dtype=torch.float64)


def compare(eng, code, tgt, L, y, S, B, tag):
    """one row of the score and one of the fit at S settings and B rows per batch; returns the medians (new score, old score, new fit, old fit) in s"""
    n = code.n
    kn = torch.from_numpy((rng.random((S, 4)) - 0.5).astype(np.float32)).cuda()
    tgt_out = tgt[L - y:]
    new_s = lambda: eng.score_knobs(code, tgt, kn, batch=B)
    old_s = lambda: old_score(eng, code, tgt_out, kn, B)
    a, b = new_s(), old_s()
    dev = float(((a - b).abs() / b).max())
    iters = max(64 // S, 1) if n < 10 * SR else max(8 // S, 1)
    t = race({"new": new_s, "old": old_s}, iters)
    mn, mo = np.median(t["new"]), np.median(t["old"])
    spread = max(max(v) - min(v) for v in t.values())
    pn, po = peak_extra(new_s), peak_extra(old_s)
    say(f"  {tag} S = {S:2d}  score ({plan_text(eng, n, S, B)}), per setting: score_knobs {fig(t['new'], S)}   decode_long + torch log-cosh {fig(t['old'], S)}")
    say(f"            old / new = {mo / mn:.2f}   gain {1e3 * (mo - mn) / S:.3f} ms per setting, largest spread {1e3 * spread / S:.3f} ms: {'beyond' if mo - mn > spread else 'WITHIN'} the spread   "
        f"peak extra memory: {pn / 2 ** 20:.3f} MiB against {po / 2 ** 20:.1f} MiB   max|J new - J old| / J = {dev:.1e}")
    new_f = lambda: eng.fit_knobs_multi(code, tgt, kn, steps=STEPS, batch=B)

    def old_f():
        return [eng.fit_knobs(code, tgt, kn[i], steps=STEPS, batch=B) for i in range(S)]
    a, b = new_f(), old_f()
    dk = max(float((a[0][i] - b[i][0]).abs().max()) for i in range(S))
    t2 = race({"new": new_f, "old": old_f}, 1)
    fn_, fo = np.median(t2["new"]), np.median(t2["old"])
    spread = max(max(v) - min(v) for v in t2.values())
    per = S * STEPS
    say(f"  {tag} S = {S:2d}  fit, {STEPS} Adam steps, per step per start: fit_knobs_multi {fig(t2['new'], per)}   {S} x fit_knobs(code) {fig(t2['old'], per)}")
    say(f"            old / new = {fo / fn_:.2f}   gain {1e3 * (fo - fn_) / per:.4f} ms, largest spread {1e3 * spread / per:.4f} ms: {'beyond' if fo - fn_ > spread else 'WITHIN'} the spread   "
        f"max|knobs new - old| = {dk:.1e}")
    return mn, mo, fn_, fo


say(f"# many knob settings from one code: score and fit, {BS} rows per batch, {STEPS} Adam steps per fit, median of {REPS} [min .. max], {torch.cuda.get_device_name(0)}"
    + ("   (--quick: a rehearsal, the figures mean nothing)" if QUICK else ""))
verdict = []
for dt in ("f32", "bf16_all"):
    torch.manual_seed(0)
    m = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=4).to("cuda:0")
    m.set_compute_dtype(dt)
    L, y = m.in_chunk_size, m.out_chunk_size
    eng = m.engine(torch.empty((), device="cuda:0").expand(BS, L))
    assert eng.fit_knobs_supported()
    for seconds in (LONG_S, SHORT_S):
        sig, tgt = recording(seconds)
        n = int(sig.numel())
        nwin = (n - L + y - 1) // y + 1
        code = eng.encode_long(sig, batch=min(BS, nwin))
        say(f"window {L} -> {y}  {dt}  {seconds:g} s = {n} samples, {nwin} windows ({'stacked' if 2 * nwin <= BS else 'not stacked'} at {BS} rows per batch)")
        if 2 * nwin > BS:
            for S in SETTINGS:
                compare(eng, code, tgt, L, y, S, BS, f"B = {BS:3d}")
        else:
            # the stacking rule: the same clip with the batch sized to the recording (every launch covers nwin rows: today's only form), at the threshold (two
            # settings per batch) and with as many settings as a batch of BS rows takes
            say(f"  the stacking rule on this clip: B = {nwin} (not stacked), B = {2 * nwin} (the threshold 2 nwin <= B: two settings per batch), B = {BS}")
            for S in SETTINGS:
                r = {B: compare(eng, code, tgt, L, y, S, B, f"B = {B:3d}") for B in (nwin, 2 * nwin)}
                r[BS] = compare(eng, code, tgt, L, y, S, BS, f"B = {BS:3d}")
                for what, i in (("score", 0), ("fit", 2)):
                    t0, t2, tb = r[nwin][i], r[2 * nwin][i], r[BS][i]
                    say(f"  => {dt} S = {S:2d} {what}: not stacked / stacked at the threshold = {t0 / t2:.2f}, not stacked / stacked at {BS} rows = {t0 / tb:.2f}")
                    verdict.append((dt, S, what, t0 / t2, t0 / tb))
            # ---- the kernel split of one stacked batch
            per = BS // nwin
            kn = torch.from_numpy((rng.random((per, 4)) - 0.5).astype(np.float32)).cuda()
            for what, fn in (("fit step", lambda: eng.fit_knobs_multi(code, tgt, kn, steps=1, batch=BS)), ("score", lambda: eng.score_knobs(code, tgt, kn, batch=BS))):
                fn()
                p = profiled(fn)
                tot = sum(v[0] for v in p.values())
                say(f"  one stacked batch of {nwin} windows x {per} settings = {nwin * per} rows, one {what}, per kernel: total {tot:.1f} us")
                for name, (us, cnt) in sorted(p.items(), key=lambda kv: -kv[1][0]):
                    say(f"    {name:22s} {us:9.1f} us  {cnt:3d} launches  {100 * us / tot:5.1f} %")
            one = lambda: eng.fit_knobs(code, tgt, kn[0], steps=1, batch=nwin)
            one()
            q = profiled(one)
            say(f"  st_fit_knobs_coded, one step of ONE start on the same clip ({nwin} rows): total {sum(v[0] for v in q.values()):.1f} us  ("
                + ", ".join(f"{k} {v[0]:.1f}" for k, v in sorted(q.items(), key=lambda kv: -kv[1][0])) + ")")
lose = [v for v in verdict if min(v[3], v[4]) < 1.0]
say("# stacking rule (2 nwin <= B): " + ("stacking is never slower than the batch sized to the recording in the rows above" if not lose else
                                          "stacking LOSES at " + "; ".join(f"{v[0]} S = {v[1]} {v[2]} ({v[3]:.2f} / {v[4]:.2f})" for v in lose)))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
