#!/usr/bin/env python3
"""Reporting a model on a folder of recordings: AudioFileDataSet.evaluate (ONE st_eval_pool call + one read of the statistics) beside the way the same figures are
had without it -- a loop over the files of StepEngine.predict_long (what predict.predict_long(route="device") runs, the prediction left in HBM) followed by torch
reductions on the device and one host read per file.  The loop is the yardstick.  Scale 1 (window 8192 -> 2048), both at 200 rows per internal batch.
    pool 1   256 files of 1.5 s (30 windows each): the launch-bound case;
    pool 2   8 files of 60 s (1290 windows each): the throughput-bound case.
Arithmetic f32 and bf16_all, pools as int16 and as float32.  Wall time from the call to the figures being on the host, median of 5 after one warm-up, [min .. max].
    python tools/eval_pool_throughput.py [--out FILE, default profiles/eval_pool_device.txt]      (GPU box)
A section of FILE that starts with the line "# statistics check" (the deviations tests/test_gpu_eval_pool.py prints) is kept as it is."""
import os, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from signaltrain_amd import datasets, nn_proc
nn_proc._QUIET = True
args = sys.argv[1:]
OUT = os.path.join(ROOT, "profiles", "eval_pool_device.txt")
if "--out" in args:
    i = args.index("--out"); OUT = args[i + 1]; del args[i:i + 2]
SR, REPS, BS = 44100, 5, 200
DEV = "cuda:0"
POOLS = (("256 x 1.5 s", 256, 1.5), ("8 x 60 s", 8, 60.0))
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def fig(ts):
    return f"{np.median(ts) * 1e3:9.3f} ms [{min(ts) * 1e3:9.3f} .. {max(ts) * 1e3:9.3f}]"


def recordings(nfiles, seconds, seed):
    """int16-exact input / target pairs (s / 32767) and one knob row per file, in an object AudioFileDataSet takes as view_of."""
    rng = np.random.default_rng(seed)
    n = int(seconds * SR)
    t = np.arange(n) / SR
    src = types.SimpleNamespace(x=[], y=[], num_knobs=3, _pcm16=True)
    for f in range(nfiles):
        x = 0.4 * np.sin(2 * np.pi * (80.0 + 3.0 * f) * t) * (0.3 + 0.7 * (np.sin(2 * np.pi * 3 * t) > 0)) + 0.02 * rng.standard_normal(n)
        y = 0.7 * np.tanh(1.5 * x)
        q = lambda a: (np.round(a * 32767.0).astype(np.int16).astype(np.float64) / 32767.0).astype(np.float32)
        src.x.append(q(x)); src.y.append(q(y))
    src.knobs = np.stack([rng.integers(0, 2, nfiles), rng.uniform(20, 80, nfiles), rng.uniform(10, 90, nfiles)], axis=1).astype(np.float32)
    src.input_filenames = [f"input_{f}_.wav" for f in range(nfiles)]
    src.target_filenames = [f"target_{f}_fx__{k[0]:g}__{k[1]:g}__{k[2]:g}.wav" for f, k in enumerate(src.knobs)]
    return src


say(f"# evaluate a folder of recordings, window 8192 -> 2048 at 44.1 kHz, {torch.cuda.get_device_name(0)}")
say(f"# pool: files resident in HBM; evaluate = AudioFileDataSet.evaluate (one st_eval_pool call, {BS} rows per batch); loop = predict_long per file ({BS} windows "
    f"per batch) + torch reductions + one host read per file; median of {REPS} [min .. max]")
fx = types.SimpleNamespace(knob_ranges=np.array([[0, 1], [0, 100], [0, 100]], np.float64), knob_names=["a", "b", "c"], is_inverse=False)
for dt in ("f32", "bf16_all"):
    torch.manual_seed(0)
    m = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=3).to(DEV)
    m.set_compute_dtype(dt)
    L, y = m.in_chunk_size, m.out_chunk_size
    eng = m.engine(torch.empty((), device=DEV).expand(BS, L))
    for name, nfiles, seconds in POOLS:
        import contextlib, io
        with contextlib.redirect_stdout(io.StringIO()):
            ds = datasets.AudioFileDataSet(L, fx, sr=SR, y_size=y, augment=False, view_of=recordings(nfiles, seconds, seed=nfiles))
        kn = torch.from_numpy(ds.feed_tables()["knobs"]).to(DEV)
        for pcm in ("s16", "f32"):
            d = ds._feed_device(torch.device(DEV), pcm)
            rep = ds.evaluate(m, pcm=pcm, batch_size=BS)
            te = [timed(lambda: ds.evaluate(m, pcm=pcm, batch_size=BS))[0] for _ in range(REPS)]
            off, ln = ds.feed_tables()["off"], ds.feed_tables()["len"]
            xs = [d["x"][int(a):int(a) + int(n)] for a, n in zip(off, ln)]
            ys = [d["y"][int(a) + (L - y):int(a) + int(n)] for a, n in zip(off, ln)]

            def loop():
                res = []
                for f in range(nfiles):
                    yh = eng.predict_long(xs[f], kn[f], batch=BS)
                    t = ys[f].float() / 32767.0 if ys[f].dtype == torch.int16 else ys[f]
                    e = (yh - t).abs()
                    lc = e + torch.log1p(torch.exp(-2.0 * e)) - 0.6931471805599453
                    res.append(torch.stack([lc.double().sum(), e.double().sum(), (e * e).double().sum(), e.max().double(), (t * t).double().sum()]).tolist())
                return np.array(res)
            ref = loop()
            tl = [timed(loop)[0] for _ in range(REPS)]
            n_out = rep["n"].astype(np.float64)
            dev_mae = float(np.abs(rep["mae"] - ref[:, 1] / n_out).max() / (ref[:, 1] / n_out).max())
            dev_peak = float(np.abs(rep["peak"] - ref[:, 3]).max() / ref[:, 3].max())
            assert dev_mae <= 1e-4 and dev_peak <= 1e-4, (dev_mae, dev_peak)      # the two ways computed the same figures
            secs = nfiles * seconds
            say(f"{dt:9s} pool {name:11s} {pcm}  evaluate {fig(te)} = {secs / np.median(te):9.0f} audio-seconds / s   loop {fig(tl)}   loop / evaluate = "
                f"{np.median(tl) / np.median(te):6.2f}   (mae agrees to {dev_mae:.1e})")
kept = []
if os.path.isfile(OUT):
    old = open(OUT).read().splitlines()
    if "# statistics check" in old:
        kept = old[old.index("# statistics check"):]
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines + kept) + "\n")
