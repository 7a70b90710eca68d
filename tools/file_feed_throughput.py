#!/usr/bin/env python3
"""Cost of the feed of recorded pairs on one GPU, written to profiles/file_feed_throughput.txt:
 1. per minibatch, alternating in one process: AudioFileDataSet.batch_device (the torch gather: index tensor, two gathers, global generator),
    batch_device_fused with float32 pools and with int16 pools (one st_file_feed launch), and st_file_feed alone into preallocated outputs --
    at B = 256, L = 8192, ysz = 2048 and at B = 64, L = 65536, ysz = 16384, K = 3, a 64-file pool generated from a seed; device events, a
    warm-up, BLOCKS blocks of BATCHES batches per contender, every block time printed; the kernel's share of the HBM floor
    (B (L + ysz) (4 + sample size) bytes at the 6.3 TB/s MI355X streams at);
 2. windows/s of train.train's loop at bf16_all with the torch gather behind the driver's former _FileLoader and with DeviceFileLoader.
Usage: tools/file_feed_throughput.py [BLOCKS [BATCHES [LOOP_STEPS]]]"""
import contextlib, ctypes as C, io, os, re, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from signaltrain_amd import _lib, audio, datasets, nn_proc, train
nn_proc._QUIET = True
BLOCKS = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 5
BATCHES = max(200, int(sys.argv[2])) if len(sys.argv) > 2 else 200
LOOP_STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 600
HBM = 6.3e12
OUT = []


def say(*a):
    line = " ".join(str(v) for v in a); print(line, flush=True); OUT.append(line)


def make_pool(root, nfiles, seconds, seed, sr=44100, nval=2):
    """input_/target_ int16 wav pairs of an 'LA2A_3c'-shaped effect (3 knobs in the target names), noise-like audio from `seed`, odd lengths."""
    rng = np.random.default_rng(seed)
    for sub, cnt in (("Train", nfiles), ("Val", nval)):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
        for i in range(cnt):
            n = int(seconds * sr) + 2 * int(rng.integers(0, 500)) + 1
            x = rng.integers(-20000, 20000, size=n, dtype=np.int16)
            y = (x // 2).astype(np.int16)
            kn = [i % 2, round(float(rng.uniform(20, 80)), 2), round(float(rng.uniform(10, 90)), 2)]
            audio.write_audio_file(os.path.join(root, sub, f"input_{i:03d}_.wav"), x, sr)
            audio.write_audio_file(os.path.join(root, sub, f"target_{i:03d}_LA2A_3c__{kn[0]:g}__{kn[1]:g}__{kn[2]:g}.wav"), y, sr)
    with open(os.path.join(root, "effect_info.ini"), "w") as f:
        f.write("[effect]\nname = 'LA2A_3c'\nknob_names = ['Limit/Comp', 'Gain', 'Gain Reduction']\nknob_ranges = [[0,1], [0,100], [0,100]]\n")
    return root


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) / n * 1e3                    # us per batch


def per_minibatch(root, B, L, ysz):
    fx = audio.FileEffect(root)
    with contextlib.redirect_stdout(io.StringIO()):
        ds = datasets.AudioFileDataSet(L, fx, path=root + "/Train/", datapoints=B * BATCHES, y_size=ysz, augment=True)
    t = ds.feed_tables()
    say(f"\n== per minibatch: B = {B}, L = {L}, ysz = {ysz}, K = 3; {len(ds.x)} files, {t['pool_samples']} samples per side "
        f"(float32 pools 2 x {t['pool_samples'] * 4 / 2**20:.0f} MiB, int16 pools 2 x {t['pool_samples'] * 2 / 2**20:.0f} MiB; default pcm = {t['pcm']})")
    dev = torch.device("cuda:0")
    raw = {}
    for pcm in ("f32", "s16"):
        d = ds._feed_device(dev, pcm)
        raw[pcm] = (d, torch.empty(B, L, device=dev), torch.empty(B, ysz, device=dev), torch.empty(B, 3, device=dev))
    lib, cnt = _lib.load(), [0]

    def kernel(pcm):
        d, x, y, kn = raw[pcm]
        _lib.check(lib.st_file_feed(7, cnt[0], B, L, ysz, 3, _lib.PCM_S16 if pcm == "s16" else _lib.PCM_F32, _lib.ptr(d["x"]), _lib.ptr(d["y"]), _lib.ptr(d["off"]),
                                    _lib.ptr(d["len"]), len(ds.x), d["min_len"], d["pool_samples"], _lib.ptr(d["kn"]), 1, _lib.ptr(x), _lib.ptr(y), _lib.ptr(kn), None,
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "st_file_feed")
        cnt[0] += B
    who = [("torch gather (batch_device)", lambda: ds.batch_device(B, dev)),
           ("fused, float32 pools", lambda: ds.batch_device_fused(B, dev, pcm="f32")),
           ("fused, int16 pools", lambda: ds.batch_device_fused(B, dev, pcm="s16")),
           ("st_file_feed alone, float32", lambda: kernel("f32")),
           ("st_file_feed alone, int16", lambda: kernel("s16"))]
    meta = ds.batch_device_fused(4096, dev, with_meta=True)[3].cpu().numpy()
    res = (t["off"][meta[:, 0]] + meta[:, 1]) % 8
    say("alignment of the timed source spans: random starts in files of odd lengths; (off + start) % 8 over 4096 windows of the stream:", np.bincount(res, minlength=8).tolist())
    for _, fn in who:
        timed(fn, 20)                                      # warm-up: pools, allocator, code objects
    times = {name: [] for name, _ in who}
    for blk in range(BLOCKS):
        for name, fn in who:                               # alternate the contenders inside every block
            times[name].append(timed(fn, BATCHES))
    say(f"us per minibatch, {BLOCKS} blocks of {BATCHES} batches (device events around each block):")
    for name, _ in who:
        v = times[name]
        say(f"  {name:32s} " + " ".join(f"{u:8.2f}" for u in v) + f"   median {np.median(v):8.2f}  spread {max(v) - min(v):6.2f}")
    for pcm, ssz in (("float32", 4), ("int16", 2)):
        byt = B * (L + ysz) * (4 + ssz)
        k = float(np.median(times[f"st_file_feed alone, {pcm}"]))
        say(f"  st_file_feed alone, {pcm}: {byt / 1e6:.2f} MB per launch -> HBM floor {byt / HBM * 1e6:.2f} us at 6.3 TB/s; measured {k:.2f} us = {byt / (k * 1e-6) / 1e12:.2f} TB/s, "
            f"{100 * byt / HBM / (k * 1e-6):.0f} % of the floor rate (back-to-back launches; pools of this size partly live in the 256 MiB Infinity Cache)")
    # the launch DeviceFileLoader makes: gen_windows = 2048 windows at once -- long enough to time the kernel itself, not the launch rate of the host
    G = 2048
    xg, yg, kg = torch.empty(G, L, device=dev), torch.empty(G, ysz, device=dev), torch.empty(G, 3, device=dev)
    for pcm, ssz in (("f32", 4), ("s16", 2)):
        raw[pcm] = (raw[pcm][0], xg, yg, kg)
    B_small, B = B, G
    timed(lambda: kernel("f32"), 3); timed(lambda: kernel("s16"), 3)
    chunk = {pcm: [] for pcm in ("f32", "s16")}
    for blk in range(BLOCKS):
        for pcm in ("f32", "s16"):
            chunk[pcm].append(timed(lambda: kernel(pcm), 20))
    for pcm, ssz in (("f32", 4), ("s16", 2)):
        byt, v = G * (L + ysz) * (4 + ssz), chunk[pcm]
        k = float(np.median(v))
        say(f"  st_file_feed alone, {G} windows per launch (DeviceFileLoader's chunk), {pcm} pools, us per launch, {BLOCKS} blocks of 20: " + " ".join(f"{u:8.2f}" for u in v))
        say(f"      {byt / 1e6:.1f} MB per launch -> HBM floor {byt / HBM * 1e6:.1f} us; median {k:.1f} us = {byt / (k * 1e-6) / 1e12:.2f} TB/s = {100 * byt / HBM / (k * 1e-6):.0f} % of the "
            f"6.3 TB/s floor rate; {k / G * B_small:.2f} us per {B_small}-window minibatch")
    B = B_small
    tg = times["torch gather (batch_device)"]
    for name in ("fused, float32 pools", "fused, int16 pools"):
        v = times[name]
        gap, spread = min(tg) - max(v), max(max(tg) - min(tg), max(v) - min(v))
        say(f"  acceptance: {name}: slowest fused block {max(v):.2f} us vs fastest torch block {min(tg):.2f} us: gap {gap:.2f} us, block-to-block spread {spread:.2f} us -> "
            f"{'FASTER by more than the spread' if gap > spread else 'NOT faster by more than the spread'}")


class TorchGatherLoader:
    """The driver's former _FileLoader: AudioFileDataSet.device_batches in line in front of the step."""

    def __init__(self, ds, batch_size, device): self.ds, self.batch_size, self.device = ds, batch_size, device
    def __iter__(self): return self.ds.device_batches(self.batch_size, self.device)
    def __len__(self): return len(self.ds) // self.batch_size


def loop_rate(root, which, B=256):
    real = train.train_loop

    def swap(model, engine, effect, device, epochs, batch_size, lr_sched, mom_sched, dataloader, dataloader_val, *a, **kw):
        assert isinstance(dataloader, datasets.DeviceFileLoader)
        if which == "torch":
            dataloader = TorchGatherLoader(dataloader.ds, batch_size, device)
        return real(model, engine, effect, device, epochs, batch_size, lr_sched, mom_sched, dataloader, dataloader_val, *a, **kw)
    train.train_loop = swap
    buf = io.StringIO()
    try:
        torch.manual_seed(0); np.random.seed(0)
        with contextlib.redirect_stdout(buf):
            train.train(effect=audio.FileEffect(root), epochs=3, n_data_points=B * LOOP_STEPS, batch_size=B, device=torch.device("cuda:0"), datapath=root,
                        device_feed=True, compute_dtype="bf16_all", device_eval=True)
    finally:
        train.train_loop = real
    m = re.search(r"\((\d+) train windows/s incl\. the data feed; last epoch (\d+)\)", buf.getvalue())
    for f in ("modelcheckpoint.tar", "vl_avg_out.dat", "val_err_mae.dat"):
        if os.path.exists(f): os.remove(f)
    return int(m.group(1)), int(m.group(2))


def main():
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    work = tempfile.mkdtemp()
    os.chdir(work)
    say(f"file_feed_throughput: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d')}")
    big = make_pool(os.path.join(work, "pool64"), 64, 20.0, seed=1)
    per_minibatch(big, 256, 8192, 2048)
    per_minibatch(big, 64, 65536, 16384)
    small = make_pool(os.path.join(work, "pool16"), 16, 10.0, seed=2, nval=16)
    say(f"\n== train.train loop, bf16_all, B = 256, 3 epochs of {LOOP_STEPS} steps, 16-file pool (windows/s over all epochs incl. the data feed; last epoch):")
    rates = {"torch": [], "fused": []}
    for rep in range(2):
        for which in ("torch", "fused"):                    # alternate
            r = loop_rate(small, which)
            rates[which].append(r)
            say(f"  run {rep + 1}: {'torch gather in line (_FileLoader)' if which == 'torch' else 'DeviceFileLoader (st_file_feed, side stream)':46s} {r[0]:8d} windows/s   last epoch {r[1]:8d}")
    lt, lf = max(r[1] for r in rates["torch"]), min(r[1] for r in rates["fused"])
    say(f"  acceptance (last-epoch rates): slowest DeviceFileLoader run {lf} vs fastest _FileLoader run {lt} windows/s -> {'not slower' if lf >= lt else 'SLOWER'}")
    dst = os.path.join(ROOT, "profiles", "file_feed_throughput.txt")
    with open(dst, "w") as f:
        f.write("\n".join(OUT) + "\n")
    print("written:", dst)


if __name__ == "__main__":
    main()
