"""GPU: the live feed's pre-roll (st_live_feed_stream, csrc/st_feed_stream.h).  With preroll = 0 the call is st_live_feed.  With a pre-roll a recorded row's
window is st_live_feed's and its target is the last ysz samples of the library's own effect entry on the extended span xe = R samples of history + the
window, R = min(preroll, start & ~3), rebuilt here from the float32 pool and the draws of datasets.live_feed_draw: every comparison is bit for bit.
Synthetic rows are st_synth_effect_families'.  Pool, seed and first window are tests/test_gpu_live_feed.py's."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_live_feed import B0, FIRST, SEED, SR, _call, _draw, _effect, _live, _pool, _stream, _synth
from tests.test_live_feed_host import make_input_dataset

pytestmark = pytest.mark.gpu
# (L, ysz, preroll): both extended rows reach 12288 samples, across the COMP_CH = 8192 chunk edge of the compressor and several ENV_CH = 2048 scan chunks
SHAPES = [(4096, 1024, 8192), (8192, 2048, 4096)]
COVERAGE = {(4096, 8192): (10, 15, 7), (8192, 4096): (14, 11, 7)}      # rows with a full history, a partial one, none (datasets.live_feed_draw)
WHOLE = 32768                                                          # above every start of the L = 4096 pool: the whole file in front of the window


def _stream_feed(name, L, ysz, B, p, preroll, pcm="s16", first=FIRST, seed=SEED, families=None, augment=1, scratch=True):
    """st_live_feed_stream -> dict(x, y, kn, meta, scr [, kw [B][4] world knobs, rr [B] = R or -1])"""
    from signaltrain_amd import _lib
    lib = _lib.load()
    fx, K, rng = _effect(name)
    P = _pool(L)
    x = torch.full((B, L), float("nan"), device="cuda"); y = torch.full((B, ysz), float("nan"), device="cuda"); kn = torch.full((B, K), float("nan"), device="cuda")
    meta = torch.full((B, 4), -7, dtype=torch.int64, device="cuda")
    lo = (C.c_float * 4)(*[float(v) for v in rng[:, 0]]); hi = (C.c_float * 4)(*[float(v) for v in rng[:, 1]])
    n = int(lib.st_live_feed_stream_scratch_floats(fx, B, L, preroll, p))
    assert n > 0 or preroll == 0
    scr = torch.full((n,), float("nan"), device="cuda") if scratch else None
    _lib.check(lib.st_live_feed_stream(fx, _lib.family_mask(families), p, preroll, seed, first, B, L, ysz, K, SR, lo, hi, augment,
                                       _lib.PCM_S16 if pcm == "s16" else _lib.PCM_F32, _lib.ptr(P[pcm]), _lib.ptr(P["d_off"]), _lib.ptr(P["d_len"]), 3,
                                       int(P["len"].min()), int(P["len"].sum()), _lib.ptr(x), _lib.ptr(y), _lib.ptr(kn), _lib.ptr(meta), _lib.ptr(scr), _stream()),
               "st_live_feed_stream")
    torch.cuda.synchronize()
    r = {"x": x, "y": y, "kn": kn, "meta": meta, "scr": scr}
    if preroll:                                                  # the scratch's head: [world knobs 4 B | R per row as int32, -1 for a synthetic row]
        r["kw"] = scr[:4 * B].reshape(B, 4).clone()
        r["rr"] = scr[4 * B:5 * B].view(torch.int32).clone()
    return r


def _history(L, B, preroll, first=FIRST, seed=SEED):
    """R per row by the law, from the host replica's starts"""
    st = _draw(L, B, 0.0, first, seed)[2]
    return np.minimum(preroll, st & ~3)


def _extended(L, rows, R, first=FIRST, seed=SEED, B=B0):
    """xe of the rows `rows` (all with the history R): [len(rows)][R + L] from the float32 pool"""
    P = _pool(L)
    _, f, st, fl = _draw(L, B, 0.0, first, seed)
    base = torch.from_numpy(P["off"][f[rows]] + st[rows] - R).cuda()
    sign = torch.from_numpy(np.where(fl[rows] == 1, -1.0, 1.0).astype(np.float32)).cuda()
    return (P["f32"][base[:, None] + torch.arange(R + L, device="cuda")[None, :]] * sign[:, None]).contiguous()


def _entry_tail(name, L, ysz, R_all, kw, want, rows=None):
    """The last `want` samples of the effect's library entry on xe, row by row (grouped by R) -> [rows][want]"""
    entry, k = {"Compressor_4c": ("st_compressor_4c", 4), "Comp_Just_Thresh": ("st_compressor_4c", 4), "DeCompressor_4c": ("st_compressor_4c", 4),
                "Compressor": ("st_compressor", 3), "LowPass": ("st_lowpass", 1), "Echo": ("st_echo", 3)}[name]
    rows = np.arange(len(R_all)) if rows is None else np.asarray(rows)
    out = torch.empty(len(rows), want, device="cuda")
    for R in sorted(set(R_all[rows].tolist())):
        sel = np.flatnonzero(R_all[rows] == R)
        out[torch.from_numpy(sel).cuda()] = _call(entry, _extended(L, rows[sel], int(R)), kw[torch.from_numpy(rows[sel]).cuda()][:, :k], want)
    return out


# ---- 1. preroll = 0 is st_live_feed
@pytest.mark.parametrize("name", ["Compressor_4c", "Compressor", "LowPass", "Echo", "Denoise", "DeCompressor_4c", "Comp_Just_Thresh"])
def test_preroll_zero_is_the_live_feed(name):
    L, ysz, B = 4096, 1024, B0
    for scratch in (True, False):
        for p in (0.0, 0.5):
            a = _stream_feed(name, L, ysz, B, p, 0, scratch=scratch)
            b = _live(name, L, ysz, B, p, scratch=scratch)
            for k in ("x", "y", "kn", "meta"):
                assert torch.equal(a[k], b[k]), (name, scratch, p, k)


# ---- 2. recorded rows against the library's entries on the extended span
@pytest.mark.parametrize("L,ysz,preroll", SHAPES)
@pytest.mark.parametrize("name", ["Compressor_4c", "Compressor", "LowPass", "Echo", "Denoise", "DeCompressor_4c", "Comp_Just_Thresh"])
def test_recorded_rows(name, L, ysz, preroll):
    B = B0
    draw = _draw(L, B, 0.0)
    f, st, fl = draw[1:]
    R = _history(L, B, preroll)
    full, part, none = R == preroll, (R > 0) & (R < preroll), R == 0
    # the cases are there before anything is compared: histories of every kind, every alignment, file and polarity, both polarities with a full history
    assert (int(full.sum()), int(part.sum()), int(none.sum())) == COVERAGE[(L, preroll)]
    assert set(st % 4) == {0, 1, 2, 3} and set(f) == {0, 1, 2} and set(fl) == {0, 1} and set(fl[full]) == {0, 1}
    assert np.all(R % 4 == 0) and np.all(R <= st) and R.max() + L > 8192
    r = _stream_feed(name, L, ysz, B, 0.0, preroll)
    live = _live(name, L, ysz, B, 0.0)
    assert all(np.array_equal(a, b) for a, b in zip(r["meta"].cpu().numpy().T, draw))
    assert torch.equal(r["kn"], live["kn"])
    assert bool(torch.isfinite(r["x"]).all()) and bool(torch.isfinite(r["y"]).all()) and bool(torch.isfinite(r["kn"]).all())
    if name == "Denoise":
        assert torch.equal(r["x"], live["x"]) and torch.equal(r["y"], live["y"])
        return
    assert r["rr"].cpu().numpy().tolist() == R.tolist()
    kw = r["kw"]
    assert bool(torch.isfinite(kw).all())
    if name == "Echo":
        assert len(set(kw[:, 2].tolist())) > 1 and torch.equal(kw[:, 0], kw[:, 0].round())
    ifull = torch.from_numpy(np.flatnonzero(full)).cuda()
    if name == "DeCompressor_4c":
        assert torch.equal(r["y"], live["y"])                    # the clean tail
        assert torch.equal(r["x"], _entry_tail(name, L, ysz, R, kw, L))
        assert not torch.equal(r["x"][ifull], live["x"][ifull])  # the history is live
        c4 = _stream_feed("Compressor_4c", L, ysz, B, 0.0, preroll)
        assert torch.equal(kw, c4["kw"]) and torch.equal(r["x"][:, -ysz:], c4["y"])
        return
    assert torch.equal(r["x"], live["x"])
    assert torch.equal(r["y"], _entry_tail(name, L, ysz, R, kw, ysz))
    # Two effects forget the history before the usual tail begins, and then st_lowpass / st_echo on xe, the reference above, give the live feed's tail bit
    # for bit.  The low-pass's slowest mode decays by exp(-pi fc / sr) per sample: over the L - ysz samples in front of the tail to below half a float32 ulp
    # of y unless fc < 76 Hz (L = 4096) or 38 Hz (L = 8192), and none of these rows' cutoffs of [10, 2000] Hz is that low.  The echo reaches back
    # echoes * delay + 1 <= 3 * 1500 + 1 samples (ECHO_WIDE): not in front of the window where the tail starts at 6144.  For these the history shows where
    # the effect still sees it, at the head of the window: ysz = L, against the entry on xe like every other row.
    if name == "LowPass" or (name == "Echo" and L - ysz > 3 * 1500 + 1):
        rl, ll = _stream_feed(name, L, L, B, 0.0, preroll), _live(name, L, L, B, 0.0)
        assert torch.equal(rl["y"], _entry_tail(name, L, L, R, rl["kw"], L)) and torch.equal(rl["kw"], kw) and torch.equal(rl["y"][:, -ysz:], r["y"])
        heard = [b for b in np.flatnonzero(full) if name != "Echo" or float(kw[b, 2]) >= 1]      # an echo count of 0 is no effect at all
        assert len(heard) >= 4 and all(not torch.equal(rl["y"][b], ll["y"][b]) for b in heard)
    else:
        assert not torch.equal(r["y"][ifull], live["y"][ifull])  # the history is live
    inone = torch.from_numpy(np.flatnonzero(none)).cuda()
    assert torch.equal(r["y"][inone], live["y"][inone])          # no history: the live feed's row


# ---- 3. the whole file in front of the window
@pytest.mark.parametrize("name", ["Compressor_4c", "LowPass"])
def test_whole_file_history(name):
    L, ysz, B = 4096, 1024, B0
    _, f, st, fl = _draw(L, B, 0.0)
    assert st.max() < WHOLE
    R = st & ~3
    r = _stream_feed(name, L, ysz, B, 0.0, WHOLE)
    assert r["rr"].cpu().numpy().tolist() == R.tolist()
    P = _pool(L)
    entry, k = ("st_compressor_4c", 4) if name == "Compressor_4c" else ("st_lowpass", 1)
    for b in range(B):                                           # file[start & 3 : start + L] through the entry
        lo, hi = int(P["off"][f[b]] + (st[b] & 3)), int(P["off"][f[b]] + st[b] + L)
        xe = (P["f32"][lo:hi] * (-1.0 if fl[b] else 1.0))[None, :].contiguous()
        assert torch.equal(r["y"][b:b + 1], _call(entry, xe, r["kw"][b:b + 1, :k], ysz)), (name, b)
    assert torch.equal(r["x"], _live(name, L, ysz, B, 0.0)["x"])


# ---- 4. pool format and batching
@pytest.mark.parametrize("name", ["Compressor_4c", "Compressor", "DeCompressor_4c"])
def test_pool_format_and_batching(name):
    L, ysz, preroll, B = 4096, 1024, 8192, B0
    whole = _stream_feed(name, L, ysz, B, 0.0, preroll)
    f32 = _stream_feed(name, L, ysz, B, 0.0, preroll, pcm="f32")
    parts = [_stream_feed(name, L, ysz, 5, 0.0, preroll), _stream_feed(name, L, ysz, 27, 0.0, preroll, first=FIRST + 5)]
    for k in ("x", "y", "kn", "meta", "kw", "rr"):
        assert torch.equal(whole[k], f32[k]), (name, k, "pool format")
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts])), (name, k, "batching")


def test_window_index_beyond_32_bits():
    L, ysz, preroll, B, first = 4096, 1024, 8192, 16, 2 ** 32 + 5
    r = _stream_feed("Compressor_4c", L, ysz, B, 0.0, preroll, first=first)
    draw = _draw(L, B, 0.0, first=first)
    assert all(np.array_equal(a, b) for a, b in zip(r["meta"].cpu().numpy().T, draw))
    R = np.minimum(preroll, draw[2] & ~3)
    assert r["rr"].cpu().numpy().tolist() == R.tolist() and R.max() > 0
    P = _pool(L)
    for b in range(B):
        lo, hi = int(P["off"][draw[1][b]] + draw[2][b] - R[b]), int(P["off"][draw[1][b]] + draw[2][b] + L)
        xe = (P["f32"][lo:hi] * (-1.0 if draw[3][b] else 1.0))[None, :].contiguous()
        assert torch.equal(r["y"][b:b + 1], _call("st_compressor_4c", xe, r["kw"][b:b + 1], ysz)), b
    low = _stream_feed("Compressor_4c", L, ysz, B, 0.0, preroll, first=5)
    assert not torch.equal(low["meta"], r["meta"]) and not torch.equal(low["x"], r["x"])      # not the alias of its low word


# ---- 5. a mixed batch
@pytest.mark.parametrize("name", ["Compressor_4c", "DeCompressor_4c"])
def test_mixed_batch(name):
    L, ysz, preroll, B = 4096, 1024, 8192, B0
    mix = _stream_feed(name, L, ysz, B, 0.5, preroll)
    rec = _stream_feed(name, L, ysz, B, 0.0, preroll)
    syn = _synth(name, L, ysz, B)
    draw = _draw(L, B, 0.5)
    assert all(np.array_equal(a, b) for a, b in zip(mix["meta"].cpu().numpy().T, draw))
    is_syn = torch.from_numpy(draw[0] == 1).cuda()
    R = _history(L, B, preroll)
    assert 0 < int(is_syn.sum()) < B and (R[draw[0] == 0] == preroll).any() and ((R[draw[0] == 0] > 0) & (R[draw[0] == 0] < preroll)).any()
    assert mix["rr"].cpu().numpy().tolist() == np.where(draw[0] == 1, -1, R).tolist()
    for k in ("x", "y", "kn"):
        assert torch.equal(mix[k][is_syn], syn[k][is_syn]), (name, k, "synthetic rows")
        assert torch.equal(mix[k][~is_syn], rec[k][~is_syn]), (name, k, "recorded rows")
    assert torch.equal(mix["kw"][~is_syn], rec["kw"][~is_syn])


# ---- 6. the history does what it is for
def test_history_brings_the_target_to_the_streamed_one():
    """Rows with start >= 8192: the deviation of y from the whole-file-history y with 8192 samples of history against none.  Only the ordering is asserted;
    the 4-control compressor's state contracts by at most exp(-ln 9 * 8192 / (44100 * 0.04)) ~ 3.7e-5 over 8192 steps (its slowest default time, 40 ms)."""
    L, ysz, B = 4096, 1024, B0
    st = _draw(L, B, 0.0)[2]
    rows = torch.from_numpy(np.flatnonzero(st >= 8192)).cuda()
    assert len(rows) >= 4
    ref = _stream_feed("Compressor_4c", L, ysz, B, 0.0, WHOLE)["y"][rows]
    err = {P: float((_stream_feed("Compressor_4c", L, ysz, B, 0.0, P)["y"][rows] - ref).abs().max()) for P in (0, 8192)}
    print("err(0) =", err[0], "err(8192) =", err[8192])
    assert err[0] > 0 and err[8192] < err[0]


# ---- 7. the Python layers
def test_dataset_loader_and_entry_agree(tmp_path):
    from signaltrain_amd import _lib, audio, datasets
    np.random.seed(3); torch.manual_seed(3)
    root = str(tmp_path / "rec")
    make_input_dataset(root, n=3 * 8192)
    fx = audio.Compressor_4c()
    L, ysz, B, preroll = 8192, 2048, 16, 1024
    ds = datasets.AudioInputDataSet(L, fx, path=root + "/Train/", datapoints=64, y_size=ysz, preroll=preroll)
    x, y, kn, meta = ds.batch_device(B, with_meta=True)
    assert ds._feed_count == B and x.shape == (B, L) and y.shape == (B, ysz) and kn.shape == (B, 4)
    # a direct call of the entry at the same (seed, window index)
    lib, d, t = _lib.load(), ds._fdev[("cuda:0", "s16")], ds.feed_tables()
    rng = fx.feed_ranges()
    lo = (C.c_float * 4)(*[float(v) for v in rng[:, 0]]); hi = (C.c_float * 4)(*[float(v) for v in rng[:, 1]])
    x2 = torch.empty_like(x); y2 = torch.empty_like(y); kn2 = torch.empty_like(kn); meta2 = torch.empty_like(meta)
    scr = torch.empty(int(lib.st_live_feed_stream_scratch_floats(fx.feed_fx, B, L, preroll, 0.0)), device="cuda")
    _lib.check(lib.st_live_feed_stream(fx.feed_fx, _lib.family_mask(ds.choosers), 0.0, preroll, ds._feed_seed, 0, B, L, ysz, 4, 44100.0, lo, hi, 1, _lib.PCM_S16,
                                       _lib.ptr(d["x"]), _lib.ptr(d["off"]), _lib.ptr(d["len"]), 2, t["min_len"], t["pool_samples"],
                                       _lib.ptr(x2), _lib.ptr(y2), _lib.ptr(kn2), _lib.ptr(meta2), _lib.ptr(scr), _stream()), "st_live_feed_stream")
    torch.cuda.synchronize()
    assert torch.equal(x, x2) and torch.equal(y, y2) and torch.equal(kn, kn2) and torch.equal(meta, meta2)
    assert int((meta[:, 2] >= 4).sum()) > 0                      # some row has a history
    plain = datasets.AudioInputDataSet(L, fx, path=root + "/Train/", datapoints=64, y_size=ysz)
    plain._feed_seed = ds._feed_seed
    xp, yp, knp = plain.batch_device(B)
    assert torch.equal(xp, x) and torch.equal(knp, kn) and not torch.equal(yp, y)
    batches = list(datasets.DeviceLiveLoader(ds, 16, "cuda:0", gen_windows=32))
    torch.cuda.synchronize()
    assert len(batches) == 64 // 16 and ds._feed_count == B + 64
    assert all(b[0].shape == (16, L) and b[1].shape == (16, ysz) and bool(torch.isfinite(b[1]).all()) for b in batches)


def test_train_on_recorded_input_with_preroll(tmp_path, monkeypatch):
    from signaltrain_amd import audio, datasets, nn_proc, train
    nn_proc._QUIET = True
    root = str(tmp_path / "rec")
    make_input_dataset(root, n=3 * 8192)
    made = []
    live = datasets.AudioInputDataSet.batch_device

    def counting(self, B, *a, **kw):
        out = live(self, B, *a, **kw); made.append((os.path.basename(self.path.rstrip("/")), B, self.preroll)); return out
    monkeypatch.setattr(datasets.AudioInputDataSet, "batch_device", counting)
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0); np.random.seed(0)
    train.train(effect=audio.Compressor_4c(), epochs=1, n_data_points=256, batch_size=64, device=torch.device("cuda:0"), input_path=root, preroll=1024, lr_max=2e-4)
    assert sum(B for p, B, _ in made if p == "Train") == 256 and sum(B for p, B, _ in made if p == "Val") == 64
    assert all(pr == 1024 for _, _, pr in made)                  # the training and the validation set both carry the history
    lines = [l.split() for l in open("vl_avg_out.dat").read().strip().splitlines()]
    assert len(lines) == 1 and np.isfinite(float(lines[0][-1]))
