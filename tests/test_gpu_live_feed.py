"""GPU: the feed of recorded input through a live effect (st_live_feed, csrc/st_feed_live.h).  Synthetic rows are st_synth_effect_families' bit for
bit; recorded rows are the pool's spans at the draws of datasets.live_feed_draw, with targets the library's own effect entries reproduce on (x, the
window's world knobs) -- the comparisons tests/test_gpu_effects.py, test_gpu_lowpass_denoise.py and test_gpu_echo_decomp.py make for the synthetic
feed; a mixed batch is row by row one or the other; a window is a function of (seed, window index); and the dataset, loader and train() on top."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests.test_live_feed_host import MIX_B, MIX_FIRST, MIX_P, MIX_SEED, make_input_dataset, pool_lengths

pytestmark = pytest.mark.gpu
SR = 44100.0
ECHO_WIDE = np.array([[100, 1500], [0.1, 0.9], [0, 3], [0, 0]], dtype=np.float64)      # fractional world delays and echo counts: the feed's rounding is live
ECHO_FAMILIES = (1, 3, 5, 6, 7)
SHAPES = [(4096, 1024), (8192, 2048)]      # two chunks of the envelope and low-pass scans (their carry crosses a chunk edge), and the training window
SEED, FIRST, B0 = 99, 700, 32


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _effect(name):
    """(ST_FX id, K, the four knob rows of the feed) of an effect class"""
    from signaltrain_amd import audio
    fx = getattr(audio, name)()
    return fx.feed_fx, len(fx.knob_names), (ECHO_WIDE if name == "Echo" else fx.feed_ranges())


@functools.lru_cache(maxsize=None)
def _pool(L):
    """The three files of pool_lengths(L) as one int16 pool and the float32 pool of the same samples, with their tables (shared, never written)."""
    ln = np.array(pool_lengths(L), dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
    assert off[1] % 2 == 1 and ln[1] % 2 == 1
    s16 = np.random.default_rng(L).integers(-32768, 32768, int(ln.sum())).astype(np.int16)
    f32 = np.array(s16 / 32767.0, dtype=np.float32)
    return {"len": ln, "off": off, "s16": torch.from_numpy(s16).cuda(), "f32": torch.from_numpy(f32).cuda(),
            "d_len": torch.from_numpy(ln).cuda(), "d_off": torch.from_numpy(off).cuda()}


def _live(name, L, ysz, B, p, pcm="s16", scratch=True, first=FIRST, seed=SEED, families=None, augment=1):
    """st_live_feed -> dict(x, y, kn, meta, scr)"""
    from signaltrain_amd import _lib
    lib = _lib.load()
    fx, K, rng = _effect(name)
    P = _pool(L)
    x = torch.full((B, L), float("nan"), device="cuda"); y = torch.full((B, ysz), float("nan"), device="cuda"); kn = torch.full((B, K), float("nan"), device="cuda")
    meta = torch.full((B, 4), -7, dtype=torch.int64, device="cuda")
    lo = (C.c_float * 4)(*[float(v) for v in rng[:, 0]]); hi = (C.c_float * 4)(*[float(v) for v in rng[:, 1]])
    scr = torch.zeros(int(lib.st_live_feed_scratch_floats(fx, B, L, p)), device="cuda") if scratch else None
    _lib.check(lib.st_live_feed(fx, _lib.family_mask(families), p, seed, first, B, L, ysz, K, SR, lo, hi, augment, _lib.PCM_S16 if pcm == "s16" else _lib.PCM_F32,
                                _lib.ptr(P[pcm]), _lib.ptr(P["d_off"]), _lib.ptr(P["d_len"]), 3, int(P["len"].min()), int(P["len"].sum()),
                                _lib.ptr(x), _lib.ptr(y), _lib.ptr(kn), _lib.ptr(meta), _lib.ptr(scr), _stream()), "st_live_feed")
    torch.cuda.synchronize()
    return {"x": x, "y": y, "kn": kn, "meta": meta, "scr": scr}


def _synth(name, L, ysz, B, scratch=True, first=FIRST, seed=SEED, families=None, augment=1):
    """st_synth_effect_families -> dict(x, y, kn)"""
    from signaltrain_amd import _lib
    lib = _lib.load()
    fx, K, rng = _effect(name)
    x = torch.empty(B, L, device="cuda"); y = torch.empty(B, ysz, device="cuda"); kn = torch.empty(B, K, device="cuda")
    lo = (C.c_float * 4)(*[float(v) for v in rng[:, 0]]); hi = (C.c_float * 4)(*[float(v) for v in rng[:, 1]])
    scr = torch.zeros(int(lib.st_synth_effect_scratch_floats(fx, B, L)), device="cuda") if scratch else None
    _lib.check(lib.st_synth_effect_families(fx, _lib.family_mask(families), seed, first, B, L, ysz, K, SR, lo, hi, augment, -1, None,
                                            _lib.ptr(x), _lib.ptr(y), _lib.ptr(kn), _lib.ptr(scr), _stream()), "st_synth_effect_families")
    torch.cuda.synchronize()
    return {"x": x, "y": y, "kn": kn}


def _draw(L, B, p, first=FIRST, seed=SEED, augment=True):
    from signaltrain_amd.datasets import live_feed_draw
    w = np.arange(B, dtype=np.uint64) + np.uint64(first)
    return live_feed_draw(seed, w, _pool(L)["len"], L, p, augment)


def _spans(L, B, first=FIRST, seed=SEED, augment=True):
    """The recorded windows the replica's draws name: pool spans times the sign, [B][L] on the device"""
    P = _pool(L)
    _, f, st, fl = _draw(L, B, 0.0, first, seed, augment)
    base = torch.from_numpy(P["off"][f] + st).cuda()
    sign = torch.from_numpy(np.where(fl == 1, -1.0, 1.0).astype(np.float32)).cuda()
    return P["f32"][base[:, None] + torch.arange(L, device="cuda")[None, :]] * sign[:, None]


def _call(entry, x, kw, ysz):
    """A library effect entry (x [B][L], world knobs [B][k]) -> y [B][ysz]"""
    from signaltrain_amd import _lib
    x, kw = x.contiguous(), kw.to(torch.float32).contiguous()
    y = torch.empty(x.shape[0], ysz, device="cuda")
    _lib.check(getattr(_lib.load(), entry)(_lib.ptr(x), _lib.ptr(kw), SR, x.shape[0], x.shape[1], ysz, _lib.ptr(y), _stream()), entry)
    return y


def _world_knobs(r, B, L):
    """The world knobs the feed left in the scratch, [B][4]"""
    return r["scr"][B * L:B * L + 4 * B].reshape(B, 4).clone()


# ---- 1. synth_prob = 1: the synthetic feed's rows
@pytest.mark.parametrize("name,families,scratch", [("Compressor_4c", None, True), ("LowPass", ECHO_FAMILIES, False), ("DeCompressor_4c", None, True),
                                                   ("DeCompressor_4c", (0, 1, 3, 4, 6, 10, 2, 7, 9), False)])
def test_all_synthetic_is_the_synthetic_feed(name, families, scratch):
    L, ysz, B = 8192, 2048, 16
    r = _live(name, L, ysz, B, 1.0, scratch=scratch, families=families)
    s = _synth(name, L, ysz, B, scratch=scratch, families=families)
    for k in ("x", "y", "kn"):
        assert torch.equal(r[k], s[k]), (name, k)
    assert r["meta"][:, 0].tolist() == [1] * B
    assert all(np.array_equal(a, b) for a, b in zip(r["meta"].cpu().numpy().T, _draw(L, B, 1.0)))      # file, start and polarity are drawn all the same


# ---- 2. synth_prob = 0: recorded rows
@pytest.mark.parametrize("L,ysz", SHAPES)
@pytest.mark.parametrize("name", ["Compressor_4c", "Compressor", "LowPass", "Echo", "Denoise", "DeCompressor_4c", "Comp_Just_Thresh"])
def test_recorded_rows(name, L, ysz):
    from signaltrain_amd import _lib, audio
    B = B0
    fx, K, rng = _effect(name)
    r = _live(name, L, ysz, B, 0.0)
    x, y, kn = r["x"], r["y"], r["kn"]
    # the draws, and the window itself
    draw = _draw(L, B, 0.0)
    assert all(np.array_equal(a, b) for a, b in zip(r["meta"].cpu().numpy().T, draw))
    f, st, fl = draw[1:]
    base = _pool(L)["off"][f] + st
    assert set(f) == {0, 1, 2} and set(fl) == {0, 1} and set(base % 4) == {0, 1, 2, 3}      # every file, both polarities, spans at every alignment down to the element's
    clean = _spans(L, B)
    assert kn.shape == (B, K) and float(kn.min()) >= -0.5 and float(kn.max()) <= 0.5 and len(set(kn[:, 0].tolist())) == B
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all())
    # the pool format changes nothing
    rf = _live(name, L, ysz, B, 0.0, pcm="f32")
    for k in ("x", "y", "kn", "meta"):
        assert torch.equal(r[k], rf[k]), (name, k)
    # the in-workgroup form of the effect
    rk = _live(name, L, ysz, B, 0.0, scratch=False)
    for k in ("x", "y", "kn", "meta"):
        assert torch.equal(r[k], rk[k]), (name, k)
    # the knobs do not depend on the effect: the first draws of the window's first sequence
    assert torch.equal(kn, _live("Compressor_4c", L, ysz, B, 0.0, scratch=False)["kn"][:, :K])
    if name in ("Compressor_4c", "Comp_Just_Thresh"):
        kw = _world_knobs(r, B, L)
        assert torch.equal(x, clean) and torch.equal(y, _call("st_compressor_4c", x, kw, ysz)) and not torch.equal(y, x[:, -ysz:])
        if name == "Comp_Just_Thresh":                           # K < 4: the knobs past K are fixed at their low end
            assert torch.equal(kw[:, 1:], torch.tensor([[3.0, 0.05, 1.0]], device="cuda").expand(B, 3))
        else:
            ref = audio._knobs_wc_device(audio.Compressor_4c().knob_ranges, kn, "cuda").to(torch.float32)
            assert torch.allclose(kw, ref, rtol=1e-5, atol=1e-5)        # Effect.knobs_wc, to the rounding of float32
    elif name == "Compressor":
        kw = _world_knobs(r, B, L)
        assert torch.equal(x, clean) and torch.equal(y, _call("st_compressor", x, kw[:, :3], ysz)) and not torch.equal(y, x[:, -ysz:])
    elif name == "LowPass":
        kw = audio._knobs_wc_device(audio.LowPass().knob_ranges, kn, "cuda")
        assert torch.equal(x, clean) and torch.equal(y, _call("st_lowpass", x, kw[:, :1], ysz)) and not torch.equal(y, x[:, -ysz:])
    elif name == "Echo":
        kw = audio._knobs_wc_device(ECHO_WIDE[:3], kn, "cuda")
        kw = torch.stack([kw[:, 0].round(), kw[:, 1], kw[:, 2].round()], 1)
        assert torch.equal(x, clean) and torch.equal(y, _call("st_echo", x, kw, ysz)) and not torch.equal(y, x[:, -ysz:])
        assert len(set(kw[:, 2].tolist())) > 1
    elif name == "Denoise":
        s = audio._knobs_wc_device(audio.Denoise().knob_ranges, kn, "cuda").to(torch.float32).contiguous()
        noisy = torch.empty_like(clean)
        _lib.check(_lib.load().st_denoise_input(SEED, FIRST, _lib.ptr(clean.contiguous()), _lib.ptr(s), B, L, _lib.ptr(noisy), _stream()), "st_denoise_input")
        assert torch.equal(y, clean[:, -ysz:]) and torch.equal(x, noisy) and not torch.equal(x, clean)
    else:
        kw = _world_knobs(r, B, L)
        assert torch.equal(y, clean[:, -ysz:]) and torch.equal(x, _call("st_compressor_4c", clean, kw, L)) and not torch.equal(x, clean)
        c4 = _live("Compressor_4c", L, ysz, B, 0.0)
        assert torch.equal(kw, _world_knobs(c4, B, L)) and torch.equal(x[:, -ysz:], c4["y"])      # the inverse problem of ST_FX_COMP4C's


def test_recorded_rows_without_augment_are_never_flipped():
    L, ysz, B = 4096, 1024, 16
    r = _live("LowPass", L, ysz, B, 0.0, augment=0)
    assert r["meta"][:, 3].tolist() == [0] * B and torch.equal(r["x"], _spans(L, B, augment=False))
    a = _live("LowPass", L, ysz, B, 0.0, augment=1)
    assert torch.equal(a["meta"][:, :3], r["meta"][:, :3]) and torch.equal(a["kn"], r["kn"]) and torch.equal(a["x"].abs(), r["x"].abs())


def test_long_window_needs_no_scratch():
    """65536 samples: eight chunks of the in-workgroup compressor, no scratch of any kind while no window is synthetic."""
    L, ysz, B = 65536, 16384, 4
    r = _live("Compressor_4c", L, ysz, B, 0.0, scratch=False)
    assert torch.equal(r["x"], _spans(L, B)) and all(np.array_equal(a, b) for a, b in zip(r["meta"].cpu().numpy().T, _draw(L, B, 0.0)))
    s = _live("Compressor_4c", L, ysz, B, 0.0, scratch=True)
    assert s["scr"].numel() == B * (L + 4) and torch.equal(r["y"], s["y"]) and torch.equal(r["kn"], s["kn"])
    assert torch.equal(r["y"], _call("st_compressor_4c", r["x"], _world_knobs(s, B, L), ysz))


# ---- 3. a mixed batch
@pytest.mark.parametrize("name,scratch", [("Compressor_4c", True), ("Compressor_4c", False), ("Compressor", True), ("DeCompressor_4c", True), ("DeCompressor_4c", False),
                                          ("LowPass", False), ("Denoise", False)])
def test_mixed_batch_rows_are_one_or_the_other(name, scratch):
    L, ysz, B = 8192, 2048, MIX_B
    kw = dict(first=MIX_FIRST, seed=MIX_SEED, scratch=scratch)
    mix = _live(name, L, ysz, B, MIX_P, **kw)
    syn = _live(name, L, ysz, B, 1.0, **kw)
    rec = _live(name, L, ysz, B, 0.0, **kw)
    draw = _draw(L, B, MIX_P, first=MIX_FIRST, seed=MIX_SEED)
    assert all(np.array_equal(a, b) for a, b in zip(mix["meta"].cpu().numpy().T, draw))
    is_syn = torch.from_numpy(draw[0] == 1).cuda()
    assert 0 < int(is_syn.sum()) < B
    for k in ("x", "y", "kn"):
        assert torch.equal(mix[k][is_syn], syn[k][is_syn]), (name, k, "synthetic rows")
        assert torch.equal(mix[k][~is_syn], rec[k][~is_syn]), (name, k, "recorded rows")
    assert not torch.equal(syn["x"][~is_syn], rec["x"][~is_syn])


# ---- 4. batching
@pytest.mark.parametrize("first", [MIX_FIRST, 2 ** 32 + 5])
def test_a_window_is_a_function_of_its_index(first):
    L, ysz, B = 4096, 1024, 32
    whole = _live("Compressor_4c", L, ysz, B, 0.5, first=first)
    parts = [_live("Compressor_4c", L, ysz, B // 2, 0.5, first=first + i * (B // 2)) for i in (0, 1)]
    for k in ("x", "y", "kn", "meta"):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts])), k
    assert all(np.array_equal(a, b) for a, b in zip(whole["meta"].cpu().numpy().T, _draw(L, B, 0.5, first=first)))
    assert 0 < int(whole["meta"][:, 0].sum()) < B
    if first >= 2 ** 32:                                         # not the alias of its low word
        low = _live("Compressor_4c", L, ysz, B, 0.5, first=first - 2 ** 32)
        assert not torch.equal(low["meta"], whole["meta"]) and not torch.equal(low["x"], whole["x"])


# ---- 5. the Python layers
def test_dataset_loader_and_one_training_step(tmp_path):
    from signaltrain_amd import audio, datasets, nn_proc
    nn_proc._QUIET = True
    np.random.seed(3); torch.manual_seed(3)
    root = str(tmp_path / "rec")
    make_input_dataset(root, n=3 * 8192)
    fx = audio.Compressor_4c()
    ds = datasets.AudioInputDataSet(8192, fx, path=root + "/Train/", datapoints=64, y_size=2048, synth_prob=0.25)
    x, y, kn, meta = ds.batch_device(16, with_meta=True)
    assert ds._feed_count == 16 and x.shape == (16, 8192) and y.shape == (16, 2048) and kn.shape == (16, 4) and x.is_cuda
    draw = datasets.live_feed_draw(ds._feed_seed, np.arange(16), ds.feed_tables()["len"], 8192, 0.25, True)
    assert all(np.array_equal(a, b) for a, b in zip(meta.cpu().numpy().T, draw))
    rec = torch.from_numpy(draw[0] == 0).cuda()
    # the dataset hands the effect's own ranges to the feed: the targets are the effect's at these knobs, to the float32 rounding of the world knobs
    # (1e-5 of max(1e-3, max |ref|): the bound between a device effect and its reference elsewhere in the suite)
    ref = fx.go_device(x, kn, 2048)
    assert 0 < int(rec.sum()) and float((y - ref).abs().max()) <= 1e-5 * max(1e-3, float(ref.abs().max()))
    xf = ds.batch_device(16, pcm="f32")[0]
    assert ds._feed_count == 32 and not torch.equal(xf, x)       # the stream went on
    model = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=4, sr=44100).to("cuda")
    eng = model.engine(torch.zeros(16, 8192, device="cuda"))
    loss = float(eng.train_step(x, kn, y, 1e-4)[0])
    assert np.isfinite(loss) and loss > 0
    batches = list(datasets.DeviceLiveLoader(ds, 16, "cuda:0", gen_windows=32))
    assert len(batches) == 64 // 16 and ds._feed_count == 32 + 64
    assert all(b[0].shape == (16, 8192) and b[1].shape == (16, 2048) and b[2].shape == (16, 4) for b in batches)
    torch.cuda.synchronize()
    assert not torch.equal(batches[0][0], batches[1][0]) and all(bool(torch.isfinite(b[1]).all()) for b in batches)


def test_train_on_recorded_input(tmp_path, monkeypatch):
    from signaltrain_amd import audio, datasets, misc, nn_proc, train
    nn_proc._QUIET = True
    root = str(tmp_path / "rec")
    make_input_dataset(root, n=3 * 8192)
    made = []
    live = datasets.AudioInputDataSet.batch_device

    def counting(self, B, *a, **kw):
        out = live(self, B, *a, **kw); made.append((os.path.basename(self.path.rstrip("/")), B)); return out
    monkeypatch.setattr(datasets.AudioInputDataSet, "batch_device", counting)
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0); np.random.seed(0)
    fx = audio.Compressor_4c()
    train.train(effect=fx, epochs=1, n_data_points=256, batch_size=64, device=torch.device("cuda:0"), input_path=root, synth_prob=0.25, lr_max=2e-4)
    assert sum(B for p, B in made if p == "Train") == 256 and sum(B for p, B in made if p == "Val") == 64      # every window came out of the live feed
    lines = [l.split() for l in open("vl_avg_out.dat").read().strip().splitlines()]
    assert len(lines) == 1 and np.isfinite(float(lines[0][-1]))
    sd, rv = misc.load_checkpoint("modelcheckpoint.tar", device="cpu")
    assert rv["effect_name"] == fx.name and list(rv["knob_names"]) == fx.knob_names and np.array_equal(rv["knob_ranges"], fx.knob_ranges)
    assert all(torch.isfinite(v).all() for v in sd.values())
