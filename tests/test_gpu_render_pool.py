"""GPU: st_render_pool (csrc/st_render_pool.h) -- a folder of recordings, one concatenated pool, WHOLE through an effect at one knob setting per file in one
call.  The yardstick is the library's own effect entries (st_compressor_4c, st_compressor, st_lowpass, st_echo, st_denoise_input; existing goldens and float64
restatements pin them to the reference), run per file with B = 1 on a zero-padded aligned copy: the render must give their bits.  One check goes past sibling
device code: the 4-control compressor's pool against audio.compressor_4controls on the host."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from signaltrain_amd import _lib

pytestmark = pytest.mark.gpu
SR = 44100.0
LL = C.POINTER(C.c_longlong)
SENTINEL = -7777.0
RAGGED = [1, 3, 64, 2049, 8193, 0, 8200, 4097]         # across ENV_CH = LP_CH = 2048 and COMP_CH = 8192, an empty file among them
FX_ALL = [_lib.FX_COMP4C, _lib.FX_COMP, _lib.FX_LOWPASS, _lib.FX_DENOISE, _lib.FX_ECHO, _lib.FX_DECOMP4C]
NK = {_lib.FX_COMP4C: 4, _lib.FX_COMP: 3, _lib.FX_LOWPASS: 1, _lib.FX_DENOISE: 1, _lib.FX_ECHO: 3, _lib.FX_DECOMP4C: 4}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def layout(lens):
    """Offsets with every residue mod 4 and gaps of 1..7 samples in front of every file; returns (off, pool_samples)."""
    off, pos = [], 0
    for f, n in enumerate(lens):
        gap = 1 + (f % 4 - (pos + 1)) % 4                 # 1..4, so that off % 4 == f % 4
        if f % 3 == 2:
            gap += 4 if gap <= 3 else 0                   # ... and some of 5..7
        pos += gap
        off.append(pos); pos += n
    off = np.array(off, np.int64)
    assert (len(lens) < 4 or set(off[:4] % 4) == {0, 1, 2, 3}) and all(1 <= off[f] - (off[f - 1] + lens[f - 1] if f else 0) <= 7 for f in range(len(lens)))
    return off, int(pos + 3)


def make_pool(lens, seed):
    """An int16 pool and its float32 image (s / 32767, the library's conversion), files of several levels with a silent stretch."""
    rng = np.random.default_rng(seed)
    off, total = layout(lens)
    s = np.zeros(total, np.int16)
    for f, n in enumerate(lens):
        v = rng.standard_normal(n) * (0.03 + 0.25 * ((f * 7) % 5) / 4)
        if n > 600:
            v[200:500] = 0.0
        s[off[f]:off[f] + n] = np.clip(np.rint(v * 32767.0), -32767, 32767).astype(np.int16)
    f32 = np.array(s / 32767.0, dtype=np.float32)          # as audio.read_audio_file converts (a tensor divided by a Python scalar is multiplied by its reciprocal)
    return off, total, torch.from_numpy(s).cuda(), torch.from_numpy(f32).cuda()


def knobs_for(fx, nfiles, seed):
    """World settings [nfiles][4] inside each effect's usual ranges (entries past the effect's count stay 0 and are not read)."""
    rng = np.random.default_rng(seed + 100 * fx)
    kw = np.zeros((nfiles, 4), np.float32)
    u = rng.random((nfiles, 4))
    if fx in (_lib.FX_COMP4C, _lib.FX_DECOMP4C):
        kw[:] = np.array([-30.0, 1.0, 1e-3, 1e-3]) + u * np.array([30.0, 4.0, 3.9e-2, 3.9e-2])
    elif fx == _lib.FX_COMP:
        kw[:, :3] = np.array([-30.0, 1.0, 1e-3]) + u[:, :3] * np.array([30.0, 4.0, 3.9e-2])
    elif fx == _lib.FX_LOWPASS:
        kw[:, 0] = 10.0 + u[:, 0] * 1990.0
    elif fx == _lib.FX_DENOISE:
        kw[:, 0] = 0.5 * u[:, 0]
    else:
        kw[:, 0] = np.array([1.0, 17.25, 5.0, 400.5, 2500.0, 33.0, 9000.0, 100.0])[np.arange(nfiles) % 8]      # whole and fractional delays, one beyond its file
        kw[:, 1] = 0.3 + 0.6 * u[:, 1]
        kw[:, 2] = np.arange(nfiles) % 9                                                                         # 0 .. ST_ECHO_MAX echoes
    return kw


def render(fx, pool, off, lens, kw, total, seed=0, first=0):
    lib = _lib.load()
    lens = np.asarray(lens, np.int64)
    n_scr = int(lib.st_render_pool_scratch_floats(fx, lens.ctypes.data_as(LL), len(lens)))
    assert (n_scr == 0) == (fx == _lib.FX_DENOISE)
    scr = torch.full((n_scr,), float("nan"), device="cuda") if n_scr else None
    out = torch.full((total,), SENTINEL, device="cuda")
    off_d, len_d, kw_d = torch.from_numpy(np.asarray(off, np.int64)).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(np.ascontiguousarray(kw, np.float32)).cuda()
    _lib.check(lib.st_render_pool(fx, SR, _lib.PCM_S16 if pool.dtype == torch.int16 else _lib.PCM_F32, _lib.ptr(pool), _lib.ptr(off_d), _lib.ptr(len_d), len(lens),
                                  int(lens.max()), total, _lib.ptr(kw_d), seed, first, _lib.ptr(out), _lib.ptr(scr), _stream()), "st_render_pool")
    torch.cuda.synchronize()
    return out


def entry(fx, xe, kw_row, seed=0, window=0):
    """The library's own entry on ONE file: xe the file's float32 samples (device), B = 1, L = ysz = len rounded up to the entry's multiple, zeros appended."""
    lib = _lib.load()
    n = xe.numel()
    Lp = -(-n // 4) * 4 if fx in (_lib.FX_LOWPASS, _lib.FX_DENOISE) else n
    x = torch.zeros(1, Lp, device="cuda"); x[0, :n] = xe
    kw = torch.from_numpy(np.ascontiguousarray(kw_row[:NK[fx]], np.float32)).cuda().reshape(1, -1)
    y = torch.empty(1, Lp, device="cuda")
    if fx == _lib.FX_DENOISE:
        _lib.check(lib.st_denoise_input(seed, window, _lib.ptr(x), _lib.ptr(kw), 1, Lp, _lib.ptr(y), _stream()), "st_denoise_input")
    else:
        name = {_lib.FX_COMP4C: "st_compressor_4c", _lib.FX_DECOMP4C: "st_compressor_4c", _lib.FX_COMP: "st_compressor", _lib.FX_LOWPASS: "st_lowpass", _lib.FX_ECHO: "st_echo"}[fx]
        _lib.check(getattr(lib, name)(_lib.ptr(x), _lib.ptr(kw), SR, 1, Lp, Lp, _lib.ptr(y), _stream()), name)
    return y[0, :n]


def bits(t):
    return t.contiguous().view(torch.int32)


def check_against_entries(fx, out, f32, off, lens, kw, total, seed=0, first=0):
    covered = torch.zeros(total, dtype=torch.bool, device="cuda")
    for f, n in enumerate(lens):
        covered[off[f]:off[f] + n] = True
        if n == 0:
            continue
        ref = entry(fx, f32[off[f]:off[f] + n], kw[f], seed, first + f)
        assert torch.equal(bits(out[off[f]:off[f] + n]), bits(ref)), (fx, f, n)
    assert bool((out[~covered] == SENTINEL).all()), fx                     # what lies between the spans is not touched


@pytest.mark.parametrize("fx", FX_ALL)
def test_ragged_pool_gives_the_entries_bits(fx):
    off, total, s16, f32 = make_pool(RAGGED, 5)
    kw = knobs_for(fx, len(RAGGED), 1)
    out = render(fx, f32, off, RAGGED, kw, total, seed=91, first=3)
    check_against_entries(fx, out, f32, off, RAGGED, kw, total, seed=91, first=3)
    out16 = render(fx, s16, off, RAGGED, kw, total, seed=91, first=3)
    assert torch.equal(bits(out16), bits(out))                             # the int16 pool gives the float32 pool's bits
    again = render(fx, f32, off, RAGGED, kw, total, seed=91, first=3)
    assert torch.equal(bits(again), bits(out))                             # a repeated call repeats its bits
    if fx != _lib.FX_ECHO:                                                 # (an echo beyond its file or a count of 0 leaves the file as it is)
        assert any(not torch.equal(out[off[f]:off[f] + n], f32[off[f]:off[f] + n]) for f, n in enumerate(RAGGED) if n > 2000), "the effect did something"


@pytest.mark.parametrize("fx", [_lib.FX_COMP4C, _lib.FX_DECOMP4C])
def test_wave_boundary(fx):
    """70 files of 5 .. 200 samples: the chain's 64-lane boundary and unequal lengths inside a wave."""
    lens = [int(v) for v in np.random.default_rng(70).integers(5, 201, size=70)]
    lens[3], lens[63], lens[64], lens[69] = 200, 5, 199, 64
    off, total, s16, f32 = make_pool(lens, 8)
    kw = knobs_for(fx, 70, 2)
    out = render(fx, s16, off, lens, kw, total)
    check_against_entries(fx, out, f32, off, lens, kw, total)


def test_echo_shorter_than_its_delay_and_without_echoes():
    lens = [300, 300, 5000, 40]
    off, total, s16, f32 = make_pool(lens, 9)
    kw = np.zeros((4, 4), np.float32)
    kw[:, :3] = [[1000.0, 0.7, 3.0], [50.0, 0.7, 0.0], [4999.5, 0.9, 8.0], [40.0, 0.5, 2.0]]
    out = render(_lib.FX_ECHO, f32, off, lens, kw, total)
    check_against_entries(_lib.FX_ECHO, out, f32, off, lens, kw, total)
    for f in (0, 1, 3):                                                    # every copy falls before the file / there is none: the file itself
        assert torch.equal(out[off[f]:off[f] + lens[f]], f32[off[f]:off[f] + lens[f]]), f
    assert not torch.equal(out[off[2]:off[2] + 5000], f32[off[2]:off[2] + 5000])


def test_denoise_first_file_beyond_32_bits():
    lens = [1000, 7, 4100]
    off, total, s16, f32 = make_pool(lens, 10)
    kw = knobs_for(_lib.FX_DENOISE, 3, 3)
    first = (1 << 32) + 12345
    out = render(_lib.FX_DENOISE, f32, off, lens, kw, total, seed=7, first=first)
    check_against_entries(_lib.FX_DENOISE, out, f32, off, lens, kw, total, seed=7, first=first)
    low = render(_lib.FX_DENOISE, f32, off, lens, kw, total, seed=7, first=12345)
    assert not torch.equal(out, low)                                       # the high word of the window index is part of the key


@pytest.mark.parametrize("fx,col,bad", [(_lib.FX_LOWPASS, 0, float("nan")), (_lib.FX_LOWPASS, 0, 30000.0), (_lib.FX_ECHO, 2, 9.0)])
def test_one_bad_setting_spoils_its_file_only(fx, col, bad):
    off, total, s16, f32 = make_pool(RAGGED, 11)
    kw = knobs_for(fx, len(RAGGED), 4)
    if fx == _lib.FX_ECHO:
        kw[:, 2] = np.minimum(kw[:, 2], 8)
    good = render(fx, f32, off, RAGGED, kw, total)
    kb = kw.copy(); kb[4, col] = bad
    out = render(fx, f32, off, RAGGED, kb, total)
    assert bool(torch.isnan(out[off[4]:off[4] + RAGGED[4]]).all())
    keep = torch.ones(total, dtype=torch.bool, device="cuda"); keep[off[4]:off[4] + RAGGED[4]] = False
    assert torch.equal(bits(out[keep]), bits(good[keep])) and not bool(torch.isnan(good[off[4]:off[4] + RAGGED[4]]).any())


def test_comp4c_pool_against_the_host_compressor():
    """Not through sibling device code: audio.compressor_4controls on the host per file, within the bound tests/test_gpu_effects.py applies between
    st_compressor_4c and that restatement."""
    from signaltrain_amd import audio
    off, total, s16, f32 = make_pool(RAGGED, 12)
    kw = knobs_for(_lib.FX_COMP4C, len(RAGGED), 5)
    out = render(_lib.FX_COMP4C, s16, off, RAGGED, kw, total).cpu().numpy().astype(np.float64)
    xh = f32.cpu().numpy()
    for f, n in enumerate(RAGGED):
        if n == 0:
            continue
        k = kw[f].astype(np.float64)
        ref = audio.compressor_4controls(xh[off[f]:off[f] + n], thresh=k[0], ratio=k[1], attackTime=k[2], releaseTime=k[3], sr=SR).astype(np.float64)
        assert np.abs(out[off[f]:off[f] + n] - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max()), f


# ---------------------------------------------------------------------------------------------- the Python layer
def write_inputs(root, lens=(9000, 8300, 10011), sub="Train", seed=0, pcm16=True):
    from signaltrain_amd import audio
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, sub), exist_ok=True)
    for i, n in enumerate(lens):
        t = np.arange(n) / SR
        x = 0.6 * np.sin(2 * np.pi * (110.0 * (i + 1)) * t) * np.exp(-3.0 * t) + 0.05 * rng.standard_normal(n)
        x = np.clip(np.rint(x * 32767.0), -32767, 32767).astype(np.int16) if pcm16 else x.astype(np.float32)
        audio.write_audio_file(os.path.join(root, sub, f"clip_{i}.wav"), x, int(SR))


@pytest.mark.parametrize("name,pcm16", [("Compressor_4c", True), ("LowPass", False), ("Echo", True), ("Denoise", True), ("DeCompressor_4c", False), ("Comp_Just_Thresh", True)])
def test_dataset_render_on_the_device(tmp_path, name, pcm16):
    from signaltrain_amd import audio, datasets
    e = getattr(audio, name)()
    write_inputs(str(tmp_path), pcm16=pcm16)
    ds_in = datasets.AudioInputDataSet(8192, e, sr=int(SR), path=str(tmp_path / "Train"), datapoints=8, y_size=2048)
    assert ds_in.feed_tables()["pcm"] == ("s16" if pcm16 else "f32")
    ds = ds_in.render(seed=4, device="cuda")
    kw, strs = datasets.render_knobs(e, 3, seed=4)
    assert np.array_equal(ds.knobs, kw.astype(np.float32)) and [os.path.basename(f) for f in ds.target_filenames] == datasets.render_names(e, strs)[1]
    rows = np.repeat(np.asarray(e.feed_ranges(), np.float64)[None, :, 0], 3, axis=0); rows[:, :kw.shape[1]] = kw
    if name == "Echo":
        rows[:, 0], rows[:, 2] = np.rint(rows[:, 0]), np.rint(rows[:, 2])
    inv = name in ("Denoise", "DeCompressor_4c")
    host = None if name == "Denoise" else ds_in.render(seed=4)
    for f in range(3):
        clean, proc = (ds.y[f], ds.x[f]) if inv else (ds.x[f], ds.y[f])
        assert np.array_equal(clean, ds_in.x[f])
        ref = entry(e.feed_fx, torch.from_numpy(ds_in.x[f]).cuda(), rows[f].astype(np.float32), seed=4, window=f).cpu().numpy()
        assert np.array_equal(proc.view(np.int32), ref.view(np.int32)), (name, f)
        if host is not None:                                               # the host effects: float64 restatements of the same laws
            hp = (host.x[f] if inv else host.y[f]).astype(np.float64)
            assert np.abs(proc - hp).max() <= 2e-6 * max(1.0, np.abs(hp).max()), (name, f)
        else:
            assert float(np.abs(proc - clean).max()) <= float(np.float32(kw[f, 0])) + 1e-6 and not np.array_equal(proc, clean)
    # the device cache evaluate() reads is the rendered pool
    d = ds._fdev[("cuda:%d" % torch.cuda.current_device(), "f32")]
    assert np.array_equal(d["x"].cpu().numpy(), np.concatenate(ds.x)) and np.array_equal(d["y"].cpu().numpy(), np.concatenate(ds.y))
    assert np.array_equal(d["kn"].cpu().numpy(), ds.feed_tables()["knobs"], equal_nan=True)      # (Echo's fixed knobs have no normalised value: 0 / 0)


def test_dataset_evaluate_equals_the_written_folder(tmp_path):
    from signaltrain_amd import audio, datasets, nn_proc
    nn_proc._QUIET = True
    e = audio.Compressor_4c()
    write_inputs(str(tmp_path / "in"))
    torch.manual_seed(0)
    m = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=4).cuda()
    L, y = m.in_chunk_size, m.out_chunk_size
    ds_in = datasets.AudioInputDataSet(L, e, sr=int(SR), path=str(tmp_path / "in" / "Train"), datapoints=8, y_size=y)
    rep = ds_in.evaluate(m, settings_per=2, seed=1, device="cuda", want_out=True)
    kw = datasets.render_knobs(e, 3, settings_per=2, seed=1)[0]
    assert np.array_equal(rep["knobs"], kw.astype(np.float32).astype(np.float64)) and rep["knobs"].shape == (3, 4)
    assert list(rep["n"]) == [len(a) - (L - y) for a in ds_in.x] and np.isfinite(rep["mae"]).all()
    out = str(tmp_path / "out")
    ds = ds_in.render(settings_per=2, seed=1, device="cuda")
    ds.write(out, "Train"); ds.write(out, "Val")
    back = datasets.AudioFileDataSet(L, audio.FileEffect(out, sr=int(SR)), sr=int(SR), path=out + "/Val/", datapoints=8, y_size=y, augment=False)
    rep2 = back.evaluate(m, device="cuda", pcm="f32", want_out=True)
    for k in ("n", "logcosh", "mae", "mse", "peak", "esr"):
        assert np.array_equal(rep[k], rep2[k]), k                           # the same pools through the same call
    assert rep["total"] == rep2["total"] and all(np.array_equal(a, b) for a, b in zip(rep["outputs"], rep2["outputs"]))


def test_train_prints_the_file_report_of_a_live_effect(tmp_path, capsys, monkeypatch):
    from signaltrain_amd import audio, nn_proc, train
    nn_proc._QUIET = True
    root = str(tmp_path / "music")
    write_inputs(root, sub="Train"); write_inputs(root, sub="Val", seed=1)
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0); np.random.seed(0)
    train.train(effect=audio.Compressor_4c(), epochs=1, n_data_points=40, batch_size=4, device=torch.device("cuda:0"), input_path=root, lr_max=2e-4, file_report=True,
                report_settings_per=2)
    text = capsys.readouterr().out
    assert "Val set, file by file" in text and "\ntotal" in text
    for i, s in enumerate(("__-30.0__1.0__0.001__0.001", "__-30.0__1.0__0.001__0.04", "__-30.0__1.0__0.04__0.001")):
        assert f"target_{i}_Compressor_4c{s}.wav" in text


def test_gen_dataset_on_the_device(tmp_path):
    from signaltrain_amd import audio, datasets
    out = str(tmp_path / "gen")
    written = datasets.gen_dataset(out, dur=0.2, num=5, effect="comp_4c", sr=int(SR), seed=1, device="cuda", log=lambda *a: None)
    assert len(written) == 5 and all(os.path.basename(os.path.dirname(p[0])) == "Train" for p in written)
    for i, (pi, pt) in enumerate(written):
        x, yy = audio.read_audio_file(pi, sr=int(SR))[0], audio.read_audio_file(pt, sr=int(SR))[0]
        assert len(x) == len(yy) == 3 * 4096 and float(np.abs(x).max()) <= 1.0 and float(np.abs(x).max()) > 0.01
        k = datasets.parse_knob_string(os.path.basename(pt))
        ref = entry(_lib.FX_COMP4C, torch.from_numpy(x).cuda(), k).cpu().numpy()
        assert np.array_equal(yy.view(np.int32), ref.view(np.int32)), i
    inv = str(tmp_path / "gen_dn")
    w2 = datasets.gen_dataset(inv, dur=0.2, num=2, effect="denoise", inpath=out, sr=int(SR), seed=2, device="cuda", log=lambda *a: None)
    clean, noisy = audio.read_audio_file(w2[1][0], sr=int(SR))[0], audio.read_audio_file(w2[1][1], sr=int(SR))[0]
    assert "inverse = True" in open(os.path.join(inv, "effect_info.ini")).read() and len(clean) == 8820 and not np.array_equal(clean, noisy)
