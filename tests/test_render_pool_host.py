"""CPU: the host side of st_render_pool (include/signaltrain_hip.h) -- a folder of recordings through an effect in one device call: the symbols, the size
function, every refusal (before any launch: runs without a GPU), audio.int2knobs, datasets.render_knobs, the host render() / write() round trip, the dataset
generator and the file-report rules of train() / run_train.py."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from signaltrain_amd import _lib, audio, datasets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL = C.POINTER(C.c_longlong)
SR = 44100


def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "signaltrain_hip.h")).read()
    lib = _lib.load()
    for name, decl in (("st_render_pool_scratch_floats", "size_t st_render_pool_scratch_floats(int effect, const long long* file_len_host, int nfiles);"),
                       ("st_render_pool", "int st_render_pool(int effect, float sr, int fmt, const void* pool_x,")):
        assert decl in hdr, name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["st_render_pool"]
    assert res is C.c_int and len(args) == 15 and args[1] is C.c_float and args[7] is C.c_longlong and args[8] is C.c_longlong and args[11] is C.c_ulonglong
    assert _lib.SIGNATURES["st_render_pool_scratch_floats"][0] is C.c_size_t


def scratch(lib, fx, lens):
    ln = np.asarray(lens, np.int64)
    return int(lib.st_render_pool_scratch_floats(fx, ln.ctypes.data_as(LL), int(ln.size)))


def test_scratch_size():
    lib = _lib.load()
    ln = np.array([5, 100], np.int64)
    assert lib.st_render_pool_scratch_floats(_lib.FX_COMP4C, None, 2) == 0
    assert lib.st_render_pool_scratch_floats(_lib.FX_COMP4C, ln.ctypes.data_as(LL), 0) == 0
    assert scratch(lib, _lib.FX_COMP4C, [5, -1]) == 0 and scratch(lib, _lib.FX_COMP4C, [5, 2 ** 31 - 64]) == 0
    assert scratch(lib, 6, [5, 100]) == 0 and scratch(lib, -1, [5, 100]) == 0
    assert scratch(lib, _lib.FX_DENOISE, [5, 100]) == 0          # streams from the pool to out
    for fx in (_lib.FX_COMP4C, _lib.FX_COMP, _lib.FX_LOWPASS, _lib.FX_ECHO, _lib.FX_DECOMP4C):
        prev = 0
        for n in (0, 1, 63, 64, 65, 4097, 2 ** 31 - 65):
            cur = scratch(lib, fx, [5, n, 100])
            assert cur >= prev and cur >= 5 + n + 100 and cur % 4 == 0       # non-decreasing as a file grows, room for every sample
            prev = cur


def call(lib, **over):
    """st_render_pool with host buffers standing in for device memory: every case here is refused before any launch."""
    pool = np.zeros(64, np.float32); tab = np.zeros(4, np.int64); kw = np.zeros(16, np.float32); out = np.zeros(64, np.float32); scr = np.zeros(1024, np.float32)
    a = dict(effect=_lib.FX_COMP4C, sr=44100.0, fmt=_lib.PCM_F32, pool_x=pool.ctypes.data, file_off=tab.ctypes.data, file_len=tab.ctypes.data, nfiles=1,
             max_len=0, pool_samples=64, knobs_wc=kw.ctypes.data, seed=0, first_file=0, out=out.ctypes.data, scratch=scr.ctypes.data, stream=None)
    assert pool.ctypes.data % 16 == 0 and out.ctypes.data % 16 == 0 and scr.ctypes.data % 16 == 0
    a.update(over)
    rc = lib.st_render_pool(a["effect"], a["sr"], a["fmt"], a["pool_x"], a["file_off"], a["file_len"], a["nfiles"], a["max_len"], a["pool_samples"], a["knobs_wc"],
                            a["seed"], a["first_file"], a["out"], a["scratch"], a["stream"])
    return rc, lib.st_last_error()


def test_refusals():
    lib = _lib.load()
    assert call(lib)[0] == 0                                     # max_len == 0: accepted, nothing launched
    base = np.zeros(64, np.float32).ctypes.data
    al = np.zeros(64, np.float32)
    cases = [(dict(pool_x=None), b"pool_x"), (dict(file_off=None), b"file_off"), (dict(file_len=None), b"file_len"), (dict(knobs_wc=None), b"knobs_wc"),
             (dict(out=None), b"out"), (dict(scratch=None), b"scratch"),
             (dict(effect=6), b"effect"), (dict(effect=-1), b"effect"), (dict(fmt=2), b"fmt"),
             (dict(nfiles=0), b"nfiles"), (dict(pool_samples=0), b"pool_samples"),
             (dict(max_len=-1), b"max_len"), (dict(max_len=2 ** 31 - 64), b"max_len"),
             (dict(sr=0.0), b"sr ="), (dict(sr=-1.0), b"sr ="),
             (dict(out=al.ctypes.data + 4), b"out must be 16-byte aligned"), (dict(scratch=al.ctypes.data + 8), b"scratch must be 16-byte aligned"),
             (dict(pool_x=al.ctypes.data + 8), b"pool_x must be 16-byte aligned"), (dict(pool_x=al.ctypes.data + 4, fmt=_lib.PCM_S16), b"pool_x must be 8-byte aligned")]
    assert base % 16 == 0 and al.ctypes.data % 16 == 0
    for over, word in cases:
        rc, msg = call(lib, **over)
        assert rc == -1 and b"st_render_pool" in msg and word in msg, (over, msg)
    assert call(lib, pool_x=al.ctypes.data + 8, fmt=_lib.PCM_S16)[0] == 0       # int16 pools need 8 bytes only
    assert call(lib, effect=_lib.FX_DENOISE, scratch=None)[0] == 0              # no scratch where the size function says 0


def test_int2knobs():
    np.testing.assert_allclose(audio.int2knobs(12345, [[-.5, .5]] * 4, 12), [0.13636363636363635, -0.40909090909090906, 0.2272727272727273, 0.31818181818181823], rtol=0, atol=1e-15)
    assert audio.int2knobs(100, [[1, 6]] * 3, 6) == [3.0, 5.0, 5.0]
    assert audio.int2knobs(1234, [[0, 9]] * 4, 10) == [1.0, 2.0, 3.0, 4.0]
    assert audio.int2knobs(0, [[2, 3], [-1, 1]], 3) == [2.0, -1.0] and audio.int2knobs(1, [[2, 3], [-1, 1]], 3) == [2.0, 0.0]      # the last knob varies fastest
    assert audio.int2knobs(8, [[2, 3], [-1, 1]], 3) == [3.0, 1.0]
    with pytest.raises(AssertionError):
        audio.int2knobs(9, [[2, 3], [-1, 1]], 3)


def test_render_knobs():
    e = audio.Compressor_4c()
    kn = np.array([[-0.5, 0.5, 0.0, 0.25], [0.1349, -0.2, 0.3, -0.5]])
    kw, strs = datasets.render_knobs(e, 2, knobs=kn)
    want = [[float('%.4g' % v) for v in e.knobs_wc(k)] for k in kn]
    assert kw.tolist() == want and kw[0].tolist() == [-30.0, 5.0, 0.0205, 0.03025]
    assert strs[0] == "__-30.0__5.0__0.0205__0.03025"
    with pytest.raises(ValueError):
        datasets.render_knobs(e, 3, knobs=kn)
    # the grid for i < sp ** K, then the seeded draws
    lp = audio.LowPass()
    kw, strs = datasets.render_knobs(lp, 6, settings_per=4, seed=5)
    assert kw[:4, 0].tolist() == [float('%.4g' % v[0]) for v in (audio.int2knobs(i, lp.knob_ranges.tolist(), 4) for i in range(4))] == [10.0, 673.3, 1337.0, 2000.0]
    draws = np.random.default_rng(5).random((6, 1)) - 0.5
    assert kw[4:, 0].tolist() == [float('%.4g' % lp.knobs_wc(draws[i])[0]) for i in (4, 5)]
    assert datasets.render_knobs(lp, 6, seed=5)[0][4:].tolist() == kw[4:].tolist()      # a file's draw does not depend on the grid
    kw2, strs2 = datasets.render_knobs(lp, 6, settings_per=4, seed=5)
    assert kw2.tolist() == kw.tolist() and strs2 == strs and datasets.render_knobs(lp, 6, settings_per=4, seed=6)[0][4:].tolist() != kw[4:].tolist()
    # %.4g rounding, and names that parse back to the same float32 values
    class Fixed(audio.Effect):
        def __init__(self):
            super().__init__(); self.name = "Fixed"; self.knob_names = ["a", "b"]; self.knob_ranges = np.array([[-10.953, -10.953], [0.00504321, 0.00504321]])
    kw, strs = datasets.render_knobs(Fixed(), 1, knobs=[[0.0, 0.0]])
    assert kw.tolist() == [[-10.95, 0.005043]] and strs == ["__-10.95__0.005043"]
    kw, strs = datasets.render_knobs(e, 40, seed=2)
    fin, ftg = datasets.render_names(e, strs, first=7)
    assert fin[0] == "input_7_.wav" and ftg[0] == "target_7_Compressor_4c" + strs[0] + ".wav"
    for i in range(40):
        assert np.array_equal(datasets.parse_knob_string(ftg[i]), kw[i].astype(np.float32))


def write_inputs(root, lens=(9000, 8300, 10011), sub="Train", seed=0):
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, sub), exist_ok=True)
    xs = []
    for i, n in enumerate(lens):
        t = np.arange(n) / SR
        x = (0.6 * np.sin(2 * np.pi * (110.0 * (i + 1)) * t) * np.exp(-3.0 * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)
        audio.write_audio_file(os.path.join(root, sub, f"clip_{i}.wav"), x, SR)
        xs.append(x)
    return xs


@pytest.mark.parametrize("name", ["Compressor_4c", "LowPass", "Denoise"])
def test_host_render_and_write_round_trip(tmp_path, name):
    e = getattr(audio, name)()
    xs = write_inputs(str(tmp_path / "in"))
    ds_in = datasets.AudioInputDataSet(8192, e, sr=SR, path=str(tmp_path / "in" / "Train"), datapoints=8, y_size=2048)
    np.random.seed(3)
    ds = ds_in.render(seed=4)
    kw, strs = datasets.render_knobs(e, 3, seed=4)
    assert isinstance(ds, datasets.AudioFileDataSet) and np.array_equal(ds.knobs, kw.astype(np.float32))
    assert [os.path.basename(f) for f in ds.input_filenames] == ["input_0_.wav", "input_1_.wav", "input_2_.wav"]
    assert [os.path.basename(f) for f in ds.target_filenames] == [f"target_{i}_{e.name}{strs[i]}.wav" for i in range(3)]
    np.random.seed(3)
    for f in range(3):
        y, x = e.go_wc(xs[f], kw[f].tolist())
        assert np.array_equal(ds.x[f], np.asarray(x, np.float32)) and np.array_equal(ds.y[f], np.asarray(y, np.float32))
        if name == "Denoise":
            assert np.array_equal(ds.y[f], xs[f]) and not np.array_equal(ds.x[f], xs[f])      # the noisy signal is what the model is fed
        else:
            assert np.array_equal(ds.x[f], xs[f])
    # write() and read back: FileEffect + AudioFileDataSet on the folder reproduce the dataset
    out = str(tmp_path / "out")
    ds.write(out, "Train"); ds.write(out, "Val")
    fe = audio.FileEffect(out, sr=SR)
    assert bool(fe.is_inverse) == bool(e.is_inverse) and fe.knob_names == list(e.knob_names) and np.array_equal(fe.knob_ranges, np.asarray(e.knob_ranges, np.float64))
    back = datasets.AudioFileDataSet(8192, fe, sr=SR, path=os.path.join(out, "Train") + "/", datapoints=8, y_size=2048)
    assert np.array_equal(back.knobs, ds.knobs)
    for f in range(3):
        assert np.array_equal(back.x[f], ds.x[f]) and np.array_equal(back.y[f], ds.y[f])


def names_in(d):
    return sorted(os.path.basename(f) for f in glob.glob(os.path.join(d, "*.wav")))


def test_gen_dataset_synthesised(tmp_path):
    out = str(tmp_path / "synth")
    written = datasets.gen_dataset(out, dur=0.2, num=5, effect="comp_4c", sr=SR, seed=1, log=lambda *a: None)
    assert len(written) == 5
    tr, va = names_in(os.path.join(out, "Train")), names_in(os.path.join(out, "Val"))
    assert [n for n in tr if n.startswith("input")] == [f"input_{i}_.wav" for i in range(5)] and len(tr) == 10 and va == []      # i / num > 0.8 sends a file to Val
    e = audio.Compressor_4c()
    for i, (pi, pt) in enumerate(written):
        x, y = audio.read_audio_file(pi, sr=SR)[0], audio.read_audio_file(pt, sr=SR)[0]
        assert len(x) == len(y) == 3 * 4096 and float(np.abs(x).max()) <= 1.0 and os.path.basename(pt).startswith(f"target_{i}_Compressor_4c__")
        assert np.array_equal(y, e.go_wc(x, datasets.parse_knob_string(os.path.basename(pt), dtype=np.float64).tolist())[0])
    ini = open(os.path.join(out, "effect_info.ini")).read()
    assert "[effect]" in ini and "name = Compressor_4c" in ini and "knob_names = ['threshold', 'ratio', 'attackTime', 'releaseTime']" in ini and "inverse" not in ini
    # a second run continues the indices; of ten files the last one has i / num > 0.8 and goes to Val/
    written2 = datasets.gen_dataset(out, dur=0.2, num=10, effect="comp_4c", sr=SR, seed=2, log=lambda *a: None)
    assert [os.path.basename(p[0]) for p in written2] == [f"input_{i}_.wav" for i in range(5, 15)]
    assert [os.path.basename(os.path.dirname(p[0])) for p in written2] == ["Train"] * 9 + ["Val"]
    # the same seed gives the same files
    other = str(tmp_path / "synth2")
    w3 = datasets.gen_dataset(other, dur=0.2, num=5, effect="comp_4c", sr=SR, seed=1, log=lambda *a: None)
    assert [os.path.basename(p[1]) for p in w3] == [os.path.basename(p[1]) for p in written]
    assert all(np.array_equal(audio.read_audio_file(a[1], sr=SR)[0], audio.read_audio_file(b[1], sr=SR)[0]) for a, b in zip(w3, written))


def test_gen_dataset_from_inpath_with_grid(tmp_path):
    src = str(tmp_path / "music")
    write_inputs(src, lens=(20000, 5000), sub="Train")
    write_inputs(src, lens=(12000,), sub="Val", seed=1)
    out = str(tmp_path / "lp")
    written = datasets.gen_dataset(out, dur=0.2, num=5, effect="lowpass", inpath=src, sr=SR, seed=3, log=lambda *a: None)
    # file i takes input i % 3 of the sorted list (Train/clip_0, Train/clip_1, Val/clip_0) and goes where its input lies
    assert [os.path.basename(os.path.dirname(p[0])) for p in written] == ["Train", "Train", "Val", "Train", "Train"]
    assert [len(audio.read_audio_file(p[0], sr=SR)[0]) for p in written] == [8820, 5000, 8820, 8820, 5000]
    lp = audio.LowPass()
    for pi, pt in written:
        x, y = audio.read_audio_file(pi, sr=SR)[0], audio.read_audio_file(pt, sr=SR)[0]
        assert np.array_equal(y, lp.go_wc(x, datasets.parse_knob_string(os.path.basename(pt), dtype=np.float64).tolist())[0])
    # --sp with an inpath that names neither Train nor Val: sp ** K / 0.8 files, the first sp ** K on the grid
    out2 = str(tmp_path / "lp_grid")
    w2 = datasets.gen_dataset(out2, dur=0.1, sp=4, effect="lowpass", inpath=src, sr=SR, seed=3, log=lambda *a: None)
    assert len(w2) == 5
    assert [float(datasets.parse_knob_string(os.path.basename(p[1]))[0]) for p in w2[:4]] == [float(np.float32(v)) for v in (10.0, 673.3, 1337.0, 2000.0)]
    inv = str(tmp_path / "dn")
    w3 = datasets.gen_dataset(inv, dur=0.2, num=2, effect="denoise", inpath=src, sr=SR, seed=3, log=lambda *a: None)
    assert "inverse = True" in open(os.path.join(inv, "effect_info.ini")).read()
    clean, noisy = audio.read_audio_file(w3[0][0], sr=SR)[0], audio.read_audio_file(w3[0][1], sr=SR)[0]
    assert not np.array_equal(clean, noisy) and float(np.abs(noisy - clean).max()) <= float(datasets.parse_knob_string(os.path.basename(w3[0][1]))[0]) * 1.0001 + 1e-7


def test_gen_dataset_cli(tmp_path):
    out = str(tmp_path / "cli")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gen_dataset.py"), out, "-d", "0.1", "-n", "2", "-e", "comp_t", "--seed", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert len(names_in(os.path.join(out, "Train"))) == 4 and "name = Comp_Just_Thresh" in open(os.path.join(out, "effect_info.ini")).read()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gen_dataset.py"), "--help"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "--seed" in r.stdout and "--device" in r.stdout and "--inpath" in r.stdout and "Generator" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gen_dataset.py"), out, "-e", "pitch"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "pitch" in (r.stdout + r.stderr)


def test_file_report_rules():
    import inspect
    from signaltrain_amd import train
    sig = inspect.signature(train.train).parameters
    assert sig["file_report"].default is False and sig["report_settings_per"].default is None
    with pytest.raises(ValueError, match="file_report"):
        train.train(file_report=True, epochs=1, n_data_points=40, batch_size=20)
    sig = inspect.signature(datasets.AudioInputDataSet.evaluate)
    assert list(sig.parameters) == ["self", "model", "knobs", "settings_per", "seed", "device", "want_out", "batch_size"]
    sig = inspect.signature(datasets.AudioInputDataSet.render)
    assert list(sig.parameters) == ["self", "knobs", "settings_per", "seed", "device", "pcm"]


def test_run_train_file_report_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_train.py"), "--file-report"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--effect files" in (r.stdout + r.stderr)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_train.py"), "--file-report", "--inpath", "nowhere", "--report-sp", "3", "--target", "nope"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "invalid target type" in (r.stdout + r.stderr)      # the parser takes the three flags together
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_train.py"), "--report-sp", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--report-sp" in (r.stdout + r.stderr)
