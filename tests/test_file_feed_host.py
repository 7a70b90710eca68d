"""CPU: the host side of the fused feed of recorded pairs (st_file_feed, csrc/st_feed_files.h) -- the symbol and its ctypes signature, its refusals
(before any launch: they run without a GPU), the draw law on its host replica datasets.file_feed_draw (the kernel is held to the replica bit for
bit in tests/test_gpu_file_feed.py), and the tables AudioFileDataSet hands to the kernel."""
import ctypes as C
import os

import numpy as np
import pytest

from signaltrain_amd import _lib, audio, datasets
from signaltrain_amd.datasets import file_feed_draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, NW, L = 1234, 8192, 1024


def test_file_feed_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "signaltrain_hip.h")).read()
    assert "int st_file_feed(unsigned seed, unsigned long long first_window" in hdr and "ST_PCM_F32 = 0, ST_PCM_S16 = 1" in hdr
    assert hasattr(_lib.load(), "st_file_feed")
    res, args = _lib.SIGNATURES["st_file_feed"]
    assert res is C.c_int and len(args) == 21 and args[1] is C.c_ulonglong and args[12] is C.c_longlong and args[13] is C.c_longlong
    assert (_lib.PCM_F32, _lib.PCM_S16) == (0, 1)


def _call(**kw):
    """st_file_feed with dummy non-null pointers (0x1000: never dereferenced on the host, and a refused call launches nothing)."""
    a = dict(B=8, L=64, ysz=16, K=3, fmt=0, pool_x=1, pool_y=1, file_off=1, file_len=1, nfiles=2, min_len=100, pool_samples=300,
             file_knobs=1, augment=1, x=1, y=1, knobs=1, meta=1)
    a.update(kw)
    p = lambda on: C.c_void_p(0x1000) if on else None
    lib = _lib.load()
    rc = lib.st_file_feed(7, 0, a["B"], a["L"], a["ysz"], a["K"], a["fmt"], p(a["pool_x"]), p(a["pool_y"]), p(a["file_off"]), p(a["file_len"]), a["nfiles"],
                          a["min_len"], a["pool_samples"], p(a["file_knobs"]), a["augment"], p(a["x"]), p(a["y"]), p(a["knobs"]), p(a["meta"]), None)
    return rc, lib.st_last_error()


@pytest.mark.parametrize("change, words", [
    (dict(pool_x=0), [b"null", b"pool_x"]), (dict(file_off=0), [b"null", b"file_off"]), (dict(file_len=0), [b"null", b"file_len"]), (dict(x=0), [b"null", b"x"]),
    (dict(pool_y=0), [b"null", b"pool_y"]), (dict(knobs=0), [b"null", b"knobs"]),
    (dict(B=0), [b"positive", b"B=0"]), (dict(L=0), [b"positive", b"L=0"]), (dict(ysz=0), [b"positive", b"ysz=0"]), (dict(nfiles=0), [b"positive", b"nfiles=0"]),
    (dict(B=-3), [b"positive"]), (dict(ysz=68), [b"ysz = 68", b"exceeds"]),
    (dict(L=66), [b"multiples of 4"]), (dict(ysz=18), [b"multiples of 4"]),
    (dict(K=-1), [b"K = -1", b"[0, 16]"]), (dict(K=17), [b"K = 17", b"[0, 16]"]),
    (dict(file_knobs=0), [b"file_knobs", b"K = 3"]), (dict(K=0), [b"file_knobs", b"NULL when K = 0"]),
    (dict(fmt=2), [b"fmt = 2", b"ST_PCM"]), (dict(fmt=-1), [b"fmt = -1"]),
    (dict(min_len=64), [b"min_len = 64", b"longer than the window"]), (dict(min_len=10), [b"min_len"]),
    (dict(pool_samples=99), [b"pool_samples = 99", b"below min_len"]),
])
def test_file_feed_refuses_by_rule(change, words):
    rc, msg = _call(**change)
    assert rc == -1 and b"st_file_feed" in msg and all(w in msg for w in words), (change, msg)


def test_draw_law_window_starts_respect_the_excluded_end():
    w = np.arange(NW)
    f, s, fl = file_feed_draw(SEED, w, [L + 1, L + 2, L + 3, L + 4, 5 * L + 3], L, True)
    assert set(f) == {0, 1, 2, 3, 4}
    assert set(s[f == 0]) == {0}                              # len - L = 1: only start 0
    assert set(s[f == 1]) == {0, 1}
    assert set(s[f == 2]) == {0, 1, 2}                        # len - L = 3: never 3
    assert set(s[f == 3]) == {0, 1, 2, 3}
    assert s[f == 4].min() >= 0 and s[f == 4].max() < 4 * L + 3 and s[f == 4].max() > 3 * L


def test_draw_law_is_uniform_over_files_and_fair_in_polarity():
    w = np.arange(NW)
    f, s, fl = file_feed_draw(SEED, w, [5000] * 4, L, True)
    counts = np.bincount(f, minlength=4)
    assert np.all(np.abs(counts - 2048) <= 235), counts       # 6 sigma of Binomial(8192, 1/4), sigma = 39
    assert abs(int(fl.sum()) - 4096) <= 272, fl.sum()          # 6 sigma of Binomial(8192, 1/2), sigma = 45
    assert set(fl) == {0, 1}
    f0, s0, fl0 = file_feed_draw(SEED, w, [5000] * 4, L, False)
    assert not fl0.any() and np.array_equal(f0, f) and np.array_equal(s0, s)       # augment only switches the flip


def test_draw_law_reaches_odd_starts_beyond_2_to_24():
    n = 2 ** 24 + 2 ** 20 + 3
    f, s, fl = file_feed_draw(SEED, np.arange(NW), [n], 256, True)
    assert not f.any() and s.min() >= 0 and s.max() < n - 256
    big = s[s > 2 ** 24]
    assert len(big) > 0 and (big % 2 == 1).any()              # float32 holds no odd integer there: a float-scaled draw cannot do this


def test_window_identity_singly_in_arrays_and_beyond_32_bits():
    lens = [5000, 7001, 9002]
    w = np.arange(40)
    f, s, fl = file_feed_draw(SEED, w, lens, L, True)
    for i in (0, 5, 39):
        assert file_feed_draw(SEED, int(w[i]), lens, L, True) == (f[i], s[i], fl[i])
    fa, sa, fla = file_feed_draw(SEED, w[7:23], lens, L, True)
    assert np.array_equal(fa, f[7:23]) and np.array_equal(sa, s[7:23]) and np.array_equal(fla, fl[7:23])
    hi = np.arange(2 ** 32, 2 ** 32 + 40, dtype=np.uint64)
    fh, sh, _ = file_feed_draw(SEED, hi, lens, L, True)
    assert file_feed_draw(SEED, 2 ** 32 + 5, lens, L, True)[:2] == (fh[5], sh[5])
    assert not np.array_equal(sh, s)                          # a window index >= 2^32 is not its low-word alias
    assert file_feed_draw(SEED, 2 ** 32 + 5, lens, L, True) != file_feed_draw(SEED, 5, lens, L, True)
    assert not np.array_equal(file_feed_draw(SEED + 1, w, lens, L, True)[1], s)


def test_int16_samples_convert_alike_in_float32_and_float64():
    """ST_PCM_S16: the kernel divides in float32; read_audio_file divides in float64 and rounds.  The same float for every int16."""
    s = np.arange(-32768, 32768, dtype=np.int16)
    a = np.array(s / 32767.0, dtype=np.float32)
    b = s.astype(np.float32) / np.float32(32767.0)
    assert b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))
    assert np.array_equal(np.rint(a.astype(np.float64) * 32767.0).astype(np.int16), s)       # ... and the pool's int16 are recovered exactly


def test_dataset_tables_and_s16_eligibility(tmp_path):
    from tests.test_device_feed import make_file_dataset
    root = make_file_dataset(str(tmp_path / "la2a"))
    fx = audio.FileEffect(root)
    np.random.seed(11)
    ds = datasets.AudioFileDataSet(8192, fx, path=root + "/Train/", datapoints=64, y_size=2048, augment=False)
    np.random.seed(11)
    assert ds._feed_seed == int(np.random.randint(0, 2 ** 31 - 1)) and ds._feed_count == 0      # the stream follows np.random.seed of the run
    t = ds.feed_tables()
    n = int(0.6 * 44100)
    assert t["off"].dtype == np.int64 and t["len"].dtype == np.int64 and t["knobs"].dtype == np.float32
    assert t["len"].tolist() == [n] * 3 and t["off"].tolist() == [0, n, 2 * n] and t["min_len"] == n and t["pool_samples"] == 3 * n
    assert t["knobs"].shape == (3, 3)
    for i in range(3):
        assert np.array_equal(t["knobs"][i], ds.knobs_nn(ds.knobs[i]))
        kw = ds.knobs[i]
        np.testing.assert_allclose(t["knobs"][i], [kw[0] - 0.5, kw[1] / 100 - 0.5, kw[2] / 100 - 0.5], atol=1e-6)
    assert t["pcm"] == "s16"                                  # int16 files at the dataset's rate, not companded
    comp = datasets.AudioFileDataSet(8192, fx, path=root + "/Train/", datapoints=8, y_size=2048, augment=False, compand=True)
    assert comp.feed_tables()["pcm"] == "f32"
    view = datasets.AudioFileDataSet(8192, fx, path=root + "/Val/", datapoints=4, y_size=2048, augment=False, view_of=ds)
    assert view.feed_tables()["pcm"] == "s16" and view._feed_seed != ds._feed_seed
    # a pair recorded at another rate is resampled on reading: float32 pool
    half = tmp_path / "half"; os.makedirs(half / "Train")
    tone = (0.5 * np.sin(2 * np.pi * 440 * np.arange(22050) / 22050.0) * 32767).astype(np.int16)
    audio.write_audio_file(str(half / "Train" / "input_0_.wav"), tone, 22050)
    audio.write_audio_file(str(half / "Train" / "target_0_LA2A_3c__0__50__50.wav"), tone, 22050)
    rs = datasets.AudioFileDataSet(8192, fx, path=str(half / "Train") + "/", datapoints=4, y_size=2048, augment=False)
    assert rs.feed_tables()["pcm"] == "f32" and abs(int(rs.feed_tables()["len"][0]) - 44100) <= 1
    info = {}
    audio.read_audio_file(str(half / "Train" / "input_0_.wav"), sr=22050, info=info)
    assert info == {"int16": True, "exact": True}


def test_fused_feed_surface_without_a_device(tmp_path):
    """batch_device / device_batches keep their CPU-device form; the fused form names what it needs; the loaders share one iteration."""
    from tests.test_device_feed import make_file_dataset
    root = make_file_dataset(str(tmp_path / "la2a"))
    fx = audio.FileEffect(root)
    ds = datasets.AudioFileDataSet(8192, fx, path=root + "/Train/", datapoints=64, y_size=2048, augment=True)
    x, y, k = ds.batch_device(4, "cpu")
    assert x.shape == (4, 8192) and y.shape == (4, 2048) and k.shape == (4, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ds.batch_device_fused(4, "cpu")
    ld = datasets.DeviceFileLoader(ds, 16, "cuda:0")
    assert len(ld) == 4 and ld.per_call == 128
    assert datasets.DeviceFileLoader.__iter__ is datasets.DeviceSynthLoader.__iter__
