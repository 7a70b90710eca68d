"""CPU: the host side of the live feed's pre-roll (st_live_feed_stream, csrc/st_feed_stream.h) -- the two symbols and their signatures, the size
function, the refusals (before any launch: they run without a GPU) and AudioInputDataSet's host path with a history in front of the window.  The
kernel is held to the library's own effect entries, bit for bit, in tests/test_gpu_stream_feed.py."""
import ctypes as C
import os

import numpy as np
import pytest

from signaltrain_amd import _lib, audio, datasets, train
from tests.test_live_feed_host import C4_RANGES, make_input_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREROLL_MAX = 1 << 22


def test_stream_feed_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "signaltrain_hip.h")).read()
    assert "size_t st_live_feed_stream_scratch_floats(int effect, int B, int L, int preroll, float synth_prob);" in hdr
    assert "int st_live_feed_stream(int effect, unsigned family_mask, float synth_prob, int preroll, unsigned seed, unsigned long long first_window," in hdr
    assert "ST_LIVE_PREROLL_MAX = 1 << 22" in hdr
    lib = _lib.load()
    assert hasattr(lib, "st_live_feed_stream") and hasattr(lib, "st_live_feed_stream_scratch_floats")
    res, args = _lib.SIGNATURES["st_live_feed_stream"]
    live = _lib.SIGNATURES["st_live_feed"][1]
    assert res is C.c_int and len(args) == 27 and args[3] is C.c_int and args[:3] == live[:3] and args[4:] == live[3:]      # st_live_feed's, preroll after synth_prob
    assert _lib.SIGNATURES["st_live_feed_stream_scratch_floats"] == (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float])
    mk = open(os.path.join(ROOT, "signaltrain_amd", "csrc", "Makefile")).read()
    assert "st_feed_stream.h" in mk
    assert os.path.isfile(os.path.join(ROOT, "signaltrain_amd", "csrc", "st_feed_stream.h"))


def test_scratch_sizes():
    lib = _lib.load()
    n, n0 = lib.st_live_feed_stream_scratch_floats, lib.st_live_feed_scratch_floats
    B = 8
    for fx in range(6):
        for Lw in (4096, 8192, 65536):
            for p in (0.0, 0.5, 1.0):
                assert n(fx, B, Lw, 0, p) == n0(fx, B, Lw, p)            # preroll = 0 is st_live_feed
    # [world knobs 4 B | R per row, round_up(B, 4) | B rows of round_up(preroll + L, 64) (none for Denoise) | st_live_feed's scratch with synthetic windows]
    assert n(_lib.FX_COMP4C, B, 4096, 8192, 0.0) == 4 * B + B + B * 12288
    assert n(_lib.FX_LOWPASS, 6, 4096, 8192, 0.0) == 4 * 6 + 8 + 6 * 12288
    assert n(_lib.FX_ECHO, B, 4096, 100, 0.0) == 4 * B + B + B * 4224       # 4196 samples: the pitch is rounded up to 64
    assert n(_lib.FX_DENOISE, B, 4096, 8192, 0.0) == 4 * B + B
    assert n(_lib.FX_DECOMP4C, B, 8192, 4096, 0.5) == 4 * B + B + B * 12288 + n0(_lib.FX_DECOMP4C, B, 8192, 0.5)
    # no size for what the entry refuses
    assert n(9, B, 8192, 4096, 0.0) == 0 and n(_lib.FX_COMP4C, 0, 8192, 4096, 0.0) == 0 and n(_lib.FX_COMP4C, B, 0, 4096, 0.0) == 0
    assert n(_lib.FX_COMP4C, B, 8192, -4, 0.0) == 0 and n(_lib.FX_COMP4C, B, 8192, 4098, 0.0) == 0 and n(_lib.FX_COMP4C, B, 8192, PREROLL_MAX + 4, 0.0) == 0
    assert n(_lib.FX_COMP4C, B, 8190, 4096, 0.0) == 0
    assert n(_lib.FX_COMP4C, B, 8192, PREROLL_MAX, 0.0) == 4 * B + B + B * (PREROLL_MAX + 8192)
    assert n(_lib.FX_COMP4C, 1 << 20, 8192, PREROLL_MAX, 0.0) == 0            # B * (preroll + L) >= 2^40
    assert n(_lib.FX_COMP4C, 1, 2 ** 31 - 8, 4096, 0.0) == 0                  # preroll + L leaves the 32-bit row index


def _call(**kw):
    """st_live_feed_stream with dummy non-null device pointers (0x1000: never dereferenced on the host, and a refused call launches nothing)."""
    a = dict(effect=_lib.FX_COMP4C, family_mask=_lib.FAMILIES_COMPRESSOR, synth_prob=0.0, preroll=64, B=8, L=64, ysz=16, K=4, sr=44100.0, lo=C4_RANGES[0],
             hi=C4_RANGES[1], fmt=0, pool_x=1, file_off=1, file_len=1, nfiles=2, min_len=100, pool_samples=300, x=1, y=1, knobs=1, meta=1, scratch=1)
    a.update(kw)
    p = lambda on: C.c_void_p(0x1000) if on else None
    f4 = lambda v: None if v is None else (C.c_float * 4)(*v)
    lib = _lib.load()
    rc = lib.st_live_feed_stream(a["effect"], a["family_mask"], a["synth_prob"], a["preroll"], 7, 0, a["B"], a["L"], a["ysz"], a["K"], a["sr"], f4(a["lo"]), f4(a["hi"]),
                                 1, a["fmt"], p(a["pool_x"]), p(a["file_off"]), p(a["file_len"]), a["nfiles"], a["min_len"], a["pool_samples"],
                                 p(a["x"]), p(a["y"]), p(a["knobs"]), p(a["meta"]), p(a["scratch"]), None)
    return rc, lib.st_last_error()


@pytest.mark.parametrize("change, words", [
    # the pre-roll's own rules; null device pointers everywhere: the rule comes before anything is touched
    (dict(preroll=-4), [b"preroll is negative", b"preroll=-4"]),
    (dict(preroll=-4, pool_x=0, x=0, y=0, knobs=0, scratch=0), [b"preroll is negative"]),
    (dict(preroll=66), [b"not a multiple of 4", b"preroll=66"]),
    (dict(preroll=2, pool_x=0, x=0, scratch=0), [b"not a multiple of 4"]),
    (dict(preroll=PREROLL_MAX + 4), [b"ST_LIVE_PREROLL_MAX", b"preroll=4194308"]),
    (dict(scratch=0), [b"null", b"scratch", b"preroll = 64"]),
    (dict(scratch=0, pool_x=0, x=0), [b"null", b"scratch"]),
    (dict(B=1 << 20, preroll=PREROLL_MAX, L=8192, ysz=2048, min_len=10000, pool_samples=20000), [b"B * (preroll + L)", b"2^40"]),
    (dict(B=1, preroll=4096, L=2 ** 31 - 8, ysz=2048, min_len=2 ** 32, pool_samples=2 ** 33), [b"preroll + L", b"32-bit row index"]),
    # everything st_live_feed refuses, with its rule
    (dict(effect=9), [b"effect 9", b"ST_FX_"]), (dict(K=5), [b"ST_FX_COMP4C", b"K=5"]), (dict(effect=_lib.FX_COMP, K=4), [b"ST_FX_COMP ", b"K=4"]),
    (dict(effect=_lib.FX_LOWPASS, K=1, lo=[100.0, 0, 0, 0], hi=[30000.0, 0, 0, 0]), [b"cutoff range", b"sr / 2"]),
    (dict(effect=_lib.FX_ECHO, K=3, lo=[100.0, 0.1, 0, 0], hi=[400.0, 0.9, 9, 0]), [b"echoes range", b"ST_ECHO_MAX"]),
    (dict(lo=None), [b"null", b"knob_lo"]),
    (dict(B=0), [b"positive", b"B=0"]), (dict(L=0), [b"positive", b"L=0"]), (dict(ysz=68), [b"ysz = 68", b"exceeds"]),
    (dict(L=66), [b"multiples of 4", b"L = 66"]), (dict(ysz=18), [b"multiples of 4", b"ysz = 18"]), (dict(sr=0.0), [b"sr = 0"]),
    (dict(synth_prob=1.5), [b"synth_prob = 1.5", b"[0, 1]"]), (dict(synth_prob=float("nan")), [b"synth_prob", b"[0, 1]"]),
    (dict(fmt=2), [b"fmt = 2", b"ST_PCM"]), (dict(min_len=64), [b"min_len = 64", b"longer than the window"]),
    (dict(pool_samples=99), [b"pool_samples = 99", b"below min_len"]),
    (dict(pool_x=0), [b"null", b"pool_x"]), (dict(file_len=0), [b"null", b"file_len"]), (dict(x=0), [b"null", b"x"]), (dict(knobs=0), [b"null", b"knobs"]),
    (dict(synth_prob=0.5, family_mask=0), [b"family_mask is empty"]),
    (dict(synth_prob=0.5, L=12000, ysz=4000, min_len=20000, pool_samples=50000), [b"12000-sample window"]),
])
def test_stream_feed_refuses_by_rule(change, words):
    rc, msg = _call(**change)
    assert rc == -1 and b"st_live_feed_stream" in msg and all(w in msg for w in words), (change, msg)


def test_preroll_zero_refuses_as_st_live_feed():
    """preroll = 0 is the call of st_live_feed: its refusals, under its name, and no scratch needed."""
    rc, msg = _call(preroll=0, scratch=0, x=0)
    assert rc == -1 and b"st_live_feed:" in msg and b"null" in msg
    rc, msg = _call(preroll=0, ysz=18)
    assert rc == -1 and b"st_live_feed:" in msg and b"multiples of 4" in msg


def test_audio_input_dataset_preroll_on_the_host(tmp_path):
    root = str(tmp_path / "rec")
    make_input_dataset(root)
    fx = audio.Compressor_4c()
    mk = lambda **kw: datasets.AudioInputDataSet(1024, fx, path=root + "/Train/", datapoints=32, y_size=256, augment=False, **kw)
    np.random.seed(11); plain = mk()
    items = [plain[i] for i in range(6)]
    np.random.seed(11); zero = mk(preroll=0)
    assert zero.preroll == 0 and plain.preroll == 0 and zero._feed_seed == plain._feed_seed
    for a, b in zip(items, [zero[i] for i in range(6)]):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    # with a history the window is the same one and the target is the tail of the effect over the extended span
    np.random.seed(11); ds = mk(preroll=512)
    pool, full, differs = ds.x, 0, 0
    for i in range(6):
        x, y, kn = ds[i]
        x0, y0, kn0 = items[i]
        assert np.array_equal(x, x0) and np.array_equal(kn, kn0) and x.shape == (1024,) and y.shape == (256,) and y.dtype == np.float32
        hits = [(f, s) for f in range(len(pool)) for s in np.flatnonzero(pool[f][:len(pool[f]) - 1023] == x[0]) if np.array_equal(pool[f][s:s + 1024], x)]
        assert len(hits) == 1
        f, ibgn = hits[0]
        R = min(512, int(ibgn) & ~3)
        kw = fx.knobs_wc(kn)
        ref = audio.compressor_4controls(pool[f][ibgn - R:ibgn + 1024], thresh=kw[0], ratio=kw[1], attackTime=kw[2], releaseTime=kw[3], sr=fx.sr)
        assert np.array_equal(y, np.asarray(ref, dtype=np.float32)[-256:])
        full += R == 512; differs += not np.array_equal(y, y0)
    assert full and differs                                       # a history was there, and it changed a target
    for bad in (-4, 6, 510, 2.5):
        with pytest.raises(ValueError, match="preroll"):
            mk(preroll=bad)


def test_train_refuses_preroll_without_input_path():
    with pytest.raises(ValueError, match="preroll = 4096.*input_path"):
        train.train(preroll=4096)


def test_run_train_has_the_preroll_flag():
    import subprocess
    import sys
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "run_train.py"), *a], capture_output=True, text=True, timeout=300)
    r = run("--inpath", "X", "--preroll", "6")
    assert r.returncode != 0 and "unrecognized arguments" not in r.stderr and "--preroll 6" in r.stderr and "multiple of 4" in r.stderr, r.stderr
    r = run("--preroll", "4096")
    assert r.returncode != 0 and "--inpath" in r.stderr and "unrecognized" not in r.stderr, r.stderr
