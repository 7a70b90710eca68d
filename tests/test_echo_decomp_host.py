"""CPU: the Echo and DeCompressor_4c effects (signaltrain/audio.py:430-443, :539-547, :573-583) on the host -- audio.echo and the two classes against
golden G18 (captured from the reference by tools/capture_golden_echo.py), their declarations, the refusals of st_echo and of the two new feed
effects (no launch: runs without a GPU) and their Dataset items through the host path."""
import ctypes as C
import hashlib
import os
import numpy as np
import pytest

from signaltrain_amd import _lib, audio

SR = 44100.0


@pytest.fixture(scope="module")
def g18(golden_dir):
    return np.load(os.path.join(golden_dir, "g18_echo_decomp.npz"))


def test_host_echo_is_the_reference_s_bit_for_bit(g18):
    """The whole grid (9 delays x 4 ratios x 5 echo counts on 4 windows) by the SHA-256 of the float32 result, and the stored results themselves."""
    X = g18["x"]
    delays, ratios, echoes = g18["delays"].tolist(), g18["ratios"].tolist(), g18["echoes"].tolist()
    assert X.shape == (4, 4096) and len(delays) == 9 and len(ratios) == 4 and echoes == [0, 1, 2, 3, 8]
    for s in range(4):
        for i, d in enumerate(delays):
            for j, r in enumerate(ratios):
                for k, e in enumerate(echoes):
                    y = audio.echo(X[s], delay_samples=d, ratio=r, echoes=e)
                    assert y.dtype == np.float32 and y.shape == (4096,)
                    if s in (1, 2):
                        assert np.array_equal(y, g18["echo_y_ib"][s - 1, i, j, k]), (s, d, r, e)
                    if s == 0 and j == 1 and e == 3:
                        assert np.array_equal(y, g18["echo_y_wn"][i]), (d, r, e)
                    assert hashlib.sha256(np.ascontiguousarray(y).tobytes()).digest() == g18["echo_sha256"][s, i, j, k].tobytes(), (s, d, r, e)
    assert np.array_equal(audio.echo(X[0], echoes=0), X[0]) and audio.echo(X[0], echoes=0) is not X[0]
    for bad in (0, 0.5, -3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            audio.echo(X[0], delay_samples=bad)


def test_echo_go_is_the_reference_s_bit_for_bit(g18):
    fx = audio.Echo()
    x = g18["x"][0]
    for i, kn in enumerate(g18["echo_knobs_nn"]):
        assert np.array_equal(np.asarray(fx.knobs_wc(kn)), g18["echo_go_knobs_wc"][i])
        y, xx = fx.go(x, kn)
        assert xx is x and y.dtype == np.float32 and np.array_equal(y, g18["echo_go_y"][i]), i
    assert not np.array_equal(g18["echo_go_y"][0], g18["echo_go_y"][2])                # the ratio knob is live


def test_decompressor_go_returns_the_clean_target_and_the_compressed_input(g18):
    """The input against the reference's: 1e-6 of the window's peak, the bound test_effects_family.py uses for compressor_4controls against its golden."""
    fx = audio.DeCompressor_4c()
    for i, (s, kn) in enumerate(zip(g18["decomp_sig"], g18["decomp_knobs_nn"])):
        x = g18["x"][s]
        assert np.array_equal(np.asarray(fx.knobs_wc(kn)), g18["decomp_go_knobs_wc"][i])
        y, xin = fx.go(x, kn)
        assert y is x                                                                 # the target is the clean window, untouched
        ref = g18["decomp_go_input"][i].astype(np.float64)
        assert xin.dtype == np.float32 and xin.shape == x.shape
        assert np.abs(xin.astype(np.float64) - ref).max() <= 1e-6 * np.abs(ref).max(), i
        assert np.array_equal(xin, audio.Compressor_4c().go(x, kn)[0])
    assert np.abs(g18["decomp_go_input"] - g18["x"][g18["decomp_sig"]]).max() > 1e-3      # the compressor did something


def test_effect_metadata_matches_reference(g18):
    for pre, fx in (("echo", audio.Echo()), ("decomp", audio.DeCompressor_4c())):
        assert fx.name == str(g18[pre + "_name"])
        assert list(fx.knob_names) == [str(s) for s in g18[pre + "_knob_names"]]
        assert np.array_equal(np.asarray(fx.knob_ranges, dtype=np.float64), g18[pre + "_knob_ranges"])
        assert bool(fx.is_inverse) == bool(g18[pre + "_is_inverse"])


def test_effect_declarations():
    ec, dc = audio.Echo(), audio.DeCompressor_4c()
    assert ec.feed_fx == _lib.FX_ECHO == 4 and ec.feed_choosers == (1, 3, 5, 6, 7) and not ec.makes_input and not ec.is_inverse
    assert dc.feed_fx == _lib.FX_DECOMP4C == 5 and dc.feed_choosers is None and dc.makes_input and dc.is_inverse
    assert ec.feed_ranges().shape == dc.feed_ranges().shape == (4, 2)
    assert np.array_equal(ec.feed_ranges(), [[400, 400], [0.4, 1.0], [2, 2], [0, 0]])
    assert np.array_equal(dc.feed_ranges(), audio.Compressor_4c().knob_ranges)
    assert _lib.ECHO_MAX == 8


def _feed_call(fx, K, lo, hi):
    lib = _lib.load()
    lo = (C.c_float * 4)(*lo); hi = (C.c_float * 4)(*hi)
    return lib.st_synth_effect(fx, 1, 0, 4, 8192, 2048, K, SR, lo, hi, 0, -1, None, None, None, None, None, None)


ECHO_LO, ECHO_HI = (400, 0.4, 2, 0), (400, 1.0, 2, 0)
C4_LO, C4_HI = (-30, 1, 1e-3, 1e-3), (0, 5, 4e-2, 4e-2)


def test_feed_refuses_bad_knob_counts_and_ranges_without_a_gpu():
    lib = _lib.load()
    for K in (2, 4):
        assert _feed_call(_lib.FX_ECHO, K, ECHO_LO, ECHO_HI) == -1 and f"K={K}".encode() in lib.st_last_error() and b"ST_FX_ECHO" in lib.st_last_error()
    for d in ((0.2, 400), (500, 400)):
        assert _feed_call(_lib.FX_ECHO, 3, (d[0], 0.4, 2, 0), (d[1], 1.0, 2, 0)) == -1
        assert b"ST_FX_ECHO" in lib.st_last_error() and b"delay" in lib.st_last_error(), (d, lib.st_last_error())
    for e in ((2, 9), (-1, 2)):
        assert _feed_call(_lib.FX_ECHO, 3, (400, 0.4, e[0], 0), (400, 1.0, e[1], 0)) == -1
        assert b"ST_FX_ECHO" in lib.st_last_error() and b"echoes" in lib.st_last_error(), (e, lib.st_last_error())
    for r in ((0.4, float("inf")), (float("nan"), 1.0), (1.0, 0.4)):
        assert _feed_call(_lib.FX_ECHO, 3, (400, r[0], 2, 0), (400, r[1], 2, 0)) == -1
        assert b"ST_FX_ECHO" in lib.st_last_error() and b"ratio" in lib.st_last_error(), (r, lib.st_last_error())
    for K in (0, 5):
        assert _feed_call(_lib.FX_DECOMP4C, K, C4_LO, C4_HI) == -1 and f"K={K}".encode() in lib.st_last_error() and b"ST_FX_DECOMP4C" in lib.st_last_error()
    assert _feed_call(6, 3, ECHO_LO, ECHO_HI) == -1 and b"ST_FX_DECOMP4C = 5" in lib.st_last_error() and b"ST_FX_ECHO = 4" in lib.st_last_error()
    # valid ids, counts and ranges get as far as the pointers: a half rounds to even (0.5 -> 0 echoes, 8.5 -> 8; 1.5 -> a delay of 2)
    assert _feed_call(_lib.FX_ECHO, 3, ECHO_LO, ECHO_HI) == -1 and b"null" in lib.st_last_error()
    assert _feed_call(_lib.FX_ECHO, 3, (1.5, -1.0, -0.5, 0), (1500, 1.0, 8.5, 0)) == -1 and b"null" in lib.st_last_error()
    for K in (1, 4):
        assert _feed_call(_lib.FX_DECOMP4C, K, C4_LO, C4_HI) == -1 and b"null" in lib.st_last_error()
    # the echo has no second-launch form: its scratch is only the long windows' noise; the de-compressor's is the compressor's
    assert lib.st_synth_effect_scratch_floats(_lib.FX_ECHO, 4, 8192) == 0
    assert lib.st_synth_effect_scratch_floats(_lib.FX_ECHO, 4, 16384) == lib.st_synth_effect_scratch_floats(_lib.FX_LOWPASS, 4, 16384) > 0
    for L in (8192, 16384, 1000):
        assert lib.st_synth_effect_scratch_floats(_lib.FX_DECOMP4C, 4, L) == lib.st_synth_effect_scratch_floats(_lib.FX_COMP4C, 4, L) > 0


def test_echo_entry_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float32)
    p = C.c_void_p(buf.ctypes.data)                  # never dereferenced: every call below is refused before any launch
    for args, what in (((None, p, SR, 1, 16, 16, p, None), b"null"), ((p, None, SR, 1, 16, 16, p, None), b"null"), ((p, p, SR, 1, 16, 16, None, None), b"null"),
                       ((p, p, SR, 1, 16, 20, p, None), b"ysz <= L"), ((p, p, SR, 0, 16, 16, p, None), b"bad sizes"), ((p, p, SR, 1, 0, 0, p, None), b"bad sizes"),
                       ((p, p, SR, 1, 16, 0, p, None), b"bad sizes")):
        assert lib.st_echo(*args) == -1 and b"st_echo" in lib.st_last_error() and what in lib.st_last_error(), (args, lib.st_last_error())


def test_dataset_items_through_the_host_path(monkeypatch):
    """Both effects behind SynthAudioDataSet's host item path.  Echo: the target is the tail of audio.echo of the item's input at its knobs.
    DeCompressor_4c: the clean windows are those of a Compressor_4c dataset built from the same seeds (the same generator draws) -- the target is
    the clean window's tail, the input the compressed window, whose tail is the compressor's target."""
    import torch
    from signaltrain_amd import datasets
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    items = {}
    for name, fx in (("ec", audio.Echo()), ("dc", audio.DeCompressor_4c()), ("c4", audio.Compressor_4c())):
        np.random.seed(21)
        ds = datasets.SynthAudioDataSet(8192, fx, y_size=2048, item_chunk=4)
        assert ds.choosers == ((1, 3, 5, 6, 7) if name == "ec" else (0, 1, 2, 4, 6, 7))
        items[name] = [ds[i] for i in range(4)]
    for x, y, k in items["ec"]:
        assert x.shape == (8192,) and y.shape == (2048,) and k.shape == (3,) and x.dtype == y.dtype == k.dtype == np.float32
        kw = audio.Echo().knobs_wc(k)
        assert kw[0] == 400.0 and kw[2] == 2.0
        assert np.array_equal(y, audio.echo(x, 400, kw[1], 2)[-2048:]) and not np.array_equal(y, x[-2048:])
    n_changed = 0
    for (x, y, k), (xc, yc, kc) in zip(items["dc"], items["c4"]):
        assert x.shape == (8192,) and y.shape == (2048,) and k.shape == (4,) and x.dtype == y.dtype == k.dtype == np.float32
        assert np.array_equal(k, kc) and np.array_equal(y, xc[-2048:])                  # the target is the clean signal's tail
        assert np.array_equal(x[-2048:], yc)                                            # the input is the compressed window
        assert np.array_equal(x, audio.Compressor_4c().go(xc, k)[0])
        n_changed += bool(np.abs(x - xc).max() > 1e-4)
    assert n_changed >= 2
