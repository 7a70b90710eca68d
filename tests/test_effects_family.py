"""CPU: the compressor family of the reference's run_train.py keys comp / comp_t / comp_one (signaltrain/audio.py:349-371, :484-536) -- the host
effects against golden G15 (captured from the reference by tools/capture_golden_r7.py), their checkpoint metadata, the run_train.py keys, the
Dataset items of the envelope compressor behind a DataLoader, and the host-side refusals of st_synth_effect (no launch: runs without a GPU)."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

from signaltrain_amd import _lib, audio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(os.path.join(golden_dir, "g15_compressor_family.npz"))


def _rel(y, ref):
    return float(np.abs(np.asarray(y, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def test_host_compressor_matches_reference_golden(g15):
    """Compressor().go: float32 result against the reference's float64 output, 1e-6 of the window's peak (the float32 rounding of y is 6e-8;
    the rest is float32 log10 and the closed-form filter coefficients against scipy.signal.butter's)."""
    fx = audio.Compressor(sr=float(g15["sr"]))
    for i in range(len(g15["comp_x"])):
        assert np.array_equal(np.asarray(fx.knobs_wc(g15["comp_kn"][i])), g15["comp_kw"][i])
        y = fx.go(g15["comp_x"][i], g15["comp_kn"][i])[0]
        assert y.dtype == np.float32 and y.shape == (8192,)
        assert _rel(y, g15["comp_y"][i]) <= 1e-6, i
    assert np.abs(g15["comp_y"][4][:2048]).max() == 0.0                    # digital silence stays silent (d = -120 dB)


def test_host_compressor_4controls_variants_match_reference_golden(g15):
    for pre, fx in (("thresh", audio.Comp_Just_Thresh()), ("one", audio.Compressor_4c_OneSetting())):
        for j, i in enumerate(g15[pre + "_idx"]):
            y = fx.go(g15["comp_x"][i], g15[pre + "_kn"][j])[0]
            assert _rel(y, g15[pre + "_y"][j]) <= 1e-6, (pre, j)


def test_effect_metadata_matches_reference(g15):
    """name / knob_names / knob_ranges go into checkpoints (misc.save_checkpoint)."""
    for pre, fx in (("comp", audio.Compressor()), ("thresh", audio.Comp_Just_Thresh()), ("one", audio.Compressor_4c_OneSetting())):
        assert fx.name == str(g15[pre + "_name"])
        assert list(fx.knob_names) == [str(s) for s in g15[pre + "_knob_names"]]
        assert np.array_equal(np.asarray(fx.knob_ranges, dtype=np.float64), g15[pre + "_knob_ranges"])


def test_effects_declare_their_device_feed():
    """The fused feed is chosen by the effect's declaration, not its class name; the four rows the feed takes carry the fixed settings."""
    assert audio.Compressor_4c.feed_fx == audio.Compressor_4c_Large.feed_fx == audio.Compressor_4c_OneSetting.feed_fx == _lib.FX_COMP4C
    assert audio.Comp_Just_Thresh.feed_fx == _lib.FX_COMP4C and audio.Compressor.feed_fx == _lib.FX_COMP
    assert audio.Effect.feed_fx is None and audio.FileEffect.feed_fx is None
    assert np.array_equal(audio.Comp_Just_Thresh().feed_ranges(), [[-50, -10], [3, 3], [.05, .05], [1, 1]])
    assert np.array_equal(audio.Compressor_4c().feed_ranges(), audio.Compressor_4c().knob_ranges)
    assert audio.Compressor().feed_ranges().shape == (4, 2)


def test_compressor_identity_and_threshold_edges():
    rng = np.random.default_rng(3)
    x = (0.4 * rng.standard_normal(5000)).astype(np.float32)
    x[:300] = 0.0
    y = audio.compressor(x, thresh=30.0, ratio=4.0, attackrel=0.01)          # the envelope never reaches +30 dB: gain exactly 1
    assert np.array_equal(y, x)
    y1 = audio.compressor(x, thresh=-40.0, ratio=1.0, attackrel=0.01)        # ratio 1: the identity curve, to rounding
    assert np.abs(y1 - x).max() <= 1e-6 * np.abs(x).max()
    y2 = audio.compressor(x, thresh=-40.0, ratio=4.0, attackrel=0.01)
    assert np.abs(y2).max() < np.abs(x).max() and np.array_equal(audio.compressor(-x, -40.0, 4.0, 0.01), -y2)     # odd in x


@pytest.mark.parametrize("key", ["comp", "comp_t", "comp_one"])
def test_run_train_builds_the_compressor_keys(key):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_train.py"), "--effect", key, "--target", "nope"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "invalid target type" in r.stderr, r.stderr          # passed the effect check
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_train.py"), "--effect", "lowpass"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "does not build" in r.stderr and "comp_large" in r.stderr and key in r.stderr.split("not built")[0]


def test_dataset_items_of_the_envelope_compressor():
    """SynthAudioDataSet items behind a plain DataLoader: the target is the effect of the item's input at the item's knobs (on a GPU box the
    main process makes them with the device feed, elsewhere with the CPU generators and the host effect)."""
    import torch
    from torch.utils.data import DataLoader
    from signaltrain_amd import datasets
    np.random.seed(7); torch.manual_seed(7)
    fx = audio.Compressor()
    ds = datasets.SynthAudioDataSet(8192, fx, datapoints=6, y_size=2048, item_chunk=6)
    n = 0
    for x, y, k in DataLoader(ds, batch_size=3, num_workers=0):
        assert tuple(x.shape) == (3, 8192) and tuple(y.shape) == (3, 2048) and tuple(k.shape) == (3, 3)
        for i in range(3):
            xi, yi, ki = x[i].numpy(), y[i].numpy(), k[i].numpy()
            assert xi.dtype == np.float32 and float(np.abs(ki).max()) <= 0.5
            ref = fx.go(xi, ki)[0][-2048:]                                   # the polarity flip is shared by x and y and the effect is odd
            assert np.abs(yi - ref).max() <= 1e-5 * max(1e-3, np.abs(ref).max())
            n += 1
    assert n == 6


def test_synth_effect_refuses_bad_effects_and_knob_counts():
    lib = _lib.load()
    lo = (C.c_float * 4)(-30, 1, 1e-3, 1e-3); hi = (C.c_float * 4)(0, 5, 4e-2, 4e-2)

    def call(fx, K):
        return lib.st_synth_effect(fx, 1, 0, 4, 8192, 2048, K, 44100.0, lo, hi, 0, -1, None, None, None, None, None, None)
    for fx, K, what in ((7, 4, b"effect 7"), (-1, 3, b"effect -1"), (_lib.FX_COMP4C, 0, b"K=0"), (_lib.FX_COMP4C, 5, b"K=5"),
                        (_lib.FX_COMP, 4, b"K=4"), (_lib.FX_COMP, 1, b"K=1")):
        assert call(fx, K) == -1 and what in lib.st_last_error(), (fx, K, lib.st_last_error())
    assert call(_lib.FX_COMP, 3) == -1 and b"null" in lib.st_last_error()          # a valid id and count gets as far as the pointers
    assert call(_lib.FX_COMP4C, 1) == -1 and b"null" in lib.st_last_error()
    assert lib.st_synth_effect_scratch_floats(9, 4, 8192) == 0
    assert lib.st_synth_effect_scratch_floats(_lib.FX_COMP, 4, 8192) == lib.st_synth_comp4c_scratch_floats(4, 8192) == 4 * (8192 + 4)
    # st_synth_comp4c keeps its contract: K must be 4
    assert lib.st_synth_comp4c(1, 0, 4, 8192, 2048, 3, 44100.0, lo, hi, 0, -1, None, None, None, None, None, None) == -1 and b"K=3" in lib.st_last_error()
