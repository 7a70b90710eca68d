"""CPU: the argument rules of the whole-signal inference entries (signaltrain_amd/engine.py: _recording, _recording_pair, _pcm, _knob_rows, _knob_settings,
_adam_state; signaltrain_amd/predict.py: _nwin) on CPU tensors -- no engine, no library, no GPU.  Every StepEngine entry applies these and nothing else to its
recordings, knobs and Adam state, so what holds here holds for predict_long, eval_pool, encode_long / decode_long, the knob fits and scores and the session."""
import numpy as np
import pytest
import torch

from oracle import host_audio
from signaltrain_amd import _lib
from signaltrain_amd.engine import _adam_state, _knob_rows, _knob_settings, _pcm, _recording, _recording_pair
from signaltrain_amd.predict import _nwin
from tests.test_predict_long_host import lengths

CPU = torch.device("cpu")
K = 3
ALIGN = {torch.float32: 16, torch.int16: 8}        # pcm_align in csrc/st_api.hip


def view_at(dtype, byte_off, n=40):
    """n samples of `dtype` as a view that starts byte_off bytes behind a 16-byte boundary."""
    size = torch.empty((), dtype=dtype).element_size()
    buf = torch.arange(n + 16, dtype=torch.float32).to(dtype)
    first = (-buf.data_ptr() % 16 + byte_off) // size
    v = buf[first:first + n]
    assert v.data_ptr() % 16 == byte_off and v.is_contiguous()
    return v


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
def test_recording_accepts_aligned_and_clones_off_the_boundary(dtype):
    t = view_at(dtype, 0)
    assert _recording("e", "signal", t, CPU) is t
    for off in ((4, 8, 12) if dtype == torch.float32 else (2, 4, 6, 10, 12, 14)):
        v = view_at(dtype, off)
        r = _recording("e", "signal", v, CPU)
        assert r.data_ptr() != v.data_ptr() and r.data_ptr() % ALIGN[dtype] == 0 and r.is_contiguous() and r.dtype == dtype and torch.equal(r, v), off
    empty = torch.empty(0, dtype=dtype)
    assert _recording("e", "signal", empty, CPU) is empty


def test_recording_takes_an_int16_view_at_8_mod_16_as_it_is():
    v = view_at(torch.int16, 8)
    assert _recording("e", "signal", v, CPU) is v
    assert _recording("e", "signal", view_at(torch.float32, 8), CPU).data_ptr() % 16 == 0       # float32 quads are 16 bytes


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
def test_recording_makes_a_strided_view_contiguous(dtype):
    v = view_at(dtype, 0)[::2]
    r = _recording("e", "signal", v, CPU)
    assert not v.is_contiguous() and r.is_contiguous() and r.data_ptr() % ALIGN[dtype] == 0 and torch.equal(r, v)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
def test_recording_refusals_name_the_entry(dtype):
    good = torch.zeros(8, dtype=dtype)
    for bad in (good.reshape(2, 4), good.double(), good.numpy(), [0.0] * 8, None, torch.zeros(8, dtype=dtype, device="meta")):
        with pytest.raises(ValueError, match=r"^some_entry: signal must be a 1-D float32 or int16 tensor on cpu$"):
            _recording("some_entry", "signal", bad, CPU)
    with pytest.raises(ValueError, match=r"^some_entry: pool_x must be a non-empty 1-D float32 or int16 tensor on cpu$"):
        _recording("some_entry", "pool_x", good[:0], CPU, nonempty=True)
    assert _recording("some_entry", "pool_x", good, CPU, nonempty=True) is good


def test_recording_pair():
    s16 = torch.tensor([0, 1, -1, 12345, 32767, -32767, -32768, 7], dtype=torch.int16)
    f32 = torch.linspace(-1, 1, 8)
    with pytest.raises(ValueError, match=r"^e: signal has 8 samples, target 7$"):
        _recording_pair("e", s16, s16[:7], CPU)
    with pytest.raises(ValueError, match=r"^e: the recording has 7 samples, target 8$"):
        _recording_pair("e", f32[:7], s16, CPU, first="the recording")
    with pytest.raises(ValueError, match=r"^e: target must be a 1-D"):
        _recording_pair("e", f32, f32.double(), CPU)
    want = (s16.double() / 32767.0).float()
    assert want[4] == 1.0 and want[5] == -1.0 and want[6] == np.float32(-32768 / 32767) and want[1] == np.float32(1 / 32767)
    for a, b in ((s16, f32), (f32, s16)):
        x, y = _recording_pair("e", a, b, CPU)
        assert x.dtype == y.dtype == torch.float32 and x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
        assert torch.equal(x if a is s16 else y, want) and (y if a is s16 else x) is f32
    for t in (s16, f32):                              # equal dtypes: nothing is converted, nothing copied
        x, y = _recording_pair("e", t, t, CPU)
        assert x is t and y is t
    v = view_at(torch.int16, 2, 8)                    # each side is aligned by its own rule
    x, y = _recording_pair("e", v, view_at(torch.int16, 8, 8), CPU)
    assert x.data_ptr() % 8 == 0 and x.data_ptr() != v.data_ptr() and torch.equal(x, v) and y.data_ptr() % 16 == 8


def test_pcm():
    assert _pcm(torch.zeros(4, dtype=torch.int16)) == _lib.PCM_S16 and _pcm(torch.zeros(4)) == _lib.PCM_F32 and _lib.PCM_S16 != _lib.PCM_F32


def test_knob_rows():
    n = 5
    per = ": one row, or one per window (5 windows for 99 samples)"
    for given, rows in ((torch.rand(K), 1), (torch.rand(1, K), 1), (torch.rand(n, K), n), ([0.1, 0.2, 0.3], 1), (np.zeros((n, K)), n)):
        kn, r = _knob_rows("e", given, K, CPU, (1, n), per)
        assert r == rows and tuple(kn.shape) == (rows, K) and kn.dtype == torch.float32 and kn.is_contiguous()
        assert torch.equal(kn, torch.as_tensor(given).float().reshape(rows, K))
    for rows in (2, n + 1):
        with pytest.raises(ValueError, match=rf"^e: knobs has {rows} rows: one row, or one per window \(5 windows for 99 samples\)$"):
            _knob_rows("e", torch.rand(rows, K), K, CPU, (1, n), per)
    with pytest.raises(ValueError, match=r"^e: knobs has 1 rows for 4 files$"):
        _knob_rows("e", torch.rand(K), K, CPU, (4,), " for 4 files")
    t = torch.rand(K, n).t()
    kn, r = _knob_rows("e", t, K, CPU, (1, n), per)
    assert not t.is_contiguous() and kn.is_contiguous() and r == n and torch.equal(kn, t)
    assert _knob_rows("e", None, 0, CPU, (1, n), per) == (None, 1)          # a model without knobs


def test_knob_settings():
    nwin, n, S = 5, 99, 4
    kn, single = _knob_settings("e", torch.rand(K), K, nwin, n, CPU)
    assert single and tuple(kn.shape) == (1, 1, K)
    g = torch.rand(S, K)
    for strict in (False, True):
        kn, single = _knob_settings("e", g, K, nwin, n, CPU, strict=strict)
        assert not single and tuple(kn.shape) == (S, 1, K) and torch.equal(kn[:, 0], g) and kn.is_contiguous()
        for rows in (1, nwin):
            g3 = torch.rand(K, rows, S).permute(2, 1, 0)
            kn, single = _knob_settings("e", g3, K, nwin, n, CPU, strict=strict)
            assert not single and tuple(kn.shape) == (S, rows, K) and torch.equal(kn, g3) and kn.is_contiguous()
        with pytest.raises(ValueError, match=r"^e: no knob setting$"):
            _knob_settings("e", torch.rand(0, 1, K), K, nwin, n, CPU, strict=strict)
    with pytest.raises(ValueError, match=r"^e: knobs \[S, rows, K\] has 2 rows per setting: one row, or one per window \(5 windows for 99 samples\)$"):
        _knob_settings("e", torch.rand(S, 2, K), K, nwin, n, CPU)
    assert tuple(_knob_settings("e", torch.rand(S, 2, K), K, 2, n, CPU)[0].shape) == (S, 2, K)
    for bad in (torch.rand(K), torch.rand(S, 2, K), torch.rand(S, K + 1), torch.rand(S, nwin, K + 1)):          # what score_knobs / fit_knobs_multi take
        with pytest.raises(ValueError, match=r"^e: knobs must be \[S, 3\] or \[S, rows, 3\] with one row per setting, or one per window \(5 windows for 99 samples\), not "):
            _knob_settings("e", bad, K, nwin, n, CPU, strict=True)


def test_adam_state():
    like = torch.rand(4, K)
    m, v, first = _adam_state(None, like, CPU)
    assert first == 1 and m.shape == v.shape == like.shape and m.dtype == v.dtype == torch.float32 and not m.any() and not v.any()
    assert m.data_ptr() != v.data_ptr()
    m0, v0 = torch.rand(4 * K), torch.rand(K, 4).t().double()
    keep = m0.clone(), v0.clone()
    m, v, first = _adam_state((m0, v0, 7.0), like, CPU)
    assert first == 7 and isinstance(first, int) and m.shape == v.shape == like.shape and m.dtype == v.dtype == torch.float32
    assert m.is_contiguous() and v.is_contiguous() and torch.equal(m, m0.reshape(4, K)) and torch.equal(v, v0.float())
    m.fill_(9.0); v.fill_(9.0)
    assert torch.equal(m0, keep[0]) and torch.equal(v0, keep[1])


@pytest.mark.parametrize("L,y", [(8192, 2048), (256, 96)])
def test_nwin_is_the_references_window_count(L, y):
    for n in lengths(L, y):
        want = host_audio.sliding_window(np.zeros(n, np.float32), L, overlap=L - y).shape[0] if n >= L else 1      # below one window the reference has no answer
        assert _nwin(n, L, y) == want, n
