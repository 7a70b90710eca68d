"""GPU: the fused feed of recorded pairs (st_file_feed, csrc/st_feed_files.h) -- kernel == host replica of the draw law == numpy gather, bit for bit,
over both pool formats, misaligned file offsets and every loop state of the mover; then AudioFileDataSet.batch_device_fused, DeviceFileLoader and
train.train(datapath=..., target_type="chunk") on top of it."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from signaltrain_amd import _lib, audio, datasets
from signaltrain_amd.datasets import file_feed_draw

pytestmark = pytest.mark.gpu
SEED = 1234


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Pool:
    """Files of int16 noise concatenated (odd lengths: misaligned offsets), as int16 and as the float32 read_audio_file makes of them."""

    def __init__(self, lens, K, seed=0):
        rng = np.random.default_rng(seed)
        self.lens = np.asarray(lens, dtype=np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.lens)[:-1]]).astype(np.int64)
        n = int(self.lens.sum())
        self.s16 = [rng.integers(-32768, 32768, size=n, dtype=np.int16) for _ in range(2)]
        self.f32 = [np.array(s / 32767.0, dtype=np.float32) for s in self.s16]
        self.K = K
        self.knobs = (rng.random((len(lens), K)) - 0.5).astype(np.float32) if K else None
        self._dev = {}

    def dev(self, fmt):
        if fmt not in self._dev:
            src = self.s16 if fmt == _lib.PCM_S16 else self.f32
            self._dev[fmt] = [torch.from_numpy(a).cuda() for a in src]
        if "t" not in self._dev:
            self._dev["t"] = (torch.from_numpy(self.off).cuda(), torch.from_numpy(self.lens).cuda(), torch.from_numpy(self.knobs).cuda() if self.K else None)
        return self._dev[fmt], self._dev["t"]

    def feed(self, first, B, L, ysz, fmt, augment=1, want_y=True, seed=SEED):
        (px, py), (off, ln, kt) = self.dev(fmt)
        x = torch.full((B, L), float("nan"), device="cuda")
        y = torch.full((B, ysz), float("nan"), device="cuda") if want_y else None
        kn = torch.full((B, self.K), float("nan"), device="cuda") if self.K else None
        meta = torch.full((B, 3), -7, dtype=torch.int64, device="cuda")
        _lib.check(_lib.load().st_file_feed(seed, first, B, L, ysz, self.K, fmt, _lib.ptr(px), _lib.ptr(py), _lib.ptr(off), _lib.ptr(ln), len(self.lens),
                                            int(self.lens.min()), int(self.lens.sum()), _lib.ptr(kt), augment, _lib.ptr(x), _lib.ptr(y), _lib.ptr(kn), _lib.ptr(meta),
                                            _stream()), "st_file_feed")
        torch.cuda.synchronize()
        return x.cpu().numpy(), (y.cpu().numpy() if want_y else None), (kn.cpu().numpy() if self.K else None), meta.cpu().numpy()

    def gather(self, meta, L, ysz):
        """The windows `meta` names, by numpy, from the float32 audio."""
        sg = np.where(meta[:, 2] == 1, np.float32(-1), np.float32(1))[:, None]
        p = self.off[meta[:, 0]] + meta[:, 1]
        x = np.stack([self.f32[0][q:q + L] for q in p]) * sg
        y = np.stack([self.f32[1][q + L - ysz:q + L] for q in p]) * sg
        return x, y, (self.knobs[meta[:, 0]] if self.K else None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(pool, first, B, L, ysz, fmt, augment=1):
    x, y, kn, meta = pool.feed(first, B, L, ysz, fmt, augment)
    f, s, fl = file_feed_draw(SEED, np.arange(first, first + B, dtype=np.uint64), pool.lens, L, bool(augment))
    assert np.array_equal(meta[:, 0], f) and np.array_equal(meta[:, 1], s) and np.array_equal(meta[:, 2], fl)        # kernel == replica
    xr, yr, kr = pool.gather(meta, L, ysz)
    assert np.array_equal(_bits(x), _bits(xr)) and np.array_equal(_bits(y), _bits(yr))                                  # kernel == host gather
    if pool.K:
        assert np.array_equal(_bits(kn), _bits(kr))
    return x, y, kn, meta


# L = 64: less than one trip; 1028: one full 256-lane x 4 trip plus a quad; 2052: one full two-trip workgroup plus a quad in a second one; 4100: three
SHAPES = [(64, 4, 0, 1, 1), (64, 64, 1, 3, 300), (1028, 4, 16, 5, 300), (1028, 1028, 3, 5, 7), (2052, 2052, 3, 4, 33), (4100, 2052, 2, 3, 300)]


@pytest.mark.parametrize("fmt", [_lib.PCM_F32, _lib.PCM_S16], ids=["f32", "s16"])
@pytest.mark.parametrize("L, ysz, K, nfiles, B", SHAPES)
def test_kernel_equals_replica_equals_gather(L, ysz, K, nfiles, B, fmt):
    lens = [(L + 5 + 38 * i) | 1 for i in range(nfiles)]                      # odd lengths: every second file starts on an odd sample
    pool = Pool(lens, K, seed=L + K)
    x, y, kn, meta = _check(pool, 0, B, L, ysz, fmt)
    if B >= 300:
        assert set(meta[:, 0]) == set(range(nfiles))
        res = (pool.off[meta[:, 0]] + meta[:, 1]) % 8
        assert set(res) == set(range(8)), set(res)                             # all 4-byte residues of a float32 span, all 2- and 8-sample residues of an int16 one
        assert set(res % 4) == {0, 1, 2, 3} and set(res % 2) == {0, 1}
        assert set(meta[:, 2]) == {0, 1}
    x0, _, _, m0 = _check(pool, 0, B, L, ysz, fmt, augment=0)
    assert not m0[:, 2].any() and np.array_equal(np.abs(x0), np.abs(x))


def test_s16_pool_equals_f32_pool_bit_for_bit():
    pool = Pool([1501, 1777, 2049], 3, seed=2)
    a = pool.feed(11, 300, 1028, 516, _lib.PCM_F32)
    b = pool.feed(11, 300, 1028, 516, _lib.PCM_S16)
    for u, v in zip(a[:3], b[:3]):
        assert np.array_equal(_bits(u), _bits(v))
    assert np.array_equal(a[3], b[3])


def test_every_int16_value_converts_as_read_audio_file_does():
    pool = Pool([65536 + 5], 0)
    allv = np.arange(-32768, 32768, dtype=np.int16)
    for i in range(2):
        pool.s16[i][:65536] = allv if i == 0 else allv[::-1]
        pool.f32[i] = np.array(pool.s16[i] / 32767.0, dtype=np.float32)
    starts = file_feed_draw(SEED, np.arange(64), pool.lens, 65536, False)[1]
    w0 = int(np.flatnonzero(starts == 0)[0])                                   # a window from sample 0 holds every int16 value once (x) and once reversed (y)
    x, y, _, meta = _check(pool, w0, 8, 65536, 65536, _lib.PCM_S16, augment=0)
    assert meta[0, 1] == 0 and np.array_equal(x[0], np.array(allv / 32767.0, dtype=np.float32))
    _check(pool, w0, 8, 65536, 65536, _lib.PCM_F32, augment=0)


def test_batching_and_window_indices_beyond_32_bits():
    pool = Pool([1501, 1777, 2049], 2, seed=3)
    L, ysz = 1028, 260
    whole = pool.feed(0, 16, L, ysz, _lib.PCM_S16)
    p1, p2 = pool.feed(0, 7, L, ysz, _lib.PCM_S16), pool.feed(7, 9, L, ysz, _lib.PCM_S16)
    for u, v, t in zip(p1, p2, whole):
        assert np.array_equal(np.concatenate([u, v]), t)
    hi = _check(pool, 2 ** 32 + 5, 16, L, ysz, _lib.PCM_S16)
    lo = _check(pool, 5, 16, L, ysz, _lib.PCM_S16)
    assert not np.array_equal(hi[3], lo[3]) and not np.array_equal(hi[0], lo[0])
    other = pool.feed(0, 16, L, ysz, _lib.PCM_S16, seed=SEED + 1)
    assert not np.array_equal(other[3], whole[3])


def test_long_file_has_starts_beyond_2_to_24():
    n = 2 ** 24 + 2 ** 20 + 3
    pool = Pool([n], 1, seed=4)
    x, y, kn, meta = _check(pool, 0, 512, 256, 64, _lib.PCM_S16)
    big = meta[:, 1][meta[:, 1] > 2 ** 24]
    assert len(big) > 0 and (big % 2 == 1).any() and meta[:, 1].max() < n - 256


def test_y_may_be_null():
    pool = Pool([1501, 1777, 2049], 3, seed=5)
    a = pool.feed(3, 40, 1028, 516, _lib.PCM_F32)
    b = pool.feed(3, 40, 1028, 516, _lib.PCM_F32, want_y=False)
    assert b[1] is None and np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[2]), _bits(b[2])) and np.array_equal(a[3], b[3])


# ---------------------------------------------------------------------------------------------------------------- the dataset on top
@pytest.fixture(scope="module")
def la2a_root(tmp_path_factory):
    from tests.test_device_feed import make_file_dataset
    return make_file_dataset(str(tmp_path_factory.mktemp("ff") / "la2a"), n_train=4, n_val=2, seconds=1.0)


def _ds(root, seed, **kw):
    np.random.seed(seed)
    return datasets.AudioFileDataSet(8192, audio.FileEffect(root), path=root + "/Train/", datapoints=kw.pop("datapoints", 64), y_size=2048, **kw)


def test_batch_device_fused_items_are_windows_of_the_files(la2a_root):
    ds = _ds(la2a_root, 3, augment=True)
    x, y, k, meta = ds.batch_device_fused(16, with_meta=True)
    assert x.shape == (16, 8192) and y.shape == (16, 2048) and k.shape == (16, 3) and x.is_cuda and ds._feed_count == 16
    x, y, k, meta = (t.cpu().numpy() for t in (x, y, k, meta))
    f, s, fl = file_feed_draw(ds._feed_seed, np.arange(16), [len(a) for a in ds.x], 8192, True)
    assert np.array_equal(meta, np.stack([f, s, fl], 1))
    for b in range(16):
        sg = -1.0 if meta[b, 2] else 1.0
        a, t, p = ds.x[meta[b, 0]], ds.y[meta[b, 0]], meta[b, 1]
        assert np.array_equal(x[b], sg * a[p:p + 8192]) and np.array_equal(y[b], sg * t[p + 8192 - 2048:p + 8192])
        assert np.array_equal(k[b], ds.knobs_nn(ds.knobs[meta[b, 0]]))
    # the property tests/test_gpu_model_api.py::test_train_driver_file_dataset_three_knobs checks for batch_device, by its search
    xs, ys, found = x[0], y[0], False
    for a, b in zip(ds.x, ds.y):
        for sgn in (1.0, -1.0):
            for p in np.where(np.isclose(a[:len(a) - 8192], sgn * xs[0], atol=1e-7))[0]:
                if np.allclose(a[p:p + 8192], sgn * xs, atol=1e-7) and np.allclose(b[p + 8192 - 2048:p + 8192], sgn * ys, atol=1e-7):
                    found = True
    assert found
    # both pool formats serve the same stream
    d32 = _ds(la2a_root, 3, augment=True)
    x32, y32, k32 = d32.batch_device_fused(16, pcm="f32")
    assert np.array_equal(_bits(x32.cpu().numpy()), _bits(x)) and np.array_equal(_bits(y32.cpu().numpy()), _bits(y))
    assert ds._fdev[("cuda:0", "s16")]["x"].dtype == torch.int16 and d32._fdev[("cuda:0", "f32")]["x"].dtype == torch.float32


def test_batch_device_fused_follows_the_numpy_seed(la2a_root):
    a, b, c = _ds(la2a_root, 3), _ds(la2a_root, 3), _ds(la2a_root, 4)
    for _ in range(2):
        ba, bb, bc = a.batch_device_fused(8), b.batch_device_fused(8), c.batch_device_fused(8)
        assert all(torch.equal(u, v) for u, v in zip(ba, bb))
        assert not torch.equal(ba[0], bc[0])
    first = _ds(la2a_root, 3).batch_device_fused(8)
    assert not torch.equal(first[0], ba[0])                                   # the stream moves on


def _c4_dataset(root, n_train=3, n_val=2, seconds=1.0, sr=44100):
    """A recorded Compressor_4c set: target names carry four world-unit knobs inside the effect's ranges."""
    rng = np.random.default_rng(9)
    n = int(seconds * sr)
    for sub, cnt in (("Train", n_train), ("Val", n_val)):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
        for i in range(cnt):
            t = np.arange(n) / sr
            x = (0.6 * np.sin(2 * np.pi * (90 + 40 * i) * t) * (0.2 + 0.8 * (np.sin(2 * np.pi * 4 * t) > 0)) + 0.02 * rng.standard_normal(n)).astype(np.float32)
            kw = [round(float(rng.uniform(-28, -5)), 2), round(float(rng.uniform(1.5, 4.5)), 3), round(float(rng.uniform(2e-3, 3e-2)), 5), round(float(rng.uniform(2e-3, 3e-2)), 5)]
            yv = audio.compressor_4controls(x, *kw)
            audio.write_audio_file(os.path.join(root, sub, f"input_{i}_.wav"), (x * 32767).astype(np.int16), sr)
            audio.write_audio_file(os.path.join(root, sub, f"target_{i}_Compressor_4c__{kw[0]:g}__{kw[1]:g}__{kw[2]:g}__{kw[3]:g}.wav"),
                                   (np.clip(yv, -1, 1) * 32767).astype(np.int16), sr)
    return root


@pytest.fixture(scope="module")
def c4_root(tmp_path_factory):
    return _c4_dataset(str(tmp_path_factory.mktemp("ff4") / "c4"))


def test_rerun_target_is_the_effect_on_the_gathered_window(c4_root, la2a_root):
    """target_type="chunk" on the device: y = effect.go_device(x) of the gathered (and flipped) window, against the HOST effect.go_wc of that window at
    the file's world-unit knobs.  Bounds quoted, not invented: st_compressor_4c against the host compressor is held to 1e-5 * max(1e-3, max|ref|) per window
    (tests/test_gpu_model_api.py::test_device_compressor_matches_reference_golden); a feed's target against st_compressor_4c on the same window
    to 1e-6 * max|y| (tests/test_gpu_feed.py, tests/test_gpu_effects.py)."""
    fx = audio.Compressor_4c()
    np.random.seed(5)
    ds = datasets.AudioFileDataSet(4096, fx, path=c4_root + "/Train/", datapoints=64, y_size=1024, rerun=True, augment=True)
    x, y, k, meta = ds.batch_device_fused(12, with_meta=True)
    assert y.shape == (12, 1024) and set(meta[:, 2].tolist()) == {0, 1}
    y4 = fx.go_device(x, k, 1024)
    print("device-vs-device", float((y - y4).abs().max()), float(y4.abs().max()))
    assert float((y - y4).abs().max()) <= 1e-6 * float(y4.abs().max())
    xh, yh, meta = x.cpu().numpy(), y.cpu().numpy(), meta.cpu().numpy()
    for b in range(12):
        sg = -1.0 if meta[b, 2] else 1.0
        assert np.array_equal(xh[b], sg * ds.x[meta[b, 0]][meta[b, 1]:meta[b, 1] + 4096])
        ref = fx.go_wc(xh[b], ds.knobs[meta[b, 0]])[0][-1024:]
        err, bound = np.abs(yh[b] - ref).max(), 1e-5 * max(1e-3, np.abs(ref).max())
        print("window", b, "err", err, "bound", bound)
        assert err <= bound, (b, err, bound)
    # an effect that exists only as recordings has no device form
    la = datasets.AudioFileDataSet(4096, audio.FileEffect(la2a_root), path=c4_root + "/Train/", datapoints=8, view_of=ds, rerun=True)
    with pytest.raises(NotImplementedError, match="rerun=True"):
        la.batch_device_fused(4)


def test_device_file_loader_yields_the_inline_stream(la2a_root):
    a, b = _ds(la2a_root, 6, datapoints=100), _ds(la2a_root, 6, datapoints=100)
    ld = datasets.DeviceFileLoader(a, 16, "cuda:0", gen_windows=48)
    assert len(ld) == 6 and ld.per_call == 3
    for epoch in range(2):
        got = [tuple(t.clone() for t in item) for item in ld]
        assert len(got) == 6
        for x, y, k in got:
            xi, yi, ki = b.batch_device_fused(16)
            assert x.shape == (16, 8192) and torch.equal(x, xi) and torch.equal(y, yi) and torch.equal(k, ki)
    assert a._feed_count == 2 * 96


def test_train_chunk_target_stays_on_the_device(c4_root, tmp_path, monkeypatch):
    from signaltrain_amd import misc, nn_proc, train
    nn_proc._QUIET = True
    seen = {}
    real_loop = train.train_loop

    def spy(model, engine, effect, device, epochs, batch_size, lr_sched, mom_sched, dataloader, dataloader_val, *a, **kw):
        seen["train"], seen["val"] = type(dataloader), type(dataloader_val)
        return real_loop(model, engine, effect, device, epochs, batch_size, lr_sched, mom_sched, dataloader, dataloader_val, *a, **kw)

    def no_workers(*a, **kw):
        raise AssertionError("a torch DataLoader was built: the chunk target left the device")
    monkeypatch.setattr(train, "train_loop", spy)
    monkeypatch.setattr(train, "DataLoader", no_workers)
    monkeypatch.chdir(tmp_path)
    model = train.train(effect=audio.Compressor_4c(), epochs=2, n_data_points=256, batch_size=32, device=torch.device("cuda:0"), datapath=c4_root,
                        target_type="chunk", device_feed=True, compute_dtype="bf16_all", lr_max=2e-4)
    assert seen["train"] is datasets.DeviceFileLoader and seen["val"] is datasets.DeviceFileLoader
    assert model.num_knobs == 4 and os.path.isfile("modelcheckpoint.tar")
    sd, rv = misc.load_checkpoint("modelcheckpoint.tar", device="cpu")
    assert sd and rv["knob_names"] == ['threshold', 'ratio', 'attackTime', 'releaseTime']
    vals = [float(l.split()[-1]) for l in open("vl_avg_out.dat").read().strip().splitlines()]
    assert len(vals) == 2 and all(np.isfinite(vals)) and all(v > 0 for v in vals)
