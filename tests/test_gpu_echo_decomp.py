"""GPU: the Echo and DeCompressor_4c effects on the device -- st_echo (csrc/st_echo.h) against a float64 restatement of the reference's echo()
(audio.py:430-443), the two effects in the fused feed (csrc/st_feed.h: the clean window, the knobs and the polarity are ST_FX_COMP4C's bit for bit;
ST_FX_ECHO's target is st_echo's, ST_FX_DECOMP4C's input st_compressor_4c's, in both forms of its compressor stage), and datasets / training steps
on their minibatches."""
import ctypes as C
import itertools
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SR = 44100.0
BOUND = 1e-5           # of max(1e-3, max |ref|): the bound between a device effect and its host reference elsewhere in the suite
ECHO_WIDE = np.array([[100, 1500], [0.1, 0.9], [0, 3], [0, 0]], dtype=np.float64)      # fractional world delays and echo counts: the feed's rounding is live
ECHO_FAMILIES = (1, 3, 5, 6, 7)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _signals(L, seed=0):
    rng = np.random.default_rng(seed)
    box = np.full(L, 0.1, dtype=np.float32); box[L // 5:L // 2] = 0.8; box[L // 2:] = 0.2
    imp = np.zeros(L, dtype=np.float32); imp[0] = 1.0
    return {"white": (2.0 * rng.random(L) - 1.0).astype(np.float32), "impulse": imp, "box": box}


def _echo(x, kw, ysz):
    """st_echo on device tensors x [B, L], world knobs kw [B, 3]"""
    from signaltrain_amd import _lib
    x = x.contiguous(); kw = kw.to(torch.float32).contiguous()
    y = torch.empty(x.shape[0], ysz, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().st_echo(_lib.ptr(x), _lib.ptr(kw), SR, x.shape[0], x.shape[1], ysz, _lib.ptr(y), _stream()), "st_echo")
    return y


def _comp4c(x, kw, ysz):
    from signaltrain_amd import _lib
    y = torch.empty(x.shape[0], ysz, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().st_compressor_4c(_lib.ptr(x.contiguous()), _lib.ptr(kw.contiguous()), SR, x.shape[0], x.shape[1], ysz, _lib.ptr(y), _stream()), "st_compressor_4c")
    return y


def _ref64(x, delay, ratio, echoes):
    """echo() of the reference in float64 on the float32 knob values the device receives"""
    L = len(x)
    x = x.astype(np.float64); y = x.copy()
    for i in range(1, int(np.rint(np.float32(echoes))) + 1):
        dl = i * float(np.float32(delay)); D = int(np.floor(dl)); diff = dl - D
        a = np.zeros(L); b = np.zeros(L)
        if D < L: a[D:] = x[:L - D]
        if D + 1 < L: b[D + 1:] = x[:L - D - 1]
        y += float(np.float32(ratio)) ** i * ((1 - diff) * a + diff * b)
    return y


def _ratio(y, ref):
    return float(np.abs(y.astype(np.float64) - ref).max() / max(1e-3, np.abs(ref).max()))


@pytest.mark.parametrize("L,ysz", [(2048, 2048), (8192, 2048), (2050, 1027), (1000, 4)])
def test_echo_matches_the_reference(L, ysz):
    """The whole window; a tail whose first echo starts before it (delay > L - ysz) and inside it; an odd window with 2 * 1487 >= L > 1487 and an odd
    tail; a tail shorter than a wave.  One launch per signal, every row with its own knobs: 8 delays x 4 echo counts x 3 ratios."""
    from signaltrain_amd import _lib
    knobs = list(itertools.product((1, 1.5, 333.3, 400, 1487, L - 1, L, 3 * L), (0.4, 1.0, -0.5), (0, 1, 2, _lib.ECHO_MAX)))
    kw = torch.tensor(knobs, dtype=torch.float32, device="cuda")
    worst = 0.0
    for name, x in _signals(L, seed=L).items():
        X = torch.from_numpy(x).cuda().expand(len(knobs), L).contiguous()
        y = _echo(X, kw, ysz).cpu().numpy()
        for b, (d, r, e) in enumerate(knobs):
            q = _ratio(y[b], _ref64(x, d, r, e)[-ysz:])
            worst = max(worst, q)
            assert q <= BOUND, (L, ysz, name, d, r, e, q)
    print(f"st_echo vs float64 echo(), L={L} ysz={ysz}: worst ratio {worst:.3g}")


def test_echo_bad_knobs_give_nan_rows_only():
    L, ysz = 8192, 2048
    x = _signals(L, seed=5)["white"]
    nan, inf = float("nan"), float("inf")
    knobs = [(400, 0.6, 2), (0, 0.6, 2), (333.3, 0.6, 1), (0.5, 0.6, 1), (1, 1.0, 8), (nan, 0.6, 1), (-3, 0.6, 1), (1487, -0.5, 3), (400, 0.6, 9),
             (400, 0.6, 8.5), (400, 0.6, -1), (400, 0.6, -0.4), (400, nan, 1), (inf, 0.6, 1), (400, 0.6, nan), (8191, 0.4, 2)]
    bad = {1, 3, 5, 6, 8, 10, 12, 13, 14}
    y = _echo(torch.from_numpy(np.stack([x] * len(knobs))).cuda(), torch.tensor(knobs, device="cuda"), ysz).cpu().numpy()
    for b, (d, r, e) in enumerate(knobs):
        if b in bad:
            assert np.isnan(y[b]).all(), (b, d, r, e)
        else:
            assert _ratio(y[b], _ref64(x, d, r, e)[-ysz:]) <= BOUND, (b, d, r, e)


@pytest.mark.parametrize("ranges", [None, ECHO_WIDE[:3]], ids=["reference", "wide"])
def test_echo_effect_go_device(ranges):
    from signaltrain_amd import audio
    fx = audio.Echo()
    if ranges is not None:
        fx.knob_ranges = ranges
    x = _signals(8192, seed=6)["white"]
    kn = torch.tensor([[-0.5, -0.5, -0.5], [0.1003, 0.1, 0.2], [0.5, 0.5, 0.5], [-0.2, 0.3, -0.1]], device="cuda")
    X = torch.from_numpy(np.stack([x] * 4)).cuda()
    y = fx.go_device(X, kn, 2048)
    kw = audio._knobs_wc_device(fx.knob_ranges, kn, "cuda")
    kwr = torch.stack([kw[:, 0].round(), kw[:, 1], kw[:, 2].round()], 1)
    assert torch.equal(y, _echo(X, kwr, 2048)) and y.shape == (4, 2048)
    if ranges is not None:
        assert not torch.equal(kw, kwr)
    for b in range(4):
        ref = audio.echo(x, float(kwr[b, 0]), float(kwr[b, 1]), float(kwr[b, 2]))[-2048:]
        assert _ratio(y[b].cpu().numpy(), ref.astype(np.float64)) <= BOUND, b
    assert torch.equal(fx.go_device(X, kn), _echo(X, kwr, 8192))


# ---- the fused feed
def _feed(fx, K, rng, B, augment, first=1000, seed=77, L=8192, ysz=2048, chooser=-1, scratch=False, families=None, pink=False):
    """(x, y, knobs, scratch) of st_synth_effect_families; pink: a [B, L] buffer in the caller-made noise's place (windows no library transform
    serves; the families forced with it use no 1/f noise)"""
    from signaltrain_amd import _lib
    lib = _lib.load()
    x = torch.empty(B, L, device="cuda"); y = torch.empty(B, ysz, device="cuda"); kn = torch.empty(B, K, device="cuda")
    lo = (C.c_float * 4)(*[float(v) for v in rng[:, 0]]); hi = (C.c_float * 4)(*[float(v) for v in rng[:, 1]])
    scr = torch.zeros(int(lib.st_synth_effect_scratch_floats(fx, B, L)), device="cuda") if scratch else None
    pk = torch.zeros(B, L, device="cuda") if pink else None
    _lib.check(lib.st_synth_effect_families(fx, _lib.family_mask(families), seed, first, B, L, ysz, K, SR, lo, hi, augment, chooser, _lib.ptr(pk),
                                            _lib.ptr(x), _lib.ptr(y), _lib.ptr(kn), _lib.ptr(scr), _stream()), "st_synth_effect_families")
    torch.cuda.synchronize()
    return x, y, kn, scr


def _echo_world_knobs(rng, kn):
    from signaltrain_amd import audio
    kw = audio._knobs_wc_device(rng[:3], kn, "cuda")
    return torch.stack([kw[:, 0].round(), kw[:, 1], kw[:, 2].round()], 1)


ECHO_CASES = {"L8192": dict(L=8192, ysz=2048), "family5": dict(L=8192, ysz=2048, chooser=5), "family3": dict(L=8192, ysz=2048, chooser=3),
              "L2048": dict(L=2048, ysz=2048, chooser=6), "L1002": dict(L=1002, ysz=501, chooser=6, pink=True)}


@pytest.mark.parametrize("augment", [0, 1], ids=["plain", "augment"])
@pytest.mark.parametrize("case", list(ECHO_CASES))
def test_feed_echo(case, augment):
    """Drawn from the echo's family set and with families 5, 3 and 6 forced; L = 1002 takes the feed's sample-by-sample pass."""
    from signaltrain_amd import _lib, audio
    kw_args = dict(ECHO_CASES[case], families=ECHO_FAMILIES)
    L, ysz = kw_args["L"], kw_args["ysz"]
    x, y, kn, _ = _feed(_lib.FX_ECHO, 3, ECHO_WIDE, 8, augment, **kw_args)
    c4 = _feed(_lib.FX_COMP4C, 4, audio.Compressor_4c().feed_ranges(), 8, augment, **kw_args)
    assert torch.equal(x, c4[0]) and torch.equal(kn, c4[2][:, :3])                      # the clean window and the knob draws are the compressor feed's
    assert kn.shape == (8, 3) and float(kn.min()) >= -0.5 and float(kn.max()) <= 0.5 and bool(torch.isfinite(x).all())
    kw = _echo_world_knobs(ECHO_WIDE, kn)
    assert torch.equal(y, _echo(x, kw, ysz))
    assert len(set(kw[:, 2].tolist())) > 1 and float(kw[:, 0].min()) >= 100 and float(kw[:, 2].max()) <= 3
    xh, yh, kwh = x.cpu().numpy(), y.cpu().numpy(), kw.cpu().numpy()
    for b in range(8):
        assert _ratio(yh[b], _ref64(xh[b], *kwh[b])[-ysz:]) <= BOUND, (case, b)
    # a window is a function of its index: one batch of 8 == two of 4
    parts = [_feed(_lib.FX_ECHO, 3, ECHO_WIDE, 4, augment, first=f, **kw_args) for f in (1000, 1004)]
    for i, whole in enumerate((x, y, kn)):
        assert torch.equal(whole, torch.cat([p[i] for p in parts])), (case, i)
    # the reference's own ranges: delay 400, two echoes
    fx = audio.Echo()
    x2, y2, kn2, _ = _feed(_lib.FX_ECHO, 3, fx.feed_ranges(), 8, augment, **kw_args)
    kw2 = _echo_world_knobs(fx.feed_ranges(), kn2)
    assert torch.equal(x2, x) and torch.equal(kn2, kn) and torch.equal(y2, _echo(x2, kw2, ysz))
    assert kw2[:, 0].tolist() == [400.0] * 8 and kw2[:, 2].tolist() == [2.0] * 8
    if L >= 2048:
        assert not torch.equal(y2, x2[:, -ysz:])


DECOMP_CASES = {"K4": dict(K=4, L=8192, ysz=2048, fx="Compressor_4c"), "K1": dict(K=1, L=8192, ysz=2048, fx="Comp_Just_Thresh"),
                "two_chunks": dict(K=4, L=16384, ysz=4096, fx="Compressor_4c", chooser=6, pink=True)}


@pytest.mark.parametrize("augment", [0, 1], ids=["plain", "augment"])
@pytest.mark.parametrize("case", list(DECOMP_CASES))
def test_feed_decompressor(case, augment):
    """The in-workgroup form against the lane-per-window form through the scratch, and both against ST_FX_COMP4C and st_compressor_4c: all bit for bit.
    L = 16384 is two chunks of the in-workgroup compressor, so its carry crosses a chunk edge while the window is rewritten in place."""
    from signaltrain_amd import _lib, audio
    c = dict(DECOMP_CASES[case]); K = c.pop("K"); rng = getattr(audio, c.pop("fx"))().feed_ranges()
    L, ysz, B = c["L"], c["ysz"], 8
    x, y, kn, _ = _feed(_lib.FX_DECOMP4C, K, rng, B, augment, **c)
    xs, ys, kns, scr = _feed(_lib.FX_DECOMP4C, K, rng, B, augment, scratch=True, **c)
    assert torch.equal(x, xs) and torch.equal(y, ys) and torch.equal(kn, kns)            # the two forms of the compressor stage agree
    cx, cy, ckn, cscr = _feed(_lib.FX_COMP4C, K, rng, B, augment, scratch=True, **c)
    assert torch.equal(kn, ckn) and kn.shape == (B, K)
    assert torch.equal(y, cx[:, -ysz:])                                                 # the target is the clean window's tail
    kw = scr[B * L:B * L + 4 * B].reshape(B, 4).clone()                                 # the world knobs the feed used
    assert torch.equal(kw, cscr[B * L:B * L + 4 * B].reshape(B, 4))
    assert torch.equal(x, _comp4c(cx, kw, L))                                           # the input is the compressed window, all of it
    assert torch.equal(x[:, -ysz:], cy)
    assert torch.equal(cy, _feed(_lib.FX_COMP4C, K, rng, B, augment, **c)[1])
    assert bool(torch.isfinite(x).all()) and float((x - cx).abs().max()) > 1e-3
    parts = [_feed(_lib.FX_DECOMP4C, K, rng, 4, augment, first=f, **c) for f in (1000, 1004)]
    for i, whole in enumerate((x, y, kn)):
        assert torch.equal(whole, torch.cat([p[i] for p in parts])), (case, i)


# ---- datasets and training
@pytest.mark.parametrize("cls", ["Echo", "DeCompressor_4c"])
def test_dataset_batches_and_one_training_step(cls):
    from signaltrain_amd import audio, datasets, nn_proc
    nn_proc._QUIET = True
    np.random.seed(3); torch.manual_seed(3)
    fx = getattr(audio, cls)()
    K = len(fx.knob_names)

    def check(x, y, kn, B=16):
        assert x.is_cuda and x.shape == (B, 8192) and y.shape == (B, 2048) and kn.shape == (B, K) and x.dtype == y.dtype == kn.dtype == torch.float32
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all()) and not torch.equal(y, x[:, -2048:])
    ds = datasets.SynthAudioDataSet(8192, fx, y_size=2048)
    assert ds.choosers == (ECHO_FAMILIES if cls == "Echo" else (0, 1, 2, 4, 6, 7))
    x, y, kn = ds.batch_device(16)
    assert ds._feed_count == 16                                                          # the fused branch
    check(x, y, kn)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    ds2 = datasets.SynthAudioDataSet(8192, fx, y_size=2048, augment=False)
    x2, y2, k2 = ds2.batch_device(16, generator=g)                                       # the generator-driven branch: the effect's go_device
    assert ds2._feed_count == 0
    check(x2, y2, k2)
    if cls == "DeCompressor_4c":                                                         # (target, input) = (clean tail, compressed window)
        assert float((x2[:, -2048:] - y2).abs().max()) > 1e-3
        assert float((x2[:, -2048:].abs() - y2.abs()).max()) <= 1e-6                     # a compressor only ever turns the signal down
    rec = datasets.DeviceRecycledDataSet(8192, fx, datapoints=16, y_size=2048, device="cuda:0", gen_batch=16)
    xr, yr, kr = next(rec.batches(16))
    check(xr, yr, kr)
    model = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=K, sr=44100).to("cuda")
    eng = model.engine(torch.zeros(16, 8192, device="cuda"))
    loss = float(eng.train_step(x, kn, y, 1e-4)[0])
    assert np.isfinite(loss) and loss > 0


@pytest.mark.parametrize("cls", ["Echo", "DeCompressor_4c"])
def test_train_on_the_device_feed(tmp_path, monkeypatch, cls):
    """train.train takes the fused feed and the recycled validation set for both effects without special cases."""
    from signaltrain_amd import audio, datasets, misc, nn_proc, train
    nn_proc._QUIET = True
    made = []
    fused = datasets.SynthAudioDataSet.batch_device

    def counting(self, B, *a, **kw):
        out = fused(self, B, *a, **kw); made.append((B, self._feed_count)); return out
    monkeypatch.setattr(datasets.SynthAudioDataSet, "batch_device", counting)
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0); np.random.seed(0)
    fx = getattr(audio, cls)()
    train.train(effect=fx, epochs=2, n_data_points=256, batch_size=64, device=torch.device("cuda:0"), device_feed=True, lr_max=2e-4)
    assert made and all(c > 0 for _, c in made) and sum(B for B, _ in made) == 2 * 256 + 64      # every window came out of the fused feed
    lines = [l.split() for l in open("vl_avg_out.dat").read().strip().splitlines()]
    assert len(lines) == 2 and all(np.isfinite(float(l[-1])) for l in lines)
    sd, rv = misc.load_checkpoint("modelcheckpoint.tar", device="cpu")
    assert rv["effect_name"] == fx.name and list(rv["knob_names"]) == fx.knob_names and np.array_equal(rv["knob_ranges"], fx.knob_ranges)
    assert all(torch.isfinite(v).all() for v in sd.values())
