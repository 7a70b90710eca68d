"""GPU: a predict session fed block by block -- st_predict_stream_* / StepEngine.open_stream / PredictStream.push / StepEngine.predict_channels /
predict.predict_stream.

C channels advance in lockstep; the history stays in HBM; every output sample is emitted as soon as its window is complete.  Checked against st_predict_long on
the concatenated signal (bit for bit where the batches hold the same rows, to 1e-6 of max|y| otherwise -- the bound test_batch_independence holds for "same
kernels, other batch"), against the float64 oracle window by window at gpu_checks.TOL, across partitions into pushes, lengths, channels, arithmetic levels,
sample formats and knob layouts, and for everything a push must leave alone.  Inputs are those of tests/test_gpu_predict_long.py."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from signaltrain_amd import _lib
from tests import gpu_checks as G
from tests.dims_table import geo_of
from tests.test_gpu_predict_long import K, KN, LEVELS, _model, case, engine, length, lengths, oracle, signal

pytestmark = pytest.mark.gpu

KN2 = -KN[::-1].copy()


def cuts(n, sizes):
    """[(start, stop, final)] of pushes of the given sizes, then the rest as the final one."""
    out, at = [], 0
    for m in sizes:
        assert m % 4 == 0 and at + m <= n
        out.append((at, at + m, False)); at += m
    return out + [(at, n, True)]


def even(n, m):
    return cuts(n, [m] * (n // m))


def three(geo, n):
    """L + 3 y, then 4 y, then the rest: batches of 4, 4 and 1 windows at nine windows."""
    return cuts(n, [geo["L"] + 3 * geo["y"], 4 * geo["y"]])


def run(st, sig, parts, knobs=KN, counts=None):
    """Push sig [n] or [C, n] (a device tensor) through the session part by part; the concatenated output.  counts: receives (emitted, plan's emitted) per push."""
    outs = []
    for a, b, final in parts:
        want = st.plan(b - a, final)[2]
        y = st.push(sig[..., a:b], G.t(knobs) if not torch.is_tensor(knobs) else knobs, final=final)
        if counts is not None:
            counts.append((int(y.shape[-1]), want))
        outs.append(y)
    return torch.cat(outs, dim=-1)


def rel(a, b):
    b = G.n(b) if torch.is_tensor(b) else np.asarray(b, np.float64)
    return float(np.abs(G.n(a) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("row", ["n256", "h256", "ragged", None])
@pytest.mark.parametrize("level", ["f32", "bf16_all"])
def test_same_rows_give_the_same_bits(level, row):
    """One channel, B = 4, pushes of L + 3 y, 4 y and the rest: the batches hold windows 0-3, 4-7 and 8, the rows of predict_long(batch=4)'s batches, and
    the same kernels run on them in the same order -- the result is bit-equal."""
    with LEVELS[level]():
        eng, geo, P = engine(row, 4)
        n = length(geo)
        sig = G.t(signal(n))
        ref = eng.predict_long(sig, G.t(KN), batch=4)
        st = eng.open_stream(1, batch=4)
        counts = []
        got = run(st, sig, three(geo, n), counts=counts)
        assert [c for c, _ in counts] == [4 * geo["y"], 4 * geo["y"], n - (geo["L"] - geo["y"]) - 8 * geo["y"]]
        assert got.dtype == torch.float32 and got.is_cuda and got.shape == ref.shape and torch.equal(got, ref), (level, row, rel(got, ref))
        assert st.received == n and st.emitted == ref.numel() and st.closed and st.pending == 0


@pytest.mark.parametrize("level", ["f32", "bf16_all"])
def test_the_partition_does_not_matter(level):
    """Pushes of 4 samples, of y, one final push, and a seeded random partition (multiples of four, some below y so that some pushes complete no window and
    only carry, a ragged final): each within 1e-6 of max|y| of predict_long(batch=16), and every push emits what st_predict_stream_plan says."""
    with LEVELS[level]():
        eng, geo, P = engine("n256", 16)
        L, y = geo["L"], geo["y"]
        n = length(geo)
        sig = G.t(signal(n, seed=6))
        ref = eng.predict_long(sig, G.t(KN), batch=16)
        rng = np.random.default_rng(17)
        sizes, left = [], n
        while left > 3 * y // 2:
            sizes.append(4 * int(rng.integers(1, 3 * y // 8))); left -= sizes[-1]
        assert min(sizes) < y < max(sizes) and left % 4 != 0
        st = eng.open_stream(1, batch=16)
        for name, parts in (("m=4", even(n, 4)), ("m=y", even(n, y)), ("one", cuts(n, [])), ("random", cuts(n, sizes))):
            st.reset()
            counts = []
            got = run(st, sig, parts, counts=counts)
            assert all(c == w for c, w in counts) and sum(c for c, _ in counts) == ref.numel() == got.numel(), name
            if name in ("m=4", "random"):
                assert any(c == 0 for c, _ in counts)
            e = rel(got, ref)
            print(f"predict stream partition {name} [{level}]: {len(parts)} pushes rel={e:.2e} bit-equal={bool(torch.equal(got, ref))}")
            assert e <= 1e-6, (level, name, e)


@pytest.mark.parametrize("row", ["n256", "tiny"])
def test_every_length_around_the_boundaries(row):
    """lengths(L, y) as one final push and as y-sized pushes plus a final one, against the float64 oracle window by window at TOL; nothing is emitted where
    n <= L - y.  tiny: L < N and y = 32."""
    eng, geo, P = engine(row, 3)
    L, y = geo["L"], geo["y"]
    st = eng.open_stream(1, batch=3)
    full = signal(L + 4 * y)
    for n in lengths(L, y):
        sig = G.t(full[:n].copy())
        ref = None
        for name, parts in (("one", cuts(n, [])), ("m=y", even(n, y))):
            st.reset()
            got = run(st, sig, parts)
            assert tuple(got.shape) == (max(n - (L - y), 0),) and st.emitted == got.numel() and st.received == n, (row, n, name)
            if n <= L - y:
                assert got.numel() == 0
                continue
            if ref is None:
                geo_, P_ = case(row)
                ref = oracle(full[:n].copy(), KN, P_, geo_)
            e = rel(got, ref)
            print(f"predict stream length n={n} [{row} {name}]: {got.numel()} samples rel={e:.2e}")
            assert e <= G.TOL, (row, n, name, e)


def test_channels():
    """Three distinct signals with one knob row per channel: the oracle per channel at TOL and three one-channel sessions at 1e-6; one knob row equals the row
    repeated bit for bit; five channels at B = 4 have more rows than a batch in every push."""
    eng, geo, P = engine("n256", 16)
    n = length(geo)
    host = np.stack([signal(n, seed=30 + c) for c in range(5)])
    kn = np.stack([KN, KN2, 0.5 * KN, -KN, 0.3 * KN2]).astype(np.float32)
    sig = G.t(host)
    parts = three(geo, n)
    st3 = eng.open_stream(3, batch=16)
    got = run(st3, sig[:3], parts, knobs=kn[:3])
    assert tuple(got.shape) == (3, n - (geo["L"] - geo["y"]))
    st1 = eng.open_stream(1, batch=16)
    solo = []
    for c in range(5):
        st1.reset()
        solo.append(run(st1, sig[c], parts, knobs=kn[c]))
    for c in range(3):
        ref = oracle(host[c], kn[c], P, geo)
        e, e1 = rel(got[c], ref), rel(got[c], solo[c])
        print(f"predict stream channel {c} of 3: oracle rel={e:.2e} one-channel session rel={e1:.2e}")
        assert e <= G.TOL and e1 <= 1e-6, (c, e, e1)
    assert rel(got[1], got[0]) > 100 * G.TOL               # the channels really differ
    st3.reset(); one = run(st3, sig[:3], parts, knobs=KN)
    st3.reset(); rep = run(st3, sig[:3], parts, knobs=np.tile(KN, (3, 1)))
    assert torch.equal(one, rep)
    eng4, _, _ = engine("n256", 4)
    st5 = eng4.open_stream(5, batch=4)
    for name, p in (("L+3y,4y,rest", parts), ("m=y", even(n, geo["y"]))):
        st5.reset()
        got5 = run(st5, sig, p, knobs=kn)
        for c in range(5):
            e = rel(got5[c], solo[c])
            assert e <= 1e-6, (name, c, e)
        print(f"predict stream 5 channels at B=4 [{name}]: max rel={max(rel(got5[c], solo[c]) for c in range(5)):.2e}")


@pytest.mark.parametrize("row", ["n384", None])
@pytest.mark.parametrize("level", list(LEVELS))
def test_levels(level, row):
    """Every arithmetic level: the stream against predict_long at the same level at 1e-6."""
    with LEVELS[level]():
        eng, geo, P = engine(row, 3)
        n = length(geo, hops=5)
        sig = G.t(signal(n, seed=5))
        ref = eng.predict_long(sig, G.t(KN), batch=3)
        got = run(eng.open_stream(1, batch=3), sig, cuts(n, [geo["L"] + 2 * geo["y"], 3 * geo["y"]]))      # 3, 3, 1 windows
        e = rel(got, ref)
        print(f"predict stream vs predict_long [{level} {row or 'default'}]: bit-equal={bool(torch.equal(got, ref))} rel={e:.2e}")
        assert got.shape == ref.shape and e <= 1e-6, (level, row, e)


def test_knob_automation():
    """One push per window (L samples, then y-sized pushes), two settings alternating: predict_long with the same rows per window at 1e-6, the oracle at TOL,
    and the second setting is audible."""
    eng, geo, P = engine("n256", 4)
    L, y = geo["L"], geo["y"]
    n = length(geo)
    host = signal(n, seed=8)
    sig = G.t(host)
    nwin = int(eng.lib.st_predict_windows(C.byref(eng.dims), n))
    assert nwin == 9
    rows = np.stack([KN if w % 2 == 0 else KN2 for w in range(nwin)]).astype(np.float32)
    st = eng.open_stream(1, batch=4)
    outs = []
    for a, b, final in cuts(n, [L] + [y] * ((n - L) // y)):
        first, cnt, _, _ = st.plan(b - a, final)
        assert cnt == 1
        outs.append(st.push(sig[a:b], G.t(rows[first]), final=final))
    got = torch.cat(outs)
    ref_dev = eng.predict_long(sig, G.t(rows))
    ref = oracle(host, rows, P, geo)
    one = oracle(host, KN, P, geo)
    e, ed = rel(got, ref), rel(got, ref_dev)
    print(f"predict stream knob automation: oracle rel={e:.2e} predict_long rel={ed:.2e}")
    assert e <= G.TOL and ed <= 1e-6
    assert np.abs(ref - one).max() > 100 * G.TOL * np.abs(one).max()


@pytest.mark.parametrize("level", ["f32", "bf16_all"])
def test_int16_blocks_equal_their_float_image(level):
    with LEVELS[level]():
        eng, geo, P = engine("n256", 4)
        n = length(geo)
        s16 = np.clip(np.round(signal(n, seed=7) * 32767.0 * 2.5), -32768, 32767).astype(np.int16)
        assert s16.min() == -32768 and s16.max() == 32767                       # both ends of the format occur
        img = (s16.astype(np.float64) / 32767.0).astype(np.float32)
        st = eng.open_stream(1, batch=4)
        parts = cuts(n, [geo["L"] + geo["y"], 4, geo["y"] - 4, 2 * geo["y"]])     # with pushes that only carry: the history is the float image
        a = run(st, torch.from_numpy(s16).to(G.DEV), parts)
        st.reset()
        b = run(st, G.t(img), parts)
        assert a.dtype == torch.float32 and a.shape == b.shape and torch.equal(a, b)
        assert float(b.abs().max()) > 0.1
        assert rel(a, eng.predict_long(G.t(img), G.t(KN), batch=4)) <= 1e-6


def test_guards():
    """block and out are views into larger buffers: NaN (int16: full scale) fills the pitch padding of block, a sentinel lies around and behind every
    channel's emitted span of out.  The results are finite and equal the unpadded run's, the sentinels stand, and parameters, moments, gradients and the
    engine's workspace are bit-unchanged."""
    eng, geo, P = engine("n256", 4)
    n = length(geo)
    assert n % 4 != 0
    for name in ("grads", "m", "v"):
        getattr(eng, name).copy_(torch.randn_like(eng.params))
    eng.ws.copy_(torch.randint(0, 255, eng.ws.shape, dtype=torch.uint8, device=G.DEV))
    before = {k: getattr(eng, k).clone() for k in ("params", "grads", "m", "v", "scalars", "ws")}
    host = np.stack([signal(n, seed=9), signal(n, seed=19)])
    parts = three(geo, n)
    st = eng.open_stream(2, batch=4)
    PAD, POISON = 64, 12345.0
    for dtype, src in ((torch.float32, host), (torch.int16, np.round(host * 20000).astype(np.int16))):
        sig = torch.from_numpy(src).to(G.DEV)
        st.reset()
        clean = run(st, sig, parts)
        st.reset()
        outs = []
        for a, b, final in parts:
            m, m4 = b - a, (b - a + 3) // 4 * 4
            buf = torch.full((2, PAD + m4 + PAD), float("nan") if dtype == torch.float32 else 32767, dtype=dtype, device=G.DEV)
            buf[:, PAD:PAD + m] = sig[:, a:b]
            emit = st.plan(m, final)[2]
            e4 = (emit + 3) // 4 * 4
            obuf = torch.full((2, PAD + e4 + PAD), POISON, dtype=torch.float32, device=G.DEV)
            y = st.push(buf[:, PAD:PAD + m], G.t(KN), final=final, out=obuf[:, PAD:PAD + e4])
            assert y.data_ptr() == obuf[:, PAD:].data_ptr() and tuple(y.shape) == (2, emit)
            assert bool((obuf[:, :PAD] == POISON).all()) and bool((obuf[:, PAD + emit:] == POISON).all())
            outs.append(y.clone())
        got = torch.cat(outs, dim=1)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, clean), dtype
        assert emit % 4 != 0                                  # the last quad of the final push was clipped
    for k, v in before.items():
        assert torch.equal(getattr(eng, k), v), k


def test_training_trajectory_is_untouched():
    """Train steps with the pushes of a session interleaved: the trajectory of the train steps alone, bit for bit -- and the session, whose parameters moved
    under it, follows them (its head is rebuilt after a step)."""
    geo, P = case("n256")
    _, X, Y, KNB, _ = G.make_case(3, 21, K=K, geo=geo_of("n256"))
    a = G.new_engine(G.dims_of(geo, 3, K)); a.load_state_dict(P)
    b = G.new_engine(G.dims_of(geo, 3, K)); b.load_state_dict(P)
    n = length(geo)
    sig = G.t(signal(n, seed=10))
    parts = three(geo, n)
    st = a.open_stream(1)
    for i in range(3):
        a.train_step(G.t(X), G.t(KNB), G.t(Y), 1e-3)
        b.train_step(G.t(X), G.t(KNB), G.t(Y), 1e-3)
        s0, s1, final = parts[i]
        y = st.push(sig[s0:s1], G.t(KN), final=final)
        if i == 2:      # the last window was computed with the parameters as they are now
            ref = b.predict_long(sig, G.t(KN))
            assert rel(y, ref[-y.numel():]) <= 1e-6
    for k in ("params", "m", "v", "grads", "scalars"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.step_count == b.step_count == 3


def test_sessions_are_independent():
    """Two sessions on one engine pushed alternately equal their solo runs bit for bit; reset() and the same pushes repeat the bits; a push after the final
    one raises, in Python and in the library."""
    eng, geo, P = engine("n256", 4)
    n = length(geo)
    sa, sb = G.t(signal(n, seed=40)), G.t(signal(n, seed=41))
    pa, pb = three(geo, n), even(n, geo["y"])
    A, B_ = eng.open_stream(1, batch=4), eng.open_stream(1, batch=4)
    solo_a = run(A, sa, pa)
    solo_b = run(B_, sb, pb, knobs=KN2)
    A.reset(); B_.reset()
    assert (A.received, A.emitted, A.pending, A.closed) == (0, 0, 0, False)
    oa, ob = [], []
    for i in range(max(len(pa), len(pb))):
        if i < len(pa):
            oa.append(A.push(sa[pa[i][0]:pa[i][1]], G.t(KN), final=pa[i][2]))
        if i < len(pb):
            ob.append(B_.push(sb[pb[i][0]:pb[i][1]], G.t(KN2), final=pb[i][2]))
    assert torch.equal(torch.cat(oa), solo_a) and torch.equal(torch.cat(ob), solo_b)
    assert not torch.equal(solo_a, solo_b)
    with pytest.raises(RuntimeError, match="closed"):
        A.push(sa[:4], G.t(KN))
    rc = eng.lib.st_predict_stream_push(C.byref(A.dims), _lib.ptr(eng.params), C.byref(A.s), 0, C.c_void_p(sa.data_ptr()), 4, 4, 0, _lib.ptr(G.t(KN)), 1,
                                        None, 0, _lib.ptr(A.state), _lib.ptr(A.ws), None)
    assert rc == -1 and b"closed" in eng.lib.st_last_error()
    A.reset()
    assert torch.equal(run(A, sa, pa), solo_a)
    with pytest.raises(ValueError, match="multiple of 4"):
        B_.reset(); B_.push(sb[:6], G.t(KN))


def test_python_routes():
    """predict_channels on a [2, n] recording against two predict_long calls at 1e-6; predict.predict_stream over numpy blocks (one channel, and two with a
    knob callable) concatenates to the same."""
    from signaltrain_amd.predict import predict_stream
    m, P, geo = _model()
    L, y = geo["L"], geo["y"]
    n = L + 4 * y + 777
    host = np.stack([signal(n, seed=11), signal(n, seed=12)])
    eng = m.engine(torch.empty((), dtype=torch.float32, device=G.DEV).expand(8, L))
    refs = torch.stack([eng.predict_long(G.t(host[c]), G.t(KN)) for c in range(2)])
    got = eng.predict_channels(G.t(host), G.t(KN))
    assert tuple(got.shape) == (2, n - (L - y)) and got.dtype == torch.float32
    e = rel(got, refs)
    print(f"predict_channels vs predict_long per channel: rel={e:.2e}")
    assert e <= 1e-6
    out = torch.zeros(2, n + 3, dtype=torch.float32, device=G.DEV)           # rows on 16-byte boundaries
    assert torch.equal(eng.predict_channels(G.t(host), G.t(KN), out=out), got) and torch.equal(out[:, :got.shape[1]], got)
    blocks = [host[0, a:b] for a, b, _ in even(n, y)]
    ys = list(predict_stream(blocks, KN, m, L, y, batch_size=8))
    assert len(ys) == len(blocks) and all(isinstance(v, np.ndarray) and v.dtype == np.float32 and v.ndim == 1 for v in ys)
    assert ys[0].size == 0 and ys[L // y - 1].size == y
    cat = np.concatenate(ys)
    assert cat.shape == (n - (L - y),) and np.abs(cat - G.n(refs[0])).max() <= 1e-6 * np.abs(G.n(refs[0])).max()
    seen = []
    ys2 = list(predict_stream((host[:, a:b] for a, b, _ in even(n, y)), lambda i: (seen.append(i), KN)[1], m, L, y, batch_size=8))
    assert seen == list(range(len(blocks)))
    cat2 = np.concatenate(ys2, axis=1)
    assert cat2.shape == (2, n - (L - y)) and np.abs(cat2 - G.n(refs)).max() <= 1e-6 * np.abs(G.n(refs)).max()
    with pytest.raises(ValueError, match="chunk_size"):
        list(predict_stream(blocks, KN, m, L, y // 2, batch_size=8))


def test_wide_geometry_raises_at_open_and_falls_back_in_predict_channels():
    """The 65536-sample window runs the wide autoencoder path, which has no predict session: open_stream raises, predict_channels warns once and returns
    what predict_long's batched route returns channel by channel."""
    from signaltrain_amd import engine as engine_mod
    from signaltrain_amd import predict
    m, P, geo = _model(scale=8)
    L, y = geo["L"], geo["y"]
    assert not _lib.load().st_predict_supported(C.byref(_lib.geometry(8, 4, K, 1)))
    eng = m.engine(torch.empty((), dtype=torch.float32, device=G.DEV).expand(2, L))
    with pytest.raises(RuntimeError, match="st_predict_supported"):
        eng.open_stream(2)
    n = L + y + 5
    host = np.stack([signal(n, seed=12), signal(n, seed=13)])
    engine_mod._warned_channels_unsupported = False
    with pytest.warns(RuntimeWarning, match="batched route"):
        a = eng.predict_channels(G.t(host), G.t(KN), batch=2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b = eng.predict_channels(G.t(host), G.t(KN), batch=2)               # the second time: no warning
    assert torch.equal(a, b) and tuple(a.shape) == (2, n - (L - y))
    for c in range(2):
        ref = predict.predict_long(host[c], KN, m, L, y, batch_size=2)
        assert np.abs(G.n(a[c]) - ref).max() <= 1e-6 * np.abs(ref).max(), c
