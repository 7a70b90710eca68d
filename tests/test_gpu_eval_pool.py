"""GPU: a folder of recordings through the model in one device call -- st_eval_pool / StepEngine.eval_pool / AudioFileDataSet.evaluate.

The pool is the one the device feeds keep (concatenated audio, per-file offsets, lengths and knob rows); batch rows are (file, window) pairs.  Checked against
st_predict_long on every file alone, against the float64 oracle, against float64 statistics formed from predict_long's output (never from the entry's own),
across offsets of every residue mod 4, sample formats, forms (predict only / score only) and for everything the call must leave alone."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from signaltrain_amd import _lib
from tests import gpu_checks as G
from tests.dims_table import geo_of
from tests.test_gpu_predict_long import K, LEVELS, case, engine, lengths, oracle, signal

pytestmark = pytest.mark.gpu

SHORT = [3, 7, 18, 29, 40]          # files too short for a single output sample at every row used here (L - y >= 64)
LOUD = 1.0e3                        # the level of one such file: a read across its border shows at once
FIG = ("logcosh", "abs", "sq", "peak", "t_sq", "y_sq")        # stats columns 1 .. 6
_RUNS, _ORACLES = {}, {}


def make_files(geo, seed=1):
    """The nine lengths around the window and hop boundaries plus the five short ones, shuffled (offsets of every residue mod 4, aligned and unaligned
    files with windows); every file at its own level, its own target and its own knob row; the 40-sample file at LOUD."""
    L, y = geo["L"], geo["y"]
    base = lengths(L, y) + SHORT
    lens = [int(base[i]) for i in np.random.default_rng(seed).permutation(len(base))]
    rng = np.random.default_rng(seed + 50)
    xs, ts = [], []
    for f, n in enumerate(lens):
        level = LOUD if n == 40 else 0.2 + 0.8 * (f + 1) / len(lens)
        xs.append((level * signal(n, seed=20 + f) / 0.55).astype(np.float32))
        ts.append((0.7 * level * signal(n, seed=60 + f) / 0.55).astype(np.float32))
    kn = rng.uniform(-0.5, 0.5, size=(len(lens), K)).astype(np.float32)
    return lens, xs, ts, kn


def layout(lens, align4=False):
    off, o = [], 0
    for n in lens:
        off.append(o)
        o += n if not align4 else (n + 3) // 4 * 4
    return np.array(off, np.int64), max(o, 1)


def pool_of(chunks, off, total, fill=0.0):
    p = np.full(total, fill, chunks[0].dtype)
    for a, o in zip(chunks, off):
        p[o:o + a.size] = a
    return p


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(G.DEV)


def per_file_reference(eng, xs, kn, B):
    """st_predict_long on every file alone (the same engine, the same batch size): float32 numpy per file, empty where the file has no output sample."""
    return [eng.predict_long(dev(x), dev(kn[f]) if kn is not None else None, batch=B).cpu().numpy() for f, x in enumerate(xs)]


def ragged_run(row, B, level):
    """One run of the ragged pool per (row, B, level), shared by the tests below and never modified."""
    key = (row, B, level)
    if key not in _RUNS:
        with LEVELS[level]():
            eng, geo, P = engine(row, B)
            lens, xs, ts, kn = make_files(geo)
            off, total = layout(lens)
            stats, out = eng.eval_pool(dev(pool_of(xs, off, total)), dev(pool_of(ts, off, total)), off, np.array(lens, np.int64), dev(kn), want_out=True, batch=B)
            ref = per_file_reference(eng, xs, kn, B)
            off4, total4 = layout(lens, align4=True)
            stats4, out4 = eng.eval_pool(dev(pool_of(xs, off4, total4, fill=LOUD)), dev(pool_of(ts, off4, total4, fill=LOUD)), off4, np.array(lens, np.int64), dev(kn),
                                         want_out=True, batch=B)
        _RUNS[key] = dict(geo=geo, P=P, lens=lens, xs=xs, ts=ts, kn=kn, off=off, off4=off4, stats=stats.cpu().numpy(), out=out.cpu().numpy(), ref=ref,
                          stats4=stats4.cpu().numpy(), out4=out4.cpu().numpy())
    return _RUNS[key]


def file_oracle(row, r):
    if row not in _ORACLES:
        _ORACLES[row] = [oracle(x, r["kn"][f], r["P"], r["geo"]) if x.size > r["geo"]["L"] - r["geo"]["y"] else np.zeros(0) for f, x in enumerate(r["xs"])]
    return _ORACLES[row]


# ---------------------------------------------------------------------------------------------- statistics: the references
def logcosh32(e):
    """The kernels' formula (st_misc.h ola_loss4_kernel) in float32 numpy."""
    a = np.abs(e).astype(np.float32)
    u = np.expm1(np.float32(0.5) * a)
    sh = np.float32(0.5) * (u + u / (u + np.float32(1.0)))
    small = np.log1p(np.float32(2.0) * sh * sh)
    big = a + np.log1p(np.exp(np.float32(-2.0) * a)) - np.float32(0.69314718056)
    return np.where(a < 8.0, small, big).astype(np.float32)


def stats64(y_hat, t):
    """float64 numpy over predict_long's output and the target: the reference."""
    y, t = y_hat.astype(np.float64), t.astype(np.float64)
    e = np.abs(y - t)
    lc = e + np.log1p(np.exp(-2.0 * e)) - np.log(2.0)
    return {"logcosh": lc.sum(), "abs": e.sum(), "sq": (e * e).sum(), "peak": e.max() if e.size else 0.0, "t_sq": (t * t).sum(), "y_sq": (y * y).sum()}


def slot_sums32(v, y):
    """float32 sums of the kernel's slots, in the kernel's order (the tree of ola_loss4_kernel): a slot is 256 consecutive samples of a window (zeros behind the
    file's end and behind the window's), per lane ((q0 + q1) + q2) + q3 in sample order, then the xor tree over the 64 lanes.  Returns the slot sums."""
    f = np.float32
    nwin, nslot = -(-v.size // y), -(-y // 256)
    w = np.zeros((nwin, nslot * 256), f)
    for i in range(nwin):
        seg = v[i * y:(i + 1) * y]
        w[i, :seg.size] = seg
    q = w.reshape(nwin * nslot, 64, 4)
    lane = ((q[:, :, 0] + q[:, :, 1]).astype(f) + q[:, :, 2]).astype(f) + q[:, :, 3]
    lane = lane.astype(f)
    idx = np.arange(64)
    for o in (1, 2, 4, 8, 16, 32):
        lane = (lane + lane[:, idx ^ o]).astype(f)
    return lane[:, 0]


def stats32(y_hat, t, y):
    """The restatement whose distance from stats64 is the yardstick: float32 per-sample terms, float32 sums per 256 samples (slot_sums32), float64 above that."""
    f = np.float32
    d = (t.astype(f) - y_hat.astype(f)).astype(f)
    terms = {"logcosh": logcosh32(d), "abs": np.abs(d), "sq": d * d, "t_sq": t.astype(f) * t.astype(f), "y_sq": y_hat.astype(f) * y_hat.astype(f)}
    out = {k: float(slot_sums32(v.astype(f), y).astype(np.float64).sum()) for k, v in terms.items()}
    out["peak"] = float(np.abs(d).max()) if d.size else 0.0
    return out


def moved_by(y_hat, t, delta):
    """What a change of y_hat by at most delta per sample can move each figure (first order in the worst direction, plus delta^2 where squared)."""
    y, t = y_hat.astype(np.float64), t.astype(np.float64)
    e = np.abs(y - t)
    return {"logcosh": float(np.tanh(e).sum() * delta), "abs": e.size * delta, "sq": float((2 * e * delta + delta * delta).sum()), "peak": delta, "t_sq": 0.0,
            "y_sq": float((2 * np.abs(y) * delta + delta * delta).sum())}


def check_stats(label, stats, refs, ts, geo, shifted):
    """stats [nfiles][8] of the entry against the float64 reference over predict_long's per-file output.  The yardstick of a figure is delta = the largest
    relative deviation, over the files with output samples, of the float32 restatement (stats32: the kernel's terms and slot tree in numpy) from the float64 reference; the entry may deviate by 4 delta
    of the reference (the project's rule: four times the float32-vs-float64 deviation of the same formula) -- plus, where its batches are not
    predict_long's (shifted), what a 1e-6 max|y| change of y_hat can move the figure.  Returns {figure: (delta, largest measured relative deviation)}."""
    L, y = geo["L"], geo["y"]
    rows = []
    for f, yh in enumerate(refs):
        if yh.size == 0:
            assert not stats[f].any(), (label, f)
            continue
        t = ts[f][L - y:]
        rows.append((f, stats64(yh, t), stats32(yh, t, y), moved_by(yh, t, 1e-6 * float(np.abs(yh).max())) if shifted else None))
        assert stats[f][0] == yh.size and stats[f][7] == 0.0
    res, bad = {}, []
    for c, k in enumerate(FIG):
        delta = max(abs(s32[k] - s64[k]) / max(abs(s64[k]), 1e-300) for _, s64, s32, _ in rows)
        worst = 0.0
        for f, s64, s32, mv in rows:
            dev_ = abs(float(stats[f][1 + c]) - s64[k])
            worst = max(worst, dev_ / max(abs(s64[k]), 1e-300))
            if dev_ > 4 * delta * abs(s64[k]) + (mv[k] if mv else 0.0):
                bad.append((k, f, dev_ / max(abs(s64[k]), 1e-300), delta))
        res[k] = (delta, worst)
        print(f"eval_pool statistics [{label}] {k:8s}: delta={delta:.3e} measured={worst:.3e}")
    assert not bad, (label, bad)
    return res


# ---------------------------------------------------------------------------------------------- 1: one file is st_predict_long
@pytest.mark.parametrize("level", ["f32", "bf16_all"])
@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_one_file_is_predict_long(level, fmt):
    """A single-file pool at offset 0 with the same d->B: out[L - y:] is st_predict_long's result bit for bit, out[:L - y] is 0; n_out is exact, max |e| is
    the float32 max |t - y_hat| exactly, and the sums hold the 4-delta bound without any allowance (the batches are predict_long's)."""
    with LEVELS[level]():
        B = 4
        eng, geo, P = engine("n256", B)
        L, y = geo["L"], geo["y"]
        n = L + 7 * y + 777 % y
        kn = np.array([[0.1, -0.3, 0.25, -0.45]], np.float32)
        x, t = signal(n, seed=31), (0.8 * signal(n, seed=32)).astype(np.float32)
        if fmt == "s16":
            xs, tg = np.round(x * 30000).astype(np.int16), np.round(t * 30000).astype(np.int16)
            x, t = (xs.astype(np.float64) / 32767.0).astype(np.float32), (tg.astype(np.float64) / 32767.0).astype(np.float32)
        else:
            xs, tg = x, t
        stats, out = eng.eval_pool(dev(xs), dev(tg), np.array([0], np.int64), np.array([n], np.int64), dev(kn), want_out=True, batch=B)
        ref = eng.predict_long(dev(xs), dev(kn[0]), batch=B)
        assert out.dtype == torch.float32 and tuple(out.shape) == (n,) and stats.dtype == torch.float64 and tuple(stats.shape) == (1, 8)
        assert torch.equal(out[L - y:], ref) and not bool(out[:L - y].any()) and float(ref.abs().max()) > 0.05
        st, yh = stats.cpu().numpy(), ref.cpu().numpy()
        assert st[0, 0] == n - (L - y) and st[0, 7] == 0.0
        assert st[0, 4] == float(np.abs(t[L - y:] - yh).max())               # float32 subtraction, its exact image in double
        check_stats(f"one file {level} {fmt}", st, [yh], [t], geo, shifted=False)


# ---------------------------------------------------------------------------------------------- 2: ragged pool
RAGGED = [("n256", 3), ("n256", 7), ("h256", 4), ("ragged", 4), ("tiny", 4)]


@pytest.mark.parametrize("level", ["f32", "bf16_all"])
@pytest.mark.parametrize("row,B", RAGGED)
def test_ragged_pool(row, B, level):
    """Fourteen files, offsets of every residue mod 4, short files that share a batch and long ones that span several: every file's span against
    st_predict_long on that file alone within 1e-6 of max|y| (the project's bound between two batch sizes), at f32 also against the float64 oracle within
    gpu_checks.TOL; files without an output sample have an all-zero span and an all-zero statistics row."""
    r = ragged_run(row, B, level)
    geo, lens, off = r["geo"], r["lens"], r["off"]
    L, y = geo["L"], geo["y"]
    assert set(int(o) % 4 for o in off) == {0, 1, 2, 3}
    assert {int(o) % 4 == 0 for o, n in zip(off, lens) if n > L - y} == {True, False}
    assert sum(n <= L - y for n in lens) >= 7 and max(lens) > L + 3 * y
    orc = file_oracle(row, r) if level == "f32" else None
    worst, worst_o = 0.0, 0.0
    for f, (o, n) in enumerate(zip(off, lens)):
        span = r["out"][o:o + n]
        assert not span[:min(L - y, n)].any(), (f, n)
        if n <= L - y:
            assert not r["stats"][f].any(), (f, n)
            assert r["ref"][f].size == 0
            continue
        got, ref = span[L - y:].astype(np.float64), r["ref"][f].astype(np.float64)
        assert got.shape == ref.shape == (n - (L - y),)
        e = float(np.abs(got - ref).max() / np.abs(ref).max())
        worst = max(worst, e)
        assert e <= 1e-6, (row, B, level, f, n, e)
        if orc is not None:
            eo = float(np.abs(got - orc[f]).max() / np.abs(orc[f]).max())
            worst_o = max(worst_o, eo)
            assert eo <= G.TOL, (row, B, f, n, eo)
    assert np.isfinite(r["out"]).all() and np.abs(r["out"]).max() < 50.0        # nothing of the LOUD neighbour leaked
    print(f"eval_pool ragged [{row} B={B} {level}]: vs predict_long per file rel={worst:.2e}" + (f", vs float64 oracle rel={worst_o:.2e}" if orc is not None else ""))


# ---------------------------------------------------------------------------------------------- 3: alignment changes no bit
@pytest.mark.parametrize("level", ["f32", "bf16_all"])
@pytest.mark.parametrize("row,B", RAGGED)
def test_alignment_changes_no_bit(row, B, level):
    """The same files in the same order with every offset a multiple of four (LOUD in the gaps): identical spans, identical statistics bits."""
    r = ragged_run(row, B, level)
    assert all(int(o) % 4 == 0 for o in r["off4"]) and any(int(o) % 4 for o in r["off"])
    for f, n in enumerate(r["lens"]):
        a, b = r["out"][r["off"][f]:r["off"][f] + n], r["out4"][r["off4"][f]:r["off4"][f] + n]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (row, B, level, f)
    assert np.array_equal(r["stats"].view(np.uint64), r["stats4"].view(np.uint64))


# ---------------------------------------------------------------------------------------------- 4: statistics
@pytest.mark.parametrize("level", ["f32", "bf16_all"])
@pytest.mark.parametrize("row,B", RAGGED)
def test_statistics(row, B, level):
    """Per file against float64 numpy over st_predict_long's output of that file (check_stats has the rule).

    Measured on the MI355X (profiles/eval_pool_device.txt has every figure): |e|, e^2, t^2, y_hat^2 and the peak equal the restatement exactly (measured ==
    delta, at most 8.1e-8 relative); log cosh deviates by at most 2.1e-7 relative here, equal to its delta -- the device's expm1f / log1pf differ from numpy's in
    the last place only in the one-file test, 1.3e-8 against a delta of 4.9e-9."""
    r = ragged_run(row, B, level)
    check_stats(f"{row} B={B} {level}", r["stats"], r["ref"], r["ts"], r["geo"], shifted=True)


# ---------------------------------------------------------------------------------------------- 5: forms and guards
def raw_call(eng, B, px, py, off_d, len_d, win_d, rows, kn, stats, out, ws):
    d = eng.dims.with_batch(B)
    d.prec, d.loss_scale, d.clip_all = _lib.PREC[eng.compute_dtype], eng.loss_scale, int(eng.clip_all)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    eng._call("st_eval_pool", C.byref(d), p(eng.params), _lib.PCM_S16 if px.dtype == torch.int16 else _lib.PCM_F32, p(px), p(py), p(off_d), p(len_d), p(win_d),
              int(off_d.numel()), int(rows), int(px.numel()), p(kn), p(stats), p(out), p(ws), eng._stream())


@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_forms_and_guards(fmt):
    """pool_y = NULL gives the out bits of the full form, out = NULL its stats bits; out and stats pre-filled with NaN are fully written and finite; the guard
    zones around out, stats and the pools keep their bits (NaN / full scale around the pools: a read there would show); a second call repeats the bits; and
    int16 pools give what their float32 images give, bit for bit."""
    B, PAD = 3, 64
    eng, geo, P = engine("n256", B)
    lens, xs, ts, kn = make_files(geo)
    if fmt == "s16":
        q = lambda a: np.clip(np.round(a * (32767.0 if np.abs(a).max() > 10 else 20000.0)), -32768, 32767).astype(np.int16)
        xs, ts = [q(a) for a in xs], [q(a) for a in ts]
    off, total = layout(lens)
    nf = len(lens)
    poison = 32767 if fmt == "s16" else float("nan")
    d = eng.dims.with_batch(B)
    ln = np.array(lens, np.int64); win = np.zeros(nf + 1, np.int64)
    LLp = C.POINTER(C.c_longlong)
    rows = int(eng.lib.st_eval_pool_rows(C.byref(d), ln.ctypes.data_as(LLp), nf, win.ctypes.data_as(LLp)))
    off_d, len_d, win_d, kn_d = dev(off), dev(ln), dev(win), dev(kn)
    ws = torch.zeros(int(eng.lib.st_eval_pool_ws_bytes(C.byref(d))), dtype=torch.uint8, device=G.DEV)

    def embed(chunks):
        buf = torch.full((PAD + total + PAD,), poison, dtype=torch.int16 if fmt == "s16" else torch.float32, device=G.DEV)
        buf[PAD:PAD + total] = dev(pool_of(chunks, off, total))
        return buf
    bx, by = embed(xs), embed(ts)
    bx0, by0 = bx.clone(), by.clone()
    px, py = bx[PAD:PAD + total], by[PAD:PAD + total]

    def run(with_y=True, with_out=True):
        ob = torch.full((PAD + total + PAD,), float("nan"), dtype=torch.float32, device=G.DEV)
        sb = torch.full((PAD + nf * 8 + PAD,), float("nan"), dtype=torch.float64, device=G.DEV)
        raw_call(eng, B, px, py if with_y else None, off_d, len_d, win_d, rows, kn_d, sb[PAD:PAD + nf * 8] if with_y else None, ob[PAD:PAD + total] if with_out else None, ws)
        for buf, n in ((ob, total), (sb, nf * 8)):
            assert bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + n:]).all())
        return ob[PAD:PAD + total].clone(), sb[PAD:PAD + nf * 8].clone()
    out, st = run()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(st).all()) and float(out.abs().max()) > 0.05 and float(st.abs().max()) > 1.0
    out_p, st_p = run(with_y=False)
    assert torch.equal(out_p, out) and bool(torch.isnan(st_p).all())
    out_s, st_s = run(with_out=False)
    assert torch.equal(st_s.view(torch.int64), st.view(torch.int64)) and bool(torch.isnan(out_s).all())
    out2, st2 = run()
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)) and torch.equal(st2.view(torch.int64), st.view(torch.int64))
    assert torch.equal(bx.view(torch.int16), bx0.view(torch.int16)) and torch.equal(by.view(torch.int16), by0.view(torch.int16))
    if fmt == "s16":
        img = lambda chunks: dev(pool_of([(a.astype(np.float64) / 32767.0).astype(np.float32) for a in chunks], off, total))
        st_f, out_f = eng.eval_pool(img(xs), img(ts), off, ln, kn_d, want_out=True, batch=B)
        assert torch.equal(out_f.view(torch.int32), out.view(torch.int32)) and torch.equal(st_f.reshape(-1).view(torch.int64), st.view(torch.int64))
        assert float(bx0[PAD:PAD + total].float().abs().max()) >= 32767.0      # the LOUD file sits at full scale beside its neighbours


def test_no_rows_writes_only_zeros():
    """total_rows == 0 (every file too short): ST_OK, every span and every statistics row zero, nothing else touched."""
    eng, geo, P = engine("n256", 3)
    lens = SHORT + [geo["L"] - geo["y"]]
    xs = [signal(n, seed=70 + i) for i, n in enumerate(lens)]
    off, total = layout(lens)
    st, out = eng.eval_pool(dev(pool_of(xs, off, total)), dev(pool_of(xs, off, total)), off, np.array(lens, np.int64), dev(np.zeros((len(lens), K), np.float32)),
                            want_out=True, batch=3)
    assert not bool(out.any()) and not bool(st.any()) and tuple(st.shape) == (len(lens), 8)


# ---------------------------------------------------------------------------------------------- 6: K = 0
def test_model_without_knobs():
    """K = 0, file_knobs = NULL: the spans are st_predict_long's per file (1e-6), the statistics hold their bound."""
    B = 4
    geo = geo_of("n256")
    _, _, _, _, P = G.make_case(1, 1, K=0, geo=geo)
    eng = G.new_engine(G.dims_of(geo, B, 0)); eng.load_state_dict(P)
    L, y = geo["L"], geo["y"]
    lens = [L + y + 5, 18, L + 3 * y + 1, L - y + 1]
    xs = [(0.5 * signal(n, seed=80 + i)).astype(np.float32) for i, n in enumerate(lens)]
    ts = [(0.4 * signal(n, seed=90 + i)).astype(np.float32) for i, n in enumerate(lens)]
    off, total = layout(lens)
    st, out = eng.eval_pool(dev(pool_of(xs, off, total)), dev(pool_of(ts, off, total)), off, np.array(lens, np.int64), None, want_out=True, batch=B)
    ref = per_file_reference(eng, xs, None, B)
    o = out.cpu().numpy()
    for f, (a, n) in enumerate(zip(off, lens)):
        if n > L - y:
            e = float(np.abs(o[a + L - y:a + n].astype(np.float64) - ref[f]).max() / np.abs(ref[f]).max())
            assert e <= 1e-6, (f, e)
    check_stats("K=0", st.cpu().numpy(), ref, ts, geo, shifted=True)


# ---------------------------------------------------------------------------------------------- 7: Python
def _file_model(scale=1):
    from signaltrain_amd import nn_proc
    from oracle import st_oracle as O
    nn_proc._QUIET = True
    P = G.make_case(1, 1, K=3, scale=scale)[4]
    m = nn_proc.st_model(scale_factor=scale, shrink_factor=4, num_knobs=3)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    return m.to(G.DEV), O.geometry(scale, 4)


def _loop_report(ds, m, L, y):
    """The per-file loop evaluate replaces: predict_long(route="device") per file, float64 figures on the host."""
    from signaltrain_amd.predict import predict_long
    kn = ds.feed_tables()["knobs"]
    rep = {k: [] for k in ("n", "logcosh", "mae", "mse", "peak", "esr")}
    outs = []
    for f, (xa, ya) in enumerate(zip(ds.x, ds.y)):
        yh = predict_long(np.asarray(xa, np.float32), kn[f], m, L, y, batch_size=200, route="device")
        s = stats64(yh, np.asarray(ya, np.float32)[L - y:])
        rep["n"].append(yh.size); rep["logcosh"].append(s["logcosh"] / yh.size); rep["mae"].append(s["abs"] / yh.size)
        rep["mse"].append(s["sq"] / yh.size); rep["peak"].append(s["peak"]); rep["esr"].append(s["sq"] / s["t_sq"])
        outs.append(yh)
    return {k: np.array(v) for k, v in rep.items()}, outs


def test_dataset_evaluate_against_the_per_file_loop(tmp_path):
    """AudioFileDataSet.evaluate on a tiny recorded dataset (int16 pools by the feed's format rule, then float32) against the loop of
    predict_long(route="device") per file: predictions within 1e-6 of max|y| (two batch sizes), figures within 2e-5 relative -- the worst case of a float32
    sum of 256 non-negative terms against float64 is 255 * 2^-24 = 1.52e-5, the per-sample float32 terms add a few 2^-24, and the 1e-6 of the predictions moves a
    mean error by less than that times max|y| / mean|e|; the pooled figures are consistent with the per-file ones."""
    from signaltrain_amd import audio, datasets
    from tests.test_device_feed import make_file_dataset
    root = make_file_dataset(str(tmp_path / "la2a"), n_train=3, n_val=1, seconds=0.6)
    m, geo = _file_model()
    L, y = geo["L"], geo["y"]
    ds = datasets.AudioFileDataSet(L, audio.FileEffect(root), path=root + "/Train/", datapoints=16, y_size=y, augment=False)
    assert ds.feed_tables()["pcm"] == "s16"
    ref, outs = _loop_report(ds, m, L, y)
    for pcm in (None, "f32"):
        rep = ds.evaluate(m, pcm=pcm, want_out=True, batch_size=7)
        assert set(rep) == {"n", "logcosh", "mae", "mse", "peak", "esr", "total", "outputs"}
        assert list(rep["n"]) == list(ref["n"]) and rep["total"]["n"] == int(ref["n"].sum())
        for f, o in enumerate(rep["outputs"]):
            assert o.dtype == np.float32 and o.shape == outs[f].shape
            assert np.abs(o.astype(np.float64) - outs[f]).max() <= 1e-6 * np.abs(outs[f]).max()
        for k in ("logcosh", "mae", "mse", "peak", "esr"):
            np.testing.assert_allclose(rep[k], ref[k], rtol=2e-5, err_msg=k)
        n = ref["n"].astype(np.float64)
        np.testing.assert_allclose(rep["total"]["mae"], (ref["mae"] * n).sum() / n.sum(), rtol=2e-5)
        np.testing.assert_allclose(rep["total"]["peak"], ref["peak"].max(), rtol=2e-5)
    assert "outputs" not in ds.evaluate(m)


def test_dataset_evaluate_wide_geometry_warns_once(tmp_path):
    from signaltrain_amd import audio, datasets
    from tests.test_device_feed import make_file_dataset
    if _lib.load().st_eval_pool_supported(C.byref(_lib.geometry(8, 4, 3, 1))):
        pytest.skip("every geometry is supported: there is no fallback to exercise")
    m, geo = _file_model(scale=8)
    L, y = geo["L"], geo["y"]
    root = make_file_dataset(str(tmp_path / "la2a"), n_train=2, n_val=1, seconds=(L + y + 100) / 44100.0)
    ds = datasets.AudioFileDataSet(L, audio.FileEffect(root), path=root + "/Train/", datapoints=4, y_size=y, augment=False)
    datasets._warned_evaluate_unsupported = False
    with pytest.warns(RuntimeWarning, match="file by file"):
        rep = ds.evaluate(m, batch_size=2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rep2 = ds.evaluate(m, batch_size=2, want_out=True)
    assert set(rep) == {"n", "logcosh", "mae", "mse", "peak", "esr", "total"} and set(rep2) == set(rep) | {"outputs"}
    assert list(rep["n"]) == [len(a) - (L - y) for a in ds.x] and np.isfinite(rep["mae"]).all() and rep["total"]["n"] == int(rep["n"].sum())


def test_train_prints_the_file_report(tmp_path, capsys, monkeypatch):
    from signaltrain_amd import audio, nn_proc, train
    from tests.test_device_feed import make_file_dataset
    nn_proc._QUIET = True
    root = make_file_dataset(str(tmp_path / "la2a"), n_train=2, n_val=2, seconds=0.6)
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0); np.random.seed(0)
    train.train(effect=audio.FileEffect(root), epochs=1, n_data_points=40, batch_size=4, device=torch.device("cuda:0"), datapath=root, lr_max=2e-4, file_report=True)
    text = capsys.readouterr().out
    assert "Val set, file by file" in text and "target_0_LA2A_3c" in text and "target_1_LA2A_3c" in text and "\ntotal" in text


# ---------------------------------------------------------------------------------------------- 8: existing behaviour
def test_training_trajectory_is_untouched():
    """A train step before and one after an eval_pool call: the trajectory of the two train steps alone, bit for bit (the call has a workspace of its own and
    only reads the parameters)."""
    geo, P = case("n256")
    _, X, Y, KNB, _ = G.make_case(3, 21, K=K, geo=geo_of("n256"))
    a = G.new_engine(G.dims_of(geo, 3, K)); a.load_state_dict(P)
    b = G.new_engine(G.dims_of(geo, 3, K)); b.load_state_dict(P)
    lens, xs, ts, kn = make_files(geo)
    off, total = layout(lens)
    px, py = dev(pool_of(xs, off, total)), dev(pool_of(ts, off, total))
    for i in range(2):
        a.train_step(G.t(X), G.t(KNB), G.t(Y), 1e-3)
        b.train_step(G.t(X), G.t(KNB), G.t(Y), 1e-3)
        if i == 0:
            gen = a.generation
            a.eval_pool(px, py, off, np.array(lens, np.int64), dev(kn), want_out=True)
            assert a.generation == gen + 1
    for k in ("params", "m", "v", "grads", "scalars"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.step_count == b.step_count == 2
