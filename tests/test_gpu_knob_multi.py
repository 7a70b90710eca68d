"""GPU: many knob settings of one recording from its code -- st_score_knobs_coded / st_fit_knobs_multi_coded, StepEngine.score_knobs / fit_knobs_multi and
predict.search_knobs.

Rows of an internal batch are (setting, window) pairs (st_knob_multi_plan): a recording of at most half a batch is stacked, a longer one runs st_decode_long's
batches with the settings loop inside.  Checked against the float64 reference of tests/knob_multi_ref.py (conditioning asserted on the CPU by
tests/test_knob_multi_host.py), against st_fit_knobs_coded bit for bit where the batches are the same, for chaining, repeatability, formats, knob automation,
the persistent loops' second trip and everything the calls must leave alone.  Shapes, helpers and case tables are those of tests/fit_knobs_ref.py,
tests/decode_ref.py, tests/test_gpu_fit_knobs.py, tests/test_gpu_predict_long.py and tests/test_gpu_decode_long.py, by import."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from signaltrain_amd import _lib
from signaltrain_amd.engine import RecordingCode
from tests import decode_ref as D
from tests import fit_knobs_ref as R
from tests import gpu_checks as G
from tests import knob_multi_ref as M
from tests import test_gpu_decode_long as DL
from tests import test_gpu_fit_knobs as FK
from tests import test_gpu_predict_long as PL
from tests.dims_table import geo_of
from tests.test_gpu_predict_long import LEVELS

pytestmark = pytest.mark.gpu

K = M.K
UNSTACKED = (M.LONG, 4)          # nine windows in batches of four: st_decode_long's batches
STACKED = (M.SHORT, 16)          # three windows, sixteen rows: four starts in one batch of twelve rows
REGIMES = {"unstacked": UNSTACKED, "stacked": STACKED}


def plan_of(eng, n, S, B):
    d = eng.dims.with_batch(B)
    cnt = eng.lib.st_knob_multi_plan(C.byref(d), n, S, None, 0)
    buf = (C.c_int * (4 * cnt))()
    assert eng.lib.st_knob_multi_plan(C.byref(d), n, S, buf, cnt) == cnt
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(cnt)]


def encode(eng, sig, B):
    return eng.encode_long(G.t(sig) if isinstance(sig, np.ndarray) else sig, batch=min(B, 4))


def relmax(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------------------------------------- the score
@pytest.mark.parametrize("hops,B", M.SCORE_BATCHES, ids=["nine_windows_b4", "three_windows_b8", "three_windows_b7"])
@pytest.mark.parametrize("row", M.SCORE_ROWS)
def test_score_against_the_float64_reference(row, hops, B):
    """fp32, the five candidates in one call: each loss[s] within gpu_checks.TOL relative of the reference J, argmin and the full ordering the reference's
    (its J are more than 100 TOL apart), the win_loss rows sum to loss[s] within 1e-6 relative and each share is within TOL of the reference's.  Nine windows at
    B = 4 run st_decode_long's batches; three windows at B = 8 are stacked 2, 2, 1 settings per batch, at B = 7 with an idle row."""
    eng, geo, P = FK.engine(row, B)
    sig, tgt = M.pair(row, hops)
    J, shares = M.scores(row, hops)
    tuples = plan_of(eng, sig.size, M.S, B)
    assert (all(t[3] == 1 for t in tuples) and len(tuples) == 3 * M.S) if hops == M.LONG else [t[3] for t in tuples] == [2, 2, 1]
    code = encode(eng, sig, B)
    loss, win = eng.score_knobs(code, G.t(tgt), G.t(M.SETTINGS), batch=B, per_window=True)
    assert loss.dtype == torch.float64 and tuple(loss.shape) == (M.S,) and win.dtype == torch.float32 and tuple(win.shape) == shares.shape and loss.is_cuda
    got, gw = G.n(loss), G.n(win).astype(np.float64)
    eJ = float((np.abs(got - J) / np.abs(J)).max())
    ew = float((np.abs(gw - shares) / np.abs(shares)).max())
    es = float((np.abs(gw.sum(1) - got) / np.abs(got)).max())
    print(f"score_knobs vs float64 reference [{row or 'default'} hops={hops} B={B}]: J {eJ:.2e}  shares {ew:.2e}  rows-sum {es:.2e}  (tol {G.TOL:.0e})")
    assert eJ <= G.TOL and ew <= G.TOL and es <= 1e-6, (row, hops, B, eJ, ew, es)
    assert int(np.argmin(got)) == int(np.argmin(J)) and np.array_equal(np.argsort(got), np.argsort(J))
    assert torch.equal(eng.score_knobs(code, G.t(tgt), G.t(M.SETTINGS), batch=B), loss)          # without win_loss: the same bits


@pytest.mark.parametrize("level", ["f32", "bf16_all"])
def test_score_equals_the_coded_fits_first_loss_bit_for_bit(level):
    """Not stacked: loss[s] is loss_hist[0] of st_fit_knobs_coded at setting s with lr = 0 -- the same batches, the same formula, the same order."""
    with LEVELS[level]():
        hops, B = UNSTACKED
        eng, geo, P = FK.engine("n256", B)
        sig, tgt = M.pair("n256", hops)
        code = encode(eng, sig, B)
        loss = eng.score_knobs(code, G.t(tgt), G.t(M.SETTINGS), batch=B)
        for s in range(M.S):
            _, lh, _, _ = eng.fit_knobs(code, G.t(tgt), G.t(M.SETTINGS[s]), steps=1, lr=0.0, batch=B)
            assert float(lh[0]) == float(loss[s]) and float(lh[0]) > 0, (level, s, float(lh[0]), float(loss[s]))


# ---------------------------------------------------------------------------------------------- the multi fit
@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("per_window", [False, True], ids=["one_row", "row_per_window"])
@pytest.mark.parametrize("level", ["f32", "bf16_all"])
def test_one_start_equals_the_coded_fit_bit_for_bit(level, per_window, regime):
    """S = 1: knobs, moments, loss history and gradient history of three steps equal st_fit_knobs_coded's bit for bit."""
    with LEVELS[level]():
        hops, B = REGIMES[regime]
        eng, geo, P = FK.engine("n256", B)
        sig, tgt = (G.t(a) for a in M.fit_pair("n256", hops))
        code = encode(eng, sig, B)
        k0 = G.t(FK.knob_rows(hops + 2) if per_window else R.KN)
        kA, lA, gA, (mA, vA, nA) = eng.fit_knobs(code, tgt, k0, steps=3, batch=B, want_grads=True)
        kB, lB, (mB, vB, nB), gB = eng.fit_knobs_multi(code, tgt, k0[None], steps=3, batch=B, want_grads=True)
    assert nA == nB == 4 and tuple(kB.shape) == (1,) + tuple(k0.shape) and tuple(lB.shape) == (3, 1) and tuple(gB.shape) == (3, 1) + tuple(gA.shape[1:])
    assert torch.equal(kB[0].reshape(-1), kA.reshape(-1)) and torch.equal(mB.reshape(-1), mA.reshape(-1)) and torch.equal(vB.reshape(-1), vA.reshape(-1))
    assert torch.equal(lB[:, 0], lA) and torch.equal(gB[:, 0], gA)
    assert not torch.equal(kA.reshape(-1), k0.reshape(-1)) and bool(torch.isfinite(gB).all())


def first_step(eng, code, tgt, starts, B):
    """steps = 1, lr = 0: (J [S], gradient [S, rows, K]) at the starts, the knobs untouched."""
    k, lh, _, g = eng.fit_knobs_multi(code, G.t(tgt) if isinstance(tgt, np.ndarray) else tgt, G.t(starts), steps=1, lr=0.0, batch=B, want_grads=True)
    assert torch.equal(k, G.t(starts))
    return G.n(lh[0]), G.n(g[0])


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("level", ["f32", "bf16_all", "f16_all"])
def test_four_starts_first_gradient_and_loss_against_the_reference(level, regime):
    """S = 4, steps = 1, lr = 0: each start's gradient within TOL_GRAD[level] of max|ref| and its J within gpu_checks.TOL relative of fit_knobs_ref.objective
    (float64) at fp32; the 16-bit levels against the mixed-mode oracle at 6e-2 for both, as tests/test_gpu_fit_knobs.py."""
    hops, B = REGIMES[regime]
    sig, tgt = M.fit_pair("n256", hops)
    if level == "f32":
        eng, geo, P = FK.engine("n256", B)
        J, g = M.gradients("n256", hops, M.STARTS)
        got_J, got_g = first_step(eng, encode(eng, sig, B), tgt, M.STARTS, B)
        tol_J = G.TOL
    else:
        with G.mixed_mode(2, half=level[:-4], loss_scale=0.0, clip_all=False):
            eng, geo, P = FK.engine("n256", B)
            ref = [R.objective(sig, tgt, k, P, geo, dtype=np.float32) for k in M.STARTS]
            J, g = np.array([r[0] for r in ref]), np.stack([r[1].sum(0, keepdims=True) for r in ref])
            got_J, got_g = first_step(eng, encode(eng, sig, B), tgt, M.STARTS, B)
        tol_J = 6e-2
    assert got_g.shape == g.shape == (4, 1, K) and got_J.shape == (4,)
    assert (len(plan_of(eng, sig.size, 4, B)) == 1) == (regime == "stacked")
    for s in range(4):
        eg, eJ = relmax(got_g[s], g[s]), abs(got_J[s] - J[s]) / abs(J[s])
        print(f"fit_knobs_multi vs reference [{level} {regime}] start {s}: grad {eg:.2e} (tol {R.TOL_GRAD[level]:.0e})  J {eJ:.2e} (tol {tol_J:.0e})")
        assert np.all(np.isfinite(got_g[s])) and eg <= R.TOL_GRAD[level] and eJ <= tol_J, (level, regime, s, eg, eJ)


@pytest.mark.parametrize("regime", list(REGIMES))
def test_four_starts_three_steps_against_the_float64_adam_replay(regime):
    """Each start against fit_knobs_ref.adam_replay on its own gradient history within the trajectory bound of tests/test_gpu_decode_long.py (_adam_bound);
    starts that begin at distinct knobs end at distinct knobs, and each start's loss history is its own."""
    hops, B = REGIMES[regime]
    eng, geo, P = FK.engine("n256", B)
    sig, tgt = (G.t(a) for a in M.fit_pair("n256", hops))
    code = encode(eng, sig, B)
    k, lh, (m, v, nxt), g = eng.fit_knobs_multi(code, tgt, G.t(M.STARTS), steps=3, lr=0.05, batch=B, want_grads=True)
    assert nxt == 4 and tuple(k.shape) == (4, K) and tuple(lh.shape) == (3, 4) and tuple(g.shape) == (3, 4, 1, K) and tuple(m.shape) == tuple(v.shape) == (4, K)
    kn, gh = G.n(k), G.n(g)
    for s in range(4):
        want, bound, yard = DL._adam_bound(M.STARTS[s], gh[:, s, 0])
        dev = float(np.abs(kn[s] - want).max())
        print(f"fit_knobs_multi Adam tail [{regime}] start {s}: device {dev:.3e}  torch float32 {yard:.3e}  bound {bound:.3e}")
        assert dev <= bound, (regime, s, dev, yard, bound)
    for i in range(4):
        for j in range(i):
            assert np.abs(kn[i] - kn[j]).max() > 1e-3 and float(lh[0, i]) != float(lh[0, j]), (i, j)
    assert bool((lh > 0).all()) and not torch.equal(k, G.t(M.STARTS))


@pytest.mark.parametrize("level", ["f32", "bf16_all"])
def test_the_starts_are_independent(level):
    """Start s of a stacked S = 4 call against the same start run alone (one batch of three rows): gradient within TOL_GRAD[level] of max|ref|, J within 1e-6
    relative -- the batch-independence bound of tests/test_gpu_decode_long.py.  Bit-equality is printed."""
    with LEVELS[level]():
        hops, B = STACKED
        eng, geo, P = FK.engine("n256", B)
        sig, tgt = M.fit_pair("n256", hops)
        code = encode(eng, sig, B)
        J4, g4 = first_step(eng, code, tgt, M.STARTS, B)
        for s in range(4):
            J1, g1 = first_step(eng, code, tgt, M.STARTS[s:s + 1], B)
            eg, eJ = relmax(g4[s], g1[0].astype(np.float64)), abs(J4[s] - J1[0]) / abs(J1[0])
            print(f"fit_knobs_multi start {s} of four vs alone [{level}]: grad {eg:.2e}  J {eJ:.2e}  bit-equal={np.array_equal(g4[s], g1[0]) and J4[s] == J1[0]}")
            assert eg <= R.TOL_GRAD[level] and eJ <= 1e-6, (level, s, eg, eJ)


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("level", ["f32", "bf16_all"])
def test_chained_single_steps_are_one_call_bit_for_bit(level, regime):
    with LEVELS[level]():
        hops, B = REGIMES[regime]
        eng, geo, P = FK.engine("n256", B)
        sig, tgt = (G.t(a) for a in M.fit_pair("n256", hops))
        code = encode(eng, sig, B)
        k0 = G.t(M.STARTS)
        kA, lA, (mA, vA, nA), gA = eng.fit_knobs_multi(code, tgt, k0, steps=3, batch=B, want_grads=True)
        k, st, ls, gs = k0, None, [], []
        for _ in range(3):
            k, l, st, g = eng.fit_knobs_multi(code, tgt, k, steps=1, batch=B, want_grads=True, state=st)
            ls.append(l); gs.append(g)
    assert nA == st[2] == 4
    assert torch.equal(kA, k) and torch.equal(mA, st[0]) and torch.equal(vA, st[1])
    assert torch.equal(lA, torch.cat(ls)) and torch.equal(gA, torch.cat(gs))
    assert not torch.equal(kA, k0) and float(lA[2, 0]) != float(lA[0, 0])


@pytest.mark.parametrize("B", [4, 7], ids=["unstacked", "stacked_idle_row"])
@pytest.mark.parametrize("level", ["f32", "f16_all"])
def test_repeated_calls_repeat_their_bits_whatever_the_workspace_held(level, B):
    """Two identical calls of the score and of the fit, the workspace filled with NaN bit patterns in between: every element read is written first, every sum
    has a fixed order."""
    with LEVELS[level]():
        hops = M.LONG if B == 4 else M.SHORT
        eng, geo, P = FK.engine("n256", B)
        sig, tgt = (G.t(a) for a in M.pair("n256", hops))
        code = encode(eng, sig, B)
        kn = G.t(M.SETTINGS)
        a = eng.score_knobs(code, tgt, kn, batch=B, per_window=True) + eng.fit_knobs_multi(code, tgt, kn, steps=2, batch=B, want_grads=True)
        eng._multi_ws.view(torch.int32).fill_(0x7fc00001)
        b = eng.score_knobs(code, tgt, kn, batch=B, per_window=True)
        eng._multi_ws.view(torch.int32).fill_(-1)
        b = b + eng.fit_knobs_multi(code, tgt, kn, steps=2, batch=B, want_grads=True)
    flat = lambda r: [t for x in r for t in (x if isinstance(x, tuple) else (x,)) if torch.is_tensor(t)]
    fa, fb = flat(a), flat(b)
    assert len(fa) == len(fb) == 7
    for x, y in zip(fa, fb):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)


def test_int16_pair_equals_its_float32_image_bit_for_bit():
    hops, B = STACKED
    eng, geo, P = FK.engine("n256", B)
    sig, tgt = M.pair("n256", hops)
    s16 = np.round(sig * 20000).astype(np.int16); t16 = np.round(tgt * 20000).astype(np.int16)
    sf = (s16.astype(np.float64) / 32767.0).astype(np.float32); tf = (t16.astype(np.float64) / 32767.0).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).to(G.DEV)
    res = []
    for s, t in ((s16, t16), (sf, tf), (s16, tf)):          # the last: mixed, the int16 one converted on the device
        code = eng.encode_long(dev(s), batch=4)
        assert code.signal.dtype == (torch.int16 if s.dtype == np.int16 else torch.float32)
        sc = eng.score_knobs(code, dev(t), G.t(M.SETTINGS), batch=B, per_window=True)
        ft = eng.fit_knobs_multi(code, dev(t), G.t(M.STARTS), steps=2, batch=B, want_grads=True)
        res.append((sc[0], sc[1], ft[0], ft[1], ft[3]))
    for other in res[1:]:
        for x, y in zip(res[0], other):
            assert torch.equal(x, y)
    assert float(res[0][0].min()) > 0


@pytest.mark.parametrize("regime", list(REGIMES))
def test_knob_automation(regime):
    """[S, nwin, K]: one row per window (decode_ref.AUTOMATION's two alternating settings; their first three rows where the recording has three windows).  The
    score against the reference with the same rows at gpu_checks.TOL, the first-step gradient of every row at TOL_GRAD["f32"] of max|ref| and its J at TOL;
    [S, K], [S, 1, K] and that row repeated over the windows score to equal bits."""
    hops, B = REGIMES[regime]
    nwin = hops + 2
    rows = np.ascontiguousarray(M.AUTOMATION[:, :nwin])
    eng, geo, P = FK.engine("n256", B)
    sig, tgt = M.pair("n256", hops)
    J, shares = M.scores("n256", hops, settings=rows)
    code = encode(eng, sig, B)
    loss, win = eng.score_knobs(code, G.t(tgt), G.t(rows), batch=B, per_window=True)
    eJ, ew = float((np.abs(G.n(loss) - J) / np.abs(J)).max()), float((np.abs(G.n(win) - shares) / np.abs(shares)).max())
    print(f"score_knobs knob automation [{regime}]: J {eJ:.2e} shares {ew:.2e}")
    assert eJ <= G.TOL and ew <= G.TOL, (regime, eJ, ew)
    one = G.n(eng.score_knobs(code, G.t(tgt), G.t(M.SETTINGS[:1]), batch=B))[0]
    assert min(abs(v - one) / one for v in G.n(loss)) > 100 * G.TOL          # the rows were really taken per window
    a = eng.score_knobs(code, G.t(tgt), G.t(M.SETTINGS), batch=B)
    b = eng.score_knobs(code, G.t(tgt), G.t(M.SETTINGS[:, None, :].copy()), batch=B)
    c = eng.score_knobs(code, G.t(tgt), G.t(np.repeat(M.SETTINGS[:, None, :], nwin, axis=1)), batch=B)
    assert torch.equal(a, b) and torch.equal(a, c)
    fsig, ftgt = M.fit_pair("n256", hops)
    fcode = encode(eng, fsig, B)
    Jg, g = M.gradients("n256", hops, rows, per_window=True)
    got_J, got_g = first_step(eng, fcode, ftgt, rows, B)
    assert got_g.shape == g.shape == (2, nwin, K)
    for s in range(2):
        eg, eJ = relmax(got_g[s], g[s]), abs(got_J[s] - Jg[s]) / abs(Jg[s])
        print(f"fit_knobs_multi knob automation [{regime}] setting {s}: grad {eg:.2e} J {eJ:.2e}")
        assert eg <= R.TOL_GRAD["f32"] and eJ <= G.TOL, (regime, s, eg, eJ)
    with pytest.raises(ValueError, match="rows"):
        eng.score_knobs(code, G.t(tgt), G.t(np.repeat(M.SETTINGS[:, None, :], nwin + 1, axis=1)), batch=B)


def test_second_trip_of_the_persistent_loops_in_a_stacked_batch():
    """Default geometry, three windows at 42 seeded settings in ONE stacked batch of 126 rows: more 16-row groups than ae_dec_fwd_kernel's grid x waves
    (decode_ref.second_trip_batch: 125 rows on the MI355X's 256 CUs, which the case is laid out for) and than ae_knob_bwd_kernel's (47 rows), so the prefetch of
    the next group crosses rows and settings.  Every J within gpu_checks.TOL of the reference; the fit's first loss within 1e-6 of the score; the gradients of
    the first, the middle and the last setting against the float64 reference at TOL_GRAD["f32"]."""
    geo, P = R.case(None)
    nb = D.second_trip_batch(torch.cuda.get_device_properties(0).multi_processor_count, geo)
    kn = M.trip_settings()
    S = kn.shape[0]
    B = S * M.TRIP_WINDOWS
    assert B >= nb > FK.second_trip_batch(geo), "the case table is laid out for the MI355X's 256 CUs"
    eng, _, _ = FK.engine(None, B)
    sig, tgt = M.pair(None, M.SHORT)
    assert plan_of(eng, sig.size, S, B) == [(0, M.TRIP_WINDOWS, 0, S)]
    J, _ = M.scores(None, M.SHORT, settings=kn)
    code = encode(eng, sig, B)
    loss = G.n(eng.score_knobs(code, G.t(tgt), G.t(kn), batch=B))
    eJ = float((np.abs(loss - J) / np.abs(J)).max())
    got_J, got_g = first_step(eng, code, tgt, kn, B)
    ef = float((np.abs(got_J - loss) / np.abs(loss)).max())
    print(f"second trip, stacked: rows={B} settings={S} J {eJ:.2e}  fit's first loss vs score {ef:.2e}  bit-equal={np.array_equal(got_J, loss)}")
    assert eJ <= G.TOL and ef <= 1e-6, (eJ, ef)
    for s in (0, S // 2, S - 1):
        _, g, _ = R.objective(sig, tgt, kn[s], P, geo)
        eg = relmax(got_g[s], g.sum(0, keepdims=True))
        print(f"second trip, stacked: setting {s} grad {eg:.2e}")
        assert eg <= R.TOL_GRAD["f32"], (s, eg)


# ---------------------------------------------------------------------------------------------- what the calls must leave alone
def test_everything_else_is_left_alone():
    """The code, the knobs handed in, the engine's parameters, gradients, moments, workspaces and step counter are bit-equal before and after a score and a multi
    fit; nothing is written behind loss + S, win_loss's end, loss_hist's end or grad_hist's end (the C calls themselves, with guard elements)."""
    hops, B = STACKED
    eng, geo, P = FK.engine("n256", B)
    sig, tgt = (G.t(a) for a in M.pair("n256", hops))
    code = encode(eng, sig, B)
    eng.fit_knobs(code, tgt, G.t(R.KN), steps=1, batch=B)          # allocates the single fit's workspace
    eng.grads.normal_(); eng.m.normal_(); eng.v.normal_(); eng.ws.random_(0, 255)
    kn = G.t(M.SETTINGS)
    keep = lambda: (eng.params, eng.grads, eng.m, eng.v, eng.scalars, eng.ws, eng._decode_ws, eng._fit_ws, code.code, code.signal, kn)
    before = [t.clone() for t in keep()]
    gen, step = eng.generation, eng.step_count
    eng.score_knobs(code, tgt, kn, batch=B, per_window=True)
    eng.fit_knobs_multi(code, tgt, kn, steps=2, batch=B, want_grads=True)
    torch.cuda.synchronize()
    for a, b in zip(before, keep()):
        assert torch.equal(a, b)
    assert eng.generation == gen and eng.step_count == step
    lib = _lib.load()
    S, steps, nwin = M.S, 2, hops + 2
    d = eng.dims.with_batch(B)
    loss = torch.full((S + 4,), -7.0, dtype=torch.float64, device=G.DEV)
    win = torch.full((S * nwin + 16,), -7.0, dtype=torch.float32, device=G.DEV)
    rc = lib.st_score_knobs_coded(C.byref(d), _lib.ptr(eng.params), _lib.ptr(code.code), _lib.PCM_F32, C.c_void_p(sig.data_ptr()), C.c_void_p(tgt.data_ptr()),
                                  sig.numel(), _lib.ptr(kn), 1, S, C.c_void_p(loss.data_ptr()), _lib.ptr(win), _lib.ptr(eng._multi_ws), G.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.st_last_error()
    assert bool((loss[S:] == -7.0).all()) and bool((loss[:S] > 0).all()) and bool((win[S * nwin:] == -7.0).all()) and bool((win[:S * nwin] > 0).all())
    k = kn.clone(); m = torch.zeros_like(k); v = torch.zeros_like(k)
    lh = torch.full((steps * S + 4,), -7.0, dtype=torch.float64, device=G.DEV)
    gh = torch.full((steps * S * K + 16,), -7.0, dtype=torch.float32, device=G.DEV)
    rc = lib.st_fit_knobs_multi_coded(C.byref(d), _lib.ptr(eng.params), _lib.ptr(code.code), _lib.PCM_F32, C.c_void_p(sig.data_ptr()), C.c_void_p(tgt.data_ptr()),
                                      sig.numel(), _lib.ptr(k), 1, S, _lib.ptr(m), _lib.ptr(v), 1, steps, 0.05, 0.9, 0.999, 1e-8,
                                      C.c_void_p(lh.data_ptr()), _lib.ptr(gh), _lib.ptr(eng._multi_ws), G.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.st_last_error()
    assert bool((lh[steps * S:] == -7.0).all()) and bool((lh[:steps * S] > 0).all())
    assert bool((gh[steps * S * K:] == -7.0).all()) and bool((gh[:steps * S * K] != -7.0).all())


def test_training_trajectory_is_untouched():
    """A train step before and one after an encode + score + multi fit: the trajectory of the two train steps alone, bit for bit."""
    geo, P = PL.case("n256")
    _, X, Y, KNB, _ = G.make_case(3, 21, K=K, geo=geo_of("n256"))
    a = G.new_engine(G.dims_of(geo, 3, K)); a.load_state_dict(P)
    b = G.new_engine(G.dims_of(geo, 3, K)); b.load_state_dict(P)
    sig, tgt = (G.t(x) for x in M.pair("n256", M.SHORT))
    for i in range(2):
        a.train_step(G.t(X), G.t(KNB), G.t(Y), 1e-3)
        b.train_step(G.t(X), G.t(KNB), G.t(Y), 1e-3)
        if i == 0:
            code = a.encode_long(sig)
            a.score_knobs(code, tgt, G.t(M.SETTINGS), batch=8)
            a.fit_knobs_multi(code, tgt, G.t(M.STARTS), steps=1, batch=16)
    for k in ("params", "m", "v", "grads", "scalars"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.step_count == b.step_count == 2


def test_a_stale_or_foreign_code_raises():
    eng, geo, P = FK.engine("n256", 8)
    other, _, _ = FK.engine("ragged", 8)
    sig, tgt = (G.t(a) for a in M.pair("n256", M.SHORT))
    code = eng.encode_long(sig, batch=4)
    kn = G.t(M.SETTINGS)
    for call in (lambda e, c: e.score_knobs(c, tgt, kn), lambda e, c: e.fit_knobs_multi(c, tgt, kn, steps=1)):
        with pytest.raises(ValueError, match="geometry"):
            call(other, code)
        with pytest.raises(ValueError, match="samples|bytes"):
            call(eng, RecordingCode(code.code[:-16], sig, code.n, code.nwin, code.geometry, code.compute_dtype))
        with pytest.raises(ValueError, match="samples|bytes"):
            call(eng, RecordingCode(code.code, sig[:-4], code.n, code.nwin, code.geometry, code.compute_dtype))
        with pytest.raises(ValueError, match="RecordingCode"):
            call(eng, code.code)
    with pytest.raises(ValueError, match="samples"):
        eng.score_knobs(code, tgt[:-1], kn)
    with G.mixed_mode(2, half="bf16"):
        half, _, _ = FK.engine("n256", 8)
        with pytest.raises(ValueError, match="compute dtype"):
            half.score_knobs(code, tgt, kn)


# ---------------------------------------------------------------------------------------------- the Python route
def test_search_knobs():
    """predict.search_knobs on the conditioned case (the model of test_gpu_predict_long._model(), n = L + 2 y, the five candidates): with lr = 0 the kept
    candidates come back in the float64 reference's order, so the scored best is the candidate the reference ranks first; with real steps the final loss is
    not above that candidate's scored loss; route="batched" names the same best candidate."""
    from signaltrain_amd import predict
    m, _, _ = PL._model()
    geo, P = M.case(M.MODEL)
    L, y = geo["L"], geo["y"]
    sig, tgt = M.pair(M.MODEL, M.SHORT, whole=True)
    J, _ = M.scores(M.MODEL, M.SHORT, whole=True)
    order = np.argsort(J)
    best, best_loss, finals, losses = predict.search_knobs(sig, tgt, m, L, y, M.SETTINGS, keep=3, steps=1, lr=0.0)
    assert best.shape == (K,) and best.dtype == np.float32 and finals.shape == (3, K) and losses.shape == (3,)
    assert np.array_equal(finals, M.SETTINGS[order[:3]]) and np.array_equal(best, M.SETTINGS[order[0]])
    eJ = float((np.abs(losses - J[order[:3]]) / J[order[:3]]).max())
    print(f"search_knobs scored losses vs float64 reference: {eJ:.2e}")
    assert eJ <= G.TOL and best_loss == losses[0]
    best2, best_loss2, finals2, losses2 = predict.search_knobs(sig, tgt, m, L, y, M.SETTINGS, keep=2, steps=5, lr=0.05)
    print(f"search_knobs: scored best {losses[0]:.6e} -> after 5 steps {best_loss2:.6e}; finals {finals2.tolist()} true knobs {M.KNOBS_TRUE.tolist()}")
    eng = m.engine(torch.empty((), dtype=torch.float32, device=G.DEV).expand(3, L))
    scored = G.n(eng.score_knobs(eng.encode_long(G.t(sig), batch=3), G.t(tgt), G.t(M.SETTINGS), batch=200))          # the call search_knobs scores with
    assert finals2.shape == (2, K) and np.all(np.abs(finals2) <= 0.5) and best_loss2 == losses2.min()
    assert best_loss2 <= scored[order[0]] and np.all(losses2 <= scored[order[:2]])
    bb, bl, bf, bls = predict.search_knobs(sig, tgt, m, L, y, M.SETTINGS, keep=1, steps=1, lr=0.0, route="batched", batch_size=3)
    print(f"search_knobs route='batched': best loss {bl:.6e} (device {losses[0]:.6e})")
    assert np.array_equal(bb, best) and bf.shape == (1, K)


def test_search_knobs_on_a_wide_model_warns_once_and_returns():
    from signaltrain_amd import predict
    m, geo = DL._wide_model()
    L, y = geo["L"], geo["y"]
    sig = PL.signal(L + y, seed=12)
    tgt = R.target_of(sig)
    predict._warned_search_unsupported = False
    with pytest.warns(RuntimeWarning, match="batched route"):
        a = predict.search_knobs(sig, tgt, m, L, y, M.SETTINGS[:2], keep=1, steps=1, batch_size=2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b = predict.search_knobs(sig, tgt, m, L, y, M.SETTINGS[:2], keep=1, steps=1, batch_size=2)          # the second time: no warning
    c = predict.search_knobs(sig, tgt, m, L, y, M.SETTINGS[:2], keep=1, steps=1, batch_size=2, route="batched")
    assert a[0].shape == (K,) and np.isfinite(a[1]) and np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0]) and a[1] == c[1]
