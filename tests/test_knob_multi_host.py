"""CPU: the host side of the multi-setting routes (st_knob_multi_plan, st_knob_multi_ws_bytes, st_score_knobs_coded, st_fit_knobs_multi_coded;
include/signaltrain_hip.h) -- the symbols, the plan's invariants, the workspace size, every refusal (before any launch: runs without a GPU), the Python
signatures, and the conditioning of every case the GPU file ranks or compares at fp32 tolerance (tests/knob_multi_ref.py)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from signaltrain_amd import _lib
from tests import fit_knobs_ref as R
from tests import gpu_checks as G
from tests import knob_multi_ref as M
from tests.dims_table import ROWS
from tests.test_fit_knobs_host import FUSED_ROWS, WIDE_ROWS, dims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "signaltrain_hip.h")).read()
    lib = _lib.load()
    for name, decl in (("st_knob_multi_plan", "st_knob_multi_plan(const st_dims* d, long long n, int n_settings, int* out, int cap);"),
                       ("st_knob_multi_ws_bytes", "st_knob_multi_ws_bytes(const st_dims* d, int n_settings);"),
                       ("st_score_knobs_coded", "st_score_knobs_coded(const st_dims* d, const float* params, const void* code, int fmt, const void* signal, const void* target, long long n,"),
                       ("st_fit_knobs_multi_coded", "st_fit_knobs_multi_coded(const st_dims* d, const float* params, const void* code, int fmt, const void* signal, const void* target, long long n,")):
        assert decl in hdr, name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["st_knob_multi_plan"]
    assert res is C.c_int and len(args) == 5 and args[1] is C.c_longlong and args[2] is C.c_int and args[4] is C.c_int
    assert _lib.SIGNATURES["st_knob_multi_ws_bytes"] == (C.c_size_t, [C.POINTER(_lib.st_dims), C.c_int])
    res, args = _lib.SIGNATURES["st_score_knobs_coded"]
    assert res is C.c_int and len(args) == 14 and args[6] is C.c_longlong and args[8] is C.c_longlong and args[9] is C.c_int
    res, args = _lib.SIGNATURES["st_fit_knobs_multi_coded"]
    coded = _lib.SIGNATURES["st_fit_knobs_coded"][1]
    assert res is C.c_int and len(args) == 22 and args[:9] == coded[:9] and args[9] is C.c_int and args[10:] == coded[9:]      # st_fit_knobs_coded with n_settings behind knob_rows


# ---------------------------------------------------------------------------------------------- the plan
def plan(lib, d, n, S, cap=None):
    cnt = lib.st_knob_multi_plan(C.byref(d), n, S, None, 0)
    cap = cnt if cap is None else cap
    buf = (C.c_int * (4 * max(cap, 1)))(*([-7] * (4 * max(cap, 1))))
    got = lib.st_knob_multi_plan(C.byref(d), n, S, buf, cap)
    return cnt, got, [tuple(buf[4 * i:4 * i + 4]) for i in range(min(cap, got))], list(buf)


def length_of(d, nwin):
    """A recording of nwin windows that is no whole number of hops (one window: shorter than the window)."""
    return d.L - 5 if nwin == 1 else d.L + (nwin - 2) * d.y + 777 % d.y


@pytest.mark.parametrize("row", [r for r in list(ROWS) + [None]])
def test_plan_invariants(row):
    """Over every dims-table row st_predict_supported admits, nwin in {1, 3, 9}, B in {4, 7, 8, 16} and S in {1, 4, 5}: every (setting, window) pair exactly
    once, the windows of a setting ascending, nw * ns <= B, st_decode_long's batches where 2 * nwin > B, the whole recording B / nwin times otherwise."""
    lib = _lib.load()
    if not lib.st_predict_supported(C.byref(dims(row))):
        assert lib.st_knob_multi_plan(C.byref(dims(row)), 10 ** 6, 4, None, 0) == 0          # the wide geometries: no plan
        return
    for B in (4, 7, 8, 16):
        d = dims(row, B=B)
        for nwin in (1, 3, 9):
            n = length_of(d, nwin)
            assert int(lib.st_predict_windows(C.byref(d), n)) == nwin
            for S in (1, 4, 5):
                cnt, got, tuples, _ = plan(lib, d, n, S)
                assert cnt == got == len(tuples) > 0
                seen, last = set(), {}
                for w0, nw, s0, ns in tuples:
                    assert nw >= 1 and ns >= 1 and nw * ns <= B and 0 <= w0 and w0 + nw <= nwin and 0 <= s0 and s0 + ns <= S, (row, B, nwin, S, tuples)
                    for s in range(s0, s0 + ns):
                        assert last.get(s, -1) < w0, (row, B, nwin, S, tuples)          # ascending windows for any one setting
                        last[s] = w0 + nw - 1
                        for w in range(w0, w0 + nw):
                            assert (s, w) not in seen
                            seen.add((s, w))
                assert len(seen) == S * nwin
                if 2 * nwin > B:          # st_decode_long's batches, the settings loop inside the window batch
                    want = [(w0, min(B, nwin - w0), s, 1) for w0 in range(0, nwin, B) for s in range(S)]
                else:
                    per = B // nwin
                    want = [(0, nwin, s0, min(per, S - s0)) for s0 in range(0, S, per)]
                assert tuples == want, (row, B, nwin, S, tuples, want)


def test_plan_stacked_batches_are_ragged_and_leave_idle_rows():
    lib = _lib.load()
    d = dims("n256", B=8)
    n = length_of(d, 3)
    assert [t[3] for t in plan(lib, d, n, 5)[2]] == [2, 2, 1]          # S = 5, B = 8, three windows: 2, 2, 1 settings
    d7 = dims("n256", B=7)
    t7 = plan(lib, d7, n, 5)[2]
    assert [t[3] for t in t7] == [2, 2, 1] and all(t[1] * t[3] < 7 for t in t7)          # B = 7: six rows, one idle
    assert plan(lib, dims("n256", B=6), n, 5)[2] == [(0, 3, 0, 2), (0, 3, 2, 2), (0, 3, 4, 1)]      # exactly half a batch: stacked
    assert plan(lib, dims("n256", B=5), n, 2)[2] == [(0, 3, 0, 1), (0, 3, 1, 1)]                    # more than half: not stacked
    assert plan(lib, dims("n256", B=16), length_of(d, 1), 40)[2] == [(0, 1, 0, 16), (0, 1, 16, 16), (0, 1, 32, 8)]


def test_plan_count_is_honest_when_cap_is_too_small():
    lib = _lib.load()
    d = dims("n256", B=4)
    n = length_of(d, 9)
    cnt, _, full, _ = plan(lib, d, n, 5)
    assert cnt == 15
    for cap in (0, 1, 7):
        c2, got, part, raw = plan(lib, d, n, 5, cap=cap)
        assert c2 == got == 15 and part == full[:cap]
        assert all(v == -7 for v in raw[4 * cap:])          # nothing behind cap is written


def test_plan_is_zero_for_bad_wide_empty_or_no_setting():
    lib = _lib.load()
    good = dims("n256")
    n = 3 * good.L
    assert lib.st_knob_multi_plan(C.byref(good), n, 2, None, 0) > 0
    for bad_n in (0, -1, -10 ** 12):
        assert lib.st_knob_multi_plan(C.byref(good), bad_n, 2, None, 0) == 0
    for S in (0, -1, -100):
        assert lib.st_knob_multi_plan(C.byref(good), n, S, None, 0) == 0
    d = dims("n256"); d.B = 0
    assert lib.st_knob_multi_plan(C.byref(d), n, 2, None, 0) == 0
    d = dims("n256"); d.y += 4
    assert lib.st_knob_multi_plan(C.byref(d), n, 2, None, 0) == 0
    d = dims("n256"); d.prec = 7
    assert lib.st_knob_multi_plan(C.byref(d), n, 2, None, 0) == 0
    n_wide = 0
    for d in [dims(r) for r in WIDE_ROWS] + [_lib.geometry(8, 4, 4, 2)]:
        if not lib.st_predict_supported(C.byref(d)):
            n_wide += 1
            assert lib.st_knob_multi_plan(C.byref(d), 3 * d.L, 2, None, 0) == 0 and lib.st_knob_multi_ws_bytes(C.byref(d), 2) == 0
    assert n_wide > 0


@pytest.mark.parametrize("row,B", [(None, 5), ("n256", 5), ("h256", 3), ("tiny", 2)])
def test_workspace_holds_the_fit_workspace_and_grows_with_the_settings(row, B):
    lib = _lib.load()
    for prec in range(6):
        d = dims(row, B=B, prec=prec)
        fit = int(lib.st_fit_knobs_ws_bytes(C.byref(d)))
        prev = 0
        for S in (1, 2, 4, 5, 64, 256, 1000):
            need = int(lib.st_knob_multi_ws_bytes(C.byref(d), S))
            assert fit > 0 and need >= fit + 4 * S * d.K and need >= prev and need % 16 == 0, (row, prec, S, need, fit)
            prev = need
        for S in (0, -1):
            assert lib.st_knob_multi_ws_bytes(C.byref(d), S) == 0
    assert lib.st_knob_multi_ws_bytes(C.byref(dims(row, B=B, K=0)), 4) == 0          # no knobs: nothing to score or fit


# ---------------------------------------------------------------------------------------------- refusals, by name, with dummy pointers
_p = lambda v: C.c_void_p(v) if v else None
SCORE_PTRS = ("params", "code", "signal", "target", "knobs", "loss", "win_loss", "ws")
FIT_PTRS = ("params", "code", "signal", "target", "knobs", "adam_m", "adam_v", "loss_hist", "grad_hist", "ws")
SCORE, FIT = b"st_score_knobs_coded", b"st_fit_knobs_multi_coded"


def _score(lib, d, n=None, fmt=0, knob_rows=1, n_settings=3, **ptrs):
    q = {k: 0x1000 for k in SCORE_PTRS}; q.update(ptrs)
    return lib.st_score_knobs_coded(C.byref(d), _p(q["params"]), _p(q["code"]), fmt, _p(q["signal"]), _p(q["target"]), 3 * d.L if n is None else n, _p(q["knobs"]),
                                    knob_rows, n_settings, _p(q["loss"]), _p(q["win_loss"]), _p(q["ws"]), None)


def _fit(lib, d, n=None, fmt=0, knob_rows=1, n_settings=3, first_step=1, steps=2, lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8, **ptrs):
    q = {k: 0x1000 for k in FIT_PTRS}; q.update(ptrs)
    return lib.st_fit_knobs_multi_coded(C.byref(d), _p(q["params"]), _p(q["code"]), fmt, _p(q["signal"]), _p(q["target"]), 3 * d.L if n is None else n,
                                        _p(q["knobs"]), knob_rows, n_settings, _p(q["adam_m"]), _p(q["adam_v"]), first_step, steps, lr, beta1, beta2, eps,
                                        _p(q["loss_hist"]), _p(q["grad_hist"]), _p(q["ws"]), None)


CALLS = ((_score, SCORE), (_fit, FIT))


def _refused(lib, rc, entry, *words):
    msg = lib.st_last_error()
    return rc == -1 and entry in msg and all(w in msg for w in words)


@pytest.mark.parametrize("missing", [p for p in SCORE_PTRS if p != "win_loss"])
def test_score_refuses_a_null_pointer_by_name(missing):
    lib = _lib.load()
    assert _refused(lib, _score(lib, dims("n256"), **{missing: 0}), SCORE, b"null", missing.encode()), lib.st_last_error()
    assert _score(lib, dims("n256"), win_loss=0, n=1) == 0          # win_loss may be NULL; no output sample: ST_OK without a launch


@pytest.mark.parametrize("missing", [p for p in FIT_PTRS if p != "grad_hist"])
def test_multi_fit_refuses_a_null_pointer_by_name(missing):
    lib = _lib.load()
    assert _refused(lib, _fit(lib, dims("n256"), **{missing: 0}), FIT, b"null", missing.encode()), lib.st_last_error()
    assert _fit(lib, dims("n256"), grad_hist=0, n=1) == 0          # grad_hist may be NULL; no output sample: ST_OK without a launch


def test_refuses_bad_lengths_formats_rows_settings_and_steps():
    lib = _lib.load()
    d = dims("n256")
    for call, entry in CALLS:
        for n in (0, -1):
            assert _refused(lib, call(lib, d, n=n), entry, b"n must be positive")
        for fmt in (-1, 2, 7):
            assert _refused(lib, call(lib, d, fmt=fmt), entry, b"fmt")
        n = d.L + 3 * d.y + 5
        nwin = int(lib.st_predict_windows(C.byref(d), n))
        assert nwin == 5
        for rows in (0, 2, nwin - 1, nwin + 1, -1):          # the rule and the wording of st_predict_long
            assert _refused(lib, call(lib, d, n=n, knob_rows=rows), entry, b"knob_rows", b"must be 1 or the window count (5 windows for n = "), rows
        for rows in (1, nwin):                               # the two accepted row counts pass this check: the next refusal is another rule's
            assert _refused(lib, call(lib, d, n=n, knob_rows=rows, ws=0x1004), entry, b"aligned"), rows
        for s in (0, -1, -100):
            assert _refused(lib, call(lib, d, n_settings=s), entry, b"n_settings"), s
        assert _refused(lib, call(lib, dims("n256", K=0)), entry, b"K = 0")
        assert call(lib, dims("n256", K=3), n=d.L - d.y) == 0          # K = 3: taken (only base pointers need alignment)
    assert _refused(lib, _fit(lib, d, steps=0), FIT, b"steps")
    assert _refused(lib, _fit(lib, d, steps=-3), FIT, b"steps")
    assert _refused(lib, _fit(lib, d, first_step=0), FIT, b"first_step")


def test_multi_fit_refuses_bad_hyper_parameters():
    lib = _lib.load()
    d = dims("n256")
    nan, inf = float("nan"), float("inf")
    for lr in (-0.1, nan, inf):
        assert _refused(lib, _fit(lib, d, lr=lr), FIT, b"lr"), lr
    for b in (-0.1, 1.0, 1.5, nan):
        assert _refused(lib, _fit(lib, d, beta1=b), FIT, b"beta1"), b
        assert _refused(lib, _fit(lib, d, beta2=b), FIT, b"beta2"), b
    for e in (0.0, -1e-8, nan, inf):
        assert _refused(lib, _fit(lib, d, eps=e), FIT, b"eps"), e
    assert _fit(lib, d, lr=0.0, n=1) == 0          # lr = 0 is a legal probe of the loss and the gradient


def test_refuses_misaligned_buffers():
    lib = _lib.load()
    d = dims("n256")
    for off in (4, 8, 12):
        for name in ("code", "knobs", "ws", "signal", "target"):
            for call, entry in CALLS:
                assert _refused(lib, call(lib, d, **{name: 0x1000 + off}), entry, name.encode() + b" must be 16-byte aligned"), (name, off)
        for name in ("adam_m", "adam_v"):
            assert _refused(lib, _fit(lib, d, **{name: 0x1000 + off}), FIT, name.encode() + b" must be 16-byte aligned"), (name, off)
    for off in (2, 4, 6):
        for name in ("signal", "target"):
            for call, entry in CALLS:
                assert _refused(lib, call(lib, d, fmt=_lib.PCM_S16, **{name: 0x1000 + off}), entry, name.encode() + b" must be 8-byte aligned")
    for call, _ in CALLS:          # an int16 pair on an 8-byte boundary is taken; an n without an output sample then ends the call without a launch
        assert call(lib, d, fmt=_lib.PCM_S16, signal=0x1008, target=0x1008, n=d.L - d.y) == 0


def test_refuses_bad_and_wide_dims():
    lib = _lib.load()
    for call, entry in CALLS:
        d = dims("n256"); d.B = 0
        assert _refused(lib, call(lib, d), entry, b"dimension")
        d = dims("n256"); d.y += 4
        assert _refused(lib, call(lib, d), entry, b"y must equal")
        d = dims("n256"); d.prec = 9
        assert _refused(lib, call(lib, d), entry, b"prec")
        n_wide = 0
        for d in [dims(r) for r in WIDE_ROWS] + [_lib.geometry(8, 4, 4, 2)]:
            if not lib.st_decode_supported(C.byref(d)):
                n_wide += 1
                assert _refused(lib, call(lib, d), entry, b"wide autoencoder geometries", b"_supported")
        assert n_wide > 0


def test_python_signatures_and_defaults():
    from signaltrain_amd import predict
    from signaltrain_amd.engine import StepEngine
    s = inspect.signature(predict.search_knobs).parameters
    assert list(s) == ["signal", "target", "model", "chunk_size", "out_chunk_size", "candidates", "keep", "steps", "lr", "batch_size", "compand", "route"]
    assert (s["keep"].default, s["steps"].default, s["lr"].default, s["batch_size"].default, s["compand"].default, s["route"].default) == \
           (8, 50, 0.05, 200, False, "device")
    with pytest.raises(ValueError, match="route"):
        predict.search_knobs(np.zeros(16, np.float32), np.zeros(16, np.float32), None, 8192, 2048, np.zeros((2, 4), np.float32), route="graph")
    with pytest.raises(ValueError, match="candidates"):
        predict.search_knobs(np.zeros(16, np.float32), np.zeros(16, np.float32), None, 8192, 2048, np.zeros(4, np.float32))
    p = inspect.signature(StepEngine.score_knobs).parameters
    assert list(p)[1:] == ["code", "target", "knobs", "batch", "per_window"] and p["batch"].default is None and p["per_window"].default is False
    f = inspect.signature(StepEngine.fit_knobs_multi).parameters
    assert list(f)[1:] == ["code", "target", "knobs", "steps", "lr", "betas", "eps", "batch", "state", "want_grads"]
    one = inspect.signature(StepEngine.fit_knobs).parameters
    for k in ("steps", "lr", "betas", "eps", "batch", "state", "want_grads"):
        assert f[k].default == one[k].default, k
    # the defaults of the existing routes do not change
    p = inspect.signature(predict.fit_knobs).parameters
    assert (p["steps"].default, p["lr"].default, p["init"].default, p["batch_size"].default, p["compand"].default, p["grad_history"].default, p["route"].default,
            p["encode_once"].default) == (50, 0.05, None, 200, False, None, "batched", False)
    s = inspect.signature(predict.predict_sweep).parameters
    assert list(s)[:5] == ["signal", "knob_settings", "model", "chunk_size", "out_chunk_size"]
    assert (s["sr"].default, s["effect"].default, s["device"].default, s["compand"].default, s["batch_size"].default, s["verbose"].default, s["route"].default) == \
           (44100, None, None, False, 200, False, "device")


# ---------------------------------------------------------------------------------------------- conditioning of the GPU cases
def regime(row, hops, S, B, whole=False):
    """The settings per batch st_knob_multi_plan gives the case: the GPU file's cases are laid out for these."""
    d = dims(None if row == M.MODEL else row, B=B)
    n = d.L + (hops + 1) * d.y if whole else R.length(M.case(row)[0], hops)
    return [t[3] for t in plan(_lib.load(), d, n, S)[2]]


@pytest.mark.parametrize("hops", [M.LONG, M.SHORT], ids=["nine_windows", "three_windows"])
@pytest.mark.parametrize("row", M.SCORE_ROWS + [M.MODEL])
def test_score_cases_are_well_conditioned(row, hops):
    """Every case the GPU file ranks: in float64 AND in float32 the candidates' J differ pairwise by more than 100 gpu_checks.TOL relative, the two orderings
    are the same, and the float32 oracle's J and per-window shares agree with the float64 oracle's to TOL / 4.  The signal seed is the first of 3, 4, 5, ...
    (five at most) at which all of that holds (the rule of tests/dims_table.py)."""
    def qualifies(seed):
        J64, w64 = M.scores(row, hops, seed=seed)
        J32, w32 = M.scores(row, hops, dtype=np.float32, seed=seed)
        eJ = float(np.abs(J32 - J64).max() / np.abs(J64).min())
        ew = float((np.abs(w32 - w64) / np.abs(w64)).max())
        sep = min(M.separation(J64), M.separation(J32))
        print(f"score case [{row or 'default'} hops={hops} seed={seed}]: J={np.array2string(J64, precision=6)} separation {sep:.2e} (> {100 * G.TOL:.0e})  "
              f"f32 vs f64: J {eJ:.2e} shares {ew:.2e} (<= {G.TOL / 4:.1e})")
        return sep > 100 * G.TOL and eJ <= G.TOL / 4 and ew <= G.TOL / 4 and np.array_equal(np.argsort(J64), np.argsort(J32))
    first = next((s for s in range(3, 8) if qualifies(s)), None)
    assert first == M.seed_of(row, hops), (row, hops, first)
    J64, w64 = M.scores(row, hops)
    assert J64.shape == (M.S,) and w64.shape == (M.S, hops + 2) and np.allclose(w64.sum(1), J64, rtol=1e-12)
    for h, B in M.SCORE_BATCHES:          # nine windows at B = 4: not stacked; three windows at B = 8 and B = 7: 2, 2, 1 settings per batch
        if h == hops:
            assert regime(row, hops, M.S, B) == ([1] * (3 * M.S) if hops == M.LONG else [2, 2, 1]), (row, hops, B)


@pytest.mark.parametrize("hops", [M.LONG, M.SHORT], ids=["nine_windows", "three_windows"])
def test_fit_cases_are_well_conditioned(hops):
    """The four starts of the multi fit at n256: the float32 oracle's gradient (window sum and per window) and J agree with the float64 oracle's to a quarter of
    the fp32 tolerances (fit_knobs_ref's own pair: knob_multi_ref.fit_pair)."""
    J64, g64 = M.gradients("n256", hops, M.STARTS, per_window=True)
    J32, g32 = M.gradients("n256", hops, M.STARTS, dtype=np.float32, per_window=True)
    for s in range(M.STARTS.shape[0]):
        e_sum = np.abs(g32[s].sum(0) - g64[s].sum(0)).max() / np.abs(g64[s].sum(0)).max()
        e_win = np.abs(g32[s] - g64[s]).max() / np.abs(g64[s]).max()
        e_J = abs(J32[s] - J64[s]) / abs(J64[s])
        print(f"multi fit case [n256 hops={hops}] start {s}: J={J64[s]:.6e} f32 vs f64: grad sum {e_sum:.2e} per window {e_win:.2e} J {e_J:.2e}")
        assert e_sum <= R.TOL_GRAD["f32"] / 4 and e_win <= R.TOL_GRAD["f32"] / 4 and e_J <= G.TOL / 4, (s, e_sum, e_win, e_J)
    assert regime("n256", hops, 4, 4 if hops == M.LONG else 16) == ([1] * 12 if hops == M.LONG else [4])          # the GPU file's two regimes


@pytest.mark.parametrize("hops", [M.LONG, M.SHORT], ids=["nine_windows", "three_windows"])
def test_automation_cases_are_well_conditioned(hops):
    """One knob row per window (decode_ref.AUTOMATION, its first rows at three windows): score and first-step gradient."""
    rows = np.ascontiguousarray(M.AUTOMATION[:, :hops + 2])
    J64, w64 = M.scores("n256", hops, settings=rows)
    J32, w32 = M.scores("n256", hops, settings=rows, dtype=np.float32)
    one = M.scores("n256", hops)[0][0]
    assert np.abs(J32 - J64).max() / np.abs(J64).min() <= G.TOL / 4 and (np.abs(w32 - w64) / np.abs(w64)).max() <= G.TOL / 4
    assert M.separation(np.append(J64, one)) > 100 * G.TOL          # the rows are really taken per window: neither J equals the one-row J at KN
    _, g64 = M.gradients("n256", hops, rows, per_window=True)
    _, g32 = M.gradients("n256", hops, rows, dtype=np.float32, per_window=True)
    for s in range(2):
        assert np.abs(g32[s] - g64[s]).max() <= R.TOL_GRAD["f32"] / 4 * np.abs(g64[s]).max(), s
    assert regime("n256", hops, 2, 4 if hops == M.LONG else 16) == ([1] * 6 if hops == M.LONG else [2])


def test_the_search_case_is_well_conditioned():
    """The Python route's case: the model of test_gpu_predict_long._model(), n = L + 2 y (three windows; the batched route's objective coincides with the
    device's), the five candidates."""
    J64, _ = M.scores(M.MODEL, M.SHORT, whole=True)
    J32, _ = M.scores(M.MODEL, M.SHORT, dtype=np.float32, whole=True)
    sep = min(M.separation(J64), M.separation(J32))
    print(f"search case: J={np.array2string(J64, precision=6)} separation {sep:.2e}")
    assert sep > 100 * G.TOL and np.abs(J32 - J64).max() / np.abs(J64).min() <= G.TOL / 4 and np.array_equal(np.argsort(J64), np.argsort(J32))
    sig, _ = M.pair(M.MODEL, M.SHORT, whole=True)
    geo = M.case(M.MODEL)[0]
    assert sig.size == geo["L"] + 2 * geo["y"]
    assert regime(M.MODEL, M.SHORT, M.S, 200, whole=True) == [M.S]          # search_knobs' default batch: all candidates in one stacked batch


def test_the_second_trip_case_is_well_conditioned_and_fills_the_mi355x_batch():
    from tests import decode_ref as D
    kn = M.trip_settings()
    nb = D.second_trip_batch(D.MI355X_CUS, R.geo_for(None))
    assert nb == 125 and kn.shape == (42, M.K) and 42 * M.TRIP_WINDOWS >= nb > 41 * M.TRIP_WINDOWS and np.abs(kn).max() < 0.45
    J64, w64 = M.scores(None, M.SHORT, settings=kn)
    J32, w32 = M.scores(None, M.SHORT, settings=kn, dtype=np.float32)
    e = float(np.abs(J32 - J64).max() / np.abs(J64).min())
    print(f"second-trip case: 42 settings x 3 windows, f32 vs f64 J {e:.2e}")
    assert e <= G.TOL / 4 and (np.abs(w32 - w64) / np.abs(w64)).max() <= G.TOL / 4
    assert regime(None, M.SHORT, 42, 126) == [42]          # one stacked batch of 126 rows
