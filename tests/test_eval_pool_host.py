"""CPU: the host side of st_eval_pool (include/signaltrain_hip.h) -- a folder of recordings through the model in one device call: the row rule of
st_eval_pool_rows against its statement, the size function, the geometries it admits, every refusal (before any launch: runs without a GPU) and the Python
signatures and defaults."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from signaltrain_amd import _lib
from tests.test_predict_long_host import FUSED_ROWS, WIDE_ROWS, dims, lengths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL = C.POINTER(C.c_longlong)


def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "signaltrain_hip.h")).read()
    lib = _lib.load()
    for name, decl in (("st_eval_pool_supported", "st_eval_pool_supported(const st_dims* d);"),
                       ("st_eval_pool_rows", "long long st_eval_pool_rows(const st_dims* d, const long long* file_len_host, int nfiles, long long* win_off_host"),
                       ("st_eval_pool_ws_bytes", "st_eval_pool_ws_bytes(const st_dims* d);"),
                       ("st_eval_pool", "int st_eval_pool(const st_dims* d, const float* params, int fmt, const void* pool_x, const void* pool_y")):
        assert decl in hdr, name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert "enum { ST_POOL_STATS = 8 };" in hdr and _lib.POOL_STATS == 8 and len(_lib.POOL_FIELDS) == 8
    res, args = _lib.SIGNATURES["st_eval_pool"]
    assert res is C.c_int and len(args) == 16 and args[8] is C.c_int and args[9] is C.c_longlong and args[10] is C.c_longlong
    assert _lib.SIGNATURES["st_eval_pool_rows"][0] is C.c_longlong and _lib.SIGNATURES["st_eval_pool_ws_bytes"][0] is C.c_size_t


def rows_of(lib, d, lens, want_table=True):
    ln = np.asarray(lens, np.int64)
    win = np.full(ln.size + 1, -7, np.int64)
    total = int(lib.st_eval_pool_rows(C.byref(d), ln.ctypes.data_as(LL), int(ln.size), win.ctypes.data_as(LL) if want_table else None))
    return total, win


@pytest.mark.parametrize("row", [None, "n256", "h256", "ragged", "tiny"])
def test_rows_follow_the_rule(row):
    """A file of len samples has st_predict_windows(d, len) rows if len > L - y and none otherwise; the table holds the prefix sums, whatever the order."""
    lib = _lib.load()
    d = dims(row)
    L, y = d.L, d.y
    base = lengths(L, y)
    assert base == [1, L - y, L - y + 1, L - 1, L, L + 1, L + y - 1, L + y, L + 3 * y + 777 % y]
    rng = np.random.default_rng(11)
    for lens in (base, base[::-1], list(rng.permutation(base)), list(rng.permutation(base + [3, 17, 40])), [L - y], [L + 1]):
        want = [(1 if n < L else -(-(n - L) // y) + 1) if n > L - y else 0 for n in lens]
        for n, w in zip(lens, want):
            assert w == (int(lib.st_predict_windows(C.byref(d), int(n))) if n > L - y else 0)
            assert (w == 0) == (int(lib.st_predict_out_samples(C.byref(d), int(n))) == 0)
            assert w == -(-max(n - (L - y), 0) // y)                 # one row per started hop of output samples
        total, win = rows_of(lib, d, lens)
        assert total == sum(want) and list(win) == list(np.concatenate([[0], np.cumsum(want)]))
        assert rows_of(lib, d, lens, want_table=False)[0] == total


def test_rows_of_bad_arguments_are_zero():
    lib = _lib.load()
    d = dims("n256")
    ln = np.array([d.L + 5], np.int64)
    assert lib.st_eval_pool_rows(C.byref(d), None, 1, None) == 0
    assert lib.st_eval_pool_rows(C.byref(d), ln.ctypes.data_as(LL), 0, None) == 0
    bad = dims("n256"); bad.y += 4
    assert lib.st_eval_pool_rows(C.byref(bad), ln.ctypes.data_as(LL), 1, None) == 0


@pytest.mark.parametrize("row,B", [(None, 5), ("n256", 5), ("h256", 3), ("tiny", 2)])
def test_size_function(row, B):
    lib = _lib.load()
    for prec in range(6):
        d = dims(row, B=B, prec=prec)
        need, base = int(lib.st_eval_pool_ws_bytes(C.byref(d))), int(lib.st_predict_ws_bytes(C.byref(d)))
        assert need >= base + 6 * B * ((d.y + 255) // 256) * 4 > 0 and need % 16 == 0


def bad_dims(lib):
    out = []
    d = dims("n256"); d.B = 0; out.append((d, b"dimension"))
    d = dims("n256"); d.y += 4; out.append((d, b"y must equal"))
    d = dims("n256"); d.prec = 9; out.append((d, b"prec"))
    for d in [dims(r) for r in WIDE_ROWS] + [_lib.geometry(8, 4, 4, 2)]:
        if not lib.st_predict_supported(C.byref(d)):
            out.append((d, b"st_eval_pool_supported"))
    assert len(out) > 3
    return out


def test_size_is_zero_for_bad_and_wide_dims():
    lib = _lib.load()
    for d, _ in bad_dims(lib):
        assert lib.st_eval_pool_ws_bytes(C.byref(d)) == 0


def test_supported_is_predict_supported_over_the_dims_table():
    lib = _lib.load()
    seen = set()
    for r in FUSED_ROWS + WIDE_ROWS + [None]:
        for K in (0, 4):
            d = dims(r, K=K)
            a, b = int(lib.st_eval_pool_supported(C.byref(d))), int(lib.st_predict_supported(C.byref(d)))
            assert a == b, r
            seen.add(a)
    for d, _ in bad_dims(lib):
        assert int(lib.st_eval_pool_supported(C.byref(d))) == int(lib.st_predict_supported(C.byref(d))) == 0
    assert seen == {0, 1}


def _call(lib, d, fmt=0, nfiles=3, total_rows=5, pool_samples=1 << 20, params=0x1000, pool_x=0x1000, pool_y=0x1000, file_off=0x1000, file_len=0x1000,
          win_off=0x1000, file_knobs=0x1000, stats=0x1000, out=0x1000, ws=0x1000):
    """st_eval_pool with dummy pointers (never dereferenced on the host; a refused call launches nothing)."""
    p = lambda v: C.c_void_p(v) if v else None
    rc = lib.st_eval_pool(C.byref(d), p(params), fmt, p(pool_x), p(pool_y), p(file_off), p(file_len), p(win_off), nfiles, total_rows, pool_samples,
                          p(file_knobs), p(stats), p(out), p(ws), None)
    return rc, lib.st_last_error()


def test_the_last_check_of_the_dummy_call_is_the_alignment():
    """The dummy call passes every rule up to the alignment ones: each refusal test below moves exactly one argument."""
    lib = _lib.load()
    rc, msg = _call(lib, dims("n256"), ws=0x1004)
    assert rc == -1 and b"st_eval_pool: ws must be 16-byte aligned" in msg


@pytest.mark.parametrize("missing", ["params", "pool_x", "file_off", "file_len", "win_off", "file_knobs", "ws"])
def test_refuses_a_null_pointer_by_name(missing):
    lib = _lib.load()
    rc, msg = _call(lib, dims("n256"), **{missing: 0})
    assert rc == -1 and b"st_eval_pool" in msg and b"null" in msg and missing.encode() in msg, msg


def test_null_pointers_that_are_allowed():
    lib = _lib.load()
    d0 = dims("n256", K=0)
    rc, msg = _call(lib, d0, file_knobs=0, ws=0x1004)                       # K = 0: null knobs pass, the next refusal is another rule's
    assert rc == -1 and b"ws must be 16-byte aligned" in msg
    d = dims("n256")
    rc, msg = _call(lib, d, pool_y=0, stats=0, ws=0x1004)                   # predict only
    assert rc == -1 and b"ws must be 16-byte aligned" in msg
    rc, msg = _call(lib, d, out=0, ws=0x1004)                               # score only
    assert rc == -1 and b"ws must be 16-byte aligned" in msg
    rc, msg = _call(lib, d, total_rows=0, ws=0x1004)                        # no rows is no error
    assert rc == -1 and b"ws must be 16-byte aligned" in msg


def test_refuses_stats_without_target_and_nothing_to_compute():
    lib = _lib.load()
    d = dims("n256")
    rc, msg = _call(lib, d, pool_y=0)
    assert rc == -1 and b"st_eval_pool: stats and pool_y come together" in msg
    rc, msg = _call(lib, d, stats=0)
    assert rc == -1 and b"st_eval_pool: stats and pool_y come together" in msg
    rc, msg = _call(lib, d, pool_y=0, stats=0, out=0)
    assert rc == -1 and b"out and stats are both null" in msg


def test_refuses_bad_formats_and_counts():
    lib = _lib.load()
    d = dims("n256")
    for fmt in (-1, 2, 7):
        rc, msg = _call(lib, d, fmt=fmt)
        assert rc == -1 and b"st_eval_pool: fmt" in msg
    for nf in (0, -3):
        rc, msg = _call(lib, d, nfiles=nf)
        assert rc == -1 and b"st_eval_pool: nfiles" in msg
    rc, msg = _call(lib, d, total_rows=-1)
    assert rc == -1 and b"st_eval_pool: total_rows" in msg
    for ps in (0, -5):
        rc, msg = _call(lib, d, pool_samples=ps)
        assert rc == -1 and b"st_eval_pool: pool_samples" in msg


def test_refuses_misaligned_pointers():
    lib = _lib.load()
    d = dims("n256")
    for off in (4, 8, 12):
        for name in ("pool_x", "pool_y", "out", "stats", "ws"):
            rc, msg = _call(lib, d, **{name: 0x1000 + off})
            assert rc == -1 and f"st_eval_pool: {name} must be 16-byte aligned".encode() in msg, (name, off)
    for off in (2, 4, 6):
        for name in ("pool_x", "pool_y"):
            rc, msg = _call(lib, d, fmt=_lib.PCM_S16, **{name: 0x1000 + off})
            assert rc == -1 and f"st_eval_pool: {name} must be 8-byte aligned".encode() in msg, (name, off)
    rc, msg = _call(lib, d, fmt=_lib.PCM_S16, pool_x=0x1008, pool_y=0x1008, ws=0x1004)      # int16 pools on an 8-byte boundary are taken
    assert rc == -1 and b"ws must be" in msg


def test_refuses_bad_and_unsupported_dims_and_batches_beyond_the_offsets():
    lib = _lib.load()
    for d, word in bad_dims(lib):
        rc, msg = _call(lib, d)
        assert rc == -1 and word in msg, msg
    d = dims("n256", B=1 << 22)                                            # B * (L + 2 N) leaves 2^30 elements
    rc, msg = _call(lib, d, total_rows=1 << 23)
    assert rc == -1 and b"32-bit element offsets" in msg


def test_python_signatures_and_defaults():
    from signaltrain_amd import datasets, train
    from signaltrain_amd.engine import StepEngine
    sig = inspect.signature(StepEngine.eval_pool)
    assert list(sig.parameters) == ["self", "pool_x", "pool_y", "off", "length", "knobs", "want_out", "batch"]
    assert sig.parameters["want_out"].default is False and sig.parameters["batch"].default is None
    assert callable(StepEngine.eval_pool_supported)
    sig = inspect.signature(datasets.AudioFileDataSet.evaluate)
    assert list(sig.parameters) == ["self", "model", "device", "pcm", "want_out", "batch_size"]
    assert [sig.parameters[k].default for k in ("device", "pcm", "want_out", "batch_size")] == [None, None, False, 200]
    assert inspect.signature(train.train).parameters["file_report"].default is False
    with pytest.raises(ValueError, match="file_report"):
        train.train(file_report=True, epochs=1, n_data_points=40, batch_size=20)


def test_report_dict_from_sums():
    """The dict AudioFileDataSet.evaluate returns, from known sums: means over n, the peak as it is, esr = sum e^2 / sum t^2, "total" pooled over all samples."""
    from signaltrain_amd import datasets
    st = np.array([[4, 2.0, 1.0, 0.5, 0.3, 8.0, 7.0, 0], [0, 0, 0, 0, 0, 0, 0, 0], [6, 3.0, 6.0, 1.5, 0.9, 2.0, 3.0, 0]], np.float64)
    rep = datasets._file_report(st)
    assert list(rep["n"]) == [4, 0, 6] and rep["n"].dtype == np.int64
    np.testing.assert_allclose(rep["logcosh"], [0.5, 0.0, 0.5]); np.testing.assert_allclose(rep["mae"], [0.25, 0.0, 1.0])
    np.testing.assert_allclose(rep["mse"], [0.125, 0.0, 0.25]); np.testing.assert_allclose(rep["peak"], [0.3, 0.0, 0.9])
    np.testing.assert_allclose(rep["esr"][[0, 2]], [0.0625, 0.75])
    tot = rep["total"]
    assert tot["n"] == 10 and tot["peak"] == 0.9
    np.testing.assert_allclose([tot["logcosh"], tot["mae"], tot["mse"], tot["esr"]], [0.5, 0.7, 0.2, 0.2])
    assert "outputs" not in rep and "total" in datasets.format_file_report(rep)


def test_run_train_has_the_file_report_flag():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_train.py"), "--file-report", "--target", "nope"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "invalid target type" in (r.stdout + r.stderr)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_train.py"), "--file-report"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--effect files" in (r.stdout + r.stderr)
