"""CPU: the host side of whole-signal inference on the device (st_predict_long, include/signaltrain_hip.h) -- the window and length rules against the
reference's (audio.sliding_window, utils/predict_long.py:72-79), the workspace size, every refusal (before any launch: runs without a GPU), the geometries
st_predict_supported admits, and the route switch of predict.predict_long."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from oracle import host_audio
from signaltrain_amd import _lib
from tests.dims_table import ROWS, geo_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED_ROWS = [r for r, (N, H, L, T, OT) in ROWS.items() if T <= 32 and OT <= 16]
WIDE_ROWS = [r for r in ROWS if r not in FUSED_ROWS]


def dims(row=None, B=3, K=4, prec=0):
    """st_dims of a table row (None: the default geometry, L = 8192, y = 2048)."""
    if row is None:
        return _lib.geometry(1, 4, K, B).with_arith(prec=prec)
    g = geo_of(row)
    d = _lib.st_dims()
    d.B, d.L, d.N, d.H, d.T, d.OT, d.F, d.K, d.y = B, g["L"], g["N"], g["H"], g["T"], g["OT"], g["F"], K, g["y"]
    d.prec = prec
    return d


def lengths(L, y):
    """The signal lengths every length-sensitive test of this feature uses."""
    return [1, L - y, L - y + 1, L - 1, L, L + 1, L + y - 1, L + y, L + 3 * y + 777 % y]


def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "signaltrain_hip.h")).read()
    lib = _lib.load()
    for name, decl in (("st_predict_windows", "long long st_predict_windows(const st_dims* d, long long n);"),
                       ("st_predict_out_samples", "long long st_predict_out_samples(const st_dims* d, long long n);"),
                       ("st_predict_supported", "st_predict_supported(const st_dims* d);"),
                       ("st_predict_ws_bytes", "st_predict_ws_bytes(const st_dims* d);"),
                       ("st_predict_long", "int st_predict_long(const st_dims* d, const float* params, int fmt, const void* signal, long long n,")):
        assert decl in hdr, name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["st_predict_long"]
    assert res is C.c_int and len(args) == 10 and args[4] is C.c_longlong and args[6] is C.c_longlong
    assert _lib.SIGNATURES["st_predict_windows"][0] is C.c_longlong and _lib.SIGNATURES["st_predict_ws_bytes"][0] is C.c_size_t


@pytest.mark.parametrize("row", [None, "n256", "h256", "ragged", "tiny"])
def test_window_and_length_rules_are_the_references(row):
    """n >= L: the window count is audio.sliding_window's with overlap L - y and every window is signal[w y, w y + L) with zeros behind the end; n < L: one
    window (the rule predict._windows restates: the reference's sliding_window has no answer below one window).  The output length is the reference's
    nwin * y - (L + (nwin - 1) y - n) = n - (L - y) (predict_long.py:72-79), and 0 where that is not positive."""
    lib = _lib.load()
    d = dims(row)
    L, y = d.L, d.y
    for n in lengths(L, y):
        nwin = int(lib.st_predict_windows(C.byref(d), n))
        n_out = int(lib.st_predict_out_samples(C.byref(d), n))
        if n >= L:
            xw = host_audio.sliding_window(np.arange(1, n + 1, dtype=np.float32), L, overlap=L - y)
            assert nwin == xw.shape[0], (row, n)
            for w in (0, nwin - 1):
                want = np.zeros(L, np.float32); m = min(L, n - w * y); want[:m] = np.arange(w * y + 1, w * y + m + 1)
                assert np.array_equal(xw[w], want), (row, n, w)
        else:
            assert nwin == 1, (row, n)
        unique = L + (nwin - 1) * y
        assert n_out == max(nwin * y - max(unique - n, 0), 0) == max(n - (L - y), 0), (row, n)
        assert (nwin - 1) * y < max(n_out, 1) <= nwin * y           # every window holds an output sample, and none is missing
    assert lib.st_predict_windows(C.byref(d), 0) == 0 and lib.st_predict_windows(C.byref(d), -5) == 0
    assert lib.st_predict_out_samples(C.byref(d), 0) == 0
    bad = dims(row); bad.F -= 1
    assert lib.st_predict_windows(C.byref(bad), L) == 0 and lib.st_predict_out_samples(C.byref(bad), 2 * L) == 0


@pytest.mark.parametrize("row,B", [(None, 5), ("n256", 5), ("n384", 4), ("h256", 3), ("tiny", 2)])
def test_workspace_covers_every_batch_at_every_level(row, B):
    lib = _lib.load()
    for prec in range(6):
        d = dims(row, B=B, prec=prec)
        need = int(lib.st_predict_ws_bytes(C.byref(d)))
        per_batch = [int(lib.st_workspace_bytes(C.byref(d.with_batch(b)))) for b in range(1, B + 1)]
        assert min(per_batch) > 0 and need >= max(per_batch), (row, prec, need, per_batch)
        # ... with room for the part that is built once per call: at least both orientations of the folded synthesis bases
        assert need - max(per_batch) >= 2 * lib.st_kp(d.F) * d.N * 2, (row, prec)
        # the part built once lies in front and does not depend on the batch: a smaller batch never needs a larger workspace
        assert int(lib.st_predict_ws_bytes(C.byref(d.with_batch(1)))) <= need


def test_workspace_is_zero_for_bad_or_unsupported_dims():
    lib = _lib.load()
    d = dims("n256"); d.B = 0
    assert lib.st_predict_ws_bytes(C.byref(d)) == 0
    d = dims("n256"); d.y += 4
    assert lib.st_predict_ws_bytes(C.byref(d)) == 0
    d = dims("n256"); d.prec = 7
    assert lib.st_predict_ws_bytes(C.byref(d)) == 0
    for row in WIDE_ROWS:
        if not lib.st_predict_supported(C.byref(dims(row))):
            assert lib.st_predict_ws_bytes(C.byref(dims(row))) == 0, row


@pytest.mark.parametrize("prec", range(6))
def test_supported_geometries(prec):
    """Every fused-autoencoder geometry (T <= 32 and OT <= 16) at every level; the wide ones either way, but then consistently with the size function."""
    lib = _lib.load()
    assert lib.st_predict_supported(C.byref(dims(None, prec=prec))) == 1
    for row in FUSED_ROWS:
        assert lib.st_predict_supported(C.byref(dims(row, prec=prec))) == 1, row
    for row in WIDE_ROWS:
        s = lib.st_predict_supported(C.byref(dims(row, prec=prec)))
        assert s in (0, 1) and (lib.st_predict_ws_bytes(C.byref(dims(row, prec=prec))) > 0) == bool(s), row
    wide = _lib.geometry(8, 4, 4, 2).with_arith(prec=prec)                # the 65536-sample window
    assert (lib.st_predict_ws_bytes(C.byref(wide)) > 0) == bool(lib.st_predict_supported(C.byref(wide)))
    bad = dims("n256", prec=prec); bad.OT = bad.T + 1
    assert lib.st_predict_supported(C.byref(bad)) == 0


def _call(lib, d, n=None, fmt=0, knob_rows=1, params=0x1000, signal=0x1000, knobs=0x1000, out=0x1000, ws=0x1000):
    """st_predict_long with dummy pointers (never dereferenced on the host; a refused call launches nothing)."""
    p = lambda v: C.c_void_p(v) if v else None
    n = 3 * d.L if n is None else n
    return lib.st_predict_long(C.byref(d), p(params), fmt, p(signal), n, p(knobs), knob_rows, p(out), p(ws), None)


@pytest.mark.parametrize("missing", ["params", "signal", "knobs", "out", "ws"])
def test_refuses_a_null_pointer_by_name(missing):
    lib = _lib.load()
    rc = _call(lib, dims("n256"), **{missing: 0})
    msg = lib.st_last_error()
    assert rc == -1 and b"st_predict_long" in msg and b"null" in msg and missing.encode() in msg, msg


def test_knobs_may_be_null_only_without_knobs():
    lib = _lib.load()
    d0 = dims("n256", K=0)
    rc = _call(lib, d0, knobs=0, out=0)              # K = 0: the null knobs pass, the next check (out) refuses -- still no launch
    assert rc == -1 and b"out" in lib.st_last_error() and b"knobs" not in lib.st_last_error()


def test_refuses_bad_lengths_formats_and_knob_rows():
    lib = _lib.load()
    d = dims("n256")
    for n in (0, -1):
        assert _call(lib, d, n=n) == -1 and b"n must be positive" in lib.st_last_error()
    for fmt in (-1, 2, 7):
        assert _call(lib, d, fmt=fmt) == -1 and b"fmt" in lib.st_last_error()
    n = d.L + 3 * d.y + 5
    nwin = int(lib.st_predict_windows(C.byref(d), n))
    assert nwin == 5
    for rows in (0, 2, nwin - 1, nwin + 1, -1):
        assert _call(lib, d, n=n, knob_rows=rows) == -1 and b"knob_rows" in lib.st_last_error(), rows
    # the two accepted row counts pass this check: the next refusal is another rule's
    for rows in (1, nwin):
        assert _call(lib, d, n=n, knob_rows=rows, out=0x1004) == -1 and b"aligned" in lib.st_last_error(), rows


def test_refuses_misaligned_signal_and_output():
    lib = _lib.load()
    d = dims("n256")
    for off in (4, 8, 12):
        assert _call(lib, d, signal=0x1000 + off) == -1 and b"signal must be 16-byte aligned" in lib.st_last_error(), off
        assert _call(lib, d, out=0x1000 + off) == -1 and b"out must be 16-byte aligned" in lib.st_last_error(), off
    for off in (2, 4, 6):
        assert _call(lib, d, fmt=_lib.PCM_S16, signal=0x1000 + off) == -1 and b"signal must be 8-byte aligned" in lib.st_last_error(), off
    # an int16 signal on an 8-byte boundary is taken; an n without an output sample then ends the call without a launch
    assert _call(lib, d, fmt=_lib.PCM_S16, signal=0x1008, n=d.L - d.y) == 0
    assert _call(lib, d, n=1) == 0


def test_refuses_bad_and_unsupported_dims():
    lib = _lib.load()
    d = dims("n256"); d.B = 0
    assert _call(lib, d) == -1 and b"dimension" in lib.st_last_error()
    d = dims("n256"); d.y += 4
    assert _call(lib, d) == -1 and b"y must equal" in lib.st_last_error()
    d = dims("n256"); d.prec = 9
    assert _call(lib, d) == -1 and b"prec" in lib.st_last_error()
    for d in [dims(r) for r in WIDE_ROWS] + [_lib.geometry(8, 4, 4, 2)]:
        if not lib.st_predict_supported(C.byref(d)):
            assert _call(lib, d) == -1 and b"st_predict_supported" in lib.st_last_error()


def test_predict_long_route_switch():
    from signaltrain_amd import predict
    from signaltrain_amd.engine import StepEngine
    p = inspect.signature(predict.predict_long).parameters
    assert p["route"].default == "batched" and predict.ROUTES == ("batched", "device")      # no existing caller changes
    with pytest.raises(ValueError, match="route"):
        predict.predict_long(np.zeros(16, np.float32), np.zeros(4, np.float32), None, 8192, 2048, route="graph")
    q = inspect.signature(StepEngine.predict_long).parameters
    assert list(q)[1:] == ["signal", "knobs", "out", "batch"] and q["out"].default is None and q["batch"].default is None
