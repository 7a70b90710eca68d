"""CPU: the host side of the coded routes (st_code_bytes, st_encode_long, st_decode_long, st_fit_knobs_coded; include/signaltrain_hip.h) -- the symbols, the
size of the code through its public contract (the layout stays opaque), every refusal (before any launch: runs without a GPU), the Python switches, and the
conditioning of every case the GPU file compares at fp32 tolerance (tests/decode_ref.py)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from signaltrain_amd import _lib
from tests import decode_ref as D
from tests import gpu_checks as G
from tests.dims_table import ROWS
from tests.test_fit_knobs_host import FUSED_ROWS, WIDE_ROWS, dims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "signaltrain_hip.h")).read()
    lib = _lib.load()
    for name, decl in (("st_decode_supported", "st_decode_supported(const st_dims* d);"),
                       ("st_decode_ws_bytes", "st_decode_ws_bytes(const st_dims* d);"),
                       ("st_code_bytes", "st_code_bytes(const st_dims* d, long long n);"),
                       ("st_encode_long", "st_encode_long(const st_dims* d, const float* params, int fmt, const void* signal, long long n, void* code, void* ws, void* stream);"),
                       ("st_decode_long", "st_decode_long(const st_dims* d, const float* params, const void* code, int fmt, const void* signal, long long n,"),
                       ("st_fit_knobs_coded", "st_fit_knobs_coded(const st_dims* d, const float* params, const void* code, int fmt, const void* signal, const void* target, long long n,")):
        assert decl in hdr, name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert "const float* knobs, long long knob_rows, int n_settings, float* out, long long out_pitch, void* ws, void* stream);" in hdr
    res, args = _lib.SIGNATURES["st_decode_long"]
    assert res is C.c_int and len(args) == 13 and args[5] is C.c_longlong and args[7] is C.c_longlong and args[8] is C.c_int and args[10] is C.c_longlong
    res, args = _lib.SIGNATURES["st_fit_knobs_coded"]
    fit = _lib.SIGNATURES["st_fit_knobs"][1]
    assert res is C.c_int and len(args) == 21 and args[:2] == fit[:2] and args[3:] == fit[2:]          # st_fit_knobs with the code after params
    assert _lib.SIGNATURES["st_code_bytes"] == (C.c_size_t, [C.POINTER(_lib.st_dims), C.c_longlong])
    assert len(_lib.SIGNATURES["st_encode_long"][1]) == 8


@pytest.mark.parametrize("prec", range(6))
def test_supported_is_predict_supported(prec):
    lib = _lib.load()
    cases = [dims(row, prec=prec, K=K) for row in ROWS for K in (0, 4)] + [dims(None, prec=prec)] + [_lib.geometry(8, 4, 4, 2).with_arith(prec=prec)]
    for d in cases:
        want = int(lib.st_predict_supported(C.byref(d)))
        assert lib.st_decode_supported(C.byref(d)) == want, (d.N, d.T, d.OT, prec)
        assert int(lib.st_decode_ws_bytes(C.byref(d))) == (int(lib.st_predict_ws_bytes(C.byref(d))) if want else 0)
    assert any(lib.st_decode_supported(C.byref(d)) for d in cases) and not all(lib.st_decode_supported(C.byref(d)) for d in cases)


@pytest.mark.parametrize("row", FUSED_ROWS + [None])
def test_code_bytes_is_the_documented_formula_whatever_the_batch(row):
    """st_code_bytes(d, n) = st_predict_windows(d, n) * (st_kp(F) / 2) * (32 + 2 OT) * sizeof(float), the formula the header documents; the same for every
    d->B (window-major: a code built at one batch size decodes at another) and for every arithmetic level."""
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "signaltrain_hip.h")).read()
    assert "st_code_bytes(d, n) = st_predict_windows(d, n) * (st_kp(d->F) / 2) * (32 + 2 * d->OT) * sizeof(float)" in hdr
    d = dims(row)
    for n in (1, d.L - d.y, d.L, d.L + 1, d.L + 7 * d.y + 5, 10 ** 7):
        nwin = int(lib.st_predict_windows(C.byref(d), n))
        want = nwin * (int(lib.st_kp(d.F)) // 2) * (32 + 2 * d.OT) * 4
        assert want > 0 and want % 64 == 0
        for B in (1, 2, 3, 16, 257):
            for prec in range(6):
                assert int(lib.st_code_bytes(C.byref(dims(row, B=B, prec=prec)), n)) == want, (row, n, B, prec)


def test_code_bytes_is_zero_for_bad_wide_or_empty():
    lib = _lib.load()
    good = dims("n256")
    assert lib.st_code_bytes(C.byref(good), good.L) > 0
    for n in (0, -1, -10 ** 12):
        assert lib.st_code_bytes(C.byref(good), n) == 0
    d = dims("n256"); d.B = 0
    assert lib.st_code_bytes(C.byref(d), d.L) == 0
    d = dims("n256"); d.y += 4
    assert lib.st_code_bytes(C.byref(d), d.L) == 0
    d = dims("n256"); d.prec = 7
    assert lib.st_code_bytes(C.byref(d), d.L) == 0
    n_wide = 0
    for d in [dims(r) for r in WIDE_ROWS] + [_lib.geometry(8, 4, 4, 2)]:
        if not lib.st_predict_supported(C.byref(d)):
            n_wide += 1
            assert lib.st_code_bytes(C.byref(d), 3 * d.L) == 0 and lib.st_decode_ws_bytes(C.byref(d)) == 0 and lib.st_decode_supported(C.byref(d)) == 0
    assert n_wide > 0


# ---------------------------------------------------------------------------------------------- refusals, by name, with dummy pointers
_p = lambda v: C.c_void_p(v) if v else None


def _decode(lib, d, n=None, fmt=0, knob_rows=1, n_settings=2, out_pitch=None, **ptrs):
    q = {k: 0x1000 for k in ("params", "code", "signal", "knobs", "out", "ws")}; q.update(ptrs)
    n = 3 * d.L if n is None else n
    n_out = max(n - (d.L - d.y), 0)
    pitch = (n_out + 3) // 4 * 4 if out_pitch is None else out_pitch
    return lib.st_decode_long(C.byref(d), _p(q["params"]), _p(q["code"]), fmt, _p(q["signal"]), n, _p(q["knobs"]), knob_rows, n_settings, _p(q["out"]), pitch,
                              _p(q["ws"]), None)


def _encode(lib, d, n=None, fmt=0, **ptrs):
    q = {k: 0x1000 for k in ("params", "code", "signal", "ws")}; q.update(ptrs)
    return lib.st_encode_long(C.byref(d), _p(q["params"]), fmt, _p(q["signal"]), 3 * d.L if n is None else n, _p(q["code"]), _p(q["ws"]), None)


FIT_PTRS = ("params", "code", "signal", "target", "knobs", "adam_m", "adam_v", "loss_hist", "grad_hist", "ws")


def _fit(lib, d, n=None, fmt=0, knob_rows=1, first_step=1, steps=2, lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8, **ptrs):
    q = {k: 0x1000 for k in FIT_PTRS}; q.update(ptrs)
    return lib.st_fit_knobs_coded(C.byref(d), _p(q["params"]), _p(q["code"]), fmt, _p(q["signal"]), _p(q["target"]), 3 * d.L if n is None else n, _p(q["knobs"]),
                                  knob_rows, _p(q["adam_m"]), _p(q["adam_v"]), first_step, steps, lr, beta1, beta2, eps, _p(q["loss_hist"]), _p(q["grad_hist"]),
                                  _p(q["ws"]), None)


def _refused(lib, rc, entry, *words):
    msg = lib.st_last_error()
    return rc == -1 and entry in msg and all(w in msg for w in words)


@pytest.mark.parametrize("missing", ["params", "code", "signal", "knobs", "out", "ws"])
def test_decode_refuses_a_null_pointer_by_name(missing):
    lib = _lib.load()
    assert _refused(lib, _decode(lib, dims("n256"), **{missing: 0}), b"st_decode_long", b"null", missing.encode()), lib.st_last_error()


@pytest.mark.parametrize("missing", ["params", "code", "signal", "ws"])
def test_encode_refuses_a_null_pointer_by_name(missing):
    lib = _lib.load()
    assert _refused(lib, _encode(lib, dims("n256"), **{missing: 0}), b"st_encode_long", b"null", missing.encode()), lib.st_last_error()


@pytest.mark.parametrize("missing", [p for p in FIT_PTRS if p != "grad_hist"])
def test_coded_fit_refuses_a_null_pointer_by_name(missing):
    lib = _lib.load()
    assert _refused(lib, _fit(lib, dims("n256"), **{missing: 0}), b"st_fit_knobs_coded", b"null", missing.encode()), lib.st_last_error()
    assert _fit(lib, dims("n256"), grad_hist=0, n=1) == 0          # grad_hist may be NULL; no output sample: ST_OK without a launch


def test_knobs_may_be_null_without_knobs():
    lib = _lib.load()
    d = dims("n256", K=0)
    assert _decode(lib, d, knobs=0, n=d.L - d.y) == 0
    assert _refused(lib, _decode(lib, d, knobs=0, ws=0x1004), b"st_decode_long", b"ws must be 16-byte aligned")


def test_refuses_bad_lengths_formats_rows_settings_and_pitches():
    lib = _lib.load()
    d = dims("n256")
    for n in (0, -1):
        assert _refused(lib, _decode(lib, d, n=n, out_pitch=4), b"st_decode_long", b"n must be positive")
        assert _refused(lib, _encode(lib, d, n=n), b"st_encode_long", b"n must be positive")
        assert _refused(lib, _fit(lib, d, n=n), b"st_fit_knobs_coded", b"n must be positive")
    for fmt in (-1, 2, 7):
        assert _refused(lib, _decode(lib, d, fmt=fmt), b"st_decode_long", b"fmt")
        assert _refused(lib, _encode(lib, d, fmt=fmt), b"st_encode_long", b"fmt")
        assert _refused(lib, _fit(lib, d, fmt=fmt), b"st_fit_knobs_coded", b"fmt")
    n = d.L + 3 * d.y + 5
    nwin = int(lib.st_predict_windows(C.byref(d), n))
    assert nwin == 5
    for rows in (0, 2, nwin - 1, nwin + 1, -1):          # the rule and the wording of st_predict_long
        assert _refused(lib, _decode(lib, d, n=n, knob_rows=rows), b"st_decode_long", b"knob_rows", b"must be 1 or the window count (5 windows for n = "), rows
        assert _refused(lib, _fit(lib, d, n=n, knob_rows=rows), b"st_fit_knobs_coded", b"knob_rows"), rows
    for rows in (1, nwin):                               # the two accepted row counts pass this check: the next refusal is another rule's
        assert _refused(lib, _decode(lib, d, n=n, knob_rows=rows, ws=0x1004), b"st_decode_long", b"aligned"), rows
    for s in (0, -1, -100):
        assert _refused(lib, _decode(lib, d, n_settings=s), b"st_decode_long", b"n_settings"), s
    n_out = n - (d.L - d.y)
    assert n_out % 4 != 0
    for pitch in (0, n_out - 1, n_out, n_out + 1, n_out + 2, (n_out + 3) // 4 * 4 - 4, -4):          # too small, or no multiple of 4
        assert _refused(lib, _decode(lib, d, n=n, out_pitch=pitch), b"st_decode_long", b"out_pitch"), pitch
    for pitch in ((n_out + 3) // 4 * 4, (n_out + 3) // 4 * 4 + 64):                                  # taken: the next refusal is another rule's
        assert _refused(lib, _decode(lib, d, n=n, out_pitch=pitch, out=0x1004), b"st_decode_long", b"out must be 16-byte aligned"), pitch
    assert _refused(lib, _fit(lib, d, steps=0), b"st_fit_knobs_coded", b"steps")
    assert _refused(lib, _fit(lib, dims("n256", K=0)), b"st_fit_knobs_coded", b"K = 0")


def test_refuses_misaligned_buffers():
    lib = _lib.load()
    d = dims("n256")
    for off in (4, 8, 12):
        assert _refused(lib, _decode(lib, d, signal=0x1000 + off), b"st_decode_long", b"signal must be 16-byte aligned")
        assert _refused(lib, _encode(lib, d, signal=0x1000 + off), b"st_encode_long", b"signal must be 16-byte aligned")
        for name in ("code", "out", "ws"):
            assert _refused(lib, _decode(lib, d, **{name: 0x1000 + off}), b"st_decode_long", name.encode() + b" must be 16-byte aligned"), (name, off)
        for name in ("code", "ws"):
            assert _refused(lib, _encode(lib, d, **{name: 0x1000 + off}), b"st_encode_long", name.encode() + b" must be 16-byte aligned"), (name, off)
        for name in ("code", "knobs", "adam_m", "adam_v", "ws", "signal", "target"):
            assert _refused(lib, _fit(lib, d, **{name: 0x1000 + off}), b"st_fit_knobs_coded", name.encode() + b" must be 16-byte aligned"), (name, off)
    for off in (2, 4, 6):
        assert _refused(lib, _decode(lib, d, fmt=_lib.PCM_S16, signal=0x1000 + off), b"st_decode_long", b"signal must be 8-byte aligned")
        assert _refused(lib, _encode(lib, d, fmt=_lib.PCM_S16, signal=0x1000 + off), b"st_encode_long", b"signal must be 8-byte aligned")
    # an int16 recording on an 8-byte boundary is taken; an n without an output sample then ends the call without a launch
    assert _decode(lib, d, fmt=_lib.PCM_S16, signal=0x1008, n=d.L - d.y) == 0
    assert _encode(lib, d, fmt=_lib.PCM_S16, signal=0x1008, n=d.L - d.y) == 0
    assert _decode(lib, d, n=1) == 0 and _encode(lib, d, n=1) == 0


def test_refuses_bad_and_wide_dims():
    lib = _lib.load()
    for call, entry in ((_decode, b"st_decode_long"), (_encode, b"st_encode_long"), (_fit, b"st_fit_knobs_coded")):
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


def test_python_switches_and_defaults():
    from signaltrain_amd import predict
    from signaltrain_amd.engine import RecordingCode, StepEngine
    p = inspect.signature(predict.fit_knobs).parameters
    assert p["route"].default == "batched" and p["encode_once"].default is False          # defaults do not change
    assert inspect.signature(predict.predict_long).parameters["route"].default == "batched"
    s = inspect.signature(predict.predict_sweep).parameters
    assert list(s)[:5] == ["signal", "knob_settings", "model", "chunk_size", "out_chunk_size"] and s["route"].default == "device"
    with pytest.raises(ValueError, match="route"):
        predict.predict_sweep(np.zeros(16, np.float32), np.zeros((2, 4), np.float32), None, 8192, 2048, route="graph")
    with pytest.raises(ValueError, match="knob_settings"):
        predict.predict_sweep(np.zeros(16, np.float32), np.zeros(4, np.float32), None, 8192, 2048)
    assert "RecordingCode" in StepEngine.fit_knobs.__doc__          # the coded fit: the code in place of the signal (it holds the recording)
    assert list(inspect.signature(StepEngine.encode_long).parameters)[1:] == ["signal", "batch"]
    assert list(inspect.signature(StepEngine.decode_long).parameters)[1:] == ["code", "knobs", "out", "batch"]
    assert "precondition" in StepEngine.encode_long.__doc__
    c = RecordingCode("code", "signal", 10, 2, (1, 2), "f32")
    assert (c.code, c.signal, c.n, c.nwin, c.geometry, c.compute_dtype) == ("code", "signal", 10, 2, (1, 2), "f32")


# ---------------------------------------------------------------------------------------------- conditioning of the GPU cases
@pytest.mark.parametrize("name", D.names())
def test_cases_are_well_conditioned(name):
    """Every recording the GPU file compares with the float64 oracle at gpu_checks.TOL (decode_ref's case table: the three-settings rows, the f32 / f32x3 level
    rows, knob automation, the second-trip recording at the MI355X's 256 CUs, the predict_sweep recording): the float32 oracle's output agrees with the float64
    oracle's to TOL / 4 at every setting used (the rule of tests/dims_table.py; every case qualifies at its first signal seed).  Where a case has several
    settings, the oracle's outputs of any two differ by more than 100 TOL of max|ref|: a decoder that ignored its knobs could not pass."""
    ref, f32 = D.reference(name), D.reference_f32(name)
    assert ref.shape == f32.shape and ref.shape[0] == len(D.case(name)[3])
    for s in range(ref.shape[0]):
        e = float(np.abs(f32[s] - ref[s]).max() / np.abs(ref[s]).max())
        print(f"decode case [{name}] setting {s}: n_out={ref.shape[1]} float32 vs float64 oracle {e:.2e} (bound {G.TOL / 4:.1e})")
        assert e <= G.TOL / 4, (name, s, e)
    for i in range(ref.shape[0]):
        for j in range(i):
            sep = float(np.abs(ref[i] - ref[j]).max())
            assert sep > 100 * G.TOL * max(np.abs(ref[i]).max(), np.abs(ref[j]).max()), (name, i, j, sep)


def test_the_second_trip_case_is_the_mi355x_batch():
    geo = D.case("second_trip")[0]
    nb = D.second_trip_batch(D.MI355X_CUS, geo)
    assert nb == 125 and nb * (int(_lib.load().st_kp(geo["F"])) // 32) > D.MI355X_CUS * D.DEC_WGS * D.DEC_NW >= (nb - 1) * (int(_lib.load().st_kp(geo["F"])) // 32)
