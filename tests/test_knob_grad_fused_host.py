"""Host side of st_model_bwd_knobs (the knob gradient out of the one backward pass of the batch): the exported symbols, the scratch size and every
refusal -- all decided before any launch, so none of this needs a device (the library loads without one, cf. tests/test_effects_family.py)."""
import ctypes as C
import os

import pytest

from signaltrain_amd import _lib

ERR_ARG, ERR_UNSUPPORTED = -1, -3
NEW = ("st_knob_grad_fused_supported", "st_model_bwd_knobs_ws_floats", "st_model_bwd_knobs")


def _dims(scale=1, shrink=4, K=4, B=3, dtype="f32"):
    d = _lib.geometry(scale, shrink, K, B)
    d.prec = _lib.PREC[dtype]
    return d


def _call(lib, d, null=None):
    """st_model_bwd_knobs with dummy host buffers (a refusal comes before anything is read or launched); null: the argument position to pass as NULL."""
    bufs = [(C.c_float * 4)() for _ in range(10)]
    args = [C.cast(b, C.c_void_p) for b in bufs]       # params grads x knobs g_y_hat g_mag_hat g_mag ws scratch g_knobs
    if null is not None:
        args[null] = None
    return lib.st_model_bwd_knobs(C.byref(d), *args, None)


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "signaltrain_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name


@pytest.mark.parametrize("scale,B", [(1, 1), (1, 3), (1, 256), (2, 3)])
def test_scratch_size(scale, B):
    lib = _lib.load()
    d = _dims(scale=scale, B=B)
    assert lib.st_model_bwd_knobs_ws_floats(C.byref(d)) == 2 * B * (lib.st_kp(d.F) // 32) * 16
    assert lib.st_kp(d.F) % 32 == 0


def test_scratch_size_is_zero_for_bad_dims():
    lib = _lib.load()
    d = _dims(); d.F += 1
    assert lib.st_model_bwd_knobs_ws_floats(C.byref(d)) == 0 and b"F must be N/2+1" in lib.st_last_error()
    d = _dims(); d.B = 0
    assert lib.st_model_bwd_knobs_ws_floats(C.byref(d)) == 0
    assert lib.st_knob_grad_fused_supported(C.byref(d)) == 0


@pytest.mark.parametrize("scale,dtype", [(1, "f32"), (1, "bf16_all"), (1, "f16_all"), (1, "bf16"), (1, "f32x3"), (2, "f32"), (2, "bf16_all"), (8, "f16_all")])
def test_supported_at_the_shipped_defaults(scale, dtype):
    lib = _lib.load()
    for K in (1, 4, 7):
        assert lib.st_knob_grad_fused_supported(C.byref(_dims(scale=scale, K=K, dtype=dtype))) == 1, (K, lib.st_last_error())
    assert lib.st_knob_grad_fused_supported(C.byref(_dims(scale=scale, K=0, dtype=dtype))) == 0
    assert b"K = 0" in lib.st_last_error()


@pytest.mark.parametrize("pos", [0, 1, 2, 3, 4, 7, 8, 9])
def test_null_pointer_is_refused(pos):
    lib = _lib.load()
    assert _call(lib, _dims(), null=pos) == ERR_ARG and b"st_model_bwd_knobs: null pointer" in lib.st_last_error()


def test_optional_upstream_gradients_may_be_null_but_the_call_still_ends_at_the_next_rule():
    """g_mag_hat / g_mag are optional: passing NULL for them is not what refuses this call (K = 0 is)."""
    lib = _lib.load()
    d = _dims(K=0)
    bufs = [(C.c_float * 4)() for _ in range(8)]
    p = [C.cast(b, C.c_void_p) for b in bufs]
    rc = lib.st_model_bwd_knobs(C.byref(d), p[0], p[1], p[2], p[3], p[4], None, None, p[5], p[6], p[7], None)
    assert rc == ERR_ARG and b"K = 0" in lib.st_last_error()


def test_bad_dims_are_refused_with_the_rule():
    lib = _lib.load()
    d = _dims(); d.y += 4
    assert _call(lib, d) == ERR_ARG and b"y must equal" in lib.st_last_error()
    d = _dims(); d.prec = 17
    assert _call(lib, d) == ERR_ARG and b"ST_PREC" in lib.st_last_error()


@pytest.mark.parametrize("code,dtype,word", [(8001, "f32", b"g_ae_split"), (8000, "bf16_all", b"g_ae_split"), (8000, "f16_all", b"g_ae_split"), (8200, "f32", b"g_ae_save")])
def test_diagnostic_routes_without_the_output_are_unsupported(code, dtype, word):
    lib = _lib.load()
    d, wide = _dims(dtype=dtype), _dims(scale=2, dtype=dtype)
    assert lib.st_knob_grad_fused_supported(C.byref(d)) == 1
    try:
        assert lib.st_set_tuning(code) == 0
        assert lib.st_knob_grad_fused_supported(C.byref(d)) == 0 and word in lib.st_last_error()
        assert _call(lib, d) == ERR_UNSUPPORTED and word in lib.st_last_error() and b"st_model_bwd_knobs" in lib.st_last_error()
        assert lib.st_knob_grad_fused_supported(C.byref(wide)) == 1          # the wide path has one kernel form, whatever these switches say
    finally:
        lib.st_reset_tuning()
    assert lib.st_knob_grad_fused_supported(C.byref(d)) == 1
