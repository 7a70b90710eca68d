"""CPU: the host side of the on-device validation pass (st_eval_step, include/signaltrain_hip.h) -- the symbol and its ctypes signature, its
refusals (before any launch: runs without a GPU), the driver's device_eval switch, and the workspace sizes, which the MAE partials must not change
(they live in the d syn area of the workspace)."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import pytest

from signaltrain_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_step_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "signaltrain_hip.h")).read()
    assert "int st_eval_step(const st_dims* d" in hdr
    lib = _lib.load()
    assert hasattr(lib, "st_eval_step")
    res, args = _lib.SIGNATURES["st_eval_step"]
    assert res is C.c_int and len(args) == 10 and args[8] is C.c_double and args[0] is C.POINTER(_lib.st_dims)


def _call(lib, d, params=1, x=1, knobs=1, y=1, ws=1, acc=1):
    """st_eval_step with dummy non-null pointers (0x1000: never dereferenced on the host, and a refused call launches nothing)."""
    p = lambda on: C.c_void_p(0x1000) if on else None
    return lib.st_eval_step(C.byref(d), p(params), p(x), p(knobs), p(y), None, p(ws), p(acc), 0.98, None)


@pytest.mark.parametrize("missing", ["params", "x", "y", "ws", "acc"])
def test_eval_step_refuses_a_null_pointer_by_name(missing):
    lib = _lib.load()
    d = _lib.geometry(1, 4, 4, 2)
    rc = _call(lib, d, **{missing: 0})
    msg = lib.st_last_error()
    assert rc == -1 and b"st_eval_step" in msg and b"null" in msg
    assert {"y": b"y_true"}.get(missing, missing.encode()) in msg, msg


def test_eval_step_knobs_may_be_null_only_without_knobs():
    lib = _lib.load()
    rc = _call(lib, _lib.geometry(1, 4, 4, 2), knobs=0)
    assert rc == -1 and b"knobs" in lib.st_last_error()
    d0 = _lib.geometry(1, 4, 0, 2)
    rc = _call(lib, d0, knobs=0, acc=0)               # K = 0: the null knobs pass, the next check (acc) refuses -- still no launch
    assert rc == -1 and b"acc" in lib.st_last_error() and b"knobs" not in lib.st_last_error()


def test_eval_step_refuses_bad_dims():
    lib = _lib.load()
    d = _lib.geometry(1, 4, 4, 2); d.B = 0
    assert _call(lib, d) == -1 and b"dimension" in lib.st_last_error()
    d = _lib.geometry(1, 4, 4, 2); d.y += 4                   # y != (OT - 1) H - N
    assert _call(lib, d) == -1 and b"y must equal" in lib.st_last_error()
    d = _lib.geometry(1, 4, 4, 2); d.F -= 1
    assert _call(lib, d) == -1 and b"F must be" in lib.st_last_error()
    d = _lib.geometry(1, 4, 4, 2); d.prec = 9
    assert _call(lib, d) == -1 and b"prec" in lib.st_last_error()


def test_run_train_has_the_device_eval_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_train.py"), "--device-eval", "--target", "nope"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "invalid target type" in r.stderr, r.stderr          # passed argument parsing


def test_driver_accepts_device_eval():
    from signaltrain_amd import train
    from signaltrain_amd.engine import StepEngine
    for fn in (train.eval_status_save, train.train_loop, train.train):
        p = inspect.signature(fn).parameters
        assert "device_eval" in p and p["device_eval"].default is False, fn.__name__      # the host path stays the default
    for name in ("eval_step", "eval_reset", "eval_read"):
        assert callable(getattr(StepEngine, name))
    p = inspect.signature(StepEngine.eval_step).parameters
    assert p["beta"].default == 0.98 and p["want_y_hat"].default is False
    assert inspect.signature(StepEngine.eval_reset).parameters["vl_avg"].default == 0.0


# (scale, shrink, K, B) -> per st_dims.prec 0..5: (st_workspace_bytes, st_workspace_bytes_max), recorded from the commit before st_eval_step existed
WS_BEFORE = {
    (1, 4, 4, 256): [(701613568, 701613568), (701613568, 701613568), (407484928, 701613568), (701613568, 701613568), (407484928, 701613568), (701613568, 701613568)],
    (8, 4, 4, 4): [(114103040, 114103040)] * 6,
    (1, 2, 4, 8): [(84867072, 84867072), (84867072, 84867072), (75675648, 84867072), (84867072, 84867072), (75675648, 84867072), (84867072, 84867072)],
    (1, 4, 4, 585): [(1413287424, 1413287424), (1413287424, 1413287424), (741161472, 1413287424), (1413287424, 1413287424), (741161472, 1413287424),
                     (1413287424, 1413287424)],
}


@pytest.mark.parametrize("geom", sorted(WS_BEFORE))
def test_workspace_sizes_are_unchanged(geom):
    lib = _lib.load()
    sc, sh, K, B = geom
    for prec in range(6):
        d = _lib.geometry(sc, sh, K, B).with_arith(prec=prec)
        got = (int(lib.st_workspace_bytes(C.byref(d))), int(lib.st_workspace_bytes_max(C.byref(d))))
        assert got == WS_BEFORE[geom][prec], (geom, prec, got)
    # ... and the MAE partials fit the area they borrow (d syn, B * (y + 2N) floats)
    d = _lib.geometry(sc, sh, K, B)
    assert lib.st_ola_loss_partials(C.byref(d)) <= d.B * (d.y + 2 * d.N)
