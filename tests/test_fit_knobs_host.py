"""CPU: the host side of the device knob fit (st_fit_knobs, include/signaltrain_hip.h) -- the symbols, the geometries it admits, the workspace size, every
refusal (before any launch: runs without a GPU), the route switch of predict.fit_knobs, and the reference the GPU tests compare against
(tests/fit_knobs_ref.py): its gradient against a finite difference of its objective, its Adam replay against torch's, and the conditioning of its cases."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from oracle import st_oracle as O
from signaltrain_amd import _lib
from tests import fit_knobs_ref as R
from tests import gpu_checks as G
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


def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "signaltrain_hip.h")).read()
    lib = _lib.load()
    for name, decl in (("st_fit_knobs_supported", "st_fit_knobs_supported(const st_dims* d);"),
                       ("st_fit_knobs_ws_bytes", "st_fit_knobs_ws_bytes(const st_dims* d);"),
                       ("st_fit_knobs", "st_fit_knobs(const st_dims* d, const float* params, int fmt, const void* signal, const void* target, long long n,")):
        assert decl in hdr, name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["st_fit_knobs"]
    assert res is C.c_int and len(args) == 20
    assert args[5] is C.c_longlong and args[7] is C.c_longlong and args[10] is C.c_longlong and args[11] is C.c_int
    assert all(a is C.c_float for a in args[12:16])
    assert _lib.SIGNATURES["st_fit_knobs_ws_bytes"][0] is C.c_size_t and _lib.SIGNATURES["st_fit_knobs_supported"][0] is C.c_int


@pytest.mark.parametrize("prec", range(6))
def test_supported_is_predict_supported_with_knobs(prec):
    lib = _lib.load()
    cases = [dims(row, prec=prec, K=K) for row in ROWS for K in (0, 1, 4)] + [dims(None, prec=prec, K=K) for K in (0, 4)] + \
            [_lib.geometry(8, 4, 4, 2).with_arith(prec=prec)]
    for d in cases:
        want = int(bool(lib.st_predict_supported(C.byref(d))) and d.K >= 1)
        assert lib.st_fit_knobs_supported(C.byref(d)) == want, (d.N, d.T, d.OT, d.K, prec)
    assert any(lib.st_fit_knobs_supported(C.byref(d)) for d in cases) and not all(lib.st_fit_knobs_supported(C.byref(d)) for d in cases)
    bad = dims("n256", prec=prec); bad.OT = bad.T + 1
    assert lib.st_fit_knobs_supported(C.byref(bad)) == 0


@pytest.mark.parametrize("row,B", [(None, 5), ("n256", 5), ("h256", 3), ("tiny", 2)])
def test_workspace_holds_the_predict_workspace(row, B):
    lib = _lib.load()
    for prec in range(6):
        d = dims(row, B=B, prec=prec)
        need, pred = int(lib.st_fit_knobs_ws_bytes(C.byref(d))), int(lib.st_predict_ws_bytes(C.byref(d)))
        assert pred > 0 and need >= pred, (row, prec, need, pred)
        # the rows, the accumulator and the per-group scratch of a batch come on top
        assert need - pred >= 4 * (B * d.K + 2 * B * (lib.st_kp(d.F) // 32) * 16), (row, prec)
        assert need % 16 == 0
        for b in range(1, B):
            assert int(lib.st_fit_knobs_ws_bytes(C.byref(d.with_batch(b)))) <= need, (row, prec, b)      # never grows for a smaller batch


def test_workspace_is_zero_for_bad_or_unsupported_dims():
    lib = _lib.load()
    d = dims("n256"); d.B = 0
    assert lib.st_fit_knobs_ws_bytes(C.byref(d)) == 0
    d = dims("n256"); d.y += 4
    assert lib.st_fit_knobs_ws_bytes(C.byref(d)) == 0
    d = dims("n256"); d.prec = 7
    assert lib.st_fit_knobs_ws_bytes(C.byref(d)) == 0
    assert lib.st_fit_knobs_ws_bytes(C.byref(dims("n256", K=0))) == 0
    for row in WIDE_ROWS:
        if not lib.st_fit_knobs_supported(C.byref(dims(row))):
            assert lib.st_fit_knobs_ws_bytes(C.byref(dims(row))) == 0, row


PTRS = ("params", "signal", "target", "knobs", "adam_m", "adam_v", "loss_hist", "grad_hist", "ws")


def _call(lib, d, n=None, fmt=0, knob_rows=1, first_step=1, steps=2, lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8, **ptrs):
    """st_fit_knobs with dummy pointers (never dereferenced on the host; a refused call launches nothing)."""
    q = {k: 0x1000 for k in PTRS}; q.update(ptrs)
    p = lambda v: C.c_void_p(v) if v else None
    n = 3 * d.L if n is None else n
    return lib.st_fit_knobs(C.byref(d), p(q["params"]), fmt, p(q["signal"]), p(q["target"]), n, p(q["knobs"]), knob_rows, p(q["adam_m"]), p(q["adam_v"]),
                            first_step, steps, lr, beta1, beta2, eps, p(q["loss_hist"]), p(q["grad_hist"]), p(q["ws"]), None)


def _refused(lib, rc, *words):
    msg = lib.st_last_error()
    return rc == -1 and b"st_fit_knobs" in msg and all(w in msg for w in words)


@pytest.mark.parametrize("missing", [p for p in PTRS if p != "grad_hist"])
def test_refuses_a_null_pointer_by_name(missing):
    lib = _lib.load()
    rc = _call(lib, dims("n256"), **{missing: 0})
    assert _refused(lib, rc, b"null", missing.encode()), lib.st_last_error()


def test_grad_hist_may_be_null():
    lib = _lib.load()
    d = dims("n256")
    assert _call(lib, d, grad_hist=0, n=d.L - d.y) == 0          # passes every check; no output sample: ST_OK without a launch
    assert _refused(lib, _call(lib, d, grad_hist=0, ws=0x1004), b"ws must be 16-byte aligned")


def test_refuses_bad_lengths_formats_rows_and_steps():
    lib = _lib.load()
    d = dims("n256")
    for n in (0, -1):
        assert _refused(lib, _call(lib, d, n=n), b"n must be positive")
    for fmt in (-1, 2, 7):
        assert _refused(lib, _call(lib, d, fmt=fmt), b"fmt")
    n = d.L + 3 * d.y + 5
    nwin = int(lib.st_predict_windows(C.byref(d), n))
    assert nwin == 5
    for rows in (0, 2, nwin - 1, nwin + 1, -1):
        assert _refused(lib, _call(lib, d, n=n, knob_rows=rows), b"knob_rows"), rows
    for rows in (1, nwin):          # the two accepted row counts pass this check: the next refusal is another rule's
        assert _refused(lib, _call(lib, d, n=n, knob_rows=rows, ws=0x1004), b"aligned"), rows
    for steps in (0, -3):
        assert _refused(lib, _call(lib, d, steps=steps), b"steps")
    for first in (0, -1):
        assert _refused(lib, _call(lib, d, first_step=first), b"first_step")
    assert _refused(lib, _call(lib, dims("n256", K=0)), b"K = 0")


def test_refuses_bad_hyperparameters():
    lib = _lib.load()
    d = dims("n256")
    inf, nan = float("inf"), float("nan")
    for lr in (-1e-3, inf, nan):
        assert _refused(lib, _call(lib, d, lr=lr), b"lr"), lr
    for b in (-0.1, 1.0, 1.5, inf, nan):
        assert _refused(lib, _call(lib, d, beta1=b), b"beta1"), b
        assert _refused(lib, _call(lib, d, beta2=b), b"beta2"), b
    for e in (0.0, -1e-8, inf, nan):
        assert _refused(lib, _call(lib, d, eps=e), b"eps"), e
    assert _call(lib, d, lr=0.0, beta1=0.0, beta2=0.0, n=1) == 0      # the closed ends are taken


def test_refuses_misaligned_buffers():
    lib = _lib.load()
    d = dims("n256")
    for name in ("signal", "target"):
        for off in (4, 8, 12):
            assert _refused(lib, _call(lib, d, **{name: 0x1000 + off}), name.encode() + b" must be 16-byte aligned"), (name, off)
        for off in (2, 4, 6):
            assert _refused(lib, _call(lib, d, fmt=_lib.PCM_S16, **{name: 0x1000 + off}), name.encode() + b" must be 8-byte aligned"), (name, off)
    for name in ("knobs", "adam_m", "adam_v", "ws"):
        for off in (4, 8, 12):
            assert _refused(lib, _call(lib, d, **{name: 0x1000 + off}), name.encode() + b" must be 16-byte aligned"), (name, off)
    # an int16 pair on an 8-byte boundary is taken; an n without an output sample then ends the call without a launch
    assert _call(lib, d, fmt=_lib.PCM_S16, signal=0x1008, target=0x1008, n=d.L - d.y) == 0
    assert _call(lib, d, n=1) == 0


def test_refuses_bad_and_unsupported_dims():
    lib = _lib.load()
    d = dims("n256"); d.B = 0
    assert _refused(lib, _call(lib, d), b"dimension")
    d = dims("n256"); d.y += 4
    assert _refused(lib, _call(lib, d), b"y must equal")
    d = dims("n256"); d.prec = 9
    assert _refused(lib, _call(lib, d), b"prec")
    n_wide = 0
    for d in [dims(r) for r in WIDE_ROWS] + [_lib.geometry(8, 4, 4, 2)]:
        if not lib.st_fit_knobs_supported(C.byref(d)):
            n_wide += 1
            assert _refused(lib, _call(lib, d), b"st_fit_knobs_supported")
    assert n_wide > 0


def test_fit_knobs_route_switch():
    from signaltrain_amd import predict
    from signaltrain_amd.engine import StepEngine
    p = inspect.signature(predict.fit_knobs).parameters
    assert p["route"].default == "batched" and predict.FIT_ROUTES == ("batched", "device")
    assert predict.ROUTES == ("batched", "device")                     # predict_long's routes: unchanged
    with pytest.raises(ValueError, match="route"):
        predict.fit_knobs(np.zeros(16, np.float32), np.zeros(16, np.float32), None, 8192, 2048, route="graph")
    q = inspect.signature(StepEngine.fit_knobs).parameters
    assert list(q)[1:] == ["signal", "target", "knobs", "steps", "lr", "betas", "eps", "batch", "state", "want_grads"]
    assert (q["steps"].default, q["lr"].default, q["betas"].default, q["eps"].default) == (50, 0.05, (0.9, 0.999), 1e-8)
    assert q["batch"].default is None and q["state"].default is None and q["want_grads"].default is False
    assert "n = L + k y" in StepEngine.fit_knobs.__doc__ and "chunk_size + k * out_chunk_size" in predict.fit_knobs.__doc__


# ---------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("row", ["tiny", "n32"])
def test_reference_gradient_is_the_derivative_of_its_objective(row):
    """The rescaled masked-tail d_knobs (summed over the windows) against a central finite difference of J in float64.  Step h = 1e-4: the truncation error
    of the central difference is h^2 / 6 * |J'''|, estimated from the differences themselves as |fd(h) - fd(2h)| / 3 (Richardson: fd(2h) - fd(h) = 3 x the
    error of fd(h) to leading order); rounding adds ~ eps64 * J / h ~ 1e-13.  Bound: 10 x that estimate + 1e-9 of max|g| -- both printed."""
    geo, P = R.case(row)
    sig, tgt = R.pair(row, hops=2)
    kn = R.KN.astype(np.float64)
    _, g, _ = R.objective(sig, tgt, kn, P, geo)
    g = g.sum(0)
    h = 1e-4

    def fd(step):
        out = np.zeros_like(kn)
        for k in range(kn.size):
            e = np.zeros_like(kn); e[k] = step
            out[k] = (R.objective(sig, tgt, kn + e, P, geo, want_grad=False)[0] - R.objective(sig, tgt, kn - e, P, geo, want_grad=False)[0]) / (2 * step)
        return out
    f1, f2 = fd(h), fd(2 * h)
    trunc = np.abs(f1 - f2) / 3
    bound = 10 * trunc + 1e-9 * np.abs(g).max()
    print(f"fit reference [{row}]: h={h:g} g={g} fd={f1} |g - fd|={np.abs(g - f1)} curvature estimate of the fd error={trunc} bound={bound}")
    assert np.abs(g).max() > 0
    assert np.all(np.abs(g - f1) <= bound), (g, f1, bound)


def test_adam_replay_is_torchs_adam_in_float64():
    rng = np.random.default_rng(5)
    k0 = np.array([[0.1, -0.3, 0.499, -0.45], [0.0, 0.2, -0.499, 0.3]])
    grads = rng.standard_normal((12, 2, 4)) * 10.0 ** rng.uniform(-4, 0, (12, 2, 4))
    grads[:, 0, 2] = -np.abs(grads[:, 0, 2])                  # pushes 0.499 up and out: the clamp acts
    p = torch.tensor(k0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=0.05, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    for g in grads:
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        with torch.no_grad():
            p.clamp_(-0.5, 0.5)
    got, m, v = R.adam_replay(k0, grads)
    st = opt.state[p]
    assert got[0, 2] == 0.5
    for a, b in ((got, p.detach().numpy()), (m, st["exp_avg"].numpy()), (v, st["exp_avg_sq"].numpy())):
        assert np.abs(a - b).max() <= 4 * np.finfo(np.float64).eps * max(np.abs(b).max(), 1e-300), np.abs(a - b).max()
    # chained through (m, v, first_step): the same trajectory
    p1, m1, v1 = R.adam_replay(k0, grads[:5])
    p2, m2, v2 = R.adam_replay(p1, grads[5:], first_step=6, m=m1, v=v1)
    assert np.array_equal(p2, got) and np.array_equal(m2, m) and np.array_equal(v2, v)


@pytest.mark.parametrize("row", R.ROWS)
def test_cases_are_well_conditioned(row):
    """Every case the GPU file compares at fp32 tolerance: the float32 oracle's d_knobs (one row and per window) and J agree with the float64 oracle's to a
    quarter of that tolerance (2e-4 of max|ref| on the gradient, gpu_checks.TOL relative on J) -- the rule of tests/dims_table.py."""
    geo, P = R.case(row)
    sig, tgt = R.pair(row)
    J64, g64, _ = R.objective(sig, tgt, R.KN, P, geo)
    J32, g32, _ = R.objective(sig, tgt, R.KN, P, geo, dtype=np.float32)
    e_sum = np.abs(g32.sum(0) - g64.sum(0)).max() / np.abs(g64.sum(0)).max()
    e_win = np.abs(g32 - g64).max() / np.abs(g64).max()
    e_J = abs(J32 - J64) / abs(J64)
    print(f"fit case [{row or 'default'}]: nwin={g64.shape[0]} J={J64:.6e} f32 vs f64: grad sum {e_sum:.2e} per window {e_win:.2e} J {e_J:.2e}")
    assert e_sum <= R.TOL_GRAD["f32"] / 4 and e_win <= R.TOL_GRAD["f32"] / 4 and e_J <= G.TOL / 4, (row, e_sum, e_win, e_J)
