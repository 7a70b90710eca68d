"""GPU: the per-epoch validation pass on the device -- st_eval_step / StepEngine.eval_step / train.eval_status_save(device_eval=True).

One validation batch of the reference's train.py:28-42 (forward, calc_loss with scale_by_freq, mae) as one C call that keeps the running average on the
device; checked against the float64 oracle, against the training step's own forward at every arithmetic level, against the rounding oracle at the 16-bit
levels, and through the driver against the host-side pass."""
import contextlib
import os

import numpy as np
import pytest
import torch

from oracle import st_oracle as O
from tests import gpu_checks as G

pytestmark = pytest.mark.gpu

# (B, make_case keywords): the geometries the validation pass must cover
GEOMETRIES = {
    "default-B5": (5, {}), "default-B64": (64, {}), "default-B256": (256, {}), "scale8-B4": (4, dict(scale=8)),
    "shrink2-B6": (6, dict(shrink=2)), "K0-B6": (6, dict(K=0)), "K1-B6": (6, dict(K=1)),
}
LEVELS = {
    "f32": contextlib.nullcontext, "f32x3": G.split_mode,
    "bf16": lambda: G.mixed_mode(1, half="bf16"), "bf16_all": lambda: G.mixed_mode(2, half="bf16"),
    "f16": lambda: G.mixed_mode(1, half="f16"), "f16_all": lambda: G.mixed_mode(2, half="f16"),
}


def _case(B, seed, **kw):
    K = kw.get("K", 4)
    geo, X, Y, KN, P = G.make_case(B, seed, **kw)
    return geo, X, Y, KN, P, G.dims_of(geo, B, K)


def _oracle_terms(X, Y, KN, P, geo):
    """loss, mean log-cosh, L1 term, MAE and y_hat of one validation batch in float64 (with whatever operand rounding the current mode gives the oracle)."""
    f = np.float64
    out, _, mag_hat = O.model_fwd(X.astype(f), KN.astype(f), {k: v.astype(f) for k, v in P.items()}, geo)
    w = O.freq_weights(geo["F"], f)
    loss = O.calc_loss(out, Y.astype(f), mag_hat, w)
    lc = float(np.mean(O.logcosh(Y.astype(f) - out)))
    l1 = float(O.L1_LAMBDA / 10 * np.mean(np.abs(mag_hat * w)))
    return float(loss), lc, l1, float(np.abs(out - Y.astype(f)).mean()), out


def _eval_once(eng, X, KN, Y, want_y_hat=True, beta=0.98):
    eng.eval_reset()
    y_hat = eng.eval_step(G.t(X), G.t(KN), G.t(Y), beta=beta, want_y_hat=want_y_hat)
    return eng.eval_read(), y_hat


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_eval_step_against_the_float64_oracle(name):
    """fp32 level: loss, mean log-cosh, L1 term and MAE within the suite's standing fp32 bar (gpu_checks.TOL = 1e-4 relative) of the float64 oracle.
    Measured worst over these geometries: see DESIGN.md section 4 (the figure is printed here)."""
    B, kw = GEOMETRIES[name]
    geo, X, Y, KN, P, d = _case(B, 11, **kw)
    eng = G.new_engine(d); eng.load_state_dict(P)
    acc, y_hat = _eval_once(eng, X, KN, Y)
    loss, lc, l1, mae, out = _oracle_terms(X, Y, KN, P, geo)
    rel = {k: abs(g - r) / abs(r) for k, g, r in (("loss", acc[1], loss), ("logcosh", acc[2], lc), ("l1_term", acc[3], l1), ("mae", acc[4], mae))}
    rel["y_hat"] = float(np.abs(G.n(y_hat) - out).max() / np.abs(out).max())
    print(f"eval_step vs float64 oracle [{name}]: " + " ".join(f"{k}={v:.2e}" for k, v in rel.items()) + f"  worst={max(rel.values()):.2e}")
    assert acc[5] == 1.0 and acc[6] == acc[1] and acc[7] == acc[4] and acc[0] == (1 - 0.98) * acc[1]
    for k, v in rel.items():
        assert v <= G.TOL, (name, k, v)


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
@pytest.mark.parametrize("level", list(LEVELS))
def test_eval_step_is_the_training_forward(level, name):
    """Every arithmetic level and every geometry: acc[1..3] and y_hat against scalars[0..2] and y_hat of loss_backward(want_outputs=True) on the same
    engine, parameters and batch -- the same kernels and summation trees, asserted to 1e-6 relative.  Whether they were bit-equal is printed per case.  As
    measured on MI355X: bit-equal (loss, mean log-cosh, L1 term and every y_hat sample) in all 42 cases.  That needs contraction off in
    eval_finalize_kernel: left on, the compiler fused the sum of the two loss terms with the product that forms the log-cosh mean, which it does not do in
    finalize_kernel, and the loss was one ulp off in a third of the cases."""
    B, kw = GEOMETRIES[name]
    with LEVELS[level]():
        geo, X, Y, KN, P, d = _case(B, 12, **kw)
        eng = G.new_engine(d); eng.load_state_dict(P)
        outs = eng.loss_backward(G.t(X), G.t(KN), G.t(Y), want_outputs=True)
        sc = eng.scalars.detach().cpu().numpy().copy()
        acc, y_hat = _eval_once(eng, X, KN, Y)
        a32 = np.asarray(acc[1:4], np.float32)
        bits = bool(np.array_equal(a32, sc[:3])) and bool(torch.equal(y_hat, outs[0]))
        print(f"eval_step vs training forward [{level} {name}]: bit-equal={bits} eval={a32.tolist()} train={sc[:3].tolist()}")
        for i in range(3):
            assert abs(acc[1 + i] - float(sc[i])) <= 1e-6 * abs(float(sc[i])), (level, name, i, acc[1 + i], sc[i])
        ref = G.n(outs[0])
        assert np.abs(G.n(y_hat) - ref).max() <= 1e-6 * np.abs(ref).max()


@pytest.mark.parametrize("half,lvl", [("bf16", 1), ("bf16", 2), ("f16", 1), ("f16", 2)])
def test_eval_step_16bit_against_the_rounding_oracle(half, lvl):
    """The 16-bit levels against the oracle that rounds the same operands, at the tolerances run_fused uses for a fused forward (mixed_mode.FUSED_TOL /
    FUSED_TOL_F16 x 1e-4): y_hat relative to max|y_hat| and the loss relative to itself, as run_fused checks them; the two terms of the loss relative to
    their sum; the MAE relative to max|y_hat|, since |d MAE| <= mean|d y_hat| <= max|d y_hat|."""
    ts = (G.mixed_mode.FUSED_TOL if half == "bf16" else G.mixed_mode.FUSED_TOL_F16)[lvl]
    with G.mixed_mode(lvl, half=half, tol_scale=ts):
        geo, X, Y, KN, P, d = _case(4, 13)
        restore = G.follow_effective_arithmetic(d)
        try:
            eng = G.new_engine(d); eng.load_state_dict(P)
            acc, y_hat = _eval_once(eng, X, KN, Y)
            loss, lc, l1, mae, out = _oracle_terms(X, Y, KN, P, geo)
        finally:
            restore()
        ymax = float(np.abs(out).max())
        res = [G.err("eval.y_hat", G.n(y_hat), out), G.err("eval.loss", acc[1], loss), G.err("eval.logcosh", acc[2], lc, scale=loss),
               G.err("eval.l1_term", acc[3], l1, scale=loss), G.err("eval.mae", acc[4], mae, scale=ymax)]
        G.report(res)
        assert all(r["ok"] for r in res), [r for r in res if not r["ok"]]


def test_running_average_on_the_device():
    """N = 12 batches of different data, beta = 0.98, seeded with acc[0] = v0: acc[0] is the host recurrence of train.py:33 over the per-batch losses,
    acc[5] counts, acc[4] is the last batch's MAE, acc[6] / acc[7] are the sums; the pass needs no read in between; eval_reset restores the seed state."""
    N, B, beta, v0 = 12, 4, 0.98, 0.37
    geo, X, Y, KN, P, _ = _case(N * B, 14)
    d = G.dims_of(geo, B, 4)
    eng = G.new_engine(d); eng.load_state_dict(P)
    eng.eval_reset(v0)
    assert eng.eval_acc.dtype == torch.float64 and eng.eval_acc.is_cuda and eng.eval_read() == [v0] + [0.0] * 7
    losses, maes, maes_host = [], [], []
    # the MAE recomputed on the host in float64 from the y_hat the call returns: the device sums B * y fp32 terms pairwise (worst case log2(n) roundings),
    # after one rounding per |y - y_hat| and before one for the mean
    mae_tol = (np.log2(B * geo["y"]) + 3) * 2.0 ** -24
    for i in range(N):
        s = slice(i * B, (i + 1) * B)
        y_hat = eng.eval_step(G.t(X[s]), G.t(KN[s]), G.t(Y[s]), beta=beta, want_y_hat=True)
        a = eng.eval_read()
        losses.append(a[1]); maes.append(a[4])
        maes_host.append(float(np.abs(G.n(y_hat) - Y[s].astype(np.float64)).mean()))
        assert a[5] == i + 1 and abs(a[4] - maes_host[-1]) <= mae_tol * maes_host[-1], (i, a[4], maes_host[-1])
        assert np.float32(a[1]) == np.float32(a[2]) + np.float32(a[3])                 # the loss is the sum of its two terms as fp32 adds them
    final = eng.eval_read()
    assert abs(final[7] - sum(maes_host)) <= mae_tol * sum(maes_host)
    v = v0
    for l in losses:
        v = beta * v + (1 - beta) * l
    assert len(set(losses)) == N and abs(final[0] - v) <= 1e-12 * abs(v), (final[0], v)
    assert final[5] == N and final[4] == maes[-1] and final[1] == losses[-1]
    assert abs(final[6] - sum(losses)) <= 1e-12 * sum(losses) and abs(final[7] - sum(maes)) <= 1e-12 * sum(maes)
    eng.eval_reset(v0)                                   # the same pass without a read in between
    for i in range(N):
        s = slice(i * B, (i + 1) * B)
        assert eng.eval_step(G.t(X[s]), G.t(KN[s]), G.t(Y[s]), beta=beta) is None
    assert eng.eval_read() == final
    eng.eval_reset(v0)
    assert eng.eval_read() == [v0] + [0.0] * 7
    eng.eval_reset()
    assert eng.eval_read() == [0.0] * 8


def test_eval_step_changes_no_training_state():
    geo, X, Y, KN, P, d = _case(6, 15)
    eng = G.new_engine(d); eng.load_state_dict(P)
    eng.train_step(G.t(X), G.t(KN), G.t(Y), 1e-3)
    before = [b.clone() for b in (eng.params, eng.grads, eng.m, eng.v, eng.scalars)]
    gen = eng.generation
    eng.eval_step(G.t(np.roll(X, 5, axis=1)), G.t(KN), G.t(np.roll(Y, 5, axis=1)), want_y_hat=True)
    torch.cuda.synchronize()
    assert eng.generation == gen + 1
    for a, b, name in zip(before, (eng.params, eng.grads, eng.m, eng.v, eng.scalars), ("params", "grads", "m", "v", "scalars")):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("level", ["f32", "bf16_all"])
def test_eval_steps_between_train_steps_leave_the_trajectory_alone(level):
    """train, eval, train, eval, train == three bare train steps, bit for bit."""
    with LEVELS[level]():
        geo, X, Y, KN, P, d = _case(6, 16)
        Xe, Ye = np.roll(X, 9, axis=1).copy(), np.roll(Y, 9, axis=1).copy()
        engs = []
        for with_eval in (True, False):
            eng = G.new_engine(d); eng.load_state_dict(P)
            for it in range(3):
                eng.train_step(G.t(np.roll(X, 17 * it, axis=1).copy()), G.t(KN), G.t(np.roll(Y, 17 * it, axis=1).copy()), 1e-3)
                if with_eval and it < 2:
                    eng.eval_step(G.t(Xe), G.t(KN), G.t(Ye))
            engs.append(eng)
        torch.cuda.synchronize()
        assert engs[0].step_count == engs[1].step_count == 3
        for name in ("params", "m", "v", "grads"):
            assert torch.equal(getattr(engs[0], name), getattr(engs[1], name)), name
        assert np.isfinite(engs[0].eval_read()).all() and engs[0].eval_read()[5] == 2


def test_eval_step_between_autograd_forward_and_backward():
    """st_model forward, eval_step on the model's engine, loss.backward(): the generation bump makes the backward recompute its forward, so the gradients
    are those of a run without the eval_step."""
    from signaltrain_amd import loss_functions, nn_proc
    nn_proc._QUIET = True
    geo, X, Y, KN, P, d = _case(3, 17)
    m = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=4)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    m = m.to("cuda:0")
    x, kn, yt = G.t(X), G.t(KN), G.t(Y)

    def run(disturb):
        m.zero_grad()
        y, mag, mag_hat = m.forward(x, kn)
        if disturb:
            m.engine(x).eval_step(torch.flip(x, dims=[1]) * 0.3, -kn, yt)
        sb = torch.exp((7. / geo["F"]) * torch.arange(0., geo["F"], device="cuda")).expand_as(mag_hat).float()
        loss_functions.calc_loss(y, yt, mag_hat, scale_by_freq=sb).backward()
        return {k: p.grad.clone() for k, p in m.named_parameters()}
    a, b = run(False), run(True)
    assert any(float(v.abs().max()) > 0 for v in a.values())
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("level", ["f32", "bf16_all"])
@pytest.mark.parametrize("name", ["default-B5", "scale8-B4", "shrink2-B6"])
def test_eval_step_does_not_depend_on_pointer_alignment(name, level):
    """st_eval_step takes the four-samples-per-thread overlap-add kernel when y_true and y_hat are 16-byte aligned and the one-sample kernel otherwise; both
    sum a slot's |y - y_hat| (and log-cosh) by one tree, so loss, log-cosh, L1 term, MAE and y_hat are bit-identical whichever runs.  The same target and
    output buffers are handed over once aligned and once from views that start 4 bytes into their allocation (x stays aligned: the fused forward reads
    it with 16-byte loads in prep_kernel, as the training entries do)."""
    import ctypes as C
    from signaltrain_amd import _lib
    B, kw = GEOMETRIES[name]
    with LEVELS[level]():
        geo, X, Y, KN, P, d = _case(B, 19, **kw)
        eng = G.new_engine(d); eng.load_state_dict(P)
        dd = eng._dims(B)
        x, kn = G.t(X), G.t(KN)

        def run(off):      # off floats into the allocations of y_true and y_hat
            yt_flat = torch.zeros(Y.size + 8, dtype=torch.float32, device=G.DEV)
            yh_flat = torch.zeros(Y.size + 8, dtype=torch.float32, device=G.DEV)
            yt, yh = yt_flat[off:off + Y.size], yh_flat[off:off + Y.size]
            yt.copy_(G.t(Y).reshape(-1))
            assert (yt.data_ptr() % 16 == 0) == (off == 0) and (yh.data_ptr() % 16 == 0) == (off == 0)
            eng.eval_reset()
            _lib.check(eng.lib.st_eval_step(C.byref(dd), _lib.ptr(eng.params), _lib.ptr(x), _lib.ptr(kn), C.c_void_p(yt.data_ptr()), C.c_void_p(yh.data_ptr()),
                                            _lib.ptr(eng.ws), C.c_void_p(eng.eval_acc.data_ptr()), 0.98, G.stream()), "st_eval_step")
            acc = eng.eval_read()
            assert float(yh_flat[:off].abs().sum()) == 0.0 and float(yh_flat[off + Y.size:].abs().sum()) == 0.0      # nothing written outside y_hat
            return acc, yh.cpu().numpy().copy()
        (a, ya), (b, yb) = run(0), run(1)
        print(f"eval_step aligned vs 4 bytes off [{level} {name}]: {a[1:5]} / {b[1:5]}")
        assert a == b and a[4] > 0 and np.array_equal(ya.view(np.uint32), yb.view(np.uint32))


@pytest.mark.parametrize("built,used", [(256, 100), (600, 585)])
def test_smaller_batch_on_a_larger_engine(built, used):
    """An engine whose workspace was sized for `built` windows evaluates `used` (585 of 600: the batch whose workspace is LARGER than its neighbours',
    DESIGN.md section 2) with the results of an engine built for exactly that batch."""
    geo, X, Y, KN, P, _ = _case(used, 18)
    big = G.new_engine(G.dims_of(geo, built, 4)); big.load_state_dict(P)
    a, ya = _eval_once(big, X, KN, Y)
    del big
    torch.cuda.empty_cache()
    exact = G.new_engine(G.dims_of(geo, used, 4)); exact.load_state_dict(P)
    b, yb = _eval_once(exact, X, KN, Y)
    assert a == b and torch.equal(ya, yb) and np.isfinite(a).all() and a[1] > 0


def _driver_run(path, **kw):
    from signaltrain_amd import audio, misc, nn_proc, train
    nn_proc._QUIET = True
    path.mkdir()
    cwd = os.getcwd(); os.chdir(path)
    try:
        torch.manual_seed(0); np.random.seed(0)
        train.train(effect=audio.Compressor_4c(), device=torch.device("cuda:0"), **kw)
        read = lambda f: [l.split() for l in open(f).read().strip().splitlines()]
        sd, _ = misc.load_checkpoint("modelcheckpoint.tar", device="cpu")
        return read("vl_avg_out.dat"), read("val_err_mae.dat"), sd
    finally:
        os.chdir(cwd)


# fp32: what the three-digit log files resolve; 16-bit levels: the fused 16-bit tolerance of gpu_checks (FUSED_TOL[2], FUSED_TOL_F16[2] x 1e-4)
DRIVER_TOL = {"f32": 2e-3, "bf16_all": G.mixed_mode.FUSED_TOL[2] * 1e-4, "f16_all": G.mixed_mode.FUSED_TOL_F16[2] * 1e-4}


@pytest.mark.parametrize("dtype", ["f32", "bf16_all", "f16_all"])
def test_driver_device_eval_matches_the_host_pass(tmp_path, dtype):
    """train.train twice from the same seeds, validation on the host and on the device: two lines in each log file, the logged values agree (fp32: to 2e-3,
    what three-digit files resolve; 16-bit levels: the fused 16-bit tolerance, because there the host pass runs st_model_fwd's fp32-operand GEMMs and the
    device pass the training forward's pre-rounded 16-bit operands), and the training itself is untouched: bit-identical checkpoints."""
    kw = dict(epochs=2, n_data_points=2048, batch_size=256, device_feed=True, compute_dtype=dtype)
    host = _driver_run(tmp_path / "host", device_eval=False, **kw)
    dev = _driver_run(tmp_path / "dev", device_eval=True, **kw)
    for h, v in zip(host[:2], dev[:2]):
        assert len(h) == 2 and len(v) == 2 and [l[0] for l in v] == ["1", "2"]
        for lh, lv in zip(h, v):
            a, b = float(lh[1]), float(lv[1])
            print(f"driver [{dtype}] epoch {lh[0]}: host {a:.3e} device {b:.3e} rel {abs(a - b) / abs(a):.1e}")
            assert np.isfinite(a) and np.isfinite(b) and abs(a - b) <= DRIVER_TOL[dtype] * abs(a), (dtype, lh, lv)
    assert list(host[2]) == list(dev[2])
    for k in host[2]:
        assert torch.equal(host[2][k], dev[2][k]), k


def test_driver_device_eval_without_a_validation_batch(tmp_path):
    """25 validation windows < one batch of 48: no eval_step call, vl_avg stays, the MAE column says nan, both files get their two lines (as the host path)."""
    vl, mae, sd = _driver_run(tmp_path / "awk", epochs=2, n_data_points=100, batch_size=48, device_eval=True)
    assert [l[0] for l in mae] == ["1", "2"] and all(l[1] == "nan" for l in mae)
    assert len(vl) == 2 and all(float(l[1]) == 0.0 for l in vl)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
