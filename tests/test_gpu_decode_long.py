"""GPU: a recording encoded once and decoded at any knob setting -- st_encode_long / st_decode_long / st_fit_knobs_coded, StepEngine.encode_long /
decode_long / fit_knobs(RecordingCode), predict.predict_sweep and predict.fit_knobs(encode_once=True).

The knob-independent half of the forward (staging, analysis GEMM, polar form, encoder layers 1..4) runs once and leaves the recording's code in HBM; every knob
setting and every step of a knob fit then runs ae_dec_fwd_kernel (layers 5..9 + polar epilogue), the frames GEMM and the overlap-add.  Checked against the
float64 oracle run window by window (conditioning asserted on the CPU by tests/test_decode_host.py), against st_predict_long / st_fit_knobs on the same input,
across batch sizes, formats and knob layouts, and for everything it must leave alone.  Shapes, helpers and case tables are those of
tests/test_gpu_predict_long.py, tests/fit_knobs_ref.py and tests/test_gpu_fit_knobs.py."""
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
from tests import test_gpu_fit_knobs as FK
from tests import test_gpu_predict_long as PL
from tests.dims_table import ROWS as DIM_ROWS, geo_of
from tests.test_gpu_predict_long import LEVELS

pytestmark = pytest.mark.gpu

K = D.K
KN = D.KN
B = 4                   # nine windows in batches of four: the last batch is one window whose tail lies behind the recording's end
TOL_16 = 6e-2           # the project's 16-bit bound (tests/fit_knobs_ref.py TOL_GRAD, tests/test_gpu_knob_grad_fused.py TOL)


def rel(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


def sweep(eng, sig, kn, batch=B, enc_batch=None):
    """encode + decode; sig and kn numpy or device tensors."""
    s = G.t(sig) if isinstance(sig, np.ndarray) else sig
    code = eng.encode_long(s, batch=enc_batch or batch)
    return eng.decode_long(code, G.t(kn) if isinstance(kn, np.ndarray) else kn, batch=batch), code


@pytest.mark.parametrize("row", D.ROWS)
def test_fp32_against_the_float64_oracle(row):
    """fp32, three settings in one call (KN, -KN reversed, zeros): each within gpu_checks.TOL of max|ref| of the float64 oracle run window by window; the
    oracle's outputs of any two settings differ by more than 100 TOL of max|ref|, so a decoder that ignored its knobs fails.  n32: one full and one mostly-pad
    group per window; t32_ot16: every output row of every lane live."""
    name = f"settings-{row or 'default'}"
    geo, P, sig, kn = D.case(name)
    ref = D.reference(name)
    eng, _, _ = PL.engine(row, B)
    y, code = sweep(eng, sig, kn)
    assert isinstance(code, RecordingCode) and code.nwin == 9 and code.n == sig.size and code.code.numel() * 4 == int(eng.lib.st_code_bytes(C.byref(eng.dims), sig.size))
    assert y.dtype == torch.float32 and y.is_cuda and tuple(y.shape) == ref.shape == (3, sig.size - (geo["L"] - geo["y"]))
    got = G.n(y)
    for s in range(3):
        e = rel(got[s], ref[s])
        print(f"decode_long vs float64 oracle [{row or 'default'}] setting {s}: rel={e:.2e}")
        assert e <= G.TOL, (row, s, e)
    for i in range(3):
        for j in range(i):
            assert np.abs(ref[i] - ref[j]).max() > 100 * G.TOL * max(np.abs(ref[i]).max(), np.abs(ref[j]).max()), (row, i, j)


@pytest.mark.parametrize("row", ["n384", None])
@pytest.mark.parametrize("level", list(LEVELS))
def test_every_level_against_the_mixed_mode_oracle_and_predict_long(level, row):
    """Every arithmetic level.  Reference: the mixed-mode oracle's output (fit_knobs_ref.objective(..., dtype=float32)[2] under the level's context; at f32 /
    f32x3 the float64 oracle).  Decode is within 6e-2 of max|ref| (f32 / f32x3: gpu_checks.TOL), and within 3 x the deviation st_predict_long -- the parent
    commit's code -- shows from the same reference on the same input: the two round the same computation at the same precision in different summation orders,
    and 3 is the factor tests/gpu_spread.py allows a miss over its spread.  Both deviations and bit-equality are printed."""
    with LEVELS[level]():
        name = f"levels-{row or 'default'}"
        geo, P, sig, _ = D.case(name)
        eng, _, _ = PL.engine(row, B)
        fp = level in ("f32", "f32x3")
        ref = D.reference(name)[0] if fp else R.objective(sig, sig, KN, P, geo, dtype=np.float32, want_grad=False)[2].astype(np.float64)
        y, _ = sweep(eng, sig, KN)
        p = eng.predict_long(G.t(sig), G.t(KN), batch=B)
        assert y.shape == p.shape == ref.shape
        ed, ep = rel(G.n(y), ref), rel(G.n(p), ref)
    print(f"decode_long [{level} {row or 'default'}]: decode {ed:.2e}  predict_long {ep:.2e}  bit-equal={bool(torch.equal(y, p))}")
    assert np.all(np.isfinite(G.n(y))) and ed <= (G.TOL if fp else TOL_16), (level, row, ed)
    assert ed <= 3 * ep, (level, row, ed, ep)


@pytest.mark.parametrize("level", ["f32", "bf16_all"])
def test_batch_independence(level):
    """Decode at 2, 5 and 16 windows per batch agrees to 1e-6 of max|y| (test_gpu_predict_long's bound), and so do a code encoded at batch 2 and one encoded
    at batch 16: the code is window-major."""
    with LEVELS[level]():
        eng, geo, P = PL.engine("n256", 16)
        sig = G.t(PL.signal(PL.length(geo), seed=6))
        kn = G.t(D.SETTINGS[:2])
        c16 = eng.encode_long(sig, batch=16)
        c2 = eng.encode_long(sig, batch=2)
        assert c16.code.shape == c2.code.shape
        ys = {b: G.n(eng.decode_long(c16, kn, batch=b)) for b in (2, 5, 16)}
        y2 = G.n(eng.decode_long(c2, kn, batch=16))
    sc = np.abs(ys[16]).max()
    for name, y in (("batch 2", ys[2]), ("batch 5", ys[5]), ("code of batch 2", y2)):
        e = float(np.abs(y - ys[16]).max() / sc)
        print(f"decode_long {name} vs one batch [{level}]: rel={e:.2e}")
        assert e <= 1e-6, (level, name, e)


@pytest.mark.parametrize("level", ["f32", "bf16_all"])
def test_int16_recording_equals_its_float_image(level):
    """ST_PCM_S16: the int16 recording gives, bit for bit, the code and the output of its float32 image (float)((double)s / 32767.0)."""
    with LEVELS[level]():
        eng, geo, P = PL.engine("n256", B)
        n = PL.length(geo)
        s16 = np.clip(np.round(PL.signal(n, seed=7) * 32767.0 * 2.5), -32768, 32767).astype(np.int16)
        assert s16.min() == -32768 and s16.max() == 32767
        img = (s16.astype(np.float64) / 32767.0).astype(np.float32)
        a, ca = sweep(eng, torch.from_numpy(s16).to(G.DEV), D.SETTINGS)
        b, cb = sweep(eng, G.t(img), D.SETTINGS)
    assert ca.signal.dtype == torch.int16 and torch.equal(ca.code, cb.code) and a.shape == b.shape and torch.equal(a, b)
    assert float(b.abs().max()) > 0.1 and bool(torch.isfinite(ca.code).all())


def test_knob_automation():
    """[S, nwin, K]: one row per window (two settings alternating, and the other way round) against the oracle with the same rows at gpu_checks.TOL; [K],
    [1, K] and that row repeated over the windows give equal bits (a row stride of 0 and of K read the same values)."""
    geo, P, sig, both = D.case("automation")
    eng, _, _ = PL.engine("n256", B)
    nwin = D.NWIN
    refs = D.reference("automation")
    code = eng.encode_long(G.t(sig), batch=B)
    got = G.n(eng.decode_long(code, G.t(both), batch=B))
    one = PL.oracle(sig, KN, P, geo)
    for s in range(2):
        ref = refs[s]
        e = rel(got[s], ref)
        print(f"decode_long knob automation setting {s}: rel={e:.2e}")
        assert e <= G.TOL, (s, e)
        assert np.abs(ref - one).max() > 100 * G.TOL * np.abs(one).max()          # the rows were really taken per window
    a = eng.decode_long(code, G.t(KN), batch=B)
    assert a.dim() == 1
    b = eng.decode_long(code, G.t(KN[None, :]), batch=B)
    c = eng.decode_long(code, G.t(np.broadcast_to(KN, (1, nwin, K)).copy()), batch=B)
    assert tuple(b.shape) == tuple(c.shape) == (1, a.numel()) and torch.equal(a, b[0]) and torch.equal(a, c[0])
    with pytest.raises(ValueError, match="rows"):
        eng.decode_long(code, G.t(both[:, :nwin - 1].copy()), batch=B)


def test_second_trip_of_the_persistent_loop():
    """Default geometry, one batch of the smallest size at which B * 33 groups exceed CUs x 2 x 8 waves (B = 125 on the MI355X's 256 CUs, which the case table
    is laid out for): the prefetch of the next group is live.  Same reference, same bound.  The recording's seed is 10, not test_gpu_fit_knobs' 9: at 9
    st_predict_long itself misses TOL at one sample ("Encode once"), so the test first asserts that st_predict_long in batches of four -- the
    existing route, no second trip anywhere -- is within TOL on this recording."""
    geo, P, sig, _ = D.case("second_trip")
    nb = D.second_trip_batch(torch.cuda.get_device_properties(0).multi_processor_count, geo)
    assert PL.windows(sig, geo).shape[0] == nb, "the case table is laid out for the MI355X's 256 CUs"
    eng, _, _ = PL.engine(None, nb)
    ref = D.reference("second_trip")[0]
    p = eng.predict_long(G.t(sig), G.t(KN), batch=4)
    ep = rel(G.n(p), ref)
    assert ep <= G.TOL, ("the recording is no yardstick at TOL: st_predict_long in batches of four", ep)
    y, _ = sweep(eng, sig, KN, batch=nb)
    e = rel(G.n(y), ref)
    print(f"decode_long second trip: B={nb} groups={nb * (int(_lib.load().st_kp(geo['F'])) // 32)} rel={e:.2e} (st_predict_long at batch 4: {ep:.2e}, "
          f"bit-equal={bool(torch.equal(y, p))})")
    assert e <= G.TOL and e <= 3 * ep, (nb, e, ep)


def test_guards():
    """Nothing outside [0, n_out) of a row of out is written (NaN pre-fill, a pitch larger than n_out, n_out % 4 != 0), nothing at or past signal + n is read
    (NaN there), the code, parameters, moments and gradients are bit-unchanged by decode, and two identical calls with the workspace NaN-filled in between
    give equal bits."""
    eng, geo, P = PL.engine("n256", B)
    n = PL.length(geo)
    n_out = n - (geo["L"] - geo["y"])
    assert n_out % 4 != 0 and n % 4 != 0
    sig = PL.signal(n, seed=9)
    for name in ("grads", "m", "v"):
        getattr(eng, name).copy_(torch.randn_like(eng.params))
    before = {k: getattr(eng, k).clone() for k in ("params", "grads", "m", "v", "scalars", "ws")}
    kn = G.t(D.SETTINGS)
    code = eng.encode_long(G.t(sig), batch=B)
    kept = code.code.clone()
    plain = eng.decode_long(code, kn, batch=B)
    eng._decode_ws.view(torch.float32).fill_(float("nan"))
    again = eng.decode_long(code, kn, batch=B)
    assert bool(torch.isfinite(plain).all()) and torch.equal(plain, again)
    PAD = 64
    pitch = (n_out + 3) // 4 * 4 + 8
    buf = torch.full((PAD + 3 * pitch + PAD,), float("nan"), dtype=torch.float32, device=G.DEV)
    view = buf[PAD:PAD + 3 * pitch].view(3, pitch)
    got = eng.decode_long(code, kn, out=view, batch=B)
    assert got.data_ptr() == view.data_ptr() and tuple(got.shape) == (3, n_out) and torch.equal(got, plain)
    assert bool(torch.isnan(view[:, n_out:]).all()) and bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + 3 * pitch:]).all())
    for dtype, host in ((torch.float32, sig), (torch.int16, np.round(sig * 20000).astype(np.int16))):
        clean, _ = sweep(eng, torch.from_numpy(host).to(G.DEV), kn)
        if dtype == torch.float32:
            sbuf = torch.full((PAD + n + PAD,), float("nan"), dtype=dtype, device=G.DEV)
        else:
            sbuf = torch.full((PAD + n + PAD,), 32767, dtype=dtype, device=G.DEV)      # int16 has no NaN: full scale where zeros are due
        sbuf[PAD:PAD + n] = torch.from_numpy(host).to(G.DEV)
        emb, _ = sweep(eng, sbuf[PAD:PAD + n], kn)
        assert bool(torch.isfinite(emb).all()) and torch.equal(emb, clean), dtype
    assert torch.equal(code.code, kept)
    for k, v in before.items():
        assert torch.equal(getattr(eng, k), v), k


# ---------------------------------------------------------------------------------------------- the coded fit
def coded_step(eng, sig, tgt, kn, batch=B):
    """steps = 1, lr = 0 from the code: the loss and the gradient at kn."""
    code = eng.encode_long(G.t(sig) if isinstance(sig, np.ndarray) else sig, batch=batch)
    return FK.one_step(eng, code, tgt, kn, batch=batch)


@pytest.mark.parametrize("per_window", [False, True], ids=["one_row", "row_per_window"])
@pytest.mark.parametrize("row", R.ROWS)
def test_coded_fit_gradient_and_loss_against_the_float64_reference(row, per_window):
    """steps = 1, lr = 0, fp32, from the code: the gradient within TOL_GRAD["f32"] of max|ref| and J within gpu_checks.TOL of the float64 reference of
    tests/fit_knobs_ref.py -- the bounds st_fit_knobs meets -- for one knob row and for one row per window."""
    eng, geo, P = FK.engine(row)
    sig, tgt = R.pair(row)
    kn = FK.knob_rows(9) if per_window else R.KN
    J, g = FK.reference(row, per_window)
    loss, grad, k = coded_step(eng, sig, tgt, kn)
    assert grad.shape == g.shape and torch.equal(k.reshape(-1), G.t(kn).reshape(-1))
    eg, eJ = float(np.abs(grad - g).max() / np.abs(g).max()), abs(loss - J) / abs(J)
    print(f"coded fit vs float64 reference [{row or 'default'} {'per window' if per_window else 'one row'}]: grad {eg:.2e}  J {eJ:.2e}")
    assert eg <= R.TOL_GRAD["f32"], (row, eg, grad, g)
    assert eJ <= G.TOL, (row, eJ, loss, J)


@pytest.mark.parametrize("row", ["n256", None])
@pytest.mark.parametrize("level", list(LEVELS))
def test_coded_fit_every_level_against_the_existing_route(level, row):
    """All six levels against forward(save_for_backward=True) + backward_with_knob_grad on the same windows materialised on the host, the reference
    test_gpu_fit_knobs.test_every_level_against_the_existing_route forms: TOL_GRAD[level] of max|ref|."""
    with LEVELS[level]():
        eng, geo, P = FK.engine(row)
        sig, tgt = R.pair(row)
        L, y = geo["L"], geo["y"]
        n_out = sig.size - (L - y)
        xw = R.windows(sig, geo); tw = R.windows(tgt, geo)[:, L - y:]
        nwin = xw.shape[0]
        valid = G.t((np.arange(nwin * y) < n_out).reshape(nwin, y).astype(np.float32))
        ref = torch.zeros(K, dtype=torch.float64, device=G.DEV)
        for b0 in range(0, nwin, B):
            xb, tb = G.t(xw[b0:b0 + B]), G.t(tw[b0:b0 + B])
            kb = G.t(np.tile(R.KN, (xb.shape[0], 1)))
            y_hat = eng.forward(xb, kb, save_for_backward=True)[0]
            g_y = (torch.tanh(y_hat - tb) * valid[b0:b0 + B] / float(n_out)).contiguous()
            ref += eng.backward_with_knob_grad(xb, kb, g_y)[1].double().sum(0)
        ref = ref.cpu().numpy()
        _, grad, _ = coded_step(eng, sig, tgt, R.KN)
    e = float(np.abs(grad[0] - ref).max() / np.abs(ref).max())
    print(f"coded fit vs backward_with_knob_grad [{level} {row or 'default'}]: {e:.2e} (tol {R.TOL_GRAD[level]:.0e})")
    assert np.all(np.isfinite(grad)) and e <= R.TOL_GRAD[level], (level, row, e, grad, ref)


@pytest.mark.parametrize("per_window", [False, True], ids=["one_row", "row_per_window"])
@pytest.mark.parametrize("level", ["f32", "bf16_all"])
def test_coded_chained_single_steps_are_one_call_bit_for_bit(level, per_window):
    with LEVELS[level]():
        eng, geo, P = FK.engine("n256")
        sig, tgt = (G.t(a) for a in R.pair("n256"))
        code = eng.encode_long(sig, batch=B)
        k0 = G.t(FK.knob_rows(9) if per_window else R.KN)
        kA, lA, gA, (mA, vA, nA) = eng.fit_knobs(code, tgt, k0, steps=3, batch=B, want_grads=True)
        k, st, ls, gs = k0, None, [], []
        for _ in range(3):
            k, l, g, st = eng.fit_knobs(code, tgt, k, steps=1, batch=B, want_grads=True, state=st)
            ls.append(l); gs.append(g)
    assert nA == st[2] == 4
    assert torch.equal(kA, k) and torch.equal(mA, st[0]) and torch.equal(vA, st[1])
    assert torch.equal(lA, torch.cat(ls)) and torch.equal(gA, torch.cat(gs))
    assert not torch.equal(kA, k0) and float(lA[2]) != float(lA[0])


def _adam_bound(k0, gh, lr=0.05):
    """test_gpu_fit_knobs.test_adam_tail_against_the_float64_replay's bound: 4 x the deviation torch's own float32 CPU Adam shows from the float64 replay on the
    same gradient history, or one unit 2^-24 of the knob scale 0.5 where that is smaller.  Returns (replayed knobs, bound, torch float32's deviation)."""
    want, _, _ = R.adam_replay(k0, gh, lr=lr)
    p = torch.tensor(k0, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    for g in gh:
        p.grad = torch.tensor(g.astype(np.float32))
        opt.step()
        with torch.no_grad():
            p.clamp_(-0.5, 0.5)
    yard = float(np.abs(p.detach().numpy().astype(np.float64) - want).max())
    return want, max(4 * yard, 0.5 * 2.0 ** -24), yard


@pytest.mark.parametrize("per_window", [False, True], ids=["one_row", "row_per_window"])
def test_coded_three_steps_against_the_float64_adam_replay(per_window):
    """The knobs after three coded steps against the float64 replay of Adam + clamp on the returned grad_hist, at the bound test_gpu_fit_knobs.py applies to
    st_fit_knobs.  One knob starts at 0.499 with a gradient that pushes it out: the clamp acts."""
    eng, geo, P = FK.engine("n256")
    sig, tgt = (G.t(a) for a in R.pair("n256"))
    code = eng.encode_long(sig, batch=B)
    k0 = (FK.knob_rows(9) if per_window else R.KN.copy()).astype(np.float32).reshape(-1, K)
    probe = FK.one_step(eng, code, tgt, k0 if per_window else R.KN)[1]
    j = int(np.argmax(np.abs(probe).min(0)))
    k0[:, j] = -0.499 * np.sign(probe[:, j])
    k0 = k0.reshape((9, K) if per_window else (K,))
    k, loss, grads, (m, v, nxt) = eng.fit_knobs(code, tgt, G.t(k0), steps=3, lr=0.05, batch=B, want_grads=True)
    gh = G.n(grads).reshape((3,) + k0.shape)
    want, bound, yard = _adam_bound(k0, gh)
    dev = float(np.abs(G.n(k).reshape(k0.shape) - want).max())
    print(f"coded fit Adam tail [{'per window' if per_window else 'one row'}]: device {dev:.3e}  torch float32 {yard:.3e}  bound {bound:.3e}")
    assert nxt == 4 and np.abs(want).max() == 0.5 and np.array_equal(np.abs(G.n(k).reshape(k0.shape)) == 0.5, np.abs(want) == 0.5)
    assert dev <= bound, (dev, yard, bound)


def test_coded_fit_leaves_the_code_and_the_engine_alone():
    eng, geo, P = FK.engine("n256")
    sig, tgt = (G.t(a) for a in R.pair("n256"))
    code = eng.encode_long(sig, batch=B)
    eng.grads.normal_(); eng.ws.random_(0, 255)
    before = [t.clone() for t in (eng.params, eng.grads, eng.ws, code.code, eng._decode_ws)]
    a = eng.fit_knobs(code, tgt, G.t(R.KN), steps=2, batch=B, want_grads=True)
    eng._fit_ws.view(torch.float32).fill_(float("nan"))
    b = eng.fit_knobs(code, tgt, G.t(R.KN), steps=2, batch=B, want_grads=True)
    for x, y in zip(a[:3] + a[3][:2], b[:3] + b[3][:2]):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    for x, y in zip(before, (eng.params, eng.grads, eng.ws, code.code, eng._decode_ws)):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------- the Python route
def test_predict_sweep_against_the_batched_route():
    """predict.predict_sweep (encode once, decode S times) against a loop of predict.predict_long(route="batched") at gpu_checks.TOL of max|ref|; and against
    the oracle at the same bound."""
    from signaltrain_amd import predict
    m, _, _ = PL._model()
    geo, P, sig, kn = D.case("sweep")
    ref = D.reference("sweep")
    L, y, n = geo["L"], geo["y"], sig.size
    got = predict.predict_sweep(sig, kn, m, L, y, batch_size=3)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (3, n - (L - y))
    for s in range(3):
        batched = predict.predict_long(sig, kn[s], m, L, y, batch_size=3)
        sc = np.abs(ref[s]).max()
        print(f"predict_sweep setting {s}: sweep-batched={np.abs(got[s] - batched).max() / sc:.2e} sweep-oracle={np.abs(got[s] - ref[s]).max() / sc:.2e}")
        assert np.abs(got[s] - batched).max() <= G.TOL * sc and np.abs(got[s] - ref[s]).max() <= G.TOL * sc
    assert np.array_equal(predict.predict_sweep(torch.from_numpy(sig).to(G.DEV), kn, m, L, y, batch_size=3), got)
    loop = predict.predict_sweep(sig, kn[:2], m, L, y, batch_size=3, route="batched")
    assert loop.shape == (2, n - (L - y)) and np.array_equal(loop[1], predict.predict_long(sig, kn[1], m, L, y, batch_size=3))


def test_fit_knobs_encode_once_returns_what_the_plain_device_route_returns():
    """predict.fit_knobs(route="device", encode_once=True) against encode_once=False, three steps at lr = 0.05: the knobs agree within the trajectory bound of
    test_coded_three_steps_against_the_float64_adam_replay (4 x torch's float32 Adam's deviation from the float64 replay on the plain route's gradient
    history, or 2^-24 of the knob scale), each run's knobs follow the replay of its own history within it, and the losses agree within gpu_checks.TOL relative.
    The gradient histories' difference is printed.  encode_once without route="device" is refused."""
    from signaltrain_amd import predict
    m, _, _ = PL._model()
    geo, P, sig, _ = D.case("sweep")
    L, y = geo["L"], geo["y"]
    tgt = R.target_of(sig)
    steps, lr = 3, 0.05
    ga, gb = [], []
    ka, ha = predict.fit_knobs(sig, tgt, m, L, y, steps=steps, lr=lr, batch_size=3, grad_history=ga, route="device", encode_once=True)
    kb, hb = predict.fit_knobs(sig, tgt, m, L, y, steps=steps, lr=lr, batch_size=3, grad_history=gb, route="device")
    assert ka.shape == kb.shape == (K,) and len(ha) == len(hb) == steps
    bound = None
    for k, g in ((ka, ga), (kb, gb)):
        want, bound, _ = _adam_bound(np.zeros(K, np.float32), np.stack(g), lr=lr)
        assert np.abs(k - want).max() <= bound
    eg = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(ga, gb))
    eJ = max(abs(a - b) / abs(b) for a, b in zip(ha, hb))
    ek = float(np.abs(ka - kb).max())
    print(f"fit_knobs encode_once vs plain device route: grad {eg:.2e}  J {eJ:.2e}  knobs {ek:.2e} (trajectory bound {bound:.2e})  bit-equal={np.array_equal(ka, kb)}")
    assert ek <= bound and eJ <= G.TOL, (ek, bound, eJ)
    with pytest.raises(ValueError, match="encode_once"):
        predict.fit_knobs(sig, tgt, m, L, y, steps=1, encode_once=True)


def _wide_model(row="t33_ot17"):
    """An st_model with the autoencoder pair of a dims-table row in place of its own (the module route of tests/test_gpu_dims_sweep.py)."""
    from signaltrain_amd import nn_proc
    nn_proc._QUIET = True
    torch.manual_seed(3)
    N, H, L, T, OT = DIM_ROWS[row]
    m = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=K)
    m.mpaec = nn_proc.AsymMPAEC(T, ft_size=N, hop_size=H, n_knobs=K, output_tf=OT)
    m.in_chunk_size, m.out_chunk_size = L, geo_of(row)["y"]
    return m.to(G.DEV), geo_of(row)


def test_wide_geometry_falls_back_with_one_warning():
    """t33_ot17, the first wide geometry: predict_sweep(route="device") warns once and returns what the loop of the batched route returns."""
    from signaltrain_amd import predict
    m, geo = _wide_model()
    L, y = geo["L"], geo["y"]
    d = G.dims_of(geo, 1, K)
    assert not _lib.load().st_decode_supported(C.byref(d))
    sig = PL.signal(L + y + 5, seed=12)
    predict._warned_sweep_unsupported = False
    with pytest.warns(RuntimeWarning, match="batched route"):
        a = predict.predict_sweep(sig, D.SETTINGS[:2], m, L, y, batch_size=2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b = predict.predict_sweep(sig, D.SETTINGS[:2], m, L, y, batch_size=2)          # the second time: no warning
    c = np.stack([predict.predict_long(sig, k, m, L, y, batch_size=2) for k in D.SETTINGS[:2]])
    assert a.shape == (2, sig.size - (L - y)) and np.array_equal(a, c) and np.array_equal(b, c)


def test_a_stale_recording_code_raises():
    """A RecordingCode from another geometry, length, device or compute dtype raises ValueError."""
    eng, geo, P = PL.engine("n256", B)
    other, geo2, _ = PL.engine("ragged", B)
    sig = G.t(PL.signal(PL.length(geo), seed=13))
    code = eng.encode_long(sig, batch=B)
    with pytest.raises(ValueError, match="geometry"):
        other.decode_long(code, G.t(KN))
    with pytest.raises(ValueError, match="geometry"):
        other.fit_knobs(code, sig, G.t(KN), steps=1)
    with G.mixed_mode(2, half="bf16"):
        half, _, _ = PL.engine("n256", B)
        assert half.compute_dtype != eng.compute_dtype
        with pytest.raises(ValueError, match="compute dtype"):
            half.decode_long(code, G.t(KN))
    for bad in (RecordingCode(code.code, sig[:-4], code.n, code.nwin, code.geometry, code.compute_dtype),              # the signal is not the n samples it was built from
                RecordingCode(code.code, sig[:-geo["y"]], code.n - geo["y"], code.nwin - 1, code.geometry, code.compute_dtype),   # a shorter recording's signal, this code
                RecordingCode(code.code[:-16], sig, code.n, code.nwin, code.geometry, code.compute_dtype)):            # a truncated code
        with pytest.raises(ValueError, match="samples|bytes"):
            eng.decode_long(bad, G.t(KN))
        with pytest.raises(ValueError, match="samples|bytes"):
            eng.fit_knobs(bad, sig, G.t(KN), steps=1)
    with pytest.raises(ValueError, match="lives on"):
        eng.decode_long(RecordingCode(code.code.cpu(), code.signal, code.n, code.nwin, code.geometry, code.compute_dtype), G.t(KN))
    with pytest.raises(ValueError, match="RecordingCode"):
        eng.decode_long(code.code, G.t(KN))


def test_training_trajectory_is_untouched():
    """A train step before and one after an encode + decode + coded fit: the trajectory of the two train steps alone, bit for bit."""
    geo, P = PL.case("n256")
    _, X, Y, KNB, _ = G.make_case(3, 21, K=K, geo=geo_of("n256"))
    a = G.new_engine(G.dims_of(geo, 3, K)); a.load_state_dict(P)
    b = G.new_engine(G.dims_of(geo, 3, K)); b.load_state_dict(P)
    sig = G.t(PL.signal(PL.length(geo), seed=10))
    for i in range(2):
        a.train_step(G.t(X), G.t(KNB), G.t(Y), 1e-3)
        b.train_step(G.t(X), G.t(KNB), G.t(Y), 1e-3)
        if i == 0:
            code = a.encode_long(sig)
            a.decode_long(code, G.t(D.SETTINGS))
            a.fit_knobs(code, sig, G.t(KN), steps=1)
    for k in ("params", "m", "v", "grads", "scalars"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.step_count == b.step_count == 2
