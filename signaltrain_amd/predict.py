"""Long-file inference -- mirror of utils/predict_long.py:30-79 (predict_long).  (The plotting helper calc_ct, :82-99, runs the
CPU effect chunk by chunk and is not part of the accelerated path: it is not mirrored.)

The reference windows the signal on the host (audio.sliding_window, audio.py:23-49), ships every batch of
overlapping windows to the device and appends the outputs on the host.  Here the (zero-padded) signal is uploaded
ONCE; the overlapping windows are a strided device view (`unfold`), each batch goes through the HIP forward
(st_model.forward / StepEngine.forward) and the non-overlapping outputs are written straight into one device buffer.
Same arguments, same return value: a 1-D float32 numpy array of len(signal) - (chunk_size - out_chunk_size) samples
(the first window's lookback has no prediction, exactly as in the reference).

route="device" runs the same prediction as ONE C call (st_predict_long, StepEngine.predict_long): the signal is uploaded as it is -- no padded copy, no
window or knob copies -- every batch is enqueued by that call, the forward is the one validation takes at the model's compute dtype, and knobs_nn may carry one
row per window.  route="batched" (the default) is the path described above.

predict_sweep renders one recording at several knob settings: the half of the forward in front of the knobs runs once (StepEngine.encode_long), the rest once per
setting (StepEngine.decode_long); fit_knobs(route="device", encode_once=True) fits from the same code."""
import warnings

import numpy as np
import torch

ROUTES = ("batched", "device")
FIT_ROUTES = ("batched", "device")
_warned_unsupported = False
_warned_fit_unsupported = False
_warned_sweep_unsupported = False
_warned_search_unsupported = False


def _nwin(n, chunk_size, out_chunk_size):
    """Windows of a recording of n samples: audio.sliding_window's count (audio.py:42-45) -- one, then one more per started out_chunk_size behind chunk_size."""
    return 1 if n < chunk_size else -(-(n - chunk_size) // out_chunk_size) + 1


def _engine_for(what, model, device, rows, chunk_size, out_chunk_size):
    """The model's engine for batches of `rows` windows on `device`, refused unless its geometry is the caller's chunk sizes."""
    eng = model.engine(torch.empty((), dtype=torch.float32, device=device).expand(rows, chunk_size))      # shape and device only: nothing is read
    if (eng.dims.L, eng.dims.y) != (chunk_size, out_chunk_size):
        raise ValueError(f"{what}: chunk_size / out_chunk_size = {chunk_size} / {out_chunk_size}, the model has {eng.dims.L} / {eng.dims.y}")
    return eng


def _compand(a):
    """audio.mu_compand of a host array, as contiguous float32 (an elementwise map: the whole recording once, where the reference compands every window)."""
    from . import audio
    return np.ascontiguousarray(audio.mu_compand(a), dtype=np.float32)


def _logcosh(d):
    """log cosh(d) elementwise, in the overflow-free form |d| + log1p(exp(-2 |d|)) - log 2: the term of every knob-fit objective."""
    a = d.abs()
    return a + torch.log1p(torch.exp(-2.0 * a)) - 0.6931471805599453


def _windows(signal, chunk_size, step, device):
    """The zero-padded signal on the device and its overlapping windows as a strided view: audio.sliding_window's padding rule (audio.py:42-45)."""
    n = signal.shape[-1]
    if n < chunk_size:
        pad = chunk_size - n
    else:
        rem = (n - chunk_size) % step
        pad = (step - rem) if rem != 0 else 0
    sig = torch.zeros(n + pad, dtype=torch.float32, device=device)
    sig[:n] = torch.from_numpy(signal).to(device)
    return sig.unfold(0, chunk_size, step)                             # [nwin, chunk_size] view, no copy


def _batched_windows(x, knobs_nn, model, out_chunk_size, batch_size):
    """The batched route on the device: x [nwin, chunk_size] (the strided view of _windows) through model.forward batch by batch; returns the
    nwin * out_chunk_size predicted samples as a device tensor (tools/predict_rtf.py times this part on its own)."""
    nwin, device = x.shape[0], x.device
    kn_np = np.asarray(knobs_nn, dtype=np.float32)
    per_window = kn_np.ndim == 2 and nwin > 1 and kn_np.shape[0] == nwin      # one row per window (what route="device" takes, kept through its fallback)
    kn_row = torch.as_tensor(kn_np if per_window else kn_np.reshape(1, -1), device=device)
    y_pred = torch.empty(nwin * out_chunk_size, dtype=torch.float32, device=device)
    bs = min(int(batch_size), nwin)
    bmax = max(int(np.round(nwin / bs)), 1)                            # the reference's batching rule (predict_long.py:53)
    with torch.no_grad():
        for b in range(bmax):
            bstart = b * bs
            nb = (nwin - bstart) if b == bmax - 1 else bs              # the last batch takes whatever is left
            xb = x[bstart:bstart + nb].contiguous()
            kb = kn_row[bstart:bstart + nb] if per_window else kn_row.expand(nb, -1)
            y_hat = model.forward(xb, kb.contiguous())[0]
            y_pred[bstart * out_chunk_size:(bstart + nb) * out_chunk_size] = y_hat.reshape(-1)
    return y_pred


def predict_long(signal, knobs_nn, model, chunk_size, out_chunk_size, sr=44100, effect=None, device=None, compand=False,
                 batch_size=200, verbose=False, route="batched"):
    """signal: a 1-D numpy array, or a 1-D tensor (a device tensor stays on the device with route="device"); knobs_nn: [K] normalised settings, with
    route="device" also [nwin, K], one row per window.  Returns a 1-D float32 numpy array of len(signal) - (chunk_size - out_chunk_size) samples."""
    if route not in ROUTES:
        raise ValueError(f"predict_long: route must be one of {ROUTES}, not {route!r}")
    device = torch.device(device) if device is not None else next(model.parameters()).device
    if route == "device":
        y = _predict_device(signal, knobs_nn, model, chunk_size, out_chunk_size, device, compand, batch_size, verbose)
        if y is not None:
            return y
    if torch.is_tensor(signal):
        pcm16 = signal.dtype == torch.int16                            # 16-bit PCM means s / 32767 on either route
        signal = signal.detach().cpu().numpy()
        if pcm16:
            signal = (signal.astype(np.float64) / 32767.0).astype(np.float32)
    signal = np.ascontiguousarray(signal, dtype=np.float32)
    if compand:                                                        # predict_long.py:38-40 compands every window; the map is elementwise, so the signal once
        print("Companding input")
        signal = _compand(signal)
    overlap = chunk_size - out_chunk_size
    step = chunk_size - overlap                                        # == out_chunk_size
    # zeros at the end until the windows tile the signal
    n = signal.shape[-1]
    x = _windows(signal, chunk_size, step, device)
    nwin = x.shape[0]
    if verbose:
        print("predict_long: chunk_size, out_chunk_size, overlap = ", chunk_size, out_chunk_size, overlap)
        print("predict_long: x.shape, signal.shape = ", tuple(x.shape), signal.shape)
    y_pred = _batched_windows(x, knobs_nn, model, out_chunk_size, batch_size)
    unique = chunk_size + (nwin - 1) * (chunk_size - overlap)          # predict_long.py:72-73
    num_extra = unique - n
    out = y_pred.cpu().numpy()
    return out[0:-num_extra] if num_extra > 0 else out


def _resident(signal, device, compand):
    """The recording on the device for the one-call routes: a tensor stays what it is (16-bit PCM included), a host array goes up as float32."""
    if torch.is_tensor(signal) and not compand:
        sig = signal.detach().to(device)
        return sig if sig.dtype == torch.int16 else sig.float()
    host = signal.detach().cpu().numpy() if torch.is_tensor(signal) else signal
    host = np.ascontiguousarray(host, dtype=np.float32)
    if compand:                                                        # a host map before the upload, as on the batched route
        print("Companding input")
        host = _compand(host)
    return torch.from_numpy(host).to(device)


def _predict_device(signal, knobs_nn, model, chunk_size, out_chunk_size, device, compand, batch_size, verbose):
    """route="device" of predict_long; None where the library does not run this geometry that way (the caller then takes the batched route)."""
    global _warned_unsupported
    n = int(signal.shape[-1])
    nwin = _nwin(n, chunk_size, out_chunk_size)
    bs = max(min(int(batch_size), nwin), 1)
    eng = _engine_for("predict_long", model, device, bs, chunk_size, out_chunk_size)
    if not eng.predict_supported():
        if not _warned_unsupported:
            _warned_unsupported = True
            warnings.warn(f"signaltrain_amd.predict_long: route='device' does not run this geometry (T={eng.dims.T}, OT={eng.dims.OT}: st_predict_supported); "
                          "taking the batched route", RuntimeWarning, stacklevel=3)
        return None
    sig = _resident(signal, device, compand)
    if verbose:
        print("predict_long (device route): chunk_size, out_chunk_size, windows = ", chunk_size, out_chunk_size, nwin)
    kn = torch.as_tensor(np.asarray(knobs_nn, dtype=np.float32), device=device)
    with torch.no_grad():
        y = eng.predict_long(sig.reshape(-1), kn, batch=bs)
    return y.cpu().numpy()


def predict_stream(blocks, knobs, model, chunk_size, out_chunk_size, device=None, batch_size=200):
    """predict_long on audio that arrives block by block: a generator over an iterable of blocks -- numpy arrays or tensors, [m] (one channel) or [C, m]
    (C channels in lockstep), float32 or int16 -- that yields what each block completes (StepEngine.open_stream / PredictStream.push): every output sample as
    soon as its window is whole, possibly none for a block.  The last block of the iterable is pushed as the final one (it also emits the zero-padded last
    window, clipped); every other block needs m % 4 == 0.  Over the iterable the outputs concatenate to predict_long's for the concatenated blocks, len - (chunk_size -
    out_chunk_size) samples per channel.  knobs: [K] or [C, K], or a callable block_index -> knobs evaluated per block (knob automation at block rate).
    A numpy block yields a numpy array, a tensor block a device tensor (no host sync then).  batch_size: most (channel, window) rows per internal batch."""
    device = torch.device(device) if device is not None else next(model.parameters()).device
    eng = _engine_for("predict_stream", model, device, max(int(batch_size), 1), chunk_size, out_chunk_size)
    session, held, index = None, None, 0

    def push(block, final):
        nonlocal session, index
        host = not torch.is_tensor(block)
        t = torch.from_numpy(np.ascontiguousarray(block if np.asarray(block).dtype == np.int16 else np.asarray(block, dtype=np.float32))) if host else block.detach()
        t = t.to(device)
        t = t if t.dtype == torch.int16 else t.float()
        if session is None:
            session = eng.open_stream(1 if t.dim() == 1 else int(t.shape[0]), batch=max(int(batch_size), 1))
        kn = knobs(index) if callable(knobs) else knobs
        index += 1
        with torch.no_grad():
            y = session.push(t, torch.as_tensor(np.asarray(kn, dtype=np.float32), device=device), final=final)
        return y.cpu().numpy() if host else y

    for block in blocks:
        if held is not None:
            yield push(held, False)
        held = block
    if held is not None:
        yield push(held, True)


def predict_sweep(signal, knob_settings, model, chunk_size, out_chunk_size, sr=44100, effect=None, device=None, compand=False,
                  batch_size=200, verbose=False, route="device"):
    """predict_long at S knob settings: knob_settings is [S, K], or [S, nwin, K] for one row per window.  Returns [S, len(signal) - (chunk_size -
    out_chunk_size)] float32.  route="device" encodes the recording ONCE (StepEngine.encode_long: everything in front of the knobs, layer 5 of 9) and decodes it
    at the S settings in one call (StepEngine.decode_long); on a geometry st_decode_supported rejects it warns once and loops over predict_long's batched route,
    which route="batched" does outright.  The parameters must not change between the encode and the decode (they cannot inside this call)."""
    global _warned_sweep_unsupported
    if route not in ROUTES:
        raise ValueError(f"predict_sweep: route must be one of {ROUTES}, not {route!r}")
    kn = np.asarray(knob_settings, dtype=np.float32)
    if kn.ndim not in (2, 3):
        raise ValueError(f"predict_sweep: knob_settings must be [S, K] or [S, nwin, K], not {kn.shape}")
    device = torch.device(device) if device is not None else next(model.parameters()).device
    if route == "device":
        n = int(signal.shape[-1])
        nwin = _nwin(n, chunk_size, out_chunk_size)
        bs = max(min(int(batch_size), nwin), 1)
        eng = _engine_for("predict_sweep", model, device, bs, chunk_size, out_chunk_size)
        if eng.decode_supported():
            sig = _resident(signal, device, compand)
            if verbose:
                print("predict_sweep (device route): chunk_size, out_chunk_size, windows, settings = ", chunk_size, out_chunk_size, nwin, kn.shape[0])
            with torch.no_grad():
                code = eng.encode_long(sig.reshape(-1), batch=bs)
                y = eng.decode_long(code, torch.from_numpy(kn).to(device), batch=bs)
            return np.ascontiguousarray(y.cpu().numpy())
        if not _warned_sweep_unsupported:
            _warned_sweep_unsupported = True
            warnings.warn(f"signaltrain_amd.predict_sweep: route='device' does not run this geometry (T={eng.dims.T}, OT={eng.dims.OT}: st_decode_supported); "
                          "taking the batched route, setting by setting", RuntimeWarning, stacklevel=2)
    return np.stack([predict_long(signal, k, model, chunk_size, out_chunk_size, sr=sr, effect=effect, device=device, compand=compand, batch_size=batch_size,
                                  verbose=verbose) for k in kn])


def fit_knobs(signal, target, model, chunk_size, out_chunk_size, steps=50, lr=0.05, init=None, batch_size=200, compand=False, grad_history=None,
              route="batched", encode_once=False):
    """The trained model used the other way round: given a recording and its processed version, the ONE knob vector (normalised settings, [-0.5, 0.5])
    for which the model turns `signal` into `target`.  Both are windowed as predict_long windows its input (the target of a window is its last
    out_chunk_size samples); the objective is the mean log-cosh of y_hat - target over all windows, minimised by torch's Adam on the K values, clamped to
    [-0.5, 0.5] after every step.  The gradient of a step is the sum over windows of d / d knobs out of the ONE backward pass per batch
    (StepEngine.backward_with_knob_grad with g_y_hat = tanh(y_hat - target) / n).
    init: start vector (default zeros).  grad_history: a list that receives every step's gradient (numpy [K]).  Returns (knobs_nn [K] float32, loss_history).
    route="device" (FIT_ROUTES) runs the whole fit as ONE C call (st_fit_knobs, StepEngine.fit_knobs): the two recordings go to the device once, every batch of
    every step is enqueued by that call and nothing synchronises with the host until the result is read.  It also takes init of shape [nwin, K] -- one knob row
    per window (knob automation; the result is then [nwin, K], grad_history receives [nwin, K] arrays).  Its objective is the mean over the
    len(signal) - (chunk_size - out_chunk_size) output samples the recording really has: positions of the last window behind the recording's end carry no loss
    and no gradient, where the batched route counts its zero-padded tail.  The two objectives coincide when len(signal) = chunk_size + k * out_chunk_size.
    On a geometry st_fit_knobs_supported rejects it warns once and takes the batched route.
    encode_once=True (route="device" only; ValueError otherwise): the recording is encoded once (StepEngine.encode_long) and every step's forward starts at the knobs' layer from that
    code (st_fit_knobs_coded) -- same objective, same steps, results equal up to the order of a few sums."""
    if route not in FIT_ROUTES:
        raise ValueError(f"fit_knobs: route must be one of {FIT_ROUTES}, not {route!r}")
    if encode_once and route != "device":
        raise ValueError(f"fit_knobs: encode_once needs route=\"device\" (route={route!r} runs the whole forward per step)")
    if route == "device":
        res = _fit_device(signal, target, model, chunk_size, out_chunk_size, steps, lr, init, batch_size, compand, grad_history, encode_once)
        if res is not None:
            return res
    device = next(model.parameters()).device
    signal = np.ascontiguousarray(signal, dtype=np.float32); target = np.ascontiguousarray(target, dtype=np.float32)
    assert signal.shape == target.shape and signal.ndim == 1, (signal.shape, target.shape)
    if compand:
        signal, target = _compand(signal), _compand(target)
    x = _windows(signal, chunk_size, out_chunk_size, device)
    t = _windows(target, chunk_size, out_chunk_size, device)[:, chunk_size - out_chunk_size:]
    nwin = x.shape[0]
    K = int(model.num_knobs)
    kn = torch.zeros(K, dtype=torch.float32, device=device) if init is None else \
        torch.as_tensor(np.asarray(init, dtype=np.float32).reshape(K), device=device).clone()
    kn.requires_grad_(True)
    opt = torch.optim.Adam([kn], lr=lr)
    bs = max(min(int(batch_size), nwin), 1)
    eng = model.engine(x[:bs].contiguous())
    n = float(nwin * out_chunk_size)
    history = []
    for _ in range(int(steps)):
        loss = torch.zeros((), dtype=torch.float32, device=device)
        grad = torch.zeros(K, dtype=torch.float32, device=device)
        with torch.no_grad():
            for b0 in range(0, nwin, bs):
                xb, tb = x[b0:b0 + bs].contiguous(), t[b0:b0 + bs]
                kb = kn.detach().reshape(1, K).expand(xb.shape[0], K).contiguous()
                y_hat = eng.forward(xb, kb, save_for_backward=True)[0]
                d = y_hat - tb
                loss += _logcosh(d).sum() / n
                g_y = torch.tanh(d) / n
                grad += eng.backward_with_knob_grad(xb, kb, g_y)[1].sum(0)
        history.append(float(loss.item()))
        if grad_history is not None:
            grad_history.append(grad.cpu().numpy().copy())
        kn.grad = grad
        opt.step()
        with torch.no_grad():
            kn.clamp_(-0.5, 0.5)
    return kn.detach().cpu().numpy(), history


def _logcosh_mean(y, t):
    """mean log cosh(y - t) in float64 on y's device: the objective of fit_knobs on outputs that exist."""
    return float(_logcosh(y.double() - t.double()).mean().item())


def _never_worse(finals, final_losses, starts, start_losses):
    """A fit that ended above its start (Adam overshoots on a short run) gives the start back: a search never returns worse than a candidate it scored."""
    finals, final_losses = np.array(finals, dtype=np.float32), np.array(final_losses, dtype=np.float64)
    worse = final_losses > start_losses
    finals[worse] = starts[worse]
    final_losses[worse] = start_losses[worse]
    return finals, final_losses


def search_knobs(signal, target, model, chunk_size, out_chunk_size, candidates, keep=8, steps=50, lr=0.05, batch_size=200, compand=False, route="device"):
    """A search for the knob vector for which the model turns `signal` into `target`, where one fit from one start is only a local answer (the objective of
    fit_knobs is not convex in the knobs): score every row of candidates [S, K], keep the `keep` lowest, fit those together for `steps` Adam steps and take the
    winner.  Returns (best_knobs [K] float32, best_loss, finals [keep, K] float32, final_losses [keep]): finals in ascending order of the candidates' SCORED loss
    (finals[0] grew from the best-scoring candidate), final_losses the objective at the fitted knobs, best the lowest of them.
    route="device": the recording is encoded ONCE (StepEngine.encode_long), the candidates are scored in one call that keeps only the S losses
    (StepEngine.score_knobs) and the kept ones are fitted in one call (StepEngine.fit_knobs_multi); a short recording fills the batch with (setting, window) rows.
    route="batched", and a geometry st_fit_knobs_supported rejects (after one warning): predict_long and fit_knobs' batched route, candidate by candidate -- the
    objective there counts the zero-padded tail of the last window, as fit_knobs' batched route does."""
    global _warned_search_unsupported
    if route not in FIT_ROUTES:
        raise ValueError(f"search_knobs: route must be one of {FIT_ROUTES}, not {route!r}")
    cand = np.ascontiguousarray(candidates, dtype=np.float32)
    if cand.ndim != 2 or cand.shape[0] < 1:
        raise ValueError(f"search_knobs: candidates must be [S, K] with S >= 1, not {cand.shape}")
    keep = max(min(int(keep), cand.shape[0]), 1)
    device = next(model.parameters()).device
    signal = np.ascontiguousarray(signal, dtype=np.float32); target = np.ascontiguousarray(target, dtype=np.float32)
    assert signal.shape == target.shape and signal.ndim == 1, (signal.shape, target.shape)
    n = int(signal.shape[0])
    nwin = _nwin(n, chunk_size, out_chunk_size)
    if route == "device":
        bs = max(int(batch_size), 1)                                       # not clipped to the window count: a short recording is stacked into the batch
        eng = _engine_for("search_knobs", model, device, min(bs, nwin), chunk_size, out_chunk_size)
        if eng.fit_knobs_supported():
            if compand:
                signal, target = _compand(signal), _compand(target)
            with torch.no_grad():
                sig, tgt = torch.from_numpy(signal).to(device), torch.from_numpy(target).to(device)
                code = eng.encode_long(sig, batch=min(bs, nwin))
                scored = eng.score_knobs(code, tgt, torch.from_numpy(cand).to(device), batch=bs).cpu().numpy()
                order = np.argsort(scored, kind="stable")[:keep]
                finals = eng.fit_knobs_multi(code, tgt, torch.from_numpy(cand[order]).to(device), steps=int(steps), lr=lr, batch=bs)[0]
                final_losses = eng.score_knobs(code, tgt, finals, batch=bs).cpu().numpy()
            finals, final_losses = _never_worse(finals.cpu().numpy(), final_losses, cand[order], scored[order])
            best = int(np.argmin(final_losses))
            return finals[best].copy(), float(final_losses[best]), finals, final_losses
        if not _warned_search_unsupported:
            _warned_search_unsupported = True
            warnings.warn(f"signaltrain_amd.search_knobs: route='device' does not run this geometry (T={eng.dims.T}, OT={eng.dims.OT}, K={eng.dims.K}: "
                          "st_fit_knobs_supported); taking the batched route, candidate by candidate", RuntimeWarning, stacklevel=2)

    def objective(k):          # the batched route's J: over the nwin * out_chunk_size window outputs, the tail behind the recording's end against zeros
        y = predict_long(signal, k, model, chunk_size, out_chunk_size, compand=compand, batch_size=batch_size)
        t = _compand(target) if compand else target
        return _logcosh_mean(torch.from_numpy(np.ascontiguousarray(y)), torch.from_numpy(t[chunk_size - out_chunk_size:][:y.shape[0]]))
    scored = np.array([objective(k) for k in cand])
    order = np.argsort(scored, kind="stable")[:keep]
    finals = np.stack([fit_knobs(signal, target, model, chunk_size, out_chunk_size, steps=steps, lr=lr, init=cand[i], batch_size=batch_size, compand=compand)[0]
                       for i in order]).astype(np.float32)
    finals, final_losses = _never_worse(finals, np.array([objective(k) for k in finals]), cand[order], scored[order])
    best = int(np.argmin(final_losses))
    return finals[best].copy(), float(final_losses[best]), finals, final_losses


def _fit_device(signal, target, model, chunk_size, out_chunk_size, steps, lr, init, batch_size, compand, grad_history, encode_once=False):
    """route="device" of fit_knobs; None where the library does not run this geometry that way (the caller then takes the batched route)."""
    global _warned_fit_unsupported
    device = next(model.parameters()).device
    signal = np.ascontiguousarray(signal, dtype=np.float32); target = np.ascontiguousarray(target, dtype=np.float32)
    assert signal.shape == target.shape and signal.ndim == 1, (signal.shape, target.shape)
    n = int(signal.shape[0])
    nwin = _nwin(n, chunk_size, out_chunk_size)
    bs = max(min(int(batch_size), nwin), 1)
    eng = _engine_for("fit_knobs", model, device, bs, chunk_size, out_chunk_size)
    if not eng.fit_knobs_supported():
        if not _warned_fit_unsupported:
            _warned_fit_unsupported = True
            warnings.warn(f"signaltrain_amd.fit_knobs: route='device' does not run this geometry (T={eng.dims.T}, OT={eng.dims.OT}, K={eng.dims.K}: "
                          "st_fit_knobs_supported); taking the batched route", RuntimeWarning, stacklevel=3)
        return None
    if compand:                                                        # a host map before the upload, as on the batched route
        signal, target = _compand(signal), _compand(target)
    K = int(model.num_knobs)
    kn0 = np.zeros(K, np.float32) if init is None else np.asarray(init, dtype=np.float32)
    kn0 = kn0.reshape(nwin, K) if (kn0.ndim == 2 and kn0.shape[0] == nwin and nwin > 1) else kn0.reshape(K)
    with torch.no_grad():
        sig = torch.from_numpy(signal).to(device)
        code = eng.encode_long(sig, batch=bs) if (encode_once and eng.decode_supported()) else None
        kn, loss, grads, _ = eng.fit_knobs(sig if code is None else code, torch.from_numpy(target).to(device), torch.from_numpy(kn0).to(device),
                                           steps=int(steps), lr=lr, batch=bs, want_grads=grad_history is not None)
    if grad_history is not None:
        g = grads.cpu().numpy()
        grad_history.extend(g[s].reshape(kn0.shape).copy() for s in range(g.shape[0]))
    return kn.cpu().numpy(), [float(v) for v in loss.cpu().numpy()]
