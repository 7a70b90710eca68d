"""Long-file inference -- mirror of utils/predict_long.py:30-79 (predict_long).  (The plotting helper calc_ct, :82-99, runs the
CPU effect chunk by chunk and is not part of the accelerated path: it is not mirrored.)

The reference windows the signal on the host (audio.sliding_window, audio.py:23-49), ships every batch of
overlapping windows to the device and appends the outputs on the host.  Here the (zero-padded) signal is uploaded
ONCE; the overlapping windows are a strided device view (`unfold`), each batch goes through the HIP forward
(st_model.forward / StepEngine.forward) and the non-overlapping outputs are written straight into one device buffer.
Same arguments, same return value: a 1-D float32 numpy array of len(signal) - (chunk_size - out_chunk_size) samples
(the first window's lookback has no prediction, exactly as in the reference)."""
import numpy as np
import torch



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


def predict_long(signal, knobs_nn, model, chunk_size, out_chunk_size, sr=44100, effect=None, device=None, compand=False,
                 batch_size=200, verbose=False):
    device = torch.device(device) if device is not None else next(model.parameters()).device
    signal = np.ascontiguousarray(signal, dtype=np.float32)
    if compand:                                                        # predict_long.py:38-40 compands every window; the map is elementwise, so the signal once
        from . import audio
        print("Companding input")
        signal = np.ascontiguousarray(audio.mu_compand(signal), dtype=np.float32)
    overlap = chunk_size - out_chunk_size
    step = chunk_size - overlap                                        # == out_chunk_size
    # zeros at the end until the windows tile the signal
    n = signal.shape[-1]
    x = _windows(signal, chunk_size, step, device)
    nwin = x.shape[0]
    if verbose:
        print("predict_long: chunk_size, out_chunk_size, overlap = ", chunk_size, out_chunk_size, overlap)
        print("predict_long: x.shape, signal.shape = ", tuple(x.shape), signal.shape)
    kn_row = torch.as_tensor(np.asarray(knobs_nn, dtype=np.float32).reshape(1, -1), device=device)
    y_pred = torch.empty(nwin * out_chunk_size, dtype=torch.float32, device=device)
    bs = min(int(batch_size), nwin)
    bmax = max(int(np.round(nwin / bs)), 1)                            # the reference's batching rule (predict_long.py:53)
    with torch.no_grad():
        for b in range(bmax):
            bstart = b * bs
            nb = (nwin - bstart) if b == bmax - 1 else bs              # the last batch takes whatever is left
            xb = x[bstart:bstart + nb].contiguous()
            y_hat = model.forward(xb, kn_row.expand(nb, -1).contiguous())[0]
            y_pred[bstart * out_chunk_size:(bstart + nb) * out_chunk_size] = y_hat.reshape(-1)
    unique = chunk_size + (nwin - 1) * (chunk_size - overlap)          # predict_long.py:72-73
    num_extra = unique - n
    out = y_pred.cpu().numpy()
    return out[0:-num_extra] if num_extra > 0 else out


def fit_knobs(signal, target, model, chunk_size, out_chunk_size, steps=50, lr=0.05, init=None, batch_size=200, compand=False, grad_history=None):
    """The trained model used the other way round: given a recording and its processed version, the ONE knob vector (normalised settings, [-0.5, 0.5])
    for which the model turns `signal` into `target`.  Both are windowed as predict_long windows its input (the target of a window is its last
    out_chunk_size samples); the objective is the mean log-cosh of y_hat - target over all windows, minimised by torch's Adam on the K values, clamped to
    [-0.5, 0.5] after every step.  The gradient of a step is the sum over windows of d / d knobs out of the ONE backward pass per batch
    (StepEngine.backward_with_knob_grad with g_y_hat = tanh(y_hat - target) / n).
    init: start vector (default zeros).  grad_history: a list that receives every step's gradient (numpy [K]).  Returns (knobs_nn [K] float32, loss_history)."""
    device = next(model.parameters()).device
    signal = np.ascontiguousarray(signal, dtype=np.float32); target = np.ascontiguousarray(target, dtype=np.float32)
    assert signal.shape == target.shape and signal.ndim == 1, (signal.shape, target.shape)
    if compand:
        from . import audio
        signal = np.ascontiguousarray(audio.mu_compand(signal), dtype=np.float32); target = np.ascontiguousarray(audio.mu_compand(target), dtype=np.float32)
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
                a = d.abs()
                loss += (a + torch.log1p(torch.exp(-2.0 * a)) - 0.6931471805599453).sum() / n
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
