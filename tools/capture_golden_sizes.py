#!/usr/bin/env python3
"""Golden vectors at OTHER (ft, hop, frame) sizes from the *imported reference* (build container only); complements tools/capture_golden*.py.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_sizes.py
Writes (small, committed) and asserts oracle/st_oracle.py against every value:

  tests/golden/g16_other_sizes.npz   the reference's AsymMPAEC built directly (as st_model never builds it) at
                                     (ft, hop, L, T, OT, K) = (64, 24, 528, 25, 9, 3) and (96, 32, 640, 24, 8, 2), B = 2:
                                     the state dict (learned-looking: perturbed bases, non-zero biases), x, knobs, target, the
                                     reference's y_hat, mag, mag_hat, its calc_loss value and its autograd gradients of all 40 tensors

Every other golden is at ft 1024 / hop 384 or a legacy multiple; the dims sweep of the GPU suite (tests/dims_table.py) compares the kernels with the
oracle at sizes away from those, so the oracle itself is pinned to the reference there.  The sizes are small so that whole tensors fit (no
fingerprints): the file stays below 600 KB.  Only data is stored.
"""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _ref_import import import_reference                       # noqa: E402
from oracle import st_oracle as O                                # noqa: E402
from tests.golden_util import perturb_stft                       # noqa: E402

R = import_reference()
nn_proc, loss_functions = R.nn_proc, R.loss_functions
torch.set_num_threads(8)

CASES = {"c64": (64, 24, 528, 25, 9, 3), "c96": (96, 32, 640, 24, 8, 2)}      # (ft, hop, L, T, OT, K)
B = 2


def report(name, a, b, tol):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    err = np.max(np.abs(a - b)) if a.size else 0.0
    scale = max(np.max(np.abs(b)), 1e-30) if b.size else 1.0
    print(f"  {name:44s} max|d|={err:.3e} rel={err/scale:.3e}")
    assert err <= tol * max(scale, 1e-30) + 1e-30, f"oracle mismatch on {name}: {err} vs scale {scale}"


out = {"cases": np.array(list(CASES)), "table": np.array(list(CASES.values()), np.int64), "param_names": np.array(O.param_order())}
for ci, (tag, (N, H, L, T, OT, K)) in enumerate(CASES.items()):
    print(f"G16 {tag}: ft {N} hop {H} L {L} T {T} OT {OT} K {K}")
    assert T == (L + N) // H + 1                                # the reference's Conv1d frame count: its first Linear layer accepts no other
    y = (OT - 1) * H - N
    geo = dict(L=L, out_chunk_intended=y, N=N, H=H, T=T, OT=OT, y=y, F=N // 2 + 1)
    rng = np.random.default_rng(1600 + ci)
    model = nn_proc.AsymMPAEC(T, ft_size=N, hop_size=H, n_knobs=K, output_tf=OT)
    P = O.init_params(geo, K, np.random.default_rng(1700 + ci))
    for k in P:
        if k.endswith(".bias"):
            P[k] = (0.05 * rng.standard_normal(P[k].shape)).astype(np.float32)
    perturb_stft(P, seed=16 + ci)
    for k in O.STFT_KEYS[:2]:
        P[k][geo["F"]:] = 0                                     # rows >= F of the analysis bases are never read (cls_fe_dft.py:55-56 keeps F rows; their gradient is exactly 0,
                                                                # asserted below): zeroed so that the full state dict fits the size budget of a committed fixture
    sd = {k.replace("mpaec.", "", 1): torch.from_numpy(v) for k, v in P.items()}
    assert list(sd) == list(model.state_dict()) and all(tuple(model.state_dict()[k].shape) == tuple(v.shape) for k, v in sd.items())
    with torch.no_grad():
        model.load_state_dict(sd)
    model.train()
    X, Y, KN = O.synth_comp4c_batch(B, L, y, rng)
    if K != 4:
        KN = (rng.beta(0.8, 0.8, size=(B, K)) - 0.5).astype(np.float32)
    Y = (Y * np.float32(1.3)).astype(np.float32)                # a target the model is away from: gradients of ordinary size
    xt, kt, yt = torch.from_numpy(X), torch.from_numpy(KN), torch.from_numpy(Y)
    y_hat, mag, mag_hat = model.forward(xt, kt)
    F = geo["F"]
    assert y_hat.shape == (B, y) and mag.shape == (B, T, F) and mag_hat.shape == (B, OT, F)
    sbf = torch.exp((7. / F) * torch.arange(0., F)).expand_as(mag_hat).float()
    loss = loss_functions.calc_loss(y_hat.float(), yt.float(), mag_hat.float(), scale_by_freq=sbf)
    model.zero_grad(); loss.backward()
    gref = {"mpaec." + k: p.grad.detach().numpy().copy() for k, p in model.named_parameters()}
    assert list(gref) == O.param_order() and len(gref) == 40
    assert all((gref[k][geo["F"]:] == 0).all() for k in O.STFT_KEYS[:2])
    # the oracle against the reference, at the tolerances tests/test_oracle_golden.py applies to G3 / G4
    f = np.float64
    yo, mo, mho = O.model_fwd(X, KN, P, geo)
    report("y_hat", yo, y_hat.detach().numpy(), 3e-6); report("mag", mo, mag.detach().numpy(), 3e-6)
    report("mag_hat", mho, mag_hat.detach().numpy(), 3e-6)
    lo, Go, _ = O.model_loss_bwd(X.astype(f), KN.astype(f), Y.astype(f), P, geo)
    report("loss", lo, loss.item(), 3e-5)
    for k in gref:
        report("grad " + k.replace("mpaec.", ""), Go[k], gref[k], 2e-5)
    out.update({f"{tag}_x": X, f"{tag}_knobs": KN, f"{tag}_y": Y, f"{tag}_y_hat": y_hat.detach().numpy(), f"{tag}_mag": mag.detach().numpy(),
                f"{tag}_mag_hat": mag_hat.detach().numpy(), f"{tag}_loss": np.float64(loss.item())})
    for i, k in enumerate(O.param_order()):                     # short member names (the zip stores each twice): index into `param_names`
        out[f"{tag}_p{i:02d}"] = P[k]; out[f"{tag}_g{i:02d}"] = gref[k]

path = os.path.join(OUT, "g16_other_sizes.npz")
np.savez_compressed(path, **out)
print(f"g16_other_sizes.npz {os.path.getsize(path)/1024:8.1f} KiB")
assert os.path.getsize(path) < 600 * 1000
print("golden capture (other sizes) OK")
