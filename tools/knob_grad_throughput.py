#!/usr/bin/env python3
"""What the knob gradient costs: backward() against backward_with_knob_grad() (st_model_bwd_knobs: the same pass, plus the per-group stores and one small
reduction) against the exact per-window route knob_grad() (st_model_knob_grad: one forward + backward per window).

One process, one engine per row (scale 1, shrink 4, K = 4, B = 256; f32 and bf16_all).  After one forward(save_for_backward=True) and a warm-up of all three:
`--blocks` ALTERNATING blocks of (1) `--reps` backward() calls, (2) `--reps` backward_with_knob_grad() calls, (3) ONE knob_grad() call; each block is timed
with device events around it, ended by a synchronise.  Reports per-call medians and the block-to-block spread (min .. max), the ratio (2) / (1) with the
spread of (1) beside it, and the largest difference between the two routes' gradients.  Needs a GPU.

    python tools/knob_grad_throughput.py --out profiles/knob_grad_throughput.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from signaltrain_amd import _lib                          # noqa: E402
from signaltrain_amd.engine import StepEngine             # noqa: E402

ROWS = ("f32", "bf16_all")


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps          # ms per call


def measure(dtype, B, blocks, reps, device):
    d = _lib.geometry(1, 4, 4, B)
    eng = StepEngine(d, device, compute_dtype=dtype)
    g = torch.Generator(device="cpu").manual_seed(218)
    for v in eng.named.values():             # xavier-sized random parameters: the kernels' time does not depend on the values, NaNs would
        v.copy_((torch.randn(v.shape, generator=g) * (2.0 / (sum(v.shape) + 1)) ** 0.5).to(device))
    x = (0.3 * torch.randn(B, d.L, generator=g)).to(device)
    kn = (torch.rand(B, d.K, generator=g) - 0.5).to(device)
    gy = (torch.randn(B, d.y, generator=g) / (B * d.y)).to(device)
    assert eng.knob_grad_fused_supported(B)
    fwd = lambda: eng.forward(x, kn, save_for_backward=True)
    plain = lambda: eng.backward(x, kn, gy)
    fused = lambda: eng.backward_with_knob_grad(x, kn, gy)
    slow = lambda: eng.knob_grad(x, kn, gy)
    fwd()
    for _ in range(3):
        plain(); fused()
    k_fused = fused()[1].clone()
    k_slow = slow().clone()                  # warm-up of the per-window route; it leaves the last window's state behind
    fwd()
    torch.cuda.synchronize()
    t = {"bwd": [], "fused": [], "slow": []}
    for _ in range(blocks):
        t["bwd"].append(timed(plain, reps))
        t["fused"].append(timed(fused, reps))
        t["slow"].append(timed(slow, 1))
        fwd()                                # the batch's state back for the next block
        torch.cuda.synchronize()
    diff = float((k_fused - k_slow).abs().max() / k_slow.abs().max())
    del eng
    torch.cuda.empty_cache()
    return t, diff


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=7, help="alternating blocks (at least 5)")
    ap.add_argument("--reps", type=int, default=50, help="calls per timed block of backward() / backward_with_knob_grad()")
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knob_grad_throughput: needs a GPU (a CPU run says nothing about these kernels)")
    if args.blocks < 5:
        raise SystemExit("knob_grad_throughput: at least 5 blocks")
    device = torch.device("cuda:0")
    lines = [f"knob gradient, scale 1 shrink 4 K 4 B {args.batch}: {args.blocks} alternating blocks of {args.reps} x backward(), {args.reps} x backward_with_knob_grad(), "
             f"1 x knob_grad(); device-event ms per call, median (min .. max over blocks)",
             f"{'dtype':9s} | {'(1) backward':>30s} | {'(2) backward_with_knob_grad':>30s} | {'(3) knob_grad, per window':>30s} | (2)/(1)  spread of (1)  (3)/(1) | max |fused - per-window| / max"]
    for dtype in ROWS:
        t, diff = measure(dtype, args.batch, args.blocks, args.reps, device)
        med = {k: statistics.median(v) for k, v in t.items()}
        cell = lambda k: f"{med[k]:9.4f} ({min(t[k]):.4f} .. {max(t[k]):.4f})"
        spread = (max(t["bwd"]) - min(t["bwd"])) / med["bwd"]
        lines.append(f"{dtype:9s} | {cell('bwd'):>30s} | {cell('fused'):>30s} | {cell('slow'):>30s} | {med['fused'] / med['bwd']:7.4f}  {spread:12.4f}  {med['slow'] / med['bwd']:7.1f} | {diff:.2e}")
        print(lines[-1], flush=True)
    txt = "\n".join(lines) + "\n"
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
