#!/usr/bin/env python3
"""Throughput of the per-epoch validation pass: host side (engine.forward + torch loss + two .item() per batch, train.eval_status_save as it always
was) against the device side (engine.eval_step per batch, one accumulator read per pass; device_eval=True).

One process, one engine per row, one DeviceRecycledDataSet of resident comp_4c validation windows.  Per row: one untimed warm-up pass of each path, then
`--passes` timed samples of each, ALTERNATING host and device, a device synchronise before each clock read; a sample is `--reps` consecutive passes.
Reports the median and the spread (min .. max) of each path in windows/s and the ratio of the medians.  Needs a GPU.

    python tools/eval_throughput.py --out profiles/eval_pass_throughput.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from signaltrain_amd import audio, datasets, nn_proc, train      # noqa: E402

ROWS = [("f32", 256, 1), ("bf16_all", 256, 1), ("f16_all", 64, 8)]       # compute_dtype, batch, scale_factor (L = 8192 x scale)


class _ValLoader:
    def __init__(self, ds, batch):
        self.ds, self.batch = ds, batch

    def __iter__(self):
        return self.ds.batches(self.batch, shuffle=False)


def one_pass(model, engine, loader, device, device_eval, vl_avg=0.0):
    """One validation pass through the driver's own function (no files, no prints: is_main=False)."""
    return train.eval_status_save(model, engine, None, 1, 10 ** 9, 0.0, 0.0, device, loader, "unused.dat", time.time(), 0.98, vl_avg,
                                  "unused.tar", False, None, 0, 0.0, model.out_chunk_size, 44100, 10, cp_every=10 ** 9, is_main=False,
                                  device_eval=device_eval)


def measure(dtype, batch, scale, windows, passes, reps, device):
    torch.manual_seed(218)
    model = nn_proc.st_model(scale_factor=scale, shrink_factor=4, num_knobs=4).to(device)
    model.set_compute_dtype(dtype)
    engine = model.engine(torch.zeros(batch, model.in_chunk_size, device=device))
    ds = datasets.DeviceRecycledDataSet(model.in_chunk_size, audio.Compressor_4c(), datapoints=windows, y_size=model.out_chunk_size, augment=False, device=device)
    loader = _ValLoader(ds, batch)
    n = (windows // batch) * batch * reps
    vals = {False: None, True: None}
    for dev in (False, True):                                   # warm-up, untimed; also the two paths' results side by side
        vals[dev] = one_pass(model, engine, loader, device, dev)
    rates = {False: [], True: []}
    for _ in range(passes):
        for dev in (False, True):
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _r in range(reps):
                one_pass(model, engine, loader, device, dev)
            torch.cuda.synchronize(device)
            rates[dev].append(n / (time.perf_counter() - t0))
    del ds, engine, model
    torch.cuda.empty_cache()
    return rates, vals


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=51200, help="resident validation windows")
    ap.add_argument("--passes", type=int, default=7, help="timed samples of each path (alternating)")
    ap.add_argument("--reps", type=int, default=2, help="validation passes per timed sample")
    ap.add_argument("--rows", default="0,1,2", help="which rows of the table to run")
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_throughput: needs a GPU (a CPU run says nothing about the validation pass)")
    nn_proc._QUIET = True
    device = torch.device("cuda:0")
    lines = [f"validation pass, {args.windows} resident comp_4c windows, {args.passes} alternating samples of {args.reps} passes each, windows/s",
             f"{'dtype':9s} {'B':>4s} {'L':>6s} | {'host median':>12s} {'host min..max':>21s} | {'device median':>13s} {'device min..max':>21s} | {'ratio':>6s} | vl_avg of one pass: host / device"]
    for i in (int(s) for s in args.rows.split(",")):
        dtype, batch, scale = ROWS[i]
        rates, vals = measure(dtype, batch, scale, args.windows, args.passes, args.reps, device)
        h, d = rates[False], rates[True]
        mh, md = statistics.median(h), statistics.median(d)
        lines.append(f"{dtype:9s} {batch:4d} {8192 * scale:6d} | {mh:12.0f} {min(h):10.0f}..{max(h):<10.0f} | {md:13.0f} {min(d):10.0f}..{max(d):<10.0f} | "
                     f"{md / mh:6.2f} | {vals[False]:.6e} / {vals[True]:.6e}")
        print(lines[-1], flush=True)
    txt = "\n".join(lines) + "\n"
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
