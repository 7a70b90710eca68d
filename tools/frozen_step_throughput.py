#!/usr/bin/env python3
"""What a train step with frozen parameter groups costs: st_train_step against st_train_step_groups at the masks 15 (nothing frozen), 12 (front end
frozen), 14 (analysis frozen) and 13 (synthesis frozen).

One process, one engine per arithmetic (scale 1, shrink 4, K = 4, B = 256; f32 and bf16_all).  After a warm-up of all five variants: `--blocks`
ALTERNATING blocks of `--reps` calls of each variant, each block timed with device events around it and ended by a synchronise.  The step numbers passed
are those of a run that has trained every group throughout (all four equal and rising), so the figures are those of the steady state.  Reports ms per
step as the median over blocks with the block-to-block spread (min .. max), each variant's saving against st_train_step of the same run, and -- from
separate, untimed passes under st_profile_enable -- the per-kernel lines of st_profile_report for the full step and for each mask, with the sum of the
full step's kernels that a mask does not launch set beside that mask's saving.  Needs a GPU.

    python tools/frozen_step_throughput.py --out profiles/frozen_step_throughput.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from signaltrain_amd import _lib, nn_proc                 # noqa: E402
from signaltrain_amd.engine import StepEngine             # noqa: E402

ROWS = ("f32", "bf16_all")
MASKS = (15, 12, 14, 13)
LR = 1e-4


class Bench:
    def __init__(self, dtype, B, device):
        d = _lib.geometry(1, 4, 4, B)
        nn_proc._QUIET = True
        torch.manual_seed(218)
        self.model = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=4).to(device)      # the model's own initialisation: DFT bases, xavier autoencoders
        self.model.set_compute_dtype(dtype)
        self.eng = eng = self.model.engine(torch.zeros(B, d.L, device=device))
        assert isinstance(eng, StepEngine)
        self.d = eng._dims(B)
        g = torch.Generator(device="cpu").manual_seed(218)
        self.x = (0.3 * torch.randn(B, d.L, generator=g)).to(device)
        self.kn = (torch.rand(B, d.K, generator=g) - 0.5).to(device)
        self.y = (0.3 * torch.randn(B, d.y, generator=g)).to(device)
        self.step = 0
        self.stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def call(self, mask):
        """mask None: st_train_step; else st_train_step_groups with that mask (four equal step numbers)."""
        e = self.eng
        self.step += 1
        head = (C.byref(self.d), _lib.ptr(e.params), _lib.ptr(e.grads), _lib.ptr(e.m), _lib.ptr(e.v), _lib.ptr(self.x), _lib.ptr(self.kn), _lib.ptr(self.y),
                _lib.ptr(e.ws), _lib.ptr(e.scalars), LR, 0.9, 0.999, 1e-8)
        if mask is None:
            rc = e.lib.st_train_step(*head, self.step, self.stream)
        else:
            rc = e.lib.st_train_step_groups(*head, (C.c_int * 4)(*([self.step] * 4)), mask, self.stream)
        _lib.check(rc, "st_train_step" if mask is None else "st_train_step_groups")

    def timed(self, mask, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            self.call(mask)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    def profile(self, mask, reps):
        """{kernel name: us per step} of `reps` steps under the library's event profiler (every launch followed by an event: not a timing of the step)."""
        lib = self.eng.lib
        _lib.check(lib.st_profile_enable(1), "st_profile_enable")
        try:
            for _ in range(reps):
                self.call(mask)
            torch.cuda.synchronize()
            buf = C.create_string_buffer(1 << 14)
            _lib.check(lib.st_profile_report(buf, len(buf)), "st_profile_report")
        finally:
            lib.st_profile_enable(0)
        out = {}
        for ln in buf.value.decode().splitlines():
            name, ms, cnt = ln.split()
            out[name] = 1e3 * float(ms) / reps
        return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=7, help="alternating blocks (at least 5)")
    ap.add_argument("--reps", type=int, default=200, help="steps per timed block")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frozen_step_throughput: needs a GPU (a CPU run says nothing about these kernels)")
    if args.blocks < 5:
        raise SystemExit("frozen_step_throughput: at least 5 blocks")
    device = torch.device("cuda:0")
    variants = [None] + list(MASKS)
    label = lambda m: "st_train_step" if m is None else f"groups mask {m}"
    lines = [f"train step with frozen groups, scale 1 shrink 4 K 4 B {args.batch}: {args.blocks} alternating blocks of {args.reps} steps per variant; "
             f"device-event ms per step, median (min .. max over blocks); saving = against st_train_step of the same run"]
    for dtype in ROWS:
        b = Bench(dtype, args.batch, device)
        for m in variants:
            for _ in range(5):
                b.call(m)
        torch.cuda.synchronize()
        t = {m: [] for m in variants}
        for _ in range(args.blocks):
            for m in variants:
                t[m].append(b.timed(m, args.reps))
        med = {m: statistics.median(v) for m, v in t.items()}
        base = med[None]
        spread = (max(t[None]) - min(t[None])) / base
        lines.append(f"\n== {dtype}   (block-to-block spread of st_train_step: {100 * spread:.2f} % of its median)")
        for m in variants:
            lines.append(f"{label(m):16s} | {med[m]:8.4f} ms ({min(t[m]):.4f} .. {max(t[m]):.4f}) | saving {1e3 * (base - med[m]):8.1f} us  {100 * (base - med[m]) / base:6.2f} %")
        prof = {m: b.profile(m, 20) for m in variants}
        full = prof[None]
        for m in MASKS[1:]:
            gone = {k: v for k, v in full.items() if k not in prof[m]}
            came = {k: v for k, v in prof[m].items() if k not in full}
            lines.append(f"mask {m}: kernels of the full step it does not launch: " + ", ".join(f"{k} {v:.1f}" for k, v in gone.items()) +
                         f" = {sum(gone.values()):.1f} us; launched under another name instead: " + (", ".join(f"{k} {v:.1f}" for k, v in came.items()) or "none") +
                         f" = {sum(came.values()):.1f} us; net {sum(gone.values()) - sum(came.values()):.1f} us against a measured saving of {1e3 * (base - med[m]):.1f} us")
        names = list(full) + [k for m in MASKS for k in prof[m] if k not in full]
        names = list(dict.fromkeys(names))
        lines.append("per-kernel us per step (st_profile_report; '-' = not launched):")
        lines.append(f"{'kernel':26s}" + "".join(f"{label(m):>18s}" for m in variants))
        for k in names:
            lines.append(f"{k:26s}" + "".join(f"{prof[m][k]:18.1f}" if k in prof[m] else f"{'-':>18s}" for m in variants))
        lines.append(f"{'sum':26s}" + "".join(f"{sum(prof[m].values()):18.1f}" for m in variants))
        sc = b.eng.scalars.tolist()
        if not (sc[0] == sc[0] and abs(sc[0]) < 1e30) or sc[5] != 0:
            raise SystemExit(f"frozen_step_throughput: the run went non-finite (loss {sc[0]}, {sc[5]} steps skipped on overflow): its steps are not the steps of a training run")
        lines.append(f"after {b.step} steps: loss {sc[0]:.4e}, steps skipped on overflow {int(sc[5])}")
        print("\n".join(lines[-(len(names) + 13):]), flush=True)
        del b
        torch.cuda.empty_cache()
    txt = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt)
        print(f"written: {args.out}")


if __name__ == "__main__":
    main()
