#!/usr/bin/env python3
"""CLI mirror of the reference's gen_dataset.py (flags of gen_dataset.py:253-259) on the MI355X-native library: pre-generates input / target wav pairs with
the knob setting of each target in its file name, every file rendered whole through the effect (one st_render_pool call per group of files with --device cuda)."""
import argparse

if __name__ == "__main__":
    p = argparse.ArgumentParser(description="Generate a dataset of input / target pairs. With --sp, Train has knob values equally spaced; everything else is random. "
                                            "Every random choice (clips, signal families, knob settings) follows ONE numpy Generator seeded with --seed, not the "
                                            "reference's per-process global generators: the same seed gives the same dataset whatever the machine.",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('name', help='directory of the dataset to write (created if missing)')
    p.add_argument('-d', '--dur', type=float, help='length of every file in seconds (synthesised files: rounded up to whole 4096-sample clips)', default=5)
    p.add_argument('--sp', type=int, help='settings per knob: Train/ then covers the grid of sp ** K settings and -n is not read', default=None)
    p.add_argument('-n', '--num', type=int, help='number of file pairs to write (not read with --sp)', default=20000)
    p.add_argument('-e', '--effect', help='effect to render: comp_4c | comp | comp_t | comp_4c_large | comp_one | lowpass | denoise | echo | decomp_4c', default="comp_4c")
    p.add_argument('--inpath', help='directory of recorded input (*.wav and */*.wav, names without "target"), already split into Train/ Val/ [Test/]; default: synthesised test signals', default=None)
    p.add_argument('--sr', type=int, help='sample rate in Hz', default=44100)
    p.add_argument('--seed', type=int, help='Seed of the one random stream of the run', default=1)
    p.add_argument('--device', help='Render on this device (e.g. cuda:0: one st_render_pool call per group of files); default: the host effects', default=None)
    args = p.parse_args()
    from signaltrain_amd import datasets
    if args.effect not in datasets.GEN_EFFECTS:
        raise SystemExit(f"-e {args.effect}: no such effect here (available: {', '.join(datasets.GEN_EFFECTS)})")
    if args.sp is None:
        print(f"About {2 * 4 * args.num * args.dur * args.sr / 1e9:.2f} GB of float32 audio will be written under {args.name}")
    datasets.gen_dataset(args.name, dur=args.dur, sp=args.sp, num=args.num, effect=args.effect, inpath=args.inpath, sr=args.sr, seed=args.seed, device=args.device)
