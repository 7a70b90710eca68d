#!/usr/bin/env python3
"""bench.py -- SignalTrain train-step throughput on MI355X (driver contract, see DESIGN.md 'Measurement').

  python bench.py --gpus N --steps K --warmup W
  (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...)

Workload = BASELINE.json configs[1]: comp_4c synthetic, 8192-sample windows, batch 256 per GPU, fp32
(weak scaling: global batch 256*N).  One step = forward + calc_loss + backward + L1 clip + Adam
[+ RCCL all-reduce of the 16.8 MB gradient], inputs resident in HBM.  Prints ONE JSON line on rank 0.

A plain run times the headline step only.  --full adds the measurements reported beside it (HIP-graph replay, f32x3,
per-kernel roofline, CPU baseline).  --dump-outputs DIR writes what the last timed step computed, for comparing two builds.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

PEAK_FP32_MFMA_TF = 157.3          # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 / 16x16x4_f32, dense fp32
PEAK_HALF_MFMA_TF = 2500.0         # MI355X_MICROARCH.md: bf16 / fp16 MFMA, DENSE (the 5 PF headline figure is 2:1 sparsity)
GEMM_KERNELS = ("analysis_fwd", "analysis_wgrad", "synthesis_frames", "synthesis_dgrad", "synthesis_wgrad")


def kernel_peak(name, dtype):
    """MFMA peak that bounds kernel `name` under --dtype: the STFT GEMMs run 16-bit operands in every mixed mode, the
    autoencoder kernels only in the *_all modes."""
    if dtype == "f32":
        return PEAK_FP32_MFMA_TF
    if dtype == "f32x3":                   # six bf16 MFMAs per fp32-grade product block: the bf16 dense peak / 6
        return PEAK_HALF_MFMA_TF / 6.0 if name in GEMM_KERNELS else PEAK_FP32_MFMA_TF
    if name in GEMM_KERNELS or dtype.endswith("_all"):
        return PEAK_HALF_MFMA_TF
    return PEAK_FP32_MFMA_TF


DTYPE_TEXT = {"f32x3": "fp32 (STFT GEMM products from a three-way bfloat16 split of the fp32 operands: six partial products on the bf16 matrix pipe, "
                       "fp32 accumulate; fp32-grade accuracy)",
              "f32": "fp32", "bf16": "bf16 GEMM operands / fp32 accumulate", "bf16_all": "bf16 operands in the STFT GEMMs and the autoencoder layers / fp32 accumulate",
              "f16": "fp16 GEMM operands / fp32 accumulate, loss scale 4096", "f16_all": "fp16 mixed precision: fp16 operands in the STFT GEMMs and the autoencoder layers / fp32 accumulate, "
                                                                                         "loss scale 4096, clip over all parameters"}


def workload_text(d, B, dtype, scale, scheme="lean"):
    if scheme != "lean":
        return (f"comp_4c synthetic, {d.L}-sample windows, legacy 'large-FFT' scheme (nn_proc.py:374-376: ft={d.N}, hop={d.H}, "
                f"{4 * d.N * d.N / 1e6:.0f} M basis parameters), batch {B}/GPU, {DTYPE_TEXT[dtype]} (SURVEY 8(f)-4, informational)")
    cfg = {(1, "f32"): "BASELINE configs[1]", (1, "bf16"): "arithmetic of BASELINE configs[2]", (1, "bf16_all"): "arithmetic of BASELINE configs[2]",
           (8, "f16"): "BASELINE configs[4] per GPU", (8, "f16_all"): "BASELINE configs[4] per GPU"}.get((scale, dtype))
    if cfg is None:
        cfg = "geometry of BASELINE configs[4]" if scale == 8 else "informational"
    return f"comp_4c synthetic, {d.L}-sample windows, batch {B}/GPU, {DTYPE_TEXT[dtype]} ({cfg})"
METRIC = "audio-frames/sec (train step) comp_4c 8192-sample windows @ 1/2/4/8 GPUs"


def algorithmic_flops(d):
    """SURVEY.md 8(d) 'useful-dense' convention, per launch of each GEMM-shaped kernel (1 MAC = 2 FLOP)."""
    B, T, OT, F, N, K = d.B, d.T, d.OT, d.F, d.N, d.K
    ae_mac = 64 * T + 32 * 64 + 16 * 32 + 16 * 16 + 16 * (16 + K) + 16 * 16 + 32 * 16 + 64 * 32 + OT * 64
    dec_mac = 16 * (16 + K) + 16 * 16 + 32 * 16 + 64 * 32 + OT * 64        # layers 5..9 (st_ae_split.h, decoder half)
    an = 2.0 * B * T * (2 * F) * N
    sy = 2.0 * B * OT * (2 * F) * N              # Hermitian-folded: 9.46 M MAC/window at the default geometry
    ae = 2.0 * B * F * 2 * ae_mac
    return {"analysis_fwd": an, "analysis_wgrad": an, "synthesis_frames": sy, "synthesis_dgrad": sy,
            "synthesis_wgrad": sy, "ae_fwd": ae, "ae_bwd": 2 * ae,
            "ae_bwd_dec": 2 * (2.0 * B * F * 2 * dec_mac), "ae_bwd_enc": 2 * (2.0 * B * F * 2 * (ae_mac - dec_mac)),
            "ae_wide_fwd": ae, "ae_wide_bwd": 2 * ae}, (2 * an + 3 * sy + 3 * ae)      # wide geometries: st_ae_wide.h


def main():
    # Native libraries write to stdout behind our back (RCCL prints a version banner at exit); the contract is ONE JSON
    # line on stdout, so fd 1 is pointed at stderr for the whole run and the result goes to the saved descriptor.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)       # defaults = the flags the round-end driver passes
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prewarm-s", type=float, default=0.5, help="untimed, REPORTED pre-warm before the declared warm-up: steps are run until this many seconds "
                                                                 "have passed (clocks / caches / allocator of a cold GPU settle; `prewarm_s`, `prewarm_steps` in the JSON line)")
    ap.add_argument("--full", action="store_true", help="also run the measurements reported beside the headline (each in its own leg after the timed steps): "
                                                        "HIP-graph replay, f32x3, per-kernel roofline, CPU baseline.  Without it only the headline step is timed")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed as DIR/<name>.npy (float32): params, grads "
                                                          "(each a fixed, seeded sample when larger than 7 M values), scalars")
    ap.add_argument("--no-f32x3", action="store_true", help="--full, N = 1, --dtype f32: skip the f32x3 measurement reported beside the exact-fp32 value (ms_per_step_f32x3)")
    ap.add_argument("--batch", type=int, default=256, help="windows per GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="--full: skip the per-kernel roofline leg")
    ap.add_argument("--bk", type=int, default=0, help="GEMM k-tile depth override (16/32)")
    ap.add_argument("--no-graph", action="store_true", help="--full, N = 1: skip the HIP-graph replay measurement (ms_per_step_graph)")
    ap.add_argument("--tune", type=int, nargs="*", default=[], help="diagnostics: st_set_tuning codes applied before the run")
    ap.add_argument("--ablate", type=int, default=0, help="diagnostics: st_set_debug bits for a library built with -DST_GEMM_ABLATE / -DST_AE_ABLATE "
                                                          "(timing-only; the numbers of such a run are INVALID as results)")
    ap.add_argument("--dp-schedule", choices=["two_bucket", "staged"], default="two_bucket", help="all-reduce schedule of the data-parallel step (signaltrain_amd/dp.py)")
    ap.add_argument("--dp-pack16", action="store_true", help="the last (exposed) exchange of the data-parallel step on bfloat16 values (library back end, *_all dtypes only)")
    ap.add_argument("--force-dp", action="store_true", help="run the N > 1 code path (bucketed RCCL all-reduce, st_dp_clip_adam) "
                                                            "even with one rank, to measure its overhead on one GPU")
    ap.add_argument("--dtype", choices=("f32", "f32x3", "bf16", "bf16_all", "f16", "f16_all"), default="f32",
                    help="f32 = the headline / parity configuration; bf16 / f16 = 16-bit operands with fp32 accumulation in the STFT GEMMs; *_all = also in the autoencoder layers "
                         "(bf16*: arithmetic of BASELINE configs[2], [3]; f16* with --scale 8 --batch 64: configs[4]; informational, never the headline number)")
    ap.add_argument("--scheme", choices=["lean", "legacy"], default="lean", help="window scaling scheme (nn_proc.py:371-376): lean keeps ft=1024/hop=384, "
                                                                                "legacy scales them with the window (scale 8: ft=8192, hop=3072, 268 M parameters)")
    ap.add_argument("--scale", type=int, default=1, help="window scale factor (8 = the 65536-sample window of BASELINE configs[4]; "
                                                          "informational -- the headline workload is scale 1)")
    ap.add_argument("--dp-backend", choices=("lib", "torch"), default="lib",
                    help="N > 1: lib = the exchange inside libsignaltrain_hip.so (its own RCCL communicator, one C call per step; torch.distributed/gloo "
                         "only bootstraps the unique id); torch = torch.distributed collectives on RCCL driven from Python")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    rank = int(os.environ.get("RANK", "0")); local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}.  N > 1 runs one process per GPU:\n  python -m torch.distributed.run "
                         f"--nnodes=1 --nproc-per-node {args.gpus} --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus {args.gpus} "
                         f"--steps {args.steps} --warmup {args.warmup}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU (there is no CPU fallback of the product path)")
    if os.environ.get("ST_BENCH_SHARE_GPU"):          # tests only: every rank on GPU 0 (with ST_RCCL_LIB = the RCCL test double) -- runs this file's N > 1 path on a one-GPU box
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import torch.distributed as dist
    dp_backend = args.dp_backend
    if world > 1 or args.force_dp:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
        if dp_backend == "lib":
            os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")          # one node: gloo would otherwise look the host name up, which need not resolve on a GPU box
            dist.init_process_group("gloo", rank=rank, world_size=world)      # bootstrap + timing fence only; gradients move on the library's RCCL communicator
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from signaltrain_amd import _lib, nn_proc, audio, datasets, learningrate
    from signaltrain_amd.engine import StepEngine
    from signaltrain_amd.dp import DataParallel
    nn_proc._QUIET = True

    B = args.batch
    if args.bk:
        _lib.check(_lib.load().st_set_tuning(args.bk), 'st_set_tuning')
    for code in args.tune:
        _lib.check(_lib.load().st_set_tuning(int(code)), 'st_set_tuning')
    if args.ablate:
        _lib.check(_lib.load().st_set_debug(int(args.ablate)), 'st_set_debug')
    d = _lib.geometry(args.scale, 4, 4, B, scale_scheme=args.scheme)
    # identical init on every rank (run_train.py:20-21 seeds 218), distinct data per rank
    torch.manual_seed(218); np.random.seed(218)
    model = nn_proc.st_model(scale_factor=args.scale, shrink_factor=4, num_knobs=4, scale_scheme=args.scheme)
    eng = StepEngine(d, dev, compute_dtype=args.dtype)
    eng.load_state_dict(model.state_dict())
    dp_note = None
    try:
        dp = DataParallel(eng, force_collectives=args.force_dp, schedule=args.dp_schedule, backend=dp_backend if (world > 1 or args.force_dp) else None,
                          pack16=args.dp_pack16)
        ok = 1
    except Exception as e:                       # the library could not bring up its communicator
        dp, ok, dp_note = None, 0, f"{type(e).__name__}: {e}"
    if (world > 1 or args.force_dp) and dp_backend == "lib":
        flag = torch.tensor([ok]); dist.all_reduce(flag, op=dist.ReduceOp.MIN)      # every rank takes the same branch
        if int(flag.item()) == 0:
            # LOUD, recorded in the JSON line: same protocol over torch.distributed's RCCL collectives instead
            print(f"bench.py: library-owned RCCL communicator unavailable ({dp_note}); using torch.distributed collectives", file=sys.stderr)
            if eng.dp is not None:
                _lib.load().st_dp_destroy(eng.dp); eng.dp = None
            dist.destroy_process_group()
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
            dp_backend = "torch"; dp_note = "fallback from lib: " + str(dp_note)
            dp = DataParallel(eng, force_collectives=args.force_dp, schedule=args.dp_schedule, backend="torch")
    elif dp is None:
        raise RuntimeError(dp_note)
    # evidence that N ranks met (VERDICT round 3 next #4c): every rank reports the world size ITS communicator was built with and the RCCL it is bound to;
    # the line carries min / max over ranks (must both equal N) and the version
    dp_evidence = None
    if (world > 1 or args.force_dp) and dp.backend == "lib":
        lib = _lib.load()
        w_here, ver = int(lib.st_dp_world(eng.dp)), int(lib.st_dp_rccl_version(eng.dp))
        lo = torch.tensor([w_here, ver], dtype=torch.int64); hi = lo.clone()
        if world > 1:
            dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        assert int(lo[0]) == int(hi[0]) == world, f"communicator world sizes over ranks: min {int(lo[0])}, max {int(hi[0])}, expected {world}"
        dp_evidence = {"dp_world_min": int(lo[0]), "dp_world_max": int(hi[0]), "rccl_version": ("test double" if int(hi[1]) == -1 else int(hi[1])),
                       "rccl_version_same_on_all_ranks": bool(int(lo[1]) == int(hi[1]))}
    dp.broadcast_parameters()
    np.random.seed(218 + 1000 * (rank + 1))
    ds = datasets.SynthAudioDataSet(d.L, audio.Compressor_4c(), y_size=d.y, augment=True)
    x, y, kn = ds.batch_device(B, dev)          # comp_4c windows from the device feed (csrc/st_feed.h): signals, knobs, compressor targets
    lrs, _ = learningrate.get_1cycle_schedule(lr_max=1e-4, n_data_points=200000, epochs=100, batch_size=B * world)

    def step(i):
        dp.train_step(x, kn, y, float(lrs[max(i - 1, 0)]))

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def all_max(val):
        if world == 1:
            return val
        tt = torch.tensor([val], dtype=torch.float64) if dist.get_backend() == "gloo" else torch.tensor([val], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item())

    def prewarm(fn):
        """Untimed and reported: chunks of 10 steps until --prewarm-s seconds have passed on the slowest rank (every rank runs the same
        number of steps -- the steps contain collectives).  A fresh box needs a few hundred ms of work before its step time is
        stationary; the declared --warmup alone (5 steps = 4 ms) does not cover that."""
        n, t_pw = 0, time.perf_counter()
        fence()
        while args.prewarm_s > 0 and n < 5000:
            for _ in range(10):
                fn(n); n += 1
            fence()
            if all_max(time.perf_counter() - t_pw) >= args.prewarm_s:
                break
        return n, time.perf_counter() - t_pw

    def timed(fn):
        for i in range(args.warmup):
            fn(i)
        fence()
        t0 = time.perf_counter()
        for i in range(args.steps):
            fn(args.warmup + i)
        fence()
        return time.perf_counter() - t0

    def restart():
        """Back to the freshly loaded model (zero Adam moments, step 0): the pre-warm runs as many steps as fit in --prewarm-s, so without
        this the state of the timed steps, and the outputs --dump-outputs writes, would depend on the speed of the build and the box.
        Device-side and stream-ordered: no host round trip that would let the warmed-up GPU idle before the warm-up steps."""
        eng.params.copy_(init); eng.m.zero_(); eng.v.zero_(); eng.scalars.zero_(); eng.step_count = 0

    def dump_outputs(path):
        """What the last timed step computed -- the updated parameters, their gradient and the step's scalars (loss, mean log-cosh, L1 term,
        L1 norm, clip coefficient, overflow-skipped steps) -- as float32 .npy files; a larger array is written as a fixed, seeded sample
        (at most 7 M values each, < 64 MB in all)."""
        os.makedirs(path, exist_ok=True)
        cap = 7_000_000
        for name, t in (("params", eng.params), ("grads", eng.grads), ("scalars", eng.scalars[:6])):
            if t.numel() > cap:
                idx = np.sort(np.random.default_rng(12345).integers(0, t.numel(), cap))
                t = t[torch.from_numpy(idx).to(t.device)]
            np.save(os.path.join(path, name + ".npy"), t.detach().float().cpu().numpy())

    init = eng.params.clone()        # restart() point, identical on every rank; allocated last, so that the step's own tensors sit where they always did
    prewarm_steps, prewarm_s = prewarm(step)
    restart()
    dt = timed(step)
    dt = all_max(dt)
    loss = dp.mean_loss()
    ms = dt / args.steps * 1e3
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs)
    # the same step replayed from ONE captured HIP graph (st_graph_*: step counter and learning rate on the device): reported
    # beside the eager number; `value` stays the eager one (the graph removes host launch work, which the asynchronous eager
    # loop already hides at this step length -- the GPU-side kernel boundaries cost the same either way)
    ms_graph = None
    if args.full and world == 1 and not args.force_dp and not args.no_graph:
        eng.graph_capture(B, lrs)
        eng.gx.copy_(x); eng.gk.copy_(kn); eng.gy.copy_(y)
        ms_graph = timed(lambda i: eng.graph_step()) / args.steps * 1e3
        eng.graph_destroy()
    # fp32-grade STFT GEMMs from the bf16 matrix pipe (compute_dtype "f32x3"), reported BESIDE the exact-fp32 headline, never as it
    ms_x3 = None
    if args.full and world == 1 and not args.force_dp and not args.no_f32x3 and args.dtype == "f32":
        eng3 = StepEngine(d, dev, compute_dtype="f32x3")
        eng3.load_state_dict(model.state_dict())
        f3 = lambda i: eng3.train_step(x, kn, y, float(lrs[max(i - 1, 0)]))
        for i in range(10):
            f3(i)
        ms_x3 = timed(f3) / args.steps * 1e3
        del eng3
    windows_s = B * world / (ms * 1e-3)

    out = None
    if rank == 0:
        flops_k, flops_step = algorithmic_flops(d)
        out = {"metric": METRIC, "value": windows_s * d.T, "unit": "frames/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "prewarm_s": prewarm_s, "prewarm_steps": prewarm_steps, "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": args.dtype, "data": "synthetic",
               "config": {"workload": workload_text(d, B, args.dtype, args.scale, args.scheme),
                          "window": d.L, "frames_per_window": d.T, "global_batch": B * world, "parallelism": f"dp{world}",
                          **({"dp_backend": dp_backend, "dp_schedule": args.dp_schedule} if (world > 1 or args.force_dp) else {}),
                          **({"dp_pack16": True} if args.dp_pack16 else {}), **(dp_evidence or {}),
                          **({"dp_note": dp_note} if dp_note else {})},
               "windows_per_s": windows_s, "samples_per_s": windows_s * d.L, "loss": loss, "ms_per_step_graph": ms_graph, "ms_per_step_f32x3": ms_x3,
               "step_tflops": flops_step / (ms * 1e-3) / 1e12 * world,
               "step_frac_of_fp32_mfma_peak": flops_step / (ms * 1e-3) / 1e12 / PEAK_FP32_MFMA_TF}
        if args.dtype != "f32":
            out["step_frac_of_16bit_mfma_peak"] = flops_step / (ms * 1e-3) / 1e12 / PEAK_HALF_MFMA_TF

    # ------------------------------------------------------------------ roofline leg (outside the timed region)
    if args.full and not args.no_roofline:
        lib = eng.lib
        _lib.check(lib.st_profile_enable(1), "profile_enable")
        nprof = min(args.steps, 20)
        for i in range(nprof):
            eng.loss_backward(x, kn, y)          # same kernels as the step; events recorded on the launch stream
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 16)
        _lib.check(lib.st_profile_report(buf, len(buf)), "profile_report")
        lib.st_profile_enable(0)
        if rank == 0:
            rows = {}
            for line in buf.value.decode().strip().splitlines():
                name, tot, cnt = line.split()
                rows[name] = (float(tot) / int(cnt), int(cnt))
            kern = {k: {"avg_us": v[0] * 1e3, "launches": v[1],
                        **({"tflops": flops_k[k] / (v[0] * 1e-3) / 1e12} if k in flops_k else {})} for k, v in rows.items()}
            # the autoencoder backward is ONE logical kernel that runs as two launches (decoder / encoder half, st_ae_split.h): it
            # competes for "dominant kernel" with its combined time and combined algorithmic FLOPs
            if "ae_bwd_dec" in rows and "ae_bwd_enc" in rows:
                rows["ae_bwd"] = (rows["ae_bwd_dec"][0] + rows["ae_bwd_enc"][0], rows["ae_bwd_dec"][1])
            dom = max((k for k in rows if k in flops_k and k not in ("ae_bwd_dec", "ae_bwd_enc")), key=lambda k: rows[k][0])
            ach = flops_k[dom] / (rows[dom][0] * 1e-3) / 1e12
            peak = kernel_peak(dom, args.dtype)
            # HBM-side bytes per launch of that kernel: PMC counters cannot be collected from inside this process, so the value
            # comes from the rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of THIS command on THIS build (tools/profile_gpu.sh ->
            # profiles/*_pmc_traffic*.json, which records the hash of the library sources and the bench arguments it measured):
            # a file measured on other sources or another workload is refused and traffic stays null.
            traffic, traffic_raw, tsrc, rocprof_us = None, None, None, None
            step_traffic, step_launches, mfma_busy = None, None, None
            try:
                import glob
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                from src_sha import src_sha
                want = {"src_sha": src_sha(), "dtype": args.dtype, "scale": args.scale, "batch": B, "scheme": args.scheme}
                keys = {"ae_bwd": ("ae_bwd_kernel", "ae_bwd_part_kernel"), "ae_fwd": ("ae_fwd_kernel", "ae_fwd32_kernel"), "analysis_wgrad": ("gemm_tn_kernel", "PlainTN"),
                        "analysis_fwd": ("AnalysisW",), "ae_wide_bwd": ("ae_bwd_kernel", "DgradStore", "DvStore"), "ae_wide_fwd": ("ae_inner_fwd_kernel", "ActStore", "OutStore")}.get(dom, ())
                refused = []
                for cand in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic*.json")), reverse=True):
                    tj = json.load(open(cand))
                    meta = tj.get("meta", {})
                    if any(meta.get(k) != v for k, v in want.items()):
                        refused.append(os.path.basename(cand)); continue
                    hit = [v for k, v in tj.get("kernels", {}).items() if any(q in k for q in keys) and ("FETCH_SIZE_KB" in v or "avg_ns" in v)]
                    if hit and all("FETCH_SIZE_KB" in h and "WRITE_SIZE_KB" in h for h in hit):
                        # MI355X_MICROARCH.md, HBM: on gfx950 FETCH_SIZE tallies the 128-byte fabric requests at 64 bytes -- double it; WRITE_SIZE at face value.
                        # Calibrated on two kernels of known traffic in these very profiles (profiles/r04_rocprofv3_summary_f32.txt): clip_adam_kernel reads 63.0 MB and
                        # writes 50.4 MB (FETCH_SIZE 31.0 MB, WRITE_SIZE 47.2 MB), comp_apply_kernel reads 4.19 MB and writes 2.10 MB (2.05 / 2.05 MB).
                        traffic_raw = sum(h["FETCH_SIZE_KB"] + h["WRITE_SIZE_KB"] for h in hit) * 1024.0   # all launches of the logical kernel
                        traffic = sum(2.0 * h["FETCH_SIZE_KB"] + h["WRITE_SIZE_KB"] for h in hit) * 1024.0
                        tsrc = (os.path.basename(cand) + " (2 x FETCH_SIZE + WRITE_SIZE per dispatch: separate rocprofv3 --pmc passes of this command on sources " + want["src_sha"]
                                + "; the factor 2 is the guide's gfx950 correction of FETCH_SIZE, checked here against clip_adam_kernel and comp_apply_kernel whose bytes are known)")
                        # round 5 (VERDICT round 4, next #3d): the WHOLE step's memory-side bytes from the same file -- every library kernel (namespaces st?::) times its launches
                        # per step (launches of a kernel / launches of the once-per-step optimizer kernel) -- beside the algorithmic bytes of SURVEY.md 8(d):
                        # batch I/O (x, y, knobs) + Adam (read p, g, m, v; write p, m, v) + one read of the weights and one write of the gradients
                        lk = {k: v for k, v in tj.get("kernels", {}).items() if any(ns in k for ns in ("stg::", "sta::", "stm::", "stw::", "stf::")) and "FETCH_SIZE_KB" in v and "WRITE_SIZE_KB" in v and v.get("calls")}
                        once = [v["calls"] for k, v in lk.items() if "clip_adam_kernel" in k]
                        if once:
                            step_traffic = sum((2.0 * v["FETCH_SIZE_KB"] + v["WRITE_SIZE_KB"]) * 1024.0 * v["calls"] / once[0] for v in lk.values())
                            step_launches = sum(v["calls"] / once[0] for v in lk.values())
                        mf = [h for h in hit if "SQ_VALU_MFMA_BUSY_CYCLES" in h and h.get("GRBM_GUI_ACTIVE")]
                        if mf and len(mf) == len(hit):      # SQ_VALU_MFMA_BUSY_CYCLES is summed over the chip's SIMDs (4 per CU); GRBM_GUI_ACTIVE is summed over the 8 XCDs
                            # (ae_bwd, fp32: 3.6e6 for a 177 us dispatch = 8 x 448 k cycles) -- so the dispatch's cycles are GRBM_GUI_ACTIVE / 8
                            mfma_busy = sum(h["SQ_VALU_MFMA_BUSY_CYCLES"] for h in mf) / (4.0 * torch.cuda.get_device_properties(dev).multi_processor_count * sum(h["GRBM_GUI_ACTIVE"] for h in mf) / 8.0)
                        if all("avg_ns" in h for h in hit) and not dom.startswith("ae_wide"):          # rocprofv3's own kernel durations of the same command (kernel-trace stats); the wide path's logical kernel is a dozen launches, only some of them keyed here
                            rocprof_us = sum(h["avg_ns"] for h in hit) * 1e-3
                        break
                if traffic is None:
                    tsrc = f"no PMC file for sources {want['src_sha']} / this workload (refused: {len(refused)} files of other builds or workloads)"
            except Exception as e:
                traffic, tsrc = None, f"traffic lookup failed: {e}"
            # `achieved` / `frac` come from the HIP events this process records around every launch (they read ~2-3 us high per launch: the events
            # themselves); when a rocprofv3 kernel trace of this command on these sources exists its average is quoted beside them
            out["roofline"] = {"bound": "mfma", "kernel": dom, "achieved": ach, "peak": peak, "unit": "TFLOP/s",
                               "frac": ach / peak, "traffic": traffic, "traffic_source": tsrc, **({"traffic_uncorrected": traffic_raw} if traffic is not None else {}),
                               "algorithmic_flops_per_launch": flops_k[dom], "avg_launch_us": rows[dom][0] * 1e3,
                               "timing": "in-process HIP events on the launch stream (~2-3 us high per launch)",
                               **({"rocprof_avg_launch_us": rocprof_us, "frac_rocprof": flops_k[dom] / (rocprof_us * 1e-6) / 1e12 / peak} if rocprof_us else {}),
                               **({"launches_per_step": 2, "note": "ae_bwd = ae_bwd_dec + ae_bwd_enc (two launches, times and FLOPs summed)"} if dom == "ae_bwd" and "ae_bwd_dec" in rows else {})}
            # whole-step traffic against the algorithmic bytes: where the 16-bit configurations lose
            n_par = int(eng.layout.total)
            step_alg = float(B) * (d.L + d.y + d.K) * 4.0 + 7.0 * 4.0 * n_par + 2.0 * 4.0 * n_par
            out["roofline"]["step_algorithmic_bytes"] = step_alg
            out["roofline"]["step_traffic"] = step_traffic
            if step_traffic is not None:
                out["roofline"]["step_traffic_ratio"] = step_traffic / step_alg
                out["roofline"]["step_kernel_launches"] = step_launches
                out["roofline"]["step_traffic_note"] = "sum over the step's kernels of (2 x FETCH_SIZE + WRITE_SIZE) x launches per step, same PMC file as `traffic`"
            kept = int(lib.st_ae_kept_activation_bytes(C.byref(eng._dims(B))))
            if kept:      # round 6: what the forward keeps for the backward (the reference's autograd keeps the same tensors); NOT part of SURVEY 8(d)'s algorithmic bytes
                out["roofline"]["step_kept_activation_bytes"] = 2 * kept
                out["roofline"]["step_kept_activation_note"] = ("autoencoder activations written once by ae_fwd and read once by ae_bwd (instead of recomputing the forward chain: "
                                                                 "-40 us of matrix + vector work for +12 us of stores at B = 256); counted in step_traffic, not in step_algorithmic_bytes")
            out["roofline"]["mfma_busy"] = mfma_busy        # SQ_VALU_MFMA_BUSY_CYCLES / (SIMDs x GRBM_GUI_ACTIVE / 8 XCDs) of the roofline kernel, same file; null without a source-matched PMC pass
            if args.dtype.endswith("_all") and dom.startswith("ae_"):
                # honest label: with 16-bit Linear layers the autoencoder kernels spend ~7 % of their time in MFMAs; what bounds them is vector-ALU work (ELU / ELU',
                # conversions, transposes) and LDS fragment traffic (PMC: profiles/r03_rocprofv3_summary_bf16_all.txt), so the fraction of the MFMA peak is small by construction
                out["roofline"]["note"] = (out["roofline"].get("note", "") + "; 16-bit Linear layers: vector-ALU / LDS bound, not MFMA bound (docs/LAB_NOTEBOOK.md)").lstrip("; ")
                gem = max((k for k in rows if k in flops_k and not k.startswith("ae_")), key=lambda k: rows[k][0], default=None)
                if gem:
                    out["roofline"]["largest_gemm"] = {"kernel": gem, "achieved": flops_k[gem] / (rows[gem][0] * 1e-3) / 1e12, "peak": kernel_peak(gem, args.dtype),
                                                       "frac": flops_k[gem] / (rows[gem][0] * 1e-3) / 1e12 / kernel_peak(gem, args.dtype), "avg_launch_us": rows[gem][0] * 1e3}
            out["kernels"] = kern
            out["kernels_note"] = "avg_us: per-launch HIP events recorded by the library (st_profile_enable) on loss_backward, each ~2-3 us above the rocprofv3 figure; the optimizer kernel is not in this list"

    # ------------------------------------------------------------------ CPU baseline (rank 0, N = 1 only, bounded)
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and args.scale == 1:
        from oracle.torch_cpu_step import CpuPort          # checker-side code: timed beside, never the product path
        # a B=32 step is a handful of small ops: past a few dozen threads torch's CPU backend only adds
        # synchronisation cost (256 threads measured 75 s/step here), so probe a few counts and time the best one
        ncpu = os.cpu_count() or 1
        Bc = 32
        X, Y, KN = (a.cpu().numpy() for a in (x, y, kn))
        port = CpuPort({k: v.detach().cpu().numpy() for k, v in model.state_dict().items()})
        xc, yc, kc = (torch.from_numpy(a[:Bc].copy()) for a in (X, Y, KN))
        best, cores = None, 1
        for nt in [c for c in (8, 16, 32, 64) if c <= ncpu] or [ncpu]:
            torch.set_num_threads(nt)
            port.step(xc, kc, yc, 1e-5)
            t1 = time.perf_counter(); port.step(xc, kc, yc, 1e-5); e = time.perf_counter() - t1
            if best is None or e < best:
                best, cores = e, nt
        torch.set_num_threads(cores)
        # BASELINE.md section 3's protocol: 5 warm-up + 20 timed steps, median (bounded: stops after 30 s of timed work)
        for _ in range(5):
            port.step(xc, kc, yc, 1e-5)
        ts, t_all = [], time.perf_counter()
        while len(ts) < 20 and (time.perf_counter() - t_all) < 30.0:
            t1 = time.perf_counter(); port.step(xc, kc, yc, 1e-5); ts.append(time.perf_counter() - t1)
        tc = float(np.median(ts))
        cpu_model = "unknown"
        try:
            for line in open("/proc/cpuinfo"):
                if line.startswith("model name"):
                    cpu_model = line.split(":", 1)[1].strip(); break
        except OSError:
            pass
        out["cpu_baseline"] = {"value": Bc * d.T / tc, "unit": "frames/s", "cores": cores, "kind": "port",
                               "cpu_model": cpu_model, "cpu_count": ncpu,
                               "sample": f"median of {len(ts)} train steps after 5 warm-up steps, batch {Bc} (BASELINE configs[0] shape), same comp_4c windows, fp32, "
                                         f"PyTorch-CPU restatement of the reference op sequence, {torch.get_num_threads()} threads "
                                         f"(thread count probed over 8/16/32/64)",
                               "ms_per_step": tc * 1e3, "windows_per_s": Bc / tc}
    if rank == 0:
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    if world > 1 or args.force_dp:
        dp.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
