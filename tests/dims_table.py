"""The (ft, hop, frame) sizes of tests/test_gpu_dims_sweep.py, shared with the host-only tests (importing this needs no GPU).

st_dims admits any N % 32 == 0, H % 4 == 0, L % 4 == 0, y % 4 == 0, OT <= T, H T >= L + N (check_dims, csrc/st_api.hip); st_geometry only ever produces
N = 1024 / H = 384 and two legacy multiples.  Each row below reaches a dispatch branch (or a boundary between two) that those never reach.  Ordered from
the shape nearest the tested ones to the farthest, so that a run that stops at the first failure (pytest -x) stops at the mildest shape that shows it.
"""
import numpy as np

from oracle import st_oracle as O

# id: (N, H, L, T, OT); y = (OT - 1) H - N.  T = (L + N) // H + 1 (the reference's Conv1d frame count) except ragged (+ 1) and short_t (- 1).
ROWS = {
    "n512": (512, 192, 4096, 25, 9),         # N % 256 == 0 (128-row tiles of the weight-gradient GEMM), two per basis half
    "n256": (256, 96, 2048, 25, 9),          # ... one per basis half
    "n384": (384, 144, 3072, 25, 9),         # N % 128 == 0 but N % 256 != 0: 16-bit operand pipeline on, 128-tile weight gradient off
    "ragged": (256, 96, 2020, 25, 9),        # T = Conv frames + 1: the last frame is all padding, the one before it partly
    "t32_ot16": (256, 96, 2784, 32, 16),     # the last fused-autoencoder geometry
    "t33_ot17": (256, 96, 2880, 33, 17),     # the first wide one, both conditions true
    "t33_ot9": (256, 96, 2880, 33, 9),       # wide through T alone
    "t25_ot17": (256, 96, 2048, 25, 17),     # wide through OT alone
    "ot_eq_t16": (256, 96, 1248, 16, 16),    # OT == T, fused
    "ot_eq_t": (256, 96, 2048, 25, 25),      # y == L, OT == T, wide
    "h512": (1024, 512, 4096, 11, 6),        # ceil(N / H) = 2 in the four-sample overlap-add kernel
    "h256": (1024, 256, 4096, 21, 8),        # ceil(N / H) = 4: the one-sample overlap-add kernel, four overlapping frames
    "n160": (160, 60, 1536, 29, 10),         # F = 81, KP = 192; N % 128 != 0: the 16-bit modes take the plain 16-bit GEMM
    "n96": (96, 32, 640, 24, 8),             # N % 32 only; KP = 128
    "short_t": (96, 32, 640, 23, 8),         # T = Conv frames - 1: the omitted frame starts at L (dead), so H T == L + N stays legal
    "h_eq_n": (256, 256, 1024, 6, 3),        # no overlap at all
    "n32": (32, 12, 256, 25, 9),             # F = 17, KP = 64; N below every tile size
    "h_gt_n": (256, 260, 1040, 5, 3),        # gaps between frames (H > N)
    "tiny": (256, 96, 96, 4, 4),             # the smallest legal y (32), L < N, one window
}

# dims that check_dims refuses: T leaves out a frame that still overlaps the signal (H T < L + N)
REFUSED = {
    "n1024_h256_t19": (1024, 256, 4096, 19, 8),       # the reference has 21 frames here; frame 20 starts at L (dead: T = 20 is legal), frame 19 holds 256 samples
    "short_t_minus_1": (96, 32, 640, 22, 8),
    "ragged_t23": (256, 96, 2020, 23, 9),
}


def conv_frames(N, H, L):
    return (L + N) // H + 1


def geo_of(row):
    """The dict O.geometry returns, for a table row (or any (N, H, L, T, OT))."""
    N, H, L, T, OT = ROWS[row] if isinstance(row, str) else row
    y = (OT - 1) * H - N
    return dict(L=L, out_chunk_intended=y, N=N, H=H, T=T, OT=OT, y=y, F=N // 2 + 1)


# ---------------------------------------------------------------------------------------------- seeds
# A comparison at tolerance tau says something about a kernel only if fp32 arithmetic itself is well inside tau on those inputs: the float32 oracle must
# agree with the float64 oracle to tau / 4 on every compared tensor (input_condition below; asserted on the CPU by tests/test_abi_and_host.py for every
# case of sweep_cases()).  Seeds 0 (per-op) and 1 (fused) qualify at every row but two, whose seeds are the first two that qualify in the order
# 0, 1, 2, ... (five tried at most): with a hop of 256 / 512 samples at 1024 taps some windows hold bins close to silence, where d atan2 is ill-conditioned
# and the analysis-basis gradients of the float32 oracle move by 5.6e-5 (h256, seed 0) and 8.8e-5 (h512, seed 1) of their maximum.
SEEDS = {"h256": (1, 2), "h512": (3, 4)}        # row -> (per-op seed, fused seed)


def seeds_of(row):
    return SEEDS.get(row, (0, 1))


# per-op (run_all) cases beyond B = 3, K = 4 at every row: (row, B, K)
PER_OP_EXTRA = [("t33_ot17", 1, 0), ("n160", 1, 0), ("h256", 2, 16), ("n32", 2, 16)]
SPLIT_ROWS = ["n384", "t33_ot17", "h256", "n160"]                                   # run_fused under f32x3
HALF_ROWS = ["n384", "t32_ot16", "t33_ot17", "ot_eq_t", "h256", "n160"]             # bf16_all and f16_all, per-op and fused
BIG_ROWS = [("n256", 600), ("n32", 600)]                                            # R = B * 7 live output frames >= 4096: the tile shape / split-K branches
BIG_SEED = 1                                # the fused seed qualifies at both rows (the oracle sums its bias gradients pairwise: 77 400 rows at n256)
EVAL_ROWS = ["t33_ot17", "h256", "n160"]
MODULE_ROWS = ["h256", "n160"]
MODULE_SEED = 1                             # K = 3 there (other knob draws than at K = 4): seed 1 qualifies at both rows


def big_seed(row):
    return BIG_SEED


def sweep_cases():
    """Every (row, B, K, seed, kind) whose inputs the GPU sweep compares against the float64 oracle at the fp32 tolerances; kind = "per-op" (run_all)
    or "fused" (run_fused, the guarded st_loss_backward, the module route)."""
    out = []
    for row in ROWS:
        a, f = seeds_of(row)
        out += [(row, 3, 4, a, "per-op"), (row, 3, 4, f, "fused")]
    out += [(row, B, K, seeds_of(row)[0], "per-op") for row, B, K in PER_OP_EXTRA]
    out += [(row, B, 4, big_seed(row), "fused") for row, B in BIG_ROWS]
    out += [(row, 3, 3, MODULE_SEED, "fused") for row in MODULE_ROWS]
    return out


TOL = 1e-4            # tests/gpu_checks.py TOL (BASELINE.json north star)
LOOSE = ("syn_wgrad.l1", "step.l1norm", "polar_bwd.dim(zero frames)")        # compared at 1e-3 by gpu_checks
TRAIN_STEPS = 2       # run_fused(steps=2) everywhere in the sweep


def condition_bound(name, kind):
    """A quarter of the tolerance the sweep applies to that tensor (tests/gpu_checks.py): 1e-4, except 2e-4 on the gradients of a fused run, 1e-3 on the two
    L1 norms and on the polar backward of all-padding frames, and 2e-5 absolute on the parameters after a train step."""
    if name in LOOSE:
        return 1e-3 / 4
    if name.endswith(".params"):
        return 2e-5 / 4
    return (2 * TOL if kind == "fused" and name.startswith("grad.") else TOL) / 4


def input_condition(geo, X, Y, KN, P, kind="fused"):
    """{tensor: max|f32 oracle - f64 oracle| / scale} of one case, for every tensor the sweep compares, named and scaled the way gpu_checks names and scales
    it.  Both kinds: y_hat, mag, mag_hat, the loss and the 40 gradient tensors (the STFT gradients by the maximum of their real / imaginary pair).
    kind = "per-op" adds what run_all compares stage by stage -- re / im, the magnitude-weighted phase, the autoencoder outputs and their polar form, the
    synthesis frames on the taps that survive the crop, the loss gradient, the data gradients of every stage, the polar backward on live and on all-padding
    frames, the L1 norm and the two partial-sum totals.  There each device stage is fed the float64 oracle's inputs, while the float32 oracle here carries
    its own error from stage to stage, so the figure is an upper estimate of the per-stage one -- except at the phase autoencoder and the polar backward,
    which are computed here as run_all runs them, in float32 from the float64 oracle's tensors: a near-silent bin turns an input error of 1e-7 into one
    of 1e-4 there, which says nothing about the stage.  kind = "fused" adds the L1 norm and the TRAIN_STEPS train
    steps on the rolled inputs: run_fused compares those with the oracle in float32, so the condition is that a float64 forward / backward in its place
    moves neither the loss nor any parameter by a quarter of the tolerance."""
    f = np.float64
    P64 = {k: v.astype(f) for k, v in P.items()}
    l64, G64, c64 = O.model_loss_bwd(X.astype(f), KN.astype(f), Y.astype(f), P64, geo)
    l32, G32, c32 = O.model_loss_bwd(X, KN, Y, P, geo)
    mx = lambda *a: max(max(float(np.abs(np.asarray(v, f)).max()) for v in a), 1e-30)
    d = lambda a, b: float(np.abs(np.asarray(a, f) - np.asarray(b, f)).max())
    rel = lambda a, b: abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)
    out = {"loss": rel(l32, l64)}
    for k in ("out", "mag", "mag_hat"):
        out[k] = d(c32[k], c64[k]) / mx(c64[k])
    ss = {"an": mx(G64[O.STFT_KEYS[0]], G64[O.STFT_KEYS[1]]), "sy": mx(G64[O.STFT_KEYS[2]], G64[O.STFT_KEYS[3]])}
    for k in G64:
        sc = ss["an"] if k in O.STFT_KEYS[:2] else ss["sy"] if k in O.STFT_KEYS[2:] else mx(G64[k])
        out["grad." + k.replace("mpaec.", "")] = d(G32[k], G64[k]) / sc
    l1 = lambda Gd, keys: sum(float(np.abs(np.asarray(Gd[k], f)).sum()) for k in keys)
    if kind == "per-op":
        N, H, T, OT, F, y = (geo[k] for k in ("N", "H", "T", "OT", "F", "y"))
        pair = lambda names, a, b, sel=slice(None): {n_: d(c32[k][:, sel], c64[k][:, sel]) / mx(c64[a][:, sel], c64[b][:, sel]) for n_, k in names}
        out.update(pair((("analysis.re", "re"), ("analysis.im", "im")), "mag", "mag"))
        dphi = np.angle(np.exp(1j * (c32["phs"].astype(f) - c64["phs"])))
        out["analysis.phs"] = float((np.abs(dphi) * c64["mag"] / mx(c64["mag"])).max())
        s32 = np.float32                                         # two stages amplify their input's error where a bin is near silence: as run_all feeds them
        e9p, _ = O.ae_fwd(c64["phs"].astype(s32), KN, P, "mpaec.phs_aenc", "")
        out["ae_fwd.phs_hat"] = d(e9p + c64["phs"].astype(s32)[:, T - OT:], c64["phs_hat"]) / mx(c64["phs_hat"])
        out.update(pair((("ae_fwd.an_real", "Are"), ("ae_fwd.an_imag", "Aim")), "Are", "Aim"))
        w = O.freq_weights(F, f)
        out["ae_fwd.reg_sum"] = rel(np.abs(c32["mag_hat"].astype(f) * w).sum(), np.abs(c64["mag_hat"] * w).sum())
        tap = H * np.arange(OT)[:, None] + np.arange(N)[None, :]
        live = (tap >= N) & (tap < N + y)
        fr = {}
        for dt, c, Pd in ((np.float32, c32, P), (f, c64, P64)):
            a, b = O.fold_synthesis(Pd[O.STFT_KEYS[2]].astype(dt), Pd[O.STFT_KEYS[3]].astype(dt), F)
            fr[dt] = (c["Are"].reshape(-1, F) @ a + c["Aim"].reshape(-1, F) @ b).reshape(-1, OT, N)[:, live]
        out["synthesis.frames"] = d(fr[np.float32], fr[f]) / mx(fr[f])
        out["ola.dsyn"] = d(c32["dy"], c64["dy"]) / mx(c64["dy"])
        out["ola.logcosh"] = rel(np.mean(O.logcosh(Y.astype(f) - c32["out"])), np.mean(O.logcosh(Y.astype(f) - c64["out"])))
        out.update(pair((("syn_dgrad.dAre", "dAre"), ("syn_dgrad.dAim", "dAim")), "dAre", "dAim"))
        out["ae_bwd.dmag"] = d(c32["dmag"], c64["dmag"]) / mx(c64["dmag"])
        out["ae_bwd.dphs"] = d(c32["dphs"], c64["dphs"]) / mx(c64["dphs"])
        re, im, mg, dm, dp = (c64[k].astype(s32) for k in ("re", "im", "mag", "dmag", "dphs"))      # the polar backward of O.model_loss_bwd in float32
        rp = re + s32(O.EPS_ATAN); den = rp * rp + im * im
        inv = np.where(mg > 0, 1 / np.where(mg > 0, mg, 1), 0)
        pb = {"dre": dm * re * inv - dp * im / den, "dim": dm * im * inv + dp * rp / den}
        mid, ends = slice(1, T - 1), [0, T - 1]                 # gpu_checks: frames 0 and T - 1 are compared apart, at 1e-3
        for k in ("dre", "dim"):
            out["polar_bwd." + k] = d(pb[k][:, mid], c64[k][:, mid]) / mx(c64["dre"][:, mid], c64["dim"][:, mid])
        out["polar_bwd.dim(zero frames)"] = d(pb["dim"][:, ends], c64["dim"][:, ends]) / mx(c64["dim"][:, ends])
        out["syn_wgrad.l1"] = rel(l1(G32, O.STFT_KEYS[2:]), l1(G64, O.STFT_KEYS[2:]))
    else:
        out["step.l1norm"] = rel(l1(G32, O.STFT_KEYS), l1(G64, O.STFT_KEYS))
        lrs, _ = O.get_1cycle_schedule(lr_max=1e-3, n_data_points=200, epochs=1, batch_size=2)        # gpu_checks._run_fused, step for step
        st = {dt: ({k: P[k].copy() for k in O.param_order()}, {k: np.zeros_like(P[k]) for k in O.param_order()},
                   {k: np.zeros_like(P[k]) for k in O.param_order()}) for dt in (np.float32, f)}
        lr = lrs[0]
        for it in range(TRAIN_STEPS):
            Xi, Yi = np.roll(X, 17 * it, axis=1).copy(), np.roll(Y, 17 * it, axis=1).copy()
            lo = {}
            for dt, (Pq, Mq, Vq) in st.items():
                lo[dt], Gq, _ = O.model_loss_bwd(Xi.astype(dt), KN.astype(dt), Yi.astype(dt), {k: v.astype(dt) for k, v in Pq.items()}, geo)
                O.clip_l1_stft(Gq)
                O.adam_step(Pq, Gq, Mq, Vq, it + 1, lr)
            lr = lrs[it]
            out[f"train{it}.loss"] = rel(lo[np.float32], lo[f])
            out[f"train{it}.params"] = max(d(st[np.float32][0][k], st[f][0][k]) for k in O.param_order())
    return out
