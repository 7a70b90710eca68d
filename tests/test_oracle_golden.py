"""CPU: the oracle (oracle/st_oracle.py) against the golden vectors captured from the imported
reference by tools/capture_golden.py.  This is what pins the oracle; it needs neither the
reference nor a GPU."""
import os
import numpy as np
import pytest
from oracle import st_oracle as O
from tests.golden_util import perturb_stft, projections, ae_keys, SAMPLE_ROWS, STFT_KEYS


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def close(a, b, rtol, what=""):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    scale = max(float(np.max(np.abs(b))), 1e-30)
    err = float(np.max(np.abs(a - b)))
    assert err <= rtol * scale, f"{what}: max|d|={err:.3e} scale={scale:.3e}"


def golden_params(golden_dir, geo, fixture="g3_forward.npz", prefix="ae_", seed=7):
    g = load(golden_dir, fixture)
    P = O.init_params(geo, 4)
    for k in ae_keys():
        P[k] = g[prefix + k]
    perturb_stft(P, seed=seed)
    return P


def test_g1_geometry(golden_dir):
    tab = load(golden_dir, "g1_geometry.npz")["table"]
    assert len(tab) >= 20
    for s, sh, legacy, L, y, T, OT, N, H in tab:
        g = O.geometry(int(s), int(sh), "legacy" if legacy else "lean")
        assert (g["L"], g["y"], g["T"], g["OT"], g["N"], g["H"]) == (L, y, T, OT, N, H)
    g = O.geometry(1, 4)
    assert (g["L"], g["y"], g["T"], g["OT"]) == (8192, 2048, 25, 9)
    g = O.geometry(8, 4)
    assert (g["L"], g["y"], g["T"], g["OT"]) == (65536, 16256, 174, 46)


def test_g2_init_bases(golden_dir):
    g = load(golden_dir, "g2_init_bases.npz")
    P = O.init_params(O.geometry(1, 4), 4)
    np.testing.assert_allclose(O.hamming(1024), g["hamming"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(O.gla_window(1024, 384), g["gla"], rtol=0, atol=1e-14)
    for k in STFT_KEYS:
        w = P[k][:, 0, :]
        # <= 1 ulp f32 on sampled rows, and column sums as a whole-tensor fingerprint
        np.testing.assert_allclose(w[SAMPLE_ROWS], g["rows_" + k], rtol=0, atol=4e-9)
        np.testing.assert_allclose(w.astype(np.float64).sum(0), g["colsum_" + k], rtol=0, atol=2e-6)


def test_frame_indexing_bit_exact():
    """Integer contract: frame starts 384t-1024, OLA offsets 384t, crop [1024, 1024+y)."""
    geo = O.geometry(1, 4)
    st = O.frame_starts(geo["T"], geo["H"], geo["N"])
    assert st[0] == -1024 and st[1] == -640 and st[24] == 8192
    x = np.arange(1, 8193, dtype=np.float32)[None]
    fr = O.frames(x, 1024, 384, 25)
    assert np.all(fr[0, 0] == 0) and np.all(fr[0, 24] == 0)          # frames 0 and 24 are all padding
    assert fr[0, 3, 0] == x[0, 3 * 384 - 1024] and fr[0, 23, 383] == x[0, 8191] and fr[0, 23, 384] == 0
    frs = np.zeros((1, 9, 1024), np.float32); frs[0, 4, 10] = 1
    full = O.overlap_add(frs, 384)
    assert full.shape == (1, 4096) and full[0, 4 * 384 + 10] == 1 and full.sum() == 1


def test_g3_forward(golden_dir):
    g = load(golden_dir, "g3_forward.npz")
    geo = O.geometry(1, 4)
    P = golden_params(golden_dir, geo)
    y, mag, mag_hat, c = O.model_fwd(g["x"], g["knobs"], P, geo, return_all=True)
    close(y, g["y_hat"], 3e-6, "y_hat"); close(mag, g["mag"], 3e-6, "mag"); close(mag_hat, g["mag_hat"], 3e-6, "mag_hat")
    close(c["re"], g["re"], 3e-6, "re"); close(c["im"], g["im"], 3e-6, "im")
    close(c["Are"], g["an_real"], 5e-6, "an_real"); close(c["Aim"], g["an_imag"], 5e-6, "an_imag")
    close(c["syn"], g["x_fwdsyn"], 5e-6, "x_fwdsyn")
    # unfolded (literal flip/cat) synthesis == folded synthesis
    syn_lit = O.synthesis_fwd(c["Are"], c["Aim"], P[STFT_KEYS[2]], P[STFT_KEYS[3]], geo, folded=False)
    close(syn_lit, c["syn"], 5e-6, "fold")
    FB = g["act_bins"]
    for pref, hs, tol in (("m", c["hs_m"], 5e-6), ("p", c["hs_p"], 5e-5)):
        for j in range(9):
            o = hs[j + 1] if j < 4 else hs[j]
            if j == 3:
                o = o[:, :, :16]
            close(o[:, FB, :], g[f"{pref}_act{j}"], tol, f"{pref} act{j}")


def test_g4_backward(golden_dir):
    g3 = load(golden_dir, "g3_forward.npz"); g = load(golden_dir, "g4_backward.npz")
    geo = O.geometry(1, 4)
    P = golden_params(golden_dir, geo)
    X, KN, Y = (g3[k].astype(np.float64) for k in ("x", "knobs", "y"))
    loss, G, _ = O.model_loss_bwd(X, KN, Y, P, geo)
    close(loss, g["loss"], 3e-5, "loss")
    for k in ae_keys():
        close(G[k], g["g_" + k], 2e-5, k)
    PROJ = projections(seed=11)
    for k in STFT_KEYS:
        gk = G[k][:, 0, :]
        close(gk[SAMPLE_ROWS], g["rows_" + k], 2e-5, "rows " + k)
        close(gk[:, SAMPLE_ROWS], g["cols_" + k], 2e-5, "cols " + k)
        close(PROJ @ gk, g["proj_" + k], 2e-5, "proj " + k)
        close(np.abs(gk).sum(), g["l1_" + k], 1e-3, "l1 " + k)
    # structural facts of SURVEY.md a11: analysis rows >= 513 are exactly zero; synthesis Hermitian symmetry
    assert np.all(G[STFT_KEYS[0]][513:] == 0) and np.all(G[STFT_KEYS[1]][513:] == 0)
    k = np.arange(1, 512)
    np.testing.assert_array_equal(G[STFT_KEYS[2]][1024 - k, 0], G[STFT_KEYS[2]][k, 0])
    np.testing.assert_array_equal(G[STFT_KEYS[3]][1024 - k, 0], -G[STFT_KEYS[3]][k, 0])
    n, coef = O.clip_l1_stft({k: v.astype(np.float32) for k, v in G.items()})
    close(n, g["clip_norm"], 1e-3, "clip norm"); close(coef, g["clip_coef"], 1e-3, "clip coef")


def test_backward_finite_difference():
    """Independent of the reference: hand-derived backward vs central differences (float64, tiny B)."""
    geo = O.geometry(1, 4)
    rng = np.random.default_rng(0)
    P = O.init_params(geo, 4, rng)
    perturb_stft(P, seed=3)
    P = {k: v.astype(np.float64) for k, v in P.items()}
    X = rng.standard_normal((1, geo["L"])) * 0.3
    KN = rng.uniform(-.5, .5, (1, 4)); Y = rng.standard_normal((1, geo["y"])) * 0.3
    loss, G, _ = O.model_loss_bwd(X, KN, Y, P, geo)
    probes = [("mpaec.aenc.fnn_enc2.weight", (3, 5)), ("mpaec.phs_aenc.fnn_addknobs.weight", (2, 18)),
              ("mpaec.phs_aenc.fnn_dec.bias", (4,)), (STFT_KEYS[0], (37, 0, 500)), (STFT_KEYS[3], (100, 0, 411)),
              (STFT_KEYS[2], (1024 - 100, 0, 411))]
    for k, idx in probes:
        h = 1e-6 * max(1.0, abs(P[k][idx]))
        old = P[k][idx]
        P[k][idx] = old + h; lp = O.model_loss_bwd(X, KN, Y, P, geo)[0]
        P[k][idx] = old - h; lm = O.model_loss_bwd(X, KN, Y, P, geo)[0]
        P[k][idx] = old
        fd = (lp - lm) / (2 * h)
        assert abs(fd - G[k][idx]) <= 2e-4 * max(abs(fd), abs(G[k][idx])) + 1e-12, (k, idx, fd, G[k][idx])


def test_g5_adam_steps(golden_dir):
    g3 = load(golden_dir, "g3_forward.npz"); g = load(golden_dir, "g5_adam.npz")
    geo = O.geometry(1, 4)
    P = golden_params(golden_dir, geo)
    P = {k: P[k].copy() for k in O.param_order()}
    M = {k: np.zeros_like(v) for k, v in P.items()}; V = {k: np.zeros_like(v) for k, v in P.items()}
    lrs, _ = O.get_1cycle_schedule(lr_max=1e-3, n_data_points=200, epochs=1, batch_size=2)
    np.testing.assert_allclose(lrs[:4], g["lrs"], rtol=1e-14)
    PROJ = projections(seed=11)
    lr = lrs[0]
    for it in range(3):
        Xi = np.roll(g3["x"], 17 * it, axis=1).copy(); Yi = np.roll(g3["y"], 17 * it, axis=1).copy()
        assert lr == g[f"lr_used{it}"]        # lr used at iteration i is lr_sched[max(i-1,0)] (train.py:150)
        loss, _, _ = O.train_step(Xi, g3["knobs"], Yi, P, M, V, it + 1, lr, geo)
        lr = lrs[it]
        close(loss, g[f"loss{it}"], 3e-5, f"loss{it}")
        for k in ae_keys():
            np.testing.assert_allclose(P[k], g[f"s{it}_" + k], rtol=0, atol=6e-7, err_msg=k)
        for k in STFT_KEYS:
            np.testing.assert_allclose(P[k][SAMPLE_ROWS, 0, :], g[f"s{it}_rows_" + k], rtol=0, atol=2e-7)
            close(PROJ @ P[k][:, 0, :].astype(np.float64), g[f"s{it}_proj_" + k], 1e-5, "proj")


def test_g6_1cycle(golden_dir):
    g = load(golden_dir, "g6_1cycle.npz")
    lr, mom = O.get_1cycle_schedule(lr_max=1e-4, n_data_points=200000, epochs=100, batch_size=200)
    assert len(lr) == int(g["n"]) == 100000
    np.testing.assert_allclose(lr[g["idx"]], g["lr"], rtol=1e-15)
    np.testing.assert_allclose(mom[g["idx"]], g["mom"], rtol=1e-15)


def test_g7_dct_variant(golden_dir):
    g = load(golden_dir, "g7_dct.npz")
    W = O.dct_bases(1024, 2048)
    np.testing.assert_array_equal(W[SAMPLE_ROWS], g["basis_rows"])
    xft = O.dct_analysis_fwd(g["x"], W, g["bias"])
    assert xft.shape == (1, 9, 1024)
    close(xft[:, :, ::8], g["xft"], 3e-6, "dct analysis")
    wav = O.dct_synthesis_fwd(xft, W)
    assert wav.shape == (1, 1, 8192)
    close(wav, g["wav"], 5e-6, "dct synthesis")


def test_g8_scale8(golden_dir):
    g = load(golden_dir, "g8_scale8.npz")
    geo = O.geometry(8, 4)
    P = golden_params(golden_dir, geo, "g8_scale8.npz", "ae_", seed=9)
    y, mag, mag_hat = O.model_fwd(g["x"], g["knobs"], P, geo)
    assert y.shape == (1, 16256) and mag_hat.shape == (1, 46, 513)
    close(y, g["y_hat"], 5e-6, "y"); close(mag_hat[:, :, ::4], g["mag_hat"], 5e-6, "mag_hat")


def test_g8b_scale8_backward(golden_dir):
    """BASELINE configs[4] geometry (T = 174, OT = 46): the reference's autograd at the 65536-sample window (golden G8b, round 3) --
    loss, all 36 autoencoder gradients, the STFT gradients by sampled rows / projections / L1 norms -- against the oracle's hand-derived
    backward, which rounds 1-2 had pinned at scale 1 only."""
    g8, g = load(golden_dir, "g8_scale8.npz"), load(golden_dir, "g8b_scale8_backward.npz")
    geo = O.geometry(8, 4)
    P = golden_params(golden_dir, geo, "g8_scale8.npz", "ae_", seed=9)
    loss, G, _ = O.model_loss_bwd(g8["x"].astype(np.float64), g8["knobs"].astype(np.float64), g["y"].astype(np.float64), P, geo)
    close(loss, g["loss"], 3e-5, "loss")
    for k in ae_keys():
        close(G[k], g["g_" + k], 3e-5, k)
    PROJ = projections(seed=13)
    for k in STFT_KEYS:
        close(G[k][SAMPLE_ROWS, 0, :], g["rows_" + k], 3e-5, "rows " + k)
        close(PROJ @ G[k][:, 0, :], g["proj_" + k], 3e-5, "proj " + k)
        close(np.abs(G[k]).sum(), g["l1_" + k], 1e-4, "l1 " + k)


def test_g9_compressor(golden_dir):
    g = load(golden_dir, "g9_compressor.npz")
    y = O.compressor_4controls(g["x"].copy(), *g["knobs"][:4], sr=g["knobs"][4])
    close(y, g["y"], 1e-6, "compressor_4controls")


def test_perfect_reconstruction_at_init():
    """Implicit invariant of the reference's init: analysis -> synthesis is identity."""
    geo = O.geometry(1, 1)                    # shrink 1: y = 8064 of the 8192 samples
    P = O.init_params(geo, 4)
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((1, geo["L"])) * 0.3).astype(np.float32)
    re, im = O.analysis_fwd(x, P[STFT_KEYS[0]], P[STFT_KEYS[1]], geo)
    syn = O.synthesis_fwd(re[:, geo["T"] - geo["OT"]:], im[:, geo["T"] - geo["OT"]:], P[STFT_KEYS[2]], P[STFT_KEYS[3]], geo)
    assert np.max(np.abs(syn - x[:, geo["L"] - geo["y"]:])) < 5e-6


# ------------------------------------------------------------------------------------------------ round-2 goldens
def test_g4b_backward_with_active_clip(golden_dir):
    """The reference's clip_grad_norm_ with n > 1 (nn_proc.py:299-302; norm 2.71 -> coefficient 0.369): the oracle's clip
    branch against the reference's own clipped gradients (G4 ran with coefficient 1.0)."""
    g = load(golden_dir, "g4b_backward_clip.npz")
    assert float(g["clip_norm"]) > 1.5 and float(g["clip_coef"]) < 0.7
    geo = O.geometry(1, 4)
    P = golden_params(golden_dir, geo)
    loss, G, _ = O.model_loss_bwd(g["x"].astype(np.float64), g["knobs"].astype(np.float64), g["y"].astype(np.float64), P, geo)
    close(loss, g["loss"], 3e-5, "loss")
    for k in ae_keys():
        close(G[k], g["g_" + k], 2e-5, k)
    PROJ = projections(seed=11)
    for k in STFT_KEYS:
        close(G[k][SAMPLE_ROWS, 0, :], g["rows_" + k], 2e-5, "rows " + k)
        close(PROJ @ G[k][:, 0, :], g["proj_" + k], 2e-5, "proj " + k)
    G32 = {k: v.astype(np.float32) for k, v in G.items()}
    n, coef = O.clip_l1_stft(G32)
    # sum |g| over 4 M fp32 values depends on the summation order at ~1.5e-4 (torch's fp32 reduction vs a float64 sum)
    close(n, g["clip_norm"], 1e-3, "clip norm"); close(coef, g["clip_coef"], 1e-3, "clip coef")
    for k in STFT_KEYS:
        close(G32[k][SAMPLE_ROWS, 0, :], g["clipped_rows_" + k], 1e-3, "clipped rows " + k)
        close(PROJ @ G32[k][:, 0, :].astype(np.float64), g["clipped_proj_" + k], 1e-3, "clipped proj " + k)
        close(np.abs(G32[k]).sum(), g["clipped_l1_" + k], 1e-3, "clipped l1 " + k)
    for k in ae_keys():                                            # the autoencoder gradients are NOT clipped on this path
        np.testing.assert_array_equal(G32[k], G[k].astype(np.float32))


def test_g5b_adam_steps_with_active_clip(golden_dir):
    g4b = load(golden_dir, "g4b_backward_clip.npz"); g = load(golden_dir, "g5b_adam_clip.npz")
    geo = O.geometry(1, 4)
    P = golden_params(golden_dir, geo)
    P = {k: P[k].copy() for k in O.param_order()}
    M = {k: np.zeros_like(v) for k, v in P.items()}; V = {k: np.zeros_like(v) for k, v in P.items()}
    lrs, _ = O.get_1cycle_schedule(lr_max=1e-3, n_data_points=300, epochs=1, batch_size=3)
    np.testing.assert_allclose(lrs[:4], g["lrs"], rtol=1e-14)
    PROJ = projections(seed=11)
    lr = lrs[0]
    for it in range(3):
        Xi = np.roll(g4b["x"], 23 * it, axis=1).copy(); Yi = np.roll(g4b["y"], 23 * it, axis=1).copy()
        assert lr == g[f"lr_used{it}"]
        loss, norm, coef = O.train_step(Xi, g4b["knobs"], Yi, P, M, V, it + 1, lr, geo)
        lr = lrs[it]
        assert float(g[f"clip_norm{it}"]) > 1.2 and coef < 0.9                   # the clip acts on every step
        close(loss, g[f"loss{it}"], 3e-5, f"loss{it}"); close(norm, g[f"clip_norm{it}"], 1e-3, f"norm{it}")
        for k in ae_keys():
            np.testing.assert_allclose(P[k], g[f"s{it}_" + k], rtol=0, atol=3e-6, err_msg=k)
        for k in STFT_KEYS:
            np.testing.assert_allclose(P[k][SAMPLE_ROWS, 0, :], g[f"s{it}_rows_" + k], rtol=0, atol=3e-6)
            close(PROJ @ P[k][:, 0, :].astype(np.float64), g[f"s{it}_proj_" + k], 1e-5, "proj")


def test_mixed_precision_switches_of_the_oracle():
    """fp16 operand rounding is IEEE (overflow -> inf, like Apex amp); the loss scale multiplies every gradient and train_step removes it;
    CLIP_ALL widens the clip to every parameter (train.py:136)."""
    a = np.array([1e6, -1e6, 0.1, 65504.0, 1e-9], np.float32)
    r = O.fp16_round(a)
    assert np.isposinf(r[0]) and np.isneginf(r[1]) and r[3] == 65504 and abs(r[2] - 0.1) < 1e-4 and r[4] == 0
    geo = O.geometry(1, 4)
    rng = np.random.default_rng(5)
    P = O.init_params(geo, 4, rng); perturb_stft(P, seed=3)
    X, Y, KN = O.synth_comp4c_batch(1, geo["L"], geo["y"], rng)
    l0, G0, _ = O.model_loss_bwd(X, KN, Y, P, geo)
    try:
        O.LOSS_SCALE = 1024.0
        l1, G1, _ = O.model_loss_bwd(X, KN, Y, P, geo)
    finally:
        O.LOSS_SCALE = 1.0
    assert l1 == l0
    for k in G0:
        close(G1[k] / 1024.0, G0[k], 1e-5, k)
    Gc = {k: v.copy() * 50 for k, v in G0.items()}
    n_stft, _ = O.clip_l1_stft({k: v.copy() for k, v in Gc.items()})
    n_all, c_all = O.clip_l1_stft(Gc, all_params=True)
    assert n_all > n_stft and c_all < 1
    k = "mpaec.aenc.fnn_enc.weight"
    close(Gc[k], G0[k] * 50 * np.float32(c_all), 1e-6, "AE gradient clipped under all_params")


def test_g10_reference_checkpoint_layout(golden_dir, tmp_path):
    """A checkpoint with exactly the layout the reference's misc.save_checkpoint wrote (header G10: top-level keys, the 40
    state_dict tensors, torch.optim.Adam's per-parameter state) loads through signaltrain_amd.misc and st_model.load_state_dict,
    the optimizer state converts to the engine's flat moments and back, and a checkpoint written by signaltrain_amd.misc has the
    same layout.  (The reference-written 50 MB file itself was read by these functions in tools/capture_golden_r2.py.)"""
    import torch
    from signaltrain_amd import misc, nn_proc
    nn_proc._QUIET = True
    g = load(golden_dir, "g10_checkpoint.npz")
    assert tuple(g["top_keys"]) == misc.CKPT_KEYS
    assert list(g["opt_top_keys"]) == ["state", "param_groups"] and list(g["opt_state_keys"]) == ["step", "exp_avg", "exp_avg_sq"]
    geo = O.geometry(1, 4)
    names = [str(k) for k in g["sd_keys"]]
    assert names == O.param_order() and len(names) == 40 and set(g["sd_dtypes"]) == {"torch.float32"}
    # rebuild the file in the reference's layout: sampled tensors from the fixture, the 4 MB bases regenerated
    P = golden_params(golden_dir, geo)
    shapes = [tuple(int(v) for v in s.split(",")) for s in g["sd_shapes"]]
    sd, st = {}, {}
    for i, (k, shp) in enumerate(zip(names, shapes)):
        if k in STFT_KEYS:
            w = P[k].copy(); m = np.zeros(shp, np.float32); v = np.zeros(shp, np.float32)
            m[SAMPLE_ROWS, 0, :] = g["m_rows_" + k]; v[SAMPLE_ROWS, 0, :] = g["v_rows_" + k]
        else:
            w, m, v = g["p_" + k], g["m_" + k], g["v_" + k]
        assert w.shape == shp and tuple(g["opt_state_shapes"][i].split(",")) == tuple(str(s) for s in shp)
        sd[k] = torch.from_numpy(np.ascontiguousarray(w))
        st[i] = {"step": torch.tensor(float(g["opt_step"])), "exp_avg": torch.from_numpy(m), "exp_avg_sq": torch.from_numpy(v)}
    group = {k: None for k in g["opt_group_keys"]}
    group.update(lr=float(g["opt_lr"]), betas=tuple(g["opt_betas"]), eps=float(g["opt_eps"]), params=[int(i) for i in g["opt_group_params"]])
    blob = {"epoch": int(g["epoch"]), "state_dict": sd, "optimizer": {"state": st, "param_groups": [group]},
            "effect_name": str(g["effect_name"]), "knob_names": [str(s) for s in g["knob_names"]], "knob_ranges": g["knob_ranges"],
            "scale_factor": int(g["scale_factor"]), "shrink_factor": int(g["shrink_factor"]), "in_chunk_size": int(g["in_chunk_size"]),
            "out_chunk_size": int(g["out_chunk_size"]), "sr": int(g["sr"])}
    f = str(tmp_path / "modelcheckpoint.tar")
    torch.save(blob, f)
    sd2, rv = misc.load_checkpoint(f, device="cpu")
    assert rv["epoch"] == 42 and rv["in_chunk_size"] == 8192 and rv["out_chunk_size"] == 2048 and rv["knob_ranges"].shape == (4, 2)
    model = nn_proc.st_model(scale_factor=rv["scale_factor"], shrink_factor=rv["shrink_factor"], num_knobs=len(rv["knob_names"]), sr=rv["sr"])
    model.load_state_dict(sd2)                                       # strict: all 40 keys, shapes of the reference
    flat = misc.flatten_optimizer_state(rv["optimizer"], shapes)
    assert flat is not None and flat["step"] == 3 and flat["lr"] == float(g["opt_lr"]) and len(flat["exp_avg"]) == 40
    k = "mpaec.phs_aenc.fnn_dec.weight"
    np.testing.assert_array_equal(flat["exp_avg"][names.index(k)], g["m_" + k].ravel())
    # ... and back: torch.optim.Adam accepts what the engine side emits
    osd = misc.adam_state_dict(flat["step"], flat["lr"], [torch.from_numpy(a.reshape(s)) for a, s in zip(flat["exp_avg"], shapes)],
                               [torch.from_numpy(a.reshape(s)) for a, s in zip(flat["exp_avg_sq"], shapes)])
    opt = torch.optim.Adam(model.parameters(), lr=1.0)
    opt.load_state_dict(osd)
    assert opt.param_groups[0]["lr"] == float(g["opt_lr"]) and float(opt.state[list(model.parameters())[5]]["step"]) == 3
    assert misc.flatten_optimizer_state({"state": {"step": 3}, "param_groups": []}, shapes) is None       # the round-1 stand-in layout is rejected
    # a checkpoint written by this package carries the reference's keys
    class _Eff: name = "comp_4c"; knob_names = rv["knob_names"]; knob_ranges = rv["knob_ranges"]
    f2 = str(tmp_path / "mine.tar")
    misc.save_checkpoint(f2, model, 41, False, opt, _Eff, 44100)
    raw = torch.load(f2, weights_only=False)
    assert tuple(raw.keys()) == tuple(g["top_keys"]) and list(raw["state_dict"].keys()) == names
    assert sorted(raw["optimizer"]["param_groups"][0].keys()) == sorted(k for k in g["opt_group_keys"] if k != "momentum")


def test_g11_host_signal_generators(golden_dir):
    """oracle/host_audio.py (the checker of the device feed's signal families) against the reference's synth_input_sample (audio.py:296-334) and
    SynthAudioDataSet.gen_single_chunk (datasets.py:312-334) at fixed seeds of numpy's global generator: bit for bit (tools/capture_golden_r4.py)."""
    from oracle import host_audio as H
    from signaltrain_amd import audio as A
    g = load(golden_dir, "g11_host_signals.npz")
    n, sr = int(g["n"]), int(g["sr"])
    t = np.arange(n, dtype=np.float32) / sr
    for c in g["choosers"]:
        for s in g["seeds"]:
            np.random.seed(int(s))
            y = H.synth_input_sample(t, int(c))
            assert np.array_equal(y, g[f"sig_c{c}_s{s}"]), f"chooser {c} seed {s}"
    eff = A.Compressor_4c()
    for s in g["item_seeds"]:
        np.random.seed(int(s))
        x, y, k = H.gen_single_chunk(t, eff, n // 2, augment=True)
        assert np.array_equal(np.asarray(k, np.float64), g[f"item_k_s{s}"]) and np.array_equal(np.asarray(x, np.float64), g[f"item_x_s{s}"])
        close(y, g[f"item_y_s{s}"], 2e-6, f"compressor target, item seed {s}")


def test_g12_knob_gradient(golden_dir):
    """Golden G12 (tools/capture_golden_r4.py): the reference's autograd w.r.t. a knobs tensor that requires grad (nn_proc.py:92-93: knob settings
    repeated over a window's rows, concatenated in front of fnn_addknobs of both autoencoders) for the G3 / G4 inputs and weights; pins the oracle's
    d_knobs (model_loss_bwd cache), the checker of st_model_knob_grad."""
    g3 = load(golden_dir, "g3_forward.npz"); g = load(golden_dir, "g12_knob_grad.npz")
    geo = O.geometry(1, 4)
    P = golden_params(golden_dir, geo)
    loss, _, c = O.model_loss_bwd(g3["x"].astype(np.float64), g3["knobs"].astype(np.float64), g3["y"].astype(np.float64), P, geo)
    close(loss, g["loss"], 3e-5, "loss")
    assert c["d_knobs"].shape == g["d_knobs"].shape == (2, 4)
    close(c["d_knobs"], g["d_knobs"], 2e-5, "d knobs (float64 oracle)")
    _, _, c32 = O.model_loss_bwd(g3["x"], g3["knobs"], g3["y"], P, geo)
    close(c32["d_knobs"], g["d_knobs"], 2e-4, "d knobs (float32 oracle)")


@pytest.mark.parametrize("ci", [0, 1])
def test_g13_near_silent_backward(golden_dir, ci):
    """G13 (tools/capture_golden_r5.py): two window sets with near-silent STFT bins through the REFERENCE's fp32 autograd.  The reference's own analysis-basis
    gradient sits 4e-4 ... 1.1e-3 of the tensor maximum away from the float64 evaluation of the same formulas (stored as ref_vs_f64): d atan2(im, re + 1e-7)
    (nn_proc.py:309-310) amplifies the fp32 rounding of re / im by 1 / mag.  Pinned here: (i) that distance really exceeds the suite's fixed 2e-4 -- so a
    fixed tolerance on these two tensors cannot be met by ANY fp32 implementation, the reference included, and tests/gpu_spread.py's per-configuration spread
    is the honest bound; (ii) the oracle in float64 and in float32 both agree with the reference within 3 x that distance on the analysis bases and at fp32
    rounding level (2e-5) on the synthesis bases; (iii) loss and the autoencoder gradients' maxima at 1e-4."""
    from tests import gpu_checks as G                       # make_case only (numpy)
    g = np.load(os.path.join(golden_dir, "g13_near_silent_backward.npz"))
    pre = f"c{ci}_"
    B, seed, K = (int(v) for v in g[pre + "cfg"])
    geo, X, Y, KN, P = G.make_case(B, seed, K=K)
    l64, g64, _ = O.model_loss_bwd(X.astype(np.float64), KN.astype(np.float64), Y.astype(np.float64), {k: v.astype(np.float64) for k, v in P.items()}, geo)
    l32, g32, _ = O.model_loss_bwd(X, KN, Y, P, geo)
    assert abs(l64 - float(g[pre + "loss"])) <= 3e-5 * abs(l64) and abs(float(l32) - float(g[pre + "loss"])) <= 3e-5 * abs(l64)
    PROJ = projections(seed=17)
    worst_an = 0.0
    for k in STFT_KEYS:
        d_ref = float(g[pre + "ref_vs_f64_" + k])
        an = "analysis" in k
        worst_an = max(worst_an, d_ref if an else 0.0)
        if not an:
            assert d_ref < 2e-5
        for name, og in (("f64", g64[k]), ("f32", g32[k].astype(np.float64))):
            m = og[:, 0, :]
            sc = float(g[pre + "max_" + k])
            tol = (3.0 * d_ref if an else 2e-5) * sc
            assert np.abs(m[SAMPLE_ROWS] - g[pre + "rows_" + k]).max() <= tol, (k, name)
            # a projection sums 1024 elements with |weights| <= 1: its error is bounded by 1024 x the element bound (and is far below it)
            assert np.abs(PROJ @ m - g[pre + "proj_" + k]).max() <= 1024 * tol, (k, name)
            assert abs(np.abs(m).sum() - float(g[pre + "l1_" + k])) <= (1e-3 if an else 1e-4) * float(g[pre + "l1_" + k]), (k, name)
    assert worst_an > 2e-4                                  # (i)
    for k in ae_keys():
        if (pre + "max_" + k) in g:
            ref = float(g[pre + "max_" + k])
            assert abs(np.abs(g64[k]).max() - ref) <= 1e-4 * max(ref, 1e-30), k


def test_spread_grading_rules_cap_and_localized_miss():
    """tests/gpu_spread.grounded() on synthetic check records (no GPU, no oracle run: the spread of the configuration comes from the committed table).
    A miss of the fixed tolerance is accepted (a) inside 3 x the spread and 10 x the tolerance; (b) round 6: over that cap only when the elements over the tolerance
    sit in <= LOCAL_ROWS rows of a tensor with >= 8 x LOCAL_ROWS rows (a near-silent bin pollutes ONE row of an analysis-basis gradient, a wrong tile covers >= 96);
    everything else stays a failure -- outside the spread, spread out over many rows, a scalar over the cap, a quantity the spread does not cover."""
    from tests import gpu_spread as S
    kw = dict(B=1, seed=499, K=2, scale=2, scheme="lean", shrink=4)           # profiles/r05_fuzz_f32_spread.json holds it (tools/fuzz_ground_f32.py case 21)
    sp = S.spread_of(kw)
    name = "grad.dft_analysis.conv_analysis_imag.weight"
    s = max(sp["f32"][name], sp["noise"][name])
    assert 5e-3 < s < 5e-2                                                       # a spread of ~1e-2: the configuration the localized rule was written for
    tol = 2e-4
    rec = lambda rel, **kwargs: dict(name=name, rel=rel, tol=tol, ok=False, err=rel, scale=1.0, **kwargs)
    inside_cap = rec(5 * tol, rows=1024, rows_over=300)
    assert S.grounded([inside_cap], kw) == [] and inside_cap["grounded"] and not inside_cap.get("localized")
    local = rec(14 * tol, rows=1024, rows_over=1)
    assert 14 * tol < 3 * s
    assert S.grounded([local], kw) == [] and local["localized"]
    edge = rec(14 * tol, rows=1024, rows_over=S.LOCAL_ROWS)
    assert S.grounded([edge], kw) == []
    for bad in (rec(14 * tol, rows=1024, rows_over=S.LOCAL_ROWS + 1),          # spread over more rows than a conditioning miss has
                rec(14 * tol, rows=1024, rows_over=128),                          # a tile's worth
                rec(14 * tol, rows=64, rows_over=1),                              # a tensor too small for "a few rows" to mean anything
                rec(14 * tol),                                                    # no row information (a scalar): the cap stands
                rec(3.5 * s, rows=1024, rows_over=1)):                            # localized but outside 3 x the spread
        assert S.grounded([bad], kw) == [bad] and not bad["ok"], bad
    unknown = dict(name="some.other.quantity", rel=1e-3, tol=1e-4, ok=False, err=1e-3, scale=1.0)
    assert S.grounded([unknown], kw) == [unknown]
    # the clip norm has a spread entry for configurations graded since round 6 ...
    kw2 = dict(B=5, seed=719, K=12, scale=1, scheme="lean", shrink=4)
    sp2 = S.spread_of(kw2)
    assert 5e-3 < max(sp2["f32"]["step.l1norm"], sp2["noise"]["step.l1norm"]) < 2e-2
    norm = dict(name="step.l1norm", rel=9.9e-3, tol=1e-3, ok=False, err=9.9e-3, scale=1.0)
    assert S.grounded([norm], kw2) == []
    # ... and stays a failure where the committed table predates it
    old = dict(B=6, seed=576, K=4, scale=1, scheme="lean", shrink=8)
    if "step.l1norm" not in S.spread_of(old)["f32"]:
        norm_old = dict(name="step.l1norm", rel=2e-3, tol=1e-3, ok=False, err=2e-3, scale=1.0)
        assert S.grounded([norm_old], old) == [norm_old]


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_g14_edges(golden_dir, ci):
    """G14 (tools/capture_golden_r6.py): three edge cases of the model surface through the REFERENCE's forward / loss / fp32 autograd -- a model without knobs
    (nn_proc.py:92-93 concatenates an empty tensor), one knob, and DIGITAL SILENCE (an all-zero window, a window that starts with half a window of zeros: 52 % of the
    STFT bins are exactly zero; the reference takes d |.| = 0 and d atan2 / d im = 1e7 there, nn_proc.py:309-310).  The oracle in float64 reproduces loss (3e-5),
    y_hat (1e-5), all 36 autoencoder gradients (1e-4 of the tensor maximum) and the fingerprints of the four STFT gradients (synthesis 2e-5; analysis
    max(2e-5, 3 x the reference's own distance from float64), as in G13)."""
    from tests.golden_util import g14_case
    g = np.load(os.path.join(golden_dir, "g14_edges.npz"))
    geo, X, Y, KN, P, K = g14_case(ci)
    assert KN.shape == (X.shape[0], K)
    l64, g64, c64 = O.model_loss_bwd(X.astype(np.float64), KN.astype(np.float64), Y.astype(np.float64), {k: v.astype(np.float64) for k, v in P.items()}, geo)
    pre = f"c{ci}_"
    assert abs(l64 - float(g[pre + "loss"])) <= 3e-5 * abs(l64)
    assert np.abs(c64["out"] - g[pre + "y_hat"]).max() <= 1e-5 * np.abs(c64["out"]).max()
    assert abs(np.abs(c64["mag"]).max() - float(g[pre + "mag_max"])) <= 1e-5 * float(g[pre + "mag_max"])
    assert abs(np.abs(c64["mag_hat"]).max() - float(g[pre + "mag_hat_max"])) <= 1e-5 * float(g[pre + "mag_hat_max"])
    if ci == 2:
        assert (c64["mag"] == 0).mean() > 0.5 and np.all(c64["out"][0] == c64["out"][0]) and all(np.isfinite(v).all() for v in g64.values())
    for k in ae_keys():
        ref = g[pre + "g_" + k].astype(np.float64)
        assert ref.shape == g64[k].shape, (k, ref.shape, g64[k].shape)
        assert np.abs(g64[k] - ref).max() <= 1e-4 * max(np.abs(ref).max(), 1e-30), k
    PROJ = projections(seed=23)
    for k in STFT_KEYS:
        m = g64[k][:, 0, :]
        sc = float(g[pre + "max_" + k])
        tol = max(2e-5, 3.0 * float(g[pre + "ref_vs_f64_" + k]) if "analysis" in k else 2e-5) * sc
        assert np.abs(m[SAMPLE_ROWS] - g[pre + "rows_" + k]).max() <= tol, k
        assert np.abs(PROJ @ m - g[pre + "proj_" + k]).max() <= 1024 * tol, k
        assert abs(np.abs(m).sum() - float(g[pre + "l1_" + k])) <= 1e-4 * float(g[pre + "l1_" + k]), k


@pytest.mark.parametrize("tag", ["c64", "c96"])
def test_g16_other_ft_hop_and_frame_sizes(golden_dir, tag):
    """Every other golden is at ft 1024 / hop 384 or a legacy multiple.  G16 (tools/capture_golden_sizes.py): the reference's AsymMPAEC built directly at
    (ft, hop, L, T, OT, K) = (64, 24, 528, 25, 9, 3) and (96, 32, 640, 24, 8, 2), B = 2 -- whole tensors, no fingerprints: forward outputs, the loss and the
    autograd gradients of all 40 tensors, at the tolerances of G3 / G4.  This is what pins the oracle at the sizes of tests/dims_table.py."""
    g = load(golden_dir, "g16_other_sizes.npz")
    N, H, L, T, OT, K = (int(v) for v in g["table"][list(g["cases"]).index(tag)])
    y = (OT - 1) * H - N
    geo = dict(L=L, out_chunk_intended=y, N=N, H=H, T=T, OT=OT, y=y, F=N // 2 + 1)
    assert T == (L + N) // H + 1
    assert list(g["param_names"]) == O.param_order()
    P = {k: g[f"{tag}_p{i:02d}"] for i, k in enumerate(O.param_order())}
    Gref = {k: g[f"{tag}_g{i:02d}"] for i, k in enumerate(O.param_order())}
    assert [P[k].shape for k in O.param_order()[4:22:2]] == O.ae_layer_shapes(T, OT, K)
    X, KN, Y = g[f"{tag}_x"], g[f"{tag}_knobs"], g[f"{tag}_y"]
    assert X.shape == (2, L) and KN.shape == (2, K) and Y.shape == (2, y)
    yh, mag, mag_hat = O.model_fwd(X, KN, P, geo)
    close(yh, g[f"{tag}_y_hat"], 3e-6, "y_hat"); close(mag, g[f"{tag}_mag"], 3e-6, "mag"); close(mag_hat, g[f"{tag}_mag_hat"], 3e-6, "mag_hat")
    loss, G, _ = O.model_loss_bwd(X.astype(np.float64), KN.astype(np.float64), Y.astype(np.float64), P, geo)
    close(loss, g[f"{tag}_loss"], 3e-5, "loss")
    for k in O.param_order():
        assert G[k].shape == Gref[k].shape
        close(G[k], Gref[k], 2e-5, k)
    F = geo["F"]
    for k in STFT_KEYS[:2]:
        assert np.all(G[k][F:] == 0) and np.all(Gref[k][F:] == 0)
