"""CPU: the C-ABI library loads and exports every symbol include/signaltrain_hip.h declares (no compute calls),
host-side geometry / layout logic, the Python mirror of the reference surface, and the CPU baseline port."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import torch

from oracle import st_oracle as O
from signaltrain_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "signaltrain_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(st_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    syms = header_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in the header but not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
    assert lib.st_version() >= 100


def test_geometry_matches_oracle_and_golden(golden_dir):
    tab = np.load(os.path.join(golden_dir, "g1_geometry.npz"))["table"]
    for s, sh, legacy, L, y, T, OT, N, H in tab:
        d = _lib.geometry(int(s), int(sh), 4, 1, "legacy" if legacy else "lean")
        assert (d.L, d.y, d.T, d.OT, d.N, d.H) == (L, y, T, OT, N, H)


def test_param_layout_and_workspace():
    d = _lib.geometry(1, 4, 4, 256)
    offs, total = _lib.param_offsets(d)
    assert offs[:5] == [0, 1 << 20, 2 << 20, 3 << 20, 4 << 20] and total == 4211096 and all(o % 4 == 0 for o in offs)
    from signaltrain_amd.engine import param_names, param_shapes
    names, shapes = param_names(), param_shapes(d)
    assert names == O.param_order() and sum(int(np.prod(s)) for s in shapes) == 4211090
    lib = _lib.load()
    assert lib.st_kp(513) == 1056
    assert 50e6 < lib.st_workspace_bytes(C.byref(d)) < 2e9
    bad = _lib.st_dims(); bad.B = 1
    assert lib.st_workspace_bytes(C.byref(bad)) == 0 and b"dimension" in lib.st_last_error()


def test_error_reporting_without_gpu():
    lib = _lib.load()
    d = _lib.geometry(1, 4, 4, 2)
    rc = lib.st_analysis_fwd(C.byref(d), None, None, None, 0.5, None, None, None, None, None)
    assert rc == -1 and b"null" in lib.st_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(rc, "st_analysis_fwd")


def test_model_mirror_state_dict_and_init(golden_dir):
    from signaltrain_amd import nn_proc
    nn_proc._QUIET = True
    m = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=4)
    sd = m.state_dict()
    assert list(sd.keys()) == O.param_order()
    assert (m.in_chunk_size, m.out_chunk_size, m.num_knobs, m.scale_factor, m.shrink_factor) == (8192, 2048, 4, 1, 4)
    g = np.load(os.path.join(golden_dir, "g2_init_bases.npz"))
    from tests.golden_util import SAMPLE_ROWS, STFT_KEYS
    for k in STFT_KEYS:                       # init bases == the reference's, to <= 1 ulp on the sampled rows
        np.testing.assert_allclose(sd[k].numpy()[SAMPLE_ROWS, 0], g["rows_" + k], rtol=0, atol=4e-9)
    assert m.mpaec.dft_analysis.conv_analysis_real.weight.shape == (1024, 1, 1024)     # io_methods.py:484-493 attribute path
    b = sd["mpaec.aenc.fnn_enc.bias"]; w = sd["mpaec.aenc.fnn_addknobs.weight"]
    assert float(b.abs().max()) == 0.0 and w.shape == (16, 20) and 0.1 < float(w.std()) < 0.4   # xavier_normal: sqrt(2/36)
    m8 = nn_proc.st_model(scale_factor=8, shrink_factor=4, num_knobs=4)
    assert (m8.in_chunk_size, m8.out_chunk_size, m8.mpaec.aenc._T, m8.mpaec.aenc._OT) == (65536, 16256, 174, 46)
    with pytest.raises(RuntimeError):         # the product path fails loudly without a GPU
        m(torch.zeros(1, 8192), torch.zeros(1, 4))


def test_checkpoint_roundtrip(tmp_path):
    from signaltrain_amd import nn_proc, misc, audio
    nn_proc._QUIET = True
    m = nn_proc.st_model(num_knobs=4)
    eff = audio.Compressor_4c()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    f = str(tmp_path / "modelcheckpoint.tar")
    misc.save_checkpoint(f, m, 4, False, opt, eff, 44100)
    sd, rv = misc.load_checkpoint(f, device="cpu")
    assert set(rv) == {"epoch", "optimizer", "effect_name", "knob_names", "knob_ranges", "scale_factor", "shrink_factor",
                       "in_chunk_size", "out_chunk_size", "sr"}           # misc.py:28-34 keys
    assert rv["epoch"] == 5 and rv["in_chunk_size"] == 8192 and rv["out_chunk_size"] == 2048
    m2 = nn_proc.st_model(num_knobs=4); m2.load_state_dict(sd)
    for k in sd:
        assert torch.equal(m2.state_dict()[k], m.state_dict()[k])


def test_learningrate_and_loss_mirrors(golden_dir):
    from signaltrain_amd import learningrate, loss_functions
    g = np.load(os.path.join(golden_dir, "g6_1cycle.npz"))
    lr, mom = learningrate.get_1cycle_schedule(lr_max=1e-4, n_data_points=200000, epochs=100, batch_size=200)
    np.testing.assert_allclose(lr[g["idx"]], g["lr"], rtol=1e-15); np.testing.assert_allclose(mom[g["idx"]], g["mom"], rtol=1e-15)
    rng = np.random.default_rng(0)
    yh, y, mh = rng.standard_normal((3, 64)), rng.standard_normal((3, 64)), rng.standard_normal((3, 9, 513))
    w = O.freq_weights(513, np.float64)
    ref = O.calc_loss(yh, y, mh, w)
    got = loss_functions.calc_loss(torch.from_numpy(yh), torch.from_numpy(y), torch.from_numpy(mh), scale_by_freq=torch.from_numpy(w))
    assert abs(float(got) - ref) < 1e-12


def test_audio_and_dataset_contract(golden_dir):
    from oracle import host_audio
    from signaltrain_amd import audio, datasets
    g = np.load(os.path.join(golden_dir, "g9_compressor.npz"))
    y = audio.compressor_4controls(g["x"], *g["knobs"][:4], sr=g["knobs"][4])
    assert np.abs(y - g["y"]).max() < 1e-6
    np.testing.assert_array_equal(host_audio.sliding_window(np.arange(10), 5, overlap=2), [[0, 1, 2, 3, 4], [3, 4, 5, 6, 7], [6, 7, 8, 9, 0]])
    # the checker-side item assembly (datasets.py:312-334) over the product's host effect: shapes, dtypes, knob range
    np.random.seed(1)
    x, yy, k = host_audio.batch(2, 8192, audio.Compressor_4c(), 2048)
    assert x.shape == (2, 8192) and yy.shape == (2, 2048) and k.shape == (2, 4) and x.dtype == np.float32 and k.dtype == np.float32
    assert np.all(np.abs(k) <= 0.5) and np.abs(x).max() < 1.5
    # the torch Dataset contract of the reference (datasets.py:305-334): items behind __getitem__ / a DataLoader, recycle=True keeps them fixed.
    # Here (no GPU) the items come from the CPU-device form of the batched generators + the effect's host go()
    ds = datasets.SynthAudioDataSet(8192, audio.Compressor_4c(), y_size=2048, item_chunk=4)
    assert len(ds) == 8000
    xi, yi, ki = ds[0]
    assert xi.shape == (8192,) and yi.shape == (2048,) and ki.shape == (4,) and xi.dtype == np.float32 and ki.dtype == np.float32
    assert np.all(np.abs(ki) <= 0.5) and 0.05 < np.abs(xi).max() < 1.5 and np.isfinite(yi).all()
    # the target IS the effect of the input at those knobs (up to the polarity flip of do_augment, applied to both)
    yy2 = audio.Compressor_4c().go(xi, ki)[0][-2048:]
    assert np.abs(yy2 - yi).max() < 1e-5
    xb, yb, kb = next(iter(torch.utils.data.DataLoader(ds, batch_size=3, num_workers=0)))
    assert tuple(xb.shape) == (3, 8192) and tuple(yb.shape) == (3, 2048) and tuple(kb.shape) == (3, 4)
    rec = datasets.SynthAudioDataSet(8192, audio.Compressor_4c(), datapoints=5, y_size=2048, recycle=True, item_chunk=4)
    assert rec.x.shape == (5, 8192) and rec.y.shape == (5, 2048) and np.array_equal(rec[3][0], rec[3][0]) and not np.array_equal(rec[3][0], rec[4][0])


def test_cpu_port_matches_oracle():
    """bench.py's cpu_baseline 'port' computes the same step as the oracle."""
    from oracle.torch_cpu_step import CpuPort
    from tests.golden_util import perturb_stft
    geo = O.geometry(1, 4)
    rng = np.random.default_rng(3)
    P = O.init_params(geo, 4, rng); perturb_stft(P, seed=5)
    X, Y, KN = O.synth_comp4c_batch(2, geo["L"], geo["y"], rng)
    port = CpuPort(P, lr=1e-3)
    Pq = {k: P[k].copy() for k in O.param_order()}
    M = {k: np.zeros_like(v) for k, v in Pq.items()}; V = {k: np.zeros_like(v) for k, v in Pq.items()}
    for it in range(2):
        lp = port.step(torch.from_numpy(X), torch.from_numpy(KN), torch.from_numpy(Y), 1e-3)
        lo, _, _ = O.train_step(X, KN, Y, Pq, M, V, it + 1, 1e-3, geo)
        assert abs(lp - lo) <= 3e-5 * abs(lo)
        for k in Pq:
            assert np.abs(port.P[k].detach().numpy() - Pq[k]).max() < 2e-5, k   # Adam normalises noise-level gradient elements: lr-sized differences are expected there


def test_no_cross_block_mfma_result_hazards():
    """ISA regression check (tools/check_mfma_hazards.py): no MFMA result is first read behind a basic-block
    boundary with fewer wait states than the compiler pads inside a block.  Round 1 found exactly that in
    ae_bwd_kernel (a run-time stage-timer branch after an MFMA chain): timing-dependent wrong results."""
    import subprocess, sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_mfma_hazards.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]


def test_hazard_scanner_flags_the_known_bad_pattern():
    """Self-test of tools/check_mfma_hazards.py on hand-written ISA: an accumulator read behind a conditional branch 3
    instructions after the MFMA (the round-1 bug) must be flagged; the same read behind an s_nop 9 in one block, or a
    dependent MFMA, must not."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("chk", os.path.join(ROOT, "tools", "check_mfma_hazards.py"))
    chk = importlib.util.module_from_spec(spec); spec.loader.exec_module(chk)
    bad = """
	v_mfma_f32_16x16x4_f32 a[0:3], v9, v159, a[0:3]
	s_and_saveexec_b64 s[2:3], s[68:69]
	s_cbranch_execz .LBB0_2
	s_memtime s[34:35]
.LBB0_2:
	s_or_b64 exec, exec, s[2:3]
	v_accvgpr_read_b32 v9, a3
""".splitlines()
    good = """
	v_mfma_f32_16x16x4_f32 a[0:3], v8, v131, a[0:3]
	v_mfma_f32_16x16x4_f32 a[0:3], v9, v159, a[0:3]
	s_nop 9
	v_accvgpr_read_b32 v9, a3
	s_cbranch_execz .LBB0_2
.LBB0_2:
	v_add_f32_e32 v1, v9, v9
""".splitlines()
    assert len(chk.scan_kernel("bad", bad)) == 1
    assert chk.scan_kernel("good", good) == []


def test_header_is_plain_c_and_links_from_c(tmp_path):
    """The drop-in boundary is a C ABI: include/signaltrain_hip.h compiles as strict C99 (no C++, no torch types), and a C program
    linked against libsignaltrain_hip.so can call the host-only entries (geometry, layout sizes, error reporting) without a GPU."""
    import shutil, subprocess, sys
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "use_abi.c"
    src.write_text('''
#include <stdio.h>
#include "signaltrain_hip.h"
int main(void)
{
    st_dims d;
    long long offs[40];
    if (st_geometry(1.0f, 4.0f, 0, 4, 256, &d) != ST_OK) { printf("geometry failed: %s\\n", st_last_error()); return 1; }
    d.prec = ST_PREC_F32X3; d.loss_scale = 0.0f; d.clip_all = 0;
    printf("%d %d %d %d %d %lld %zu\\n", d.L, d.T, d.OT, d.F, d.y, (long long)st_param_offsets(&d, (int64_t*)offs), st_workspace_bytes(&d));
    d.B = -1;
    if (st_workspace_bytes(&d) != 0) return 2;                      /* bad dims are rejected on the host ... */
    if (st_last_error()[0] == 0) return 3;                          /* ... with a message */
    return 0;
}
''')
    exe = tmp_path / "use_abi"
    lib_dir = os.path.join(root, "signaltrain_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"), str(src),
                        "-o", str(exe), "-L", lib_dir, "-l:libsignaltrain_hip.so", "-Wl,-rpath," + lib_dir],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    L, T, OT, F, y, total, wsb = (int(v) for v in r.stdout.split())
    assert (L, T, OT, F, y) == (8192, 25, 9, 513, 2048) and total == 4211096 and wsb > 100e6


def test_tuning_defaults_are_frozen():
    """The shipped values of the library's diagnostic switches (ST_TUNING_LIST in st_api.hip), in st_get_tuning's order.  A changed default has to be
    changed HERE as well -- it cannot ship unnoticed -- and tests/conftest.py asserts after every test that the live state equals these values.
    The accepted codes are exactly those of the table k_tuning_codes: each moves one switch (16 / 32: two), everything else -- retired switches, retired
    values of kept switches, arbitrary numbers -- is an error that names the code and changes nothing."""
    lib = _lib.load()
    n = lib.st_get_tuning(None, 0)
    cur, dflt = (C.c_int * n)(), (C.c_int * n)()
    assert lib.st_get_tuning(cur, n) == n and lib.st_tuning_defaults(dflt, n) == n
    frozen = [-1, 1, 1, 0, 0, 0, 3, 1, 0, 1, 1, 1, 0, 32, 16, 0, 1, 1, 3, 15]
    assert list(dflt) == frozen and list(cur) == frozen

    def state():
        assert lib.st_get_tuning(cur, n) == n
        return list(cur)
    # a switch is visible in the state and reset restores it
    assert lib.st_set_tuning(9500) == 0 and state() != frozen
    assert lib.st_reset_tuning() == 0 and state() == frozen
    # timing-only ablations (invalid results) are not in the product build: rejected, and the error names the offending code
    assert lib.st_set_tuning(9681) != 0 and b"9681" in lib.st_last_error()
    assert lib.st_set_tuning(96801) != 0 and b"96801" in lib.st_last_error()
    # one code of each retired switch; arbitrary unknown codes; retired values of kept switches
    rejected = [9800, 2002, 210, 1100, 6001, 3001, 4002, 9516, 9632, 9701, 5000, 9960, 9900, 9681, 96801] + [9999, 250, 99, 0, -1] + [9101, 9102, 101]
    for code in rejected:
        assert lib.st_set_tuning(code) != 0 and str(code).encode() in lib.st_last_error(), code
        assert state() == frozen, code
    # the table: switch index in st_get_tuning's order -> {code: stored value}
    table = {0: {8000: 0, 8001: 1, 8002: -1}, 1: {8200: 0, 8201: 1}, 2: {8300: 0, 8301: 1}, 3: {9400: 0, 9401: 1}, 4: {9300: 0, 9301: 1}, 5: {9200: 0, 9201: 1},
             6: {9100: 0, 9103: 3}, 7: {9600: 0, 9601: 1}, 8: {9690 + i: i for i in range(4)}, 9: {9950: 0, 9951: 1}, 10: {9500: 0, 9501: 1, 9580: 2, 9581: 1},
             11: {9000: 0, 9001: 1}, 12: {7000: 0, 7001: 1}, 15: {100: 0, 102: 2}, 16: {8100: 0, 8101: 1}, 17: {9970: 0, 9971: 1},
             18: {9540 + i: i for i in range(4)}, 19: {9560 + i: i for i in range(16)}}
    try:
        for idx, codes in table.items():
            for code, val in codes.items():
                want = list(frozen); want[idx] = val
                assert lib.st_set_tuning(code) == 0 and state() == want, code
                assert lib.st_reset_tuning() == 0 and state() == frozen
        for bk in (16, 32):                                    # the k-tile depth sets the analysis GEMM's and the family's together
            want = list(frozen); want[13] = want[14] = bk
            assert lib.st_set_tuning(bk) == 0 and state() == want, bk
            assert lib.st_reset_tuning() == 0 and state() == frozen
        # no run-time ablations
        assert lib.st_set_debug(0) == 0
        assert lib.st_set_debug(256) != 0 and b"ablation" in lib.st_last_error() and state() == frozen
    finally:
        lib.st_reset_tuning()


def test_kept_activation_bytes_follow_geometry_and_arithmetic():
    """Round 6: what a training-step forward keeps for the backward (st_ae_kept_activation_bytes) -- 2 nets x B * ceil(F / 16) row groups x 17 tiles of 1 KB where the
    autoencoder layers run in fp32 on the fused kernels, nothing elsewhere (16-bit layers, the wide path, the recompute switch) -- and the autoencoder workspace has room for it."""
    lib = _lib.load()
    d = _lib.st_dims()
    for B in (1, 3, 256, 1024):
        assert lib.st_geometry(1.0, 4.0, 0, 4, B, C.byref(d)) == 0
        for prec, keeps in ((0, True), (1, True), (3, True), (5, True), (2, False), (4, False)):       # f32, bf16 GEMMs, f16 GEMMs, f32x3 keep fp32 layers; bf16_all / f16_all do not
            d.prec = prec
            want = 2 * B * ((d.F + 15) // 16) * 17 * 1024 if keeps else 0
            assert lib.st_ae_kept_activation_bytes(C.byref(d)) == want, (B, prec)
            if keeps: assert lib.st_ae_bwd_ws_floats(C.byref(d)) * 4 > want and lib.st_workspace_bytes(C.byref(d)) > want
        d.prec = 0
        try:
            assert lib.st_set_tuning(8200) == 0 and lib.st_ae_kept_activation_bytes(C.byref(d)) == 0
        finally:
            assert lib.st_set_tuning(8201) == 0
    assert lib.st_geometry(8.0, 4.0, 0, 4, 64, C.byref(d)) == 0      # the 65536-sample window: wide path, feature-major activations of its own
    d.prec = 0
    assert lib.st_ae_kept_activation_bytes(C.byref(d)) == 0


def test_effective_precision_is_reported():
    """st_effective_prec = the arithmetic a call really runs.  Until round 4 the wide autoencoder path (T > 32 or OT > 16: the 65536-sample window, lean
    scale 2, shrink 1) needed an EVEN batch for 16-bit Linear layers and ran fp32 layers for odd ones -- reported, but a cliff.  Round 5: its weight-gradient
    GEMMs take 16-deep k-tiles when B * 528 is 16 mod 32, so the effective arithmetic equals the request for every geometry and every batch."""
    lib = _lib.load()
    d = _lib.st_dims()
    for scale, shrink in ((8.0, 4.0), (2.0, 4.0), (1.0, 1.0), (1.0, 4.0)):
        for B in (1, 3, 9, 63, 64):
            assert lib.st_geometry(scale, shrink, 0, 4, B, C.byref(d)) == 0
            for prec in (0, 1, 2, 3, 4, 5):
                d.prec = prec
                assert lib.st_effective_prec(C.byref(d)) == prec, (scale, shrink, B, prec)


@pytest.mark.parametrize("B,shrink", [(256, 4), (128, 4), (192, 4), (64, 4), (3, 4), (1, 4), (256, 8), (100, 2), (512, 4), (384, 4), (1024, 4)])
def test_nt128_worklist_covers_exactly_the_live_taps(B, shrink):
    """Round 5: the 128 x 128-tile synthesis GEMMs no longer multiply the structural zeros of the cropped transposed convolution
    (cls_fe_dft.py:112-113: of output frame t' only the taps n with N <= H t' + n < N + y survive the crop).  Host logic only (st_nt128_worklist):
    frames GEMM -- every live (frame, tap) lies in a listed tile, each listed tile gets its whole reduction exactly once per active slab and zeros
    in the others; data gradient -- every tile row's slices partition a k range that holds all its frames' live taps, every spectral column is
    produced exactly once per slab (tiles + the Nyquist entries), unused slabs are zero-filled.  B = 256: one workgroup per CU; B = 384 / 512: several
    rounds of the same list (the k-slice count is the cheapest by the builder's cost model)."""
    lib = _lib.load()
    ncus = 256
    d = _lib.geometry(1, shrink, 4, B)
    N, H, OT, y, F = d.N, d.H, d.OT, d.y, d.F
    KP = lib.st_kp(F)
    live_t = [t for t in range(OT) if H * t + N > N and H * t < N + y]        # frames with at least one tap inside the crop [N, N + y)
    t_lo, Tv = live_t[0], len(live_t)
    assert live_t == list(range(t_lo, t_lo + Tv))
    R = B * Tv

    def tap_range(t):
        return max(0, N - H * t), min(N, N + y - H * t)

    def entries(which):
        out = (C.c_uint * 1024)(); head = (C.c_int * 6)()
        n = lib.st_nt128_worklist(C.byref(d), which, ncus, out, 1024, head)
        assert 0 <= n <= 768
        ku = head[4] if n else 1
        ents = [dict(mt=out[i] & 255, nt=(out[i] >> 8) & 63, z=(out[i] >> 14) & 3, zf=(out[i] >> 16) & 3, kind=(out[i] >> 18) & 1,
                     k0=((out[i] >> 19) & 63) * ku, kl=(out[i] >> 25) * ku) for i in range(n)]
        for e in ents:
            e["k1"] = min(e["k0"] + e["kl"], head[5])
        return n, ents, list(head)

    # ---------------------------------------------------------------- frames GEMM: C[row][tap] over k in [0, KP)
    n, ents, head = entries(0)
    nsl = lib.st_synth_frame_slabs(C.byref(d))
    if n:
        assert head[0] == nsl and head[1] == 0 and head[3] == B and head[5] == KP // 32 and all(e["kind"] == 0 for e in ents)
        tiles = {}
        for e in ents:
            tiles.setdefault((e["mt"], e["nt"]), []).append(e)
        nacts = set()
        for (mt, nt), es in tiles.items():
            es.sort(key=lambda e: e["z"])
            nact = len(es); nacts.add(nact)
            assert [e["z"] for e in es] == list(range(nact)) and nact <= nsl
            assert es[0]["k0"] == 0 and es[-1]["k1"] == KP // 32
            assert all(es[i]["k1"] == es[i + 1]["k0"] for i in range(nact - 1))
            assert es[0]["zf"] == (nact if nact < nsl else 0) and all(e["zf"] == 0 for e in es[1:])       # slabs [nact, nsl) zero-filled once, by slice 0
        assert len(nacts) == 1
        for r in range(R):                                     # frame-major compact rows
            t = t_lo + r // B
            lo, hi = tap_range(t)
            for ntile in range(N // 128):
                if lo < 128 * ntile + 128 and hi > 128 * ntile:
                    assert (r // 128, ntile) in tiles, (r, t, ntile)
        if B % 128 == 0:                                       # one frame per tile row: nothing but live tiles is computed
            for (mt, nt) in tiles:
                lo, hi = tap_range(t_lo + (128 * mt) // B)
                assert lo < 128 * nt + 128 and hi > 128 * nt
        if (B, shrink) == (256, 4):
            assert len(tiles) == 84 and n == 252               # 84 of 112 tiles, three k-slices: one workgroup per CU
        if (B, shrink) == (512, 4):
            assert len(tiles) == 168 and n == 504              # two rounds of three k-slices
        if (B, shrink) == (384, 4):
            assert len(tiles) == 126 and n == 252              # two k-slices: one full round beats three slices in two rounds
    else:
        assert B >= 1024 or nsl > 3                            # B = 1024: 336 tiles, one slab -> a second round at 31 %: stays on gemm_kernel<4, ...>
    # ---------------------------------------------------------------- data gradient: C[row][spectral column] over the taps
    n, ents, head = entries(1)
    nsl = lib.st_synth_slabs(C.byref(d))
    if n:
        assert head[0] == nsl
        col_h, col_stride = head[1], head[2]
        assert (col_h, col_stride) == (F - 1, KP // 2)         # N = 1024: the Nyquist columns are kind-1 entries
        MT = (R + 127) // 128
        for mt in range(MT):
            rows = range(128 * mt, min(128 * mt + 128, R))
            lo = min(tap_range(t_lo + r // B)[0] for r in (rows[0], rows[-1])); hi = max(tap_range(t_lo + r // B)[1] for r in (rows[0], rows[-1]))
            mine = [e for e in ents if e["mt"] == mt]
            nyq = [e for e in mine if e["kind"] == 1]
            assert len(nyq) == 1 and 32 * nyq[0]["k0"] <= lo and 32 * nyq[0]["k1"] >= hi
            cols = sorted(set(e["nt"] for e in mine if e["kind"] == 0))
            assert cols == list(range(2 * (F - 1) // 128))
            for nt in cols:
                es = sorted((e for e in mine if e["kind"] == 0 and e["nt"] == nt), key=lambda e: e["z"])
                sl = len(es)
                assert [e["z"] for e in es] == list(range(sl)) and sl <= nsl and es[0]["zf"] == (sl if sl < nsl else 0) and all(e["zf"] == 0 for e in es[1:])
                assert 32 * es[0]["k0"] <= lo and 32 * es[-1]["k1"] >= hi
                assert all(es[i]["k1"] == es[i + 1]["k0"] for i in range(sl - 1))
                if B % 128 == 0:                               # no k-tile outside the live taps
                    assert 32 * es[0]["k0"] >= lo - 31 and 32 * es[-1]["k1"] <= hi + 31
        if (B, shrink) == (256, 4):
            assert n == 240 + 14 and max(e["kl"] for e in ents if e["kind"] == 0) == 12      # 3 / 2 / 1 slices of <= 384 taps, Nyquist columns on the 14 spare CUs
        if (B, shrink) == (512, 4):
            assert n == 480 + 28 and max(e["kl"] for e in ents if e["kind"] == 0) == 12
    else:
        assert B > 1024


def test_frame_major_division_bound_and_worklist_is_a_pure_function():
    """ADVICE round 5.  (1) The frame-major row order splits a compact row r into (r // B, r % B) with a multiply-high by floor(2^32 / B) + 1
    (st_gemm.h RowMap::magic); that is exact only while r * B < 2^32.  st_fm_div_exact is the host-side gate every frame-major switch asks: where it
    says yes the multiply-high is exact for the rows near every multiple of B up to R (brute force on the boundary rows, where it fails first), and
    just past the bound a wrong quotient exists (B = 32768 at 7 live frames: r >= 2^17 + ...).  (2) st_nt128_worklist with an explicit CU count
    is a pure function of its arguments: two different counts give the lists their own cost model asks for, never the probed device's."""
    lib = _lib.load()

    def mulhi_div(r, B):
        magic = (1 << 32) // B + 1
        return (r * magic) >> 32

    def first_wrong(R, B):
        for q in range(1, R // B + 1):            # the quotient is first wrong just below a multiple of B (or at it)
            for r in (q * B - 1, q * B):
                if r < R and mulhi_div(r, B) != r // B:
                    return r
        return None

    for B, Tv in [(256, 7), (1024, 23), (4096, 7), (24000, 7), (32768, 7), (40000, 7), (65536, 23), (9000, 46)]:
        R = B * Tv
        ok = lib.st_fm_div_exact(R, B)
        assert ok == (1 if R * B < (1 << 32) else 0)
        if ok:
            assert first_wrong(R, B) is None
    assert lib.st_fm_div_exact(7 * 32768, 32768) == 0 and first_wrong(7 * 32768, 32768) is not None       # the advisor's case really is wrong without the gate
    # (2) purity in ncus: B = 3 has 1 tile row -- with 8 "CUs" the one-round rule fails, the crop rule (>= 10 % of the taps) still holds: the list does not depend on a device
    d = _lib.geometry(1, 4, 4, 256)
    out = (C.c_uint * 1024)(); head = (C.c_int * 6)()
    n256 = lib.st_nt128_worklist(C.byref(d), 0, 256, out, 1024, head); a = list(out[:n256])
    n256b = lib.st_nt128_worklist(C.byref(d), 0, 256, out, 1024, head); b = list(out[:n256b])
    n304 = lib.st_nt128_worklist(C.byref(d), 0, 304, out, 1024, head)
    assert n256 == n256b == 252 and a == b and n304 > 0


def test_run_train_accepts_the_reference_effect_keys():
    """run_train.py --effect: the reference's keys (run_train.py:55-80).  comp_4c / comp_large / files are built (argument parsing only here: the run itself
    needs a GPU); the reference's other keys and unknown ones exit with a message that names what is available, as the reference does for unknown effects."""
    import subprocess, sys
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "run_train.py"), *a], capture_output=True, text=True, timeout=300)
    r = run("--effect", "denoise")
    assert r.returncode != 0 and "does not build" in r.stderr and "comp_large" in r.stderr
    r = run("--effect", "bogus")
    assert r.returncode != 0 and "is not yet added" in r.stderr
    r = run("--effect", "comp_large", "--target", "nope")
    assert r.returncode != 0 and "invalid target type" in r.stderr            # comp_large passed the effect check (argparse used to reject it)


def test_dims_edge_cases_are_refused_with_a_message():
    """Edge cases at the C ABI, before any launch (host-side validation only: runs without a GPU).  Empty batch, a geometry that is not the reference's
    (F != N/2 + 1, y != (OT - 1) H - N: nn_proc.py:357-385), more knobs than the fused kernels carry, an unknown arithmetic level, a negative / infinite loss
    scale, and the MAXIMUM sizes: batches whose row count or operand sizes leave the 24-bit row / 32-bit element indexing of the kernels (include/signaltrain_hip.h)
    are refused by name instead of wrapping around.  The largest admitted batch still reports a layout and a workspace size."""
    import ctypes as C
    lib = _lib.load()
    good = _lib.geometry(1, 4, 4, 256)
    assert lib.st_param_offsets(C.byref(good), None) > 0 and lib.st_workspace_bytes(C.byref(good)) > 0

    def refused(mut, needle):
        d = good.with_batch(good.B); mut(d)
        assert lib.st_param_offsets(C.byref(d), None) == -1, needle
        msg = lib.st_last_error().decode()
        assert needle in msg, (needle, msg)
        # a compute entry refuses the same dims before it looks at any pointer
        assert lib.st_analysis_fwd(C.byref(d), None, None, None, 0.5, None, None, None, None, None) < 0
    refused(lambda d: setattr(d, "B", 0), "non-positive")
    refused(lambda d: setattr(d, "B", -3), "non-positive")
    refused(lambda d: setattr(d, "K", -1), "non-positive")
    refused(lambda d: setattr(d, "K", 17), "at most 16 knobs")
    refused(lambda d: setattr(d, "F", d.F - 1), "F must be N/2+1")
    refused(lambda d: setattr(d, "y", d.y + 4), "y must equal")
    refused(lambda d: setattr(d, "OT", d.T + 1), "y must equal")           # OT > T also breaks y = (OT - 1) H - N first
    refused(lambda d: setattr(d, "prec", 99), "ST_PREC")
    refused(lambda d: setattr(d, "loss_scale", -1.0), "loss_scale")
    refused(lambda d: setattr(d, "loss_scale", float("inf")), "loss_scale")
    refused(lambda d: setattr(d, "L", d.L + 2), "required")                # ragged window length: L % 4
    # maximum sizes: rows B * T < 2^24, B * T * KP and B * (L + 2 N) < 2^30 elements
    kp = int(lib.st_kp(good.F))
    b_max = min(((1 << 24) - 1) // good.T, ((1 << 30) - 1) // (good.T * kp), ((1 << 30) - 1) // (good.L + 2 * good.N))
    ok = good.with_batch(b_max)
    assert lib.st_param_offsets(C.byref(ok), None) > 0, lib.st_last_error()
    assert lib.st_workspace_bytes(C.byref(ok)) > lib.st_workspace_bytes(C.byref(good))
    refused(lambda d: setattr(d, "B", b_max + 1), "batch too large")
    refused(lambda d: setattr(d, "B", 1 << 30), "batch too large")
    # the 65536-sample window has its own, smaller limit
    wide = _lib.geometry(8, 4, 4, 64)
    kpw = int(lib.st_kp(wide.F))
    bw = min(((1 << 24) - 1) // wide.T, ((1 << 30) - 1) // (wide.T * kpw), ((1 << 30) - 1) // (wide.L + 2 * wide.N))
    assert bw < b_max and lib.st_param_offsets(C.byref(wide.with_batch(bw)), None) > 0
    assert lib.st_param_offsets(C.byref(wide.with_batch(bw + 1)), None) == -1 and b"batch too large" in lib.st_last_error()
    # a null dims pointer
    assert lib.st_param_offsets(None, None) == -1 and b"null dims" in lib.st_last_error()


def test_workspace_of_the_fp32_level_bounds_every_arithmetic_level():
    """st_workspace_bytes depends on the arithmetic level of the dims (fp32 autoencoder layers keep their activations for the backward, the 16-bit levels carry
    operand copies and the h4 exchange of the split backward).  Hosts size ONE workspace and may switch levels on a live engine (StepEngine.set_arithmetic,
    st_model.set_compute_dtype): the size reported for ST_PREC_F32 must bound every other level's, at every geometry / batch / knob count / clip scope --
    and StepEngine sizes by the maximum anyway."""
    import ctypes as C
    lib = _lib.load()
    for scale, scheme in ((1, "lean"), (2, "lean"), (2, "legacy"), (8, "lean")):
        for shrink in (1, 4, 8):
            for B in (1, 3, 64, 130, 256, 257, 1024):
                for K in (0, 4, 16):
                    d = _lib.geometry(scale, shrink, K, B, scale_scheme=scheme)
                    base = lib.st_workspace_bytes(C.byref(d.with_arith(prec=_lib.PREC["f32"], loss_scale=0.0, clip_all=0)))
                    assert base > 0
                    for name, p in _lib.PREC.items():
                        for ca in (0, 1):
                            n = lib.st_workspace_bytes(C.byref(d.with_arith(prec=p, loss_scale=(4096.0 if name.startswith("f16") else 0.0), clip_all=ca)))
                            assert 0 < n <= base, (scale, scheme, shrink, B, K, name, ca, n, base)


def test_one_workspace_serves_every_smaller_batch():
    """st_workspace_bytes is NOT monotonic in the batch: the split-K slab counts of the weight-gradient / synthesis GEMMs are picked per batch, so e.g. 585 windows of 8192
    samples need 85.6 MB MORE than 586 do, and 93 windows of 65536 samples 63 MB more than 94.  A host that sizes its workspace for its largest batch and then runs a smaller
    one (a last partial batch, predict_long's remainder, a validation batch) would be written past the end.  engine.workspace_bytes_upto is what StepEngine allocates: the
    maximum over every batch 1 .. max_batch, every arithmetic level and clip scope -- the C entry st_workspace_bytes_max (INTEGRATION.md "Sizing the workspace")."""
    import ctypes as C
    from signaltrain_amd.engine import workspace_bytes_upto
    lib = _lib.load()
    seen_non_monotonic = False
    for scale, shrink, bmax in ((1, 4, 586), (1, 4, 600), (1, 4, 256), (1, 1, 179), (8, 4, 94), (8, 4, 64), (2, 4, 342)):
        d = _lib.geometry(scale, shrink, 4, bmax)
        cap = workspace_bytes_upto(lib, d, bmax)
        own = {name: lib.st_workspace_bytes(C.byref(d.with_arith(prec=p))) for name, p in _lib.PREC.items()}
        assert cap >= max(own.values())
        for b in range(1, bmax + 1):
            for name, p in _lib.PREC.items():
                n = lib.st_workspace_bytes(C.byref(d.with_batch(b).with_arith(prec=p, clip_all=int(name.startswith("f16")))))
                assert 0 < n <= cap, (scale, shrink, bmax, b, name, n, cap)
                seen_non_monotonic |= n > own[name]
    assert seen_non_monotonic          # the property this test exists for (if the library ever becomes monotonic, drop this line and the loop stays a valid guarantee)
    # st_workspace_bytes_max IS that maximum (the C entry the engine calls), also from dims that carry a 16-bit level, and 0 for bad dims
    d = _lib.geometry(1, 4, 4, 600)
    brute = max(lib.st_workspace_bytes(C.byref(d.with_batch(b).with_arith(prec=p, clip_all=ca))) for b in range(1, 601) for p in _lib.PREC.values() for ca in (0, 1))
    assert lib.st_workspace_bytes_max(C.byref(d)) == brute == lib.st_workspace_bytes_max(C.byref(d.with_arith(prec=_lib.PREC["bf16_all"], clip_all=1)))
    assert lib.st_workspace_bytes_max(C.byref(d.with_batch(0))) == 0


# ------------------------------------------------------------------------------ the host gate of the generic front end (st_fe_supported)
FE_DIV_TABLE = [      # (B, L, C, KW, hop, pad): the two largest exact row splits of KW = 16, hop = 4 and the first inexact ones above them
    (1, 262144, 16, 16, 4, 0), (16, 65536, 16, 16, 4, 0),      # R * T = 4 294 574 089 and 4 293 394 576: below 2^32
    (2, 262144, 16, 16, 4, 0), (17, 65536, 16, 16, 4, 0),      # over: the last row's quotient is wrong
]
FE_ORDINARY = [(1, 64, 16, 16, 4, 0), (3, 256, 16, 16, 4, 16), (5, 1000, 112, 48, 20, 12), (7, 1204, 16, 64, 100, 0), (2, 400, 32, 64, 12, 128),
               (9, 4096, 208, 144, 36, 72), (16, 1616, 32, 16, 8, 0), (3, 8192, 512, 1024, 256, 512), (16, 8192, 16, 16, 4, 8), (3, 8192, 1024, 2048, 1024, 1024),
               (256, 8192, 1056, 1024, 384, 1024)]


def fe_violations(B, L, C, KW, hop, pad):
    """The limits of include/signaltrain_hip.h (st_fe_supported) in Python integers: the names of the violated ones."""
    if min(B, L, C, KW, hop) <= 0 or pad < 0:
        return ["non-positive"]
    bad = [n for n, v, m in (("KW%16", KW, 16), ("C%16", C, 16), ("hop%4", hop, 4), ("pad%4", pad, 4), ("L%4", L, 4)) if v % m]
    if bad:
        return bad
    if KW > L + 2 * pad:
        return ["no frame"]
    T = (L + 2 * pad - KW) // hop + 1
    R, wide = B * T, L + 2 * pad + 2 * KW
    lim = [("rows", R, 1 << 24), ("samples", wide, 1 << 24), ("B*L", B * L, 1 << 30), ("B*wide", B * wide, 1 << 30), ("R*KW", R * KW, 1 << 30),
           ("R*C", R * C, 1 << 30), ("C*KW", C * KW, 1 << 30), ("split", (R - 1) * T, 1 << 32)]
    return [n for n, v, m in lim if v >= m]


def test_fe_gate_is_exactly_the_row_split_bound():
    """RowMap::split (st_gemm.h) divides a compact row r < B * T by T with a multiply-high by floor(2^32 / T) + 1.  st_fe_supported says yes exactly where that is the
    true quotient for every row (brute force on the rows next to every multiple of T, where it fails first), and at the two refused shapes the brute force really finds a
    wrong quotient: without the gate the last row's frame index would be -1."""
    lib = _lib.load()

    def first_wrong(R, T):
        magic = (1 << 32) // T + 1
        for q in range(1, R // T + 1):
            for r in (q * T - 1, q * T):
                if r < R and (r * magic) >> 32 != r // T:
                    return r
        return None

    for s in FE_DIV_TABLE + FE_ORDINARY:
        B, L, C_, KW, hop, pad = s
        T = lib.st_fe_frames(L, KW, hop, pad); R = B * T
        wrong = first_wrong(R, T)
        assert lib.st_fe_supported(*s) == (1 if wrong is None else 0), (s, wrong)
        assert (wrong is None) == ((R - 1) * T < (1 << 32)), (s, wrong)
    assert [lib.st_fe_supported(*s) for s in FE_DIV_TABLE] == [1, 1, 0, 0]
    assert first_wrong(2 * 65533, 65533) == 2 * 65533 - 1 and first_wrong(17 * 16381, 16381) == 17 * 16381 - 1      # the last row, as recorded
    # every compute entry and the workspace size refuse such a shape on the host, by name, before they look at a pointer
    for s in FE_DIV_TABLE[2:]:
        B, L, C_, KW, hop, pad = s
        T = lib.st_fe_frames(L, KW, hop, pad)
        assert lib.st_fe_ws_floats(*s) == 0
        for rc in (lib.st_fe_analysis_fwd(None, B, L, None, None, C_, KW, hop, pad, None, None),
                   lib.st_fe_analysis_bwd(None, B, L, None, C_, KW, hop, pad, None, None, None, None, None, None),
                   lib.st_fe_synthesis_fwd(None, B, T, None, C_, KW, hop, pad, None, None, None),
                   lib.st_fe_synthesis_bwd(None, B, T, None, C_, KW, hop, pad, None, None, None, None, None)):
            assert rc == -1 and b"row split" in lib.st_last_error(), (s, rc, lib.st_last_error())


FE_LIMIT_PAIRS = [      # (limit, a shape just inside it, a shape just outside it)
    ("rows", (65535, 1036, 16, 16, 4, 0), (65536, 1036, 16, 16, 4, 0)),                          # T = 256: R = 2^24 - 256 | 2^24
    ("samples", (1, (1 << 24) - 36, 16, 16, 512, 0), (1, (1 << 24) - 32, 16, 16, 512, 0)),      # L + 2 KW = 2^24 - 4 | 2^24
    ("B*L", (1024, (1 << 20) - 36, 16, 16, 4096, 0), (1024, 1 << 20, 16, 16, 4096, 0)),        # B * L = 2^30 (then B * (L + 2 KW) is over as well)
    ("B*wide", (1024, (1 << 20) - 36, 16, 16, 4096, 0), (1024, (1 << 20) - 32, 16, 16, 4096, 0)),      # B * L < 2^30 <= B * (L + 2 KW)
    ("R*KW", (1, 163832, 16, 32768, 4, 0), (1, 163836, 16, 32768, 4, 0)),                       # T = 32767 | 32768 frames of 32768 taps
    ("R*C", (1, 131080, 32768, 16, 4, 0), (1, 131084, 32768, 16, 4, 0)),                        # T = 32767 | 32768 frames of 32768 channels
    ("C*KW", (1, 32768, 32752, 32768, 4, 0), (1, 32768, 32768, 32768, 4, 0)),
    ("split", (1, 262144, 16, 16, 4, 0), (1, 262160, 16, 16, 4, 0)),                            # T = 65533 | 65537: T (T - 1) crosses 2^32
    ("split", (16, 65536, 16, 16, 4, 0), (17, 65536, 16, 16, 4, 0)),
    ("KW%16", (2, 256, 32, 48, 8, 8), (2, 256, 32, 40, 8, 8)),
    ("C%16", (2, 256, 48, 32, 8, 8), (2, 256, 40, 32, 8, 8)),
    ("hop%4", (2, 256, 32, 32, 12, 8), (2, 256, 32, 32, 10, 8)),
    ("pad%4", (2, 256, 32, 32, 8, 12), (2, 256, 32, 32, 8, 10)),
    ("L%4", (2, 260, 32, 32, 8, 8), (2, 258, 32, 32, 8, 8)),
    ("no frame", (1, 64, 16, 80, 4, 8), (1, 64, 16, 96, 4, 8)),                                  # KW = | > L + 2 pad: T = 1 | 0
    ("non-positive", (1, 64, 16, 16, 4, 0), (0, 64, 16, 16, 4, 0)),
    ("non-positive", (1, 64, 16, 16, 4, 0), (1, 64, 16, 16, 4, -4)),
    ("non-positive", (1, 64, 16, 16, 4, 0), (1, 64, 16, 16, 0, 0)),
]


def test_fe_gate_limits_one_shape_inside_and_one_outside_each():
    """Every limit of st_fe_supported against integer arithmetic in Python: the shape just inside violates nothing and is accepted, the shape just outside violates
    the named limit (and, except where one limit implies another, only that one) and is refused -- by the predicate, by the workspace size and, with a message, by a
    compute entry that has not looked at a pointer yet.  A seeded random sweep around the limits then has predicate and Python agree shape by shape."""
    lib = _lib.load()
    implied = {"B*L": {"B*L", "B*wide"}}
    for name, inside, outside in FE_LIMIT_PAIRS:
        assert fe_violations(*inside) == [] and lib.st_fe_supported(*inside) == 1, (name, inside, fe_violations(*inside))
        assert set(fe_violations(*outside)) == implied.get(name, {name}), (name, outside, fe_violations(*outside))
        assert lib.st_fe_supported(*outside) == 0 and lib.st_fe_ws_floats(*outside) == 0, (name, outside)
        B, L, C_, KW, hop, pad = outside
        assert lib.st_fe_analysis_fwd(None, B, L, None, None, C_, KW, hop, pad, None, None) == -1 and len(lib.st_last_error()) > 20
        assert b"null" not in lib.st_last_error(), lib.st_last_error()
    rng = np.random.default_rng(11)
    seen = {0: 0, 1: 0}
    for _ in range(4000):
        KW = 16 * int(rng.integers(1, 5)) if rng.random() < 0.8 else 16 * int(rng.integers(1, 4096))
        C_ = 16 * int(rng.integers(1, 5)) if rng.random() < 0.8 else 16 * int(rng.integers(1, 4096))
        hop = 4 * int(rng.integers(1, 2 ** int(rng.integers(1, 12))))
        pad = 4 * int(rng.integers(0, 64))
        L = 4 * int(rng.integers(1, 2 ** int(rng.integers(3, 23))))
        B = int(rng.integers(1, 2 ** int(rng.integers(1, 18))))
        s = (B, L, C_, KW, hop, pad)
        ok = lib.st_fe_supported(*s)
        assert ok == (0 if fe_violations(*s) else 1), (s, fe_violations(*s))
        seen[ok] += 1
    assert min(seen.values()) > 200, seen      # the sweep really reaches both sides


def test_fe_workspace_size_is_zero_exactly_where_the_gate_refuses():
    """st_fe_ws_floats is 0 exactly where st_fe_supported is 0 (like st_workspace_bytes on bad dims); where the shape is accepted it covers what st_fe_analysis_bwd
    and st_fe_synthesis_bwd carve: ns slabs of the weight gradient, the frame buffer and the padded gradient signal, ns = clamp(B * T // 200, 1, 16)
    (the tuning defaults frozen by test_tuning_defaults_are_frozen)."""
    lib = _lib.load()
    shapes = FE_DIV_TABLE + FE_ORDINARY + [s for _, a, b in FE_LIMIT_PAIRS for s in (a, b)]
    for s in shapes:
        B, L, C_, KW, hop, pad = s
        n = lib.st_fe_ws_floats(*s)
        assert (n == 0) == (lib.st_fe_supported(*s) == 0), s
        if n:
            T = (L + 2 * pad - KW) // hop + 1
            assert T == lib.st_fe_frames(L, KW, hop, pad)
            ns = min(max(B * T // 200, 1), 16)
            assert n >= ns * C_ * KW + B * T * KW + B * (L + 2 * pad), (s, n)


def test_model_dims_are_refused_past_the_row_split_bound():
    """check_dims carries the same rule for the model's framed GEMMs: (B * T - 1) * T < 2^32 (their live-frame maps divide by Tv <= T).  No training geometry comes
    near it -- every configuration of BASELINE.md and the largest admitted batches of test_dims_edge_cases_are_refused_with_a_message still report a layout."""
    lib = _lib.load()
    d = _lib.geometry(1, 4, 4, 1)
    d.T = 65536
    assert (d.B * d.T - 1) * d.T < (1 << 32) and lib.st_param_offsets(C.byref(d), None) > 0, lib.st_last_error()
    d.T = 65537
    assert (d.B * d.T - 1) * d.T >= (1 << 32) and d.B * d.T < (1 << 24) and d.B * d.T * lib.st_kp(d.F) < (1 << 30)      # no other limit is in the way
    assert lib.st_param_offsets(C.byref(d), None) == -1 and b"row split" in lib.st_last_error()
    assert lib.st_workspace_bytes(C.byref(d)) == 0
    assert lib.st_analysis_fwd(C.byref(d), None, None, None, 0.5, None, None, None, None, None) < 0 and b"row split" in lib.st_last_error()
    d.B, d.T = 3, 40000                                          # R = 120000 rows: 119999 * 40000 >= 2^32
    assert d.B * d.T * lib.st_kp(d.F) < (1 << 30) and lib.st_param_offsets(C.byref(d), None) == -1 and b"row split" in lib.st_last_error()
    for scale, scheme, batches in ((1, "lean", (32, 256, 1024, 2048)), (8, "lean", (64, 512)), (2, "legacy", (256,))):
        for Bn in batches:
            g = _lib.geometry(scale, 4, 4, Bn, scale_scheme=scheme)
            assert (g.B * g.T - 1) * g.T < (1 << 32) // 100
            assert lib.st_param_offsets(C.byref(g), None) > 0 and lib.st_workspace_bytes(C.byref(g)) > 0, (scale, scheme, Bn, lib.st_last_error())


# ---------------------------------------------------------------------------------------------- the (ft, hop, frame) sizes of tests/test_gpu_dims_sweep.py
def _dims_of_row(shape, B=3, K=4):
    from tests import dims_table as D
    g = D.geo_of(shape)
    d = _lib.st_dims()
    d.B, d.L, d.N, d.H, d.T, d.OT, d.F, d.K, d.y = B, g["L"], g["N"], g["H"], g["T"], g["OT"], g["F"], K, g["y"]
    return d


def _sweep_case_ids():
    from tests import dims_table as D
    return [f"{r}-B{b}-K{k}-seed{s}-{kind}" for r, b, k, s, kind in D.sweep_cases()]


def _sweep_cases():
    from tests import dims_table as D
    return D.sweep_cases()


@pytest.mark.parametrize("case", _sweep_cases(), ids=_sweep_case_ids())
def test_sweep_inputs_leave_fp32_arithmetic_inside_a_quarter_of_the_tolerance(case):
    """A GPU comparison at tolerance tau means something only if fp32 arithmetic itself is well inside tau on those inputs: for every (shape, batch, knobs,
    seed) of the dims sweep, the oracle run in float32 agrees with its float64 run to tau / 4 on every tensor the sweep compares (y_hat, mag, mag_hat, the
    loss at 1e-4; the 40 gradients at 1e-4 per-op and 2e-4 fused; the per-op intermediates of run_all; the L1 norm and, on the rolled inputs of both train
    steps, the loss and the parameters of run_fused: dims_table.input_condition), with gpu_checks' scaling.  CPU only."""
    from tests import dims_table as D
    from tests import gpu_checks as G                        # make_case only (numpy); no GPU touched
    row, B, K, seed, kind = case
    geo = D.geo_of(row)
    _, X, Y, KN, P = G.make_case(B, seed, K=K, geo=geo)
    c = D.input_condition(geo, X, Y, KN, P, kind)
    assert len(c) == {"per-op": 62, "fused": 49}[kind]
    over = {k: v for k, v in c.items() if not v <= D.condition_bound(k, kind)}
    assert not over, (case, over)


def test_host_size_functions_at_every_sweep_row():
    """Host only: layout and workspace arithmetic at the sizes st_geometry never produces -- positive sizes, parameter offsets aligned to 4 floats, the
    forward state inside the workspace, and one workspace for every smaller batch no smaller than the exact one."""
    from tests import dims_table as D
    lib = _lib.load()
    for row in D.ROWS:
        for B, K in ((3, 4), (1, 0), (2, 16)):
            d = _dims_of_row(row, B, K)
            offs = (C.c_int64 * 40)()
            total = lib.st_param_offsets(C.byref(d), offs)
            assert total > 0 and all(o % 4 == 0 for o in offs) and list(offs) == sorted(set(offs)) and offs[39] < total, (row, lib.st_last_error())
            from signaltrain_amd.engine import param_shapes
            assert total >= sum(int(np.prod(s)) for s in param_shapes(d)) > total - 4 * 40
            for prec in (0, 2, 4, 5):
                d.prec = prec
                nb = lib.st_workspace_bytes(C.byref(d))
                assert nb > 0 and nb % 4 == 0 and lib.st_workspace_bytes_max(C.byref(d)) >= nb, (row, prec)
                w8 = (C.c_int64 * 8)()
                assert lib.st_workspace_offsets(C.byref(d), w8) == 0
                KP = lib.st_kp(d.F)
                sizes = [B * d.T * d.F] * 4 + [B * d.OT * d.F] * 2 + [B * d.OT * KP, B * d.y]
                spans = sorted((o, o + n) for o, n in zip(w8, sizes))
                assert spans[0][0] >= 0 and spans[-1][1] * 4 <= nb and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (row, prec, spans)
            d.prec = 0
            assert lib.st_norm_partials(C.byref(d)) > 0 and lib.st_synth_slabs(C.byref(d)) > 0
            assert lib.st_ola_loss_partials(C.byref(d)) == B * -(-d.y // 256)
            assert lib.st_ae_acts_floats(C.byref(d)) == B * d.F * (272 + K + d.OT)


def test_a_frame_count_that_drops_live_frames_is_refused_by_name():
    """check_dims: H T >= L + N.  Frame t starts at H t - N; the reference's Conv1d has (L + N) // H + 1 of them and its first Linear layer raises on any other
    count.  Here a larger T (all-padding frames: st_geometry emits it) and the omission of the one frame that starts exactly at L stay legal; a T that drops a
    frame overlapping the signal comes back as -1 / 0 from every host size function, with the rule and the four numbers in st_last_error()."""
    from tests import dims_table as D
    lib = _lib.load()
    for name, shape in D.REFUSED.items():
        N, H, L, T, OT = shape
        assert H * T < L + N
        d = _dims_of_row(shape)
        for fn, want in (("st_param_offsets", -1), ("st_workspace_bytes", 0), ("st_workspace_bytes_max", 0), ("st_norm_partials", 0), ("st_ola_loss_partials", 0),
                         ("st_synth_slabs", 0), ("st_ae_acts_floats", 0), ("st_ae_fwd_ws_floats", 0), ("st_ae_bwd_ws_floats", 0), ("st_ae_fwd_partials", 0),
                         ("st_synth_frame_slabs", 0), ("st_wgrad_ws_floats", 0), ("st_ae_kept_activation_bytes", 0), ("st_model_input_grad_ws_floats", 0)):
            lib.st_workspace_bytes(C.byref(_dims_of_row("n256")))        # a good call in between: the message must come from THIS refusal
            got = lib.st_param_offsets(C.byref(d), None) if fn == "st_param_offsets" else getattr(lib, fn)(C.byref(d))
            msg = lib.st_last_error()
            assert got == want and b"T too small" in msg, (name, fn, got, msg)
            assert all(f"{k}={v}".encode() in msg for k, v in (("T", T), ("L", L), ("N", N), ("H", H))), msg
        assert lib.st_workspace_offsets(C.byref(d), (C.c_int64 * 8)()) == -1
        assert lib.st_analysis_fwd(C.byref(d), None, None, None, 0.5, None, None, None, None, None) == -1 and b"T too small" in lib.st_last_error()
        d.T = -(-(L + N) // H)                                   # the smallest legal T
        d.OT = min(d.OT, d.T); d.y = (d.OT - 1) * H - N
        assert lib.st_param_offsets(C.byref(d), None) > 0, (name, lib.st_last_error())
    # nothing st_geometry produces violates the rule: ceil(L / H) + ceil(N / H) >= (L + N) / H
    for scale in (1, 2, 4, 8):
        for shrink in (1, 2, 4, 8):
            for scheme in ("lean", "legacy"):
                g = _lib.geometry(scale, shrink, 4, 2, scale_scheme=scheme)
                assert g.H * g.T >= g.L + g.N and lib.st_workspace_bytes(C.byref(g)) > 0, (scale, shrink, scheme, lib.st_last_error())
    # the standalone modules build their own dims: one autoencoder alone at the 89 output frames of scale 4 / shrink 1
    d = _lib.st_dims(); d.B, d.N, d.F, d.T, d.OT, d.K, d.H = 1, 1024, 513, 89, 89, 3, 384
    d.y = (d.OT - 1) * d.H - d.N; d.L = d.y
    assert lib.st_ae_acts_floats(C.byref(d)) == 513 * (272 + 3 + 89), lib.st_last_error()
