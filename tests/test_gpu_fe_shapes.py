"""Shape sweep of the generic learned-basis front end (st_fe_* of include/signaltrain_hip.h) through the C ABI.

Every entry -- analysis / synthesis, forward / backward, with their optional outputs present and NULL -- against float64 torch conv1d /
conv_transpose1d (and its autograd) on the CPU from the same fp32 inputs, at the smallest shapes that reach each edge of the framed GEMM family:
a single ragged tile, a single k-tile, frames wholly in the padding, hop that does not divide the window, gaps between frames, samples no frame uses,
a column tile crossed, the XCD swizzle with a workgroup count that is no multiple of 8 and its many-rows branch, every split-K regime of the
weight-gradient GEMM (1, 5 with a ragged last slice, 16 with an empty last slice) and the largest row counts whose (window, frame) split is still exact.

Tile arithmetic (st_gemm.h): launch<2,16> = 64 x 96 tiles, launch<3,16> = 96 x 96 tiles, k-tiles of 16; split-K = clamp(R / 200, 1, 16) slices rounded
up to 32 rows; the swizzle is active from 16 workgroups.  Tolerance: the project's max|got - ref| <= 1e-4 max|ref| per tensor.  Outputs live inside
larger buffers filled with a sentinel that must survive on both sides; workspaces are st_fe_ws_floats() floats with a sentinel tail.

The shapes past the exact row split are never launched: st_fe_supported must say 0 on the host first, and the entries must then refuse them."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from signaltrain_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4            # BASELINE.json north_star, as tests/gpu_checks.py and test_dct_front_end_golden_and_autograd
SENT = 12345.0        # sentinel of the guard bands (and of every workspace before the call: nothing may rely on its contents)
GUARD = 1024          # floats on either side of an output (keeps the 16-byte alignment of the view)

# (B, L, C, KW, hop, pad)
ANALYSIS = {
    "1-one-ragged-tile-one-ktile": (1, 64, 16, 16, 4, 0),             # R = 13: below one 64-row tile; KW = one k-tile; pad = 0
    "2-pad-eq-KW-dead-frames": (3, 256, 16, 16, 4, 16),               # frames 0 and T-1 lie in the padding; R = 207: four 64-row tiles, the last ragged
    "3-column-tile-crossed-hop-not-dividing": (5, 1000, 112, 48, 20, 12),      # 96 < C < 192; three k-tiles; 16 trailing padded samples (4 real) in no frame
    "4-hop-gt-KW-gaps": (7, 1204, 16, 64, 100, 0),
    "5-pad-gt-KW": (2, 400, 32, 64, 12, 128),                         # several dead frames at each end
    "6-splitk5-ragged-slice-swizzle51": (9, 4096, 208, 144, 36, 72),  # R = 1026: split-K 5 x 224 rows (last 130); forward grid 3 x 17 = 51 workgroups; wgrad 3 x 2 x 5
    "7-splitk16-empty-last-slice": (16, 1616, 32, 16, 8, 0),          # T = 201, R = 3216: 16 slices of 224, slice 14 holds 80 rows, slice 15 starts past R
    "8-module-512-1024-256": (3, 8192, 512, 1024, 256, 512),
    "9-many-tile-rows-swizzle-ny-gt-nx": (16, 8192, 16, 16, 4, 8),    # R = 32784: 513 x 1 tiles, split-K 16
    "10a-largest-exact-split-B1": (1, 262144, 16, 16, 4, 0),          # T = 65533: R * T = 4 294 574 089 < 2^32
    "10b-largest-exact-split-B16": (16, 65536, 16, 16, 4, 0),         # T = 16381: R * T = 4 293 394 576 < 2^32
}
REFUSED = [(2, 262144, 16, 16, 4, 0), (17, 65536, 16, 16, 4, 0)]      # (B*T - 1) * T >= 2^32: the last row's frame index would be -1


def frames_of(L, KW, hop, pad):
    return (L + 2 * pad - KW) // hop + 1


def synth_cases():
    """(B, T, C, KW, hop, crop): T, C, KW, hop of the analysis shapes 1-9 with crop = pad; crop = 0 for shapes 3 and 6; shape 8 with crop != pad."""
    out = {}
    for name, (B, L, Cn, KW, hop, pad) in ANALYSIS.items():
        if name.startswith("10"):
            continue
        T = frames_of(L, KW, hop, pad)
        out[name] = (B, T, Cn, KW, hop, pad)
        if name[0] in "36":
            out[name + "-crop0"] = (B, T, Cn, KW, hop, 0)
        if name[0] == "8":
            out[name + "-crop256"] = (B, T, Cn, KW, hop, 256)
    return out


SYNTHESIS = synth_cases()


def lib():
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


class Guarded:
    """An output of n floats inside a larger buffer pre-filled with the sentinel."""

    def __init__(self, n, tail_only=False):
        self.head = 0 if tail_only else GUARD
        self.buf = torch.full((self.head + n + GUARD,), SENT, device=DEV)
        self.view = self.buf[self.head:self.head + n]
        self.n = n

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def intact(self):
        return bool((self.buf[:self.head] == SENT).all()) and bool((self.buf[self.head + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())

    def get(self, *shape):
        return self.view.reshape(*shape).cpu().numpy()


def close(case, name, got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max()
    err = np.abs(np.asarray(got, dtype=np.float64) - ref).max()
    rel = err / scale if scale > 0 else err
    print(f"FE_ERR | {case} | {name} | {rel:.3e}")
    assert got.shape == ref.shape and np.isfinite(got).all() and err <= TOL * scale, (case, name, err, scale)


@functools.lru_cache(maxsize=None)
def analysis_case(shape):
    """Seeded inputs and the float64 reference of one analysis shape (computed once, shared, never modified)."""
    B, L, Cn, KW, hop, pad = shape
    T = frames_of(L, KW, hop, pad)
    rng = np.random.default_rng(1000 + B + L + Cn + KW + hop + pad)
    x = (0.3 * rng.standard_normal((B, L))).astype(np.float32)
    W = (0.05 * rng.standard_normal((Cn, KW))).astype(np.float32)
    bias = (0.1 * rng.standard_normal(Cn)).astype(np.float32)
    proj = rng.standard_normal((B, T, Cn)).astype(np.float32)
    xc = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    Wc = torch.tensor(W[:, None, :], dtype=torch.float64, requires_grad=True)
    bc = torch.tensor(bias, dtype=torch.float64, requires_grad=True)
    ft = Fn.conv1d(xc[:, None, :], Wc, bc, stride=hop, padding=pad).transpose(1, 2)
    assert ft.shape == (B, T, Cn)
    (ft * torch.tensor(proj, dtype=torch.float64)).sum().backward()
    with torch.no_grad():
        ft0 = Fn.conv1d(xc[:, None, :], Wc, None, stride=hop, padding=pad).transpose(1, 2)
    # geometry: frames that lie wholly in the padding, samples that no frame covers -- and the reference agrees with both
    starts = np.arange(T) * hop - pad
    dead = (starts + KW <= 0) | (starts >= L)
    covered = np.zeros(L, dtype=bool)
    for s in starts:
        covered[max(s, 0):max(min(s + KW, L), 0)] = True
    ref = dict(ft=ft.detach().numpy(), ft0=ft0.numpy(), gW=Wc.grad.numpy()[:, 0, :], gbias=bc.grad.numpy(), gx=xc.grad.numpy())
    assert (ref["ft0"][:, dead, :] == 0).all() and (ref["ft0"][:, ~dead, :] != 0).any(axis=2).all()
    assert (ref["gx"][:, ~covered] == 0).all() and (ref["gx"][:, covered] != 0).all()
    return dict(x=x, W=W, bias=bias, proj=proj, T=T, dead=dead, covered=covered, ref=ref)


@functools.lru_cache(maxsize=None)
def synthesis_case(shape):
    B, T, Cn, KW, hop, crop = shape
    n = (T - 1) * hop + KW - 2 * crop
    rng = np.random.default_rng(2000 + B + T + Cn + KW + hop + crop)
    xft = (0.3 * rng.standard_normal((B, T, Cn))).astype(np.float32)
    W = (0.05 * rng.standard_normal((Cn, KW))).astype(np.float32)
    proj = rng.standard_normal((B, n)).astype(np.float32)
    xc = torch.tensor(xft, dtype=torch.float64, requires_grad=True)
    Wc = torch.tensor(W[:, None, :], dtype=torch.float64, requires_grad=True)
    wave = Fn.conv_transpose1d(xc.transpose(1, 2), Wc, stride=hop)[..., crop:n + crop][:, 0, :]
    assert wave.shape == (B, n)
    (wave * torch.tensor(proj, dtype=torch.float64)).sum().backward()
    covered = np.zeros(n + 2 * crop, dtype=bool)
    for t in range(T):
        covered[t * hop:t * hop + KW] = True
    covered = covered[crop:n + crop]
    ref = dict(wave=wave.detach().numpy(), gW=Wc.grad.numpy()[:, 0, :], g_xft=xc.grad.numpy())
    assert (ref["wave"][:, ~covered] == 0).all()
    return dict(xft=xft, W=W, proj=proj, n=n, covered=covered, ref=ref)


def test_the_shapes_reach_the_edges_they_are_listed_for():
    """The tile and slice arithmetic of the module docstring, so that a change of a shape cannot quietly lose its edge (host arithmetic only)."""
    A = {k[:k.index("-")]: v for k, v in ANALYSIS.items()}
    rows = lambda s: s[0] * frames_of(s[1], s[3], s[4], s[5])
    split = lambda R: min(max(R // 200, 1), 16)
    ceil = lambda a, b: -(-a // b)
    slice_rows = lambda R: ceil(ceil(R, split(R)), 32) * 32      # st_gemm.h launch(): ksplit = round_up(ceil(K / nsplit), BK = 32)
    assert rows(A["1"]) == 13 and A["1"][3] == 16 and split(13) == 1
    assert rows(A["2"]) == 207 and -(-207 // 64) == 4 and 207 % 64 != 0
    assert 96 < A["3"][2] < 192 and A["3"][3] == 3 * 16 and A["3"][3] % A["3"][4] != 0
    assert A["4"][4] > A["4"][3] and A["5"][5] > A["5"][3]
    R6 = rows(A["6"]); assert R6 == 1026 and split(R6) == 5 and slice_rows(R6) == 224 and R6 - 4 * 224 == 130
    assert (-(-A["6"][2] // 96), -(-R6 // 64)) == (3, 17) and 51 % 8 != 0 and (-(-A["6"][3] // 96), -(-A["6"][2] // 96)) == (2, 3)
    R7 = rows(A["7"]); assert R7 == 3216 and split(R7) == 16 and slice_rows(R7) == 224 and R7 - 14 * 224 == 80 and 15 * 224 > R7
    R9 = rows(A["9"]); assert R9 == 32784 and -(-R9 // 64) == 513 and split(R9) == 16
    for k in ("10a", "10b"):
        T = frames_of(A[k][1], 16, 4, 0); R = A[k][0] * T
        assert R * T < (1 << 32) and ((A[k][0] + 1) * T - 1) * T >= (1 << 32)
    for s in list(ANALYSIS.values()):
        assert lib().st_fe_supported(*s) == 1, s
    for B, T, Cn, KW, hop, crop in SYNTHESIS.values():
        n = (T - 1) * hop + KW - 2 * crop
        assert n > 0 and n % 4 == 0 and lib().st_fe_supported(B, n, Cn, KW, hop, crop) == 1 and lib().st_fe_frames(n, KW, hop, crop) == T
    for s in REFUSED:
        assert lib().st_fe_supported(*s) == 0, s
    assert any(analysis_case(A[k])["dead"].sum() >= 2 for k in ("2",)) and analysis_case(A["5"])["dead"].sum() >= 4
    assert (~analysis_case(A["3"])["covered"]).sum() == 4 and (~analysis_case(A["4"])["covered"]).sum() > 0


@pytest.mark.parametrize("case", list(ANALYSIS))
def test_analysis_forward_and_backward_against_float64(case):
    shape = ANALYSIS[case]
    B, L, Cn, KW, hop, pad = shape
    assert lib().st_fe_supported(*shape) == 1      # host check first: an inexact row split is never launched
    c = analysis_case(shape); T, ref = c["T"], c["ref"]
    assert lib().st_fe_frames(L, KW, hop, pad) == T
    x, W, bias, g = dev(c["x"]), dev(c["W"]), dev(c["bias"]), dev(c["proj"])
    p = lambda t: C.c_void_p(t.data_ptr())
    # forward, with and without the bias
    out = Guarded(B * T * Cn)
    _lib.check(lib().st_fe_analysis_fwd(p(x), B, L, p(W), p(bias), Cn, KW, hop, pad, out.ptr(), stream()), "st_fe_analysis_fwd")
    torch.cuda.synchronize()
    ft = out.get(B, T, Cn)
    close(case, "ft", ft, ref["ft"])
    assert out.intact()
    if c["dead"].any():
        assert (ft[:, c["dead"], :] == c["bias"]).all(), "a frame in the padding is not the bias bit for bit"
    out0 = Guarded(B * T * Cn)
    _lib.check(lib().st_fe_analysis_fwd(p(x), B, L, p(W), None, Cn, KW, hop, pad, out0.ptr(), stream()), "st_fe_analysis_fwd")
    torch.cuda.synchronize()
    ft0 = out0.get(B, T, Cn)
    close(case, "ft(bias NULL)", ft0, ref["ft0"])
    assert out0.intact() and (ft0[:, c["dead"], :] == 0).all()
    # backward: all outputs, then the optional ones NULL
    nws = lib().st_fe_ws_floats(*shape)
    assert nws > 0
    for full in (True, False):
        ws = Guarded(nws, tail_only=True)
        gW, gb, gx = Guarded(Cn * KW), Guarded(Cn), Guarded(B * L)
        _lib.check(lib().st_fe_analysis_bwd(p(x), B, L, p(W), Cn, KW, hop, pad, p(g), ws.ptr(), gW.ptr(), gb.ptr() if full else None,
                                            gx.ptr() if full else None, stream()), "st_fe_analysis_bwd")
        torch.cuda.synchronize()
        close(case, "gW" if full else "gW(gbias, gx NULL)", gW.get(Cn, KW), ref["gW"])
        assert gW.intact() and ws.intact()
        if full:
            close(case, "gbias", gb.get(Cn), ref["gbias"])
            gxv = gx.get(B, L)
            close(case, "gx", gxv, ref["gx"])
            assert gb.intact() and gx.intact()
            assert (gxv[:, ~c["covered"]] == 0).all(), "the gradient of a sample no frame covers is not exactly 0"
        else:
            assert gb.untouched() and gx.untouched()


@pytest.mark.parametrize("case", list(SYNTHESIS))
def test_synthesis_forward_and_backward_against_float64(case):
    shape = SYNTHESIS[case]
    B, T, Cn, KW, hop, crop = shape
    c = synthesis_case(shape); n, ref = c["n"], c["ref"]
    assert lib().st_fe_supported(B, n, Cn, KW, hop, crop) == 1
    xft, W, g = dev(c["xft"]), dev(c["W"]), dev(c["proj"])
    p = lambda t: C.c_void_p(t.data_ptr())
    ws = Guarded(B * T * KW, tail_only=True)       # the forward's workspace: the frames (cls_fe_dct_bases._SynthesisFn.forward)
    out = Guarded(B * n)
    _lib.check(lib().st_fe_synthesis_fwd(p(xft), B, T, p(W), Cn, KW, hop, crop, ws.ptr(), out.ptr(), stream()), "st_fe_synthesis_fwd")
    torch.cuda.synchronize()
    wave = out.get(B, n)
    close(case, "wave", wave, ref["wave"])
    assert out.intact() and ws.intact()
    assert (wave[:, ~c["covered"]] == 0).all(), "a sample in a gap between frames is not exactly 0"
    if hop > KW:
        assert (~c["covered"]).any()
    nws = lib().st_fe_ws_floats(B, n, Cn, KW, hop, crop)      # as cls_fe_dct_bases._SynthesisFn.backward sizes it
    assert nws > 0
    for full in (True, False):
        ws = Guarded(nws, tail_only=True)
        gW, gxf = Guarded(Cn * KW), Guarded(B * T * Cn)
        _lib.check(lib().st_fe_synthesis_bwd(p(xft), B, T, p(W), Cn, KW, hop, crop, p(g), ws.ptr(), gW.ptr(), gxf.ptr() if full else None,
                                             stream()), "st_fe_synthesis_bwd")
        torch.cuda.synchronize()
        close(case, "gW" if full else "gW(g_xft NULL)", gW.get(Cn, KW), ref["gW"])
        assert gW.intact() and ws.intact()
        if full:
            close(case, "g_xft", gxf.get(B, T, Cn), ref["g_xft"])
            assert gxf.intact()
        else:
            assert gxf.untouched()


@pytest.mark.parametrize("ft,w,hop,L", [(512, 1024, 256, 8192), (64, 128, 32, 1000)])
def test_modules_with_non_default_sizes_through_backward(ft, w, hop, L):
    """cls_fe_dct_bases.Analysis / Synthesis built with other sizes than their defaults, B = 3, random learned bases, through .backward()."""
    from signaltrain_amd import cls_fe_dct_bases as D
    B = 3
    an, sy = D.Analysis(ft, w, hop).cuda(), D.Synthesis(ft, w, hop).cuda()
    assert an.conv_analysis.weight.shape == (ft, 1, w) and sy.conv_synthesis.weight.shape == (ft, 1, w)
    rng = np.random.default_rng(ft + w + hop)
    Wa = (0.05 * rng.standard_normal((ft, 1, w))).astype(np.float32); Ws = (0.05 * rng.standard_normal((ft, 1, w))).astype(np.float32)
    bias = (0.1 * rng.standard_normal(ft)).astype(np.float32)
    x = (0.3 * rng.standard_normal((B, L))).astype(np.float32)
    T = frames_of(L, w, hop, ft); n = (T - 1) * hop + w - 2 * ft
    proj = rng.standard_normal((B, 1, n)).astype(np.float32)
    xc = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    Wac = torch.tensor(Wa, dtype=torch.float64, requires_grad=True); bc = torch.tensor(bias, dtype=torch.float64, requires_grad=True)
    Wsc = torch.tensor(Ws, dtype=torch.float64, requires_grad=True)
    ftr = Fn.conv1d(xc[:, None, :], Wac, bc, stride=hop, padding=ft).transpose(1, 2)
    wv = Fn.conv_transpose1d(ftr.transpose(1, 2), Wsc, stride=hop)[..., ft:n + ft]
    (wv * torch.tensor(proj, dtype=torch.float64)).sum().backward()
    with torch.no_grad():
        an.conv_analysis.weight.copy_(torch.from_numpy(Wa)); an.conv_analysis.bias.copy_(torch.from_numpy(bias)); sy.conv_synthesis.weight.copy_(torch.from_numpy(Ws))
    xg = torch.from_numpy(x).cuda().requires_grad_(True)
    ftg = an.forward(xg); wvg = sy.forward(ftg)
    assert ftg.shape == (B, T, ft) and wvg.shape == (B, 1, n)
    (wvg * torch.from_numpy(proj).cuda()).sum().backward()
    case = f"module-{ft}-{w}-{hop}"
    num = lambda t: t.detach().cpu().numpy()
    close(case, "ft", num(ftg), ftr.detach().numpy()); close(case, "wave", num(wvg), wv.detach().numpy())
    close(case, "g_x", num(xg.grad), xc.grad.numpy()); close(case, "g_Wa", num(an.conv_analysis.weight.grad), Wac.grad.numpy())
    close(case, "g_bias", num(an.conv_analysis.bias.grad), bc.grad.numpy()); close(case, "g_Ws", num(sy.conv_synthesis.weight.grad), Wsc.grad.numpy())


@pytest.mark.parametrize("shape", REFUSED, ids=lambda s: f"B{s[0]}-L{s[1]}")
def test_shapes_past_the_exact_row_split_are_refused_not_run(shape):
    """(B*T - 1) * T >= 2^32: the predicate says no on the host FIRST (a missing or wrong predicate fails here, before anything is launched); then every compute
    entry, given real and correctly sized buffers, answers ST_ERR_ARG with a message and leaves its outputs alone -- and the Python wrapper raises."""
    B, L, Cn, KW, hop, pad = shape
    assert lib().st_fe_supported(*shape) == 0
    assert lib().st_fe_ws_floats(*shape) == 0
    T = frames_of(L, KW, hop, pad); n = (T - 1) * hop + KW - 2 * pad
    assert (B * T - 1) * T >= (1 << 32) and n == L and lib().st_fe_supported(B, n, Cn, KW, hop, pad) == 0
    p = lambda t: C.c_void_p(t.data_ptr())
    x, W, bias = torch.zeros(B, L, device=DEV), torch.zeros(Cn, KW, device=DEV), torch.zeros(Cn, device=DEV)
    xft = torch.zeros(B, T, Cn, device=DEV)
    ws = Guarded(B * T * KW + 16 * Cn * KW + B * (L + 2 * KW + 2 * pad) + 1024)      # what the size formula would be for an accepted shape
    out, gW, gb, gx, wave, gxf = Guarded(B * T * Cn), Guarded(Cn * KW), Guarded(Cn), Guarded(B * L), Guarded(B * n), Guarded(B * T * Cn)

    def refused(rc):
        assert rc == -1 and len(lib().st_last_error()) > 0 and b"row split" in lib().st_last_error(), (rc, lib().st_last_error())
    refused(lib().st_fe_analysis_fwd(p(x), B, L, p(W), p(bias), Cn, KW, hop, pad, out.ptr(), stream()))
    refused(lib().st_fe_analysis_bwd(p(x), B, L, p(W), Cn, KW, hop, pad, p(xft), ws.ptr(), gW.ptr(), gb.ptr(), gx.ptr(), stream()))
    refused(lib().st_fe_synthesis_fwd(p(xft), B, T, p(W), Cn, KW, hop, pad, ws.ptr(), wave.ptr(), stream()))
    refused(lib().st_fe_synthesis_bwd(p(xft), B, T, p(W), Cn, KW, hop, pad, p(x), ws.ptr(), gW.ptr(), gxf.ptr(), stream()))
    torch.cuda.synchronize()
    for b in (ws, out, gW, gb, gx, wave, gxf):
        assert b.untouched()
    from signaltrain_amd import cls_fe_dct_bases as D
    with pytest.raises(RuntimeError, match="row split"):
        D._AnalysisFn.apply(x, W[:, None, :], bias, hop, pad)
    with pytest.raises(RuntimeError, match="row split"):
        D._SynthesisFn.apply(xft, W[:, None, :], hop, pad)
