"""The plan of the analysis forward, synthesis frames and synthesis data-gradient GEMMs (st_stft_plan; csrc/st_api.hip: stft_family, synth_tile, stft_plan),
host arithmetic only.

Four operand families (fp32 MFMA, operands converted while staged, bfloat16 planes, the 16-bit pipeline) on five kernel forms.  The rules are restated here from
their comments and compared with what the library reports -- the same function its launches ask -- under the default tuning state and under every switch that
moves one of them.  Then what every launch must keep: the slab counts are the ones the workspace is carved for (st_synth_frame_slabs / st_synth_slabs), whatever
the family, and within what the consumers sum; the work-list form reports the list st_nt128_worklist returns; frame-major rows only where the kernels' division
by B is exact; the 16-bit family only where N % 128 == 0.
"""
import ctypes as C

import pytest

from signaltrain_amd import _lib
from tests import dims_table as D

ANALYSIS, FRAMES, DGRAD = 0, 1, 2
PADDED, G16, SFOLDT = 1, 2, 4
FAM_FP32, FAM_HALF, FAM_PLANES, FAM_G16 = range(4)
FORM_SMALL, FORM_NT128, FORM_PLANES, FORM_NT16, FORM_NT256 = range(5)
(I_FAMILY, I_FORM, I_WAVES, I_BK, I_XT, I_R, I_M, I_NC, I_K, I_NS, I_FM, I_CROP, I_WORK, I_T_LO, I_TV, N_INTS) = range(16)
BATCHES = [1, 2, 3, 5, 64, 179, 256, 585, 586, 600, 1024]      # 586: the first batch at which 7 live output frames reach 4096 rows
PRECS = [0, 1, 2, 3, 4, 5]                                      # ST_PREC_F32, BF16, BF16_ALL, F16, F16_ALL, F32X3
HT = {0: 0, 1: 1, 2: 1, 3: 2, 4: 2, 5: 3}                       # operand type of the STFT GEMMs: fp32 / bfloat16 / float16 / three bfloat16 planes
NCUS = [64, 256, 304]
FLAGS = [0, PADDED | SFOLDT, PADDED | SFOLDT | G16]             # the per-op entries, the autograd entries, the training entries
ROWS = list(D.ROWS) + [None]                                    # None: the st_geometry default (N = 1024, H = 384)
TALL_ROWS = 4096
# the switches the plan reads, at their shipped defaults, and the st_set_tuning codes that move them (csrc/st_api.hip: k_tuning_codes)
DEFAULTS = dict(an_bk=32, bk=16, xt=0, frs_nt=1, nt128=1, pl_shape=3, pl_dgrad=0, pl_bf16=0, g16=1, g16_dma=0, g16_crop=15)
TUNING = {None: {}, 16: dict(an_bk=16, bk=16), 7001: dict(xt=1), 9000: dict(frs_nt=0), 9950: dict(nt128=0), 9100: dict(pl_shape=0), 9201: dict(pl_dgrad=1),
          9401: dict(pl_bf16=1), 9600: dict(g16=0), 9691: dict(g16_dma=1), 9692: dict(g16_dma=2), 9693: dict(g16_dma=3),
          9560: dict(g16_crop=0), 9561: dict(g16_crop=1), 9562: dict(g16_crop=2)}


def _dims(row, B, prec=0, K=4):
    d = _lib.st_dims()
    if row is None:
        assert _lib.load().st_geometry(1.0, 4.0, 0, K, B, C.byref(d)) == 0
    else:
        g = D.geo_of(row)
        d.B, d.L, d.N, d.H, d.T, d.OT, d.F, d.K, d.y = B, g["L"], g["N"], g["H"], g["T"], g["OT"], g["F"], K, g["y"]
    d.prec = prec
    return d


_OUT = (C.c_int * N_INTS)()
_WK = (C.c_uint * 1024)()
_HEAD = (C.c_int * 6)()


def _plan(lib, d, which, flags, ncus):
    n = lib.st_stft_plan(C.byref(d), which, flags, ncus, _OUT, N_INTS)
    assert n == N_INTS, (n, lib.st_last_error())
    return tuple(_OUT)


# ---------------------------------------------------------------------------------------------- the rules, restated
def _kp(F):
    return 2 * (-(-F // 16)) * 16


def _live_frames(T, H, N, Ls):
    """(first, count) of the frames with a tap inside the signal: tap n of frame t sits at sample H t + n of the signal padded by N zeros on both sides."""
    live = [t for t in range(T) if max(H * t, N) < min(H * t + N, N + Ls)]
    return (live[0], len(live)) if live else (0, T)


def _fm_exact(R, B):
    return R * B < 2 ** 32


def _expect(d, which, flags, sw):
    """The plan by the rules, but for the one decision the work-list builder makes: form is None where the 128 x 128 work-list kernel MAY run (then WAVES .. WORK
    depend on whether a list fits, which st_nt128_worklist reports)."""
    N, F, KP, B, ht = d.N, d.F, _kp(d.F), d.B, HT[d.prec]
    t_lo, Tv = _live_frames(d.T, d.H, N, d.L) if which == ANALYSIS else _live_frames(d.OT, d.H, N, d.y)
    R = B * Tv
    Nc = (2 * F, N, KP)[which]
    K = KP if which == FRAMES else N
    # the analysis forward: 4-wave tiles, one slab; the synthesis pair: 4-wave tiles and one slab from 4096 rows on, else 2-wave tiles and K over 3 slabs
    waves, ns = (4, 1) if which == ANALYSIS or R >= TALL_ROWS else (2, 3)
    padded = bool(flags & PADDED)
    planes_ok = (ht == 3 or (ht == 1 and sw["pl_bf16"])) and N % 16 == 0
    if padded and (flags & G16) and sw["g16"] and ht in (1, 2) and not sw["pl_bf16"] and N % 128 == 0:
        family = FAM_G16
    elif padded and planes_ok and (which != DGRAD or sw["pl_dgrad"]):
        family = FAM_PLANES
    else:
        family = FAM_FP32 if ht == 0 else FAM_HALF
    bk = xt = fm = crop = 0
    if family == FAM_G16:
        dma = (1, 0, 2)[which]                                   # g_g16_dma: bit 0 the analysis forward, bit 1 the data gradient
        form, waves = (FORM_NT256 if (sw["g16_dma"] & dma) and N % 64 == 0 and N // 64 >= ns else FORM_NT16), 0
        want = (0, sw["g16_crop"] & 1, (sw["g16_crop"] & 2) and not (sw["g16_dma"] & 2))[which]
        if want and _fm_exact(R, B):
            fm, crop = 1, which
    elif family == FAM_PLANES:
        form = FORM_PLANES
        if which == ANALYSIS and ht == 3 and sw["pl_shape"] == 3:
            waves = 8
    else:
        k_contiguous = (False, bool(flags & SFOLDT) and sw["frs_nt"], padded)[which]
        may = sw["nt128"] and ht == 0 and N % 32 == 0 and -(-R // 128) <= 255 and _fm_exact(R, B) and k_contiguous
        form = None if may else FORM_SMALL
        if family == FAM_FP32:
            bk, xt = (sw["an_bk"] if which == ANALYSIS and padded else sw["bk"]), sw["xt"]
    return [family, form, waves, bk, xt, R, R, Nc, K, ns, fm, crop, 0, t_lo, Tv]


def _check(lib, d, which, flags, ncus, sw):
    p = _plan(lib, d, which, flags, ncus)
    want = _expect(d, which, flags, sw)
    if want[I_FORM] is None:                                     # fused entry on fp32 operands: the list of st_nt128_worklist, or the small-tile kernel
        n = lib.st_nt128_worklist(C.byref(d), which - 1, ncus, _WK, 1024, _HEAD)
        assert n >= 0
        if n > 0:
            want[I_FORM], want[I_WAVES], want[I_BK], want[I_XT], want[I_FM], want[I_CROP], want[I_WORK] = FORM_NT128, 0, 0, 0, 1, which, n
            assert _HEAD[0] == want[I_NS]                        # the list's slab count is the plan's
        else:
            want[I_FORM] = FORM_SMALL
    assert p == tuple(want), (which, flags, ncus, p, want)
    # what every launch must keep
    assert 1 <= p[I_NS] <= 3                                     # the consumers instantiate with_slabs for 1..3 only
    if which == FRAMES:
        assert p[I_NS] == lib.st_synth_frame_slabs(C.byref(d))   # the room carve gives frs ...
    if which == DGRAD:
        assert p[I_NS] == lib.st_synth_slabs(C.byref(d))         # ... and dAA, for every family
    if p[I_FM]:
        assert lib.st_fm_div_exact(p[I_R], d.B) == 1
    if p[I_FORM] == FORM_NT128:
        assert want[I_WORK] > 0 and p[I_WORK] == want[I_WORK]     # the entry count st_nt128_worklist gave above for the same (d, which, ncus)
    else:
        assert p[I_WORK] == 0
    if p[I_FAMILY] == FAM_G16:
        assert d.N % 128 == 0


def _sweep(lib, row, sw):
    for B in BATCHES:
        for prec in PRECS:
            d = _dims(row, B, prec)
            for flags in FLAGS:
                for ncus in NCUS:
                    for which in (ANALYSIS, FRAMES, DGRAD):
                        _check(lib, d, which, flags, ncus, sw)


# ---------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("row", ROWS, ids=lambda r: r or "default")
def test_plan_follows_the_restated_rules_under_every_tuning_state(row):
    lib = _lib.load()
    try:
        for code, moved in TUNING.items():
            lib.st_reset_tuning()
            if code is not None:
                assert lib.st_set_tuning(code) == 0
            try:
                _sweep(lib, row, dict(DEFAULTS, **moved))
            except AssertionError as e:
                raise AssertionError(f"tuning {code}, row {row}: {e}") from e
    finally:
        lib.st_reset_tuning()


def test_the_sweep_reaches_every_family_and_form():
    lib = _lib.load()
    seen = set()
    try:
        for code in (None, 9401, 9691):
            lib.st_reset_tuning()
            if code is not None:
                assert lib.st_set_tuning(code) == 0
            for row in ("n512", "n160", None):
                for B in (3, 64, 600):
                    for prec in PRECS:
                        d = _dims(row, B, prec)
                        for flags in FLAGS:
                            for which in (ANALYSIS, FRAMES, DGRAD):
                                p = _plan(lib, d, which, flags, 256)
                                seen.add((p[I_FAMILY], p[I_FORM]))
    finally:
        lib.st_reset_tuning()
    assert seen >= {(FAM_FP32, FORM_SMALL), (FAM_FP32, FORM_NT128), (FAM_HALF, FORM_SMALL), (FAM_PLANES, FORM_PLANES), (FAM_G16, FORM_NT16), (FAM_G16, FORM_NT256)}, seen


def test_tall_tiles_start_at_586_windows_of_seven_live_frames():
    lib = _lib.load()
    for B, want in ((585, (2, 3)), (586, (4, 1))):
        d = _dims("n512", B)
        for which in (FRAMES, DGRAD):
            p = _plan(lib, d, which, 0, 256)
            assert p[I_TV] == 7 and (p[I_WAVES], p[I_NS]) == want, (B, which, p)


def test_current_device_count_answers_as_its_explicit_count():
    lib = _lib.load()
    ncus = 256                                                   # without a device the library assumes 256 CUs, the MI355X's count
    for row in ("n512", "n384", None):
        for prec in (0, 2, 5):
            d = _dims(row, 64, prec)
            for flags in FLAGS:
                for which in (ANALYSIS, FRAMES, DGRAD):
                    assert _plan(lib, d, which, flags, 0) == _plan(lib, d, which, flags, ncus)


def test_refusals():
    lib = _lib.load()
    out = (C.c_int * N_INTS)()
    d = _dims("n512", 3)
    ok = lambda *a: lib.st_stft_plan(*a)
    assert ok(C.byref(d), FRAMES, PADDED, 256, out, N_INTS) == N_INTS
    assert ok(C.byref(d), FRAMES, PADDED, 256, None, 0) == N_INTS              # sizing call
    assert ok(None, FRAMES, PADDED, 256, out, N_INTS) < 0
    for name, (N, H, L, T, OT) in D.REFUSED.items():
        r = _dims("n512", 3)
        r.N, r.H, r.L, r.T, r.OT, r.F, r.y = N, H, L, T, OT, N // 2 + 1, (OT - 1) * H - N
        assert ok(C.byref(r), FRAMES, PADDED, 256, out, N_INTS) < 0, name
    for which in (-1, 3):
        assert ok(C.byref(d), which, PADDED, 256, out, N_INTS) < 0, which
    assert ok(C.byref(d), FRAMES, PADDED, 256, out, -1) < 0
    assert ok(C.byref(d), FRAMES, PADDED, 256, None, 4) < 0
    assert ok(C.byref(d), FRAMES, 8, 256, out, N_INTS) < 0                     # an unknown flag
    assert ok(C.byref(d), FRAMES, G16, 256, out, N_INTS) < 0                   # the 16-bit pipeline and the transposed fold exist in the fused entries only
    assert ok(C.byref(d), FRAMES, SFOLDT, 256, out, N_INTS) < 0
