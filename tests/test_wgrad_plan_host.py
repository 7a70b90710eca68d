"""The plan of a weight-gradient GEMM and of its slab sum (st_wgrad_plan; csrc/st_api.hip: wgrad_slices, wgrad_plan), host arithmetic only.

Three kernel forms (the 128 x 128 fp32 kernel, the 96 x 96 three-wave kernel, the 16-bit kernel), each over the whole tensor or over one basis of the
analysis pair: six k-slice rules.  They are restated here from their comments, with the slab count the area holds (`room`) and the live-row count, and
compared with what the library reports -- the same function its launches ask.  Then the one invariant every launch must keep: its slabs, and behind them
its Nyquist partials, fit the area st_wgrad_ws_floats reserves, for every batch, precision, half, layout and kernel form.
"""
import ctypes as C

import pytest

from signaltrain_amd import _lib
from tests import dims_table as D

FORM_TN128, FORM_96, FORM_TN16 = 0, 1, 2
PADDED, G16, STAGED = 1, 2, 4
I_FORM, I_R, I_NS, I_M0, I_M, I_FM, I_TRIM, I_NYQ_P, I_NYQ_OFF, I_NYQ_WRITE, I_USED, N_INTS = range(12)
BATCHES = [1, 2, 3, 5, 32, 64, 179, 256, 586, 600, 1024]
PRECS = [0, 1, 2, 3, 4, 5]                          # ST_PREC_F32, BF16, BF16_ALL, F16, F16_ALL, F32X3
NCUS = [64, 256, 304]
FLAGS = [0, PADDED, PADDED | G16, PADDED | STAGED]  # the per-op entries, the autograd entries, the training entries, st_loss_backward_stage
ROWS = list(D.ROWS) + [None]                        # None: the st_geometry default (N = 1024, H = 384)
SWEEP_ROWS = ["n512", "n256", "n384", "n32"]        # every B from 1 to 600


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


def _plan(lib, d, which, half, flags, ncus):
    n = lib.st_wgrad_plan(C.byref(d), which, half, flags, ncus, _OUT, N_INTS)
    assert n == N_INTS, (n, lib.st_last_error())
    return tuple(_OUT)


def _cases(d):
    """(which, half, flags, ncus) of one st_dims: halves for the analysis bases only."""
    for flags in FLAGS:
        for ncus in NCUS:
            for which, half in ((0, -1), (0, 0), (0, 1), (1, -1)):
                yield which, half, flags, ncus


# ---------------------------------------------------------------------------------------------- the rules, restated
def _cdiv(a, b):
    return -(-a // b)


def _kp(F):
    return 2 * _cdiv(F, 16) * 16


def _live_frames(T, H, N, Ls):
    """Frames with a tap inside the signal, by direct count: tap n of frame t sits at sample H t + n of the signal padded by N zeros on both sides."""
    n = sum(1 for t in range(T) if max(H * t, N) < min(H * t + N, N + Ls))
    return n if n > 0 else T


def _slices_96(R, KP, N, cus):
    """200 reduction rows per slice, 16 at most, and no more than keep six 3-wave workgroups per CU co-resident (an even count)."""
    s = min(max(R // 200, 1), 16)
    fit = max(6 * cus // (_cdiv(KP, 96) * _cdiv(N, 96)), 1)
    if fit >= 2:
        fit &= ~1
    return min(s, fit)


def _slices_96_half(R, KP, N, cus):
    """One basis: of the counts in [ns / 2, ns] the one whose last round of one-workgroup-per-CU tiles is fullest (the largest such count)."""
    ns = _slices_96(R, KP, N, cus)
    tiles = _cdiv(KP // 2, 96) * _cdiv(N, 96)
    best, bf = ns, -1.0
    for c in range(ns, max((ns + 1) // 2, 1) - 1, -1):
        f = tiles * c / (_cdiv(tiles * c, cus) * cus)
        if f > bf + 1e-9:
            best, bf = c, f
    return best


def _slices_tn128(R, N, cus):
    """One workgroup per CU, 16 slices at most, no slice under 64 reduction rows."""
    return max(1, min(cus // max((N // 128) ** 2, 1), 16, R // 64))


def _slices_tn128_half(R, N, cus, room):
    return max(1, min(cus // max(((N // 2) // 128) * (N // 128), 1), 16, R // 64, room))


def _slices_16(R, M, N, cus, room):
    """About two workgroups per CU, no slice under 128 reduction rows, no more slabs than the area holds (M = KP, or KP / 2 for one basis)."""
    return max(1, min(2 * cus // max(_cdiv(M, 128) * (N // 128), 1), R // 128, room))


def _room(d):
    """Slabs the area st_wgrad_ws_floats reserves holds once 64 Nyquist partials [2][N] are set aside.  The area is what the caller allocated for the device
    at hand, so it does not follow the CU count a query assumes."""
    area = _lib.load().st_wgrad_ws_floats(C.byref(d))
    return (area - 64 * 2 * d.N) // (_kp(d.F) * d.N)


def _area_rule(d, cus):
    """The area's own size rule: the larger of the two whole-tensor fp32 rules over all B * T frames, then the partials."""
    KP = _kp(d.F)
    return (max(_slices_96(d.B * d.T, KP, d.N, cus), _slices_tn128(d.B * d.T, d.N, cus)) * KP + 64 * 2) * d.N


def _expect(d, which, half, flags, cus, room, tn128=True, wg_split=False):
    """(form, R, slices) by the rules above, under the default tuning state (tn128 / wg_split: the switches the tuning test moves)."""
    KP, N = _kp(d.F), d.N
    Tv = _live_frames(d.OT, d.H, N, d.y) if which else _live_frames(d.T, d.H, N, d.L)
    R = d.B * Tv
    fp32_mfma = d.prec == 0 or (d.prec == 5 and not wg_split)          # ST_PREC_F32X3 keeps its weight gradients on the fp32 MFMA
    if (flags & G16) and d.prec in (1, 2, 3, 4) and N % 128 == 0:
        return FORM_TN16, R, _slices_16(R, KP if half < 0 else KP // 2, N, cus, room)
    # every rule: never more slabs than the area holds (the two whole-tensor fp32 rules size the area, so there this binds only under an assumed CU count
    # above the device's)
    if tn128 and (flags & PADDED) and fp32_mfma and N % 256 == 0 and Tv >= 2 and not (half >= 0 and (flags & STAGED)):
        return FORM_TN128, R, (min(_slices_tn128(R, N, cus), room) if half < 0 else _slices_tn128_half(R, N, cus, room))
    return FORM_96, R, min(_slices_96(R, KP, N, cus) if half < 0 else _slices_96_half(R, KP, N, cus), room)


def _check_invariant(p, d, half, area, room):
    KP, N = _kp(d.F), d.N
    slab = KP * N
    nyq = p[I_NYQ_P] > 0
    assert p[I_NS] >= 1
    assert p[I_NS] * slab + (p[I_NYQ_P] * 2 * N if nyq else 0) <= area
    assert p[I_USED] <= area
    if nyq:
        assert p[I_FORM] == FORM_TN128 and p[I_NYQ_P] <= 64
        assert p[I_NYQ_OFF] >= p[I_NS] * slab                              # the partials begin at or behind the last slab
        assert p[I_NYQ_OFF] + p[I_NYQ_P] * 2 * N <= area
        assert p[I_NYQ_OFF] == (p[I_NS] if half < 0 else room) * slab
    else:
        assert p[I_NYQ_WRITE] == 0 and p[I_NYQ_OFF] == 0
    assert (p[I_M0], p[I_M]) == {-1: (0, KP), 0: (0, KP // 2), 1: (KP // 2, KP // 2)}[half]      # the two halves' rows partition [0, KP)
    assert p[I_TRIM] <= p[I_FM] and (p[I_FM] == 0 or (d.B >= 2 and p[I_FORM] != FORM_96))


# ---------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("row", ROWS, ids=lambda r: r or "default")
def test_plan_follows_the_restated_rules_and_fits_the_area(row):
    lib = _lib.load()
    for B in BATCHES:
        for prec in PRECS:
            d = _dims(row, B, prec)
            area, room = lib.st_wgrad_ws_floats(C.byref(d)), _room(d)
            assert area > 0, lib.st_last_error()
            for which, half, flags, ncus in _cases(d):
                p = _plan(lib, d, which, half, flags, ncus)
                want = _expect(d, which, half, flags, ncus, room)
                assert (p[I_FORM], p[I_R], p[I_NS]) == want, (row, B, prec, which, half, flags, ncus, p, want)
                _check_invariant(p, d, half, area, room)


@pytest.mark.parametrize("row", SWEEP_ROWS)
def test_every_batch_up_to_600_fits_the_area(row):
    lib = _lib.load()
    for B in range(1, 601):
        for prec in PRECS:
            d = _dims(row, B, prec)
            area, room = lib.st_wgrad_ws_floats(C.byref(d)), _room(d)
            for which, half, flags, ncus in _cases(d):
                _check_invariant(_plan(lib, d, which, half, flags, ncus), d, half, area, room)


def test_current_device_count_answers_as_its_explicit_count():
    lib = _lib.load()
    ncus = 256                                                  # without a device the library assumes 256 CUs, the MI355X's count
    for row in ("n512", "n384", None):
        for prec in (0, 2):
            d = _dims(row, 64, prec)
            for which, half, flags, _ in _cases(d):
                if lib.st_wgrad_ws_floats(C.byref(d)) == _area_rule(d, ncus):
                    assert _plan(lib, d, which, half, flags, 0) == _plan(lib, d, which, half, flags, ncus)


@pytest.mark.parametrize("row", [None, "n512", "n256"])
def test_pair_plan_runs_the_two_plans_slice_counts(row):
    lib = _lib.load()
    for B in BATCHES:
        for ncus in NCUS:
            d = _dims(row, B)
            n = lib.st_wgrad_pair_plan(C.byref(d), ncus, None, 0)
            assert n >= 0
            if n == 0:
                continue
            out = (C.c_int * (10 * n))()
            assert lib.st_wgrad_pair_plan(C.byref(d), ncus, out, n) == n
            for job, which in ((0, 0), (1, 1)):
                ns = 1 + max(out[10 * i + 5 * job + 2] for i in range(n))
                p = _plan(lib, d, which, -1, PADDED, ncus)
                assert p[I_FORM] == FORM_TN128 and p[I_NS] == ns, (row, B, ncus, job, ns, p)


def test_tuning_codes_move_the_form_as_their_switches_say():
    lib = _lib.load()
    forms = lambda d, **kw: [(_plan(lib, d, w, h, f, 256)[:3], _expect(d, w, h, f, 256, _room(d), **kw)) for w, h, f, _ in _cases(d)]
    try:
        for code, kw in ((9500, dict(tn128=False)),             # g_tn128 = 0: gemm_kernel<3, ...> everywhere the 128 x 128 kernel ran
                         (9580, {}), (9582, {}),                # its round-3 loop / one launch per GEMM: the same form and slices
                         (102, dict(tn128=False)),              # g_wg_mode = 2: the 96 x 96 kernel on the k-quad-major staging
                         (9301, dict(wg_split=True))):          # g_wg_split: ST_PREC_F32X3 on the in-kernel three-plane split of the 96 x 96 kernel
            assert lib.st_set_tuning(code) == 0
            for row in ("n512", "n384", None):
                for prec in (0, 1, 5):
                    for got, want in forms(_dims(row, 64, prec), **kw):
                        assert got == want, (code, row, prec, got, want)
            lib.st_reset_tuning()
        moved = [g[0] for g, _ in forms(_dims("n512", 64, 5))]
        assert FORM_TN128 in moved
    finally:
        lib.st_reset_tuning()


def test_refusals():
    lib = _lib.load()
    out = (C.c_int * N_INTS)()
    d = _dims("n512", 3)
    ok = lambda *a: lib.st_wgrad_plan(*a)
    assert ok(C.byref(d), 0, -1, PADDED, 256, out, N_INTS) == N_INTS
    assert ok(C.byref(d), 0, -1, PADDED, 256, None, 0) == N_INTS            # sizing call
    assert ok(None, 0, -1, PADDED, 256, out, N_INTS) < 0
    for name, (N, H, L, T, OT) in D.REFUSED.items():
        r = _dims("n512", 3)
        r.N, r.H, r.L, r.T, r.OT, r.F, r.y = N, H, L, T, OT, N // 2 + 1, (OT - 1) * H - N
        assert ok(C.byref(r), 0, -1, PADDED, 256, out, N_INTS) < 0, name
    for which, half in ((-1, -1), (2, -1), (0, -2), (0, 2), (1, 0), (1, 1)):
        assert ok(C.byref(d), which, half, PADDED, 256, out, N_INTS) < 0, (which, half)
    assert ok(C.byref(d), 0, -1, PADDED, 256, out, -1) < 0
    assert ok(C.byref(d), 0, -1, PADDED, 256, None, 4) < 0
    assert ok(C.byref(d), 0, -1, 8, 256, out, N_INTS) < 0                   # an unknown flag
    assert ok(C.byref(d), 0, -1, G16, 256, out, N_INTS) < 0                 # the 16-bit pipeline exists on the padded layout only
