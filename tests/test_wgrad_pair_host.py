"""The plan of the fp32 step's pair launch (st_wgrad_pair_plan; csrc/st_gemm_tn.h: gemm_tn128_pair_kernel), host logic only.

The pair launch runs both 128 x 128-tile weight-gradient GEMMs -- analysis bases (reduction over the live input frames, padded signal of L samples) and
synthesis bases (live output frames, padded d syn of y samples) -- in one launch: every workgroup slot runs one k-slice of an analysis tile and then one k-slice
of a synthesis tile.  What must hold for the results to stay what the two launches compute: every (GEMM, tile row, tile column, k-slice) is run exactly once,
and over exactly the reduction rows the single-GEMM kernel derives for that (tile column, k-slice).  That rule is restated here from the geometry alone:
frames enumerated frame-major (row = (t - t_lo) * B + b), per tile column the contiguous run of frames that carry a tap inside the unpadded signal
(stg::frame_trim), that run divided into `ns` slices of whole 32-row k-tiles.  What the pairing is for: the slot with the most k-tiles is as short as any
column pairing can make it (longest analysis columns against shortest synthesis columns).
"""
import ctypes as C

import pytest

from signaltrain_amd import _lib

NCUS = 256
BKT = 32
BATCHES = [2, 3, 8, 64, 128, 130, 200, 256, 384, 512, 1024]


def _dims(row, B, K=4):
    if row is None:
        d = _lib.st_dims()
        assert _lib.load().st_geometry(1.0, 4.0, 0, K, B, C.byref(d)) == 0
        return d
    from tests import dims_table as D
    g = D.geo_of(row)
    d = _lib.st_dims()
    d.B, d.L, d.N, d.H, d.T, d.OT, d.F, d.K, d.y = B, g["L"], g["N"], g["H"], g["T"], g["OT"], g["F"], K, g["y"]
    return d


def _plan(d):
    lib = _lib.load()
    n = lib.st_wgrad_pair_plan(C.byref(d), NCUS, None, 0)
    assert n >= 0, lib.st_last_error()
    out = (C.c_int * (10 * max(n, 1)))()
    assert lib.st_wgrad_pair_plan(C.byref(d), NCUS, out, n) == n
    return [tuple(out[10 * i:10 * i + 10]) for i in range(n)]


def _live(T, H, N, Ls):
    """First live frame and live frame count of a signal of Ls samples padded by N on both sides (stg::live_frames with pad = N)."""
    lo, hi = 0, T - 1
    while lo < T and H * lo - N + N <= 0:
        lo += 1
    while hi >= lo and H * hi - N >= Ls:
        hi -= 1
    return lo, hi - lo + 1


def _rule(B, T, H, N, Ls):
    """{(tile column, slice): (k_begin, k_end)} and the slice count of one GEMM by the single-job rule (gemm_tn128_kernel; B >= 2: frame-major rows)."""
    t_lo, Tv = _live(T, H, N, Ls)
    R = B * Tv
    tiles = (N // 128) ** 2
    ns = max(1, min(NCUS // tiles, 16, R // 64))
    out = {}
    for j in range(N // 128):
        n0, a, b = 128 * j, 0, Tv
        while a < b and H * (t_lo + a) + n0 + 127 < N:
            a += 1
        while b > a and H * (t_lo + b - 1) + n0 >= N + Ls:
            b -= 1
        lo, hi = a * B, b * B
        per = -(-(-(-(hi - lo) // ns)) // BKT) * BKT
        for z in range(ns):
            k0 = lo + z * per
            out[(j, z)] = (k0, min(k0 + per, hi))
    return out, ns


def _ktiles(k0, k1):
    return -(-(k1 - k0) // BKT) if k1 > k0 else 0


@pytest.mark.parametrize("row", [None, "n512"])
@pytest.mark.parametrize("B", BATCHES)
def test_plan_runs_every_slice_of_both_gemms_once_over_the_single_job_ranges(row, B):
    d = _dims(row, B)
    plan = _plan(d)
    nt = d.N // 128
    rules = [_rule(B, d.T, d.H, d.N, d.L), _rule(B, d.OT, d.H, d.N, d.y)]
    nz = max(rules[0][1], rules[1][1])
    assert len(plan) == nz * nt * nt, (len(plan), nz, nt)
    seen = [set(), set()]
    slot_tiles = []
    for slot in plan:
        total = 0
        for job in range(2):
            ty, tx, z, k0, k1 = slot[5 * job:5 * job + 5]
            if ty < 0:
                assert (ty, tx, z, k0, k1) == (-1,) * 5
                continue
            key = (ty, tx, z)                                   # one field group per job: a slot cannot hold two entries of the same job
            assert key not in seen[job], (job, key)
            seen[job].add(key)
            assert (k0, k1) == rules[job][0][(tx, z)], (job, key, (k0, k1), rules[job][0][(tx, z)])
            total += _ktiles(k0, k1)
        slot_tiles.append(total)
    for job in range(2):
        want = {(ty, tx, z) for ty in range(nt) for tx in range(nt) for z in range(rules[job][1])}
        assert seen[job] == want, (job, len(seen[job]), len(want))
    # surplus slices (different slice counts) leave their slots with one entry
    both = sum(1 for s in plan if s[0] >= 0 and s[5] >= 0)
    assert both == min(rules[0][1], rules[1][1]) * nt * nt
    # the longest slot is the best any column pairing reaches: the per-column k-tile counts (slice 0, the longest) sorted against each other
    col = [[_ktiles(*rules[job][0][(j, 0)]) for j in range(nt)] for job in range(2)]
    best = max(a + s for a, s in zip(sorted(col[0], reverse=True), sorted(col[1])))
    assert max(slot_tiles) == best, (max(slot_tiles), best, col)
    if row is None and B == 256:
        assert best == 54 and max(col[0]) + max(col[1]) == 56
    # all slots of a tile column share one synthesis column (a permutation of the columns)
    perm = {}
    for s in plan:
        if s[0] >= 0 and s[5] >= 0:
            assert perm.setdefault(s[1], s[6]) == s[6]
    assert sorted(perm.values()) == list(range(nt))


def test_geometries_and_modes_outside_the_pair_launch_report_none():
    lib = _lib.load()
    assert _plan(_dims("n384", 64)) == []                       # N % 256 != 0: the 128-row tiles do not cover a basis half
    assert _plan(_dims("t33_ot17", 64)) == []                   # wide autoencoder geometry
    for prec in (1, 2, 3, 4, 5):                                # 16-bit and split operands
        d = _dims(None, 64); d.prec = prec
        assert _plan(d) == [], prec
    try:
        for code in (9582, 9580, 9500):                         # one launch per GEMM / the round-3 loop / the small-tile kernel
            assert lib.st_set_tuning(code) == 0
            assert _plan(_dims(None, 64)) == [], code
        assert lib.st_set_tuning(9581) == 0
        assert len(_plan(_dims(None, 64))) > 0
    finally:
        lib.st_reset_tuning()
    assert lib.st_wgrad_pair_plan(None, NCUS, None, 0) < 0


def test_tuning_code_9582_stores_3_and_the_other_codes_keep_their_values():
    lib = _lib.load()
    n = lib.st_get_tuning(None, 0)
    cur, dflt = (C.c_int * n)(), (C.c_int * n)()
    lib.st_tuning_defaults(dflt, n)
    try:
        for code, val in ((9582, 3), (9580, 2), (9581, 1), (9501, 1), (9500, 0)):
            assert lib.st_set_tuning(code) == 0
            lib.st_get_tuning(cur, n)
            changed = [i for i in range(n) if cur[i] != dflt[i]]
            assert (changed == [] and val == 1) or (len(changed) == 1 and cur[changed[0]] == val and dflt[changed[0]] == 1), (code, changed)
            lib.st_reset_tuning()
    finally:
        lib.st_reset_tuning()
