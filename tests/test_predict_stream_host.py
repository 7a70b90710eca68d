"""CPU: the host side of a predict session (st_predict_stream_*, include/signaltrain_hip.h) -- the schedule st_predict_stream_plan states (which windows a push
completes, what it emits, what stays held) over every length and several partitions into pushes, the size functions, and every refusal of the push and the open
(before any launch: runs without a GPU)."""
import ctypes as C
import os

import numpy as np
import pytest

from signaltrain_amd import _lib
from tests.test_gpu_predict_long import lengths
from tests.test_predict_long_host import WIDE_ROWS, dims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_ROWS = ["n256", "h256", "ragged", "tiny", "ot_eq_t16", None]


def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "signaltrain_hip.h")).read()
    lib = _lib.load()
    for name, decl in (("st_predict_stream_state_bytes", "size_t st_predict_stream_state_bytes(const st_dims* d, int channels);"),
                       ("st_predict_stream_ws_bytes", "size_t st_predict_stream_ws_bytes(const st_dims* d);"),
                       ("st_predict_stream_plan", "st_predict_stream_plan(const st_dims* d, long long n_in, long long m, int final, long long out4[4]);"),
                       ("st_predict_stream_open", "st_predict_stream_open(const st_dims* d, const float* params, int channels, st_predict_stream* s, void* state, void* ws, void* stream);"),
                       ("st_predict_stream_push", "st_predict_stream_push(const st_dims* d, const float* params, st_predict_stream* s, int fmt, const void* block, long long m, long long block_pitch,"),
                       ("st_predict_stream_reset", "st_predict_stream_reset(st_predict_stream* s);")):
        assert decl in hdr, name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert "typedef struct st_predict_stream {" in hdr and "} st_predict_stream;" in hdr
    res, args = _lib.SIGNATURES["st_predict_stream_push"]
    assert res is C.c_int and len(args) == 15 and args[5] is C.c_longlong and args[6] is C.c_longlong and args[9] is C.c_longlong and args[11] is C.c_longlong
    assert _lib.SIGNATURES["st_predict_stream_state_bytes"][0] is C.c_size_t and _lib.SIGNATURES["st_predict_stream_ws_bytes"][0] is C.c_size_t
    # the mirror of the struct: two 64-bit counters, fourteen ints
    assert C.sizeof(_lib.st_predict_stream) == 2 * 8 + 14 * 4
    assert [n for n, _ in _lib.st_predict_stream._fields_] == ["received", "emitted", "channels", "held", "half", "closed", "L", "N", "H", "T", "OT", "F", "K", "y", "prec", "B"]


def plan(lib, d, n_in, m, final):
    out4 = (C.c_longlong * 4)()
    assert lib.st_predict_stream_plan(C.byref(d), n_in, m, int(final), out4) == 0
    return tuple(int(v) for v in out4)


def partitions(n, y, seed):
    """Pushes (m, final) that sum to n: all m = 4, m = y, one push, and seeded random multiples of 4 (some below y) with a ragged final."""
    def chop(step):
        ms = [step] * (n // step)
        return [(m, False) for m in ms] + [(n - sum(ms), True)]
    rng = np.random.default_rng(seed)
    rand, left = [], n
    while left > 3 * y // 2:
        m = 4 * int(rng.integers(1, max(3 * y // 8, 2)))
        rand.append((m, False)); left -= m
    rand.append((left, True))
    return {"m=4": chop(4), "m=y": chop(y), "one": [(n, True)], "random": rand}


@pytest.mark.parametrize("row", PLAN_ROWS)
def test_plan_tiles_the_windows_and_the_output(row):
    """Whatever the partition: the windows of the pushes concatenate to 0 .. st_predict_windows - 1 without gap or repeat (none at all where the signal has no
    output sample), the emitted counts sum to st_predict_out_samples, and what stays held never exceeds L - 1 and is a multiple of four after every
    non-final push -- the room of a history half and the alignment the kernels rely on."""
    lib = _lib.load()
    d = dims(row)
    L, y = d.L, d.y
    for n in lengths(L, y):
        n_out = int(lib.st_predict_out_samples(C.byref(d), n))
        nwin = int(lib.st_predict_windows(C.byref(d), n)) if n_out > 0 else 0
        for name, pushes in partitions(n, y, seed=n).items():
            assert sum(m for m, _ in pushes) == n and pushes[-1][1] and all(m % 4 == 0 for m, f in pushes if not f)
            got, nxt, emitted = 0, 0, 0
            for m, final in pushes:
                first, cnt, emit, held = plan(lib, d, got, m, final)
                assert first == nxt and cnt >= 0, (row, n, name, got, m)
                nxt += cnt; emitted += emit; got += m
                if final:
                    assert held == 0
                    assert emit == max(n_out - first * y, 0)
                else:
                    assert emit == cnt * y
                    assert 0 <= held <= L - 1 and held % 4 == 0 and held == got - nxt * y, (row, n, name, got, held)
                    assert held == (got if got < L else L - y + (got - L) % y)
            assert nxt == nwin and emitted == n_out, (row, n, name, nxt, nwin, emitted, n_out)


def test_plan_refuses_bad_arguments():
    lib = _lib.load()
    d = dims("n256")
    out4 = (C.c_longlong * 4)()
    assert lib.st_predict_stream_plan(C.byref(d), -4, 4, 0, out4) == -1 and b"st_predict_stream_plan" in lib.st_last_error()
    assert lib.st_predict_stream_plan(C.byref(d), 0, -4, 0, out4) == -1 and b"st_predict_stream_plan" in lib.st_last_error()
    assert lib.st_predict_stream_plan(C.byref(d), 0, 4, 0, None) == -1 and b"out4" in lib.st_last_error()
    bad = dims("n256"); bad.y += 4
    assert lib.st_predict_stream_plan(C.byref(bad), 0, 4, 0, out4) == -1 and b"y must equal" in lib.st_last_error()


@pytest.mark.parametrize("row,B", [(None, 5), ("n256", 5), ("h256", 3), ("tiny", 2)])
def test_size_functions(row, B):
    lib = _lib.load()
    for prec in range(6):
        d = dims(row, B=B, prec=prec)
        assert int(lib.st_predict_stream_ws_bytes(C.byref(d))) >= int(lib.st_predict_ws_bytes(C.byref(d))) > 0
        for ch in (1, 2, 7):
            assert int(lib.st_predict_stream_state_bytes(C.byref(d), ch)) == 2 * ch * d.L * 4


def test_sizes_are_zero_for_bad_or_unsupported_dims():
    lib = _lib.load()
    bads = []
    d = dims("n256"); d.B = 0; bads.append(d)
    d = dims("n256"); d.y += 4; bads.append(d)
    d = dims("n256"); d.prec = 7; bads.append(d)
    bads += [dims(r) for r in WIDE_ROWS if not lib.st_predict_supported(C.byref(dims(r)))]
    wide = _lib.geometry(8, 4, 4, 2)
    if not lib.st_predict_supported(C.byref(wide)):
        bads.append(wide)
    assert len(bads) > 3
    for d in bads:
        assert lib.st_predict_stream_ws_bytes(C.byref(d)) == 0 and lib.st_predict_stream_state_bytes(C.byref(d), 2) == 0
    for ch in (0, -1):
        assert lib.st_predict_stream_state_bytes(C.byref(dims("n256")), ch) == 0


def session(d, channels=2, received=0):
    """The host struct as st_predict_stream_open leaves it (open itself launches), `received` samples in (a multiple of four)."""
    s = _lib.st_predict_stream()
    s.channels = channels
    for f in ("L", "N", "H", "T", "OT", "F", "K", "y", "prec", "B"):
        setattr(s, f, getattr(d, f))
    s.received = received
    s.held = received if received < d.L else d.L - d.y + (received - d.L) % d.y
    return s


def _push(lib, d, s=None, m=None, fmt=0, pitch=None, final=0, knob_rows=1, opitch=None, params=0x1000, block=0x1000, knobs=0x1000, out=0x1000, state=0x1000, ws=0x1000):
    """st_predict_stream_push with dummy pointers (never dereferenced on the host; a refused call launches nothing)."""
    p = lambda v: C.c_void_p(v) if v else None
    s = session(d) if s is None else s
    m = d.L + d.y if m is None else m
    pitch = (m + 3) // 4 * 4 if pitch is None else pitch
    opitch = 2 * d.y if opitch is None else opitch
    rc = lib.st_predict_stream_push(C.byref(d), p(params), C.byref(s) if s is not False else None, fmt, p(block), m, pitch, final, p(knobs), knob_rows,
                                    p(out), opitch, p(state), p(ws), None)
    return rc, lib.st_last_error()


def test_the_last_check_of_the_dummy_call_is_the_alignment():
    """The dummy call passes every rule up to the alignment ones: each refusal test below moves exactly one argument."""
    lib = _lib.load()
    rc, msg = _push(lib, dims("n256"), out=0x1004)
    assert rc == -1 and b"out must be 16-byte aligned" in msg


@pytest.mark.parametrize("missing", ["params", "block", "knobs", "out", "state", "ws"])
def test_push_refuses_a_null_pointer_by_name(missing):
    lib = _lib.load()
    rc, msg = _push(lib, dims("n256"), **{missing: 0})
    assert rc == -1 and b"st_predict_stream_push" in msg and b"null" in msg and missing.encode() in msg, msg


def test_push_null_pointers_that_are_allowed():
    lib = _lib.load()
    d0 = dims("n256", K=0)
    rc, msg = _push(lib, d0, s=session(d0), knobs=0, out=0x1004)            # K = 0: null knobs pass, the next refusal is another rule's
    assert rc == -1 and b"aligned" in msg and b"knobs" not in msg
    d = dims("n256")
    rc, msg = _push(lib, d, m=0, block=0, pitch=0, out=0, opitch=0, ws=0x1004)      # m = 0: block may be null, and nothing is emitted: out may be null
    assert rc == -1 and b"ws must be 16-byte aligned" in msg
    rc, msg = _push(lib, d, m=d.L - 4, out=0, opitch=0, ws=0x1004)          # no window completes: out may be null
    assert rc == -1 and b"ws must be 16-byte aligned" in msg
    rc, msg = _push(lib, d, s=False)
    assert rc == -1 and b"null pointer (s)" in msg


def test_push_refuses_bad_lengths_formats_rows_and_pitches():
    lib = _lib.load()
    d = dims("n256")
    for m in (-4, (1 << 30) + 4):
        rc, msg = _push(lib, d, m=m, pitch=1 << 31)
        assert rc == -1 and b"st_predict_stream_push: m = " in msg and b"2^30" in msg, m
    for m in (d.L + 1, d.L + 2, 3):
        rc, msg = _push(lib, d, m=m)
        assert rc == -1 and b"non-final push must be a multiple of 4" in msg, m
        rc, msg = _push(lib, d, m=m, final=1, out=0x1004)                   # a final push takes any m
        assert rc == -1 and b"aligned" in msg, m
    for fmt in (-1, 2, 7):
        rc, msg = _push(lib, d, fmt=fmt)
        assert rc == -1 and b"fmt" in msg
    for rows in (0, 3, -1):
        rc, msg = _push(lib, d, knob_rows=rows)
        assert rc == -1 and b"knob_rows" in msg and b"channel count (2)" in msg, rows
    for rows in (1, 2):
        rc, msg = _push(lib, d, knob_rows=rows, out=0x1004)
        assert rc == -1 and b"aligned" in msg, rows
    m = d.L + d.y
    for pitch in (m - 4, m + 2, 0):
        rc, msg = _push(lib, d, m=m, pitch=pitch)
        assert rc == -1 and b"block_pitch" in msg, pitch
    for opitch in (2 * d.y - 4, 2 * d.y + 2, 0):                           # the plan emits two windows: 2 y samples per channel
        rc, msg = _push(lib, d, m=m, opitch=opitch)
        assert rc == -1 and b"out_pitch" in msg and str(2 * d.y).encode() in msg, opitch
    # a final push of the same m emits the clipped last window as well; its count is the plan's
    emit = plan(lib, d, 0, m + 5, True)[2]
    assert emit == 2 * d.y + 5
    rc, msg = _push(lib, d, m=m + 5, final=1, opitch=2 * d.y + 4)
    assert rc == -1 and b"out_pitch" in msg and str(emit).encode() in msg


def test_push_refuses_misaligned_pointers():
    lib = _lib.load()
    d = dims("n256")
    for off in (4, 8, 12):
        for name in ("block", "out", "state", "ws"):
            rc, msg = _push(lib, d, **{name: 0x1000 + off})
            assert rc == -1 and f"{name} must be 16-byte aligned".encode() in msg, (name, off)
    for off in (2, 4, 6):
        rc, msg = _push(lib, d, fmt=_lib.PCM_S16, block=0x1000 + off)
        assert rc == -1 and b"block must be 8-byte aligned" in msg, off
    rc, msg = _push(lib, d, fmt=_lib.PCM_S16, block=0x1008, out=0x1004)     # an int16 block on an 8-byte boundary is taken
    assert rc == -1 and b"out must be" in msg


def test_push_refuses_other_dims_than_the_sessions_and_a_closed_session():
    lib = _lib.load()
    d = dims("n256")
    rc, msg = _push(lib, dims("h256"), s=session(d))
    assert rc == -1 and b"st_predict_stream_push: dims differ" in msg
    rc, msg = _push(lib, dims("n256", K=3), s=session(d))
    assert rc == -1 and b"dims differ" in msg
    rc, msg = _push(lib, dims("n256", prec=2), s=session(d))
    assert rc == -1 and b"prec = 2 differs" in msg
    rc, msg = _push(lib, dims("n256", B=4), s=session(d))
    assert rc == -1 and b"B = 4 differs" in msg
    s = session(d); s.closed = 1
    rc, msg = _push(lib, d, s=s)
    assert rc == -1 and b"closed" in msg and b"st_predict_stream_reset" in msg
    assert lib.st_predict_stream_reset(C.byref(s)) == 0 and s.closed == 0 and s.received == 0 and s.held == 0 and s.channels == 2 and s.L == d.L
    rc, msg = _push(lib, d, s=s, out=0x1004)                                # open again: the next refusal is another rule's
    assert rc == -1 and b"aligned" in msg
    s = _lib.st_predict_stream()                                            # never opened
    rc, msg = _push(lib, d, s=s)
    assert rc == -1 and b"channels = 0" in msg
    assert lib.st_predict_stream_reset(C.byref(s)) == -1 and lib.st_predict_stream_reset(None) == -1


def test_push_and_open_refuse_bad_and_unsupported_dims():
    lib = _lib.load()
    good = dims("n256")
    bads = []
    d = dims("n256"); d.B = 0; bads.append((d, b"dimension"))
    d = dims("n256"); d.y += 4; bads.append((d, b"y must equal"))
    d = dims("n256"); d.prec = 9; bads.append((d, b"prec"))
    for d in [dims(r) for r in WIDE_ROWS] + [_lib.geometry(8, 4, 4, 2)]:
        if not lib.st_predict_supported(C.byref(d)):
            bads.append((d, b"st_predict_supported"))
    s = _lib.st_predict_stream()
    p = C.c_void_p(0x1000)
    for d, word in bads:
        rc, msg = _push(lib, d, s=session(good))
        assert rc == -1 and word in msg, msg
        assert lib.st_predict_stream_open(C.byref(d), p, 2, C.byref(s), p, p, None) == -1 and word in lib.st_last_error()


def test_open_refuses_channels_null_pointers_and_misalignment():
    lib = _lib.load()
    d = dims("n256")
    s = _lib.st_predict_stream()
    p = lambda v: C.c_void_p(v) if v else None
    for ch in (0, -2, 1 << 16):
        assert lib.st_predict_stream_open(C.byref(d), p(0x1000), ch, C.byref(s), p(0x1000), p(0x1000), None) == -1
        assert b"st_predict_stream_open: channels" in lib.st_last_error()
    for i, name in enumerate(("params", "s", "state", "ws")):
        a = [p(0x1000), C.byref(s), p(0x1000), p(0x1000)]
        a[i] = None
        assert lib.st_predict_stream_open(C.byref(d), a[0], 2, a[1], a[2], a[3], None) == -1
        msg = lib.st_last_error()
        assert b"st_predict_stream_open: null pointer" in msg and f"({name})".encode() in msg, msg
    assert lib.st_predict_stream_open(C.byref(d), p(0x1000), 2, C.byref(s), p(0x1008), p(0x1000), None) == -1 and b"state must be 16-byte aligned" in lib.st_last_error()
    assert lib.st_predict_stream_open(C.byref(d), p(0x1000), 2, C.byref(s), p(0x1000), p(0x1004), None) == -1 and b"ws must be 16-byte aligned" in lib.st_last_error()
    assert s.channels == 0                                                   # a refused open leaves the struct alone
