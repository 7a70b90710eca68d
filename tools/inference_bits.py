#!/usr/bin/env python3
"""Every output of the whole-signal inference family, from fixed seeds, into one .npz -- so that two builds of the library can be compared bit for bit.

    python tools/inference_bits.py OUT.npz                  (GPU box; the library is the one signaltrain_amd loads: ST_LIB_PATH selects another build)
    python tools/inference_bits.py --compare A.npz B.npz    (anywhere: same names, dtypes, shapes and bytes, or exit status 1)

Entries: st_predict_long, st_encode_long / st_decode_long, st_fit_knobs, st_fit_knobs_coded, st_score_knobs_coded, st_fit_knobs_multi_coded, the predict
session (st_predict_stream_*) and st_eval_pool.  Shapes are the smallest at which each path can go wrong: B = 3 rows per batch and n = L + 3 y + 777 % y samples
(five windows: the last batch is partial and the last quad clipped) at the dims-table rows tiny (L < N), ragged (a dead frame), h256 (four overlapping frames: the
looped overlap-add) and n256, at f32 and bf16_all (fp32 and 16-bit staged rows and d-syn operands), float32 and int16 recordings, one knob row and one per
window.  Two runs of ONE build must already agree (no atomics, fixed summation orders); then equality between two builds says the builds compute the same."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np


def digest(arrays):
    h = hashlib.sha256()
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        h.update(f"{k}|{a.dtype.str}|{a.shape}|".encode()); h.update(a.tobytes())
    return h.hexdigest()


def compare(pa, pb):
    a, b = dict(np.load(pa)), dict(np.load(pb))
    print(f"{pa}: {len(a)} arrays, content sha256 {digest(a)}")
    print(f"{pb}: {len(b)} arrays, content sha256 {digest(b)}")
    assert sorted(a) == sorted(b), ("array names differ", sorted(set(a) ^ set(b)))
    bad = []
    for k in sorted(a):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        same = x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        if not same:
            n = int((x != y).sum()) if x.shape == y.shape else -1
            bad.append(k); print(f"DIFFERS {k}: {x.dtype}{x.shape} vs {y.dtype}{y.shape}, {n} elements")
    assert not bad, f"{len(bad)} of {len(a)} arrays differ"
    print(f"equal: all {len(a)} arrays, bit for bit")


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    compare(sys.argv[2], sys.argv[3]); sys.exit(0)
if len(sys.argv) != 2 or sys.argv[1].startswith("-"):
    sys.exit(__doc__)

import ctypes as C
import torch
from signaltrain_amd import _lib
from signaltrain_amd.engine import StepEngine

DEV, B, K, S = "cuda:0", 3, 3, 3
ROWS = {"tiny": (256, 96, 96, 4, 4), "ragged": (256, 96, 2020, 25, 9), "h256": (1024, 256, 4096, 21, 8), "n256": (256, 96, 2048, 25, 9)}      # tests/dims_table.py
out = {}


def keep(name, t):
    assert name not in out, name
    out[name] = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).copy()


def recording(n, seed):
    """(input, target) as float32 and as int16 device tensors"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    x = 0.4 * np.sin(2 * np.pi * 220.0 * t) * (0.3 + 0.7 * (np.sin(2 * np.pi * 31 * t) > 0)) + 0.02 * rng.standard_normal(n)
    pair = (x, 0.7 * np.tanh(1.5 * x))
    f32 = tuple(torch.from_numpy(a.astype(np.float32)).to(DEV) for a in pair)
    s16 = tuple(torch.from_numpy(np.round(a * 32767.0).astype(np.int16)).to(DEV) for a in pair)
    return {"f32": f32, "s16": s16}


def engine(row, level):
    N, H, L, T, OT = ROWS[row]
    d = _lib.st_dims()
    d.B, d.L, d.N, d.H, d.T, d.OT, d.F, d.K, d.y = B, L, N, H, T, OT, N // 2 + 1, K, (OT - 1) * H - N
    eng = StepEngine(d, DEV, max_batch=B, compute_dtype=level)
    g = torch.Generator().manual_seed(sum(map(ord, row)))
    for name, v in eng.named.items():
        w = torch.randn(v.shape, generator=g) * (0.05 if name.endswith(".bias") else 1.0 / np.sqrt(v.shape[-1]))
        v.copy_(w.to(DEV))
    return eng, d


def plan_of(eng, d, n):
    buf = (C.c_int * (4 * 64))()
    cnt = int(eng.lib.st_knob_multi_plan(C.byref(d), n, S, buf, 64))
    return np.array(buf[:4 * cnt], np.int32).reshape(cnt, 4)      # (w0, nw, s0, ns) per batch


for row in ROWS:
    for level in ("f32", "bf16_all"):
        eng, d = engine(row, level)
        L, y = d.L, d.y
        n, n_short = L + 3 * y + 777 % y, L - y + 777 % y
        nwin = int(eng.lib.st_predict_windows(C.byref(d), n))
        rng = np.random.default_rng(7)
        k1 = torch.from_numpy(rng.uniform(-0.4, 0.4, (K,)).astype(np.float32)).to(DEV)
        kw = torch.from_numpy(rng.uniform(-0.4, 0.4, (nwin, K)).astype(np.float32)).to(DEV)
        ks = torch.from_numpy(rng.uniform(-0.4, 0.4, (S, K)).astype(np.float32)).to(DEV)
        ksw = torch.from_numpy(rng.uniform(-0.4, 0.4, (S, nwin, K)).astype(np.float32)).to(DEV)
        rec, rec_short = recording(n, 1), recording(n_short, 2)
        plans = {"long": plan_of(eng, d, n), "short": plan_of(eng, d, n_short)}
        assert nwin == 5 and plans["long"][0, 3] == 1 and plans["short"][0, 3] == S, (nwin, plans)      # five windows, not stacked; one window, stacked
        for fmt in ("f32", "s16"):
            p = f"{row}.{level}.{fmt}."
            x, t = rec[fmt]
            for kn_name, kn in (("one", k1), ("win", kw)):
                keep(p + f"predict.{kn_name}.out", eng.predict_long(x, kn))
                res = eng.fit_knobs(x, t, kn, steps=2, want_grads=True)
                for nm, v in zip(("knobs", "loss_hist", "grad_hist", "m", "v"), res[:3] + res[3][:2]):
                    keep(p + f"fit.{kn_name}.{nm}", v)
            code = eng.encode_long(x)
            keep(p + "code", code.code)
            keep(p + "decode.set.out", eng.decode_long(code, ks[:2]))
            keep(p + "decode.win.out", eng.decode_long(code, ksw[:2]))
            for kn_name, kn in (("one", k1), ("win", kw)):
                res = eng.fit_knobs(code, t, kn, steps=2, want_grads=True)
                for nm, v in zip(("knobs", "loss_hist", "grad_hist", "m", "v"), res[:3] + res[3][:2]):
                    keep(p + f"fit_coded.{kn_name}.{nm}", v)
            for ln, (xx, tt), cc in (("long", rec[fmt], code), ("short", rec_short[fmt], None)):
                cc = cc or eng.encode_long(xx)
                keep(p + f"multi.{ln}.plan", plans[ln])
                for kn_name, kn in (("set", ks), ("win", ksw if ln == "long" else ksw[:, :1])):
                    loss, win = eng.score_knobs(cc, tt, kn, per_window=True)
                    keep(p + f"score.{ln}.{kn_name}.loss", loss); keep(p + f"score.{ln}.{kn_name}.win_loss", win)
                    kf, lh, (m, v, _), gh = eng.fit_knobs_multi(cc, tt, kn, steps=2, want_grads=True)
                    for nm, a in zip(("knobs", "loss_hist", "m", "v", "grad_hist"), (kf, lh, m, v, gh)):
                        keep(p + f"fit_multi.{ln}.{kn_name}.{nm}", a)
            # the session: 2 channels, pushes of m = y, then a ragged final push
            x2 = torch.stack([x, torch.flip(x, (0,))]).contiguous()
            for kn_name, kn in (("one", k1), ("chan", ks[:2])):
                st = eng.open_stream(2)
                outs, counters, pos = [], [], 0
                while n - pos > y + 5:
                    outs.append(st.push(x2[:, pos:pos + y], kn)); pos += y
                    counters.append((st.received, st.emitted, st.pending, int(st.closed)))
                outs.append(st.push(x2[:, pos:], kn, final=True))
                counters.append((st.received, st.emitted, st.pending, int(st.closed)))
                keep(p + f"stream.{kn_name}.out", torch.cat(outs, dim=1)); keep(p + f"stream.{kn_name}.counters", np.array(counters, np.int64))
            # the pool: 3 files.  File 0 (five windows) at offset 0: the aligned quads; file 1 shorter than L - y: no window, the side role alone; file 2
            # (three windows, the last clipped) at an offset that is 2 mod 4: staged, residual, target and output all sample by sample
            lens = np.array([n, L - y - 5, L + y + 3], np.int64)
            off = np.zeros(3, np.int64)
            off[1] = (lens[0] + 3) // 4 * 4 + 1
            off[2] = (off[1] + lens[1] + 3) // 4 * 4 + 2
            assert off[2] % 4 == 2 and lens[2] > L - y and lens[1] < L - y
            total = int(off[2] + lens[2])
            src = recording(total, 3)[fmt]
            kf = torch.from_numpy(rng.uniform(-0.4, 0.4, (3, K)).astype(np.float32)).to(DEV)
            stats, po = eng.eval_pool(src[0], src[1], off, lens, kf, want_out=True)
            keep(p + "pool.stats", stats); keep(p + "pool.out", po)
            _, po2 = eng.eval_pool(src[0], None, off, lens, kf)
            keep(p + "pool.predict_only.out", po2)
            for name in (p + "pool.out", p + "pool.predict_only.out"):      # `out` is written over the files' spans only: keep those
                out[name] = np.concatenate([out[name][int(a):int(a) + int(ln)] for a, ln in zip(off, lens)])
        torch.cuda.synchronize()
        del eng
nonfinite = [k for k, a in out.items() if a.dtype.kind == "f" and not np.isfinite(a).all()]
assert not nonfinite, ("non-finite outputs", nonfinite)
np.savez(sys.argv[1], **out)
print(f"{sys.argv[1]}: {len(out)} arrays, {sum(a.nbytes for a in out.values())} bytes, content sha256 {digest(out)}  (library {_lib.LIB_PATH})")
