#!/usr/bin/env python3
"""Bit equality of the STFT GEMM paths: the parent commit's library against this tree's, both loaded in one process.

    python tools/gemm_plan_ab.py wgrad PARENT_LIBRARY.so profiles/wgrad_plan_refactor_ab.txt
    python tools/gemm_plan_ab.py stft  PARENT_LIBRARY.so profiles/stft_plan_refactor_ab.txt [--tuning 0,3,4]

wgrad: every entry that reaches a weight-gradient GEMM; grads, parameters, moments, scalars, stage compared as bytes.
stft:  every entry that reaches the analysis forward, synthesis frames or synthesis data-gradient GEMM; its output buffers and the workspace's forward state
       (re, im, mag, phs, mag_hat, phs_hat, AA, y_hat through st_workspace_offsets; frs / dAA for the per-op entries) compared as bytes.
--tuning: positions in the subject's list of tuning states (a long run in several visits); the result file names the states that ran.
The same seeded inputs go through both libraries.  Stops at the first library error (no further GPU work after it)."""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("ST_RCCL_LIB", os.path.join(ROOT, "tests", "libfake_rccl.so"))
from signaltrain_amd import _lib          # noqa: E402
from tests import dims_table as D         # noqa: E402

DEV = torch.device("cuda:0")
LEVELS = [("f32", 0, 0.0, 0), ("f32x3", 5, 0.0, 0), ("bf16", 1, 0.0, 0), ("bf16_all", 2, 0.0, 0), ("f16_all", 4, 4096.0, 1)]
SUBJECTS = {
    "wgrad": dict(
        title="weight-gradient plan refactor",
        entries=["loss_backward", "train_step", "groups2", "groups12", "groups14", "p1_p2_staged", "stages", "per_op", "dp1", "dp3", "dp7"],
        shapes=[(r, B) for r in ("n512", "n256", "n384", "n160", "t33_ot17", None) for B in (3, 64)] + [("n256", 600)],
        tuning=[None, 9500, 9580, 9582, 9540, 9564, 9568]),
    "stft": dict(
        title="forward / data-gradient GEMM plan refactor",
        entries=["analysis_fwd", "synthesis_frames", "synthesis_dgrad", "model_fwd0", "model_fwd1", "model_bwd", "loss_backward", "train_step", "eval_step",
                 "predict_long", "stage0", "stage1", "stage2", "stage3", "dp1"],
        shapes=[(r, B) for r in ("n512", "n256", "n384", "n160", "n96", "n32", "ragged", "h256", "t33_ot17", None) for B in (3, 64)] + [("n256", 600)],
        tuning=[None, 16, 7001, 9000, 9950, 9100, 9201, 9401, 9600, 9691, 9692, 9693, 9560, 9561, 9562]),
}


def load(path, older=False):
    lib = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if older and not hasattr(lib, name):      # the parent lacks the entries this tree adds; the tool calls none of them
            continue
        fn = getattr(lib, name); fn.restype = res; fn.argtypes = args
    return lib


def dims(lib, row, B, prec, ls, clip_all):
    d = _lib.st_dims()
    if row is None:
        assert lib.st_geometry(1.0, 4.0, 0, 4, B, C.byref(d)) == 0
    else:
        g = D.geo_of(row)
        d.B, d.L, d.N, d.H, d.T, d.OT, d.F, d.K, d.y = B, g["L"], g["N"], g["H"], g["T"], g["OT"], g["F"], 4, g["y"]
    d.prec, d.loss_scale, d.clip_all = prec, ls, clip_all
    return d


P = _lib.ptr


class Case:
    """Host master copies of one (shape, level); run(lib, entry) gives the output tensors of that entry on fresh device buffers."""

    def __init__(self, lib, d):
        self.d = d
        offs = (C.c_int64 * 40)()
        self.total = lib.st_param_offsets(C.byref(d), offs)
        self.offs = list(offs)
        g = torch.Generator().manual_seed(1234 + d.N + d.B)
        r = lambda *s, sc=1.0: (sc * torch.randn(*s, generator=g)).to(DEV)
        self.params = r(self.total, sc=0.05)
        self.params[:self.offs[4]] *= 0.5
        torch.cuda.synchronize()
        self.x, self.y, self.kn = r(d.B, d.L, sc=0.3), r(d.B, d.y, sc=0.3), (torch.rand(d.B, d.K, generator=g) - 0.5).to(DEV)
        KP = self.KP = 2 * ((d.F + 15) // 16 * 16)
        self.dG, self.AA, self.dsyn = r(d.B * d.T, KP, sc=0.1), r(d.B * d.OT, KP, sc=0.1), r(d.B, d.y, sc=0.1)
        self.g_mag_hat, self.g_mag = r(d.B * d.OT * d.F, sc=0.01), r(d.B * d.T * d.F, sc=0.01)
        self.n_sig = d.L + d.y * (d.B + 1) + 5                    # st_predict_long: two batches of windows, the second and the last window partial
        self.signal = r(self.n_sig, sc=0.3)
        self.ws_bytes = lib.st_workspace_bytes_max(C.byref(d))
        self.pws_bytes = lib.st_predict_ws_bytes(C.byref(d))
        self.wg_floats = lib.st_wgrad_ws_floats(C.byref(d))
        self.np = lib.st_norm_partials(C.byref(d))
        so = (C.c_int64 * 8)()
        assert lib.st_workspace_offsets(C.byref(d), so) == 0, lib.st_last_error()
        nt, no = d.B * d.T * d.F, d.B * d.OT * d.F
        self.state = list(zip(so, [nt, nt, nt, nt, no, no, d.B * d.OT * KP, d.B * d.y]))      # re, im, mag, phs, mag_hat, phs_hat, AA, y_hat

    def run(self, lib, entry, dp=None):
        d, dv = self.d, lambda t: t.clone()
        z = lambda n: torch.zeros(n, device=DEV)
        params, grads, m, v = dv(self.params), z(self.total), z(self.total), z(self.total)
        x, y, kn = dv(self.x), dv(self.y), dv(self.kn)
        ws, sc, stage = torch.zeros(self.ws_bytes // 4 + 64, device=DEV), z(16), z(2 * d.F * d.N)
        s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        D_ = C.byref(d)
        ck = lambda rc: (_ for _ in ()).throw(RuntimeError(f"{entry}: rc {rc}: {lib.st_last_error().decode()}")) if rc else None
        hyp = (1e-3, 0.9, 0.999, 1e-8)
        outs = [grads, params, m, v, sc, stage]
        state = lambda: [ws[o:o + n] for o, n in self.state] if self.subject == "stft" else []      # stft: the forward state the fused entries leave in the workspace
        nt, no = d.B * d.T * d.F, d.B * d.OT * d.F
        if entry == "loss_backward":
            ck(lib.st_loss_backward(D_, P(params), P(grads), P(x), P(kn), P(y), None, None, None, P(ws), P(sc), s))
            outs = outs + state()
        elif entry == "train_step":
            for it in (1, 2):
                ck(lib.st_train_step(D_, P(params), P(grads), P(m), P(v), P(x), P(kn), P(y), P(ws), P(sc), *hyp, it, s))
            outs = outs + state()
        elif entry.startswith("groups"):
            mask = int(entry[6:])
            ck(lib.st_train_step_groups(D_, P(params), P(grads), P(m), P(v), P(x), P(kn), P(y), P(ws), P(sc), *hyp, (C.c_int * 4)(1, 1, 1, 1), mask, s))
        elif entry == "p1_p2_staged":
            ck(lib.st_loss_backward_p1(D_, P(params), P(grads), P(x), P(kn), P(y), P(ws), s))
            ck(lib.st_loss_backward_p2_staged(D_, P(grads), P(stage), P(x), P(ws), P(sc), s))
        elif entry == "stages":
            for st in range(4):
                ck(lib.st_loss_backward_stage(D_, P(params), P(grads), P(x), P(kn), P(y), P(ws), P(sc), st, s))
        elif entry.startswith("stage"):                           # the schedule up to and including that stage
            for st in range(int(entry[5:]) + 1):
                ck(lib.st_loss_backward_stage(D_, P(params), P(grads), P(x), P(kn), P(y), P(ws), P(sc), st, s))
            outs = outs + state()
        elif entry == "per_op":
            n_t = self.offs[1] - self.offs[0]
            g = [z(n_t) for _ in range(4)]
            wg, na, ns_ = z(self.wg_floats), z(self.np), z(self.np)
            ck(lib.st_analysis_wgrad(D_, P(self.dG), P(x), 0.5, P(wg), P(g[0]), P(g[1]), P(na), s))      # inputs are read only: the masters themselves (a temporary clone would be freed, and its memory reused, before the kernel ran)
            torch.cuda.synchronize()
            ck(lib.st_synthesis_wgrad(D_, P(self.AA), P(self.dsyn), P(wg), P(g[2]), P(g[3]), P(ns_), s))
            outs = g + [na, ns_]
        elif entry.startswith("dp"):
            ck(lib.st_dp_train_step(dp, D_, P(params), P(grads), P(m), P(v), P(stage), P(x), P(kn), P(y), P(ws), P(sc), *hyp, 1, int(entry[2:]), s))
            outs = outs + state()
        elif entry == "analysis_fwd":                             # the per-op entries: unpadded inputs
            outs = [z(nt) for _ in range(4)]
            ck(lib.st_analysis_fwd(D_, P(x), P(params[self.offs[0]:]), P(params[self.offs[1]:]), 0.5, *[P(t) for t in outs], s))
        elif entry in ("synthesis_frames", "synthesis_dgrad"):
            fold = z(self.KP * d.N)
            ck(lib.st_synth_fold(D_, P(params[self.offs[2]:]), P(params[self.offs[3]:]), P(fold), s))
            if entry == "synthesis_frames":
                outs = [z(lib.st_synth_frame_slabs(D_) * d.B * d.OT * d.N)]
                ck(lib.st_synthesis_frames(D_, P(self.AA), P(fold), P(outs[0]), s))
            else:
                outs = [z(lib.st_synth_slabs(D_) * d.B * d.OT * self.KP)]
                ck(lib.st_synthesis_dgrad(D_, P(self.dsyn), P(fold), P(outs[0]), s))
        elif entry in ("model_fwd0", "model_fwd1", "model_bwd"):
            y_hat, mag, mag_hat = z(d.B * d.y), z(nt), z(no)
            ck(lib.st_model_fwd(D_, P(params), P(x), P(kn), P(y_hat), P(mag), P(mag_hat), P(ws), 0 if entry == "model_fwd0" else 1, s))
            if entry == "model_bwd":
                ck(lib.st_model_bwd(D_, P(params), P(grads), P(x), P(kn), P(self.dsyn), P(self.g_mag_hat), P(self.g_mag), P(ws), s))
            outs = [y_hat, mag, mag_hat, grads] + state()
        elif entry == "eval_step":
            acc, y_hat = torch.zeros(8, device=DEV, dtype=torch.float64), z(d.B * d.y)
            ck(lib.st_eval_step(D_, P(params), P(x), P(kn), P(y), P(y_hat), P(ws), C.c_void_p(acc.data_ptr()), 0.9, s))
            outs = [acc.view(torch.float32), y_hat] + state()
        elif entry == "predict_long":
            pws, out = torch.zeros(self.pws_bytes // 4 + 64, device=DEV), z(self.n_sig)
            ck(lib.st_predict_long(D_, P(params), _lib.PCM_F32, P(self.signal), self.n_sig, P(kn), 1, P(out), P(pws), s))
            outs = [out]
        else:
            raise ValueError(entry)
        torch.cuda.synchronize()
        return [t.view(torch.int32) for t in outs]


def main():
    subject, parent_path, out_path = sys.argv[1], sys.argv[2], sys.argv[3]
    S = SUBJECTS[subject]
    Case.subject = subject
    tuning = S["tuning"]
    if len(sys.argv) > 5 and sys.argv[4] == "--tuning":
        tuning = [S["tuning"][int(i)] for i in sys.argv[5].split(",")]
    libs = {"parent": load(parent_path, older=True), "branch": load(_lib.LIB_PATH)}
    comms = {}
    for k, lib in libs.items():
        uid = C.create_string_buffer(128)
        assert lib.st_dp_unique_id(uid) == 0, lib.st_last_error()
        p = C.c_void_p()
        assert lib.st_dp_init(uid, 0, 1, C.byref(p)) == 0, lib.st_last_error()
        comms[k] = p
    cases = nbytes = ndiff = 0
    bad, refused = [], []
    for code in tuning:
        for lib in libs.values():
            lib.st_reset_tuning()
            if code is not None:
                assert lib.st_set_tuning(code) == 0
        for row, B in S["shapes"]:
            for lname, prec, ls, ca in LEVELS:
                d = dims(libs["branch"], row, B, prec, ls, ca)
                c = Case(libs["branch"], d)
                for entry in S["entries"]:
                    got, err = {}, {}
                    for k, lib in libs.items():
                        try:
                            got[k] = c.run(lib, entry, comms[k])
                        except RuntimeError as e:
                            err[k] = str(e)
                            if "rc -1:" not in err[k]:      # not an argument refusal (those come before any launch): nothing more runs on the GPU
                                print("ERROR", code, row, B, lname, entry, k, err[k], flush=True)
                                return 2
                    if err:      # an entry both libraries refuse before any launch, with the same words, is equal behaviour; anything else ends the run
                        if len(err) == 2 and err["parent"] == err["branch"]:
                            refused.append((code, row, B, lname, entry)); continue
                        print("ERROR", code, row, B, lname, entry, err, flush=True)
                        return 2
                    diff = sum(int((a != b).sum()) * 4 for a, b in zip(got["parent"], got["branch"]))
                    nb = sum(a.numel() * 4 for a in got["parent"])
                    cases += 1; nbytes += nb; ndiff += diff
                    if diff:
                        bad.append((code, row, B, lname, entry, diff))
                        print("DIFF", bad[-1], flush=True)
                del c
                torch.cuda.empty_cache()
        print(f"tuning {code}: {cases} cases so far, {ndiff} differing bytes", flush=True)
    for lib in libs.values():
        lib.st_reset_tuning()
    txt = (f"{S['title']}, parent library against this tree's in one process (one MI355X)\n"
           f"entries: {', '.join(S['entries'])}\nshapes: {S['shapes']}\nlevels: {[l[0] for l in LEVELS]}\ntuning states: {tuning}\n"
           f"cases {cases}, bytes compared {nbytes}, differing bytes {ndiff}; refused alike by both (argument check, no launch): {len(refused)} {sorted(set(r[1:] for r in refused))}\n" + "".join(f"DIFF {b}\n" for b in bad) +
           ("RESULT: bit-identical\n" if not ndiff else "RESULT: DIFFERENT\n"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(txt)
    print(txt)
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())
