"""The cases the host and GPU tests of the coded routes (st_encode_long / st_decode_long / st_fit_knobs_coded) share: rows, knob settings, recordings and the
float64 oracle's outputs, computed once and never modified.  Needs no GPU.  Helpers and case tables are those of tests/test_gpu_predict_long.py and
tests/fit_knobs_ref.py, by import.

Every recording the GPU file compares with the float64 oracle at gpu_checks.TOL comes out of the case table below, and tests/test_decode_host.py asserts for each that
the float32 oracle agrees with the float64 one to TOL / 4 (the rule of tests/dims_table.py).  The coded fit's comparisons use fit_knobs_ref's own cases, whose
conditioning tests/test_fit_knobs_host.py asserts."""
import numpy as np

from tests import fit_knobs_ref as R
from tests import gpu_checks as G
from tests import test_gpu_predict_long as PL

K = PL.K
KN = PL.KN
# the rows of the three-settings comparison; None is the default geometry.  n32: F = 17, one full group and one mostly-pad group per window; t32_ot16: every
# `to` row of every lane live
ROWS = ["n256", "h256", "ragged", "tiny", "n32", "t32_ot16", None]
LEVEL_ROWS = ["n384", None]
# three settings in one call
SETTINGS = np.stack([KN, -KN[::-1], np.zeros(K, np.float32)]).astype(np.float32)
NWIN = 9                # hops = 7: batches of four end in a single window whose tail lies behind the recording's end
AUTOMATION = np.stack([[KN if w % 2 == e else -KN[::-1] for w in range(NWIN)] for e in (0, 1)]).astype(np.float32)      # [2, nwin, K]: two rows alternating, and the other way round
# ae_dec_fwd_kernel: waves per workgroup and workgroups per CU (AE_DEC_NW, AE_DEC_WGS, csrc/st_decode.h), and the CU count of the MI355X
DEC_NW, DEC_WGS, MI355X_CUS = 8, 2, 256


def second_trip_batch(cus, geo):
    """The smallest batch whose group count exceeds grid x waves of ae_dec_fwd_kernel: its persistent loop takes a second trip."""
    return cus * DEC_WGS * DEC_NW // ((geo["F"] * 2 + 31) // 32) + 1


def _geo_p(row):
    return PL.case(row)


def _model_case():
    """Geometry and parameters of test_gpu_predict_long._model(): the Python routes' model."""
    from oracle import st_oracle as O
    return O.geometry(1, 4), G.make_case(1, 1, K=K, scale=1)[4]


def _std_len(geo):
    return PL.length(geo)


# name -> (geometry and parameters, signal length, signal seed, knob settings [S, K] or [S, nwin, K]).  Signal seeds: the first of the file's own seed, + 1,
# + 2, ... (five at most) at which the case qualifies; every case qualifies at its first seed.  second_trip: its seed 10 is the first of 9, 10, ... at which ALSO
# st_predict_long in batches of four is within TOL on the device ("Encode once": at seed 9 it is 1.19e-4 off at one sample).
def _cases():
    c = {}
    for row in ROWS:
        c[f"settings-{row or 'default'}"] = (_geo_p(row), _std_len, 3, SETTINGS)
    for row in LEVEL_ROWS:
        c[f"levels-{row or 'default'}"] = (_geo_p(row), _std_len, 5, KN[None, :])
    c["automation"] = (_geo_p("n256"), _std_len, 8, AUTOMATION)
    c["second_trip"] = (_geo_p(None), lambda geo: geo["L"] + (second_trip_batch(MI355X_CUS, geo) - 1) * geo["y"] - 5 * 4 - 1, 10, KN[None, :])
    c["sweep"] = (_model_case(), lambda geo: geo["L"] + 4 * geo["y"] + 777, 11, SETTINGS)
    return c


_CASES, _REF = None, {}


def names():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return list(_CASES)


def case(name):
    """(geo, P, recording, knob settings) of a case."""
    names()
    (geo, P), length, seed, kn = _CASES[name]
    return geo, P, PL.signal(length(geo), seed), kn


def reference(name):
    """[S, n_out] float64: the oracle's output at every setting of the case."""
    if name not in _REF:
        geo, P, sig, kn = case(name)
        _REF[name] = np.stack([PL.oracle(sig, k, P, geo) for k in kn])
    return _REF[name]


def reference_f32(name):
    """The same from the float32 oracle (fit_knobs_ref.objective's forward)."""
    geo, P, sig, kn = case(name)
    return np.stack([R.objective(sig, sig, k, P, geo, dtype=np.float32, want_grad=False)[2] for k in kn])
