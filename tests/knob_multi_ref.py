"""The cases the host and GPU tests of the multi-setting routes (st_knob_multi_plan / st_score_knobs_coded / st_fit_knobs_multi_coded) share: rows, candidate
settings, recordings and the float64 reference's J, per-window shares and gradients, computed once and never modified.  Needs no GPU.  Objective, recordings
and parameters are those of tests/fit_knobs_ref.py, the settings those of tests/decode_ref.py plus two, by import.

Every J the GPU file ranks comes out of `scores` below; tests/test_knob_multi_host.py asserts for each case that the candidates' J differ pairwise by more than
100 gpu_checks.TOL relative and that the float32 oracle agrees with the float64 one to a quarter of the tolerances, so that every ranking assertion is something
the reference alone satisfies with margin."""
import numpy as np

from oracle import st_oracle as O
from tests import decode_ref as D
from tests import fit_knobs_ref as R

K = R.K
# the candidates: decode_ref's three settings and two more
SETTINGS = np.concatenate([D.SETTINGS, np.array([[0.4, 0.2, -0.1, 0.3], [-0.25, 0.45, 0.05, -0.15]], np.float32)]).astype(np.float32)
S = SETTINGS.shape[0]
STARTS = SETTINGS[[0, 1, 3, 4]].copy()          # the four starts of the multi fit: distinct, none at the clamp
SCORE_ROWS = ["n256", "n32", "t32_ot16", None]
# (hops, B): nine windows in batches of four (2 * 9 > 4: st_decode_long's batches); three windows at B = 8 (stacked: 2, 2, 1 settings of S = 5) and at B = 7
# (stacked, one idle row per batch)
LONG, SHORT = 7, 1
SCORE_BATCHES = [(LONG, 4), (SHORT, 8), (SHORT, 7)]
# signal seed per (row, hops) where it is not 3: the first of 3, 4, 5, ... at which the case qualifies (tests/test_knob_multi_host.py asserts the rule; the rule
# of tests/dims_table.py).  n256 with three windows: at 3 candidates 0 and 2 are 0.2 % apart.
SIGNAL_SEED = {("n256", 1): 4}
# knob automation: [2, nwin, K], decode_ref's two alternating rows, at nine windows
AUTOMATION = D.AUTOMATION


# The target: the float64 oracle's output at a setting that is none of the candidates, plus a little noise -- "a recording and its processed version" whose knobs
# the search is to find.  (fit_knobs_ref.target_of, a residual of order 0.1 that no knob setting explains, leaves the candidates' J within a fraction of a percent
# of each other: no ranking could be asserted on it.)
KNOBS_TRUE = np.array([0.35, 0.15, -0.4, 0.05], np.float32)
NOISE = 0.01
MODEL = "model"         # the st_model of tests/test_gpu_predict_long._model(): the row of the Python route's case


def seed_of(row, hops):
    return SIGNAL_SEED.get((row, hops), 3)


def case(row):
    """(geo, P) of a row of fit_knobs_ref (None: the default geometry) or of the Python routes' model."""
    return D._model_case() if row == MODEL else R.case(row)


_PAIRS = {}


def pair(row, hops, seed=None, whole=False):
    """(signal, target) float32, made once: the lookback of the first window has no output, its target samples are zeros.  whole: hops + 2 windows exactly
    (n = L + (hops + 1) y), where the objective of the batched Python route coincides with the device's."""
    seed = seed_of(row, hops) if seed is None else seed
    if (row, hops, seed, whole) not in _PAIRS:
        geo, P = case(row)
        sig = R.signal(geo["L"] + (hops + 1) * geo["y"] if whole else R.length(geo, hops), seed)
        out = R.objective(sig, sig, KNOBS_TRUE, P, geo, want_grad=False)[2]
        tgt = np.zeros(sig.size, np.float64)
        tgt[geo["L"] - geo["y"]:] = out + NOISE * np.random.default_rng(seed + 100).standard_normal(out.size)
        _PAIRS[(row, hops, seed, whole)] = (sig, tgt.astype(np.float32))
    return _PAIRS[(row, hops, seed, whole)]


def fit_pair(row, hops):
    """The recordings of the comparisons with the fit's reference (gradient, J, Adam): fit_knobs_ref's own pair, whose residual of order 0.1 is the one the
    project's gradient bounds -- the 16-bit levels' 6e-2 among them -- were set on."""
    return R.pair(row, hops)


# the second trip of the persistent loops in a STACKED batch: three windows of the default geometry at as many seeded settings as fill
# decode_ref.second_trip_batch rows on the MI355X
TRIP_WINDOWS = SHORT + 2


def trip_settings(cus=D.MI355X_CUS):
    nb = D.second_trip_batch(cus, R.geo_for(None))
    ns = -(-nb // TRIP_WINDOWS)
    return (0.9 * (np.random.default_rng(23).random((ns, K)) - 0.5)).astype(np.float32)


def window_shares(sig, tgt, out, geo):
    """[nwin]: the sum of log-cosh over window w's valid output samples times 1 / n_out (float64); the shares sum to J."""
    L, y = geo["L"], geo["y"]
    n_out = sig.size - (L - y)
    lc = O.logcosh(np.asarray(out, np.float64) - tgt[L - y:L - y + n_out].astype(np.float64))
    nwin = (n_out + y - 1) // y
    return np.array([lc[w * y:(w + 1) * y].sum() for w in range(nwin)]) / n_out


_REF = {}


def scores(row, hops, settings=None, dtype=np.float64, seed=None, whole=False):
    """(J [S], shares [S, nwin]) of the case at `settings` ([S, K] or [S, nwin, K]; default SETTINGS) in `dtype` arithmetic; computed once."""
    key = (row, hops, dtype, None if settings is None else np.asarray(settings).tobytes(), seed, whole)
    if key not in _REF:
        geo, P = case(row)
        sig, tgt = pair(row, hops, seed, whole)
        Js, sh = [], []
        for kn in (SETTINGS if settings is None else settings):
            J, _, out = R.objective(sig, tgt, kn, P, geo, dtype=dtype, want_grad=False)
            Js.append(J); sh.append(window_shares(sig, tgt, out, geo))
        _REF[key] = (np.array(Js), np.stack(sh))
    return _REF[key]


def gradients(row, hops, starts, dtype=np.float64, per_window=False):
    """(J [S], gradient [S, rows, K]) of the reference on fit_pair at every start ([S, K] or [S, nwin, K]): rows = 1, the sum over the windows; per_window,
    each window's own.  Computed once per case (in the arithmetic modes of the oracle at the first call: float64 and float32 callers set none)."""
    key = ("g", row, hops, dtype, np.asarray(starts).tobytes(), per_window)
    if key not in _REF:
        geo, P = case(row)
        sig, tgt = fit_pair(row, hops)
        Js, gs = [], []
        for kn in starts:
            J, g, _ = R.objective(sig, tgt, kn, P, geo, dtype=dtype)
            Js.append(J); gs.append(g if per_window else g.sum(0, keepdims=True))
        _REF[key] = (np.array(Js), np.stack(gs))
    return _REF[key]


def separation(J):
    """The smallest relative gap between any two of the values."""
    J = np.asarray(J, np.float64)
    return min(abs(J[i] - J[j]) / max(abs(J[i]), abs(J[j])) for i in range(J.size) for j in range(i))
