// st_filter.h -- the third-order Butterworth low-pass of the reference's LowPass effect (audio.py:610-625: scipy butter(3, cutoff / (sr / 2)) and
// lfilter without zi, i.e. from a zero state) as a parallel scan over the window (gfx950), one window per 256-thread workgroup.
//
// The scan runs on the MODES of the filter, not on lfilter's direct-form state.  With K = tan(pi fc / sr) the bilinear transform puts the poles at
//   p_k = (1 + K s_k) / (1 - K s_k),   s_0 = -1, s_1,2 = e^{+-2 pi i / 3}   (the analog Butterworth poles),
// and at the low end of the knob range (10 Hz at 44.1 kHz: K = 7e-4) all three lie within 1.4e-3 of z = 1.  The 3x3 maps of the direct-form
// (companion) state then have condition numbers beyond 1 / eps and a chunked scan over them loses every digit (deviation O(1) at 10 Hz, 2e-6 at
// 100 Hz; DESIGN.md section 4, "LowPass and Denoise").  In the parallel form
//   H(z) = d + sum_k r_k / (1 - p_k z^-1),   b0 = K^3 / ((1 + K)(1 + K + K^2)),   r_k = b0 (1 + 1 / p_k)^3 / prod_{j != k} (1 - p_j / p_k),
//   d = -b0 / (p_0 p_1 p_2)
// every mode is its own first-order recurrence with |p| < 1 and residues of size O(K):
//   s0[n] = p_0 s0[n-1] + x[n] (real),   s1[n] = p_1 s1[n-1] + x[n] (complex; the third mode is its conjugate),
//   y[n]  = d x[n] + r_0 s0[n] + 2 Re(r_1 s1[n]),
// all float64, y rounded to float32 on the store.  The real mode's two terms are regrouped as (d + r_0) x[n] + (r_0 p_0) s0[n-1] with
//   d + r_0 = b0 - 2 Re(r_1)   (H at z = infinity is b0),   r_0 p_0 = b0 (1 + p_0)^3 / |p_0 - p_1|^2,
// the same sum without 1 / p_0 in it: at the cutoff sr / 4 the real pole sits at the origin, d and r_0 diverge and only their sum is finite.
// A run of m samples is the affine map s -> p^m s + v, and the maps compose associatively:
// the chunk / run / wave-shuffle / four-wave-LDS / carry structure is env_compressor_window's (st_misc.h), with one real and one complex map.
// Measured against scipy.signal.lfilter in float64 (which itself is 7.5e-8 away from a long-double run of its own coefficients at 10 Hz): at most
// 3.5e-7 of max(1e-3, max |y|) on the device over cutoffs 10 ... 2000 Hz, 3.0e-7 for the numpy restatement of this scan in
// tests/test_lowpass_denoise_host.py.
#pragma once
#include "st_common.h"

namespace stm {

constexpr int LP_R = 8, LP_CH = 256 * LP_R;
struct LpLds {
    float x[LP_CH + LP_CH / LP_R];               // the chunk's x[n], one pad float per run: thread t reads from 9 t on, conflict-free
    float y[LP_CH];                              // the chunk's output (coalesced store pass)
    double wa0[4], wb0[4];                       // per-wave composed maps: the real mode ...
    double wa1r[4], wa1i[4], wb1r[4], wb1i[4];   // ... and the complex one
    double c0, c1r, c1i;                         // the modes' states after the previous chunk's last sample
};
struct LpCoef { double p0, p1r, p1i, g, q0, r1r, r1i; bool ok; };      // g = d + r_0, q0 = r_0 p_0
// The design for one cutoff.  ok == false: the cutoff is not inside (0, sr / 2) (or is NaN).
__device__ __forceinline__ LpCoef lowpass_coef(const double fc, const double sr)
{
#pragma clang fp contract(off)      // every product and sum as written, in every kernel the function is inlined into: the feed and st_lowpass agree bit for bit
    LpCoef c;
    c.ok = fc > 0.0 && fc < 0.5 * sr;                                          // false for NaN
    const double K = tan(3.14159265358979323846 * fc / sr);
    const double sr3 = 0.86602540378443864676 * K;                             // K Im(s_1);  K Re(s_1) = -K / 2
    // p_1 = (1 - K / 2 + i sr3) / (1 + K / 2 - i sr3)
    const double nr = 1.0 - 0.5 * K, dr = 1.0 + 0.5 * K, dn = dr * dr + sr3 * sr3;
    c.p0 = (1.0 - K) / (1.0 + K);
    c.p1r = (nr * dr - sr3 * sr3) / dn; c.p1i = (sr3 * dr + nr * sr3) / dn;
    const double b0 = K * K * K / ((1.0 + K) * (1.0 + K + K * K));
    const double m1 = c.p1r * c.p1r + c.p1i * c.p1i;                           // |p_1|^2 = p_1 p_2
    // r_0 p_0 = b0 (1 + p_0)^3 / |p_0 - p_1|^2
    const double q1 = 1.0 + c.p0, er = c.p0 - c.p1r;
    c.q0 = b0 * q1 * q1 * q1 / (er * er + c.p1i * c.p1i);
    // r_1 = b0 (1 + 1 / p_1)^3 / ((1 - p_0 / p_1)(1 - p_2 / p_1)),   1 / p_1 = conj(p_1) / |p_1|^2
    const double ir = c.p1r / m1, ii = -c.p1i / m1;
    const double ar = 1.0 + ir, ai = ii;
    const double a2r = ar * ar - ai * ai, a2i = 2.0 * ar * ai;
    const double a3r = a2r * ar - a2i * ai, a3i = a2r * ai + a2i * ar;         // (1 + 1 / p_1)^3
    const double fr = 1.0 - c.p0 * ir, fi = -c.p0 * ii;                        // 1 - p_0 / p_1
    const double g2r = c.p1r * ir + c.p1i * ii, g2i = c.p1r * ii - c.p1i * ir; // p_2 / p_1 = conj(p_1) / p_1
    const double gr = 1.0 - g2r, gi = -g2i;
    const double hr = fr * gr - fi * gi, hi = fr * gi + fi * gr, hn = hr * hr + hi * hi;
    c.r1r = b0 * (a3r * hr + a3i * hi) / hn; c.r1i = b0 * (a3i * hr - a3r * hi) / hn;
    c.g = b0 - 2.0 * c.r1r;
    return c;
}
// (ar + i ai)(br + i bi) + (cr + i ci) with explicit fused multiply-adds: the same roundings wherever it is inlined
__device__ __forceinline__ void lp_cfma(const double ar, const double ai, const double br, const double bi, const double cr, const double ci, double& zr, double& zi)
{
    const double r = __builtin_fma(ar, br, __builtin_fma(-ai, bi, cr)), q = __builtin_fma(ar, bi, __builtin_fma(ai, br, ci));
    zr = r; zi = q;
}
// one window; every thread of a 256-thread workgroup calls it.  y receives the last ysz samples (all NaN if !c.ok).  The same function serves
// st_lowpass and the feed, so both give identical y.  L, ysz: any 0 < ysz <= L (runs and chunks may be ragged at the window's end).
__device__ __forceinline__ void
lowpass_window(const float* __restrict__ xb, float* __restrict__ yb, const LpCoef c, const int L, const int ysz, LpLds* __restrict__ s)
{
#pragma clang fp contract(off)
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, i0 = t * LP_R;
    if (!c.ok) {                                                               // workgroup-uniform
        for (int j = t; j < ysz; j += 256) yb[j] = __builtin_nanf("");
        return;
    }
    if (t == 0) { s->c0 = 0.0; s->c1r = 0.0; s->c1i = 0.0; }
    for (int c0 = 0; c0 < L; c0 += LP_CH) {
        const int n = L - c0 < LP_CH ? L - c0 : LP_CH;
        const bool out = c0 + n > L - ysz;                                     // workgroup-uniform: the chunk reaches the stored samples
        for (int i = t; i < LP_CH; i += 256) s->x[i + i / LP_R] = i < n ? xb[c0 + i] : 0.f;
        __syncthreads();
        double xv[LP_R];
#pragma unroll
        for (int k = 0; k < LP_R; ++k) xv[k] = (double)s->x[t * (LP_R + 1) + k];
        // the run's maps from a zero start: s -> A s + B with A = p^m
        double A0 = 1.0, B0 = 0.0, A1r = 1.0, A1i = 0.0, B1r = 0.0, B1i = 0.0;
#pragma unroll
        for (int k = 0; k < LP_R; ++k) {
            if (i0 + k >= n) break;
            A0 *= c.p0; B0 = __builtin_fma(c.p0, B0, xv[k]);
            lp_cfma(A1r, A1i, c.p1r, c.p1i, 0.0, 0.0, A1r, A1i);
            lp_cfma(c.p1r, c.p1i, B1r, B1i, xv[k], 0.0, B1r, B1i);
        }
        // inclusive scan over the wave: this map after the one of lanes below, (A, B) o (Ao, Bo) = (A Ao, A Bo + B)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double Ao0 = __shfl_up(A0, o), Bo0 = __shfl_up(B0, o);
            const double Aor = __shfl_up(A1r, o), Aoi = __shfl_up(A1i, o), Bor = __shfl_up(B1r, o), Boi = __shfl_up(B1i, o);
            if (lane >= o) {
                B0 = __builtin_fma(A0, Bo0, B0); A0 *= Ao0;
                lp_cfma(A1r, A1i, Bor, Boi, B1r, B1i, B1r, B1i);
                lp_cfma(A1r, A1i, Aor, Aoi, 0.0, 0.0, A1r, A1i);
            }
        }
        if (lane == 63) { s->wa0[w] = A0; s->wb0[w] = B0; s->wa1r[w] = A1r; s->wa1i[w] = A1i; s->wb1r[w] = B1r; s->wb1i[w] = B1i; }
        double Ae0 = __shfl_up(A0, 1), Be0 = __shfl_up(B0, 1);
        double Aer = __shfl_up(A1r, 1), Aei = __shfl_up(A1i, 1), Ber = __shfl_up(B1r, 1), Bei = __shfl_up(B1i, 1);
        if (lane == 0) { Ae0 = 1.0; Be0 = 0.0; Aer = 1.0; Aei = 0.0; Ber = 0.0; Bei = 0.0; }
        __syncthreads();
        double s0 = s->c0, s1r = s->c1r, s1i = s->c1i;                         // the states at sample c0 - 1
        for (int v = 0; v < w; ++v) {
            s0 = __builtin_fma(s->wa0[v], s0, s->wb0[v]);
            lp_cfma(s->wa1r[v], s->wa1i[v], s1r, s1i, s->wb1r[v], s->wb1i[v], s1r, s1i);
        }
        s0 = __builtin_fma(Ae0, s0, Be0);
        lp_cfma(Aer, Aei, s1r, s1i, Ber, Bei, s1r, s1i);                       // the states before the run
#pragma unroll
        for (int k = 0; k < LP_R; ++k) {
            if (i0 + k >= n) break;
            lp_cfma(c.p1r, c.p1i, s1r, s1i, xv[k], 0.0, s1r, s1i);
            if (out) s->y[i0 + k] = (float)__builtin_fma(c.g, xv[k], __builtin_fma(c.q0, s0, 2.0 * __builtin_fma(c.r1r, s1r, -(c.r1i * s1i))));      // s0 is still s0[n-1]
            s0 = __builtin_fma(c.p0, s0, xv[k]);
        }
        __syncthreads();
        if (t == 255) { s->c0 = s0; s->c1r = s1r; s->c1i = s1i; }             // read after the next chunk's second barrier
        if (out) {
            for (int i = t; i < n; i += 256) {
                const int j = c0 + i - (L - ysz);
                if (j >= 0) yb[j] = s->y[i];
            }
        }
    }
}
// st_lowpass: knobs_wc [B][1] = the cutoff in Hz; one workgroup per window
__global__ void __launch_bounds__(256)
lowpass_kernel(const float* __restrict__ x, const float* __restrict__ knobs_wc, const float sr, const int L, const int ysz, float* __restrict__ y)
{
    __shared__ LpLds s;
    const int b = blockIdx.x;
    lowpass_window(x + (size_t)b * L, y + (size_t)b * ysz, lowpass_coef((double)knobs_wc[b], (double)sr), L, ysz, &s);
}

}  // namespace stm
