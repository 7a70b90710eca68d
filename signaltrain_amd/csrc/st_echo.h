// st_echo.h -- the reference's Echo effect (audio.py:430-443, echo()): up to ST_ECHO_MAX delayed, attenuated copies of the window added to it,
// with a fractional delay as a two-tap linear interpolation (gfx950).  Per row, with knobs (delay in samples, ratio, echoes):
//   E = rint(echoes)                                        (round half to even, as np.round)
//   y[n] = x[n];   for i = 1 .. E:
//       dl = i * (double)delay,  D = floor(dl),  diff = dl - D,   w0 = (float)(1 - diff),  w1 = (float)diff,  c = (float)pow((double)ratio, i)
//       xd = w0 * x[n - D] + w1 * x[n - D - 1]              (x[m] = 0 for m < 0: the reference pads with zeros)
//       y[n] = y[n] + c * xd
// float64 only for the delay length and the power; every float32 product and sum is rounded on its own (contraction off), which is what numpy
// computes on a float32 window with Python-float weights.  Nothing is skipped where a tap falls before the window: the reference adds c * 0 there
// too (a -0 sample becomes +0, an infinite power times zero a NaN).
// No recurrence: every output sample reads 1 + 2 E input samples of its own row, which the row's first reader brings into L2.  One 256-thread workgroup
// per (window, tile of the tail); the E taps are worked out once per workgroup (lane i < E: one float64 pow each) and kept in LDS.  A delayed read is
// unaligned by nature, so loads and stores are one float per lane, consecutive lanes on consecutive samples; any L.
// A row whose knobs cannot be an echo -- a delay that is not a finite number >= 1 (the reference raises at 0), rint(echoes) outside 0 .. ST_ECHO_MAX,
// a NaN knob -- is all NaN, and only that row (the knobs are device data: the host cannot refuse them).
#pragma once
#include "st_common.h"

namespace stm {

struct EchoTap { int D; float w0, w1, c; };           // echo i: delay floor(i delay) clamped to L (every read before the window), interpolation weights, ratio^i
struct EchoLds { EchoTap tap[ST_ECHO_MAX]; };
// The last ysz samples of one window's echo from sample j0 of the tail on, every `stride` samples' worth of 256-sample trips (j = j0 + threadIdx.x + k * stride).
// Every thread of a 256-thread workgroup calls it; s is the workgroup's.  The same function serves st_echo and the feed, so both give identical y.
__device__ __forceinline__ void
echo_window(const float* xb, float* yb, const float delay, const float ratio, const float echoes, const int L, const int ysz, const int j0, const int stride,
            EchoLds* s)
{
#pragma clang fp contract(off)      // every product and sum as written, wherever the function is inlined
    const float er = rintf(echoes);
    const bool ok = delay >= 1.0f && delay <= 3.402823466e38f && er >= 0.0f && er <= (float)ST_ECHO_MAX && ratio == ratio;      // false for NaN knobs
    const int E = ok ? (int)er : 0;
    if ((int)threadIdx.x < E) {
        const int i = (int)threadIdx.x + 1;
        const double dl = (double)i * (double)delay, Dd = floor(dl), diff = dl - Dd;
        EchoTap t;
        t.D = Dd < (double)L ? (int)Dd : L;
        t.w0 = (float)(1.0 - diff); t.w1 = (float)diff; t.c = (float)pow((double)ratio, (double)i);
        s->tap[threadIdx.x] = t;
    }
    __syncthreads();
    const int n0 = L - ysz;
    for (int j = j0 + (int)threadIdx.x; j < ysz; j += stride) {
        const int n = n0 + j;
        float v = xb[n];
        for (int i = 0; i < E; ++i) {
            const EchoTap t = s->tap[i];
            const int m = n - t.D;
            const float a = m >= 0 ? xb[m] : 0.0f, b = m >= 1 ? xb[m - 1] : 0.0f;
            const float p0 = t.w0 * a, p1 = t.w1 * b;
            const float xd = p0 + p1;
            const float e = t.c * xd;
            v = v + e;
        }
        yb[j] = ok ? v : __builtin_nanf("");
    }
}
// st_echo: knobs_wc [B][3] = (delay in samples, ratio, echoes); workgroup (b, tile): window b = blockIdx.x, tiles of the tail along blockIdx.y
__global__ void __launch_bounds__(256)
echo_kernel(const float* __restrict__ x, const float* __restrict__ knobs_wc, const int L, const int ysz, float* __restrict__ y)
{
    __shared__ EchoLds s;
    const int b = blockIdx.x;
    echo_window(x + (size_t)b * L, y + (size_t)b * ysz, knobs_wc[3 * (size_t)b], knobs_wc[3 * (size_t)b + 1], knobs_wc[3 * (size_t)b + 2], L, ysz,
                (int)blockIdx.y * 256, (int)gridDim.y * 256, &s);
}

}  // namespace stm
