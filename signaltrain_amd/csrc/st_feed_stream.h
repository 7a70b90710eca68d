// st_feed_stream.h -- the live feed of recorded input with the effect's HISTORY (gfx950): st_live_feed_stream, the STREAMED target of st_live_feed.
//
// st_live_feed (st_feed_live.h) starts every effect from its zero state at the first sample of the window: the reference's chunked target
// (target_type="chunk").  The reference's default, and what its results rest on, is the streamed target: the effect has run over the whole recording
// (gen_dataset.py:135-136) and a window's target carries the state the effect had reached when the window began.  Here the effect runs over up to
// `preroll` samples of the window's own file in front of the window, the PRE-ROLL; only the window (x) and the effect's tail (y) leave.  With a
// pre-roll that reaches the head of the file the target is the streamed render of that file at the window's knob setting.  preroll = 0 is st_live_feed.
//
// THE LAW.  Window w = first_window + b of stream `seed` has exactly st_live_feed's draws (st_feed_live.h: synthetic, file, start, flipped = indices 16..19
// of the second sequence, datasets.live_feed_draw their host replica; the knobs the first draws of the first sequence; the world knobs by the synthetic
// feed's rule); meta [B][4] is st_live_feed's.  On top of that, with `start` the clamped value that goes into meta[2]:
//   R     = min(preroll, start & ~3)                       preroll % 4 == 0, so R % 4 == 0: at most three samples at a file's head stay out of the history
//   xe[n] = +-pool[file_off[file] + start - R + n],        n in [0, R + L): the polarity flip covers the whole span; ST_PCM_S16 converts as in st_file_feed
//   x     = xe[R:]                                         st_live_feed's x, bit for bit (except ST_FX_DENOISE / ST_FX_DECOMP4C, below)
// and per effect, through the device functions the live feed calls, so that the library's own entries on xe reproduce every row:
//   ST_FX_COMP4C    y = last ysz of st_compressor_4c(xe)
//   ST_FX_COMP      y = last ysz of st_compressor(xe)      the envelope starts at d[0] of the extended span
//   ST_FX_LOWPASS   y = last ysz of st_lowpass(xe)
//   ST_FX_ECHO      y = last ysz of st_echo(xe)            the delayed copies read recorded history instead of zeros
//   ST_FX_DENOISE   st_live_feed's row, bit for bit        no state; the noise index is relative to the window (R = 0 for this effect's loads)
//   ST_FX_DECOMP4C  y = the clean tail, x = last L of st_compressor_4c(xe)
// A synthetic row (synth_prob > 0) has no history: row w of st_synth_effect_families, bit for bit, as in st_live_feed.  A recorded row depends on
// (seed, w), the pool and preroll only -- not on synth_prob, the batching or the other rows.
//
// Addresses: feed_span's clamps first (st_feed_files.h: file < nfiles, off + start in [0, pool_samples - L]), then start = clamp(base - file_off[file], 0, base) and R from
// that, so base - R >= 0: whatever the tables say, every address formed lies inside the pool, and with truthful tables the history never leaves the window's file.
//
// HOW IT RUNS.  One 256-lane workgroup per window, quads loaded before the first store, file_quad for unaligned spans, as live_feed_kernel.  The scratch holds
// one buffer buf [B][P], P = round_up(preroll + L, 64), with every row RIGHT-aligned: row b's span is buf[b][P - R - L .. P), so rows with a short history share
// the pitch.
//   ST_FX_COMP / ST_FX_LOWPASS / ST_FX_ECHO: buf is the float image of xe; the workgroup then runs env_compressor_window / lowpass_window / echo_window on
//     (buf[b] + P - R - L, R + L): a pointer into the row and a length, so e[0] = d[0] and the zero-state starts fall on the row's true first sample.
//   ST_FX_COMP4C / ST_FX_DECOMP4C: buf is the static gain curve of xe, 0 over the missing prefix AND at the true first sample.  The attack / release state
//     starts at 0 and a gain of 0 leaves it at exactly 0 (g + a (0 - g) with g = 0), which is the reference's lin_A[0] = 0: the chain may start anywhere in
//     the prefix.  stream_smooth_kernel is comp_smooth_kernel's chain (one lane per window, same step arithmetic: bit-identical) at pitch P; it starts at the
//     first 64-sample tile any of its 64 rows has data in, skips synthetic rows, and stores only the tiles the apply kernels read -- history samples advance
//     the state and leave nothing.  stream_apply_kernel then writes y from (x's tail, gain), stream_apply_inplace_kernel compresses x in place: each sample
//     is read and written once by one thread, and neither touches a synthetic row (rr[b] < 0), whose own chain ran at pitch L before.
// The sequential chain is the cost: it grows with (preroll + L) / L (profiles/stream_feed_throughput.txt).
#pragma once
#include "st_feed_live.h"

namespace stf {

struct StreamFeedArgs {
    LiveFeedArgs live;                      // gc / kw unused here: the stream form's scratch is below
    float* buf;                             // [B][P]: xe's float image, or its static gain curve (ST_FX_COMP4C / ST_FX_DECOMP4C); NULL for ST_FX_DENOISE
    float* kw;                              // [B][4] world knobs of the recorded rows
    int* rr;                                // [B]: the row's R, or -1 for a synthetic row
    int P, preroll;
};

template <int FX, typename T>
__global__ void __launch_bounds__(256)
stream_feed_kernel(const StreamFeedArgs s)
{
    extern __shared__ __attribute__((aligned(16))) float stream_lds[];    // float[COMP_CH]: the in-workgroup effect's buffer (ST_FX_COMP / LOWPASS / ECHO)
    const LiveFeedArgs& a = s.live;
    const int b = blockIdx.x, L = a.L;
    const unsigned key = feed_key(a.seed, a.first + (unsigned long long)b);

    // ---- the window's four scalar draws: st_live_feed's, clamps included
    const unsigned key2 = feed_key2(key);
    const bool synthetic = u01(h2(key2, 16u)) < a.synth_prob;
    const auto [f, base, flip] = feed_span(h2(key2, 17u), h2(key2, 18u), h2(key2, 19u), a.file_off, a.file_len, a.nfiles, L, a.pool_samples, a.augment);
    const long long start = base - a.file_off[f];
    if (a.meta && threadIdx.x == 64) {
        long long* m = a.meta + (size_t)b * 4;
        m[0] = synthetic ? 1 : 0; m[1] = f; m[2] = start; m[3] = flip ? 1 : 0;
    }
    if (synthetic) {                                                 // workgroup-uniform: the row is synth_feed_kernel's
        if (threadIdx.x == 0) s.rr[b] = -1;
        return;
    }
    // ---- the history: R samples of the same file in front of the window; base - R >= 0 whatever the tables say
    const long long sc = start < 0 ? 0 : (start > base ? base : start);
    const long long hist = sc & ~3LL;
    const int R = FX == ST_FX_DENOISE ? 0 : (int)(hist < (long long)s.preroll ? hist : (long long)s.preroll);

    // ---- the knobs: st_live_feed's (st_feed.h: feed_knobs)
    Draw d{key, 0u};
    float kn[4], kw[4];
    feed_knobs<FX>(d, a.lo, a.hi, a.K, kn, kw);

    // ---- the extended span: LIVE_TRIPS quads per lane and trip, all loads before the first store; the window's part goes to x (and y), the whole of it,
    // as samples or as their static gain, into the row's right-aligned place in buf
    constexpr bool GAIN = FX == ST_FX_COMP4C || FX == ST_FX_DECOMP4C;
    const T* __restrict__ src = reinterpret_cast<const T*>(a.pool) + (base - (long long)R);
    float* __restrict__ xb = a.x + (size_t)b * L;
    float* __restrict__ yb = a.y + (size_t)b * a.ysz;
    const unsigned len = (unsigned)(R + L), hist_n = (unsigned)R, tail = (unsigned)(L - a.ysz);
    const unsigned pad = (unsigned)s.P - len;                        // % 4 == 0
    float* eb = FX == ST_FX_DENOISE ? nullptr : s.buf + (size_t)b * s.P + pad;
    if (GAIN) {                                                      // the missing prefix: gain 0 keeps the state at 0
        float* __restrict__ zb = s.buf + (size_t)b * s.P;
        for (unsigned i = 4u * threadIdx.x; i < pad; i += 4u * 256u) *reinterpret_cast<float4*>(zb + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float sg = flip ? -1.f : 1.f;
    for (unsigned i0 = 0; i0 < len; i0 += 4u * 256u * LIVE_TRIPS) {
        float4 q[LIVE_TRIPS];
        load_quads<LIVE_TRIPS>(src, i0, len, q);
#pragma unroll
        for (int t = 0; t < LIVE_TRIPS; ++t) {
            const unsigned i = quad_at(i0, t);
            if (i >= len) continue;                                  // len % 4 == 0: a quad lies inside the span or outside it
            float4 v = quad_sign(q[t], sg);
            if (GAIN) {
                float4 g = comp_gain_curve4(v, kw[0], kw[1]);
                if (i == 0u) g.x = 0.f;                              // lin_A[0] = 0 at the span's true first sample
                *reinterpret_cast<float4*>(eb + i) = g;
            } else if (FX != ST_FX_DENOISE) {
                *reinterpret_cast<float4*>(eb + i) = v;
            }
            if (i < hist_n) continue;                                // R % 4 == 0: a quad is history or window
            const unsigned j = i - hist_n;
            if (FX == ST_FX_DENOISE || FX == ST_FX_DECOMP4C) {       // the target is the clean tail
                if (j >= tail) *reinterpret_cast<float4*>(yb + (j - tail)) = v;
            }
            if (FX == ST_FX_DENOISE) v = denoise_add4(key, j, kw[0], v);      // the noise index is relative to the window
            *reinterpret_cast<float4*>(xb + j) = v;
        }
    }
    if (threadIdx.x == 0) {
        for (int k = 0; k < 4; ++k) if (k < a.K) a.knobs[(size_t)b * a.K + k] = kn[k];
        for (int k = 0; k < 4; ++k) s.kw[(size_t)b * 4 + k] = kw[k];
        s.rr[b] = R;
    }
    if (FX == ST_FX_DENOISE || GAIN) return;                         // GAIN: stream_smooth_kernel and an apply kernel finish the row
    // ---- the effect over the extended span, inside this workgroup: a pointer into the row and a length
    __threadfence_block();
    __syncthreads();
    const float* xe = eb;
    const int n = (int)len;
    if (FX == ST_FX_LOWPASS) {
        stm::lowpass_window(xe, yb, stm::lowpass_coef((double)kw[0], (double)a.sr), n, a.ysz, reinterpret_cast<stm::LpLds*>(stream_lds));
        return;
    }
    if (FX == ST_FX_ECHO) {
        stm::echo_window(xe, yb, kw[0], kw[1], kw[2], n, a.ysz, 0, 256, reinterpret_cast<stm::EchoLds*>(stream_lds));
        return;
    }
    stm::env_compressor_window(xe, nullptr, yb, (double)kw[0], (double)kw[1], stm::env_coef((double)kw[2], (double)a.sr), n, a.ysz, reinterpret_cast<stm::EnvLds*>(stream_lds));
}

// comp_smooth_kernel's chain (st_misc.h: one lane per window, [64 windows][64 samples] tiles through LDS, the same step arithmetic) over the right-aligned
// rows g [B][P] of the stream feed.  The block starts at the first tile any of its rows has data in (gain 0 in front keeps the state at 0, so a row may join
// early), reads zeros for synthetic rows (rr < 0: their part of g was never written) and stores only tiles from `keep0` on, the ones an apply kernel reads.
// Requires P % 64 == 0.
__global__ void __launch_bounds__(64)
stream_smooth_kernel(float* __restrict__ g, const float* __restrict__ kw, const int* __restrict__ rr, const float sr, const int B, const int L, const int P, const int keep0)
{
    __shared__ float tile[64][65];
    const int lane = threadIdx.x, b0 = blockIdx.x * 64, b = b0 + lane;
    const int r = b < B ? rr[b] : -1;
    const unsigned long long alive = __ballot(r >= 0);               // bit i: row b0 + i is a recorded row
    if (alive == 0ull) return;                                       // wave-uniform (the block is one wave)
    int c_begin = r >= 0 ? P - r - L : P;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int v = __shfl_xor(c_begin, o); c_begin = v < c_begin ? v : c_begin; }
    c_begin &= ~63;
    const float k2 = r >= 0 ? kw[4 * (size_t)b + 2] : 1.f, k3 = r >= 0 ? kw[4 * (size_t)b + 3] : 1.f;
    const double alphaA = exp(-log(9.0) / ((double)sr * (double)k2));
    const double alphaR = exp(-log(9.0) / ((double)sr * (double)k3));
    const int q = lane >> 4, c4 = 4 * (lane & 15);
    float prev = 0.f;
    float4 nx[16];                                         // the next tile, loaded while this one's chain runs
    auto load = [&](const int c0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = 4 * i + q;
            nx[i] = (alive >> row) & 1ull ? *reinterpret_cast<const float4*>(g + (size_t)(b0 + row) * P + c0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    load(c_begin);
    for (int c0 = c_begin; c0 < P; c0 += 64) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = 4 * i + q;
            tile[row][c4] = nx[i].x; tile[row][c4 + 1] = nx[i].y; tile[row][c4 + 2] = nx[i].z; tile[row][c4 + 3] = nx[i].w;
        }
        __syncthreads();
        load(c0 + 64 < P ? c0 + 64 : c0);
        float gv[64];
#pragma unroll
        for (int k = 0; k < 64; ++k) gv[k] = tile[lane][k];
#pragma unroll
        for (int k = 0; k < 64; ++k) {                      // no first-sample case: the feed kernel wrote gain 0 there, which leaves prev = 0 and puts out 0
            const float gi_f = gv[k];
            const double a = gi_f < prev ? alphaA : alphaR;
            const double gi = gi_f;
            prev = (float)__builtin_fma(a, (double)prev - gi, gi);
            gv[k] = prev;
        }
        if (c0 < keep0) { __syncthreads(); continue; }      // block-uniform: a history tile advances the state and leaves nothing
#pragma unroll
        for (int k = 0; k < 64; ++k) tile[lane][k] = gv[k];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) {                      // smoothed gain back in place, coalesced rows
            const int row = 4 * i + q;
            if ((alive >> row) & 1ull) *reinterpret_cast<float4*>(g + (size_t)(b0 + row) * P + c0 + c4) = make_float4(tile[row][c4], tile[row][c4 + 1], tile[row][c4 + 2], tile[row][c4 + 3]);
        }
        __syncthreads();
    }
}
// dB -> linear and apply (comp_apply_kernel's arithmetic) on the last ysz samples of the recorded rows: x [B][L], g [B][P]
__global__ void __launch_bounds__(256)
stream_apply_kernel(const float* __restrict__ x, const float* __restrict__ g, const int* __restrict__ rr, const int L, const int P, const int ysz, float* __restrict__ y)
{
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= ysz || rr[b] < 0) return;
    y[(size_t)b * ysz + j] = stm::comp_db_to_lin(g[(size_t)b * P + (P - ysz) + j]) * x[(size_t)b * L + (L - ysz) + j];
}
// ... over the whole window of the recorded rows, in place (ST_FX_DECOMP4C).  Each sample is read and written by one thread, once.
__global__ void __launch_bounds__(256)
stream_apply_inplace_kernel(float* x, const float* __restrict__ g, const int* __restrict__ rr, const int L, const int P)
{
    const int b = blockIdx.y;
    if (rr[b] < 0) return;
    const size_t r = (size_t)b * L, gr = (size_t)b * P + (P - L);
    for (int n = blockIdx.x * 256 + threadIdx.x; n < L; n += gridDim.x * 256) x[r + n] = stm::comp_db_to_lin(g[gr + n]) * x[r + n];
}

}  // namespace stf
