// st_feed_live.h -- the training feed of RECORDED input through a LIVE effect (gfx950): st_live_feed.
//
// The case SignalTrain is used for: recorded audio (music, speech) through a software effect whose knobs vary continuously.  The reference reaches
// it only by rendering a dataset first (gen_dataset.py --inpath: wav pairs at one knob setting per file) and carries an unused `synthprob` argument
// for mixing test tones with recordings (run_train.py:82-87).  Here one 256-lane workgroup makes one training item, as synth_feed_kernel does, but
// the window's signal is a span of the device-resident audio pool of st_file_feed (st_feed_files.h) instead of a generated test signal: the knobs
// are drawn per window and the effect runs on the spot, through the device functions the synthetic feed calls (compressor_window,
// env_compressor_window, lowpass_window, echo_window, denoise_add, compressor_window_inplace).
//
// THE DRAW LAW.  Window b of a launch is window w = first_window + b of the stream `seed`; key = feed_key(seed, w) is the key of every feed of
// this library.  The four scalar draws use indices 16 to 19 of the second, loop-free sequence of st_feed.h (integer hashes; datasets.live_feed_draw
// is their host replica):   key2 = feed_key2(key),   h_i = mix32(key2 + 0x9E3779B9 i),   u_i = (h_i >> 8) / 2^24,   below(h, n) = (uint64 h * n) >> 32
//   16  synthetic  iff u_16 < synth_prob (float32 compare): 0 = never, 1 = always
//   17, 18, 19  (file, start, flipped) = feed_span(h_17, h_18, h_19, ...)   (st_feed_files.h: THE SPAN CHOICE of every feed of recorded input)
// Every window has all four draws, whatever it turns out to be; meta [B][4] = (synthetic, file, start, flipped) records them.
// A RECORDED window is x[n] = +-pool[file_off[file] + start + n] (ST_PCM_S16: (float)s / 32767.0f, st_feed_files.h), minus where flipped.  It gets
// neither the 1e-8 noise nor the random polarity of audio.py:334: those belong to synth_input_sample, and the reference's file dataset flips only
// under `augment`.  Its knobs are kn[k] = Draw{key, 0}.beta(0.8f) - 0.5f, k = 0..3 -- the first draws of the first sequence, all four drawn whatever
// K is -- and its world knobs follow the synthetic feed's rule (st_feed.h: the same arithmetic, knobs past K fixed at their low end, the float32
// forms of LowPass / Denoise / Echo), so st_compressor_4c / st_compressor / st_lowpass / st_echo / st_denoise_input on (x, these knobs) reproduce y.
// ST_FX_DENOISE: y is the clean tail and x leaves with denoise_add on it (stream 11 of the window key).  ST_FX_DECOMP4C: y is the clean tail and x
// becomes the compressed window.
// A SYNTHETIC window is, bit for bit, row w of st_synth_effect_families(effect, family_mask, seed, ...): synth_feed_kernel generates the whole batch
// first and this kernel then overwrites the recorded rows (a synthetic row's workgroup leaves after its meta).  Both kernels leave the compressors'
// gain curve (ST_FX_COMP: dB signal) and world knobs in the scratch, and ONE chain of comp_smooth_kernel + comp_apply_kernel / compressor_env_kernel /
// comp_apply_inplace_kernel finishes every row afterwards: comp_smooth_kernel works in place, so no row may pass it twice.
// Every output row is a function of (seed, w) and the pool only, whatever the batching and whatever the other rows are.
//
// Addresses, as in st_file_feed: feed_span's clamps keep every address formed inside the pool, whatever the tables say.  A span starts at ANY sample:
// the loads go through load_quads / file_quad's vector types declared with the element's alignment.  Destination rows are 16-byte aligned
// (L % 4 == ysz % 4 == 0): 16-byte stores.
#pragma once
#include "st_feed_files.h"

namespace stf {

constexpr int LIVE_TRIPS = 4;               // quads of 4 samples a lane loads before its first store

struct LiveFeedArgs {
    const void* pool; const long long* file_off; const long long* file_len;
    float* x; float* y; float* knobs; long long* meta;      // meta [B][4] or NULL
    float* gc; float* kw;                   // optional scratch [B][L] + [B][4], as FeedArgs': the effect finishes in the next launches; NULL: inside this kernel
    long long pool_samples;
    unsigned seed; unsigned long long first;
    int L, ysz, K, nfiles, augment;
    float sr, synth_prob;
    float lo[4], hi[4];                     // knob ranges
};

template <int FX, typename T>
__global__ void __launch_bounds__(256)
live_feed_kernel(const LiveFeedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float live_lds[];      // float[COMP_CH]: the in-workgroup effect's buffer
    __shared__ float carry;
    const int b = blockIdx.x, L = a.L;
    const unsigned key = feed_key(a.seed, a.first + (unsigned long long)b);

    // ---- the window's four scalar draws (law: top of this file)
    const unsigned key2 = feed_key2(key);
    const bool synthetic = u01(h2(key2, 16u)) < a.synth_prob;
    const auto [f, base, flip] = feed_span(h2(key2, 17u), h2(key2, 18u), h2(key2, 19u), a.file_off, a.file_len, a.nfiles, L, a.pool_samples, a.augment);
    if (a.meta && threadIdx.x == 64) {
        long long* m = a.meta + (size_t)b * 4;
        m[0] = synthetic ? 1 : 0; m[1] = f; m[2] = base - a.file_off[f]; m[3] = flip ? 1 : 0;
    }
    if (synthetic) return;                                           // workgroup-uniform: the row is synth_feed_kernel's

    // ---- the knobs: the first draws of the first sequence, world values by the synthetic feed's rule (st_feed.h: feed_knobs)
    Draw d{key, 0u};
    float kn[4], kw[4];
    feed_knobs<FX>(d, a.lo, a.hi, a.K, kn, kw);

    // ---- the window: LIVE_TRIPS quads per lane and trip, all loads before the first store; with the second-launch form of the effect the static
    // gain curve of each sample right away, from the value in registers
    const T* __restrict__ src = reinterpret_cast<const T*>(a.pool) + base;
    float* __restrict__ xb = a.x + (size_t)b * L;
    float* __restrict__ yb = a.y + (size_t)b * a.ysz;
    float* __restrict__ gcb = a.gc ? a.gc + (size_t)b * L : nullptr;
    const float sg = flip ? -1.f : 1.f;
    const unsigned len = (unsigned)L, tail = (unsigned)(L - a.ysz);
    for (unsigned i0 = 0; i0 < len; i0 += 4u * 256u * LIVE_TRIPS) {
        float4 q[LIVE_TRIPS];
        load_quads<LIVE_TRIPS>(src, i0, len, q);
#pragma unroll
        for (int t = 0; t < LIVE_TRIPS; ++t) {
            const unsigned i = quad_at(i0, t);
            if (i >= len) continue;                                  // L % 4 == 0: a quad lies inside the row or outside it
            float4 v = quad_sign(q[t], sg);
            if (FX == ST_FX_DENOISE || FX == ST_FX_DECOMP4C) {       // the target is the clean tail (ysz % 4 == 0: whole quads) ...
                if (i >= tail) *reinterpret_cast<float4*>(yb + (i - tail)) = v;
            }
            if (FX == ST_FX_DENOISE) v = denoise_add4(key, i, kw[0], v);      // ... and the input leaves with the noise on it
            *reinterpret_cast<float4*>(xb + i) = v;
            if (gcb) *reinterpret_cast<float4*>(gcb + i) = FX == ST_FX_COMP ? env_db4(v) : comp_gain_curve4(v, kw[0], kw[1]);
        }
    }
    if (threadIdx.x == 0) { for (int k = 0; k < 4; ++k) if (k < a.K) a.knobs[(size_t)b * a.K + k] = kn[k]; }
    if (FX == ST_FX_DENOISE) return;
    if (a.gc) {                                                      // workgroup-uniform: the effect finishes in the next launches
        if (threadIdx.x == 0) { for (int k = 0; k < 4; ++k) a.kw[(size_t)b * 4 + k] = kw[k]; }
        return;
    }
    // ---- the effect on the finished window, inside this workgroup: what synth_feed_kernel does after its barrier
    __threadfence_block();
    __syncthreads();
    if (FX == ST_FX_LOWPASS) {
        stm::lowpass_window(xb, yb, stm::lowpass_coef((double)kw[0], (double)a.sr), L, a.ysz, reinterpret_cast<stm::LpLds*>(live_lds));
        return;
    }
    if (FX == ST_FX_ECHO) {
        stm::echo_window(xb, yb, kw[0], kw[1], kw[2], L, a.ysz, 0, 256, reinterpret_cast<stm::EchoLds*>(live_lds));
        return;
    }
    if (FX == ST_FX_COMP) {
        stm::env_compressor_window(xb, nullptr, yb, (double)kw[0], (double)kw[1], stm::env_coef((double)kw[2], (double)a.sr), L, a.ysz, reinterpret_cast<stm::EnvLds*>(live_lds));
        return;
    }
    const double alphaA = exp(-log(9.0) / ((double)a.sr * (double)kw[2])), alphaR = exp(-log(9.0) / ((double)a.sr * (double)kw[3]));
    if (FX == ST_FX_DECOMP4C) {                                      // the compressed window is the item's input: over the whole of x, in place
        stm::compressor_window_inplace(xb, (double)kw[0], (double)kw[1], alphaA, alphaR, L, live_lds, &carry);
        return;
    }
    stm::compressor_window(xb, yb, (double)kw[0], (double)kw[1], alphaA, alphaR, L, a.ysz, live_lds, &carry);
}

}  // namespace stf
