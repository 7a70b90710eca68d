// st_feed.h -- the comp_4c training feed as ONE kernel per minibatch (gfx950): SURVEY.md 8(f)-1.
//
// Reference: datasets.py:312-334 (SynthAudioDataSet.gen_single_chunk: chooser in {0, 1, 2, 4, 6, 7}, knobs = Beta(0.8, 0.8) - 0.5, target = effect
// output's last y_size samples, random polarity flip of the pair :27-29) over audio.py:85-196 / :296-334 (the test signals) and
// audio.py:380-426 (compressor_4controls).  Round 2 evaluated the signals with a few dozen torch launches per batch (2.9 ms per 256
// windows) and a separate compressor launch; here one workgroup makes one training item end to end:
//   draw   the window's parameters from a counter-based generator keyed by (seed, global window index): no state, no host RNG, any number
//          of windows per launch, reproducible per window whatever the batching;
//   pink   1/f noise as the reference builds it -- inverse FFT of the REAL spectrum (2u - 1) / sqrt(k + 1) -- with a radix-2 FFT in LDS
//          (64 KB for the 8192-sample window; longer windows take the noise from a caller-provided buffer);
//   signal the chosen family evaluated per sample, peak-normalised (normish: two passes, the first only takes the maximum), polarity, 1e-8 noise;
//   effect the 4-control compressor on the finished window (stm::compressor_window: parallel gain computer, sequential attack / release
//          smoother in one lane, parallel apply) -> the last ysz samples; or (ST_FX_COMP) the envelope compressor of audio.py:349-371, whose
//          linear envelope runs as a parallel scan (stm::env_compressor_window).  1 <= K <= 4 knobs: the ones past K are fixed at their low end.
//          ST_FX_LOWPASS (audio.py:610-625): the third-order Butterworth low-pass as a scan over the filter's modes (stm::lowpass_window, st_filter.h).
//          ST_FX_DENOISE (audio.py:558-571): the target is the clean window's tail and x leaves with strength * (2u - 1) added (denoise_add).
//          ST_FX_ECHO (audio.py:430-443, :539-547): delayed copies of the finished window added to its tail (stm::echo_window, st_echo.h).
//          ST_FX_DECOMP4C (audio.py:573-583): the target is the clean window's tail and x leaves as the 4-control compressor of the whole window.
// Output contract: x [B][L], y [B][ysz], knobs [B][K] in [-0.5, 0.5] (float32), as the reference's collated batch (train.py:104-120 casts y to float).
// Parity is DISTRIBUTIONAL (another generator than numpy's): tests compare per-family peak ranges, the even symmetry and 1/f slope of the noise,
// the box structure, the Beta(0.8, 0.8) law, and the compressor against golden G9 through the same device function.
//
// Signal families (audio.py:296-334).  0 sine, 1 noisy sine, 2 pluck, 4 box, 6 noisy box, 7 noisy pluck are the compressor's set (datasets.py:317) and
// the kernel it always was (synth_feed_kernel<FX, false>).  synth_feed_kernel<FX, true> adds 3 triangle + 1/f noise, 5 spikes + normal noise,
// 8 ampexpstepup(start_dB = -30), 9 sweep, 10 box + white + 1/f noise, 11 scaled 1/f noise -- with the reference's oddities kept: the spike index is
// int(int(u L - 2) + t[-1]) (two truncations toward zero, index -1 wraps), later spikes overwrite earlier ones, triangle and spikes are not
// peak-normalised, env = 10^(env_dB / 10) in family 8 (env_dB = -30 + (30 n) / (L - 1) in integers == floor(linspace(-30, 0, L))), the sweep's
// constant is 20 whatever f_low is.  The superposition (chooser >= 12) is not built.
//
// THE SECOND DRAW SEQUENCE.  The first sequence (Draw, below: family of the compressor's set, knobs, randsine, pluck, box, normish gain, noise
// amounts, polarity) is unchanged, so the compressor-set stream keeps its bits; it has rejection loops on __powf and therefore no exact host replica.
// Everything the families 3, 5, 8, 9, 10, 11 and a custom family set add is drawn from a second, loop-free sequence that datasets.synth_feed_draw
// replicates exactly on the host:   key2 = mix32(key ^ 0x2545F491),   h_i = mix32(key2 + 0x9E3779B9 i),   u_i = (h_i >> 8) / 2^24 (float32),
// below(h, n) = (h * n) >> 32 (64-bit product).  Every window has every draw, at a fixed index i, in float32 with each step rounded on its own:
//    1  family        member number below(h_1, |set|) of the set in ascending order -- unless the set is {0,1,2,4,6,7}: then the first sequence's law
//    2  tri height    (0.4 u + 0.4) * sign,   3  sign = h_3 >> 31 ? +1 : -1,   4  tri half-width u / 4 * tl,   5  tri t0 = 2 width + 0.4 u tl,
//    6  tri 1/f amount 0.1 u + 0.02          (tl = float32(L - 1) / sr, the last time value;  t_n = float32(n) / sr)
//    7  spikes' normal-noise amount 0.1 u
//    8  step frequency 400 + 4600 u (rad/s, as the reference uses it)
//    9  sweep f_low = 20 + below(h, 980),  10  f_high = 1000 + below(h, 19000),  11  amp_too = below(h, 3) == 2,  12  sweep amplitude 0.9 u
//   13  family 10 white amount 0.2 u,  14  family 10 1/f amount 0.2 u,  15  family 11 1/f amount 0.6 u + 0.2
//   32 + 2 j, 33 + 2 j  (j < 50)  spike j: position int(int(u L - 2) + tl) in float64, height (2 u - 1) * 0.7
// Box (family 10), normish gain (8, 9) and the polarity come from the first sequence.  Per-sample streams: 3 white noise, 5 the 1e-8 noise, 7 the 1/f
// spectrum, 11 Denoise, 13 and 17 the Box-Muller pair of family 5: z_n = sqrt(-2 ln(1 - u13_n)) cos(2 pi u17_n).
#pragma once
#include "st_common.h"
#include "st_misc.h"
#include "st_filter.h"
#include "st_echo.h"

namespace stf {

__device__ __forceinline__ unsigned mix32(unsigned x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float u01(const unsigned h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }      // [0, 1)
struct Draw {              // sequential scalar draws of one window (every thread evaluates the same sequence)
    unsigned key, ctr;
    __device__ unsigned h() { return mix32(key + 0x9E3779B9u * (++ctr)); }      // the next 32-bit hash itself (integer draws: st_feed_files.h)
    __device__ float u() { return u01(mix32(key + 0x9E3779B9u * (++ctr))); }
    __device__ float sign() { return u() < 0.5f ? -1.f : 1.f; }
    __device__ int randint(int lo, int hi) { const int v = lo + (int)(u() * (float)(hi - lo)); return v < hi ? v : hi - 1; }      // [lo, hi)
    // Beta(a, a), a < 1: Joehnk's method (accept x + y <= 1 with x = u^(1/a), y = v^(1/a); acceptance 0.61 for a = 0.8)
    __device__ float beta(const float a) {
        float x = 0.5f, y = 0.5f;
        for (int it = 0; it < 64; ++it) {
            x = __powf(fmaxf(u(), 1e-30f), 1.0f / a); y = __powf(fmaxf(u(), 1e-30f), 1.0f / a);
            if (x + y <= 1.0f && x + y > 0.f) break;
        }
        return x / (x + y);
    }
};
// per-sample streams: value n of stream s of the window
__device__ __forceinline__ float su01(const unsigned key, const unsigned s, const unsigned n) { return u01(mix32(mix32(key ^ (0xA511E9B3u * (s + 1u))) + 0x9E3779B9u * n)); }

// ---- the second draw sequence (law: top of this file)
constexpr unsigned FAMILIES_COMPRESSOR = 0xD7u, FAMILIES_ALL = 0xFFFu;      // bit f = family f
constexpr int N_SPIKES = 50, SPIKE_MAP_BITS = 65536;
__device__ __forceinline__ unsigned feed_key2(const unsigned key) { return mix32(key ^ 0x2545F491u); }
__device__ __forceinline__ unsigned h2(const unsigned key2, const unsigned i) { return mix32(key2 + 0x9E3779B9u * i); }
__device__ __forceinline__ int below(const unsigned h, const int n) { return (int)(((unsigned long long)h * (unsigned long long)(unsigned)n) >> 32); }
struct ExtDraws { float tl, tri_h, tri_w, tri_t0, tri_amp, sp_amp, st_frq, sw_amp, c_white10, c_pink10, c_pink11; int sw_flo, sw_fhi, sw_too; };
__device__ __forceinline__ ExtDraws ext_draws(const unsigned key2, const int L, const float sr)
{
#pragma clang fp contract(off)
    ExtDraws e;
    e.tl = (float)(L - 1) / sr;
    const float th = 0.4f * u01(h2(key2, 2u)) + 0.4f;
    e.tri_h = th * ((h2(key2, 3u) >> 31) ? 1.f : -1.f);
    e.tri_w = u01(h2(key2, 4u)) / 4.f * e.tl;
    const float tc = 0.4f * u01(h2(key2, 5u)) * e.tl;
    e.tri_t0 = 2.f * e.tri_w + tc;
    e.tri_amp = 0.1f * u01(h2(key2, 6u)) + 0.02f;
    e.sp_amp = 0.1f * u01(h2(key2, 7u));
    e.st_frq = 400.f + 4600.f * u01(h2(key2, 8u));
    e.sw_flo = 20 + below(h2(key2, 9u), 980); e.sw_fhi = 1000 + below(h2(key2, 10u), 19000); e.sw_too = below(h2(key2, 11u), 3) == 2;
    e.sw_amp = 0.9f * u01(h2(key2, 12u));
    e.c_white10 = 0.2f * u01(h2(key2, 13u)); e.c_pink10 = 0.2f * u01(h2(key2, 14u));
    e.c_pink11 = 0.6f * u01(h2(key2, 15u)) + 0.2f;
    return e;
}
// spike j of the window: position (audio.py:178, in float64; an index outside the window wraps, as numpy's -1 does) and height
__device__ __forceinline__ void ext_spike(const unsigned key2, const int j, const int L, const float tl, int* loc, float* height)
{
#pragma clang fp contract(off)
    const int i0 = (int)((double)u01(h2(key2, 32u + 2u * (unsigned)j)) * (double)L - 2.0);
    const int i1 = (int)((double)i0 + (double)tl);
    *loc = ((i1 % L) + L) % L;
    const float c = 2.f * u01(h2(key2, 33u + 2u * (unsigned)j)) - 1.f;
    *height = c * 0.7f;
}
__device__ __forceinline__ bool family_wants_pink(const int ch) { return ch == 1 || ch == 7 || ch == 100 || ch == 3 || ch == 10 || ch == 11; }

// The Denoise effect's input (audio.py:571): clean sample v of index n of the window `key` plus strength * (2u - 1), u = value n of stream 11 of the
// window (streams 3, 5 and 7 belong to the signals).  The noise is formed and added in float32, each step rounded on its own, as the reference
// casts its noise to float32 before the sum: contraction is switched off here (HIP's __fmul_rn / __fadd_rn are plain operators and would be fused
// into one FMA with a single rounding), so x - clean is the float32 noise to one rounding of the sum, in the feed and in st_denoise_input alike.
__device__ __forceinline__ float denoise_add(const unsigned key, const unsigned n, const float strength, const float v)
{
#pragma clang fp contract(off)
    const float noise = strength * (2.f * su01(key, 11u, n) - 1.f);
    return v + noise;
}
// Effect.knobs_wc in float32 with every step rounded (what torch gives for float32 tensors): lo + (knob + 0.5) * (hi - lo)
__device__ __forceinline__ float world_knob_f32(const float lo, const float hi, const float kn)
{
#pragma clang fp contract(off)
    const float t = (kn + 0.5f) * (hi - lo);
    return lo + t;
}
// THE KNOB RULE of every feed with drawn knobs (synth_feed_kernel, live_feed_kernel, stream_feed_kernel): kn[k] = Beta(0.8, 0.8) - 0.5 from the next draws of
// `d` -- all four, whatever K is: one stream for every K -- and the world knobs kw[k] = lo + (kn + 0.5) (hi - lo), the ones past K fixed at their low end.
// ST_FX_LOWPASS / ST_FX_DENOISE: the one knob as float32 Effect.knobs_wc gives it, every step rounded.  ST_FX_ECHO: Echo.go_wc (audio.py:547), float32 world
// knobs with the delay and the echo count rounded half to even.  So st_compressor_4c / st_compressor / st_lowpass / st_echo / st_denoise_input on
// (x, these knobs) reproduce the feed bit for bit.
template <int FX>
__device__ __forceinline__ void feed_knobs(Draw& d, const float (&lo)[4], const float (&hi)[4], const int K, float (&kn)[4], float (&kw)[4])
{
    for (int k = 0; k < 4; ++k) { kn[k] = d.beta(0.8f) - 0.5f; kw[k] = lo[k] + (kn[k] + 0.5f) * (hi[k] - lo[k]); }
    for (int k = K; k < 4; ++k) kw[k] = lo[k];
    if (FX == ST_FX_LOWPASS || FX == ST_FX_DENOISE) kw[0] = world_knob_f32(lo[0], hi[0], kn[0]);
    if (FX == ST_FX_ECHO) {
        kw[0] = rintf(world_knob_f32(lo[0], hi[0], kn[0]));
        kw[1] = world_knob_f32(lo[1], hi[1], kn[1]);
        kw[2] = rintf(world_knob_f32(lo[2], hi[2], kn[2]));
    }
}
// four consecutive samples at once: denoise_add on samples n .. n + 3, and what the compressors' second launches read (the static gain curve; ST_FX_COMP: the dB signal)
__device__ __forceinline__ float4 denoise_add4(const unsigned key, const unsigned n, const float strength, const float4 v)
{
    return make_float4(denoise_add(key, n, strength, v.x), denoise_add(key, n + 1u, strength, v.y), denoise_add(key, n + 2u, strength, v.z), denoise_add(key, n + 3u, strength, v.w));
}
__device__ __forceinline__ float4 comp_gain_curve4(const float4 v, const float thresh, const float ratio)
{
    return make_float4(stm::comp_gain_curve(v.x, (double)thresh, (double)ratio), stm::comp_gain_curve(v.y, (double)thresh, (double)ratio),
                       stm::comp_gain_curve(v.z, (double)thresh, (double)ratio), stm::comp_gain_curve(v.w, (double)thresh, (double)ratio));
}
__device__ __forceinline__ float4 env_db4(const float4 v) { return make_float4(stm::env_db(v.x), stm::env_db(v.y), stm::env_db(v.z), stm::env_db(v.w)); }
struct FeedArgs {
    float* x; float* y; float* knobs;       // outputs
    const float* pink_in;                   // [B][L] 1/f noise for windows longer than the in-kernel FFT handles (else NULL): unit-peak from the caller, or
    const float* pink_peak;                 // ... unnormalised from pink_long_pass1 / 2 below with its per-window peak here (NULL: pink_in is unit-peak)
    unsigned seed; unsigned long long first;   // global index of window 0 of this launch
    int L, ysz, K; float sr;
    float lo[4], hi[4];                     // knob ranges (Effect.knob_ranges, audio.py:493-510)
    int augment;
    float* gc; float* kw;                   // optional scratch [B][L] + [B][4]: the generator leaves the gain curve (ST_FX_COMP: the dB signal) and the world-coordinate knobs there and
                                            // stm::comp_smooth_apply_kernel finishes the effect (lane per window); NULL: the effect runs inside this kernel
                                            // (ST_FX_DECOMP4C: comp_smooth_kernel, then comp_apply_inplace_kernel over the whole of x)
    int chooser;                            // -1: drawn per window from `families`; else forced (tests); 100 = the bare 1/f noise (tests)
    unsigned families;                      // bit f allows family f (synth_feed_kernel<FX, true>; the <FX, false> kernel draws from {0, 1, 2, 4, 6, 7})
};
constexpr int FFT_MAX = 8192;

// in-place inverse FFT (radix-2, decimation in time; the caller stored the spectrum bit-reversed), N a power of two <= FFT_MAX
__device__ __forceinline__ void ifft_lds(float2* a, const int N, const int logN)
{
    for (int s = 1; s <= logN; ++s) {
        const int half = 1 << (s - 1);
        for (int j = threadIdx.x; j < N / 2; j += 256) {
            const int grp = j >> (s - 1), pos = j & (half - 1);
            const int i0 = (grp << s) + pos, i1 = i0 + half;
            float sn, cs; __sincosf(6.28318530717958648f * (float)pos / (float)(2 * half), &sn, &cs);
            const float2 u = a[i0], v = a[i1];
            const float2 t = make_float2(v.x * cs - v.y * sn, v.x * sn + v.y * cs);
            a[i0] = make_float2(u.x + t.x, u.y + t.y);
            a[i1] = make_float2(u.x - t.x, u.y - t.y);
        }
        __syncthreads();
    }
}
__device__ __forceinline__ float block_max(float v, float* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return m;
}

// ---- 1/f noise of LONG windows (L = 2^m > FFT_MAX, e.g. the 65536-sample window of BASELINE configs[4]): the same inverse FFT of the real spectrum
// (2u - 1) / sqrt(k + 1) (audio.py:85-94), as a four-step transform N = N1 * N2 (N1 = 256) through a global scratch -- two launches, no FFT library:
//   y[N2 n1 + n2] = sum_k1 e^{2 pi i k1 n1 / N1} ( e^{2 pi i k1 n2 / N} sum_k2 X[k1 + N1 k2] e^{2 pi i k2 n2 / N2} )
//   pass 1  (k1 fixed, eight k1 per workgroup): the spectrum values are GENERATED (counter-based, stream 7 of the window's key -- the same law and the
//           same per-window reproducibility as the in-LDS transform of the short windows), N2-point transform over k2 in LDS, twiddle, -> scr[n2][k1];
//   pass 2  (n2 fixed, eight n2 per workgroup): 256-point transform over k1 of a contiguous 2 KB row, real part -> pink[N2 n1 + n2], |.| peak -> peak[b]
//           (atomicMax on the bits of a non-negative float); the generator kernel divides by the peak when it mixes the noise in.
// Only windows whose family uses the noise (chooser 1, 7 and -- of a wider family set -- 3, 10, 11; 100 in tests) do any work: a third of the compressor's stream.  Round 3 took this noise from
// torch.fft (rocFFT) driven by a stateful torch.Generator: 2 ms of full-width GPU time per 2048 windows and not reproducible per window index.
constexpr int PL_N1 = 256, PL_G = 16;      // 16 transforms per workgroup: 128-byte segments in pass 1's transposed store, 64-byte ones in pass 2's
__device__ __forceinline__ int feed_family(Draw& d, const int chooser, const unsigned families = FAMILIES_COMPRESSOR)
{
    const int ci = d.randint(0, 6);                                     // drawn whatever the set is: the first sequence does not move
    if (chooser >= 0) return chooser;
    if (families == FAMILIES_COMPRESSOR) return ci < 3 ? ci : (ci == 3 ? 4 : (ci == 4 ? 6 : 7));
    unsigned m = families;                                              // draw 1 of the second sequence: a uniform member of the set, ascending
    for (int i = below(h2(feed_key2(d.key), 1u), __popc(families)); i > 0; --i) m &= m - 1u;
    return __ffs(m) - 1;
}
__device__ __forceinline__ unsigned feed_key(const unsigned seed, const unsigned long long w)
{
    return mix32(seed ^ mix32((unsigned)w + 1u) ^ mix32((unsigned)(w >> 32) + 0x51ED27u));
}
// st_denoise_input: x_noisy [B][L] = denoise_add of x [B][L] (may be the same buffer: each sample is read and written by one thread)
__global__ void __launch_bounds__(256)
denoise_input_kernel(const unsigned seed, const unsigned long long first, const float* x, const float* __restrict__ knobs_wc, const int L, float* x_noisy)
{
    const int b = blockIdx.x;
    const unsigned key = feed_key(seed, first + (unsigned long long)b);
    const float sgth = knobs_wc[b];
    for (int n4 = blockIdx.y * 256 + threadIdx.x; n4 < L / 4; n4 += gridDim.y * 256) {
        const size_t o = (size_t)b * L + 4 * (size_t)n4;
        const unsigned n = 4u * (unsigned)n4;
        *reinterpret_cast<float4*>(x_noisy + o) = denoise_add4(key, n, sgth, *reinterpret_cast<const float4*>(x + o));
    }
}
// G independent in-place inverse FFTs of length n = 2^logn in LDS (a[g * n + i], input stored bit-reversed), 256 threads; tw[k] = e^{2 pi i k / n}, k < n / 2
__device__ __forceinline__ void ifft_batch_lds(float2* a, const float2* tw, const int n, const int logn, const int G)
{
    const int half_total = G * (n >> 1);
    for (int s = 1; s <= logn; ++s) {
        const int half = 1 << (s - 1), tstep = n >> s;
        for (int j = threadIdx.x; j < half_total; j += 256) {
            const int g = j / (n >> 1), jj = j - g * (n >> 1);
            const int grp = jj >> (s - 1), pos = jj & (half - 1);
            const int i0 = g * n + (grp << s) + pos, i1 = i0 + half;
            const float2 w = tw[pos * tstep];
            const float2 u = a[i0], v = a[i1];
            const float2 t = make_float2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x);
            a[i0] = make_float2(u.x + t.x, u.y + t.y);
            a[i1] = make_float2(u.x - t.x, u.y - t.y);
        }
        __syncthreads();
    }
}
__device__ __forceinline__ void twiddle_table(float2* tw, const int n)
{
    for (int k = threadIdx.x; k < n / 2; k += 256) { float sn, cs; sincospif(2.0f * (float)k / (float)n, &sn, &cs); tw[k] = make_float2(cs, sn); }
}
__global__ void __launch_bounds__(256)
pink_long_pass1_kernel(const unsigned seed, const unsigned long long first, const int L, const int chooser, const unsigned families,
                       float2* __restrict__ scr, float* __restrict__ peak)
{
    __shared__ float2 lds[PL_G * 256];
    __shared__ float2 tw[128];
    const int b = blockIdx.y, N2 = L / PL_N1;
    const unsigned long long w = first + (unsigned long long)b;
    Draw d{feed_key(seed, w), 0u};
    const unsigned key = d.key;
    const int ch = feed_family(d, chooser, families);
    if (!family_wants_pink(ch)) return;                                 // workgroup-uniform
    if (blockIdx.x == 0 && threadIdx.x == 0) peak[b] = 0.f;
    int logn = 0; while ((1 << logn) < N2) ++logn;
    twiddle_table(tw, N2);
    const int k1_0 = blockIdx.x * PL_G;
    for (int j = threadIdx.x; j < PL_G * N2; j += 256) {
        const int g = j / N2, k2 = j - g * N2;
        const int k = k1_0 + g + PL_N1 * k2;
        const int kk = k <= L / 2 ? k : L - k;                           // Hermitian extension of a real spectrum
        const float v = (2.f * su01(key, 7u, (unsigned)kk) - 1.f) * rsqrtf((float)kk + 1.f);
        lds[g * N2 + (int)(__brev((unsigned)k2) >> (32 - logn))] = make_float2(v, 0.f);
    }
    __syncthreads();
    ifft_batch_lds(lds, tw, N2, logn, PL_G);
    float2* out = scr + (size_t)b * L;
    for (int j = threadIdx.x; j < PL_G * N2; j += 256) {
        const int n2 = j / PL_G, g = j - n2 * PL_G, k1 = k1_0 + g;
        float sn, cs; sincospif(2.0f * (float)(k1 * n2) / (float)L, &sn, &cs);      // k1 n2 < 2^24: exact in float
        const float2 v = lds[g * N2 + n2];
        out[(size_t)n2 * PL_N1 + k1] = make_float2(v.x * cs - v.y * sn, v.x * sn + v.y * cs);
    }
}
__global__ void __launch_bounds__(256)
pink_long_pass2_kernel(const unsigned seed, const unsigned long long first, const int L, const int chooser, const unsigned families, const float2* __restrict__ scr,
                       float* __restrict__ pink, float* __restrict__ peak)
{
    __shared__ float2 lds[PL_G * PL_N1];
    __shared__ float2 tw[PL_N1 / 2];
    __shared__ float red[4];
    const int b = blockIdx.y, N2 = L / PL_N1;
    const unsigned long long w = first + (unsigned long long)b;
    Draw d{feed_key(seed, w), 0u};
    const int ch = feed_family(d, chooser, families);
    if (!family_wants_pink(ch)) return;
    twiddle_table(tw, PL_N1);
    const int n2_0 = blockIdx.x * PL_G;
    const float2* in = scr + (size_t)b * L + (size_t)n2_0 * PL_N1;
    for (int j = threadIdx.x; j < PL_G * PL_N1; j += 256) {
        const int g = j >> 8, k1 = j & 255;
        lds[g * PL_N1 + (int)(__brev((unsigned)k1) >> 24)] = in[j];
    }
    __syncthreads();
    ifft_batch_lds(lds, tw, PL_N1, 8, PL_G);
    float m = 0.f;
    float* o = pink + (size_t)b * L;
    for (int j = threadIdx.x; j < PL_G * PL_N1; j += 256) {
        const int n1 = j / PL_G, g = j - n1 * PL_G;
        const float v = lds[g * PL_N1 + n1].x;
        o[(size_t)N2 * n1 + n2_0 + g] = v;
        m = fmaxf(m, fabsf(v));
    }
    m = block_max(m, red);
    if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned*>(peak + b), __float_as_uint(m));
}

// the effect a feed launch applies (include/signaltrain_hip.h ST_FX_*): a template parameter, so the comp_4c instantiation is the kernel it always was.
// EXT: the families beyond the compressor's set and the family set of a.families (the second draw sequence); false = the kernel it always was.
template <int FX, bool EXT>
__global__ void __launch_bounds__(256)
synth_feed_kernel(const FeedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float feed_lds[];      // float2[FFT_MAX] (pink) -- later float[COMP_CH] (compressor)
    __shared__ float red[4];
    __shared__ float carry;
    __shared__ int sp_loc[EXT ? N_SPIKES : 1];                            // family 5: the spikes' positions and heights
    __shared__ float sp_h[EXT ? N_SPIKES : 1];
    __shared__ unsigned sp_map[EXT ? SPIKE_MAP_BITS / 32 : 1];            // bit (n mod 65536): some spike touches sample n -- 150 of the window's samples look further
    __shared__ double env_tab[EXT ? 32 : 1];                              // family 8: 10^(dB / 10), dB = -30 .. 0
    const int b = blockIdx.x, L = a.L;
    const unsigned long long w = a.first + (unsigned long long)b;
    Draw d{feed_key(a.seed, w), 0u};
    const unsigned key = d.key;
    const float dt = 1.0f / a.sr, tl = (float)(L - 1) * dt;

    // ---- the window's parameters (datasets.py:317, audio.py:296-334)
    const int ch = EXT ? feed_family(d, a.chooser, a.families) : feed_family(d, a.chooser);      // {0, 1, 2, 4, 6, 7} unless EXT
    float kn[4], kw[4];
    feed_knobs<FX>(d, a.lo, a.hi, a.K, kn, kw);                      // the next draws of the first sequence (the knob rule: feed_knobs)
    // randsine (audio.py:96-104)
    const int s_n = d.randint(1, 3);
    float s_amp[2], s_frq[2], s_t0[2];
    for (int i = 0; i < 2; ++i) { s_amp[i] = i < s_n ? 0.2f + 0.7f * d.u() : 0.f; s_frq[i] = 5.f + 145.f * d.u(); s_t0[i] = d.u() * tl; }
    // pluck (audio.py:138-148) and its decay envelope (audio.py:126-136)
    const int p_n = d.randint(1, 4);
    float p_amp[3], p_frq[3], p_t0[3];
    for (int i = 0; i < 3; ++i) { const float am = (0.45f * d.u() + 0.5f) * d.sign(); p_amp[i] = i < p_n ? am : 0.f; p_t0[i] = (2.f * d.u() - 1.f) * 0.3f * tl; p_frq[i] = 50.f + 6350.f * d.u(); }
    const float e_t0 = 0.35f * d.u() * tl, e_hi = 0.35f * d.u() + 0.6f, e_lo = 0.1f * d.u() + 0.1f, e_dec = 12.f * d.u();
    // box (audio.py:106-124)
    const float b_h0 = 0.15f * d.u(), b_h1 = 0.35f * d.u() + 0.6f, b_h2 = 0.2f * d.u() + 0.1f;
    const int b_up = (int)(0.3f * d.u() * (float)L);
    int b_dn = b_up + (int)((0.3f + 0.35f * d.u()) * (float)L); if (b_dn > L - 1) b_dn = L - 1;
    const float nrm_u = 0.6f + 0.3f * d.u();                       // normish: U(0.6, 0.9) / peak
    const float c_pink1 = 0.2f * d.u(), c_white1 = 0.2f * d.u(), c_pink7 = 0.3f * d.u() + 0.1f;
    float pol = d.sign();
    if (a.augment) pol *= d.sign();                                  // datasets.py:27-29: the effect is odd in x, so flipping the pair == flipping x first
    const bool want_pink = EXT ? family_wants_pink(ch) : (ch == 1 || ch == 7 || ch == 100);
    // ---- the families beyond the compressor's set: parameters from the second sequence, values in float64 where float32 would not carry the phase
    // (the sweep reaches 2.7e4 rad at the 65536-sample window, the step tone 7e3 rad: an ulp of a float32 phase is 2e-3 rad there)
    ExtDraws e = {};
    double sw_c = 0.0, sw_r = 0.0;
    if (EXT) {
        const unsigned key2 = feed_key2(key);
        e = ext_draws(key2, L, a.sr);
        const double lnfr = log((double)e.sw_fhi / (double)e.sw_flo), tmax = fmax((double)e.tl, 1e-30);
        sw_c = 20.0 * 2.0 * 3.14159265358979323846 * tmax / lnfr; sw_r = lnfr / tmax;
        if (ch == 5) {                                               // workgroup-uniform
            for (int i = threadIdx.x; i < SPIKE_MAP_BITS / 32; i += 256) sp_map[i] = 0u;
            __syncthreads();
            if (threadIdx.x < N_SPIKES) {
                ext_spike(key2, (int)threadIdx.x, L, e.tl, &sp_loc[threadIdx.x], &sp_h[threadIdx.x]);
                for (int dl = -1; dl <= 1; ++dl) {
                    const unsigned m = (unsigned)((sp_loc[threadIdx.x] + dl + L) % L) & (unsigned)(SPIKE_MAP_BITS - 1);
                    atomicOr(&sp_map[m >> 5], 1u << (m & 31u));
                }
            }
            __syncthreads();
        }
        if (ch == 8) {
            if (threadIdx.x <= 30) env_tab[threadIdx.x] = exp(0.1 * 2.30258509299404568402 * (double)((int)threadIdx.x - 30));
            __syncthreads();
        }
    }
    const int Lm1 = L > 1 ? L - 1 : 1;
    auto tq = [&](const int n) { return (float)n / a.sr; };          // the reference's float32 time value, correctly rounded
    auto stepv = [&](const int n) {                                  // ampexpstepup (audio.py:149-161) before normish
        const int up = L <= (1 << 26) ? (int)((30u * (unsigned)n) / (unsigned)Lm1) : (int)((30ll * (long long)n) / (long long)Lm1);      // 0 .. 30
        return (float)(env_tab[up] * sin((double)e.st_frq * (double)tq(n)));
    };
    auto sweepv = [&](const int n) {                                 // sweep (audio.py:164-173) before normish
        const double g = exp(sw_r * (double)tq(n));
        const double y = (double)e.sw_amp * sin(sw_c * (g - 1.0));
        return (float)(e.sw_too ? y * g : y);
    };
    auto triv = [&](const int n) {                                   // triangle (audio.py:188-194) without its noise
        const float t = tq(n);
        return (t < e.tri_t0 - e.tri_w || t > e.tri_t0 + e.tri_w) ? 0.f : e.tri_h * (1.f - fabsf(t - e.tri_t0) / fmaxf(e.tri_w, 1e-30f));
    };
    auto spikev = [&](const int n) {                                 // spikes (audio.py:175-186): the last spike that touches the sample wins
        float v = 0.f;
        const unsigned m = (unsigned)n & (unsigned)(SPIKE_MAP_BITS - 1);
        if ((sp_map[m >> 5] >> (m & 31u)) & 1u) for (int j = N_SPIKES - 1; j >= 0; --j) {
            const int dl = n - sp_loc[j];
            if (dl == 0) { v = sp_h[j]; break; }
            if (dl == 1 || dl == -1 || dl == L - 1 || dl == 1 - L) { v = 0.5f * sp_h[j]; break; }
        }
        const float z = sqrtf(-2.f * logf(1.f - su01(key, 13u, (unsigned)n))) * cospif(2.f * su01(key, 17u, (unsigned)n));
        return v + e.sp_amp * z;
    };

    // ---- 1/f noise (audio.py:85-94)
    float2* fa = reinterpret_cast<float2*>(feed_lds);
    float pink_peak = 1.f;
    if (want_pink && !a.pink_in) {                                   // workgroup-uniform
        int logN = 0; while ((1 << logN) < L) ++logN;
        for (int k = threadIdx.x; k < L; k += 256) {
            const int kk = k <= L / 2 ? k : L - k;                   // Hermitian extension of a real spectrum: X[N - k] = X[k]
            const float v = (2.f * su01(key, 7u, (unsigned)kk) - 1.f) * rsqrtf((float)kk + 1.f);
            fa[__brev((unsigned)k) >> (32 - logN)] = make_float2(v, 0.f);
        }
        __syncthreads();
        ifft_lds(fa, L, logN);
        float m = 0.f;
        for (int n = threadIdx.x; n < L; n += 256) m = fmaxf(m, fabsf(fa[n].x));
        pink_peak = fmaxf(block_max(m, red), 1e-30f);
    }
    if (a.pink_in && a.pink_peak) pink_peak = fmaxf(a.pink_peak[b], 1e-30f);
    auto sine = [&](const float t) { return s_amp[0] * __cosf(s_frq[0] * (t - s_t0[0])) + s_amp[1] * __cosf(s_frq[1] * (t - s_t0[1])); };
    auto plk = [&](const float t) {
        const float env = t < e_t0 ? e_lo : __expf(-e_dec * (t - e_t0)) * e_hi;
        return (p_amp[0] * __sinf(p_frq[0] * (t - p_t0[0])) + p_amp[1] * __sinf(p_frq[1] * (t - p_t0[1])) + p_amp[2] * __sinf(p_frq[2] * (t - p_t0[2]))) * env;
    };
    auto boxv = [&](const int n) { return n < b_up - 1 ? b_h0 : ((n >= b_up && n < b_dn) ? b_h1 : b_h2); };

    // ---- pass 1: the peak normish divides by (families built on randsine / pluck)
    float scale = 1.f;
    if (ch == 0 || ch == 1 || ch == 2 || ch == 7) {
        float m = 0.f;
        for (int n = threadIdx.x; n < L; n += 256) { const float t = (float)n * dt; m = fmaxf(m, fabsf((ch == 0 || ch == 1) ? sine(t) : plk(t))); }
        scale = nrm_u / fmaxf(block_max(m, red), 1e-30f);
    }
    if (EXT && (ch == 8 || ch == 9)) {
        float m = 0.f;
        for (int n = threadIdx.x; n < L; n += 256) m = fmaxf(m, fabsf(ch == 8 ? stepv(n) : sweepv(n)));
        scale = nrm_u / fmaxf(block_max(m, red), 1e-30f);
    }
    // ---- pass 2: the window -- four consecutive samples per thread and trip (16-byte loads of the long-window noise, 16-byte stores), and with the
    // lane-per-window form of the effect the static gain curve of each sample right away, from the value in registers.  (Round 3 wrote the window and
    // then re-read it sample by sample in a third loop: without __restrict__ every trip's load waited for the previous trip's store -- 256 dependent
    // memory round trips per thread at the 65536-sample window, most of the generator's 300 us per window.)
    float* __restrict__ xb = a.x + (size_t)b * L;
    float* __restrict__ gcb = a.gc ? a.gc + (size_t)b * L : nullptr;
    const float* __restrict__ pin = a.pink_in ? a.pink_in + (size_t)b * L : nullptr;
    const float inv_peak = 1.0f / pink_peak;
    auto sample = [&](const int n, const float pk) {
        const float t = (float)n * dt;
        float v;
        if (ch == 0) v = sine(t) * scale;
        else if (ch == 1) v = sine(t) * scale + c_pink1 * pk + c_white1 * (2.f * su01(key, 3u, (unsigned)n) - 1.f);
        else if (ch == 2) v = plk(t) * scale;
        else if (ch == 4) v = boxv(n);
        else if (ch == 6) v = boxv(n) * (2.f * su01(key, 3u, (unsigned)n) - 1.f);
        else if (ch == 100) v = pk;
        else if (EXT && ch == 3) v = triv(n) + e.tri_amp * pk;
        else if (EXT && ch == 5) v = spikev(n);
        else if (EXT && ch == 8) v = stepv(n) * scale;
        else if (EXT && ch == 9) v = sweepv(n) * scale;
        else if (EXT && ch == 10) v = boxv(n) + e.c_white10 * (2.f * su01(key, 3u, (unsigned)n) - 1.f) + e.c_pink10 * pk;
        else if (EXT && ch == 11) v = e.c_pink11 * pk;
        else v = plk(t) * scale + c_pink7 * pk;
        return ch == 100 ? v : v * pol + su01(key, 5u, (unsigned)n) * 1e-8f;       // audio.py:333
    };
    if ((L & 3) == 0) {
        for (int n4 = threadIdx.x; n4 < L / 4; n4 += 256) {
            const int n = 4 * n4;
            float4 pk = make_float4(0.f, 0.f, 0.f, 0.f);
            if (want_pink) {
                if (pin) { pk = *reinterpret_cast<const float4*>(pin + n); if (a.pink_peak) { pk.x *= inv_peak; pk.y *= inv_peak; pk.z *= inv_peak; pk.w *= inv_peak; } }
                else pk = make_float4(fa[n].x * inv_peak, fa[n + 1].x * inv_peak, fa[n + 2].x * inv_peak, fa[n + 3].x * inv_peak);
            }
            float4 v = make_float4(sample(n, pk.x), sample(n + 1, pk.y), sample(n + 2, pk.z), sample(n + 3, pk.w));
            if (FX == ST_FX_DENOISE || FX == ST_FX_DECOMP4C) {       // the target is the clean tail ...
                float* __restrict__ yb = a.y + (size_t)b * a.ysz;
                const int j = n - (L - a.ysz);
                if (j >= 0) yb[j] = v.x;
                if (j + 1 >= 0) yb[j + 1] = v.y;
                if (j + 2 >= 0) yb[j + 2] = v.z;
                if (j + 3 >= 0) yb[j + 3] = v.w;
            }
            if (FX == ST_FX_DENOISE) v = denoise_add4(key, (unsigned)n, kw[0], v);      // ... and the input leaves with the noise on it
            *reinterpret_cast<float4*>(xb + n) = v;
            if (gcb) *reinterpret_cast<float4*>(gcb + n) = FX == ST_FX_COMP ? env_db4(v) : comp_gain_curve4(v, kw[0], kw[1]);
        }
    } else {
        for (int n = threadIdx.x; n < L; n += 256) {
            const float pk = want_pink ? (pin ? (a.pink_peak ? pin[n] * inv_peak : pin[n]) : fa[n].x * inv_peak) : 0.f;
            float v = sample(n, pk);
            if ((FX == ST_FX_DENOISE || FX == ST_FX_DECOMP4C) && n >= L - a.ysz) a.y[(size_t)b * a.ysz + n - (L - a.ysz)] = v;
            if (FX == ST_FX_DENOISE) v = denoise_add(key, (unsigned)n, kw[0], v);
            xb[n] = v;
            if (gcb) gcb[n] = FX == ST_FX_COMP ? stm::env_db(v) : stm::comp_gain_curve(v, (double)kw[0], (double)kw[1]);
        }
    }
    if (threadIdx.x == 0) { for (int k = 0; k < 4; ++k) if (k < a.K) a.knobs[(size_t)b * a.K + k] = kn[k]; }
    if (FX == ST_FX_DENOISE) return;
    if (a.gc) {                                                      // workgroup-uniform: the effect finishes in the next launches (comp_smooth_kernel +
        if (threadIdx.x == 0) { for (int k = 0; k < 4; ++k) a.kw[(size_t)b * 4 + k] = kw[k]; }      // comp_apply_kernel, or compressor_env_kernel)
        return;
    }
    __threadfence_block();
    __syncthreads();                                                 // the window is complete (and the FFT buffer is dead)
    if (FX == ST_FX_LOWPASS) {                                       // the Butterworth low-pass (audio.py:610-625), a scan over the filter's modes
        stm::lowpass_window(xb, a.y + (size_t)b * a.ysz, stm::lowpass_coef((double)kw[0], (double)a.sr), L, a.ysz, reinterpret_cast<stm::LpLds*>(feed_lds));
        return;
    }
    if (FX == ST_FX_ECHO) {                                          // the echo (audio.py:430-443): reads of the finished window, no recurrence
        stm::echo_window(xb, a.y + (size_t)b * a.ysz, kw[0], kw[1], kw[2], L, a.ysz, 0, 256, reinterpret_cast<stm::EchoLds*>(feed_lds));
        return;
    }
    if (FX == ST_FX_COMP) {                                          // the envelope compressor (audio.py:349-371), a scan over the window
        stm::env_compressor_window(xb, nullptr, a.y + (size_t)b * a.ysz, (double)kw[0], (double)kw[1], stm::env_coef((double)kw[2], (double)a.sr),
                                   L, a.ysz, reinterpret_cast<stm::EnvLds*>(feed_lds));
        return;
    }
    // ---- the effect (audio.py:380-426) on the finished window, inside this workgroup
    const double alphaA = exp(-log(9.0) / ((double)a.sr * (double)kw[2])), alphaR = exp(-log(9.0) / ((double)a.sr * (double)kw[3]));
    if (FX == ST_FX_DECOMP4C) {                                      // the compressed window is the item's input (audio.py:573-583): over the whole of x, in place
        stm::compressor_window_inplace(xb, (double)kw[0], (double)kw[1], alphaA, alphaR, L, feed_lds, &carry);
        return;
    }
    stm::compressor_window(xb, a.y + (size_t)b * a.ysz, (double)kw[0], (double)kw[1], alphaA, alphaR, L, a.ysz, feed_lds, &carry);
}

}  // namespace stf
