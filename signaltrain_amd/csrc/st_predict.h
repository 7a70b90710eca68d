// st_predict.h -- the two HBM streamers of st_predict_long (gfx950): whole-signal inference without a window copy.
//
// Reference: utils/predict_long.py:30-79 windows the recording on the host (audio.sliding_window, audio.py:23-49: overlap L - y, zeros behind the end),
// ships every batch of overlapping windows to the device and appends the y-sample outputs.  Here the recording stays where it is: window w IS
// signal[w y .. w y + L), so a batch of windows is a set of rows of pitch y inside the signal, and output sample i = w y + j (window i / y, position i % y)
// belongs to input sample (L - y) + i.  Neither the windows nor the concatenated output exist as copies.
//
//   predict_stage_kernel   what prep_kernel's per-batch part does for a batch that lies in [B][L] rows, read from the signal instead: x/2 (nn_proc.py:307) with
//                          the Conv1d padding materialised (cls_fe_dft.py:28-31) as fp32 or as the 16-bit GEMM operand, zeros past sample n, the exact zeros
//                          of the all-padding frames, and -- one knob setting for the whole signal -- that setting repeated over the batch's knob rows.
//   predict_ola_kernel     overlap-add + crop (cls_fe_dft.py:112-113), residual and x2 (nn_proc.py:332,340) of ola_loss4_kernel / ola_loss_kernel without loss,
//                          partials or d syn: the residual comes from the signal itself and the result goes straight to its place in the output, clipped to n_out.
//
// Addresses.  y % 4 == 0, L % 4 == 0, N % 32 == 0, H % 4 == 0 (check_dims) and the signal / output bases are 16-byte aligned (int16: 8-byte; the entry refuses
// anything else), so every quad of four samples is ONE aligned 16-byte (int16: 8-byte) access.  A quad is read whole only where all four samples lie below n;
// the one quad that straddles n is read sample by sample and nothing at or past n is ever addressed, whatever lies there.  Output quads are clipped the same way
// at n_out.  Sample offsets are 64-bit (a recording may be longer than 2^31 samples); offsets inside a batch's workspace rows stay within check_dims' 2^30 elements.
// ST_PCM_S16 converts as the feeds do (st_feed_files.h): (float)s / 32767.0f, the same float as (float)((double)s / 32767.0) for every int16 s.
#pragma once
#include "st_common.h"
#include "st_misc.h"

namespace stp {

__device__ __forceinline__ float pcm_one(const float* p) { return *p; }
__device__ __forceinline__ float pcm_one(const short* p) { return (float)*p / 32767.0f; }
__device__ __forceinline__ float4 pcm_quad(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 pcm_quad(const short* p)
{
    const short4 v = *reinterpret_cast<const short4*>(p);
    return make_float4((float)v.x / 32767.0f, (float)v.y / 32767.0f, (float)v.z / 32767.0f, (float)v.w / 32767.0f);
}
// samples [g, g + 4) of the signal, zero from sample n on (g % 4 == 0, g >= 0)
template <typename T>
__device__ __forceinline__ float4 pcm_quad_upto(const T* __restrict__ sig, const long long g, const long long n)
{
    if (g + 4 <= n) return pcm_quad(sig + g);
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = g + q < n ? pcm_one(sig + g + q) : 0.f;
    return make_float4(v[0], v[1], v[2], v[3]);
}

struct StageArgs {
    const void* signal; long long n, s0;      // s0: first sample of the batch's first window (= its first output sample: first window * y)
    int y, L, pad, nb;                        // row pitch inside the signal, window length, Conv1d padding (= N), windows of this batch
    float* xp; unsigned short* xp16; int ht;  // ht != 0: the padded rows go out as the 16-bit GEMM operand INSTEAD of fp32 (as prep_kernel writes them)
    int nbx, n_pad;                           // blocks per window, blocks of the padded copy
    float *mag, *phs; int T, F, t_lo, Tv, n_dead;      // all-padding frames: mag = 0, phs = atan2(0, 1e-7) = 0
    const float* knob_row; float* knobs; int K, n_kn;  // n_kn > 0: knobs[b][k] = knob_row[k] for the nb rows of the batch
};
// Block ranges: [0, n_pad) the padded half-scaled rows, element for element pad_scale_block's arithmetic (zero margins, v * 0.5f, rounded once where ht);
// [n_pad, n_pad + n_dead) the all-padding frames; the rest the knob rows.  One quad per lane and trip, its load issued before its store; 16-byte stores (8-byte: 16-bit).
template <typename T>
__global__ void __launch_bounds__(256)
predict_stage_kernel(const StageArgs a)
{
    const int blk = blockIdx.x;
    if (blk < a.n_pad) {
        const int b = blk / a.nbx, bx = blk - b * a.nbx;
        const T* __restrict__ sig = reinterpret_cast<const T*>(a.signal);
        const long long w0 = a.s0 + (long long)b * a.y;
        const int Lp4 = (a.L + 2 * a.pad) / 4;
        float4* dst = reinterpret_cast<float4*>(a.xp + (size_t)b * (a.L + 2 * a.pad));
        uint2* dst16 = reinterpret_cast<uint2*>(a.xp16 + (size_t)b * (a.L + 2 * a.pad));
        for (int i = bx * 256 + threadIdx.x; i < Lp4; i += a.nbx * 256) {
            const int j = i - a.pad / 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j >= 0 && j < a.L / 4) {
                const long long g = w0 + 4ll * j;
                if (g < a.n) { v = pcm_quad_upto(sig, g, a.n); v.x *= 0.5f; v.y *= 0.5f; v.z *= 0.5f; v.w *= 0.5f; }
            }
            if (a.ht) dst16[i] = st_to_h16x4(v, a.ht);
            else dst[i] = v;
        }
    }
    else if (blk < a.n_pad + a.n_dead) stm::zero_dead_frame(nullptr, nullptr, a.mag, a.phs, a.T, a.F, a.t_lo, a.Tv, blk - a.n_pad);
    else {
        const int i = (blk - a.n_pad - a.n_dead) * 256 + (int)threadIdx.x;
        if (i < a.nb * a.K) a.knobs[i] = a.knob_row[i % a.K];
    }
}

// Four output samples per lane, grid (ceil(y / 4 / 256), windows of the batch).  Per sample the frames are summed in the order of ola_loss_kernel / ola_loss4_kernel
// (frames outer, slabs inner, from 0.f), then 2 * (s + x / 2) with x the residual sample of the signal.
//   NF = 3: ceil(N / H) <= 3 -- at most three frames meet a sample: all 3 x NS 16-byte loads are issued before the first add, a frame past the last live one
//           re-reads the last live one (valid address, value dropped), exactly as ola_loss4_kernel does;
//   NF = 0: any overlap (ceil(N / H) = 4 at N = 1024, H = 256; the geometries ola_loss_kernel serves): a loop over the live frames, NS loads in flight per trip.
// H % 4 == 0 makes the frame set the same for the four samples of a quad and every tap offset N + j - H t a multiple of four.
template <typename T, int NS, int NF>
__global__ void __launch_bounds__(256)
predict_ola_kernel(const float* __restrict__ frs, const size_t slab, const T* __restrict__ sig, float* __restrict__ out,
                   const long long s0, const long long n_out, const int L, const int N, const int H, const int OT, const int ysz)
{
    const int b = blockIdx.y;
    const int j = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (j >= ysz) return;
    const long long i = s0 + (long long)b * ysz + j;      // output sample; its input sample is (L - ysz) + i < n wherever i < n_out
    if (i >= n_out) return;
    const int t0 = j / H + 1;                             // first frame with N + j - H t < N
    int t1 = (N + j) / H;                                 // last frame with N + j - H t >= 0
    if (t1 > OT - 1) t1 = OT - 1;
    const float* fb = frs + (size_t)b * OT * N;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    float4 xv;
    if constexpr (NF > 0) {
        float4 v[NF][NS];
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            const int t = t0 + u <= t1 ? t0 + u : t1;
            const size_t o = (size_t)t * N + (size_t)(N + j - H * t);
#pragma unroll
            for (int z = 0; z < NS; ++z) v[u][z] = *reinterpret_cast<const float4*>(fb + z * slab + o);
        }
        xv = pcm_quad_upto(sig, i + (L - ysz), n_out + (L - ysz));
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            const bool live = t0 + u <= t1;
#pragma unroll
            for (int z = 0; z < NS; ++z) {
                s[0] += live ? v[u][z].x : 0.f; s[1] += live ? v[u][z].y : 0.f; s[2] += live ? v[u][z].z : 0.f; s[3] += live ? v[u][z].w : 0.f;
            }
        }
    } else {
        xv = pcm_quad_upto(sig, i + (L - ysz), n_out + (L - ysz));
        for (int t = t0; t <= t1; ++t) {
            const size_t o = (size_t)t * N + (size_t)(N + j - H * t);
            float4 v[NS];
#pragma unroll
            for (int z = 0; z < NS; ++z) v[z] = *reinterpret_cast<const float4*>(fb + z * slab + o);
#pragma unroll
            for (int z = 0; z < NS; ++z) { s[0] += v[z].x; s[1] += v[z].y; s[2] += v[z].z; s[3] += v[z].w; }
        }
    }
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
    float r[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = 2.0f * (s[q] + 0.5f * xs[q]);
    if (i + 4 <= n_out) *reinterpret_cast<float4*>(out + i) = make_float4(r[0], r[1], r[2], r[3]);
    else {
#pragma unroll
        for (int q = 0; q < 4; ++q) if (i + q < n_out) out[i + q] = r[q];
    }
}

}  // namespace stp
