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
//
// Shared with the predict session (st_predict_stream.h), st_eval_pool (st_eval_pool.h) and the knob fits (st_fit.h), whose kernels differ from the two above in
// their sample source, their knob-row source and what they do with the sum -- and in nothing else, which is what their bit-for-bit promises rest on:
//   StageCommon / stage_blocks   the staged rows, the dead frames and the knob-row fill of every stage kernel;
//   ola_frame_sum                the overlap-add of a quad's frames (NF = 3 and NF = 0) of every overlap-add kernel;
//   ola_out / ola_out4, store_quad_upto, logcosh_term   the residual term, the clipped quad store and the loss term.
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

// What every stage kernel of this family is told about the batch (the stream's and the pool's StageArgs embed it too): only the sample source and the
// knob-row source are the kernel's own.
struct StageCommon {
    int y, L, pad, nb;                        // row pitch inside the signal, window length, Conv1d padding (= N), rows of this batch
    float* xp; unsigned short* xp16; int ht;  // ht != 0: the padded rows go out as the 16-bit GEMM operand INSTEAD of fp32 (as prep_kernel writes them)
    int nbx, n_pad;                           // blocks per row, blocks of the padded copy
    float *mag, *phs; int T, F, t_lo, Tv, n_dead;      // all-padding frames: mag = 0, phs = atan2(0, 1e-7) = 0
    float* knobs; int K, n_kn;                // n_kn > 0: knobs[b][k] = (row b's source row)[k] for the nb rows of the batch
};
// Block ranges: [0, n_pad) the padded half-scaled rows, element for element pad_scale_block's arithmetic (zero margins, v * 0.5f, rounded once where ht);
// [n_pad, n_pad + n_dead) the all-padding frames; [.., + n_kn) the knob rows.  One quad per lane and trip, its load issued before its store; 16-byte stores
// (8-byte: 16-bit).  row_of(b) is called once per block and returns the reader of row b -- reader(g): samples [g, g + 4) of the row's window, g % 4 == 0, zeros
// behind the source's end; knob_row_of(b): row b's source knob row.  false: the block lies behind the three ranges (the pool's side role).
template <typename RowOf, typename KnobRowOf>
__device__ __forceinline__ bool stage_blocks(const StageCommon& a, const int blk, RowOf row_of, KnobRowOf knob_row_of)
{
    if (blk < a.n_pad) {
        const int b = blk / a.nbx, bx = blk - b * a.nbx;
        const auto quad = row_of(b);
        const int Lp4 = (a.L + 2 * a.pad) / 4;
        float4* dst = reinterpret_cast<float4*>(a.xp + (size_t)b * (a.L + 2 * a.pad));
        uint2* dst16 = reinterpret_cast<uint2*>(a.xp16 + (size_t)b * (a.L + 2 * a.pad));
        for (int i = bx * 256 + threadIdx.x; i < Lp4; i += a.nbx * 256) {
            const int j = i - a.pad / 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j >= 0 && j < a.L / 4) { v = quad(4ll * j); v.x *= 0.5f; v.y *= 0.5f; v.z *= 0.5f; v.w *= 0.5f; }
            if (a.ht) dst16[i] = st_to_h16x4(v, a.ht);
            else dst[i] = v;
        }
    }
    else if (blk < a.n_pad + a.n_dead) stm::zero_dead_frame(nullptr, nullptr, a.mag, a.phs, a.T, a.F, a.t_lo, a.Tv, blk - a.n_pad);
    else if (blk < a.n_pad + a.n_dead + a.n_kn) {
        const int i = (blk - a.n_pad - a.n_dead) * 256 + (int)threadIdx.x;
        if (i < a.nb * a.K) a.knobs[i] = knob_row_of(i / a.K)[i % a.K];
    }
    else return false;
    return true;
}

struct StageArgs {
    StageCommon c;
    const void* signal; long long n, s0;      // s0: first sample of the batch's first window (= its first output sample: first window * y)
    const float* knob_row;                    // one knob setting for the whole signal
};
template <typename T>
__global__ void __launch_bounds__(256)
predict_stage_kernel(const StageArgs a)
{
    const T* __restrict__ sig = reinterpret_cast<const T*>(a.signal);
    stage_blocks(a.c, blockIdx.x,
                 [&](const int b) {
                     const long long w0 = a.s0 + (long long)b * a.c.y;
                     return [=, &a](const long long g) { return w0 + g < a.n ? pcm_quad_upto(sig, w0 + g, a.n) : make_float4(0.f, 0.f, 0.f, 0.f); };
                 },
                 [&](const int) { return a.knob_row; });
}

// The overlap-add of four output samples j .. j + 3 of row b's frames, into s (from 0.f): per sample the frames are summed in the order of ola_loss_kernel /
// ola_loss4_kernel (frames outer, slabs inner).  H % 4 == 0 makes the frame set the same for the four samples of a quad and every tap offset N + j - H t a
// multiple of four.
//   NF = 3: ceil(N / H) <= 3 -- at most three frames meet a sample: all 3 x NS 16-byte loads are issued before the first add, a frame past the last live one
//           re-reads the last live one (valid address, value dropped), exactly as ola_loss4_kernel does;
//   NF = 0: any overlap (ceil(N / H) = 4 at N = 1024, H = 256; the geometries ola_loss_kernel serves): a loop over the live frames, NS loads in flight per trip.
// side(): the caller's own loads (residual, target), issued behind the frame loads of the NF = 3 form and before the first add of either form.
template <int NS, int NF, typename Side>
__device__ __forceinline__ void ola_frame_sum(const float* __restrict__ fb, const size_t slab, const int N, const int H, const int OT, const int j, float s[4], Side side)
{
    const int t0 = j / H + 1;                             // first frame with N + j - H t < N
    int t1 = (N + j) / H;                                 // last frame with N + j - H t >= 0
    if (t1 > OT - 1) t1 = OT - 1;
    s[0] = s[1] = s[2] = s[3] = 0.f;
    if constexpr (NF > 0) {
        float4 v[NF][NS];
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            const int t = t0 + u <= t1 ? t0 + u : t1;
            const size_t o = (size_t)t * N + (size_t)(N + j - H * t);
#pragma unroll
            for (int z = 0; z < NS; ++z) v[u][z] = *reinterpret_cast<const float4*>(fb + z * slab + o);
        }
        side();
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            const bool live = t0 + u <= t1;
#pragma unroll
            for (int z = 0; z < NS; ++z) {
                s[0] += live ? v[u][z].x : 0.f; s[1] += live ? v[u][z].y : 0.f; s[2] += live ? v[u][z].z : 0.f; s[3] += live ? v[u][z].w : 0.f;
            }
        }
    } else {
        side();
        for (int t = t0; t <= t1; ++t) {
            const size_t o = (size_t)t * N + (size_t)(N + j - H * t);
            float4 w[NS];
#pragma unroll
            for (int z = 0; z < NS; ++z) w[z] = *reinterpret_cast<const float4*>(fb + z * slab + o);
#pragma unroll
            for (int z = 0; z < NS; ++z) { s[0] += w[z].x; s[1] += w[z].y; s[2] += w[z].z; s[3] += w[z].w; }
        }
    }
}
// residual and x2 (nn_proc.py:332,340): the output sample of overlap-added sample s and input sample x
__device__ __forceinline__ float ola_out(const float s, const float x) { return 2.0f * (s + 0.5f * x); }
__device__ __forceinline__ void ola_out4(const float s[4], const float4 xv, float r[4])
{
    r[0] = ola_out(s[0], xv.x); r[1] = ola_out(s[1], xv.y); r[2] = ola_out(s[2], xv.z); r[3] = ola_out(s[3], xv.w);
}
// the quad r to o[i .. i + 3], o the address of output sample 0: one 16-byte store where the quad ends at or below `end` (and, the pool's case, its address is
// aligned), else sample by sample; nothing at or past o[end] is addressed.  The samples are indexed o[i + q], not (o + i)[q]: from the latter the compiler merges
// the first three clipped stores behind branches of their own, 14 .. 20 instructions more in every predict_ola_kernel instantiation.
__device__ __forceinline__ void store_quad_upto(float* __restrict__ o, const float r[4], const long long i, const long long end, const bool aligned = true)
{
    if (i + 4 <= end && aligned) *reinterpret_cast<float4*>(o + i) = make_float4(r[0], r[1], r[2], r[3]);
    else {
#pragma unroll
        for (int q = 0; q < 4; ++q) if (i + q < end) o[i + q] = r[q];
    }
}
// log cosh e for e = |d| >= 0 as ola_loss4_kernel forms it (st_misc.h): the loss term of st_fit_knobs and of st_eval_pool's statistics
__device__ __forceinline__ float logcosh_term(const float e)
{
    if (e < 8.0f) { const float u = expm1f(0.5f * e); const float sh = 0.5f * (u + u / (u + 1.0f)); return log1pf(2.0f * sh * sh); }
    return e + log1pf(__expf(-2.0f * e)) - 0.69314718056f;
}

// Four output samples per lane, grid (ceil(y / 4 / 256), windows of the batch): ola_frame_sum with the residual from the signal itself, the result straight to its
// place in the output, clipped to n_out.
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
    float s[4], r[4];
    float4 xv;
    ola_frame_sum<NS, NF>(frs + (size_t)b * OT * N, slab, N, H, OT, j, s, [&] { xv = pcm_quad_upto(sig, i + (L - ysz), n_out + (L - ysz)); });
    ola_out4(s, xv, r);
    store_quad_upto(out, r, i, n_out);
}

}  // namespace stp
