// st_predict_stream.h -- the three HBM streamers of a predict session (st_predict_stream_*, gfx950): st_predict_long's forward fed block by block, C channels in lockstep.
//
// The model has no look-ahead: window w reads signal[w y, w y + L) and predicts its last y samples, so output sample i belongs to input sample (L - y) + i and the
// only state between two pushes is the tail of the signal no complete window has consumed yet.  A session keeps that tail per channel in HBM (float32 whatever the
// block format) and a push brings m new samples per channel.  With n0 samples received before the push and n1 = n0 + m after it, the signal a push can see is the pair
//
//     (history | block):   sample g of channel c  =  hist[c][g - a]   for a <= g < n0      (a = first sample held, a % 4 == 0; n0 - a samples held)
//                                                 =  block[c][g - n0] for n0 <= g < n1
//                                                 =  0                from n1 on            (reached in a final push only: the zero-padded last window)
//
//   stream_stage_kernel   stp::stage_blocks (st_predict.h) with that pair as the signal; the knob rows are ALWAYS filled here, row b from the knob row of its
//                         channel (or from the one row).
//   stream_ola_kernel     stp::ola_frame_sum with the residual from the pair; row (c, k) goes to out + c * out_pitch + k * y, clipped to the push's emitted count.
//   stream_carry_kernel   the samples to keep, [Wc(n1) y, n1) of every channel, from the pair into the OTHER history half (the halves then swap on the host): no
//                         quad is read and written in the same half, so the kernel needs no order among its lanes.
//
// Rows.  A push that computes windows first .. first + nw - 1 of C channels has C * nw rows, row r = c * nw + k being window first + k of channel c (channel-major:
// the overlapping windows of one channel are neighbours).  A batch is rows [r0, r0 + nb), nb <= d->B.
//
// Addresses.  Every non-final push has m % 4 == 0, so n0 % 4 == 0 for every push, and a, every window start and every residual offset are multiples of four
// (y % 4 == 0, L % 4 == 0): a quad of four samples lies wholly in the history or wholly in the block -- none straddles the join -- and is ONE aligned 16-byte
// (int16 block: 8-byte) access, the block base and pitch being aligned as the entry demands.  Only a final push may end off a quad; the one quad that straddles n1
// is read sample by sample (stp::pcm_quad_upto) and nothing at or past block[c] + m is addressed, whatever the pitch padding holds.  Output quads are clipped the
// same way at the emitted count.  History offsets stay below L; block and output offsets are 64-bit.
#pragma once
#include "st_predict.h"

namespace sts {

struct Src {
    const float* hist; const void* block;      // the current history half [C][hist_pitch], the push's block [C][block_pitch]
    long long a, n0, m, block_pitch;           // first sample held, samples received before the push, samples of the push
    int hist_pitch;                            // = L
};
// samples [g, g + 4) of channel c of the pair, a <= g, g % 4 == 0
template <typename T>
__device__ __forceinline__ float4 src_quad(const Src& s, const long long c, const long long g)
{
    if (g < s.n0) return *reinterpret_cast<const float4*>(s.hist + c * s.hist_pitch + (g - s.a));      // g + 4 <= n0: both multiples of four
    const long long o = g - s.n0;
    if (o >= s.m) return make_float4(0.f, 0.f, 0.f, 0.f);
    return stp::pcm_quad_upto(reinterpret_cast<const T*>(s.block) + c * s.block_pitch, o, s.m);
}

struct StageArgs {
    stp::StageCommon c;
    Src s;
    long long first, nw, r0;                  // first window of the push, windows of the push per channel, first row of this batch
    const float* knob_src; int knob_stride;   // knobs[b][k] = knob_src[ch * knob_stride + k], ch the channel of row r0 + b (knob_stride = 0: one setting for all channels)
};
template <typename T>
__global__ void __launch_bounds__(256)
stream_stage_kernel(const StageArgs a)
{
    stp::stage_blocks(a.c, blockIdx.x,
                      [&](const int b) {
                          const long long r = a.r0 + b, ch = r / a.nw, k = r - ch * a.nw;
                          const long long w0 = (a.first + k) * a.c.y;
                          return [=, &a](const long long g) { return src_quad<T>(a.s, ch, w0 + g); };
                      },
                      [&](const int b) { return a.knob_src + (a.r0 + b) / a.nw * a.knob_stride; });
}

// stp::ola_frame_sum with the residual from the pair; grid (ceil(y / 4 / 256), rows of the batch); row (c, k) goes to out + c * out_pitch + k * y.
// emit: samples this push emits per channel -- nw * y, less in a final push whose last window is clipped.
template <typename T, int NS, int NF>
__global__ void __launch_bounds__(256)
stream_ola_kernel(const float* __restrict__ frs, const size_t slab, const Src src, float* __restrict__ out, const long long out_pitch,
                  const long long first, const long long nw, const long long r0, const long long emit,
                  const int L, const int N, const int H, const int OT, const int ysz)
{
    const int b = blockIdx.y;
    const int j = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (j >= ysz) return;
    const long long r = r0 + b, c = r / nw, k = r - c * nw;
    const long long i = k * ysz + j;                      // output sample within the push's span of channel c; its input sample lies below n1 wherever i < emit
    if (i >= emit) return;
    const long long gx = (first + k) * ysz + (L - ysz) + j;      // the residual's input sample
    float s[4], rr[4];
    float4 xv;
    stp::ola_frame_sum<NS, NF>(frs + (size_t)b * OT * N, slab, N, H, OT, j, s, [&] { xv = src_quad<T>(src, c, gx); });
    stp::ola_out4(s, xv, rr);
    stp::store_quad_upto(out + c * out_pitch, rr, i, emit);
}

// Non-final pushes only (m % 4 == 0): quads [a1, n1) of every channel to the head of the other half; grid (ceil(held / 4 / 256), C).  held1 = n1 - a1 < L.
template <typename T>
__global__ void __launch_bounds__(256)
stream_carry_kernel(const Src src, float* __restrict__ next, const long long a1, const int held1)
{
    const int i = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (i >= held1) return;
    const long long c = blockIdx.y;
    const float4 v = src_quad<T>(src, c, a1 + i);
    *reinterpret_cast<float4*>(next + c * src.hist_pitch + i) = v;
}

}  // namespace sts
