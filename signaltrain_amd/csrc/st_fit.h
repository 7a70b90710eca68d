// st_fit.h -- the device route of predict.fit_knobs (st_fit_knobs, gfx950): the knob settings for which the model turns a recording into its processed version.
//
// Objective: J(knobs) = (1 / n_out) * sum_{i < n_out} logcosh(y_hat_i - target_i), y_hat as st_predict_long forms it (st_predict.h: window w IS signal[w y, w y + L),
// output sample i belongs to input sample (L - y) + i, and so does its target).  The knobs enter at fnn_addknobs, layer 5 of 9 (nn_proc.py:92-93), so behind the
// forward d J / d knobs needs the synthesis data-gradient GEMM, the data-gradient chain of layers 9..6 and ELU' at layer 5 -- and nothing else:
//
//   fit_ola_kernel        predict_ola_kernel's overlap-add (stp::ola_frame_sum, the same residual from the recording) with the loss side: d = y_hat - target, the
//                         target read straight from the target recording; 2 tanh(d) into the padded d syn operand of the data-gradient GEMM (fp32, or rounded to
//                         the 16-bit operand type where the 16-bit pipeline runs), zero margins, zeros at and behind the recording's end, and the per-slot
//                         log-cosh partials (stp::logcosh_term) in ola_loss4_kernel's tree.  d syn is NOT scaled by 1 / n_out: tanh / n_out of a ten-minute recording
//                         is ~1e-7, below the fp16 subnormal range -- the scale is applied in fp32 behind W5 (fit_tail_kernel).
//   ae_knob_bwd_kernel    the decoder half of st_ae_split.h without its 17 weight-gradient tiles, bias gradients, d a4, tails, gradient images and end-of-kernel
//                         reduction: h4 (kept by the forward kernel) -> layers 5..9 recomputed -> d out -> data gradients 9, 8, 7, 6 -> ELU' at layer 5 ->
//                         the group's column sums of d a5 (group_colsum_store), [net][group][16].
//   fit_tail_kernel       one small launch per batch: the batch's loss partials into loss_hist[s] in double; the batch's per-window gradient rows (knob_grad_kernel)
//                         summed in ascending window order (one knob row) or taken row by row (one row per window); after the step's last batch 1 / n_out,
//                         grad_hist[s], torch.optim.Adam's update and the clamp to [-0.5, 0.5].
// No float atomics; every sum has a fixed order.
#pragma once
#include "st_ae_split.h"
#include "st_predict.h"

namespace stf {

// Four output samples per lane, grid (ceil(y / 4 / 256), windows of the batch): stp::ola_frame_sum (NF = 3 / NF = 0 as there), then the loss side.  A wave's 64
// quads are one slot of 256 samples: slot = 4 * blockIdx.x + wave, nslot = ceil(y / 256) per window, the tree of ola_loss4_kernel.  Samples at or behind n_out carry
// neither loss nor gradient.  dsyn16 != NULL: the operand goes out rounded to the 16-bit type ht INSTEAD of fp32 (what the 16-bit data-gradient GEMM reads).
// STK (st_multi.h): 0, the kernel as it was (nw is not read).  1: rows of the batch are (setting, window) pairs -- the frames, the d-syn row and the partials are
// row b's, the recording's samples those of window b % nw.  2: the same rows, the score form: the sums and the log-cosh partials, no d-syn operand written.
template <typename T, int NS, int NF, int STK = 0>
__global__ void __launch_bounds__(256)
fit_ola_kernel(const float* __restrict__ frs, const size_t slab, const T* __restrict__ sig, const T* __restrict__ tgt,
               float* __restrict__ dsyn, unsigned short* __restrict__ dsyn16, const int ht, float* __restrict__ loss_partial, const int nslot,
               const long long s0, const long long n_out, const int L, const int N, const int H, const int OT, const int ysz, const int nw)
{
    const int b = blockIdx.y;
    const int j = 4 * (blockIdx.x * 256 + threadIdx.x);
    const long long i = s0 + (long long)(STK ? b % nw : b) * ysz + j;      // output sample; its input and target sample is (L - ysz) + i < n wherever i < n_out
    float lc = 0.f;
    float ds[4] = {0.f, 0.f, 0.f, 0.f};
    if (j < ysz && i < n_out) {
        float s[4], out[4];
        float4 xv, tv;
        stp::ola_frame_sum<NS, NF>(frs + (size_t)b * OT * N, slab, N, H, OT, j, s, [&] {
            xv = stp::pcm_quad_upto(sig, i + (L - ysz), n_out + (L - ysz));
            tv = stp::pcm_quad_upto(tgt, i + (L - ysz), n_out + (L - ysz));
        });
        stp::ola_out4(s, xv, out);
        const float ts[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool valid = i + q < n_out;
            const float dlt = ts[q] - out[q];
            const float l1 = stp::logcosh_term(fabsf(dlt));
            lc += valid ? l1 : 0.f;
            ds[q] = valid ? -2.0f * tanhf(dlt) : 0.f;      // 2 tanh(y_hat - target): d y_hat / d (overlap-added sample) = 2; 1 / n_out comes behind W5
        }
    }
    if constexpr (STK != 2) {
        const size_t ro = (size_t)b * (ysz + 2 * N);
        if (j < ysz) {
            if (dsyn16) *reinterpret_cast<uint2*>(dsyn16 + ro + N + j) = st_to_h16x4(make_float4(ds[0], ds[1], ds[2], ds[3]), ht);
            else *reinterpret_cast<float4*>(dsyn + ro + N + j) = make_float4(ds[0], ds[1], ds[2], ds[3]);
        }
        for (int m = blockIdx.x * 256 + threadIdx.x; m < 2 * N; m += gridDim.x * 256) {      // the Conv padding of the gradient signal
            if (dsyn16) dsyn16[ro + (m < N ? m : ysz + m)] = 0;
            else dsyn[ro + (m < N ? m : ysz + m)] = 0.f;
        }
    }
    float q = lc;        // ((l0 + l1) + l2) + l3, formed in sample order above
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) q += __shfl_xor(q, o);
    const int slot = 4 * blockIdx.x + (threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0 && slot < nslot) loss_partial[blockIdx.y * nslot + slot] = q;
}

// The per-batch tail, one workgroup of 256 threads.
//   loss: the batch's n_lp partials, lane-strided in double, then a fixed tree over the 256 lanes; *loss = (first batch of the step ? 0 : *loss) + that, and after the
//         last batch times 1 / n_out: J at the knobs before the update.
//   rows: [nb][K] = sum over both nets and the window's rows of W5[o][16 + k] * d a5 (knob_grad_kernel), this batch's windows.
//         per_window == 0: acc[k] = (first ? 0 : acc[k]) + rows[0][k] + rows[1][k] + ... in ascending window order; after the last batch g = acc * inv_n -> Adam on
//                          the one knob row.  per_window != 0: g = rows[b][k] * inv_n -> Adam on this batch's rows of knobs / m / v / grad (the pointers are the batch's).
//   Adam: torch.optim.Adam's single-tensor step in ST_ADAM1's arithmetic (st_misc.h), then the clamp.
struct TailArgs {
    const float* loss_p; int n_lp; double* loss; double inv_n_d;
    const float* rows; int nb, K; float* acc;
    float *knobs, *m, *v, *grad;      // grad may be NULL
    int per_window, first, last;
    float inv_n, neg_step, w1, b2, w2, bc2_sqrt, eps;
};
__device__ __forceinline__ void fit_adam_one(const TailArgs& a, const int e, const float g)
{
    if (a.grad) a.grad[e] = g;
    float M = a.m[e], V = a.v[e], P = a.knobs[e];
    M = M + a.w1 * (g - M);
    V = V * a.b2 + (a.w2 * g) * g;
    const float den = sqrtf(V) / a.bc2_sqrt + a.eps;
    P = P + (a.neg_step * M) / den;
    P = fminf(fmaxf(P, -0.5f), 0.5f);
    a.m[e] = M; a.v[e] = V; a.knobs[e] = P;
}
constexpr int FIT_TAIL_BUF = 4096;
__global__ void __launch_bounds__(256)
fit_tail_kernel(const TailArgs a)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < a.n_lp; i += 256) s += (double)a.loss_p[i];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        double t = (a.first ? 0.0 : *a.loss) + red[0];
        if (a.last) t *= a.inv_n_d;
        *a.loss = t;
    }
    if (a.per_window) {
        for (int e = tid; e < a.nb * a.K; e += 256) fit_adam_one(a, e, a.rows[e] * a.inv_n);
    } else {
        // the rows come in through LDS, FIT_TAIL_BUF floats at a time, loaded by all lanes at once: lane k then adds its column in ascending window order without a
        // dependent global load per window (256 windows: ~20 us of round trips otherwise)
        __shared__ float buf[FIT_TAIL_BUF];
        const int per = FIT_TAIL_BUF / a.K;      // 1 <= K <= 16 (check_dims)
        float acc = (a.first || tid >= a.K) ? 0.f : a.acc[tid];
        for (int r0 = 0; r0 < a.nb; r0 += per) {
            const int nr = a.nb - r0 < per ? a.nb - r0 : per;
            for (int e = tid; e < nr * a.K; e += 256) buf[e] = a.rows[(size_t)r0 * a.K + e];
            __syncthreads();
            if (tid < a.K) {
#pragma unroll 8
                for (int b = 0; b < nr; ++b) acc += buf[b * a.K + tid];
            }
            __syncthreads();
        }
        if (tid < a.K) {
            a.acc[tid] = acc;
            if (a.last) fit_adam_one(a, tid, acc * a.inv_n);
        }
    }
}

}  // namespace stf

namespace sta {

// grid (x: workgroups, y: net 0 = magnitude 'sf' / 1 = phase); the persistent loop of the decoder half: wave w of workgroup x walks groups x NW + w, + gridDim.x NW, ...
// LDS: the decoder half's compact images (CP<1>: forward images and biases of layers 5..9, their data-gradient images) + one 16 x 16 transpose scratch per wave.
// No weight-gradient accumulators live across the loop: the fp32 form needs 132 registers or so at its peak (fragments of layers 8 and 9, the raw d-out loads, the
// activations), which spills at the 128 of four waves per SIMD and fits the 168 of three -- so NW = 12: one 12-wave workgroup per CU, three waves per SIMD, for
// every operand type (DESIGN.md has the compiler's figures).
// kg[net][group][16]: the group's column sums of d a5 (the bias gradient of fnn_addknobs of a batch that holds this group alone).
constexpr int ae_knob_lds_floats(int nw) { return CP<1>::TOTAL + nw * 320; }
template <int NW, int BF = 0>
__global__ void __launch_bounds__(NW * 64, 3)
ae_knob_bwd_kernel(const float* __restrict__ mag, const float* __restrict__ knobs,
                   const float* __restrict__ ae_m, const float* __restrict__ ae_p, const AEOffsets go,
                   const float* __restrict__ mag_hat, const float* __restrict__ phs_hat, const float* __restrict__ dAA,
                   const float* __restrict__ h4x, float* __restrict__ kg,
                   const int B, const int T, const int OT, const int F, const int K, const int KP,
                   const int to_lo, const int to_hi, const int nslab, const size_t slab)
{
    using P = CP<1>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int ae = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    float* lw = lds;
    float* XD = lds + P::TOTAL + wave * 320;
    ae_load_lds_tab<NW * 64, BF>(lw, P::tab(), ae ? ae_p : ae_m, go, T, OT, K, tid, P::L0, P::L1);
    __syncthreads();

    const int FP = KP / 2, gpw = FP / 16;
    const int ngroups = B * gpw;
    const int gstride = gridDim.x * NW;
    const float4* h4v = reinterpret_cast<const float4*>(h4x) + (size_t)ae * ngroups * 64;

    // per-group inputs prefetched one group ahead: h4 (one 16-byte load) and the knob values as a D-layout tile
    auto load_in = [&](int gq, f32x4& h4q, f32x4& k4) {
        const float4 v = h4v[(size_t)gq * 64 + lane];
        h4q = (f32x4){v.x, v.y, v.z, v.w};
        const unsigned kb = ST_MUL24(gq / gpw, K);
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int kidx = 4 * g + r; k4[r] = ldg32(knobs, kb + (unsigned)(kidx < K ? kidx : 0)); }
    };
    auto mask_kn = [&](f32x4& d4) {
#pragma unroll
        for (int r = 0; r < 4; ++r) d4[r] = (4 * g + r) < K ? d4[r] : 0.f;
    };
    int grp = blockIdx.x * NW + wave;
    f32x4 h4c = (f32x4){0.f, 0.f, 0.f, 0.f}, kn = h4c;
    if (grp < ngroups) { load_in(grp, h4c, kn); mask_kn(kn); }
    for (; grp < ngroups; grp += gstride) {
        asm volatile("" ::: "memory");
        const int b = grp / gpw, f = (grp - b * gpw) * 16 + c;
        const bool fv = f < F;
        const int fq = fv ? f : 0;
        // ---- d-out inputs (D layout: t' = 4g + r): raw loads, sums and masks formed later (as the decoder half)
        float q_x[4][3], q_y[4][3], q_ph[4], q_mh[4], q_mt[4];
        {
            const size_t o1 = nslab > 1 ? slab : 0, o2 = nslab > 2 ? 2 * slab : 0;
            const float* const dA0 = dAA, * const dA1 = dAA + o1, * const dA2 = dAA + o2;
            const float* const dB0 = dA0 + FP, * const dB1 = dA1 + FP, * const dB2 = dA2 + FP;
            const unsigned bOT = ST_MUL24(b, OT), btF = ST_MUL24(ST_MUL24(b, T), F) + (unsigned)fq;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int to = 4 * g + r;
                const bool ok = fv && to < OT;
                const bool lv = ok && to >= to_lo && to <= to_hi;
                const unsigned ro = bOT + (unsigned)(ok ? to : 0);
                const unsigned p0 = ST_MUL24(lv ? ro : bOT + (unsigned)to_lo, KP) + (unsigned)fq;      // a dead or padding row re-reads the window's first live row (value dropped)
                const unsigned pF = ST_MUL24(ro, F) + (unsigned)fq;
                q_x[r][0] = ldg32(dA0, p0); q_x[r][1] = ldg32(dA1, p0); q_x[r][2] = ldg32(dA2, p0);
                q_y[r][0] = ldg32(dB0, p0); q_y[r][1] = ldg32(dB1, p0); q_y[r][2] = ldg32(dB2, p0);
                q_ph[r] = ldg32(phs_hat, pF); q_mh[r] = ldg32(mag_hat, pF);
                q_mt[r] = ldg32(mag, btF + ST_MUL24(ok ? T - OT + to : 0, F));
            }
        }
        f32x4 h4n, knn;
        const int gnext = grp + gstride < ngroups ? grp + gstride : grp;
        load_in(gnext, h4n, knn);
        // ---- forward recompute, layers 5..9 (the decoder half's chain: rolling fragment prefetch)
        f32x4 h5[1], h6[1], h7[2], h8[4], e9[1];
        f32x4 fr5[1 * 2]; frags_fwd<1, 2, CL::O4, BF>(fr5, lw + P::A4, g, c);
        f32x4 fr6[1 * 1]; frags_fwd<1, 1, CL::O5, BF>(fr6, lw + P::A5, g, c); ST_FENCE();
        { const f32x4 hk[2] = {h4c, kn}; fwdD_fr<1, 2, BF>(fr5, lw + P::B4, hk, h5, g); }
        f32x4 fr7[2 * 1]; frags_fwd<2, 1, CL::O6, BF>(fr7, lw + P::A6, g, c); ST_FENCE(); fwdD_fr<1, 1, BF>(fr6, lw + P::B5, h5, h6, g);
        f32x4 fr8[4 * 2]; frags_fwd<4, 2, CL::O7, BF>(fr8, lw + P::A7, g, c); ST_FENCE(); fwdD_fr<2, 1, BF>(fr7, lw + P::B6, h6, h7, g);
        f32x4 fr9[1 * 4]; frags_fwd<1, 4, CL::O8, BF>(fr9, lw + P::A8, g, c); ST_FENCE(); fwdD_fr<4, 2, BF>(fr8, lw + P::B7, h7, h8, g);
        // ---- d out (nn_proc.py:322-326 backward; no L1 term in J), its first part under the layer-9 MFMAs
        float dxA[4];
        ST_FENCE();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int to = 4 * g + r;
            const bool ok = fv && to < OT;
            const bool lv = ok && to >= to_lo && to <= to_hi;
            const float gre = lv ? q_x[r][0] + (nslab > 1 ? q_x[r][1] : 0.f) + (nslab > 2 ? q_x[r][2] : 0.f) : 0.f;
            const float gim = lv ? q_y[r][0] + (nslab > 1 ? q_y[r][1] : 0.f) + (nslab > 2 ? q_y[r][2] : 0.f) : 0.f;
            const float ph = q_ph[r], mh = q_mh[r];
            float sn, cs; st_sincos(ph, sn, cs);
            const float dmh = gre * cs + gim * sn;
            const float dph = mh * (gim * cs - gre * sn);
            dxA[r] = ok ? (ae == 0 ? dmh * q_mt[r] : dph) : 0.f;      // 'sf': mag_hat = e9 * mag tail
        }
        fwdD_fr<1, 4, BF>(fr9, lw + P::B8, h8, e9, g);
        f32x4 fd9[4 * 1]; frags_dgrad<1, 4, CL::I8, BF>(fd9, lw + P::G8, g, c);
        f32x4 fd8[2 * 4]; frags_dgrad<4, 2, CL::I7, BF>(fd8, lw + P::G7, g, c);
        ST_FENCE();
        f32x4 da9[1];
#pragma unroll
        for (int r = 0; r < 4; ++r) da9[0][r] = dxA[r] * elu_grad_from_out(e9[0][r]);
        // ---- data gradients 9..6, ELU' at 8..5
        f32x4 da8[4], da7[2], da6[1], da5[1], daT5[1];
        dgradD_fr<1, 4, BF>(fd9, da9, da8); mul_elu_grad<4>(da8, h8);
        f32x4 fd7[1 * 2]; frags_dgrad<2, 1, CL::I6, BF>(fd7, lw + P::G6, g, c);
        f32x4 fd6[1]; frags_dgrad<1, 1, CL::I5, BF>(fd6, lw + P::G5, g, c);
        ST_FENCE();
        dgradD_fr<4, 2, BF>(fd8, da8, da7); mul_elu_grad<2>(da7, h7);
        dgradD_fr<2, 1, BF>(fd7, da7, da6); mul_elu_grad<1>(da6, h6);
        dgradD_fr<1, 1, BF>(fd6, da6, da5); mul_elu_grad<1>(da5, h5);
        to_T<1>(XD, da5, daT5, g, c);
        group_colsum_store(kg + ((size_t)ae * ngroups + grp) * 16, daT5[0], g, c);
        mask_kn(knn); kn = knn; h4c = h4n;
    }
}

}  // namespace sta
