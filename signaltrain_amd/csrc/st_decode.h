// st_decode.h -- a recording encoded once, decoded at any knob setting (st_encode_long / st_decode_long / st_fit_knobs_coded, gfx950).
//
// The knobs enter at fnn_addknobs, layer 5 of 9 (nn_proc.py:92-96): window staging, the analysis GEMM, the polar form and encoder layers 1..4 of both autoencoders
// do not depend on them.  For one recording and one parameter set they are computed ONCE and kept in HBM as the recording's CODE; a knob sweep and every step of a
// knob fit then run only what the knobs reach -- layers 5..9, the 'sf' skip and the phase residual, the polar epilogue -- in front of the frames GEMM.
//
// The code, window-major (independent of the batch it was built or is read at), CW = FP * (32 + 2 OT) floats per window, FP = KP / 2, gpw = FP / 16:
//     [h4 of the magnitude net : gpw groups x 64 lanes x float4, the D layout the forward kernels write (lane (g, c): features 4g .. 4g + 3 of bin 16 group + c)]
//     [h4 of the phase net     : the same]
//     [mag tail : OT rows of FP floats -- frames T - OT .. T - 1 of the window's mag, zeros in the pad bins f >= F]
//     [phs tail : the same of phs]
// Every block starts on a 64-byte boundary (FP % 16 == 0).  It is valid for the arithmetic level, the parameters and the recording it was built from.
//
//   code_pack_kernel      a plain HBM streamer behind the code-only pass of the forward kernel: the batch's h4 ([net][group of the batch][lane], 16-byte loads) and
//                         the two tails (rows of 4 F bytes: scalar loads) to their place in the code, 16-byte stores, no atomics.
//   ae_dec_fwd_kernel     the second half of ae_fwd_kernel: both nets in one wave (the polar epilogue needs mag_hat and phs_hat together), the same layer routine,
//                         the same epilogue; layer 5 takes the knob row as a second input tile, as the recompute of ae_knob_bwd_kernel does.
#pragma once
#include "st_ae_split.h"

namespace stc {

__host__ __device__ constexpr size_t code_window_floats(const int FP, const int OT) { return (size_t)FP * (size_t)(32 + 2 * OT); }

// grid (x: chunks, y: windows of the batch).  h4x: the exchange buffer of the batch ([net][B * gpw][64] float4), mag / phs: [B][T][F].
__global__ void __launch_bounds__(256)
code_pack_kernel(const float* __restrict__ h4x, const float* __restrict__ mag, const float* __restrict__ phs, float* __restrict__ code,
                 const int B, const int T, const int OT, const int F, const int FP)
{
    const int b = blockIdx.y;
    const int gpw = FP / 16, q4 = FP / 4;
    const int nh4 = gpw * 64, ntl = OT * q4;      // 16-byte elements of one net's h4 and of one tail
    const int n4 = 2 * nh4 + 2 * ntl;
    const float4* const h4v = reinterpret_cast<const float4*>(h4x);
    float4* const dst = reinterpret_cast<float4*>(code) + (size_t)b * n4;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        float4 v;
        if (i < 2 * nh4) {
            const int net = i >= nh4, j = i - net * nh4;
            v = h4v[((size_t)net * B + b) * nh4 + j];
        } else {
            int k = i - 2 * nh4;
            const int net = k >= ntl;
            k -= net * ntl;
            const int to = k / q4, f = (k - to * q4) * 4;
            const float* const src = (net ? phs : mag) + ((size_t)b * T + (size_t)(T - OT + to)) * F;
            v.x = f < F ? src[f] : 0.f; v.y = f + 1 < F ? src[f + 1] : 0.f; v.z = f + 2 < F ? src[f + 2] : 0.f; v.w = f + 3 < F ? src[f + 3] : 0.f;
        }
        dst[i] = v;
    }
}

}  // namespace stc

namespace sta {

// LDS: the forward images and biases of layers 5..9 of both nets and nothing else (CP<1> without its data-gradient images): 2 x 4496 floats = 35 KB of the
// 2 x 9488 the forward kernel keeps.  The compiler's figures leave the wave under 128 registers for every operand type: four waves per SIMD, as
// 8-wave workgroups, two per CU.
constexpr int AE_DEC_NW = 8, AE_DEC_WGS = 2;
constexpr int ae_dec_lds_floats() { return 2 * CP<1>::FWD_END; }

#define ST_DW2(off_) {lw[0] + (off_), lw[1] + (off_)}
struct DecIn { f32x4 h4[2]; f32x4 kn; float tl[2][4]; };

// grid.x workgroups of NW waves; each wave walks 16-row groups (group id = b * gpw + fg, fwd_group_walk's order), the inputs of the next group in flight.
//   code     the batch's first window of the code (layout above); 32-bit element offsets inside the batch (the host checks B * CW < 2^30)
//   knobs    row b * kstride of the batch: kstride = K, one row per window; kstride = 0, one setting for every window (no per-batch knob fill)
//   mag_hat, phs_hat   [B][OT][F], written only where the caller asks (both or neither): ae_knob_bwd_kernel reads them, the overlap-add does not
//   AA / AA16          [B][OT][KP] spectra, fp32 or rounded to the GEMM's operand type (AA16 != NULL), exactly as ae_fwd_kernel chooses; pad bins get zeros
//   h4_keep, mag_keep, kn_keep (all or none): the batch-layout copies ae_knob_bwd_kernel reads -- h4 [net][B * gpw][64] float4, the tail rows of a [B][T][F] mag,
//                      the knob row repeated over the batch [B][K] (kstride == 0 only)
// STK (st_multi.h): rows of the batch are (setting, window) pairs -- row b is window b % nw of the batch's windows at setting b / nw: it reads the code of window
//                      b % nw and the knob row at (b / nw) * set_stride + (b % nw) * kstride, and kn_keep always receives the [B][K] copy of the rows' knobs.
//                      STK == false is the kernel as it was: nw and set_stride are not read.
template <int NW, int BF = 0, bool STK = false>
__global__ void __launch_bounds__(NW * 64, 4)
ae_dec_fwd_kernel(const float* __restrict__ code, const float* __restrict__ knobs, const int kstride,
                  const float* __restrict__ ae_m, const float* __restrict__ ae_p, const AEOffsets go,
                  float* __restrict__ mag_hat, float* __restrict__ phs_hat, float* __restrict__ AA, unsigned short* __restrict__ AA16, const int aa_ht,
                  float* __restrict__ h4_keep, float* __restrict__ mag_keep, float* __restrict__ kn_keep,
                  const int B, const int T, const int OT, const int F, const int K, const int KP, const int nw, const unsigned set_stride)
{
    using P = CP<1>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    {
        const float* const nets[2] = {ae_m, ae_p};
        ae_load_nets<NW * 64, BF, 2>(lds, P::tab(), nets, go, T, OT, K, tid, P::L0, P::L1, false, false);
    }
    const float* const lw[2] = {lds, lds + P::FWD_END};
    const int FP = KP / 2, gpw = FP / 16;
    const int ngroups = B * gpw;
    const unsigned CW = ST_MUL24(FP, 32 + 2 * OT);
    const unsigned tl0 = (unsigned)FP * 32u, tl1 = tl0 + ST_MUL24(OT, FP);
    unsigned toK[4], toT[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { const int to = 4 * g + r; toK[r] = ST_MUL24(to, KP); toT[r] = ST_MUL24(to < OT ? to : 0, FP); }
    __syncthreads();

    // RAW loads from always valid addresses (a padding row re-reads row 0 of the tail, a knob past K knob 0); masked where they are consumed
    auto load_in = [&](const int gq, DecIn& in) {
        const int b = gq / gpw, fg = gq - b * gpw;
        const int bs = STK ? b / nw : 0, bw = STK ? b - bs * nw : b;      // the row's setting and window inside the batch
        const unsigned wb = ST_MUL24(bw, CW);
        const unsigned h = wb + (unsigned)(fg * 256 + lane * 4);
        in.h4[0] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(code) + (size_t)(h << 2));
        in.h4[1] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(code) + (size_t)((h + (unsigned)FP * 16u) << 2));
        const unsigned tb = wb + (unsigned)(fg * 16 + c);
        const unsigned kb = ST_MUL24(bw, kstride) + (STK ? (unsigned)bs * set_stride : 0u);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            in.tl[0][r] = ldg32(code, tb + tl0 + toT[r]); in.tl[1][r] = ldg32(code, tb + tl1 + toT[r]);
            const int kidx = 4 * g + r;
            in.kn[r] = ldg32(knobs, kb + (unsigned)(kidx < K ? kidx : 0));
        }
    };
    const GroupWalk gw = fwd_group_walk(ngroups, NW, wave);
    int grp = gw.first;
    DecIn cur;
    if (grp < gw.end) load_in(grp, cur);
    for (; grp < gw.end; grp += gw.stride) {
        asm volatile("" ::: "memory");      // keep the (loop-invariant) LDS weight fetches inside the loop
        const int b = grp / gpw, fg = grp - b * gpw, f = fg * 16 + c;
        const bool fv = f < F;
        DecIn nxt;
        load_in(grp + gw.stride < gw.end ? grp + gw.stride : grp, nxt);      // last trip: a harmless reload of this group

        f32x4 hk[2][2], h5[2][1], h6[2][1], h7[2][2], h8[2][4], e9[2][1];
        hk[0][0] = cur.h4[0]; hk[1][0] = cur.h4[1];
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float k = (4 * g + r) < K ? cur.kn[r] : 0.f; hk[0][1][r] = k; hk[1][1][r] = k; }
        if (h4_keep) {                                                        // wave-uniform: the fit's knob-only backward reads the batch layout
            f32x4* const hv = reinterpret_cast<f32x4*>(h4_keep);
            hv[(size_t)grp * 64 + lane] = cur.h4[0];
            hv[((size_t)ngroups + grp) * 64 + lane] = cur.h4[1];
            const unsigned mo = ST_MUL24(ST_MUL24(b, T) + (unsigned)(T - OT), F) + (unsigned)f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int to = 4 * g + r;
                if (fv && to < OT) stg32(mag_keep, mo + ST_MUL24(to, F), cur.tl[0][r]);
                if ((STK || kstride == 0) && fg == 0 && c == 0 && to < K) kn_keep[ST_MUL24(b, K) + (unsigned)to] = cur.kn[r];
            }
        }
        { const float* const W[2] = ST_DW2(P::A4); const float* const bb[2] = ST_DW2(P::B4); layer_fwd<2, 1, 2, CL::O4, BF>(W, bb, hk, h5, g, c); }
        { const float* const W[2] = ST_DW2(P::A5); const float* const bb[2] = ST_DW2(P::B5); layer_fwd<2, 1, 1, CL::O5, BF>(W, bb, h5, h6, g, c); }
        { const float* const W[2] = ST_DW2(P::A6); const float* const bb[2] = ST_DW2(P::B6); layer_fwd<2, 2, 1, CL::O6, BF>(W, bb, h6, h7, g, c); }
        { const float* const W[2] = ST_DW2(P::A7); const float* const bb[2] = ST_DW2(P::B7); layer_fwd<2, 4, 2, CL::O7, BF>(W, bb, h7, h8, g, c); }
        { const float* const W[2] = ST_DW2(P::A8); const float* const bb[2] = ST_DW2(P::B8); layer_fwd<2, 1, 4, CL::O8, BF>(W, bb, h8, e9, g, c); }
        // ---- epilogue (nn_proc.py:115,117,322-326), ae_fwd_kernel's without the L1 partials
        const unsigned boF = ST_MUL24(ST_MUL24(b, OT), F) + (unsigned)f, boK = ST_MUL24(ST_MUL24(b, OT), KP) + (unsigned)f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int to = 4 * g + r;
            if (to < OT) {
                float mh = 0.f, ph = 0.f, sn = 0.f, cs = 1.f;
                if (fv) {
                    mh = e9[0][0][r] * cur.tl[0][r];             // 'sf' skip-filter
                    ph = e9[1][0][r] + cur.tl[1][r];             // phase residual
                    st_sincos(ph, sn, cs);
                    if (mag_hat) {                               // wave-uniform
                        stg32(mag_hat, boF + ST_MUL24(to, F), mh);
                        stg32(phs_hat, boF + ST_MUL24(to, F), ph);
                    }
                }
                if (AA16) {                                      // wave-uniform
                    const int ht = BF ? BF : aa_ht;              // *_all modes: the spectra's type IS the layers' type
                    AA16[boK + toK[r]] = st_to_h16(mh * cs, ht);
                    AA16[boK + toK[r] + (unsigned)FP] = st_to_h16(mh * sn, ht);
                } else {
                    stg32(AA, boK + toK[r], mh * cs);            // f < FP always: pads get zeros
                    stg32(AA, boK + toK[r] + (unsigned)FP, mh * sn);
                }
            }
        }
        cur = nxt;
    }
}

}  // namespace sta
