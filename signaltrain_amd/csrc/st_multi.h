// st_multi.h -- many knob settings of one recording's code in one call (st_knob_multi_plan / st_score_knobs_coded / st_fit_knobs_multi_coded, gfx950).
//
// The knob objective J (st_fit.h) is not convex in the knobs: a search scores many candidate settings, keeps the best few and refines them together.  Both steps
// ride on the recording's code (st_decode.h) and on batches whose ROWS ARE (SETTING, WINDOW) PAIRS, so that a recording shorter than a batch still fills it:
//
//   row map     a plan batch (w0, nw, s0, ns) holds windows w0 .. w0 + nw - 1 at settings s0 .. s0 + ns - 1, nw * ns <= d->B rows; row r is setting s0 + r / nw at
//               window w0 + r % nw.  The frames, the d-syn rows, the kept h4 / magnitude tail / knob copy and the per-group scratch are the ROW's; the code and
//               the recording's samples are the WINDOW's.
//   plan rule   2 * nwin > d->B: st_decode_long's batches, ns == 1, nw = min(B, nwin - w0), the settings loop inside the window batch.  Otherwise every batch
//               holds the whole recording ns = min(B / nwin, S - s0) times.
//   kernels     ae_dec_fwd_kernel<.., STK = true> (st_decode.h) and fit_ola_kernel<.., STK = 1 | 2> (st_fit.h) are the existing kernels with the row map compiled in
//               (2: the score form, the same sums and log-cosh partials with no store of d syn); the frames GEMM, the data-gradient GEMM, ae_knob_bwd_kernel and
//               knob_grad_kernel see nw * ns independent rows and do not change.  multi_tail_kernel below is fit_tail_kernel per setting of the batch.
//   tails       the fit needs a setting's tail behind each of its batches (Adam follows the last).  The score of a recording that is not stacked keeps the partials
//               of EVERY setting of a window batch ([S][d->B * nslot] in the workspace) and folds them in one tail launch of S workgroups behind the last setting:
//               a launch per (batch, setting) of a kernel that lasts microseconds would cost more than the torch pass it replaces.
// No float atomics; every sum has a fixed order.
#pragma once
#include "st_fit.h"

namespace stx {

// ---- the plan: host arithmetic only.  Batch i of count(); for any one setting its windows come in ascending order, every (setting, window) pair exactly once.
struct MultiBatch { int w0, nw, s0, ns; };
struct MultiPlan {
    long long nwin; int B, S; bool stacked; int per;      // per: settings of a full stacked batch
    __host__ long long count() const { return stacked ? ((long long)S + per - 1) / per : ((nwin + B - 1) / B) * (long long)S; }
    __host__ MultiBatch at(const long long i) const
    {
        MultiBatch m;
        if (stacked) { m.w0 = 0; m.nw = (int)nwin; m.s0 = (int)(i * per); m.ns = S - m.s0 < per ? S - m.s0 : per; }
        else { const long long wb = i / S; m.w0 = (int)(wb * B); m.nw = (int)(nwin - m.w0 < B ? nwin - m.w0 : B); m.s0 = (int)(i - wb * S); m.ns = 1; }
        return m;
    }
};
// nwin >= 1, B >= 1, S >= 1.  The stacking threshold: a recording of at most half a batch.
__host__ inline MultiPlan multi_plan(const long long nwin, const int B, const int S)
{
    MultiPlan p; p.nwin = nwin; p.B = B; p.S = S;
    p.stacked = 2 * nwin <= (long long)B;
    p.per = p.stacked ? (int)(B / nwin) : 1;
    return p;
}

// ---- the per-batch tail, one workgroup of 256 threads PER SETTING of the batch (grid.x = ns): fit_tail_kernel's arithmetic on the setting's rows.
//   loss: the setting's nw * nslot partials (at loss_p + sidx * lp_stride: rows sidx * nw .. of a stacked batch), lane-strided in double, then the fixed tree
//         over the 256 lanes; loss[s] = (first batch of this setting ? 0 : loss[s]) + that, and after its last batch times 1 / n_out.  loss[s] is the setting's
//         accumulator between its batches.
//   win_loss (score, may be NULL): window w's nslot partials summed in ascending slot order in double, times 1 / n_out -> win_loss[s][w0 + w].
//   fit (rows != NULL): the setting's nw gradient rows summed in ascending window order into acc[s][K] through LDS as fit_tail_kernel does (one knob row), or taken
//         row by row (one row per window); after the setting's last batch 1 / n_out, grad, fit_adam_one and the clamp on the setting's rows of knobs / m / v.
struct MultiTailArgs {
    stf::TailArgs t;           // hyper-parameters, K, per_window, first, last; its pointers are those of setting s0 (window w0 where per_window)
    int nw, nslot;             // windows of the batch, partials per window
    size_t lp_stride;          // floats between two settings' partials in t.loss_p
    size_t set_stride;         // floats between two settings' rows of knobs / m / v / grad
    double* loss;              // loss[s0]
    float* win_loss;           // win_loss[s0][w0], or NULL
    long long win_pitch;       // nwin
    float* acc;                // acc[s0][16]
};
__global__ void __launch_bounds__(256)
multi_tail_kernel(const MultiTailArgs m)
{
    __shared__ double red[256];
    const int tid = threadIdx.x, sidx = blockIdx.x;
    stf::TailArgs a = m.t;
    const int n_lp = m.nw * m.nslot;
    const float* const lp = a.loss_p + (size_t)sidx * m.lp_stride;
    double s = 0.0;
    for (int i = tid; i < n_lp; i += 256) s += (double)lp[i];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        double t = (a.first ? 0.0 : m.loss[sidx]) + red[0];
        if (a.last) t *= a.inv_n_d;
        m.loss[sidx] = t;
    }
    if (m.win_loss) {
        for (int w = tid; w < m.nw; w += 256) {
            double q = 0.0;
            for (int k = 0; k < m.nslot; ++k) q += (double)lp[w * m.nslot + k];
            m.win_loss[(size_t)sidx * m.win_pitch + w] = (float)(q * a.inv_n_d);
        }
    }
    if (!a.rows) return;
    const size_t so = (size_t)sidx * m.set_stride;
    a.rows += (size_t)sidx * m.nw * a.K; a.nb = m.nw;
    a.knobs += so; a.m += so; a.v += so; if (a.grad) a.grad += so;
    if (a.per_window) {
        for (int e = tid; e < a.nb * a.K; e += 256) stf::fit_adam_one(a, e, a.rows[e] * a.inv_n);
    } else {
        __shared__ float buf[stf::FIT_TAIL_BUF];
        float* const accp = m.acc + (size_t)sidx * 16;
        const int per = stf::FIT_TAIL_BUF / a.K;      // 1 <= K <= 16 (check_dims)
        float acc = (a.first || tid >= a.K) ? 0.f : accp[tid];
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
            accp[tid] = acc;
            if (a.last) stf::fit_adam_one(a, tid, acc * a.inv_n);
        }
    }
}

}  // namespace stx
