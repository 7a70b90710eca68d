// st_eval_pool.h -- the three kernels of st_eval_pool (gfx950): a folder of recordings, kept in HBM as one concatenated pool, through the model in one call.
//
// Reference: reporting a model on a SignalTrain test set is utils/predict_long.py:30-79 per file (each at the knob setting in its name, datasets.py:64-259)
// followed by the error figures per file.  The device feeds already keep such a folder as a pool (st_feed_files.h: pool_x / pool_y, file_off, file_len, one
// knob row per file); here every file is run WHOLE, st_predict_long's way (st_predict.h: window w of a file IS file[w y, w y + L), output sample i belongs to
// the file's sample (L - y) + i), with batch rows that are (file, window) pairs so that short clips share a batch and a long file spans several.
//
// Rows.  Row r of the pool is window r - win_off[f] of file f, win_off[f] <= r < win_off[f + 1]: file-major, windows ascending.  win_off[nfiles + 1] (int64, device)
// holds the prefix sums of the files' window counts (st_eval_pool_rows); every kernel finds f by a binary search of it.  A batch is rows [r0, r0 + nb), nb <= d->B.
//
//   pool_stage_kernel   stp::stage_blocks (st_predict.h) with the window read from its file, zeros behind the file's end, and the knob rows ALWAYS filled: row b
//                       gets its file's row of file_knobs.  A side role (extra blocks, the call's first launch only) writes what no row writes: the zero head of
//                       every file's span of `out` and the zero statistics of the files without a window.
//   pool_ola_kernel     stp::ola_frame_sum, the residual from the file, the result at out[file_off + (L - y) + i] -- time-aligned with the input -- clipped at the
//                       file's end; with a target pool, the per-slot float32 partials of log cosh e (stp::logcosh_term), |e|, e^2, t^2, y_hat^2 and max |e|
//                       (e = y_hat - t), one slot = one wave = 256 samples.
//   pool_tail_kernel    one launch per batch, one workgroup per file the batch touches: that file's partials of the batch into stats[f] in double.
//
// Addresses.  file_off[f] need not be a multiple of four.  A quad of four samples is ONE 16-byte access (int16: 8-byte) only where its pool address is aligned and
// it lies wholly inside the file; otherwise it is read (written) sample by sample -- the values are the same either way.  file_span() clamps what the tables say:
// off to [0, pool_samples], len to [0, pool_samples - off], and file_of() the window index to >= 0 -- so whatever the tables hold, every address formed lies inside
// [0, pool_samples) of the pools and of out, and inside [0, nfiles) of the tables (as st_file_feed's clamps, st_feed_files.h).  Truthful tables are never clamped.
// No float atomics; every sum has a fixed order; a repeated call repeats its bits.
#pragma once
#include "st_predict.h"

namespace stq {

enum { POOL_STATS = 8, POOL_PART = 6 };      // stats per file (ST_POOL_STATS); partial planes per batch: logcosh, |e|, e^2, t^2, y_hat^2, max |e|

struct Tables {
    const long long *file_off, *file_len, *win_off;      // device: [nfiles], [nfiles], [nfiles + 1]
    int nfiles; long long pool_samples;
};
struct FileRow { int f; long long off, len, w, first, end; };      // file, its clamped span, the window of the row, the file's first row and the row behind its last

// file f's span as the tables give it, clamped: off to [0, pool_samples], len to [0, pool_samples - off]
__device__ __forceinline__ void file_span(const Tables& t, const int f, long long& off, long long& len)
{
    off = t.file_off[f]; len = t.file_len[f];
    off = off < 0 ? 0 : (off > t.pool_samples ? t.pool_samples : off);
    len = len < 0 ? 0 : (len > t.pool_samples - off ? t.pool_samples - off : len);
}
// the file of row r: the last f with win_off[f] <= r (files without a window share their successor's entry and are passed over)
__device__ __forceinline__ FileRow file_of(const Tables& t, const long long r)
{
    int lo = 0, hi = t.nfiles;      // win_off[lo] <= r < win_off[hi] wherever the table is truthful
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.win_off[mid] <= r) lo = mid; else hi = mid;
    }
    FileRow q;
    q.f = lo;
    file_span(t, lo, q.off, q.len);
    q.first = t.win_off[lo]; q.end = t.win_off[lo + 1];
    q.w = r - q.first; if (q.w < 0) q.w = 0;
    return q;
}
// samples [g, g + 4) of a file (g >= 0, g % 4 == 0), zero from sample len on
template <typename T>
__device__ __forceinline__ float4 file_quad(const T* __restrict__ pool, const long long off, const long long g, const long long len)
{
    if (g + 4 <= len && ((off + g) & 3) == 0) return stp::pcm_quad(pool + off + g);
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = g + q < len ? stp::pcm_one(pool + off + g + q) : 0.f;
    return make_float4(v[0], v[1], v[2], v[3]);
}

// a * a as a float32 term of its own: rounded before it is added to a sum, never fused into the addition (the statistics' per-sample terms are float32 values)
__device__ __forceinline__ float square_rn(const float a)
{
#pragma clang fp contract(off)
    return a * a;
}

struct StageArgs {
    stp::StageCommon c;
    const void* pool_x; Tables t;
    long long r0;                             // first row of this batch
    const float* file_knobs;                  // knobs[b][k] = file_knobs[f][k], f the file of row r0 + b
    float* out; double* stats; int n_zero;    // the side role: n_zero blocks (0 in every launch but the call's first); out / stats may be NULL
};
// stp::stage_blocks' three ranges; behind them the n_zero blocks of the side role, file f by block f % n_zero.
template <typename T>
__global__ void __launch_bounds__(256)
pool_stage_kernel(const StageArgs a)
{
    const T* __restrict__ pool = reinterpret_cast<const T*>(a.pool_x);
    const bool staged = stp::stage_blocks(a.c, blockIdx.x,
        [&](const int b) {
            const FileRow fr = file_of(a.t, a.r0 + b);
            const long long w0 = fr.w * a.c.y;
            return [=](const long long g) { return w0 + g < fr.len ? file_quad(pool, fr.off, w0 + g, fr.len) : make_float4(0.f, 0.f, 0.f, 0.f); };
        },
        [&](const int b) { return a.file_knobs + (size_t)file_of(a.t, a.r0 + b).f * a.c.K; });
    if (staged) return;
    for (int f = blockIdx.x - a.c.n_pad - a.c.n_dead - a.c.n_kn; f < a.t.nfiles; f += a.n_zero) {
        long long off, len; file_span(a.t, f, off, len);
        const long long head = len < a.c.L - a.c.y ? len : a.c.L - a.c.y;      // no window predicts these samples
        if (a.out) for (long long i = threadIdx.x; i < head; i += 256) a.out[off + i] = 0.f;
        if (a.stats && a.t.win_off[f + 1] <= a.t.win_off[f] && threadIdx.x < POOL_STATS) a.stats[(size_t)f * POOL_STATS + threadIdx.x] = 0.0;
    }
}

// Four output samples per lane, grid (ceil(y / 4 / 256), rows of the batch): stp::ola_frame_sum, then stp::ola_out4 with x the residual sample of the file.
// tgt != NULL: the loss side as fit_ola_kernel forms it -- a wave's 64 quads are one slot of
// 256 samples, slot = 4 * blockIdx.x + wave, nslot = ceil(y / 256) per row; per lane ((q0 + q1) + q2) + q3 in sample order, then the xor tree over the 64 lanes (max for
// the peak).  Samples at or behind the file's end carry nothing.  part: [POOL_PART][plane] floats, plane >= rows of the batch * nslot, element b * nslot + slot.
// out == NULL: the score form, nothing stored but the partials.
template <typename T, int NS, int NF>
__global__ void __launch_bounds__(256)
pool_ola_kernel(const float* __restrict__ frs, const size_t slab, const T* __restrict__ pool_x, const T* __restrict__ tgt, float* __restrict__ out,
                float* __restrict__ part, const size_t plane, const int nslot, const Tables tb, const long long r0,
                const int L, const int N, const int H, const int OT, const int ysz)
{
    const int b = blockIdx.y;
    const int j = 4 * (blockIdx.x * 256 + threadIdx.x);
    const FileRow fr = file_of(tb, r0 + b);
    const long long n_out = fr.len - (L - ysz);
    const long long i = fr.w * ysz + j;                   // output sample within the file; its input and target sample is (L - ysz) + i < len wherever i < n_out
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float peak = 0.f;
    if (j < ysz && i < n_out) {
        float s[4], r[4];
        float4 xv, tv = make_float4(0.f, 0.f, 0.f, 0.f);
        stp::ola_frame_sum<NS, NF>(frs + (size_t)b * OT * N, slab, N, H, OT, j, s, [&] {
            xv = file_quad(pool_x, fr.off, i + (L - ysz), fr.len);
            if (tgt) tv = file_quad(tgt, fr.off, i + (L - ysz), fr.len);
        });
        stp::ola_out4(s, xv, r);
        if (out) stp::store_quad_upto(out + fr.off + (L - ysz), r, i, n_out, (fr.off & 3) == 0);
        if (tgt) {
            const float ts[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool valid = i + q < n_out;
                const float dlt = ts[q] - r[q];
                const float e = fabsf(dlt);
                const float l1 = stp::logcosh_term(e);
                acc[0] += valid ? l1 : 0.f;
                acc[1] += valid ? e : 0.f;
                acc[2] += valid ? square_rn(dlt) : 0.f;
                acc[3] += valid ? square_rn(ts[q]) : 0.f;
                acc[4] += valid ? square_rn(r[q]) : 0.f;
                peak = valid ? fmaxf(peak, e) : peak;
            }
        }
    }
    if (tgt) {      // uniform over the grid
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
            for (int k = 0; k < 5; ++k) acc[k] += __shfl_xor(acc[k], o);
            peak = fmaxf(peak, __shfl_xor(peak, o));
        }
        const int slot = 4 * blockIdx.x + (threadIdx.x >> 6);
        if ((threadIdx.x & 63) == 0 && slot < nslot) {
            const size_t e = (size_t)b * nslot + slot;
#pragma unroll
            for (int k = 0; k < 5; ++k) part[k * plane + e] = acc[k];
            part[5 * plane + e] = peak;
        }
    }
}

// grid (rows of the batch): workgroup g serves the file of row r0 + g if that row is the file's first one INSIDE the batch (else it leaves at once), so every file the
// batch touches has exactly one workgroup.  It folds the file's rows of the batch, [r0 + g, min(end of the file, r0 + nb)): the partials lane-strided in ascending
// (row, slot) order in double, then a fixed tree over the 256 lanes (max for the peak), and
//     stats[f] = (the file's first row lies in this batch ? 0 : stats[f]) + that;     stats[f][0] = n_out, stats[f][7] = 0.
__global__ void __launch_bounds__(256)
pool_tail_kernel(const float* __restrict__ part, const size_t plane, const int nslot, const Tables tb, const long long r0, const int nb, const int L, const int ysz,
                 double* __restrict__ stats)
{
    __shared__ double red[POOL_PART][256];
    const int g = blockIdx.x, tid = threadIdx.x;
    const FileRow fr = file_of(tb, r0 + g);
    if (g > 0 && file_of(tb, r0 + g - 1).f == fr.f) return;
    long long last = fr.end < r0 + nb ? fr.end : r0 + nb;      // the row behind the file's last one in this batch
    const long long rows = last - (r0 + g) > 0 ? last - (r0 + g) : 0;
    const size_t e0 = (size_t)g * nslot, n = (size_t)rows * nslot;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    float pk = 0.f;
    for (size_t i = tid; i < n; i += 256) {
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] += (double)part[k * plane + e0 + i];
        pk = fmaxf(pk, part[5 * plane + e0 + i]);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) red[k][tid] = s[k];
    red[5][tid] = (double)pk;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int k = 0; k < 5; ++k) red[k][tid] += red[k][tid + o];
            red[5][tid] = fmax(red[5][tid], red[5][tid + o]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool first = fr.first >= r0;      // the file's first row lies in this batch: its statistics start here
        double* st = stats + (size_t)fr.f * POOL_STATS;
        const long long n_out = fr.len - (L - ysz);
        st[0] = (double)(n_out > 0 ? n_out : 0);
        st[1] = (first ? 0.0 : st[1]) + red[0][0];
        st[2] = (first ? 0.0 : st[2]) + red[1][0];
        st[3] = (first ? 0.0 : st[3]) + red[2][0];
        st[4] = fmax(first ? 0.0 : st[4], red[5][0]);
        st[5] = (first ? 0.0 : st[5]) + red[3][0];
        st[6] = (first ? 0.0 : st[6]) + red[4][0];
        st[7] = 0.0;
    }
}

}  // namespace stq
