// st_render_pool.h -- the kernels of st_render_pool (gfx950): a folder of recordings, kept in HBM as one concatenated pool, WHOLE through an effect, one knob
// setting per file, in one call.
//
// Reference: gen_dataset.py renders a dataset this way (every file through the effect at one setting, the setting in the target's name); the device feeds keep
// such a folder as a pool (st_feed_files.h: pool_x, file_off, file_len), and the effect entries (st_compressor_4c, st_compressor, st_lowpass, st_echo,
// st_denoise_input) take rows of one common length.  Here the rows are ragged: file f is pool[file_off[f] .. + file_len[f]), any offset, any length.
//
// THE LAW.  With xe the float32 image of file f (ST_PCM_S16 converts as in st_file_feed) and kw = knobs_wc[f] (world coordinates, four floats per file),
// out[file_off[f] + n], n in [0, len), is bit for bit sample n of the effect's own entry on (xe, kw) with B = 1 and L = ysz = len (rounded up to the multiple
// the entry demands, zeros appended: every effect is causal, so the appended samples change nothing before them):
//   ST_FX_COMP4C / ST_FX_DECOMP4C   st_compressor_4c      ST_FX_COMP   st_compressor      ST_FX_LOWPASS   st_lowpass      ST_FX_ECHO   st_echo
//   ST_FX_DENOISE                   st_denoise_input(seed, first_file + f, xe, kw[0])
// The bits are the entries' because the code is: the window functions take a pointer and a length and chunk from the span's first sample.
//
// HOW IT RUNS.  The scratch holds [row_off int64 [nfiles + 1], padded to 64 floats | the rows]: row f has round_up(len, 64) floats and starts at row_off[f], the
// prefix sum render_rows_kernel builds on the device from the clamped lengths.
//   render_rows_kernel     one workgroup: the prefix sums.
//   render_stage_kernel    grid (file, 2048-sample tile): the pool at any offset in either format (stq::file_quad) -> the row, as samples (COMP, LOWPASS, ECHO)
//                          or as the static gain curve with g[0] = 0 (COMP4C, DECOMP4C; zeros behind the file's end).
//   render_scan_kernel     COMP / LOWPASS: one workgroup per file calls env_compressor_window / lowpass_window on (row, len), storing at out + file_off.
//   render_echo_kernel     grid (file, tile): echo_window, as echo_kernel.
//   render_smooth_kernel   COMP4C / DECOMP4C: comp_smooth_kernel's chain with a base and a length per lane -- one LANE per file, 64 files per wave, [64 files][64
//                          samples] tiles through LDS, the same step arithmetic.  A row past its end loads zeros and stores nothing; the wave runs to the longest of
//                          its 64 rows.  No first-sample case: the stage kernel wrote gain 0 there, which leaves the state at 0 and puts out 0 (st_feed_stream.h).
//   render_apply_kernel    grid (file, tile): dB -> linear on the smoothed gain times the pool's sample (comp_apply_kernel's arithmetic).
//   render_denoise_kernel  grid (file, tile): denoise_add4 from the pool to out, no scratch.
// The chain is the cost: sequential per file, so a pool of a few long files keeps a few lanes busy for len steps each.
//
// Addresses.  render_span() is stq::file_span's clamp (off to [0, pool_samples], len to [0, pool_samples - off]) and len to max_len on top, so whatever the tables
// hold every address formed lies inside [0, pool_samples) of the pool and of out.  The rows of the scratch are sized by the size function from the HOST lengths:
// the device lengths must not exceed them.  A quad is one 16-byte access (int16: 8-byte) only where its address is aligned and it lies wholly inside the file.
// No float atomics: a repeated call repeats its bits.
#pragma once
#include "st_eval_pool.h"
#include "st_feed.h"
#include "st_filter.h"
#include "st_echo.h"

namespace str {

constexpr int TILE = 2048;      // samples per workgroup and trip of the tiled kernels: 256 lanes x 2 quads

struct Pool {
    const void* pool; const long long *file_off, *file_len;      // device tables [nfiles]
    int nfiles; long long pool_samples, max_len;
    const float* kw;                                              // [nfiles][4] world knobs
    long long* row_off;                                           // [nfiles + 1], in the scratch
    float* rows;                                                  // the rows, 16-byte aligned
    float* out;
};

__device__ __forceinline__ void render_span(const Pool& p, const int f, long long& off, long long& len)
{
    const stq::Tables t{p.file_off, p.file_len, nullptr, p.nfiles, p.pool_samples};
    stq::file_span(t, f, off, len);
    len = len > p.max_len ? p.max_len : len;
}
__device__ __forceinline__ long long row_len(const long long len) { return (len + 63) & ~63LL; }

// row_off[f] = sum of row_len over the files before f, row_off[nfiles] the total.  One 256-thread workgroup: a contiguous run of files per thread.
__global__ void __launch_bounds__(256)
render_rows_kernel(const Pool p)
{
    __shared__ long long part[256];
    const int t = threadIdx.x;
    const long long per = ((long long)p.nfiles + 255) / 256;
    const long long f0 = t * per < p.nfiles ? t * per : p.nfiles, f1 = (t + 1) * per < p.nfiles ? (t + 1) * per : p.nfiles;
    long long s = 0;
    for (long long f = f0; f < f1; ++f) { long long off, len; render_span(p, (int)f, off, len); s += row_len(len); }
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        long long acc = 0;
        for (int i = 0; i < 256; ++i) { const long long v = part[i]; part[i] = acc; acc += v; }
    }
    __syncthreads();
    long long o = part[t];
    for (long long f = f0; f < f1; ++f) { long long off, len; render_span(p, (int)f, off, len); p.row_off[f] = o; o += row_len(len); }
    if (t == 255) p.row_off[p.nfiles] = o;
}

// grid (file, tile): the file's row of the scratch.  GAIN: the static gain curve of the sample (kw[0] threshold, kw[1] ratio), 0 at sample 0 and behind the end.
template <typename T, bool GAIN>
__global__ void __launch_bounds__(256)
render_stage_kernel(const Pool p)
{
    const int f = blockIdx.x;
    long long off, len; render_span(p, f, off, len);
    const long long rl = row_len(len);
    const T* __restrict__ pool = reinterpret_cast<const T*>(p.pool);
    float* __restrict__ row = p.rows + p.row_off[f];
    const float th = GAIN ? p.kw[4 * (size_t)f] : 0.f, ra = GAIN ? p.kw[4 * (size_t)f + 1] : 1.f;
    for (long long t0 = (long long)blockIdx.y * TILE; t0 < rl; t0 += (long long)gridDim.y * TILE) {
        float4 v[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const long long g = t0 + 4 * (k * 256 + (int)threadIdx.x);
            v[k] = g < len ? stq::file_quad(pool, off, g, len) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const long long g = t0 + 4 * (k * 256 + (int)threadIdx.x);
            if (g >= rl) continue;
            float4 w = v[k];
            if (GAIN) {
                w = stf::comp_gain_curve4(w, th, ra);
                if (g == 0) w.x = 0.f;                               // lin_A[0] = 0 at the file's first sample
                if (g + 0 >= len) w.x = 0.f;
                if (g + 1 >= len) w.y = 0.f;
                if (g + 2 >= len) w.z = 0.f;
                if (g + 3 >= len) w.w = 0.f;
            }
            *reinterpret_cast<float4*>(row + g) = w;
        }
    }
}

// ST_FX_COMP / ST_FX_LOWPASS: one workgroup per file, the entries' window functions on (row, len); the result goes straight to out + file_off
template <int FX>
__global__ void __launch_bounds__(256)
render_scan_kernel(const Pool p, const float sr)
{
    __shared__ std::conditional_t<FX == ST_FX_COMP, stm::EnvLds, stm::LpLds> s;
    const int f = blockIdx.x;
    long long off, len; render_span(p, f, off, len);
    if (len <= 0) return;
    const float* __restrict__ xb = p.rows + p.row_off[f];
    float* __restrict__ yb = p.out + off;
    const float* kw = p.kw + 4 * (size_t)f;
    if constexpr (FX == ST_FX_COMP)
        stm::env_compressor_window(xb, nullptr, yb, (double)kw[0], (double)kw[1], stm::env_coef((double)kw[2], (double)sr), (int)len, (int)len, &s);
    else
        stm::lowpass_window(xb, yb, stm::lowpass_coef((double)kw[0], (double)sr), (int)len, (int)len, &s);
}

// ST_FX_ECHO: grid (file, tile), echo_kernel's split of the samples over blockIdx.y
__global__ void __launch_bounds__(256)
render_echo_kernel(const Pool p)
{
    __shared__ stm::EchoLds s;
    const int f = blockIdx.x;
    long long off, len; render_span(p, f, off, len);
    if ((long long)blockIdx.y * 256 >= len) return;                  // workgroup-uniform
    const float* kw = p.kw + 4 * (size_t)f;
    stm::echo_window(p.rows + p.row_off[f], p.out + off, kw[0], kw[1], kw[2], (int)len, (int)len, (int)blockIdx.y * 256, (int)gridDim.y * 256, &s);
}

// ST_FX_COMP4C / ST_FX_DECOMP4C: the attack / release chain over the rows' gain curves, in place.  One wave per 64 files, lane = file.
__global__ void __launch_bounds__(64)
render_smooth_kernel(const Pool p, const float sr)
{
    __shared__ float tile[64][65];
    const int lane = threadIdx.x, b0 = blockIdx.x * 64, b = b0 + lane;
    const int q = lane >> 4, c4 = 4 * (lane & 15);
    // the 16 rows this lane moves (4 i + q): base and length
    long long rb[16]; int rn[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = b0 + 4 * i + q;
        long long off, len = 0;
        if (r < p.nfiles) render_span(p, r, off, len);
        rb[i] = r < p.nfiles ? p.row_off[r] : 0; rn[i] = (int)row_len(len);
    }
    int c_end = 0;                                                    // the longest row of the wave
    {
        long long off, len = 0;
        if (b < p.nfiles) render_span(p, b, off, len);
        c_end = (int)row_len(len);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const int v = __shfl_xor(c_end, o); c_end = v > c_end ? v : c_end; }
    }
    const int bc = b < p.nfiles ? b : p.nfiles - 1;
    const double alphaA = exp(-log(9.0) / ((double)sr * (double)p.kw[4 * (size_t)bc + 2]));
    const double alphaR = exp(-log(9.0) / ((double)sr * (double)p.kw[4 * (size_t)bc + 3]));
    float prev = 0.f;
    float4 nx[16];                                         // the next tile, loaded while this one's chain runs
    auto load = [&](const int c0) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            nx[i] = c0 < rn[i] ? *reinterpret_cast<const float4*>(p.rows + rb[i] + c0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    load(0);
    for (int c0 = 0; c0 < c_end; c0 += 64) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = 4 * i + q;
            tile[r][c4] = nx[i].x; tile[r][c4 + 1] = nx[i].y; tile[r][c4 + 2] = nx[i].z; tile[r][c4 + 3] = nx[i].w;
        }
        __syncthreads();
        load(c0 + 64 < c_end ? c0 + 64 : c0);
        float gv[64];
#pragma unroll
        for (int k = 0; k < 64; ++k) gv[k] = tile[lane][k];
#pragma unroll
        for (int k = 0; k < 64; ++k) {                      // no first-sample case: the stage kernel wrote gain 0 there, which leaves prev = 0 and puts out 0
            const float gi_f = gv[k];
            const double a = gi_f < prev ? alphaA : alphaR;
            const double gi = gi_f;
            prev = (float)__builtin_fma(a, (double)prev - gi, gi);
            gv[k] = prev;
        }
#pragma unroll
        for (int k = 0; k < 64; ++k) tile[lane][k] = gv[k];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) {                      // smoothed gain back in place, coalesced rows
            const int r = 4 * i + q;
            if (c0 < rn[i]) *reinterpret_cast<float4*>(p.rows + rb[i] + c0 + c4) = make_float4(tile[r][c4], tile[r][c4 + 1], tile[r][c4 + 2], tile[r][c4 + 3]);
        }
        __syncthreads();
    }
}

// grid (file, tile): out = 10^(g / 20) * x over the whole file (comp_apply_kernel's arithmetic), x from the pool
template <typename T>
__global__ void __launch_bounds__(256)
render_apply_kernel(const Pool p)
{
    const int f = blockIdx.x;
    long long off, len; render_span(p, f, off, len);
    const T* __restrict__ pool = reinterpret_cast<const T*>(p.pool);
    const float* __restrict__ row = p.rows + p.row_off[f];
    const bool aligned = (off & 3) == 0;
    for (long long t0 = (long long)blockIdx.y * TILE; t0 < len; t0 += (long long)gridDim.y * TILE) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const long long g = t0 + 4 * (k * 256 + (int)threadIdx.x);
            if (g >= len) continue;
            const float4 x = stq::file_quad(pool, off, g, len), gq = *reinterpret_cast<const float4*>(row + g);      // the row is padded to 64 samples
            const float r[4] = {stm::comp_db_to_lin(gq.x) * x.x, stm::comp_db_to_lin(gq.y) * x.y, stm::comp_db_to_lin(gq.z) * x.z, stm::comp_db_to_lin(gq.w) * x.w};
            stp::store_quad_upto(p.out + off, r, g, len, aligned);
        }
    }
}

// ST_FX_DENOISE: grid (file, tile): file f is window first + f of the noise stream `seed`, kw[0] the strength
template <typename T>
__global__ void __launch_bounds__(256)
render_denoise_kernel(const Pool p, const unsigned seed, const unsigned long long first)
{
    const int f = blockIdx.x;
    long long off, len; render_span(p, f, off, len);
    const T* __restrict__ pool = reinterpret_cast<const T*>(p.pool);
    const unsigned key = stf::feed_key(seed, first + (unsigned long long)f);
    const float sgth = p.kw[4 * (size_t)f];
    const bool aligned = (off & 3) == 0;
    for (long long t0 = (long long)blockIdx.y * TILE; t0 < len; t0 += (long long)gridDim.y * TILE) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const long long g = t0 + 4 * (k * 256 + (int)threadIdx.x);
            if (g >= len) continue;
            const float4 v = stf::denoise_add4(key, (unsigned)g, sgth, stq::file_quad(pool, off, g, len));
            const float r[4] = {v.x, v.y, v.z, v.w};
            stp::store_quad_upto(p.out + off, r, g, len, aligned);
        }
    }
}

}  // namespace str
