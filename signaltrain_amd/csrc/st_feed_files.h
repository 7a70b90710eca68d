// st_feed_files.h -- the training feed of RECORDED input / target pairs as ONE kernel per minibatch (gfx950): st_file_feed.
//
// Reference: datasets.py:225-253 (AudioFileDataSet.get_single_chunk: a file chosen uniformly over the files, a window start chosen with
// np.random.randint(0, len - chunk_size), the target cropped to its last y_size samples, the file's knob settings, random polarity flip of the
// pair :27-29).  The audio of all files lies concatenated in HBM (`pool_x`, `pool_y`: float32, or the int16 the wav files hold), file f at
// samples [file_off[f], file_off[f] + file_len[f]).  One launch cuts B windows out of it; window b of the launch is window w = first_window + b of
// the stream `seed`, a function of (seed, w) only -- no state, no host RNG, any batching, reproducible per window.
//
// THE DRAW LAW (integer arithmetic only; datasets.file_feed_draw is its host replica):
//   key     = feed_key(seed, w)                                        (st_feed.h: the window key of every feed of this library)
//   h_i     = mix32(key + 0x9E3779B9 * i)   (mod 2^32), i = 1, 2, 3    (Draw::h(): the i-th 32-bit hash of the window's sequential stream)
//   (file, start, flipped) = feed_span(h_1, h_2, h_3, ...)             (below: THE SPAN CHOICE of every feed of recorded input; h_3 is drawn either way)
// Outputs: x [B][L] = pool_x[off + start .. + L), y [B][ysz] = the last ysz samples of the same span of pool_y, both times -1 where flipped;
// knobs [B][K] = row `file` of file_knobs; meta [B][3] = (file, start, flipped).
// ST_PCM_S16 converts a sample s as audio.read_audio_file does, (float)((double)s / 32767.0).  The float32 division (float)s / 32767.0f is
// correctly rounded and gives the same float for every int16 s (checked exhaustively by tests/test_file_feed_host.py: the double quotient
// never sits close enough to a float32 tie for the second rounding to matter), so that is what the kernel evaluates.
//
// The kernel is a pure HBM mover: grid (segments of x + segments of y, B), 256 lanes, FILE_TRIPS quads of 4 samples per lane -- a workgroup
// moves up to FILE_SEG = 2048 samples (8 KB out), whatever L: 1280 workgroups at B = 256, L = 8192, ysz = 2048; 40 per window at L = 65536.
// Destination rows are 16-byte aligned (L % 4 == ysz % 4 == 0, hipMalloc'ed bases): 16-byte stores.  A source span starts at ANY sample, so the
// loads go through vector types DECLARED with the element's alignment (f32x4_a4: 16 bytes aligned 4; s16x4_a2: 8 bytes aligned 2) -- never a
// float4 / short4 pointer at an address below its alignment.  All of a lane's loads are issued before its first store.
// Addresses: feed_span's clamps (below) keep every address formed inside [0, pool_samples), whatever the tables say.
#pragma once
#include "st_feed.h"

namespace stf {

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef short s16x4_a2 __attribute__((ext_vector_type(4), aligned(2)));
constexpr int FILE_TRIPS = 2, FILE_SEG = 256 * 4 * FILE_TRIPS;

struct FileFeedArgs {
    const void* pool_x; const void* pool_y;
    const long long* file_off; const long long* file_len; const float* file_knobs;
    float* x; float* y; float* knobs; long long* meta;
    long long pool_samples;
    unsigned seed; unsigned long long first;
    int L, ysz, K, nfiles, augment, nsx;        // nsx: segments of x per window (the y segments follow in blockIdx.x)
};

__device__ __forceinline__ float4 file_quad(const float* p) { const f32x4_a4 v = *reinterpret_cast<const f32x4_a4*>(p); return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ float4 file_quad(const short* p)
{
    const s16x4_a2 v = *reinterpret_cast<const s16x4_a2*>(p);
    return make_float4((float)v.x / 32767.0f, (float)v.y / 32767.0f, (float)v.z / 32767.0f, (float)v.w / 32767.0f);
}

// THE SPAN CHOICE of every feed of recorded input (file_feed_kernel, live_feed_kernel, stream_feed_kernel), from three 32-bit hashes of the window:
//   file    = (uint64(h_file) * nfiles) >> 32                          in [0, nfiles): uniform over files, not weighted by length
//   start   = (uint64(h_start) * (file_len[file] - L)) >> 32           in [0, len - L): the last position is excluded, as np.random.randint excludes it
//   flipped = augment ? h_flip >> 31 : 0
// A bounded draw ((uint64)h * n) >> 32 reaches every value below n <= 2^31 - 1 (n <= 2^32 values spread over 2^32 hashes), so every start of
// a file of up to 2^31 - 1 samples can occur; a float32-scaled draw cannot place a start on an odd sample beyond 2^24.
// Addresses: file < nfiles by construction; len - L is clamped to [1, 2^31 - 1] and base = off + start to [0, pool_samples - L], so whatever the tables
// say, every address of the span [base, base + L) lies inside [0, pool_samples) (the entries refuse pool_samples <= L).  Truthful tables are never clamped.
struct FeedSpan { int f; long long base; bool flip; };      // base: the span's first sample in the pool; start = base - file_off[f]
__device__ __forceinline__ FeedSpan feed_span(const unsigned h_file, const unsigned h_start, const unsigned h_flip, const long long* file_off, const long long* file_len,
                                              const int nfiles, const int L, const long long pool_samples, const int augment)
{
    const int f = below(h_file, nfiles);
    long long n = file_len[f] - (long long)L;
    n = n < 1 ? 1 : (n > 0x7fffffffLL ? 0x7fffffffLL : n);
    long long base = file_off[f] + (long long)(((unsigned long long)h_start * (unsigned long long)n) >> 32);
    const long long top = pool_samples - (long long)L;
    base = base < 0 ? 0 : (base > top ? top : base);
    return {f, base, augment && (h_flip >> 31)};
}

// THE WINDOW LOADER: TRIPS quads of 4 samples per lane, quad t of a lane at sample quad_at(i0, t) of a span of len samples (len % 4 == 0: a quad lies
// inside the span or outside it).  The loads are unconditional -- a quad past the end re-reads the span's last one -- so no branch stands between them,
// and the caller stores only after the call: all of a lane's loads are issued before its first store.
__device__ __forceinline__ unsigned quad_at(const unsigned i0, const int t) { return i0 + 4u * (t * 256 + threadIdx.x); }
template <int TRIPS, typename T>
__device__ __forceinline__ void load_quads(const T* __restrict__ src, const unsigned i0, const unsigned len, float4 (&q)[TRIPS])
{
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
        const unsigned i = quad_at(i0, t);
        q[t] = file_quad(src + (i < len ? i : len - 4u));
    }
}
__device__ __forceinline__ float4 quad_sign(const float4 v, const float sg) { return make_float4(v.x * sg, v.y * sg, v.z * sg, v.w * sg); }

template <typename T>
__global__ void __launch_bounds__(256)
file_feed_kernel(const FileFeedArgs a)
{
    const int b = blockIdx.y, L = a.L;
    const unsigned long long w = a.first + (unsigned long long)b;
    Draw d{feed_key(a.seed, w), 0u};
    const unsigned h1 = d.h(), h2 = d.h(), h3 = d.h();
    const auto [f, base, flip] = feed_span(h1, h2, h3, a.file_off, a.file_len, a.nfiles, L, a.pool_samples, a.augment);
    const float sg = flip ? -1.f : 1.f;

    const bool is_y = (int)blockIdx.x >= a.nsx;                          // workgroup-uniform
    const int seg = is_y ? (int)blockIdx.x - a.nsx : (int)blockIdx.x;
    const unsigned len = (unsigned)(is_y ? a.ysz : L);
    const T* __restrict__ src = reinterpret_cast<const T*>(is_y ? a.pool_y : a.pool_x) + base + (is_y ? L - a.ysz : 0);
    float* __restrict__ dst = is_y ? a.y + (size_t)b * a.ysz : a.x + (size_t)b * L;
    float4 v[FILE_TRIPS];
    load_quads<FILE_TRIPS>(src, (unsigned)seg * FILE_SEG, len, v);
#pragma unroll
    for (int t = 0; t < FILE_TRIPS; ++t) {
        const unsigned i = quad_at((unsigned)seg * FILE_SEG, t);
        if (i < len) *reinterpret_cast<float4*>(dst + i) = quad_sign(v[t], sg);
    }
    if (blockIdx.x == 0) {
        if ((int)threadIdx.x < a.K) a.knobs[(size_t)b * a.K + threadIdx.x] = a.file_knobs[(size_t)f * a.K + threadIdx.x];
        if (a.meta && threadIdx.x == 64) {
            long long* m = a.meta + (size_t)b * 3;
            m[0] = f; m[1] = base - a.file_off[f]; m[2] = flip ? 1 : 0;
        }
    }
}

}  // namespace stf
