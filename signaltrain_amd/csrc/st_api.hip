// st_api.hip -- extern "C" entry points of libsignaltrain_hip.so (see include/signaltrain_hip.h).
// All device work is launched on the caller's stream; no allocation, no synchronisation.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <mutex>
#include <set>
#include <type_traits>
#include <utility>
#include "st_common.h"
#include "st_gemm.h"
#include "st_gemm_planes.h"
#include "st_gemm_tn.h"
#include "st_gemm16.h"
#include "st_misc.h"
#include "st_ae.h"
#include "st_ae_wide.h"
#include "st_ae_split.h"
#include "st_ae32.h"
#include "st_dp.h"
#include "st_feed.h"
#include "st_feed_files.h"
#include "st_feed_live.h"
#include "st_feed_stream.h"
#include "st_predict.h"
#include "st_predict_stream.h"
#include "st_eval_pool.h"
#include "st_render_pool.h"
#include "st_decode.h"
#include "st_fit.h"
#include "st_multi.h"

// ------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
int st_fail(int code, const char* fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
    return code;
}
int st_check_launch(const char* what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return st_fail(ST_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return ST_OK;
}
static void prof_mark(const char* name, void* stream);
#define ST_LAUNCHED(what) do { int rc_ = st_check_launch(what); if (rc_ != ST_OK) return rc_; prof_mark(what, stream); } while (0)
#define ST_TRY(x) do { int rc_ = (x); if (rc_ != ST_OK) return rc_; } while (0)
#define ST_REQ(cond, ...) do { if (!(cond)) return st_fail(ST_ERR_ARG, __VA_ARGS__); } while (0)

extern "C" const char* st_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------ optional event profiling
// Off by default (zero overhead).  When enabled, every kernel launch of the library is followed by a
// hipEventRecord on the launch stream; st_profile_report() turns consecutive events into per-kernel
// durations.  Used by bench.py's roofline leg only -- never inside the timed region.
#define ST_PROF_MAX 4096
static bool g_prof = false;
static int g_prof_n = 0;
static hipEvent_t g_prof_ev[ST_PROF_MAX];
static const char* g_prof_name[ST_PROF_MAX];
static bool g_prof_init = false;
static void prof_mark(const char* name, void* stream)
{
    if (!g_prof || g_prof_n >= ST_PROF_MAX) return;
    (void)hipEventRecord(g_prof_ev[g_prof_n], st_stream(stream));
    g_prof_name[g_prof_n++] = name;
}
extern "C" int st_profile_enable(int on)
{
    if (on && !g_prof_init) {
        for (int i = 0; i < ST_PROF_MAX; ++i)
            if (hipEventCreate(&g_prof_ev[i]) != hipSuccess) return st_fail(ST_ERR_LAUNCH, "hipEventCreate");
        g_prof_init = true;
    }
    g_prof = on != 0; g_prof_n = 0;
    return ST_OK;
}
// Writes "name total_ms count\n" lines (aggregated by kernel name) into buf; caller must have synchronised the stream.
extern "C" int st_profile_report(char* buf, int buflen)
{
    if (!buf || buflen <= 0) return st_fail(ST_ERR_ARG, "st_profile_report: bad buffer");
    const char* names[64]; double tot[64]; int cnt[64]; int nn = 0;
    for (int i = 1; i < g_prof_n; ++i) {
        if (!strcmp(g_prof_name[i], "begin")) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_prof_ev[i - 1], g_prof_ev[i]) != hipSuccess) continue;
        int k = 0; for (; k < nn; ++k) if (!strcmp(names[k], g_prof_name[i])) break;
        if (k == nn) { if (nn == 64) continue; names[nn] = g_prof_name[i]; tot[nn] = 0; cnt[nn] = 0; ++nn; }
        tot[k] += ms; cnt[k]++;
    }
    int off = 0; buf[0] = 0;
    for (int k = 0; k < nn; ++k) off += snprintf(buf + off, off < buflen ? buflen - off : 0, "%s %.6f %d\n", names[k], tot[k], cnt[k]);
    g_prof_n = 0;
    return ST_OK;
}
extern "C" int st_version(void) { return 100; }
extern "C" int st_kp(int F) { return st_kp_of(F); }

// ------------------------------------------------------------------------------ geometry / layout
extern "C" int st_geometry(double scale_factor, double shrink_factor, int legacy, int K, int B, st_dims* o)
{
    ST_REQ(o && scale_factor > 0 && shrink_factor > 0, "st_geometry: bad arguments");
    const int chunk = (int)(8192 * scale_factor);              // nn_proc.py:357
    const int out_chunk = (int)(chunk / shrink_factor);        // nn_proc.py:358
    int ft = 1024, hop = 384;                                  // nn_proc.py:370-371
    if (legacy) { ft = (int)(ft * scale_factor); hop = (int)(hop * scale_factor); }   // nn_proc.py:374-376
    o->B = B; o->L = chunk; o->N = ft; o->H = hop; o->K = K;
    o->T = (int)(ceil(chunk / (double)hop) + ceil(ft / (double)hop));                 // nn_proc.py:378
    o->OT = (int)(ceil(out_chunk / (double)hop) + ceil(ft / (double)hop));            // nn_proc.py:379
    o->y = (o->OT - 1) * hop - ft;                                                    // nn_proc.py:380
    o->F = ft / 2 + 1;
    return ST_OK;
}

static int check_dims(const st_dims* d)
{
    ST_REQ(d, "null dims");
    ST_REQ(d->B > 0 && d->L > 0 && d->N > 0 && d->H > 0 && d->T > 0 && d->OT > 0 && d->K >= 0, "non-positive dimension");
    ST_REQ(d->F == d->N / 2 + 1, "F must be N/2+1");
    ST_REQ(d->N % 32 == 0 && d->H % 4 == 0 && d->L % 4 == 0 && d->y % 4 == 0, "N%%32, H%%4, L%%4, y%%4 required");
    ST_REQ(d->y == (d->OT - 1) * d->H - d->N && d->y > 0 && d->y <= d->L, "y must equal (OT-1)*H-N");
    ST_REQ(d->OT <= d->T, "OT must be <= T");
    // the reference's Conv1d (padding N, stride H) yields (L + N) / H + 1 frames and its first Linear layer refuses any other count; here frame t starts
    // at sample H t - N, so a T with H T < L + N leaves out a frame that still overlaps the signal.  A larger T only adds all-padding frames (st_geometry
    // emits that: ceil(L / H) + ceil(N / H) frames), a frame starting exactly at L is dead and may be omitted.
    ST_REQ((long long)d->H * d->T >= (long long)d->L + d->N, "T too small: H*T >= L+N required, or a frame overlapping the signal is dropped (T=%d L=%d N=%d H=%d)",
           d->T, d->L, d->N, d->H);
    ST_REQ(d->K <= 16, "at most 16 knobs");
    ST_REQ(d->prec >= ST_PREC_F32 && d->prec <= ST_PREC_F32X3, "st_dims.prec = %d is not an ST_PREC_* level", d->prec);
    ST_REQ(d->loss_scale >= 0.f && d->loss_scale <= 3.0e38f, "st_dims.loss_scale must be 0 (none) or a positive finite scale");
    // the kernels address every operand with 32-bit element offsets from a wave-uniform base and index rows with 24-bit
    // multiplies: rows (B*T) < 2^24, the largest per-batch operands (B*T x KP spectra, B x (L + 2N) padded signals) < 2^30 elements
    ST_REQ((size_t)d->B * d->T < ((size_t)1 << 24) && (size_t)d->B * d->T * st_kp_of(d->F) < ((size_t)1 << 30) &&
           (size_t)d->B * ((size_t)d->L + 2 * (size_t)d->N) < ((size_t)1 << 30), "batch too large for 32-bit element offsets (B=%d)", d->B);
    // ... and split a compact row r < B*T into (window, frame) with a multiply-high by floor(2^32 / Tv) + 1, Tv <= T (st_gemm.h RowMap::split): exact while
    // r * T < 2^32; the largest row decides (st_fe_supported has the same rule for the generic front end)
    ST_REQ(((unsigned long long)d->B * d->T - 1) * (unsigned long long)d->T < (1ull << 32), "row split inexact: (B*T - 1)*T must stay below 2^32 (B=%d T=%d)", d->B, d->T);
    return ST_OK;
}

static void ae_shapes(const st_dims* d, int* out, int* in)
{
    const sta::AEShape sh{d->T, d->OT, d->K};      // the layer table of st_ae.h
    for (int l = 0; l < sta::NL; ++l) { out[l] = sh.out(l); in[l] = sh.in(l); }
}

static int64_t param_offsets(const st_dims* d, int64_t* offs)
{
    int64_t off = 0; int n = 0;
    auto put = [&](int64_t sz) { if (offs) offs[n] = off; ++n; off += (sz + 3) / 4 * 4; };
    for (int s = 0; s < 4; ++s) put((int64_t)d->N * d->N);
    int out[9], in[9]; ae_shapes(d, out, in);
    for (int a = 0; a < 2; ++a)
        for (int l = 0; l < 9; ++l) { put((int64_t)out[l] * in[l]); put(out[l]); }
    return off;
}
extern "C" int64_t st_param_offsets(const st_dims* d, int64_t* offs) { return check_dims(d) != ST_OK ? -1 : param_offsets(d, offs); }

struct Layout {            // everything derived from dims that the host side needs
    int64_t offs[40]; int64_t total; int64_t n_stft; int PG; sta::AEOffsets go; int KP;
};
static int make_layout(const st_dims* d, Layout* L)
{
    ST_TRY(check_dims(d));
    L->total = param_offsets(d, L->offs);
    L->n_stft = L->offs[4];
    L->PG = (int)(L->offs[22] - L->offs[4]);
    for (int l = 0; l < 9; ++l) {
        L->go.w[l] = (int)(L->offs[4 + 2 * l] - L->offs[4]);
        L->go.b[l] = (int)(L->offs[5 + 2 * l] - L->offs[4]);
    }
    L->KP = st_kp_of(d->F);
    return ST_OK;
}

// ------------------------------------------------------------------------------ launch parameters
static int num_cus()
{
    static int n = 0;
    if (!n) { int dev = 0; (void)hipGetDevice(&dev); hipDeviceProp_t p; if (hipGetDeviceProperties(&p, dev) == hipSuccess) n = p.multiProcessorCount; if (n <= 0) n = 256; }
    return n;
}
// The product library has no run-time ablations: a timing-only ablation exists only as a -D constant the Makefile never sets (ST_GEMM_ABLATE, ST_AE_ABLATE,
// ST_PL_ABLATE, ST_G128_ABLATE).  The entry stays for callers that pass their --ablate argument through; it accepts 0 alone.
extern "C" int st_set_debug(int v) { return v == 0 ? ST_OK : st_fail(ST_ERR_ARG, "st_set_debug(%d): the product library has no run-time ablations (build with -DST_*_ABLATE=bits)", v); }
static int g_dp_inline = 1;  // st_dp_train_step: 1 = the last (exposed) exchange is issued in line on the compute stream (round 6), 0 = on the communicator stream between two hand-offs
static int g_ae_save = 1;    // fused geometries, fp32 autoencoder layers: 1 = the forward kernel keeps the activations and the backward reads them (round 6), 0 = the backward recomputes them;
                             // 2 = as 1, with the LDS weight images built inside the kernels instead of once per step by prep_kernel (round 10: A/B timing, bit-equality tests)
static int g_ae_split = -1;  // autoencoder backward of the fused geometries: 0 = the single kernel, 1 = the two kernels of st_ae_split.h,
                             // -1 = by precision (default): fp32 -> single (179.5 us against 87.0 + 92.4 us at B = 256 -- equal: the fp32 MFMA holds the vector ALUs, a partner
                             // wave has nothing to overlap with -- and the split moves 66 MB more per step: h4 / d a4 / tails hand-over); 16-bit Linear layers -> split (the
                             // matrix pipe is then a separate unit and two waves per SIMD overlap it with the ELU / conversion / transpose work: 102 -> 48 + 44 us at
                             // B = 256, 354 -> 152 + 138 us at B = 1024, bf16_all)
static int g_ae32 = 1;       // 16-bit autoencoder forward of the fused geometries on 32-row groups / v_mfma_f32_32x32x16 (st_ae32.h); 0 = the 16-row kernel of st_ae.h
static int g_pl_bf16 = 0;    // ST_PREC_BF16*: analysis / frames GEMMs on the plane kernel with ONE plane (bf16 copies of the bases, k-chunk-major).  MEASURED SLOWER at B = 256
                             // (analysis 53.8 vs 49.8 us + 12 us for the copies): three MFMAs per 16-deep k-tile and barrier; needs a 64-deep tile
static int g_wg_split = 0;   // ST_PREC_F32X3: weight-gradient GEMMs on the in-kernel three-plane split instead of the fp32 MFMA kernel (see wgrad_small_gemm)
static int g_pl_dgrad = 0;   // ST_PREC_F32X3: synthesis data gradient on the plane kernel (measured slower than the fp32 MFMA kernel at B = 256: 57 vs 45 us)
static int g_pl_shape = 3;   // analysis plane GEMM tile (ST_PREC_F32X3): 0 = 4 waves x (32 x 96) [91.9 us], 1 = 2 waves x (64 x 96) [117], 2 = 4 waves x (64 x 96) [112],
                             // 3 = 8 waves x (32 x 96) = 256 x 96, one workgroup per CU: a quarter less L2 traffic at the same two waves per SIMD [88.1]
static int g_g16 = 1;        // 16-bit configurations: the fused step's GEMMs on pre-rounded 16-bit operands (st_gemm16.h); 0 = gemm_half_kernel on fp32 operands
static int g_g16_dma = 0;    // bit 0 / bit 1: its analysis forward / synthesis data-gradient GEMM on the LDS-DMA kernel gemm16_nt256_kernel.  MEASURED EQUAL to
                             // gemm16_nt_kernel (analysis forward, bf16, B = 256 / 1024: 34.2 / 138.6 us against 35.5 / 137.2): both deliver ~20 B/clk/CU from L2 to LDS, see st_gemm16.h
static int g_nt128 = 1;      // fp32 synthesis frames / data-gradient GEMMs on the 128 x 128-tile NT kernel (st_gemm_tn.h); 0 = gemm_kernel<2, ...>
static int g_tn128 = 1;      // weight-gradient GEMMs on the 128 x 128-tile kernel (st_gemm_tn.h) where it applies; 0 = gemm_kernel<3, ...>; 2 = its round-3 k-tile loop;
                             // 1 (default) also runs the two GEMMs of the fp32 step as ONE launch (wgrad_pair); 3 = the pipelined loop, one launch per GEMM (A/B timing, bit-equality test)
static int g_tn_fm = 3;      // round 5: frame-major reduction order + per-tile-column row ranges (structural zeros skipped) in the 128 x 128 weight-gradient GEMMs: bit 0 synthesis
                             // (25 % of its reduction rows are cropped taps: 41.7 -> 37.0 us), bit 1 analysis (7.6 %: 113.8 -> 109.5 us)
static int g_g16_crop = 15;  // round 5, 16-bit operand pipeline: structural zeros skipped (frame-major rows): bit 0 frames GEMM (dead tile columns return), bit 1 data gradient (live taps per tile row),
                             // bit 2 / bit 3 synthesis / analysis weight gradient (reduction rows per tile column)
static int g_frs_nt = 1;     // synthesis frames GEMM against the transposed fold (both operands K-contiguous); 0 = the k-major form
static int g_xt = 0;       // 1: M/N-contiguous operands staged k-quad-major (st_gemm.h XT).  MEASURED SLOWER at B=256 although
                           // conflict-free with a third fewer LDS cycles: analysis wgrad 173 vs 145 us, synthesis frames 63 vs 60 us (16 more prefetch
                           // registers -> 4 instead of 4.5 waves per SIMD, and 16 v_mov per micro-tile): the k-major staging stays the default
static const int NORM_E_PARTIALS = 32;     // |g| partials of the autoencoder gradient range (st_dims.clip_all) when they come from l1_partial_kernel
static const int NORM_E_MAX = 4096;        // room for the per-block partials of the reducing kernels themselves (post_ae_kernel / wide_grad_finish_kernel)
static int g_wide_direct = 1; // wide geometries: the analysis epilogue writes the wide autoencoder path's feature-major input itself (no wide_in_kernel in the fused step); 0 = copy kernel
static int g_an_bk = 32;   // k-tile depth of the analysis forward GEMM (see stft_plan)
static int g_bk = 16;   // k-tile depth of the GEMM family (16: 36 KB LDS/WG -> 4 WGs/CU; 32: 64 KB -> 2 WGs/CU)
static int g_wg_mode = 0;    // weight-gradient GEMMs: 0 = three waves share a 96 x 96 tile (32 x 96 strips), 2 = the same on the k-quad-major staging (see g_xt)
// The diagnostic switches above as ONE readable state, in st_get_tuning's order, with their shipped defaults.  The product path never sets them;
// tests/conftest.py asserts after every test that the state is back at the defaults (a wrong default can then not ship unnoticed, and a test cannot
// leak a switch into the next one).
#define ST_TUNING_LIST(X) X(g_ae_split, -1) X(g_ae_save, 1) X(g_dp_inline, 1) X(g_pl_bf16, 0) X(g_wg_split, 0) X(g_pl_dgrad, 0) X(g_pl_shape, 3) X(g_g16, 1) X(g_g16_dma, 0) \
    X(g_nt128, 1) X(g_tn128, 1) X(g_frs_nt, 1) X(g_xt, 0) X(g_an_bk, 32) X(g_bk, 16) X(g_wg_mode, 0) X(g_ae32, 1) X(g_wide_direct, 1) X(g_tn_fm, 3) X(g_g16_crop, 15)
// ... and the WHOLE interface that sets them: code first + i (0 <= i < count) stores value + i into *var (and into *also, where given).  A code that is not
// listed here is an error and changes nothing.
static const struct { int first, count; int* var; int value; int* also; } k_tuning_codes[] = {
    {16, 1, &g_an_bk, 16, &g_bk}, {32, 1, &g_an_bk, 32, &g_bk},      // k-tile depth of the fp32 GEMM family
    {100, 1, &g_wg_mode, 0, nullptr}, {102, 1, &g_wg_mode, 2, nullptr},
    {7000, 2, &g_xt, 0, nullptr},
    {8000, 2, &g_ae_split, 0, nullptr}, {8002, 1, &g_ae_split, -1, nullptr},      // single kernel / two kernels / by precision
    {8100, 2, &g_ae32, 0, nullptr},
    {8200, 3, &g_ae_save, 0, nullptr},      // 8202: kept activations, in-kernel weight images
    {8300, 2, &g_dp_inline, 0, nullptr},
    {9000, 2, &g_frs_nt, 0, nullptr},
    {9100, 1, &g_pl_shape, 0, nullptr}, {9103, 1, &g_pl_shape, 3, nullptr},
    {9200, 2, &g_pl_dgrad, 0, nullptr},
    {9300, 2, &g_wg_split, 0, nullptr},
    {9400, 2, &g_pl_bf16, 0, nullptr},
    {9500, 2, &g_tn128, 0, nullptr}, {9580, 1, &g_tn128, 2, nullptr}, {9581, 1, &g_tn128, 1, nullptr},      // 9580: its round-3 k-tile loop (A/B timing, bit-equality test)
    {9582, 1, &g_tn128, 3, nullptr},      // the pipelined loop without the pair launch of the fp32 step: one launch per GEMM
    {9540, 4, &g_tn_fm, 0, nullptr},
    {9560, 16, &g_g16_crop, 0, nullptr},
    {9600, 2, &g_g16, 0, nullptr},
    {9690, 4, &g_g16_dma, 0, nullptr},
    {9950, 2, &g_nt128, 0, nullptr},
    {9970, 2, &g_wide_direct, 0, nullptr},
};
extern "C" int st_set_tuning(int code)
{
    for (const auto& t : k_tuning_codes)
        if (code >= t.first && code < t.first + t.count) { *t.var = t.value + (code - t.first); if (t.also) *t.also = *t.var; return ST_OK; }
    return st_fail(ST_ERR_ARG, "st_set_tuning(%d): no such code", code);
}
extern "C" int st_get_tuning(int* out, int n)
{
    int i = 0;
#define X(v_, d_) if (out && i < n) out[i] = v_; ++i;
    ST_TUNING_LIST(X)
#undef X
    return i;                      // number of switches (call with out = NULL to size the array)
}
extern "C" int st_tuning_defaults(int* out, int n)
{
    int i = 0;
#define X(v_, d_) if (out && i < n) out[i] = d_; ++i;
    ST_TUNING_LIST(X)
#undef X
    return i;
}
extern "C" int st_reset_tuning(void)
{
#define X(v_, d_) v_ = d_;
    ST_TUNING_LIST(X)
#undef X
    return ST_OK;
}
// Arithmetic of a call = st_dims::prec (ST_PREC_*; round 1 had a process-wide switch here, which raced between engines):
// half type (0 none / 1 bfloat16 / 2 float16) of the STFT GEMM operands and of the autoencoder layers.
// gemm_ht: 3 = fp32 operands as three bfloat16 planes (ST_PREC_F32X3; st_gemm.h gemm_half_kernel PL = 3)
static inline int gemm_ht(int prec) { return (prec == ST_PREC_BF16 || prec == ST_PREC_BF16_ALL) ? 1 : ((prec == ST_PREC_F16 || prec == ST_PREC_F16_ALL) ? 2 : (prec == ST_PREC_F32X3 ? 3 : 0)); }
static inline int ae_ht(int prec) { return prec == ST_PREC_BF16_ALL ? 1 : (prec == ST_PREC_F16_ALL ? 2 : 0); }
static inline float loss_scale_of(const st_dims* d) { return d->loss_scale > 0.f ? d->loss_scale : 1.0f; }
// The model's constants, each in ONE place: the L1 regulariser's weight of loss_functions.py:36 per element of mag_hat (reg_scale_of), the same times the loss scale
// as the backward kernels take it (reg_coef_of: (loss scale * c) / elements, in this order -- the fused tests compare bits), and the slope of its frequency weights
static inline float reg_scale_of(const st_dims* d) { return (float)(2e-5 / 10.0) / ((float)d->B * (float)d->OT * (float)d->F); }
static inline float reg_coef_of(const st_dims* d) { return loss_scale_of(d) * (float)(2e-5 / 10.0) / ((float)d->B * (float)d->OT * (float)d->F); }
static inline float expfac_of(const st_dims* d) { return (float)(7.0 / d->F); }
// Kernels with > 64 KB of dynamic LDS need the attribute once per (device, kernel); the result is checked (round 1 discarded
// it behind non-atomic flags: a failure surfaced later as an opaque launch error).
static int ensure_dyn_lds(const void* fn, const char* name)
{
    static std::mutex mu; static std::set<std::pair<int, const void*>> done;
    int dev = 0; (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({dev, fn})) return ST_OK;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return st_fail(ST_ERR_LAUNCH, "hipFuncSetAttribute(%s, 160 KB dynamic LDS): %s", name, hipGetErrorString(e));
    done.insert({dev, fn});
    return ST_OK;
}
// One launch of a kernel that may need more than 64 KB of dynamic LDS: the attribute (once per device and kernel), then the launch.  The arguments convert to
// the kernel's parameter types as in a plain call; ST_LAUNCHED("name") follows the launch, or the group of launches that shares one mark.
template <class... P, class... A>
static int launch_lds(const char* name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A&&... args)
{
    static_assert(sizeof...(P) == sizeof...(A), "launch_lds: argument count");
    ST_TRY(ensure_dyn_lds(reinterpret_cast<const void*>(kernel), name));
    hipLaunchKernelGGL(kernel, grid, block, lds, s, static_cast<P>(args)...);
    return ST_OK;
}
// From a run-time value to a template argument: f is a generic lambda that receives the value as a std::integral_constant (HT() is a constant expression) and is
// instantiated once per member of the set -- so a family that exists for a subset only is dispatched over that subset.  Each returns what f returns.
template <int V> using ic = std::integral_constant<int, V>;
template <class F> static inline auto with_ht(int ht, F&& f) { return ht == 1 ? f(ic<1>{}) : ht == 2 ? f(ic<2>{}) : f(ic<0>{}); }      // 0 fp32 / 1 bfloat16 / 2 float16
template <class F> static inline auto with_ht16(int ht, F&& f) { return ht == 2 ? f(ic<2>{}) : f(ic<1>{}); }                          // the two 16-bit levels
template <class F> static inline auto with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <class F> static inline auto with_var(int var, F&& f) { return with_ht(var, f); }                                        // ae_bwd_kernel's VAR: 0 / 1 / 2 as well (see ae_bwd_body)
template <class F> static inline auto with_fx(int effect, F&& f)                                                                  // a feed's ST_FX_* id (feed_effect_ok checked it before)
{
    return effect == ST_FX_COMP ? f(ic<ST_FX_COMP>{}) : effect == ST_FX_LOWPASS ? f(ic<ST_FX_LOWPASS>{}) : effect == ST_FX_DENOISE ? f(ic<ST_FX_DENOISE>{}) :
           effect == ST_FX_ECHO ? f(ic<ST_FX_ECHO>{}) : effect == ST_FX_DECOMP4C ? f(ic<ST_FX_DECOMP4C>{}) : f(ic<ST_FX_COMP4C>{});
}
template <class F> static inline auto with_pcm(int fmt, F&& f) { return fmt == ST_PCM_S16 ? f(short()) : f(float()); }              // a value of the pool's sample type: ST_PCM_S16 / ST_PCM_F32
template <class F> static inline auto with_slabs(int ns, F&& f) { return ns == 3 ? f(ic<3>{}) : ns == 2 ? f(ic<2>{}) : f(ic<1>{}); }   // 1..3 split-K slabs
static const int AE_FWD_NW = 8, AE_BWD_NW = 4;
template <class F> static inline auto with_fwd_nw(int nw, F&& f) { return nw == 11 ? f(ic<11>{}) : f(ic<AE_FWD_NW>{}); }                             // ae_fwd_nw: {8, 11}
template <class F> static inline auto with_inner_nw(int nw, F&& f) { return nw == 9 ? f(ic<9>{}) : nw == 12 ? f(ic<12>{}) : f(ic<AE_FWD_NW>{}); }   // ae_inner_nw: {8, 9, 12}
// The small-tile GEMM (st_gemm.h: W waves share a (32 W) x 96 tile) at the arithmetic of `prec`: the converting gemm_half_kernel for the 16-bit levels and for
// ST_PREC_F32X3 (its in-kernel three-plane split), else the fp32 MFMA kernel with bk-deep k-tiles (16: 36 KB LDS/WG -> 4 WGs/CU; 32: 64 KB -> 2 WGs/CU) on the
// k-major or (xt) k-quad-major staging.  Every launcher's return code is the function's.
template <int W, class AL, class BL, class EPI>
static int small_gemm(int prec, int bk, bool xt, const AL& al, const BL& bl, const EPI& ep, int M, int Nc, int K, int ns, hipStream_t s)
{
    const int ht = gemm_ht(prec);
    if (ht == 3) return stg::launch_half<W, 1, 3>(al, bl, ep, M, Nc, K, ns, s);
    if (ht != 0) return with_ht16(ht, [&](auto HT) { return stg::launch_half<W, HT()>(al, bl, ep, M, Nc, K, ns, s); });
    with_bool(xt, [&](auto XT) { if (bk == 16) stg::launch<W, 16, XT()>(al, bl, ep, M, Nc, K, ns, s); else stg::launch<W, 32, XT()>(al, bl, ep, M, Nc, K, ns, s); });
    return ST_OK;
}
// The 96 x 96 three-wave form of the weight-gradient GEMMs (WG_96).  ST_PREC_F32X3: they reduce along the ROWS of both operands (k-major staging, 4x4 register
// transposes); their in-kernel three-plane split measured slower than the fp32 MFMA kernel (176 vs 141 us, 62 vs 55 us at B = 256), so that precision level keeps
// them on the fp32 kernel (st_set_tuning(9301) selects the split form).
template <class AL, class BL, class EPI>
static int wgrad_small_gemm(int prec, const AL& al, const BL& bl, const EPI& ep, int M, int Nc, int K, int ns, hipStream_t s)
{
    const int ht = gemm_ht(prec);
    if (g_wg_mode == 2 && ht == 0) { stg::launch<3, 16, true>(al, bl, ep, M, Nc, K, ns, s); return ST_OK; }
    if (ht == 3 && !g_wg_split) { stg::launch<3, 16>(al, bl, ep, M, Nc, K, ns, s); return ST_OK; }
    return small_gemm<3>(prec, g_bk, g_xt != 0, al, bl, ep, M, Nc, K, ns, s);
}
static int synth_live_rows(const st_dims* d);
static bool ae_is_wide(const st_dims* d);
// Waves per workgroup of the fused forward kernel: 8, or 11 where that removes the tail round.  A wave walks whole 16-row groups,
// one workgroup per CU: at B = 256 there are 8448 = 256 * 33 groups -- 4.125 per wave with 8 waves (five rounds, the fifth 12 %
// full), exactly 3 per wave with 11 (2.75 waves per SIMD, the fp32 kernel's 152 registers allow 3).  Time goes with
// rounds x waves sharing a SIMD: 5 x 8 against 3 x 11.  The 16-bit instantiations (176 registers) stay at 8.
static int ae_fwd_groups(const st_dims* d) { return d->B * (st_kp_of(d->F) / 32); }
static int ae_fwd_nw(const st_dims* d)
{
    if (ae_is_wide(d) || ae_ht(d->prec) != 0) return AE_FWD_NW;
    const int groups = ae_fwd_groups(d), c = num_cus();
    auto cost = [&](int nw) { int grid = (groups + nw - 1) / nw; if (grid > c) grid = c; const int rounds = (groups + grid * nw - 1) / (grid * nw); return rounds * nw; };
    return cost(11) < cost(AE_FWD_NW) ? 11 : AE_FWD_NW;
}
// Wide path, layers 2..8 (ae_inner_fwd_kernel: 116-126 registers, up to four waves per SIMD): waves per workgroup out of {8, 9, 12} by
// rounds x waves sharing the busiest SIMD.  B = 64 at the 65536-sample window is 2112 = 256 * 8.25 groups: with 8 waves 64 of the 2048 waves walked a
// second group (two rounds for 3 % more work); 9 waves on 235 workgroups take one.
static int ae_inner_nw(const st_dims* d)
{
    const int groups = ae_fwd_groups(d), c = num_cus();
    int best = AE_FWD_NW, best_cost = 1 << 30;
    for (int nw : {8, 9, 12}) {
        int grid = (groups + nw - 1) / nw; if (grid > c) grid = c;
        const int rounds = (groups + grid * nw - 1) / (grid * nw), cost = rounds * ((nw + 3) / 4);
        if (cost < best_cost) { best_cost = cost; best = nw; }
    }
    return best;
}
static int ae_inner_grid(const st_dims* d) { const int nw = ae_inner_nw(d); int g = (ae_fwd_groups(d) + nw - 1) / nw; int c = num_cus(); return g < c ? g : c; }
static int ae_fwd_grid(const st_dims* d) { const int nw = ae_fwd_nw(d); int g = (ae_fwd_groups(d) + nw - 1) / nw; int c = num_cus(); return g < c ? g : c; }
static int ae_bwd_grid(const st_dims* d) { int groups = d->B * (st_kp_of(d->F) / 32); int g = (groups + AE_BWD_NW - 1) / AE_BWD_NW; int c = num_cus() / 2; if (c < 1) c = 1; return g < c ? g : c; }
// split-K factors.  fp32 MFMA tiles are long serial chains (48 MFMAs x 64 cycles per k-tile per wave), so a GEMM
// needs >= ~2 waves per SIMD (2048 waves) to overlap its load/LDS phases; the small-M synthesis GEMMs and the
// 121-tile weight-gradient GEMMs get there by splitting K and summing the slabs in the consumer kernel.
static const int WSPLIT_ROWS = 200, WSPLIT_MAX = 16;      // reduction rows per weight-gradient k-slice, and the cap of the slice count
static int wgrad_split(int R) { int s = R / WSPLIT_ROWS; if (s < 1) s = 1; if (s > WSPLIT_MAX) s = WSPLIT_MAX; return s; }
// The k-slice count of a weight-gradient GEMM: ONE function for the three kernel forms, each over the whole tensor (M = KP output rows) or over one basis of the
// analysis pair (M = KP / 2), so six rules side by side.  R: live reduction rows.  room: slabs the workspace area holds once its Nyquist partials are set aside
// (wgrad_area_slabs): no rule exceeds it.  The two whole-tensor fp32 rules are what the area is sized by (over all B * T frames, on the device's CU count), so
// there the cap binds only when a query assumes more CUs than the device has.  ncus > 0 makes the function pure given its arguments (the host queries);
// otherwise the current device's CU count.
enum { WG_TN128 = 0, WG_96 = 1, WG_TN16 = 2 };      // the 128 x 128 TN kernel (st_gemm_tn.h), the 96 x 96 three-wave kernel behind wgrad_small_gemm, the 16-bit TN kernel (st_gemm16.h)
static int wgrad_slices(int form, bool one_basis, int R, int KP, int N, int room, int ncus = 0)
{
    const int cus = ncus > 0 ? ncus : num_cus(), M = one_basis ? KP / 2 : KP;
    auto per_tiles = [](int n, int tiles) { return n / (tiles > 0 ? tiles : 1); };
    int s;
    if (form == WG_TN128) {
        // as many slices as fill the CUs with one workgroup each, never slices shorter than 64 reduction rows.  One basis: half the tiles, so each half
        // fills the chip with twice the k-slices of the whole-tensor launch and the two launches together do the work of the one
        s = per_tiles(cus, (one_basis ? (N / 2) / 128 : N / 128) * (N / 128)); if (s > 16) s = 16;
        if (s > R / 64) s = R / 64;
        if (one_basis && s > room) s = room;
    } else if (form == WG_TN16) {
        // about two workgroups per CU (their time is staging, not matrix work), never slices under 128 reduction rows, never more slabs than the workspace holds
        s = per_tiles(2 * cus, ((M + 127) / 128) * (N / 128));
        if (s > R / 128) s = R / 128;
        if (s > room) s = room;
    } else {
        // never more k-slices than keep all workgroups co-resident: the 3-wave weight-gradient workgroup (25 KB of LDS, 95 registers)
        // fits six to a CU, and a second, partly filled round costs more than the shorter k-chains save (measured sawtooth at B = 256,
        // 121 tiles: 10 / 12 / 16 slices -> 151 / 153 / 160 us incl. the slab reduce; 11, 13 -> 160, 169)
        s = wgrad_split(R);
        int fit = per_tiles(6 * cus, ((KP + 95) / 96) * ((N + 95) / 96)); if (fit < 1) fit = 1;
        if (fit >= 2) fit &= ~1;                       // even slice counts: odd ones leave a ragged last slice (k-slices are multiples of 32 rows)
        if (fit < s) s = fit;
        if (one_basis) {
            // One-basis GEMM: 6 x 11 tiles of 96 x 96, one 3-wave workgroup per CU at a time, so the run time goes with
            // ceil(tiles * ns / CUs) / ns (measured sawtooth, B=256: ns = 7, 11, 15 are the minima, 8 / 12 / 16 cost +40..60 us).
            // Pick the split in [ns/2, ns] that fills its last round best; never above the slab count the workspace holds.
            const int tiles = ((M + 95) / 96) * ((N + 95) / 96);
            int best = s; double bf = -1.0;
            for (int c = s; c >= (s + 1) / 2 && c >= 1; --c) {
                const int w = tiles * c, rounds = (w + cus - 1) / cus;
                const double f = (double)w / ((double)rounds * cus);
                if (f > bf + 1e-9) { bf = f; best = c; }
            }
            s = best;
        }
    }
    if (s > room) s = room;      // every form, whatever CU count is assumed: never more slabs than the workspace area holds
    return s < 1 ? 1 : s;
}
// The two synthesis GEMMs (frames, data gradient) over R live rows: from STFT_TALL_ROWS rows on, 4-wave tiles (128 rows) and the whole reduction in one slab
// fill the chip; below, 2-wave tiles (64 rows) and K split over 3 slabs (frames GEMM: 3, 4 measured equal, 6 slower -- only 66 k-tiles to split).  The consumers
// (ola_loss_kernel, ae_bwd_kernel: with_slabs) sum at most 3 slabs; the workspace (carve) holds as many as this rule says, for every operand family.
static const int STFT_TALL_ROWS = 4096;
struct SynthTile { int waves, ns; };
static SynthTile synth_tile(int R) { return R >= STFT_TALL_ROWS ? SynthTile{4, 1} : SynthTile{2, 3}; }

// Sizes for internal code, which holds checked dims; the extern "C" functions of these names ask check_dims first
// (the host size functions answer 0 for dims outside the supported family, with the rule in st_last_error(): check_dims)
static int ae_fwd_partials(const st_dims* d) { return ae_fwd_grid(d) * ae_fwd_nw(d); }
static int ola_loss_partials(const st_dims* d) { return d->B * ((d->y + 255) / 256); }
static int norm_partials(const st_dims* d) { return stm::norm_partial_count(d->F, d->N); }
extern "C" int st_ae_fwd_partials(const st_dims* d) { return check_dims(d) != ST_OK ? 0 : ae_fwd_partials(d); }
extern "C" int st_ola_loss_partials(const st_dims* d) { return check_dims(d) != ST_OK ? 0 : ola_loss_partials(d); }
extern "C" int st_norm_partials(const st_dims* d) { return check_dims(d) != ST_OK ? 0 : norm_partials(d); }
// The slab area of the weight-gradient GEMMs: room for the larger of the two whole-tensor fp32 rules over ALL B * T frames (the live rows of either GEMM are
// no more), then 64 Nyquist partials [2][N] of the 128 x 128-tile form.  What every launch must keep (tests/test_wgrad_plan_host.py): its slabs, and behind
// them its Nyquist partials, fit this area -- for every batch, precision, half and kernel form.
static const int WGRAD_NYQ_MAX = 64;
static int wgrad_area_slabs(const st_dims* d)      // always by the device's own CU count: the area is what the caller allocated, whatever count a query assumes
{
    const int KP = st_kp_of(d->F), R = d->B * d->T, unbounded = 1 << 30;      // the two rules that size the area, before any area bounds them
    const int s = wgrad_slices(WG_96, false, R, KP, d->N, unbounded), s2 = wgrad_slices(WG_TN128, false, R, KP, d->N, unbounded);
    return s2 > s ? s2 : s;
}
static size_t wgrad_ws_floats(const st_dims* d)
{
    return (size_t)wgrad_area_slabs(d) * st_kp_of(d->F) * d->N + (size_t)WGRAD_NYQ_MAX * 2 * d->N;
}
extern "C" size_t st_wgrad_ws_floats(const st_dims* d) { return check_dims(d) != ST_OK ? 0 : wgrad_ws_floats(d); }
// split-K slabs of the synthesis data-gradient GEMM (dAA; summed inside ae_bwd_kernel) and of the synthesis frames GEMM (frs; summed by ola_loss_kernel): synth_tile
static int synth_slabs(const st_dims* d) { return synth_tile(synth_live_rows(d)).ns; }
extern "C" int st_synth_slabs(const st_dims* d) { return check_dims(d) != ST_OK ? 0 : synth_slabs(d); }
static int frame_slabs(const st_dims* d) { return synth_tile(synth_live_rows(d)).ns; }
extern "C" int st_synth_frame_slabs(const st_dims* d) { return check_dims(d) != ST_OK ? 0 : frame_slabs(d); }
// Wide geometries (T > 32 or OT > 16) run the autoencoders as feature-major GEMMs (st_ae_wide.h) and need workspace
// for the activations [features][B*FP]; the fused kernels of st_ae.h need none in forward.
static bool ae_is_wide(const st_dims* d) { return d->T > 32 || d->OT > 16; }
struct WideWS {
    float *W1p[2], *W5p[2], *V[2], *H[2][8], *E9[2];         // forward: H[a][j] = output of layer j+1 (H[a][3] has 16 + K rows: [h4 ; knobs])
    float *DA[2][9], *TL[2], *slabs, *inner_ws;               // backward: dA_l, skip/residual tails, split-K slabs (one set per net), workgroup partials of the fused inner kernel
    // every layer-input buffer (V, H[.][j]) has ONE extra row (index = that layer's IN) of ones: bias gradient via the wgrad GEMM
    size_t fwd_floats, floats; int Tp, nsplit; size_t R, SL; int so[10];
};
static void wide_carve(const st_dims* d, const Layout& L, float* base, WideWS* w)
{
    const int FP = st_kp_of(d->F) / 2;
    const size_t R = (size_t)d->B * FP;
    int out[9], in[9]; ae_shapes(d, out, in);      // H[.][j] is the input of layer j + 1, DA[.][l] the output gradient of layer l
    w->R = R; w->Tp = st_round_up(d->T, 32);      // 32: k-tile of the bf16 GEMM kernel (level-2 precision)
    { long ns = (long)(R / 128); w->nsplit = (int)(ns < 1 ? 1 : (ns > 256 ? 256 : ns)); }   // wgrad K = R: short k-chains on many workgroups
    w->so[0] = 0;
    for (int l = 0; l < 9; ++l) w->so[l + 1] = w->so[l] + st_round_up(out[l] * (in[l] + 1), 64);
    w->SL = (size_t)w->so[9];
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += (n + 63) / 64 * 64; return p; };
    for (int a = 0; a < 2; ++a) {
        w->W1p[a] = take((size_t)64 * w->Tp); w->W5p[a] = take(16 * 32);
        w->V[a] = take((size_t)(d->T + 1) * R);
        for (int j = 0; j < 8; ++j) w->H[a][j] = take((size_t)(in[j + 1] + 1) * R);
        w->E9[a] = take((size_t)d->OT * R);
    }
    w->fwd_floats = off;
    for (int a = 0; a < 2; ++a) {
        for (int l = 0; l < 9; ++l) w->DA[a][l] = take((size_t)out[l] * R);
        w->TL[a] = take((size_t)d->OT * R);
    }
    w->slabs = take((size_t)2 * w->nsplit * w->SL);
    w->inner_ws = take((size_t)ae_bwd_grid(d) * 2 * L.PG);
    w->floats = off;
}
// Fused geometries: the autoencoder workspace is [h4 exchange | d a4 exchange | workgroup gradient partials]; the first two are the
// 16-wide code of both nets and its gradient, [net][group][lane] float4 each, that connect the forward kernel and the two halves
// of the split backward (st_ae_split.h).  g_ae_split = 0 runs the single-kernel backward (st_set_tuning(8000), diagnostics).
static const int AE_SPLIT_NW = 8;
static size_t ae_h4_floats(const st_dims* d) { return (size_t)2 * ae_fwd_groups(d) * 256; }
static int ae_split_grid(const st_dims* d) { int g = (ae_fwd_groups(d) + AE_SPLIT_NW - 1) / AE_SPLIT_NW; int c = num_cus() / 2; if (c < 1) c = 1; return g < c ? g : c; }
// The split form pays where the MFMAs are long (fp32: measured 181 vs 188 us at B = 256); with 16-bit operands the matrix time is a
// few microseconds, the kernel is all instruction issue, and two kernels only add a second prologue (bf16_all: 128 vs 124 us): those
// precisions keep the single kernel.
// 16-bit operands in the split form were tried (decoder + encoder halves 49 + 45 us against 101 us for the single kernel, the step did not
// move) and are NOT instantiated: the compiler emitted a cross-block MFMA-result hazard in the 16-bit encoder half (tools/check_mfma_hazards.py).
static bool ae_use_split(const st_dims* d) { return (g_ae_split < 0 ? ae_ht(d->prec) != 0 : g_ae_split != 0) && !ae_is_wide(d); }
// Round 6: kept activations of the fused fp32 autoencoders ([net][group][17 tiles][64 lanes] float4, st_ae.h): the workspace always has room for them where the
// autoencoder layers run in fp32 (the tuning switch picks the kernels, not the size); they sit BEHIND the workgroup partials.
static size_t ae_sv_floats(const st_dims* d) { return (!ae_is_wide(d) && ae_ht(d->prec) == 0) ? (size_t)2 * ae_fwd_groups(d) * sta::AE_SV_TILES * 256 : 0; }
static int ae_parts_max(const st_dims* d) { return ae_split_grid(d) > ae_bwd_grid(d) ? ae_split_grid(d) : ae_bwd_grid(d); }
static bool ae_use_saved(const st_dims* d) { return g_ae_save && !ae_is_wide(d) && ae_ht(d->prec) == 0 && !ae_use_split(d); }
static float* ae_sv_ptr(const st_dims* d, const Layout& L, float* aews) { return aews + 2 * ae_h4_floats(d) + (size_t)ae_parts_max(d) * 2 * L.PG; }
// Round 10: the ready-made LDS weight images of both nets + the frequency-weight table (st_ae.h ae_img_floats), written by prep_kernel in front of every fused forward and
// read by the prologues of ae_fwd_kernel and of the kept-activation ae_bwd_kernel.  They need no workspace of their own: with fp32 layers on the single-kernel backward
// nothing uses the h4 / d a4 exchange areas at the head of the autoencoder workspace (they connect the forward to the SPLIT backward), 1024 floats per row group, and the
// images lie there -- as much of them as fits: the forward's part (both forward images + the table) from 20 groups (at the default geometry: B >= 1 ), the backward's
// data-gradient images behind it from 38 (B >= 2).  A kernel whose part does not fit (tiny batches of tiny geometries) builds its images itself, as do all other paths.
static int ae_img_level(const st_dims* d)      // 0: no ready-made images, 1: the forward's part, 2: the backward's too
{
    if (g_ae_save == 2 || ae_is_wide(d) || ae_ht(d->prec) != 0 || ae_use_split(d)) return 0;
    const int FP = st_kp_of(d->F) / 2;
    const size_t room = 2 * ae_h4_floats(d);
    if (FP > sta::CL::FWD_TOTAL || room < (size_t)sta::ae_img_fwd_floats(FP)) return 0;      // FP <= FWD_TOTAL: the backward kernel keeps its copy of the table in the place of the forward images
    return room >= (size_t)sta::ae_img_floats(FP) ? 2 : 1;
}
static float* ae_img_ptr(float* aews) { return aews; }
// st_model_bwd_knobs: does the autoencoder backward this geometry / precision / tuning state routes to (behind a forward that kept its state) exist with the
// per-group d a5 output?  Instantiated: the wide path's fused kernel, the kept-activation fp32 kernel and the 16-bit decoder half -- what the shipped
// defaults reach.  A diagnostic switch away from its default (g_ae_split, g_ae_save) can route elsewhere.
static const char* ae_kg_why(const st_dims* d)
{
    if (ae_is_wide(d)) return nullptr;
    if (ae_use_split(d)) return ae_ht(d->prec) != 0 ? nullptr : "g_ae_split routes fp32 layers to the split kernels";
    if (ae_ht(d->prec) != 0) return "g_ae_split routes 16-bit layers to the single kernel";
    return ae_use_saved(d) ? nullptr : "g_ae_save is off: the recomputing fp32 kernel";
}
static bool ae_kg_route(const st_dims* d) { return ae_kg_why(d) == nullptr; }
extern "C" size_t st_ae_fwd_ws_floats(const st_dims* d)
{
    Layout L; if (make_layout(d, &L) != ST_OK) return 0;
    if (!ae_is_wide(d)) return ae_h4_floats(d);             // optional for the forward alone (ws may be NULL: h4 is then not kept)
    WideWS w; wide_carve(d, L, nullptr, &w); return w.fwd_floats;
}
extern "C" size_t st_ae_kept_activation_bytes(const st_dims* d)
{
    if (check_dims(d) != ST_OK || !ae_use_saved(d)) return 0;
    return ae_sv_floats(d) * sizeof(float);
}
static size_t ae_bwd_ws_floats(const st_dims* d, const Layout& L)
{
    if (ae_is_wide(d)) { WideWS w; wide_carve(d, L, nullptr, &w); return w.floats; }
    return 2 * ae_h4_floats(d) + (size_t)ae_parts_max(d) * 2 * L.PG + ae_sv_floats(d);
}
extern "C" size_t st_ae_bwd_ws_floats(const st_dims* d) { Layout L; return make_layout(d, &L) != ST_OK ? 0 : ae_bwd_ws_floats(d, L); }
static int ae_wide_fwd(const st_dims* d, const Layout& L, const float* mag, const float* phs, const float* knobs,
                       const float* ae_m, const float* ae_p, float* mag_hat, float* phs_hat, float* AA, float* reg_partial,
                       WideWS& w, void* stream, unsigned short* AA16 = nullptr, bool in_done = false);

// ------------------------------------------------------------------------------ per-op entry points
// Feature-major destination of the polar epilogue on wide geometries (st_gemm.h PolarStore::Vm / Vp): the wide autoencoder path's input layout
struct PolarWide { float* Vm; float* Vp; int FP; unsigned RV; };
static inline void polar_wide_set(stg::PolarStore& ep, const PolarWide* pw) { if (pw && pw->Vm) { ep.Vm = pw->Vm; ep.Vp = pw->Vp; ep.FP = pw->FP; ep.RV = pw->RV; } }
static int pad_scale(const float* in, float* out, int B, int Ls, int pad, float s, void* stream)
{
    hipLaunchKernelGGL(stm::pad_scale_kernel, dim3(((Ls + 2 * pad) / 4 + 255) / 256, B), dim3(256), 0, st_stream(stream), in, out, Ls, pad, s);
    ST_LAUNCHED("pad_scale");
    return ST_OK;
}

// AA16 != NULL (fused step of the 16-bit GEMM configurations): the spectra are written rounded to the operand type, not as fp32
static int ae_fwd_body(const st_dims* d, const Layout& L, const float* mag, const float* phs, const float* knobs,
                       const float* ae_m, const float* ae_p, float* mag_hat, float* phs_hat, float* AA,
                       float* reg_partial, float* ws, void* stream, unsigned short* AA16 = nullptr, bool wide_in_done = false, float* sv = nullptr, const float* img = nullptr)
{      // sv != NULL (fused fp32 geometries, training step): the activations are kept for the backward (ae_sv_floats)
       // img != NULL (fused step, fp32 layers): prep_kernel built the weight images of this step (ae_img_level); the per-op entry builds them in the kernel
    const int aa_ht = AA16 ? gemm_ht(d->prec) : 0;
    ST_REQ(mag && phs && (knobs || d->K == 0) && ae_m && ae_p && ((mag_hat && phs_hat && AA) || (!mag_hat && !phs_hat && !AA && ws)), "st_ae_fwd: null pointer");
    if (!knobs) knobs = ae_m;      // K == 0: the kernels issue one clamped, masked load of knobs[0] -- any resident float will do
    if (ae_is_wide(d)) {
        ST_REQ(mag_hat, "st_ae_fwd: the code-only pass exists for the fused geometries only");
        ST_REQ(ws, "st_ae_fwd: this geometry (T=%d, OT=%d) needs st_ae_fwd_ws_floats() floats of workspace", d->T, d->OT);
        WideWS w; wide_carve(d, L, ws, &w);
        return ae_wide_fwd(d, L, mag, phs, knobs, ae_m, ae_p, mag_hat, phs_hat, AA, reg_partial, w, stream, AA16, wide_in_done);
    }
    ST_REQ((size_t)d->B * d->T * d->F < ((size_t)1 << 30) && (size_t)d->B * d->OT * L.KP < ((size_t)1 << 30),
           "st_ae_fwd: batch too large for the kernel's 32-bit element offsets (B=%d)", d->B);
    const size_t lds = ((size_t)2 * sta::CL::FWD_TOTAL + (size_t)(L.KP / 2)) * sizeof(float);      // two forward images + the per-bin frequency weights
    const float expfac = expfac_of(d);
    const int ht = ae_ht(d->prec);
    const dim3 grid(ae_fwd_grid(d));
    hipStream_t s = st_stream(stream);
    const bool use32 = g_ae32 && ht != 0 && L.KP / 2 <= 17 * 32 && AE_FWD_NW == 8;
    if (use32)                      // 16-bit layers only: 32-row groups (st_ae32.h)
        ST_TRY(with_ht16(ht, [&](auto HT) {
            return launch_lds("ae_fwd32_kernel", sta::ae_fwd32_kernel<AE_FWD_NW, HT()>, grid, dim3(AE_FWD_NW * 64), (size_t)sta::ae32_lds_floats(L.KP / 2) * sizeof(float), s,
                              mag, phs, knobs, ae_m, ae_p, L.go, mag_hat, phs_hat, AA, reg_partial, d->B, d->T, d->OT, d->F, d->K, L.KP, expfac, ws, AA16, aa_ht); }));
    else if (ht != 0)               // ... on 16-row groups: no kept activations, no ready-made images
        ST_TRY(with_ht16(ht, [&](auto HT) {
            return launch_lds("ae_fwd_kernel", sta::ae_fwd_kernel<AE_FWD_NW, HT()>, grid, dim3(AE_FWD_NW * 64), lds, s,
                              mag, phs, knobs, ae_m, ae_p, L.go, mag_hat, phs_hat, AA, reg_partial, d->B, d->T, d->OT, d->F, d->K, L.KP, expfac, ws, AA16, aa_ht, nullptr, nullptr); }));
    else if (sv) {                  // fp32 layers: 8 or 11 waves (ae_fwd_nw), with or without the kept activations
        ST_REQ(mag_hat, "st_ae_fwd: internal: kept activations on a code-only pass");
        ST_TRY(with_fwd_nw(ae_fwd_nw(d), [&](auto NW) {
            return launch_lds("ae_fwd_kernel", sta::ae_fwd_kernel<NW(), 0, true>, grid, dim3(NW() * 64), lds, s,
                              mag, phs, knobs, ae_m, ae_p, L.go, mag_hat, phs_hat, AA, reg_partial, d->B, d->T, d->OT, d->F, d->K, L.KP, expfac, ws, AA16, aa_ht, sv, img); }));
    } else
        ST_TRY(with_fwd_nw(ae_fwd_nw(d), [&](auto NW) {
            return launch_lds("ae_fwd_kernel", sta::ae_fwd_kernel<NW(), 0>, grid, dim3(NW() * 64), lds, s,
                              mag, phs, knobs, ae_m, ae_p, L.go, mag_hat, phs_hat, AA, reg_partial, d->B, d->T, d->OT, d->F, d->K, L.KP, expfac, ws, AA16, aa_ht, nullptr, img); }));
    ST_LAUNCHED("ae_fwd"); return ST_OK;
}
extern "C" int st_ae_fwd(const st_dims* d, const float* mag, const float* phs, const float* knobs,
                         const float* ae_m, const float* ae_p, float* mag_hat, float* phs_hat, float* AA,
                         float* reg_partial, float* ws, void* stream)
{
    Layout L; ST_TRY(make_layout(d, &L));
    return ae_fwd_body(d, L, mag, phs, knobs, ae_m, ae_p, mag_hat, phs_hat, AA, reg_partial, ws, stream);
}

extern "C" int st_synth_fold(const st_dims* d, const float* Sr, const float* Si, float* Sfold, void* stream)
{
    ST_TRY(check_dims(d)); ST_REQ(Sr && Si && Sfold, "st_synth_fold: null pointer");
    const int KP = st_kp_of(d->F);
    hipLaunchKernelGGL(stm::fold_kernel, dim3(KP), dim3(256), 0, st_stream(stream), Sr, Si, Sfold, d->N, d->F, KP);
    ST_LAUNCHED("synth_fold"); return ST_OK;
}

static stg::RowMap synth_live(const st_dims* d) { return stg::live_frames(d->OT, d->H, d->N, d->N, d->y); }
static int synth_live_rows(const st_dims* d) { return synth_live(d).rows(d->B); }

// Fraction of the synthesis frames' taps that the crop of cls_fe_dft.py:113 throws away (the structural zeros the work list skips): 25 % at the 8192-sample window
// (7 live frames), 4 % at the 65536-sample window (44 live frames)
static double synth_crop_fraction(const st_dims* d)
{
    const stg::RowMap ms = synth_live(d);
    long live = 0;
    for (int t = ms.t_lo; t < ms.t_lo + ms.Tv; ++t) { int lo, hi; stg::ntw_live_taps(t, t, d->H, d->N, d->N, d->y, lo, hi); live += hi - lo; }
    return 1.0 - (double)live / ((double)ms.Tv * (double)d->N);
}
// the frame-major row order splits a compact row r < R = frames * B into (frame, window) with a multiply-high by the reciprocal of B
// (RowMap::magic, rowmap_magic()), which is exact only while r * B < 2^32.  Every switch that turns the frame-major order on asks this first; past the bound
// (B = 32768 at 7 live frames) the launch keeps the window-major order, i.e. the untrimmed / uncropped kernels of round 4.
static inline bool fm_div_exact(int R, int B) { return R >= 0 && B >= 1 && (unsigned long long)(unsigned)R * (unsigned long long)(unsigned)B < (1ull << 32); }
extern "C" int st_fm_div_exact(int R, int B) { return fm_div_exact(R, B) ? 1 : 0; }
// the 128 x 128-tile work-list kernel (st_gemm_tn.h): fp32 products, up to 255 tile rows.  Used where one workgroup per CU covers the whole GEMM in one round (the rule
// of rounds 3-4: small batches at any geometry) or where the crop is worth the frame-major row order (>= 10 % of the taps: every geometry of the 8192-sample window) --
// several rounds are then fine (B = 512: 61 / 69 us against 107 / 107 on gemm_kernel<2, ...>).  MEASURED the other way at the 65536-sample window (B = 64, 4 % cropped, 510 workgroups
// in two rounds): 80 / 77 us against 64 / 65 -- a tile's 128 rows there are 64 windows 194 KB apart; that geometry stays on the small-tile kernel.  Whether a list fits (and with
// how many k-slices) is the builder's decision (ntw_frames / ntw_dgrad return false -> gemm_kernel<4, ...> / <2, ...>).
static bool use_nt128(const st_dims* d, int M, int Nc, int ncus = 0)      // a pure function of (d, ncus) once ncus > 0 (st_nt128_worklist's override: ADVICE round 5)
{
    if (!(g_nt128 && gemm_ht(d->prec) == 0 && d->N % 32 == 0 && (M + 127) / 128 <= 255 && fm_div_exact(M, d->B))) return false;
    if (ncus <= 0) ncus = num_cus();
    return ((M + 127) / 128) * ((Nc + 127) / 128) * 2 <= ncus || synth_crop_fraction(d) >= 0.10;
}
// ------------------------------------------------------------------------------ the forward and data-gradient GEMMs: plan, launch
// The three STFT GEMMs that are no weight gradient -- the analysis forward (frames of x / 2 times the analysis bases, polar epilogue), the synthesis frames
// (spectra times the folded synthesis bases) and the synthesis data gradient (frames of d syn times the fold) -- decided in one place (stft_plan; it launches
// nothing) for the per-op entries, the fused steps, st_predict_long and the host queries (st_stft_plan, st_nt128_worklist), and launched in one (stft_gemm).
enum { GEMM_ANALYSIS = 0, GEMM_FRAMES = 1, GEMM_DGRAD = 2 };
enum { SGP_PADDED = 1,         // operands in the padded workspace layout (the fused entries); else the per-op entries' unpadded signal with its in_scale
       SGP_G16 = 2,            // the entry asks for the 16-bit operand pipeline (WS::g16 is its answer)
       SGP_SFOLDT = 4 };       // the transposed fold [N][KP] is there (the fused forward builds it: prep_kernel) -- both operands of the frames GEMM K-contiguous
enum { GF_FP32 = 0,            // fp32 operands, fp32 MFMA
       GF_HALF = 1,            // fp32 operands converted as they are staged: gemm_half_kernel (bf16 / f16 / the in-kernel three-plane split of ST_PREC_F32X3)
       GF_PLANES = 2,          // bfloat16 planes of the once-per-step operands (st_gemm_planes.h; planes_prepare writes them)
       GF_G16 = 3 };           // the 16-bit operand pipeline (st_gemm16.h): every operand pre-rounded by its producer
enum { GK_SMALL = 0,           // gemm_kernel / gemm_half_kernel: `waves` waves share a (32 waves) x 96 tile (small_gemm)
       GK_NT128 = 1,           // the 128 x 128 work-list kernel (st_gemm_tn.h) on the plan's NTWork list
       GK_PLANES = 2,          // gemm_planes_kernel, `waves` x (32 x 96)
       GK_NT16 = 3, GK_NT256 = 4 };      // launch16_nt / the LDS-DMA kernel behind launch16_nt256
// The operand family: the ONE statement of the rule.  The per-op entries have fp32 operands and nothing else; a fused entry runs the 16-bit pipeline where it
// asks for it and use_g16 admits the precision, else the plane kernel where use_planes does (ST_PREC_F32X3; the bf16 levels under g_pl_bf16, which turns the
// 16-bit pipeline off) -- the data gradient only under g_pl_dgrad (measured slower than the fp32 MFMA kernel) --, else the kernels of the per-op entries.
static bool use_planes(const st_dims* d) { return (gemm_ht(d->prec) == 3 || (gemm_ht(d->prec) == 1 && g_pl_bf16)) && d->N % 16 == 0 && st_kp_of(d->F) % 16 == 0; }
static int planes_of(const st_dims* d) { return gemm_ht(d->prec) == 3 ? 3 : 1; }
template <class F> static inline auto with_planes(int pl, F&& f) { return pl == 1 ? f(ic<1>{}) : f(ic<3>{}); }
static bool use_g16(const st_dims* d)
{
    const int ht = gemm_ht(d->prec);
    return g_g16 && (ht == 1 || ht == 2) && !g_pl_bf16 && d->N % 128 == 0 && num_cus() > 0;
}
static int stft_family(const st_dims* d, int which, int flags)
{
    if (flags & SGP_PADDED) {
        if ((flags & SGP_G16) && use_g16(d)) return GF_G16;
        if (use_planes(d) && (which != GEMM_DGRAD || g_pl_dgrad)) return GF_PLANES;
    }
    return gemm_ht(d->prec) == 0 ? GF_FP32 : GF_HALF;
}
// The operand pointers of whichever family is taken.  A: the signal (x, or the padded x / 2), the spectra AA, d syn.  B: Wr, Sfold, Sfold; B2: Wi resp. the
// transposed fold.  A16 / B16: the 16-bit copies (B16 of the frames GEMM: SfoldT16).  Bpl: the plane copy of B (frames GEMM: of the transposed fold).
struct GemmOps { const float *A, *B, *B2; const unsigned short *A16, *B16, *Bpl; float in_scale; };
struct GemmPlan {
    const st_dims* d; GemmOps o;
    int which, flags, family, form;
    int waves, bk, xt;          // GK_SMALL / GK_PLANES: waves per workgroup (tile height 32 * waves); GK_SMALL on GF_FP32: k-tile depth, k-quad-major staging (g_xt); else 0
    bool transposed;            // frames GEMM on GK_SMALL / GK_NT128: B is the transposed fold (SGP_SFOLDT and g_frs_nt)
    stg::RowMap live;           // the frames with a tap inside the signal, window-major
    int R, M, Nc, K, ns;        // live rows; the GEMM is M = R x Nc over K; split-K slabs
    size_t slab;                // slab stride of the output (frs, dAA)
    bool frame_major; int crop; // rows enumerated frame-major; structural zeros of the crop (cls_fe_dft.py:113) skipped: 0 none, 1 the frames GEMM's dead tile columns,
                                // 2 the data gradient's dead taps per tile row -- stg::Crop16::mode on GF_G16, the work list on GK_NT128
    stg::NTWork wk;             // GK_NT128: the list, built here once (wk.n = 0 on every other form)
};
// ncus > 0 makes the plan a pure function of its arguments and the tuning state (the host queries); otherwise the current device's CU count.
static GemmPlan stft_plan(const st_dims* d, int which, int flags, const GemmOps& o, int ncus = 0)
{
    const int KP = st_kp_of(d->F), N = d->N;
    const bool padded = (flags & SGP_PADDED) != 0;
    GemmPlan p; p.d = d; p.o = o; p.which = which; p.flags = flags;
    p.live = which == GEMM_ANALYSIS ? stg::live_frames(d->T, d->H, N, N, d->L)      // frames entirely inside the Conv1d padding are skipped
                                    : synth_live(d);                                // output frames that land wholly in the cropped margins are never needed
    p.R = p.M = p.live.rows(d->B);
    p.Nc = which == GEMM_ANALYSIS ? 2 * d->F : which == GEMM_FRAMES ? N : KP; p.K = which == GEMM_FRAMES ? KP : N;
    // the analysis forward (Nc = 2 F columns) fills the chip with 4-wave tiles and one slab at every batch; the synthesis pair by synth_tile
    const SynthTile t = which == GEMM_ANALYSIS ? SynthTile{4, 1} : synth_tile(p.R);
    p.waves = t.waves; p.ns = t.ns; p.slab = which == GEMM_ANALYSIS ? 0 : (size_t)d->B * d->OT * p.Nc;
    p.family = stft_family(d, which, flags);
    p.bk = p.xt = 0; p.transposed = false; p.frame_major = false; p.crop = 0; p.wk.n = 0;
    if (p.family == GF_G16) {
        // g_g16_dma: bit 0 the analysis forward, bit 1 the data gradient on the LDS-DMA kernel (64-deep k-tiles, at least one per slab); it has no crop
        const int dma = which == GEMM_ANALYSIS ? 1 : which == GEMM_DGRAD ? 2 : 0;
        p.form = ((g_g16_dma & dma) && N % 64 == 0 && N / 64 >= p.ns) ? GK_NT256 : GK_NT16; p.waves = 0;
        // g_g16_crop: bit 0 the frames GEMM, bit 1 the data gradient (off wherever g_g16_dma asks for the DMA kernel); on the frame-major row order
        const bool crop = which == GEMM_FRAMES ? (g_g16_crop & 1) != 0 : which == GEMM_DGRAD && (g_g16_crop & 2) && !(g_g16_dma & 2);
        if (crop && fm_div_exact(p.R, d->B)) { p.frame_major = true; p.crop = which; }
    } else if (p.family == GF_PLANES) {
        p.form = GK_PLANES;
        if (which == GEMM_ANALYSIS && planes_of(d) == 3 && g_pl_shape == 3) p.waves = 8;      // 256 x 96, one workgroup per CU
    } else {
        p.form = GK_SMALL;
        p.transposed = which == GEMM_FRAMES && (flags & SGP_SFOLDT) && g_frs_nt;
        const int cus = ncus > 0 ? ncus : num_cus();
        // the work-list kernel takes K-contiguous operands in the padded layout; whether a list fits (and with how many k-slices) is the builder's decision
        if ((which == GEMM_FRAMES ? p.transposed : which == GEMM_DGRAD && padded) && use_nt128(d, p.R, p.Nc, cus) &&
            (which == GEMM_FRAMES ? stg::ntw_frames(p.wk, p.live, d->B, d->H, N, N, d->y, KP, p.ns, cus)
                                  : stg::ntw_dgrad(p.wk, p.live, d->B, d->H, N, N, d->y, d->F, KP, p.ns, cus))) {
            p.form = GK_NT128; p.waves = 0; p.frame_major = true; p.crop = which;
        } else {
            p.wk.n = 0;
            // the padded analysis forward (K = N = 1024, two 4-wave workgroups per CU either way) runs 5 % faster with 32-deep k-tiles (half the barriers);
            // every other GEMM of the step is faster with 16 (more workgroups per CU)
            if (p.family == GF_FP32) { p.bk = (which == GEMM_ANALYSIS && padded) ? g_an_bk : g_bk; p.xt = g_xt ? 1 : 0; }
        }
    }
    return p;
}
// Where a plan's GEMM writes: re / im / mag / phs [B][T][F] (any may be NULL) and, on wide geometries, the feature-major copy `pw` of the analysis forward;
// C = frs (ns slabs [B * OT][N]; st_ola_loss sums them) resp. dAA (ns slabs [B * OT][KP]; st_ae_bwd sums them and treats the rows of dead frames, which are
// NOT written, as zero) of the synthesis pair.
struct GemmOut { float *re, *im, *mag, *phs; const PolarWide* pw; float* C; };
static GemmOut slabs_at(float* C) { return GemmOut{nullptr, nullptr, nullptr, nullptr, nullptr, C}; }
// The GEMM of a plan, whatever its family and form.  Rows of the data gradient: dfrs[b, t, n] = dfull[b, H t + n] with dfull = zero-pad(d syn, N each side).
static int stft_gemm(const GemmPlan& p, const GemmOut& out, void* stream)
{
    const st_dims* d = p.d; const GemmOps& o = p.o; hipStream_t s = st_stream(stream);
    const int KP = st_kp_of(d->F), N = d->N, R = p.R;
    const stg::RowMap rows = p.frame_major ? stg::frame_major(p.live, d->B) : p.live;      // the epilogue's row order
    auto g16 = [&](const stg::Rows16& ra, const stg::Rows16& rb, const auto& ep, const stg::Crop16* cr) {
        return with_ht16(gemm_ht(d->prec), [&](auto HT) {
            return p.form == GK_NT256 ? stg::launch16_nt256<HT()>(ra, rb, ep, p.M, p.Nc, p.K, p.ns, s) : stg::launch16_nt<HT()>(ra, rb, ep, p.M, p.Nc, p.K, p.ns, s, cr); }); };
    if (p.which == GEMM_ANALYSIS) {
        stg::PolarStore ep{out.re, out.im, out.mag, out.phs, R, d->F, rows};
        polar_wide_set(ep, out.pw);
        if (p.family == GF_G16)
            ST_TRY(g16(stg::rows16(o.A16, (unsigned)(d->L + 2 * N), (unsigned)d->H, p.live, R), stg::rows16_plain(o.B16, (unsigned)N, 2 * d->F), ep, nullptr));
        else if (!(p.flags & SGP_PADDED)) {
            stg::FramedNT<false> al{o.A, d->L, d->H, N, R, N, o.in_scale, p.live};
            ST_TRY(small_gemm<4>(d->prec, p.bk, p.xt != 0, al, stg::AnalysisW{o.B, o.B2, d->F, N}, ep, p.M, p.Nc, p.K, p.ns, s));
        } else {      // the workspace copy [B][N + L + N] (zero margins, input scale applied)
            stg::FramedNT<true> al{o.A, d->L, d->H, N, R, N, 1.0f, p.live};
            if (p.family == GF_PLANES) {
                stg::ChunkP bl{o.Bpl, 2 * d->F};
                ST_TRY((planes_of(d) == 1 ? stg::launch_planes<4, 1>(al, bl, ep, p.M, p.Nc, p.K, p.ns, s) :
                        p.waves == 8 ? stg::launch_planes<8, 3>(al, bl, ep, p.M, p.Nc, p.K, p.ns, s) : stg::launch_planes<4, 3>(al, bl, ep, p.M, p.Nc, p.K, p.ns, s)));
            } else ST_TRY(small_gemm<4>(d->prec, p.bk, p.xt != 0, al, stg::AnalysisW{o.B, o.B2, d->F, N}, ep, p.M, p.Nc, p.K, p.ns, s));
        }
        ST_LAUNCHED("analysis_fwd");
        return ST_OK;
    }
    const bool frames = p.which == GEMM_FRAMES;
    const unsigned s_win = frames ? (unsigned)(d->OT * KP) : (unsigned)(d->y + 2 * N), s_frm = frames ? (unsigned)KP : (unsigned)d->H;      // A's window and frame strides
    auto small = [&](const auto& al, const auto& bl) {
        const stg::StoreC ep{out.C, R, p.Nc, p.Nc, p.slab, rows};
        return p.waves == 4 ? small_gemm<4>(d->prec, p.bk, p.xt != 0, al, bl, ep, p.M, p.Nc, p.K, p.ns, s) : small_gemm<2>(d->prec, p.bk, p.xt != 0, al, bl, ep, p.M, p.Nc, p.K, p.ns, s); };
    auto planes = [&](const auto& al) {
        const stg::StoreC ep{out.C, R, p.Nc, p.Nc, p.slab, rows}; const stg::ChunkP bl{o.Bpl, p.Nc};
        return with_planes(planes_of(d), [&](auto PL) {
            return p.waves == 4 ? stg::launch_planes<4, PL()>(al, bl, ep, p.M, p.Nc, p.K, p.ns, s) : stg::launch_planes<2, PL()>(al, bl, ep, p.M, p.Nc, p.K, p.ns, s); }); };
    if (p.family == GF_G16) {
        // crop 1: tile columns without a tap inside the crop are not computed (ola_loss_kernel never reads them); 2: per tile row only the taps that lie inside
        // d syn (the rest of the padded copy is zeros)
        const stg::Rows16 ra = p.frame_major ? stg::rows16_frame_major(o.A16, s_win, s_frm, p.live, d->B, R) : stg::rows16(o.A16, s_win, s_frm, p.live, R);
        const stg::Crop16 cr{p.crop, d->B, d->H, N, N, d->y, p.live.t_lo, R, 1};
        ST_TRY(g16(ra, stg::rows16_plain(o.B16, (unsigned)p.K, p.Nc), stg::StoreC{out.C, R, p.Nc, p.Nc, p.slab, rows}, &cr));
    } else if (p.form == GK_NT128) {
        // frame-major rows.  Frames GEMM: only the tile columns whose taps survive the crop.  Data gradient: per tile row only the taps inside d syn (the margins
        // of the padded copy are zeros), the Nyquist columns apart
        const stg::NTRows ra = stg::ntrows_frame_major(o.A, s_win, s_frm, p.live, d->B, R);
        const stg::NTRows rb = frames ? stg::NTRows{o.B2, (unsigned)KP, 0u, 0u, 1, 0, N} :
                               p.wk.col_h ? stg::NTRows{o.B, (unsigned)((KP / 2) * N), (unsigned)N, stg::rowmap_magic(d->F - 1), d->F - 1, 0, 2 * (d->F - 1)}
                                          : stg::NTRows{o.B, (unsigned)N, 0u, 0u, 1, 0, KP};
        ST_TRY(stg::launch_nt128(ra, rb, stg::StoreSlab{out.C, R, p.Nc, p.Nc, p.slab, rows}, p.wk, s));
    } else if (frames) {
        const stg::PlainNT al{o.A, R, KP, KP, p.live};
        if (p.family == GF_PLANES) ST_TRY(planes(al));
        else if (p.transposed) ST_TRY(small(al, stg::PlainNT{o.B2, N, KP, KP, stg::all_frames(1)}));
        else ST_TRY(small(al, stg::PlainTN{o.B, KP, N, N, stg::all_frames(1)}));
    } else {
        const stg::PlainNT bl{o.B, KP, N, N, stg::all_frames(1)};
        if (!(p.flags & SGP_PADDED)) ST_TRY(small(stg::FramedNT<false>{o.A, d->y, d->H, N, R, N, 1.0f, p.live}, bl));
        else {
            const stg::FramedNT<true> al{o.A, d->y, d->H, N, R, N, 1.0f, p.live};
            if (p.family == GF_PLANES) ST_TRY(planes(al)); else ST_TRY(small(al, bl));
        }
    }
    ST_LAUNCHED(frames ? "synthesis_frames" : "synthesis_dgrad");
    return ST_OK;
}
extern "C" int st_analysis_fwd(const st_dims* d, const float* x, const float* Wr, const float* Wi, float in_scale,
                               float* re, float* im, float* mag, float* phs, void* stream)
{
    ST_TRY(check_dims(d)); ST_REQ(x && Wr && Wi, "st_analysis_fwd: null input");
    const GemmPlan p = stft_plan(d, GEMM_ANALYSIS, 0, GemmOps{x, Wr, Wi, nullptr, nullptr, nullptr, in_scale});
    ST_TRY(stft_gemm(p, GemmOut{re, im, mag, phs, nullptr, nullptr}, stream));
    if (p.live.Tv < d->T) {   // the skipped frames are exact zeros (re=im=mag=0, phs=atan2(0,1e-7)=0); the fused entries fill them in prep_kernel
        hipLaunchKernelGGL(stm::zero_dead_frames_kernel, dim3(d->B * (d->T - p.live.Tv)), dim3(256), 0, st_stream(stream),
                           re, im, mag, phs, d->T, d->F, p.live.t_lo, p.live.Tv);
        ST_LAUNCHED("zero_dead_frames");
    }
    return ST_OK;
}
extern "C" int st_synthesis_frames(const st_dims* d, const float* AA, const float* Sfold, float* frs, void* stream)
{
    ST_TRY(check_dims(d)); ST_REQ(AA && Sfold && frs, "st_synthesis_frames: null pointer");
    return stft_gemm(stft_plan(d, GEMM_FRAMES, 0, GemmOps{AA, Sfold, nullptr, nullptr, nullptr, nullptr, 1.0f}), slabs_at(frs), stream);
}
extern "C" int st_synthesis_dgrad(const st_dims* d, const float* dsyn, const float* Sfold, float* dAA, void* stream)
{
    ST_TRY(check_dims(d)); ST_REQ(dsyn && Sfold && dAA, "st_synthesis_dgrad: null pointer");
    return stft_gemm(stft_plan(d, GEMM_DGRAD, 0, GemmOps{dsyn, Sfold, nullptr, nullptr, nullptr, nullptr, 1.0f}), slabs_at(dAA), stream);
}

// Host-side view of the work list of the 128 x 128-tile synthesis GEMMs (st_gemm_tn.h, round 5): which = 0 the frames GEMM, 1 the data gradient -- the list of the
// plan a fused entry on fp32 operands launches.
// out[i] = the packed entry i (tile row (8 bits) | tile column (6) << 8 | slab (2) << 14 | first zero-filled slab (2; 0 = none) << 16 | kind (1) << 18 | first k unit (6) << 19 |
// k units (7) << 25); head6 = {slabs, col_h, col_stride, frame-major windows per frame, k-tiles (of 32) per k unit, k-tiles of the whole reduction}.  Returns the number of
// entries (= workgroups), 0 when this geometry does not run on the work-list kernel, < 0 on bad arguments.  No device work: the CPU test-suite checks the list against the
// cropping rule of cls_fe_dft.py:113.
extern "C" int st_nt128_worklist(const st_dims* d, int which, int ncus, unsigned* out, int cap, int* head6)
{
    if (check_dims(d) != ST_OK || !out || !head6 || cap < 0 || (which != 0 && which != 1)) return -1;
    const GemmPlan p = stft_plan(d, which ? GEMM_DGRAD : GEMM_FRAMES, SGP_PADDED | SGP_SFOLDT, GemmOps{}, ncus);
    if (p.form != GK_NT128) return 0;
    const stg::NTWork& wk = p.wk;
    head6[0] = wk.nslabs; head6[1] = wk.col_h; head6[2] = wk.col_stride; head6[3] = d->B; head6[4] = wk.kunit; head6[5] = wk.kt_total;
    for (int i = 0; i < wk.n && i < cap; ++i) out[i] = wk.e[i];
    return wk.n;
}
// Host-side view of ONE of the three GEMMs (no device work): the plan the launches themselves ask for, as ST_STFT_PLAN_INTS ints (signaltrain_hip.h).
// which: ST_STFT_*; flags: ST_STFTPLAN_*; ncus <= 0: the current device's CU count -- then the answer is what a launch on this device does under the current
// tuning state.  Fills min(cap, count) ints and returns the count; < 0 on bad arguments.
extern "C" int st_stft_plan(const st_dims* d, int which, int flags, int ncus, int* out, int cap)
{
    static_assert(ST_STFT_ANALYSIS == GEMM_ANALYSIS && ST_STFT_FRAMES == GEMM_FRAMES && ST_STFT_DGRAD == GEMM_DGRAD, "st_stft_plan: which values");
    static_assert(ST_STFTPLAN_PADDED == SGP_PADDED && ST_STFTPLAN_G16 == SGP_G16 && ST_STFTPLAN_SFOLDT == SGP_SFOLDT, "st_stft_plan: flag values");
    if (check_dims(d) != ST_OK || cap < 0 || (cap > 0 && !out) || which < GEMM_ANALYSIS || which > GEMM_DGRAD) return -1;
    if ((flags & ~(SGP_PADDED | SGP_G16 | SGP_SFOLDT)) || ((flags & (SGP_G16 | SGP_SFOLDT)) && !(flags & SGP_PADDED))) return -1;      // the fused entries' alone
    const GemmPlan p = stft_plan(d, which, flags, GemmOps{}, ncus);
    const int v[ST_STFT_PLAN_INTS] = {p.family, p.form, p.waves, p.bk, p.xt, p.R, p.M, p.Nc, p.K, p.ns, p.frame_major ? 1 : 0, p.crop, p.wk.n, p.live.t_lo, p.live.Tv};
    for (int i = 0; i < ST_STFT_PLAN_INTS && i < cap; ++i) out[i] = v[i];
    return ST_STFT_PLAN_INTS;
}

// with_mae (the validation pass, st_eval_step): the kernels' MAE instantiations -- loss_partial then has room for a second array of st_ola_loss_partials() floats, the
// |y - y_hat| partials, at stm::mae_partial_offset() -- and no d syn is written
static int ola_loss_impl(const st_dims* d, const float* frs, const float* x, const float* y_true,
                         float* y_hat, float* dsyn, int dsyn_pad, float* loss_partial, void* stream, unsigned short* dsyn16 = nullptr,
                         bool with_mae = false)
{
    if (with_mae) ST_REQ(y_true && loss_partial && !dsyn, "ola_loss: the MAE partials come with a target and without d syn");
    const float inv = loss_scale_of(d) / ((float)d->B * (float)d->y);     // d loss / d y_hat, times the loss scale (train.py:134-135)
    {   // four samples per thread (round 5) where the geometry and the pointers allow 16-byte accesses: always inside the fused step
        const int ns = frame_slabs(d), nslot = (d->y + 255) / 256;
        auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
        const bool ok4 = d->H % 4 == 0 && d->N % 4 == 0 && d->y % 4 == 0 && d->L % 4 == 0 && dsyn_pad % 4 == 0 && ns >= 1 && ns <= 3 && (d->N + d->H - 1) / d->H <= 3 &&
                         al16(frs) && al16(x) && al16(y_true) && al16(y_hat) && al16(dsyn) && al16(dsyn16) && ((size_t)d->B * d->OT * d->N) % 4 == 0;
        if (ok4) {
            const dim3 grid((d->y / 4 + 255) / 256, d->B);
            const size_t slab = (size_t)d->B * d->OT * d->N;
            unsigned short* d16 = dsyn ? dsyn16 : nullptr; const int ht = dsyn16 ? gemm_ht(d->prec) : 0;
            with_bool(with_mae, [&](auto MAE) { with_slabs(ns, [&](auto NS) {
                hipLaunchKernelGGL((stm::ola_loss4_kernel<NS(), MAE()>), grid, dim3(256), 0, st_stream(stream), frs, x, y_true, y_hat, dsyn, loss_partial, d->L, d->N, d->H, d->OT, d->y, inv, slab, dsyn_pad, nslot, d16, ht); }); });
            ST_LAUNCHED("ola_loss");
            return ST_OK;
        }
    }
    with_bool(with_mae, [&](auto MAE) {
        hipLaunchKernelGGL(stm::ola_loss_kernel<MAE()>, dim3((d->y + 255) / 256, d->B), dim3(256), 0, st_stream(stream),
                           frs, x, y_true, y_hat, dsyn, loss_partial, d->L, d->N, d->H, d->OT, d->y, inv,
                           frame_slabs(d), (size_t)d->B * d->OT * d->N, dsyn_pad, dsyn ? dsyn16 : nullptr, dsyn16 ? gemm_ht(d->prec) : 0); });
    ST_LAUNCHED("ola_loss");
    return ST_OK;
}
extern "C" int st_ola_loss(const st_dims* d, const float* frs, const float* x, const float* y_true,
                           float* y_hat, float* dsyn, float* loss_partial, void* stream)
{
    ST_TRY(check_dims(d)); ST_REQ(frs, "st_ola_loss: null pointer");
    return ola_loss_impl(d, frs, x, y_true, y_hat, dsyn, 0, loss_partial, stream);
}

// The 128 x 128-tile form (st_gemm_tn.h): fp32 products (ST_PREC_F32, and ST_PREC_F32X3 whose weight gradients stay on the fp32 MFMA), operands
// in the padded workspace layout, N a multiple of 256 (so that the F - 1 non-Nyquist bins of each basis are whole 128-row tiles)
static bool use_tn128(const st_dims* d, bool padded)
{
    const int ht = gemm_ht(d->prec);
    return g_tn128 && padded && (ht == 0 || (ht == 3 && !g_wg_split)) && d->N % 256 == 0 && g_wg_mode == 0;
}
// Frame-major reduction order (round 5): k -> frame t_lo + k / B, window k % B.  The operands keep their layout; only the strides swap roles and the
// origin moves to frame t_lo.  B >= 2 (the kernel divides by the inner count with a multiply-high); B = 1 keeps the window-major order (identical rows).
struct TNFrameMajor { stg::TNOperand a, b; stg::RowMap map; stg::FrameTrim trim; bool on; };
static TNFrameMajor tn_frame_major(const stg::TNOperand& ta, const stg::TNOperand& tb, const stg::RowMap& live, int B, int H, int Ntaps, int pad, int Ls, bool enable)
{
    TNFrameMajor f; f.on = enable && B >= 2 && fm_div_exact(live.Tv * B, B); f.a = ta; f.b = tb; f.map = live; f.trim = stg::FrameTrim{}; f.trim.on = 0;
    if (!f.on) return f;
    f.a = stg::TNOperand{ta.base + (size_t)live.t_lo * ta.S2, ta.S2, ta.S1};
    f.b = stg::TNOperand{tb.base + (size_t)live.t_lo * tb.S2, tb.S2, tb.S1};
    f.map.Tv = B; f.map.t_lo = 0; f.map.magic = stg::rowmap_magic(B); f.map.fm = 0;      // the kernel's (outer, inner) = (frame, window)
    f.trim = stg::frame_trim(live, B, H, Ntaps, pad, Ls);
    return f;
}
// g_tn128 == 2: the round-3 k-tile loop (st_set_tuning(9580)); otherwise the pipelined one (st_gemm_tn.h, round 7)
#define ST_TN128(...) do { if (g_tn128 == 2) ST_TRY((stg::launch_tn128<32, false>(__VA_ARGS__))); else ST_TRY((stg::launch_tn128<32, true>(__VA_ARGS__))); } while (0)
// ------------------------------------------------------------------------------ the weight-gradient GEMMs: plan, launch, slab sum
// Everything ONE weight-gradient GEMM and the sum of its slabs need, decided in one place (wgrad_plan; it launches nothing) for the per-op entries, the fused
// steps, the staged and data-parallel schedules, the pair launch and the host queries (st_wgrad_plan, st_wgrad_pair_plan).
// which: 0 = the analysis bases (A = d G, B = the padded x / 2, L samples): taps of the partly padded frames (Conv1d padding, cls_fe_dft.py:28-31) are zeros;
//        1 = the synthesis bases (A = the spectra, B = the padded d syn, y samples): taps of d syn's frames outside the crop are zeros.
// half = -1: both bases in one GEMM (M = KP output rows = columns of A); 0 / 1: only the real / imaginary basis of the analysis pair (rows [m0, m0 + KP / 2)),
// so that in data parallel the first basis' all-reduce runs under the second basis' GEMM (st_loss_backward_stage; st_dp_train_step, exchange flag 2: only F * N
// values -- 2.1 MB; 1.05 MB bf16-packed -- stay exposed behind the last GEMM of the step).
enum { WGP_PADDED = 1,         // operands in the padded workspace layout (the fused entries); else the per-op entries' unpadded signal
       WGP_G16 = 2,            // the call runs the 16-bit operand pipeline (WS::g16)
       WGP_HALVES_96 = 4 };    // st_loss_backward_stage: its one-basis launches stay on the 96 x 96 form (st_dp_train_step's take the 128 x 128 one where it applies)
struct WgOps { const float *A, *B; const unsigned short *A16, *B16; float in_scale; };      // in_scale: the per-op analysis entry's signal is x, not x / 2
struct WgradPlan {
    const st_dims* d; WgOps o; float* area;            // area: the slabs [ns][KP][N], the Nyquist partials behind them (st_wgrad_ws_floats)
    int which, half, flags, form, R, ns, m0, M, Ls;    // form: WG_*; R: live reduction rows; ns: k-slices = slabs; output rows [m0, m0 + M); Ls: samples of B's signal
    unsigned SA1, SB1; size_t slab;                    // window strides of the padded operands; slab stride
    stg::RowMap live;                                  // the frames with a tap inside the signal, window-major (all-zero frames contribute nothing)
    bool frame_major; stg::FrameTrim trim;             // round 5: reduction rows enumerated frame-major, and (trim.on) only the rows each tile column needs
    // The rows the 128-row tiles do not cover (the Nyquist bin of each basis).  nyq_P > 0: the slab sum takes them from nyq_P partials [2][N] at area + nyq_off
    // (whole tensor: right behind its ns slabs; one basis: behind all the slabs the area holds, where both halves find them); nyq_write: this launch forms them
    // (half 0 for BOTH bases -- its A origin is column 0 --, half 1 has no Nyquist slice)
    int nyq_P; size_t nyq_off; bool nyq_write;
    stg::TNOperand a, b; stg::RowMap map; stg::TNLaunch tn;      // WG_TN128: operands and rows as the kernel takes them, and its job (the pair launch joins two)
    size_t used() const { const size_t s = (size_t)ns * slab, q = nyq_P > 0 ? nyq_off + (size_t)nyq_P * 2 * d->N : 0; return s > q ? s : q; }
    stm::NyqJob nyq() const { stm::NyqJob q{}; q.on = nyq_P > 0 ? 1 : 0; if (q.on) { q.part = area + nyq_off; q.P = nyq_P; } return q; }
};
static WgradPlan wgrad_plan(const st_dims* d, int which, int half, int flags, const WgOps& o, float* area, int ncus = 0)
{
    const int KP = st_kp_of(d->F), N = d->N, Tf = which ? d->OT : d->T, room = wgrad_area_slabs(d);
    WgradPlan p; p.d = d; p.o = o; p.area = area; p.which = which; p.half = half; p.flags = flags;
    p.Ls = which ? d->y : d->L; p.live = stg::live_frames(Tf, d->H, N, N, p.Ls); p.R = p.live.rows(d->B);
    p.M = half < 0 ? KP : KP / 2; p.m0 = half > 0 ? KP / 2 : 0; p.slab = (size_t)KP * N;
    p.SA1 = (unsigned)(Tf * KP); p.SB1 = (unsigned)(p.Ls + 2 * N);
    const stg::TNOperand ta{o.A + p.m0, p.SA1, (unsigned)KP}, tb{o.B, p.SB1, (unsigned)d->H};
    const int Mt = half < 0 ? N : N / 2;               // rows the 128-row tiles cover: the F - 1 non-Nyquist bins of each basis
    if (flags & WGP_G16) p.form = WG_TN16;
    else p.form = (use_tn128(d, (flags & WGP_PADDED) != 0) && !(half >= 0 && (flags & WGP_HALVES_96)) &&
                   stg::tn128_fits(ta, tb, tb.base, p.live, Mt, N, (size_t)d->B * Tf * KP, (size_t)d->B * p.SB1)) ? WG_TN128 : WG_96;
    p.ns = wgrad_slices(p.form, half >= 0, p.R, KP, N, room, ncus);
    const bool fm = p.form == WG_TN128 ? (g_tn_fm & (which ? 1 : 2)) != 0 : p.form == WG_TN16 && (g_g16_crop & (which ? 4 : 8)) != 0;
    const TNFrameMajor f = tn_frame_major(ta, tb, p.live, d->B, d->H, N, N, p.Ls, fm);
    p.frame_major = f.on; p.trim = f.trim; p.a = f.a; p.b = f.b; p.map = f.map;
    p.nyq_P = 0; p.nyq_off = 0; p.nyq_write = false;
    if (p.form == WG_TN128) {
        p.nyq_off = (size_t)(half < 0 ? p.ns : room) * p.slab; p.nyq_write = half <= 0;
        p.tn = stg::tn128_job(32, p.a, p.b, tb.base, p.map, p.R, Mt, (N / 2) / 128, (unsigned)(KP / 2), N, area + (size_t)p.m0 * N, N, p.slab, p.ns,
                              p.nyq_write ? area + p.nyq_off : nullptr, (unsigned)(d->F - 1), (unsigned)(KP / 2 + d->F - 1), nullptr, &p.trim);
        p.nyq_P = p.tn.j.nyq_P;
    }
    return p;
}
// WG_TN16.  A: [rows (b, t)][KP] 16-bit (d G or the spectra), B: frames of a padded 16-bit signal whose first N elements are zero (the block of zeros)
static int wgrad_gemm16(const WgradPlan& p, void* stream)
{
    const st_dims* d = p.d; const stg::RowMap& map = p.live;
    const int KP = st_kp_of(d->F), R = p.R;
    const unsigned short *A = p.o.A16, *Bsig = p.o.B16, *lo = A < Bsig ? A : Bsig;
    const unsigned SA1 = p.SA1, SB1 = p.SB1;
    ST_REQ((size_t)(A - lo) + (size_t)R / map.Tv * SA1 + 256 < ((size_t)1 << 30) && (size_t)(Bsig - lo) + (size_t)R / map.Tv * SB1 + 256 < ((size_t)1 << 30) && map.Tv >= 2 &&
           SA1 < (1u << 23) && SB1 < (1u << 23), "16-bit weight-gradient GEMM: operands out of the 32-bit / 24-bit addressing range (B=%d)", d->B);
    stg::TN16Job j;
    j.base = lo; j.a0 = (unsigned)(A - lo) + (unsigned)p.m0; j.b0 = (unsigned)(Bsig - lo); j.zero = j.b0;
    j.SA1 = SA1; j.SA2 = (unsigned)KP; j.SB1 = SB1; j.SB2 = (unsigned)d->H;
    j.magic = map.magic; j.Tv = map.Tv; j.t_lo = map.t_lo; j.K = R;
    j.trim = 0; j.fB = 0; j.nsplit = 1;
    for (int i = 0; i < 64; ++i) { j.fa[i] = 0; j.fb[i] = 0; }
    if (p.frame_major) {
        // (outer, inner) = (frame, window): the strides swap roles, the origins move to frame t_lo (the zero block stays where it is)
        j.a0 += (unsigned)map.t_lo * (unsigned)KP; j.b0 += (unsigned)map.t_lo * (unsigned)d->H;
        j.SA1 = (unsigned)KP; j.SA2 = SA1; j.SB1 = (unsigned)d->H; j.SB2 = SB1;
        j.magic = stg::rowmap_magic(d->B); j.Tv = d->B; j.t_lo = 0;
        j.trim = p.trim.on; j.fB = d->B;
        for (int i = 0; i < 64; ++i) { j.fa[i] = p.trim.fa[i]; j.fb[i] = p.trim.fb[i]; }
    }
    stg::StoreC ep{p.area + (size_t)p.m0 * d->N, p.M, d->N, d->N, p.slab, stg::all_frames(1)};
    return with_ht16(gemm_ht(d->prec), [&](auto HT) { return stg::launch16_tn<HT(), 64>(j, ep, p.M, d->N, p.ns, st_stream(stream)); });
}
// The GEMM of a plan, whatever its form, into the plan's slabs
static int wgrad_gemm(const WgradPlan& p, void* stream)
{
    const st_dims* d = p.d; const int KP = st_kp_of(d->F), N = d->N;
    if (p.form == WG_TN128)
        ST_TN128(p.a, p.b, p.o.B, p.map, p.R, p.tn.M, p.tn.j.mh, p.tn.j.mstride, N, p.tn.out, N, p.slab, p.ns, st_stream(stream),
                 p.tn.j.nyq_out, p.tn.j.nyq_c0, p.tn.j.nyq_c1, nullptr, &p.trim);
    else if (p.form == WG_TN16) ST_TRY(wgrad_gemm16(p, stream));
    else {
        stg::PlainTN al{p.o.A + p.m0, p.R, KP, p.M, p.live};
        stg::StoreC ep{p.area + (size_t)p.m0 * N, p.M, N, N, p.slab, stg::all_frames(1)};
        if (p.flags & WGP_PADDED) { stg::FramedTN<true> bl{p.o.B, p.Ls, d->H, N, p.R, N, 1.0f, p.live}; ST_TRY(wgrad_small_gemm(d->prec, al, bl, ep, p.M, N, p.R, p.ns, st_stream(stream))); }
        else { stg::FramedTN<false> bl{p.o.B, p.Ls, d->H, N, p.R, N, p.o.in_scale, p.live}; ST_TRY(wgrad_small_gemm(d->prec, al, bl, ep, p.M, N, p.R, p.ns, st_stream(stream))); }
    }
    ST_LAUNCHED(p.which ? "synthesis_wgrad" : "analysis_wgrad");
    return ST_OK;
}
// The sum of a plan's slabs (and Nyquist partials) into the two gradient tensors, the |g| partials into `norm`, the live analysis rows also packed into `stage`
// where given: the ONE place that spells out wgrad_reduce_kernel's arguments.  Grid: the gradient rows of this plan, then its share of the Nyquist blocks resp.
// unused partial slots -- all of them for the whole tensor, each basis' own half for a one-basis plan.  On `s`: st_dp_train_step sums on its communicator stream.
static void wgrad_reduce(const WgradPlan& p, float* gRe, float* gIm, float* norm, float* stage, int stage_bf16, hipStream_t s)
{
    const st_dims* d = p.d; const int F = d->F, per = stm::nyq_blocks(d->N) / 2;
    const int nrows = p.half < 0 ? 2 * F : F, extra = p.half < 0 ? 2 * per : per;
    hipLaunchKernelGGL(stm::wgrad_reduce_kernel, dim3(nrows + extra), dim3(256), 0, s,
                       p.area, p.ns, gRe, gIm, norm, d->N, F, st_kp_of(F), p.which, p.half > 0 ? F : 0, nrows, stage, p.nyq(), p.half > 0 ? per : 0, stage_bf16);
}
static int wgrad_gemm_and_sum(const WgradPlan& p, float* gRe, float* gIm, float* norm, float* stage, int stage_bf16, void* stream)
{
    ST_TRY(wgrad_gemm(p, stream));
    wgrad_reduce(p, gRe, gIm, norm, stage, stage_bf16, st_stream(stream));
    ST_LAUNCHED(p.which ? "synthesis_wgrad_reduce" : "analysis_wgrad_reduce");
    return ST_OK;
}
extern "C" int st_synthesis_wgrad(const st_dims* d, const float* AA, const float* dsyn, float* ws,
                                  float* gSr, float* gSi, float* norm_partial, void* stream)
{
    ST_TRY(check_dims(d)); ST_REQ(AA && dsyn && ws && gSr && gSi && norm_partial, "st_synthesis_wgrad: null pointer");
    return wgrad_gemm_and_sum(wgrad_plan(d, 1, -1, 0, WgOps{AA, dsyn, nullptr, nullptr, 1.0f}, ws), gSr, gSi, norm_partial, nullptr, 0, stream);
}


// ------------------------------------------------------------------------------ wide-geometry autoencoders (st_ae_wide.h)
// The arithmetic a call REALLY runs.  Since round 5 that is the request for every geometry and batch; the entry stays so that callers (and the tests) can
// keep asserting it instead of assuming it.
extern "C" int st_effective_prec(const st_dims* d)
{
    if (!d) return -1;
    return d->prec;
}
// BM = 64, k-tile 16 (every K below is a multiple of 16 or checked).  Level-2 precision: the 16-bit kernel (k-tile 32: W1 is padded to a multiple of 32
// columns).  The weight-gradient GEMMs reduce over the R = B * 528 columns: a multiple of 32 for even batches; for ODD batches (R = 16 mod 32) they run
// the same kernel on 16-deep k-tiles (round 5) -- until round 4 an odd batch dropped the whole wide path to fp32 layers (and said so: st_effective_prec),
// the last place where the arithmetic of a call depended on its batch size.  wide_ht, the first argument of wgemm_pair: 0 fp32 / 1 bf16 / 2 fp16.
// the same GEMM for both autoencoders: ONE launch in the 16-bit configurations (gemm_half_pair_kernel), two on the fp32 kernel
template <class AL, class BL, class EPI>
static void wgemm_pair(int wide_ht, const AL& a0, const BL& b0, const EPI& e0, const AL& a1, const BL& b1, const EPI& e1, int M, int Nc, int K, int ns, hipStream_t s)
{
    if (wide_ht) with_ht16(wide_ht, [&](auto HT) { stg::launch_half_pair<2, HT()>(a0, b0, e0, a1, b1, e1, M, Nc, K, ns, s); });
    else { stg::launch<2, 16>(a0, b0, e0, M, Nc, K, ns, s); stg::launch<2, 16>(a1, b1, e1, M, Nc, K, ns, s); }
}
// The four pad jobs of the wide path's side work (stw::PadJobs): W1 of either net padded to Tp columns, W5 to 32.  Returns their block count.
static int fill_pad_jobs(stw::PadJobs& pj, const st_dims* d, const Layout& L, const float* ae_m, const float* ae_p, const WideWS& w)
{
    int blk = 0;
    for (int a = 0; a < 2; ++a) {
        const float* ae = a ? ae_p : ae_m;
        pj.src[2 * a] = ae + L.go.w[0]; pj.dst[2 * a] = w.W1p[a]; pj.rows[2 * a] = 64; pj.cols[2 * a] = d->T; pj.pitch[2 * a] = w.Tp;
        pj.blk0[2 * a] = blk; blk += (64 * w.Tp + 255) / 256;
        pj.src[2 * a + 1] = ae + L.go.w[4]; pj.dst[2 * a + 1] = w.W5p[a]; pj.rows[2 * a + 1] = 16; pj.cols[2 * a + 1] = 16 + d->K; pj.pitch[2 * a + 1] = 32;
        pj.blk0[2 * a + 1] = blk; blk += 2;
    }
    pj.blk0[4] = blk;
    return blk;
}
static int ae_wide_fwd(const st_dims* d, const Layout& L, const float* mag, const float* phs, const float* knobs,
                       const float* ae_m, const float* ae_p, float* mag_hat, float* phs_hat, float* AA, float* reg_partial,
                       WideWS& w, void* stream, unsigned short* AA16, bool in_done)
{
    hipStream_t s = st_stream(stream);
    const int FP = L.KP / 2, F = d->F, T = d->T, OT = d->OT, R = (int)w.R, Tp = w.Tp;
    const int wide_ht = ae_ht(d->prec);
    ST_REQ(w.R * (size_t)(T > 64 ? T : 64) < ((size_t)1 << 30), "wide autoencoder path: batch too large (B=%d)", d->B);
    const stg::RowMap id = stg::all_frames(1);
    int out[9], in[9]; ae_shapes(d, out, in);
    if (!in_done) {      // the fused step's analysis GEMM wrote V itself and prep_kernel did the side jobs (round 4); the per-op entry copies here
        stw::PadJobs pj; const int blk = fill_pad_jobs(pj, d, L, ae_m, ae_p, w);
        ST_REQ(FP % 4 == 0 && (size_t)(T + d->K) * d->B * (FP / 4) < ((size_t)1 << 31), "wide autoencoder path: batch too large (B=%d)", d->B);
        const int n_copy = (int)(((size_t)(T + d->K) * d->B * (FP / 4) + 255) / 256);
        hipLaunchKernelGGL(stw::wide_in_kernel, dim3(n_copy + blk), dim3(256), 0, s, mag, phs, knobs, w.V[0], w.V[1], w.H[0][3], w.H[1][3],
                           d->B, T, F, FP, d->K, n_copy, pj);
        ST_LAUNCHED("ae_wide_in");
    }
    // layers 1..8: GEMM for layer 1 (K = T), layers 2..8 in one fused kernel for both nets
    {
        stg::PlainNT al0{w.W1p[0], out[0], Tp, Tp, id}, al1{w.W1p[1], out[0], Tp, Tp, id};
        stg::PlainTN bl0{w.V[0], in[0], R, R, id}, bl1{w.V[1], in[0], R, R, id};
        stw::ActStore ep0{w.H[0][0], ae_m + L.go.b[0], out[0], R, FP, F}, ep1{w.H[1][0], ae_p + L.go.b[0], out[0], R, FP, F};
        wgemm_pair(wide_ht, al0, bl0, ep0, al1, bl1, ep1, out[0], R, Tp, 1, s);
    }
    {
        const size_t lds = (size_t)2 * sta::CL::FWD_TOTAL * sizeof(float);
        ST_TRY(with_ht(wide_ht, [&](auto HT) { return with_inner_nw(ae_inner_nw(d), [&](auto NW) {
            return launch_lds("ae_inner_fwd_kernel", sta::ae_inner_fwd_kernel<NW(), HT()>, dim3(ae_inner_grid(d)), dim3(NW() * 64), lds, s,
                              w.H[0][0], w.H[1][0], knobs, ae_m, ae_p, L.go, w.H[0][7], w.H[1][7], d->B, F, d->K, L.KP); }); }));
    }
    {
        stg::PlainNT al0{ae_m + L.go.w[8], OT, 64, 64, id}, al1{ae_p + L.go.w[8], OT, 64, 64, id};
        stg::PlainTN bl0{w.H[0][7], 64, R, R, id}, bl1{w.H[1][7], 64, R, R, id};
        stw::OutStore ep0{w.E9[0], mag_hat, w.V[0] + (size_t)(T - OT) * R, ae_m + L.go.b[8], OT, R, FP, F, 0};
        stw::OutStore ep1{w.E9[1], phs_hat, w.V[1] + (size_t)(T - OT) * R, ae_p + L.go.b[8], OT, R, FP, F, 1};
        wgemm_pair(wide_ht, al0, bl0, ep0, al1, bl1, ep1, OT, R, 64, 1, s);
    }
    ST_LAUNCHED("ae_wide_fwd");
    if (AA) {
        hipLaunchKernelGGL(stw::wide_polar_out_kernel, dim3(ae_fwd_partials(d)), dim3(256), 0, s, mag_hat, phs_hat, AA, reg_partial,
                           d->B, OT, F, FP, L.KP, expfac_of(d), AA16, AA16 ? gemm_ht(d->prec) : 0);
        ST_LAUNCHED("ae_wide_polar_out");
    }
    return ST_OK;
}

// one weight-gradient GEMM of the wide path for both nets: dW_l (+ bias via the ones row) as split-K slabs.  In the one 16-bit launch net 1's slabs follow net 0's
// (slab z of the pair launch = net * nsplit + slice), so both epilogues share one origin
static void wide_wgrad_pair(const st_dims* d, WideWS& w, int l, const int* out, const int* in, hipStream_t s, const int wide_ht)
{
    const int R = (int)w.R;
    const stg::RowMap id = stg::all_frames(1);
    stg::PlainNT al0{w.DA[0][l], out[l], R, R, id}, al1{w.DA[1][l], out[l], R, R, id};
    stg::PlainNT bl0{l == 0 ? w.V[0] : w.H[0][l - 1], in[l] + 1, R, R, id}, bl1{l == 0 ? w.V[1] : w.H[1][l - 1], in[l] + 1, R, R, id};
    stg::StoreC ep0{w.slabs + w.so[l], out[l], in[l] + 1, in[l] + 1, w.SL, id};
    stg::StoreC ep1 = ep0;
    if (!wide_ht) ep1.out = w.slabs + (size_t)w.nsplit * w.SL + w.so[l];      // two launches: each with its own z = 0 .. nsplit - 1
    if (wide_ht && R % 32) {      // odd batch: the reduction length is 16 mod 32 -> 16-deep k-tiles of the same kernel
        with_ht16(wide_ht, [&](auto HT) { stg::launch_half_pair<2, HT(), 1, 16>(al0, bl0, ep0, al1, bl1, ep1, out[l], in[l] + 1, R, w.nsplit, s); });
        return;
    }
    wgemm_pair(wide_ht, al0, bl0, ep0, al1, bl1, ep1, out[l], in[l] + 1, R, w.nsplit, s);
}

// Where the gradient w.r.t. the autoencoder inputs goes on the fused path: straight through the polar backward into d G (wide_dv_polar_kernel)
struct PolarSink { const float* re; const float* im; const float* g_mag; float* dG; unsigned short* dG16; };
static int ae_wide_bwd(const st_dims* d, const Layout& L, const float* mag, const float* phs, const float* knobs,
                       const float* ae_m, const float* ae_p, const float* mag_hat, const float* phs_hat, const float* dAA,
                       const float* g_mag_hat, float reg_coef, float* dmag, float* dphs, WideWS& w, float* g_m, float* g_p,
                       bool have_fwd, void* stream, const PolarSink* sink = nullptr,
                       const stw::SynReduce* syn = nullptr, float* norm_e = nullptr, int* n_norm_e = nullptr, float* kg = nullptr, bool no_dinput = false)
{   // no_dinput (st_train_step_groups, analysis bases frozen): the layer-1 data gradient + polar backward launch at the end is left out
    // kg (st_model_bwd_knobs): the fused kernel of layers 2..8 also writes the per-group column sums of d a5 there
    hipStream_t s = st_stream(stream);
    const int FP = L.KP / 2, F = d->F, T = d->T, OT = d->OT, R = (int)w.R;
    const int wide_ht = ae_ht(d->prec);
    const stg::RowMap id = stg::all_frames(1);
    int out[9], in[9]; ae_shapes(d, out, in);
    // forward state (activations + ELU outputs of layer 9): recomputed into the workspace unless the fused step's own
    // forward just left it there (same workspace, same layout); no user-visible outputs
    if (!have_fwd) ST_TRY(ae_wide_fwd(d, L, mag, phs, knobs, ae_m, ae_p, nullptr, nullptr, nullptr, nullptr, w, stream));
    stw::OnesRows rows;
    for (int a = 0; a < 2; ++a) {
        rows.p[9 * a] = w.V[a] + (size_t)in[0] * R;
        for (int j = 0; j < 8; ++j) rows.p[9 * a + 1 + j] = w.H[a][j] + (size_t)in[j + 1] * R;
    }
    const float expfac = expfac_of(d);
    const stg::RowMap ms = synth_live(d);
    {
        const size_t n = (size_t)d->B * OT * FP;
        ST_REQ(n < ((size_t)1 << 30), "wide autoencoder path: batch too large (B=%d)", d->B);
        int grid = (int)((n + 255) / 256); if (grid > 8192) grid = 8192;
        hipLaunchKernelGGL(stw::wide_dout_kernel, dim3(grid + 18 * d->B), dim3(256), 0, s, dAA, synth_slabs(d), (size_t)d->B * OT * L.KP,
                           mag_hat, phs_hat, w.E9[0], w.E9[1], w.V[0] + (size_t)(T - OT) * R, g_mag_hat, reg_coef, expfac,
                           w.DA[0][8], w.DA[1][8], w.TL[0], w.TL[1], d->B, OT, F, FP, L.KP, ms.t_lo, ms.t_lo + ms.Tv - 1, grid, rows);
        ST_LAUNCHED("ae_wide_dout");
    }
    stw::GradTab tab;
    for (int l = 0; l < 9; ++l) { tab.so[l] = w.so[l]; tab.out[l] = out[l]; tab.in[l] = in[l]; tab.gw[l] = L.go.w[l]; tab.gb[l] = L.go.b[l]; }
    tab.so[9] = w.so[9];
    int inner_parts = 0;
    // layer 9 as GEMMs, layers 8..2 in one fused kernel (both nets), layer 1 as GEMMs
    wide_wgrad_pair(d, w, 8, out, in, s, wide_ht);
    {   // d H8 = W9^T d A9 of both nets (the fused kernel applies ELU')
        stg::PlainTN al0{ae_m + L.go.w[8], out[8], in[8], in[8], id}, al1{ae_p + L.go.w[8], out[8], in[8], in[8], id};
        stg::PlainTN bl0{w.DA[0][8], out[8], R, R, id}, bl1{w.DA[1][8], out[8], R, R, id};
        stg::StoreC ep0{w.DA[0][7], in[8], R, R, 0, id}, ep1{w.DA[1][7], in[8], R, R, 0, id};
        wgemm_pair(wide_ht, al0, bl0, ep0, al1, bl1, ep1, in[8], R, out[8], 1, s);
    }
    {
        const size_t lds = (size_t)sta::ae_bwd_lds_floats(AE_BWD_NW) * sizeof(float);
        const int grid = ae_bwd_grid(d);
        ST_TRY(with_ht(wide_ht, [&](auto HT) { return with_bool(kg != nullptr, [&](auto KG) {
            return launch_lds("ae_bwd_kernel", sta::ae_bwd_kernel<AE_BWD_NW, true, HT(), 0, false, KG()>, dim3(grid, 2), dim3(AE_BWD_NW * 64), lds, s,
                              w.H[0][0], w.H[1][0], knobs, ae_m, ae_p, L.go, L.PG, w.DA[0][7], w.DA[1][7], nullptr, nullptr, 0.f, 0.f,
                              w.DA[0][0], w.DA[1][0], w.inner_ws, d->B, T, OT, F, d->K, L.KP, 0, 0, 1, (size_t)0, nullptr, kg, nullptr); }); }));
        inner_parts = grid;                          // summed by the second role of wide_grad_finish_kernel below (was a launch of its own)
    }
    for (int l = 1; l < 8; ++l) tab.out[l] = 0;                 // the finish kernel only scatters layers 1 and 9
    wide_wgrad_pair(d, w, 0, out, in, s, wide_ht);
    if (norm_e && 2 * ((w.so[9] + 63) / 64 + (L.PG + 63) / 64) > NORM_E_MAX) norm_e = nullptr;
    hipLaunchKernelGGL(stw::wide_grad_finish_kernel, dim3((w.so[9] + 63) / 64 + (L.PG + 63) / 64 + (syn ? norm_partials(d) : 0), 2), dim3(256), 0, s, w.slabs, w.nsplit, w.SL, tab, g_m, g_p,
                       (w.so[9] + 63) / 64, (const float*)w.inner_ws, inner_parts, L.PG, syn ? *syn : stw::SynReduce{}, norm_e);
    if (norm_e && n_norm_e) *n_norm_e = 2 * ((w.so[9] + 63) / 64 + (L.PG + 63) / 64);
    if (no_dinput) { ST_LAUNCHED("ae_wide_bwd_noin"); return ST_OK; }
    {   // layer-1 data gradient + polar backward of both nets in one kernel
        stw::DvPolarArgs q;
        q.DA1m = w.DA[0][0]; q.DA1p = w.DA[1][0]; q.TLm = w.TL[0]; q.TLp = w.TL[1]; q.W1m = ae_m + L.go.w[0]; q.W1p = ae_p + L.go.w[0];
        q.re = sink ? sink->re : nullptr; q.im = sink ? sink->im : nullptr; q.g_mag = sink ? sink->g_mag : nullptr;
        q.dG = sink ? sink->dG : nullptr; q.dG16 = sink ? sink->dG16 : nullptr;
        q.dmag = sink ? nullptr : dmag; q.dphs = sink ? nullptr : dphs;          // fused step: d mag / d phs never leave the kernel
        q.ht = gemm_ht(d->prec) <= 2 ? gemm_ht(d->prec) : 0; q.sat = gemm_ht(d->prec) == 2 ? 65504.0f : 0.0f;
        q.B = d->B; q.T = T; q.OT = OT; q.F = F; q.FP = FP; q.KP = L.KP;
        const int TP16 = (T + 15) / 16 * 16, groups = d->B * (FP / 16);
        ST_REQ(TP16 <= 192, "wide autoencoder path: T = %d frames exceeds the layer-1 data-gradient kernel's 192", T);
        const size_t lds = (size_t)2 * (wide_ht ? 32 : 64) * TP16 * sizeof(float);          // 16-bit images take half the room
        int grid = ((groups + 7) / 8) * (TP16 / 16); if (grid > num_cus()) grid = num_cus();      // units of (8 adjacent groups, 16-frame tile), shared equally; one workgroup per CU
                                                                                                  // (two or three per CU measured slower: 146.6 / 155.5 us against 141.1 for the whole
                                                                                                  // wide backward -- every workgroup stages the layer-1 weights, ~10 us of dependent loads)
        ST_TRY(with_ht(wide_ht, [&](auto HT) { return launch_lds("wide_dv_polar_kernel", stw::wide_dv_polar_kernel<HT()>, dim3(grid), dim3(512), lds, s, q); }));
    }
    ST_LAUNCHED("ae_wide_bwd");
    return ST_OK;
}

static int ae_bwd_body(const st_dims* d, const Layout& L, const float* mag, const float* phs, const float* knobs,
                       const float* ae_m, const float* ae_p, const float* mag_hat, const float* phs_hat,
                       const float* dAA, const float* g_mag_hat, float reg_coef, float* dmag, float* dphs, float* ws,
                       float* g_m, float* g_p, bool have_fwd, void* stream, bool* defer_reduce = nullptr,
                       const PolarSink* sink = nullptr, const stw::SynReduce* syn = nullptr, float* norm_e = nullptr, int* n_norm_e = nullptr,
                       float* kg = nullptr, bool have_img = false, bool no_dinput = false)
{
    // no_dinput (st_train_step_groups, analysis bases frozen): nothing reads d mag / d phs.  The fused geometries' kernel runs as its NOIN instantiation;
    // the split 16-bit kernels and the wide path's fused inner kernel keep forming the input gradient (the wide path drops its layer-1 data-gradient + polar launch)
    // have_img: the forward of this workspace was a fused one whose prep_kernel left the weight images there (ae_img_ptr)
    // kg (st_model_bwd_knobs): the kernel that holds d a5 also writes its per-group column sums there ([net][group][16]); only the instantiations the shipped
    // tuning defaults reach exist in that form (ae_kg_route)
    // defer_reduce: in -> the caller will sum the workgroup partials itself (post_ae_kernel, together with the polar backward);
    // out -> false if this geometry's path already reduced them (wide geometries)
    ST_REQ(mag && phs && (knobs || d->K == 0) && ae_m && ae_p && mag_hat && phs_hat && dAA && dmag && dphs && ws && g_m && g_p, "st_ae_bwd: null pointer");
    if (!knobs) knobs = ae_m;
    if (ae_is_wide(d)) {
        if (defer_reduce) *defer_reduce = false;
        WideWS w; wide_carve(d, L, ws, &w);
        return ae_wide_bwd(d, L, mag, phs, knobs, ae_m, ae_p, mag_hat, phs_hat, dAA, g_mag_hat, reg_coef, dmag, dphs, w, g_m, g_p, have_fwd, stream, sink, syn, norm_e, n_norm_e, kg, no_dinput);
    }
    ST_REQ(!no_dinput || (!kg && !g_mag_hat), "st_ae_bwd: the form without the input gradient takes neither an upstream d mag_hat nor the knob-gradient output");
    if (kg && !(ae_kg_route(d) && have_fwd)) return st_fail(ST_ERR_UNSUPPORTED, "st_ae_bwd: no per-group d a5 output on this autoencoder backward route (%s)", ae_kg_why(d));
    const size_t lds = (size_t)sta::ae_bwd_lds_floats(AE_BWD_NW) * sizeof(float);
    static_assert((size_t)sta::ae_bwd_lds_floats(AE_BWD_NW) * sizeof(float) <= 160 * 1024, "ae_bwd LDS budget");
    ST_REQ((size_t)synth_slabs(d) * d->B * d->OT * L.KP < ((size_t)1 << 30) && (size_t)d->B * d->T * L.KP < ((size_t)1 << 30),
           "st_ae_bwd: batch too large for the kernel's 32-bit element offsets (B=%d)", d->B);
    const float expfac = expfac_of(d);
    const stg::RowMap live = synth_live(d);
    const int t_hi = live.t_lo + live.Tv - 1, nsl = synth_slabs(d);
    const size_t slab = (size_t)d->B * d->OT * L.KP;
    hipStream_t s = st_stream(stream);
    float* h4x = ws;                                      // workspace: [h4 | d a4 | workgroup partials] (st_ae_bwd_ws_floats)
    float* da4x = ws + ae_h4_floats(d);
    float* parts = ws + 2 * ae_h4_floats(d);
    int grid = ae_bwd_grid(d);
    const int ht = ae_ht(d->prec);
    if (ae_use_split(d)) {
        // two kernels at two waves per SIMD (st_ae_split.h): decoder half (layers 5..9, from the code h4 the forward kernel kept),
        // then encoder half (layers 1..4, from d a4 and the tails the first one left)
        if (!have_fwd)                                     // per-op entry without a preceding forward in this workspace: code-only forward pass
            ST_TRY(ae_fwd_body(d, L, mag, phs, knobs, ae_m, ae_p, nullptr, nullptr, nullptr, nullptr, h4x, stream));
        grid = ae_split_grid(d);
        static_assert((size_t)sta::ae_split_lds_floats<1>(AE_SPLIT_NW) * sizeof(float) <= 160 * 1024 && (size_t)sta::ae_split_lds_floats<2>(AE_SPLIT_NW) * sizeof(float) <= 160 * 1024, "split ae_bwd LDS budget");
        auto part = [&](auto PART, auto HT, auto GM, auto KG) {
            return launch_lds("ae_bwd_part_kernel", sta::ae_bwd_part_kernel<AE_SPLIT_NW, PART(), HT(), GM(), KG()>, dim3(grid, 2), dim3(AE_SPLIT_NW * 64),
                              (size_t)sta::ae_split_lds_floats<PART()>(AE_SPLIT_NW) * sizeof(float), s,
                              mag, phs, knobs, ae_m, ae_p, L.go, L.PG, mag_hat, phs_hat, dAA, g_mag_hat, reg_coef, expfac, dmag, dphs, parts,
                              h4x, da4x, d->B, d->T, d->OT, d->F, d->K, L.KP, live.t_lo, t_hi, nsl, slab, kg); };
        auto halves = [&](auto HT, auto KG) -> int {      // KG: the decoder half (it holds d a5) also writes the per-group sums
            ST_TRY(with_bool(g_mag_hat != nullptr, [&](auto GM) { return part(ic<1>{}, HT, GM, KG); }));
            ST_LAUNCHED("ae_bwd_dec");
            ST_TRY(part(ic<2>{}, HT, std::false_type{}, std::false_type{}));
            ST_LAUNCHED("ae_bwd_enc");
            return ST_OK; };
        if (kg) ST_TRY(with_ht16(ht, [&](auto HT) { return halves(HT, std::true_type{}); }));      // 16-bit layers only (ae_kg_route)
        else ST_TRY(with_ht(ht, [&](auto HT) { return halves(HT, std::false_type{}); }));
    } else {
        // kernel variant: 1 = an upstream d/d mag_hat arrives (autograd entry), 2 = T - OT == 16 (tails already in registers), 0 = neither
        const int var = g_mag_hat ? 1 : (d->T - d->OT == 16 ? 2 : 0);
        if (no_dinput) {                                  // VAR 0 / 2 only (no upstream d mag_hat), no per-group d a5 output
            if (have_fwd && ae_use_saved(d)) {
                const float* sv = ae_sv_ptr(d, L, ws);
                const float* img = (have_img && ae_img_level(d) == 2) ? ae_img_ptr(ws) : nullptr;
                ST_TRY(with_bool(var == 2, [&](auto T16) { return with_bool(img != nullptr, [&](auto IMG) {
                    return launch_lds("ae_bwd_kernel", sta::ae_bwd_kernel<AE_BWD_NW, false, 0, T16() ? 2 : 0, true, false, IMG(), true>, dim3(grid, 2), dim3(AE_BWD_NW * 64), lds, s,
                                      mag, phs, knobs, ae_m, ae_p, L.go, L.PG, mag_hat, phs_hat, dAA, g_mag_hat, reg_coef, expfac,
                                      dmag, dphs, parts, d->B, d->T, d->OT, d->F, d->K, L.KP, live.t_lo, t_hi, nsl, slab, sv, kg, img); }); }));
            } else
                ST_TRY(with_ht(ht, [&](auto HT) { return with_bool(var == 2, [&](auto T16) {
                    return launch_lds("ae_bwd_kernel", sta::ae_bwd_kernel<AE_BWD_NW, false, HT(), T16() ? 2 : 0, false, false, false, true>, dim3(grid, 2), dim3(AE_BWD_NW * 64), lds, s,
                                      mag, phs, knobs, ae_m, ae_p, L.go, L.PG, mag_hat, phs_hat, dAA, g_mag_hat, reg_coef, expfac,
                                      dmag, dphs, parts, d->B, d->T, d->OT, d->F, d->K, L.KP, live.t_lo, t_hi, nsl, slab, nullptr, nullptr, nullptr); }); }));
        } else
        if (have_fwd && ae_use_saved(d)) {               // round 6: the forward of this workspace kept the activations -- no recompute (fp32 layers only)
            const float* sv = ae_sv_ptr(d, L, ws);
            const float* img = (have_img && ae_img_level(d) == 2) ? ae_img_ptr(ws) : nullptr;
            ST_TRY(with_var(var, [&](auto VAR) { return with_bool(kg != nullptr, [&](auto KG) { return with_bool(img != nullptr, [&](auto IMG) {
                return launch_lds("ae_bwd_kernel", sta::ae_bwd_kernel<AE_BWD_NW, false, 0, VAR(), true, KG(), IMG()>, dim3(grid, 2), dim3(AE_BWD_NW * 64), lds, s,
                                  mag, phs, knobs, ae_m, ae_p, L.go, L.PG, mag_hat, phs_hat, dAA, g_mag_hat, reg_coef, expfac,
                                  dmag, dphs, parts, d->B, d->T, d->OT, d->F, d->K, L.KP, live.t_lo, t_hi, nsl, slab, sv, kg, img); }); }); }));
        } else
            ST_TRY(with_ht(ht, [&](auto HT) { return with_var(var, [&](auto VAR) {
                return launch_lds("ae_bwd_kernel", sta::ae_bwd_kernel<AE_BWD_NW, false, HT(), VAR()>, dim3(grid, 2), dim3(AE_BWD_NW * 64), lds, s,
                                  mag, phs, knobs, ae_m, ae_p, L.go, L.PG, mag_hat, phs_hat, dAA, g_mag_hat, reg_coef, expfac,
                                  dmag, dphs, parts, d->B, d->T, d->OT, d->F, d->K, L.KP, live.t_lo, t_hi, nsl, slab, nullptr, nullptr, nullptr); }); }));
        ST_LAUNCHED("ae_bwd");
    }
    if (defer_reduce && *defer_reduce) return ST_OK;
    hipLaunchKernelGGL(stm::ae_grad_reduce_kernel, dim3((L.PG + 63) / 64, 2), dim3(256), 0, s, parts, grid, L.PG, g_m, g_p);
    ST_LAUNCHED("ae_grad_reduce"); return ST_OK;
}
extern "C" int st_ae_bwd(const st_dims* d, const float* mag, const float* phs, const float* knobs,
                         const float* ae_m, const float* ae_p, const float* mag_hat, const float* phs_hat,
                         const float* dAA, const float* g_mag_hat, float reg_coef, float* dmag, float* dphs, float* ws,
                         float* g_m, float* g_p, void* stream)
{
    Layout L; ST_TRY(make_layout(d, &L));
    return ae_bwd_body(d, L, mag, phs, knobs, ae_m, ae_p, mag_hat, phs_hat, dAA, g_mag_hat, reg_coef, dmag, dphs, ws, g_m, g_p, false, stream);
}

extern "C" int st_polar_bwd(const st_dims* d, const float* re, const float* im, const float* dmag, const float* dphs,
                            const float* g_mag, float* dG, void* stream)
{
    ST_TRY(check_dims(d)); ST_REQ(re && im && dmag && dphs && dG, "st_polar_bwd: null pointer");
    const int R = d->B * d->T, KP = st_kp_of(d->F);
    hipLaunchKernelGGL(stm::polar_bwd_kernel, dim3((KP / 2 + 255) / 256, R), dim3(256), 0, st_stream(stream),
                       re, im, dmag, dphs, g_mag, dG, R, d->F, KP, gemm_ht(d->prec) == 2 ? 65504.0f : 0.0f);
    ST_LAUNCHED("polar_bwd"); return ST_OK;
}

extern "C" int st_analysis_wgrad(const st_dims* d, const float* dG, const float* x, float in_scale, float* ws,
                                 float* gWr, float* gWi, float* norm_partial, void* stream)
{
    ST_TRY(check_dims(d)); ST_REQ(dG && x && ws && gWr && gWi && norm_partial, "st_analysis_wgrad: null pointer");
    return wgrad_gemm_and_sum(wgrad_plan(d, 0, -1, 0, WgOps{dG, x, nullptr, nullptr, in_scale}, ws), gWr, gWi, norm_partial, nullptr, 0, stream);
}

static stm::FinArgs fin_args(const st_dims* d, const float* loss_partial, const float* reg_partial, const float* norm_a, const float* norm_s, float norm_scale)
{
    const float inv_y = 1.0f / ((float)d->B * (float)d->y);
    return stm::FinArgs{loss_partial, ola_loss_partials(d), reg_partial, ae_fwd_partials(d),
                        norm_a, norm_partials(d), norm_s, norm_s ? norm_partials(d) : 0, inv_y, reg_scale_of(d), norm_scale, nullptr, 0};
}
static int finalize_scalars(const st_dims* d, const float* loss_partial, const float* reg_partial,
                            const float* norm_a, const float* norm_s, float inv_world, float* scalars, void* stream)
{
    ST_REQ(scalars, "st_finalize_scalars: null pointer");
    stm::FinArgs f = fin_args(d, loss_partial, reg_partial, norm_a, norm_s, inv_world);
    f.n_ns = norm_partials(d);      // counted whether or not norm_s is given, as this entry always has
    hipLaunchKernelGGL(stm::finalize_kernel, dim3(1), dim3(256), 0, st_stream(stream), f, scalars);
    ST_LAUNCHED("finalize_scalars"); return ST_OK;
}
extern "C" int st_finalize_scalars(const st_dims* d, const float* loss_partial, const float* reg_partial,
                                   const float* norm_a, const float* norm_s, float inv_world, float* scalars, void* stream)
{
    ST_TRY(check_dims(d));
    return finalize_scalars(d, loss_partial, reg_partial, norm_a, norm_s, inv_world, scalars, stream);
}

// fin != nullptr: the clip coefficient (and, if fin->loss_partial, the loss scalars) are derived inside the kernel from
// the partial sums -- no separate finalize launch; `scalars` is then an output.
static int clip_adam_impl(float* params, float* grads, float* m, float* v, int64_t n_total, int64_t n_stft /* clipped range */,
                          float* scalars, float grad_scale, float lr, float beta1, float beta2, float eps, int step,
                          const stm::FinArgs* fin, void* stream, bool dev_hyper = false)
{
    ST_REQ(params && grads && m && v && scalars, "st_clip_adam: null pointer");
    ST_REQ(n_total > 0, "st_clip_adam: n_total must be positive (an empty range would be a zero-block launch)");
    ST_REQ(n_stft >= 0, "st_clip_adam: n_stft must not be negative");
    ST_REQ(n_total % 4 == 0 && n_stft % 4 == 0, "st_clip_adam: n_total and n_stft must be multiples of 4");
    ST_REQ(n_stft <= n_total, "st_clip_adam: n_stft exceeds n_total");
    ST_REQ(step >= 1, "st_clip_adam: step must be at least 1");
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    const float neg_step = (float)(-(double)lr / bc1);
    const float bc2s = (float)sqrt(bc2);
    const float w1 = (float)(1.0 - (double)beta1), w2 = (float)(1.0 - (double)beta2);
    int grid = (int)((n_total / 4 + 255) / 256); if (grid > 2048) grid = 2048;
    if (dev_hyper) {          // step number and learning rate from scalars[6], scalars[7] (captured step, st_graph_*)
        ST_REQ(fin, "device-side hyper-parameters need the fused finalize");
        hipLaunchKernelGGL((stm::clip_adam_kernel<true, true>), dim3(grid), dim3(256), 0, st_stream(stream),
                           params, grads, m, v, n_total / 4, n_stft / 4, scalars, grad_scale, 0.f, w1, beta2, w2, 1.f, eps, *fin, beta1);
    } else if (fin)
        hipLaunchKernelGGL(stm::clip_adam_kernel<true>, dim3(grid), dim3(256), 0, st_stream(stream),
                           params, grads, m, v, n_total / 4, n_stft / 4, scalars, grad_scale, neg_step, w1, beta2, w2, bc2s, eps, *fin);
    else
        hipLaunchKernelGGL(stm::clip_adam_kernel<false>, dim3(grid), dim3(256), 0, st_stream(stream),
                           params, grads, m, v, n_total / 4, n_stft / 4, scalars, grad_scale, neg_step, w1, beta2, w2, bc2s, eps, stm::FinArgs{});
    ST_LAUNCHED("clip_adam"); return ST_OK;
}
extern "C" int st_clip_adam(float* params, float* grads, float* m, float* v, int64_t n_total, int64_t n_stft,
                            const float* scalars, float grad_scale, float lr, float beta1, float beta2, float eps, int step,
                            void* stream)
{
    return clip_adam_impl(params, grads, m, v, n_total, n_stft, const_cast<float*>(scalars), grad_scale, lr, beta1, beta2, eps, step, nullptr, stream);
}

// ------------------------------------------------------------------------------ workspace
struct WS {
    // dAA, frs: NOT every element is written per step (the pitch-padding columns [F, FP) of dAA's halves, the all-cropped tiles of frs): no consumer may read those -- the
    // contract is stated at st_workspace_bytes in the header; the Python engine zero-fills the buffer once when it allocates it
    float *re, *im, *mag, *phs, *mag_hat, *phs_hat, *AA, *dAA, *Sfold, *SfoldT, *frs, *y_hat, *dsyn, *dmag, *dphs, *dG, *xp;
    float *wg, *wg2, *aews, *loss_p, *reg_p, *norm_a, *norm_s, *norm_e;      // wg2: the synthesis weight gradient's own slabs in the data-parallel step and in the pair launch of the fp32 step (see carve)
    // bfloat16 planes of the operands that are written once per step (st_gemm_planes.h): [3][same layout as the fp32 tensor]
    unsigned short *pl_W, *pl_Sfold, *pl_SfoldT;      // k-chunk-major: [K / 16][rows][3][16]
    // 16-bit GEMM operands (st_gemm16.h), each written by its producer in the layout of its fp32 counterpart: padded x/2, the analysis
    // bases as rows (bin, re | im) [2F][N], the folded synthesis bases [KP][N] and [N][KP], the spectra, the padded d syn, d G
    unsigned short *xp16, *W16, *Sfold16, *SfoldT16, *AA16, *dsyn16, *dG16;
    int n_norm_e;      // > 0: the autoencoder backward of this call left that many |g| partials of its gradients in norm_e (clip_all needs no l1_partial launch)
    bool g16;          // this call runs the 16-bit operand pipeline (call_begin's g16 argument and stft_family; the autograd entries and the
                       // four-stage schedule keep fp32 operands + gemm_half_kernel)
    size_t bytes;
};
static void carve(const st_dims* d, const Layout& L, void* base, WS* w)
{
    const size_t RT = (size_t)d->B * d->T, RO = (size_t)d->B * d->OT, F = d->F, KP = st_kp_of(d->F), N = d->N;
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? reinterpret_cast<float*>(base) + off : nullptr; off += (n + 63) / 64 * 64; return p; };
    w->re = take(RT * F); w->im = take(RT * F); w->mag = take(RT * F); w->phs = take(RT * F);
    w->mag_hat = take(RO * F); w->phs_hat = take(RO * F);
    const size_t nsl = synth_slabs(d), nfs = frame_slabs(d);
    w->AA = take(RO * KP); w->dAA = take(nsl * RO * KP);
    w->Sfold = take(KP * N); w->SfoldT = take(KP * N); w->frs = take(nfs * RO * N);
    w->y_hat = take((size_t)d->B * d->y); w->dsyn = take((size_t)d->B * (d->y + 2 * d->N));   // dsyn padded [B][N + y + N]
    w->xp = take((size_t)d->B * (d->L + 2 * d->N));                                               // x/2 padded  [B][N + L + N]
    w->dmag = take(RT * F); w->dphs = take(RT * F); w->dG = take(RT * KP);
    w->wg = take(wgrad_ws_floats(d)); w->aews = take(ae_bwd_ws_floats(d, L));
    w->loss_p = take(ola_loss_partials(d)); w->reg_p = take(ae_fwd_partials(d));
    w->norm_a = take(norm_partials(d)); w->norm_s = take(norm_partials(d)); w->norm_e = take(NORM_E_MAX); w->n_norm_e = 0;
    auto take16 = [&](size_t n) { return reinterpret_cast<unsigned short*>(take((n + 1) / 2)); };      // always sized for three planes: 19 MB
    w->pl_W = take16((size_t)3 * 2 * F * N); w->pl_Sfold = take16((size_t)3 * KP * N); w->pl_SfoldT = take16((size_t)3 * KP * N);
    // (+ 256: the 128-wide tiles of the TN kernel read up to 96 elements past the last row of an M/N-contiguous operand; masked outputs)
    w->xp16 = take16((size_t)d->B * (d->L + 2 * d->N) + 256); w->W16 = take16((size_t)2 * F * N); w->Sfold16 = take16(KP * N); w->SfoldT16 = take16(KP * N);
    w->AA16 = take16(RO * KP + 256); w->dsyn16 = take16((size_t)d->B * (d->y + 2 * d->N) + 256); w->dG16 = take16(RT * KP + 256);
    // Round 6: a second slab area for the SYNTHESIS weight gradient alone.  In the data-parallel step its slabs are summed on the communicator stream beside the autoencoder
    // backward; with a buffer of their own the analysis weight-gradient GEMM (which reuses the first area) needs no communicator -> compute wait before it starts -- one
    // barrier packet (~6 us of bubble on this stack) less on the compute stream.  Same size as the first: every slice rule is bounded by that area's size (wgrad_slices).
    w->wg2 = take(wgrad_ws_floats(d));      // last: every earlier offset stays what it was
    w->g16 = false;
    w->bytes = off * sizeof(float);
}
// float offsets of the forward state inside a workspace carved for `d` (after st_model_fwd with save_for_backward):
// re, im, mag, phs [B][T][F]; mag_hat, phs_hat [B][OT][F]; AA [B*OT][KP] (an_real at columns [0, F), an_imag at [KP/2, KP/2 + F)); y_hat [B][y].
// For diagnostics (st_model.forward(return_acts=True), nn_proc.py:311-338): the caller views its own buffer, nothing is copied.
extern "C" int st_workspace_offsets(const st_dims* d, int64_t* offs8)
{
    Layout L; ST_TRY(make_layout(d, &L)); ST_REQ(offs8, "st_workspace_offsets: null pointer");
    WS w; carve(d, L, reinterpret_cast<void*>(sizeof(float)), &w);       // a non-null dummy base: pointer differences are the offsets
    float* base = reinterpret_cast<float*>(sizeof(float));
    float* p[8] = {w.re, w.im, w.mag, w.phs, w.mag_hat, w.phs_hat, w.AA, w.y_hat};
    for (int i = 0; i < 8; ++i) offs8[i] = (int64_t)(p[i] - base);
    return ST_OK;
}
// The ten return_acts tensors of ONE autoencoder (nn_proc.py:77-126), [B][F][width] each, concatenated in `acts`
// (widths 64, 32, 16, 16, 16 + K, 16, 16, 32, 64, OT; st_ae_acts_floats() floats).  v: [B][T][F] (mag or phs); ae: that autoencoder's
// packed parameters (st_param_offsets order); sf != 0: the skip-filter output (magnitude net), else the bare ELU output (phase net).
extern "C" size_t st_ae_acts_floats(const st_dims* d)
{
    if (check_dims(d) != ST_OK) return 0;
    return (size_t)d->B * d->F * (64 + 32 + 16 + 16 + 16 + d->K + 16 + 16 + 32 + 64 + d->OT);
}
extern "C" int st_ae_acts(const st_dims* d, const float* v, const float* knobs, const float* ae, int sf, float* acts, void* stream)
{
    Layout L; ST_TRY(make_layout(d, &L));
    ST_REQ(v && (knobs || d->K == 0) && ae && acts, "st_ae_acts: null pointer");
    if (!knobs) knobs = ae;
    stm::AeActsArgs a;
    a.v = v; a.knobs = knobs; a.ae = ae; a.B = d->B; a.T = d->T; a.OT = d->OT; a.F = d->F; a.K = d->K; a.sf = sf;
    for (int l = 0; l < 9; ++l) { a.w_off[l] = L.go.w[l]; a.b_off[l] = L.go.b[l]; }
    int out[9], in[9], widths[10]; ae_shapes(d, out, in);
    for (int i = 0; i < 10; ++i) widths[i] = i < 4 ? out[i] : i == 4 ? in[4] : out[i - 1];      // layer outputs, with [z ; knobs] (the input of layer 4) between
    size_t off = 0;
    for (int i = 0; i < 10; ++i) { a.out[i] = acts + off; off += (size_t)d->B * d->F * widths[i]; }
    hipLaunchKernelGGL(stm::ae_acts_kernel, dim3((d->B * d->F + 63) / 64), dim3(64), 0, st_stream(stream), a);
    ST_LAUNCHED("ae_acts"); return ST_OK;
}
extern "C" size_t st_workspace_bytes(const st_dims* d)
{
    Layout L; if (make_layout(d, &L) != ST_OK) return 0;
    WS w; carve(d, L, nullptr, &w); return w.bytes;
}
// ONE workspace for every batch 1 .. d->B at every arithmetic level and clip scope: the exact size above is monotonic in none of them (header).
extern "C" size_t st_workspace_bytes_max(const st_dims* d)
{
    Layout L; if (make_layout(d, &L) != ST_OK) return 0;      // the layout depends on neither batch, precision nor clip scope
    size_t best = 0;
    st_dims q = *d;
    for (int b = 1; b <= d->B; ++b)
        for (int prec = ST_PREC_F32; prec <= ST_PREC_F32X3; ++prec)
            for (int ca = 0; ca < 2; ++ca) {
                q.B = b; q.prec = prec; q.clip_all = ca;
                WS w; carve(&q, L, nullptr, &w);
                if (w.bytes > best) best = w.bytes;
            }
    return best;
}

// ------------------------------------------------------------------------------ the plane GEMMs of the fused step (ST_PREC_F32X3)
// Operands written once per step -- the padded waveform, the F used rows of the analysis bases, the folded synthesis bases in both
// orientations -- become three bfloat16 planes in one elementwise launch; the spectra AA and d syn (one consumer each) are split as
// their GEMM stages them (stft_plan: GF_PLANES).  The weight-gradient GEMMs (reduction along the rows of both operands) keep the fp32 MFMA kernel.
static int planes_prepare(const st_dims* d, const float* Wr, const float* Wi, WS& w, void* stream)
{
    const int KP = st_kp_of(d->F);
    stg::WPlanesArgs a; a.njobs = 3;
    a.job[0] = stg::WPlanesJob{Wr, Wi, w.pl_W, 2 * d->F, d->N, d->N};                 // rows (bin, re | im) interleaved
    a.job[1] = stg::WPlanesJob{w.Sfold, nullptr, w.pl_Sfold, KP, d->N, d->N};
    a.job[2] = stg::WPlanesJob{w.SfoldT, nullptr, w.pl_SfoldT, d->N, KP, KP};
    a.job[3] = a.job[2];
    unsigned blk = 0;
    for (int j = 0; j < 3; ++j) { a.blk0[j] = blk; blk += (unsigned)(((size_t)a.job[j].rows * (a.job[j].K / 4) + 255) / 256); }
    a.blk0[3] = blk; a.blk0[4] = blk;
    with_planes(planes_of(d), [&](auto PL) { hipLaunchKernelGGL(stg::wplanes_kernel<PL()>, dim3(blk), dim3(256), 0, st_stream(stream), a); });
    ST_LAUNCHED("planes");
    return ST_OK;
}

// ------------------------------------------------------------------------------ fused entry points
// What a fused entry derives from its arguments before its first launch, handed down in one piece.  call_begin validates the dims (and nothing else: every
// entry keeps its own pointer checks, after it), lays out the parameters, carves the workspace and lets knobs fall back to any resident float where K == 0.
// g16 is each entry's own choice: the training and validation entries ask for the 16-bit operand pipeline (taken where stft_family admits the precision),
// the autograd entries and the four-stage schedule do not and keep fp32 operands + gemm_half_kernel.
struct Call { const st_dims* d; Layout L; WS w; const float* knobs; void* stream; };
static const bool G16_PIPELINE = true, FP32_OPERANDS = false;
static int call_begin(Call* c, const st_dims* d, const float* params, const float* knobs, void* ws, void* stream, bool g16)
{
    ST_TRY(make_layout(d, &c->L));
    c->d = d; c->knobs = knobs ? knobs : params; c->stream = stream;
    carve(d, c->L, ws, &c->w);
    c->w.g16 = g16 && stft_family(d, GEMM_ANALYSIS, SGP_PADDED | SGP_G16) == GF_G16;
    return ST_OK;
}
// A weight-gradient plan on the workspace's own operands.  area: where the slabs go (default: the first area, w.wg); more: WGP_HALVES_96; ncus: the host queries
static WgradPlan step_wgrad_plan(const st_dims* d, const WS& w, int which, int half = -1, float* area = nullptr, int more = 0, int ncus = 0)
{
    const WgOps o = which ? WgOps{w.AA, w.dsyn, w.AA16, w.dsyn16, 1.0f} : WgOps{w.dG, w.xp, w.dG16, w.xp16, 1.0f};
    return wgrad_plan(d, which, half, WGP_PADDED | (w.g16 ? WGP_G16 : 0) | more, o, area ? area : w.wg, ncus);
}
// One of the three GEMMs of stft_plan on the workspace's own operands (Wr, Wi: the analysis bases, which live with the parameters)
static GemmPlan step_stft_plan(const st_dims* d, const WS& w, int which, const float* Wr = nullptr, const float* Wi = nullptr)
{
    const GemmOps o = which == GEMM_ANALYSIS ? GemmOps{w.xp, Wr, Wi, w.xp16, w.W16, w.pl_W, 1.0f} :
                      which == GEMM_FRAMES ? GemmOps{w.AA, w.Sfold, w.SfoldT, w.AA16, w.SfoldT16, w.pl_SfoldT, 1.0f} : GemmOps{w.dsyn, w.Sfold, nullptr, w.dsyn16, w.Sfold16, w.pl_Sfold, 1.0f};
    return stft_plan(d, which, SGP_PADDED | SGP_SFOLDT | (w.g16 ? SGP_G16 : 0), o);
}
static int forward_impl(Call& c, const float* params, const float* x, const float* y_true, float* y_hat, float* mag, float* mag_hat, bool save, float* eval_p = nullptr)
{
    const st_dims* d = c.d; const Layout& L = c.L; WS& w = c.w; void* stream = c.stream;
    const float* knobs = c.knobs;
    const float* Wr = params + L.offs[0]; const float* Wi = params + L.offs[1];
    const float* Sr = params + L.offs[2]; const float* Si = params + L.offs[3];
    const float* ae_m = params + L.offs[4]; const float* ae_p = params + L.offs[22];
    // wide geometries (round 4): the analysis epilogue writes mag / phs straight into the wide autoencoder path's feature-major input
    const bool wide_direct = ae_is_wide(d) && g_wide_direct && (size_t)d->B * (L.KP / 2) * (size_t)(d->T > 64 ? d->T : 64) < ((size_t)1 << 30);
    WideWS ww; if (wide_direct) wide_carve(d, L, w.aews, &ww);
    PolarWide pwide{nullptr, nullptr, 0, 0u};
    if (wide_direct) pwide = PolarWide{ww.V[0], ww.V[1], L.KP / 2, (unsigned)ww.R};
    // saved-for-backward state always lives in the workspace; user-visible outputs are copies
    {   // one launch: x/2 (nn_proc.py:307) with the Conv1d padding materialised, the Hermitian fold of the synthesis bases
        // (cls_fe_dft.py:109-110 on the weights) and the exact zeros of the frames that lie wholly in the padding
        const stg::RowMap map = stg::live_frames(d->T, d->H, d->N, d->N, d->L);
        stm::PrepArgs a;
        a.x = x; a.xp = w.xp; a.Ls = d->L; a.pad = d->N; a.scale = 0.5f;
        a.nbx = ((d->L + 2 * d->N) / 4 + 255) / 256; a.n_pad = a.nbx * d->B;
        a.Sr = Sr; a.Si = Si; a.Sfold = w.Sfold; a.SfoldT = w.SfoldT; a.N = d->N; a.F = d->F; a.KP = L.KP; a.n_fold = (L.KP / 32) * (d->N / 32);
        a.re = save ? w.re : nullptr; a.im = save ? w.im : nullptr; a.mag = w.mag; a.phs = w.phs; a.T = d->T; a.t_lo = map.t_lo; a.Tv = map.Tv;
        const int n_dead = d->B * (d->T - map.Tv);
        a.n_dead = n_dead; a.ht = w.g16 ? gemm_ht(d->prec) : 0; a.n_w16 = 0;
        a.xp16 = w.xp16; a.Sfold16 = w.Sfold16; a.SfoldT16 = w.SfoldT16; a.W16 = w.W16; a.Wr = Wr; a.Wi = Wi;
        if (a.ht) a.n_w16 = (int)(((size_t)2 * d->F * (d->N / 4) + 255) / 256);
        a.wd = stm::PrepWide{}; a.wd.n_vpad = a.wd.n_kn = a.wd.n_pj = 0;
        if (wide_direct) {       // wide geometries: the side jobs of the feature-major input (see stm::PrepWide)
            const int FP = L.KP / 2;
            a.wd.Vm = ww.V[0]; a.wd.Vp = ww.V[1]; a.wd.FP = FP; a.wd.B = d->B; a.wd.R = (unsigned)ww.R;
            a.wd.H4Km = ww.H[0][3]; a.wd.H4Kp = ww.H[1][3]; a.wd.knobs = knobs; a.wd.K = d->K;
            a.wd.n_pj = fill_pad_jobs(a.wd.pj, d, L, ae_m, ae_p, ww);
            a.wd.n_vpad = (int)(((size_t)d->B * d->T * (FP - d->F) + 255) / 256); if (a.wd.n_vpad < 1) a.wd.n_vpad = 1;
            a.wd.n_kn = (int)(((size_t)d->K * d->B * (FP / 4) + 255) / 256);
        }
        a.ai = sta::AEImgJob{}; a.ai.n_blk = 0;
        if (ae_img_level(d)) {      // round 10: the autoencoders' LDS weight images, once per step instead of once per workgroup of ae_fwd / ae_bwd
            a.ai.ae[0] = ae_m; a.ai.ae[1] = ae_p; a.ai.img = ae_img_ptr(w.aews); a.ai.go = L.go;
            a.ai.T = d->T; a.ai.OT = d->OT; a.ai.K = d->K; a.ai.F = d->F; a.ai.FP = L.KP / 2; a.ai.expfac = expfac_of(d);
            a.ai.n = ae_img_level(d) == 2 ? sta::ae_img_floats(L.KP / 2) : sta::ae_img_fwd_floats(L.KP / 2); a.ai.n_blk = (a.ai.n + 255) / 256;
        }
        hipLaunchKernelGGL(stm::prep_kernel, dim3(a.n_pad + a.n_fold + n_dead + a.wd.n_vpad + a.wd.n_kn + a.wd.n_pj + a.ai.n_blk + a.n_w16), dim3(256), 0, st_stream(stream), a);
        ST_LAUNCHED("prep");
    }
    // a training call (target given, no user-visible |STFT| requested) on the direct wide path needs mag / phs ONLY in the feature-major layout
    const bool polar_rows = !(wide_direct && y_true && !mag);
    float* const pmag = polar_rows ? w.mag : nullptr; float* const pphs = polar_rows ? w.phs : nullptr;
    const GemmPlan ap = step_stft_plan(d, w, GEMM_ANALYSIS, Wr, Wi);
    if (ap.family == GF_PLANES) ST_TRY(planes_prepare(d, Wr, Wi, w, stream));
    ST_TRY(stft_gemm(ap, GemmOut{save ? w.re : nullptr, save ? w.im : nullptr, pmag, pphs, &pwide, nullptr}, stream));
    float* const sv = (save && ae_use_saved(d)) ? ae_sv_ptr(d, L, w.aews) : nullptr;      // round 6: the activations stay for the backward
    ST_TRY(ae_fwd_body(d, L, w.mag, w.phs, knobs, ae_m, ae_p, w.mag_hat, w.phs_hat, w.AA, w.reg_p,
                       (ae_is_wide(d) || (save && ae_use_split(d))) ? w.aews : nullptr, stream, w.g16 ? w.AA16 : nullptr, wide_direct, sv,
                       ae_img_level(d) ? ae_img_ptr(w.aews) : nullptr));     // fused geometries: the code h4 is kept for the split backward
    ST_TRY(stft_gemm(step_stft_plan(d, w, GEMM_FRAMES), slabs_at(w.frs), stream));
    ST_TRY(ola_loss_impl(d, w.frs, x, y_true, y_hat ? y_hat : w.y_hat, (save && y_true) ? w.dsyn : nullptr, d->N,
                         eval_p ? eval_p : y_true ? w.loss_p : nullptr, stream, w.g16 ? w.dsyn16 : nullptr, eval_p != nullptr));      // eval_p: loss + MAE partials (st_eval_step)
    const size_t nm = (size_t)d->B * d->T * d->F * sizeof(float), nh = (size_t)d->B * d->OT * d->F * sizeof(float);
    if (mag && hipMemcpyAsync(mag, w.mag, nm, hipMemcpyDeviceToDevice, st_stream(stream)) != hipSuccess) return st_fail(ST_ERR_LAUNCH, "copy mag");
    if (mag_hat && hipMemcpyAsync(mag_hat, w.mag_hat, nh, hipMemcpyDeviceToDevice, st_stream(stream)) != hipSuccess) return st_fail(ST_ERR_LAUNCH, "copy mag_hat");
    return ST_OK;
}

// backward of everything behind d syn (workspace holds the forward state): autograd of train.py:138.
// phase 1 = synthesis dgrad/wgrad + autoencoders + polar backward (fills grads[n_stft/2 ..));
// phase 2 = analysis weight gradient (fills rows [0,F) of the first two tensors).
// stages (ST_STAGE_*, st_train_step_groups): a stage outside the set is not launched; every other caller runs them all
static const int ST_STAGE_EVERY = ST_STAGE_SYN_DGRAD | ST_STAGE_SYN_WGRAD | ST_STAGE_AE_BWD | ST_STAGE_AE_DINPUT | ST_STAGE_ANA_WGRAD;
static int backward_syn(Call& c, float* grads, const WgradPlan* deferred = nullptr, int stages = ST_STAGE_EVERY)
{   // deferred: the caller's synthesis plan, whose slabs the caller sums itself (post_ae_kernel, the gradient-finish launch, the communicator stream); else summed here
    const st_dims* d = c.d; const Layout& L = c.L; WS& w = c.w; void* stream = c.stream;
    if (stages & ST_STAGE_SYN_DGRAD) ST_TRY(stft_gemm(step_stft_plan(d, w, GEMM_DGRAD), slabs_at(w.dAA), stream));
    if (!(stages & ST_STAGE_SYN_WGRAD)) return ST_OK;
    if (deferred) return wgrad_gemm(*deferred, stream);
    return wgrad_gemm_and_sum(step_wgrad_plan(d, w, 1), grads + L.offs[2], grads + L.offs[3], w.norm_s, nullptr, 0, stream);
}
static int backward_ae(Call& c, const float* params, float* grads, const float* g_mag_hat, const float* g_mag, float reg_coef, const WgradPlan* syn_plan = nullptr,
                       float* kg = nullptr, int stages = ST_STAGE_EVERY)
{   // stages without ST_STAGE_AE_DINPUT (st_train_step_groups, analysis bases frozen): no input gradient is wanted and no polar backward runs
    // syn_plan: the synthesis weight-gradient slabs of that plan are still to be summed (done by post_ae_kernel)
    const st_dims* d = c.d; const Layout& L = c.L; WS& w = c.w; void* stream = c.stream;
    const int syn_slabs = syn_plan ? syn_plan->ns : 0;
    const float* ae_m = params + L.offs[4]; const float* ae_p = params + L.offs[22];
    bool deferred = true;
    const PolarSink sink{w.re, w.im, g_mag, w.g16 ? nullptr : w.dG, w.g16 ? w.dG16 : nullptr};
    stw::SynReduce syn{};
    if (syn_slabs > 0 && ae_is_wide(d)) {              // wide geometries: the synthesis slab sum rides in the gradient-finish launch of the autoencoder backward
        syn.wg = syn_plan->area; syn.nz = syn_slabs; syn.gSr = grads + L.offs[2]; syn.gSi = grads + L.offs[3]; syn.norm_s = w.norm_s; syn.N = d->N; syn.F = d->F; syn.KP = L.KP;
        syn.nyq = syn_plan->nyq();
    }
    ST_TRY(ae_bwd_body(d, L, w.mag, w.phs, c.knobs, ae_m, ae_p, w.mag_hat, w.phs_hat, w.dAA, g_mag_hat, reg_coef, w.dmag, w.dphs,
                       w.aews, grads + L.offs[4], grads + L.offs[22], true, stream, &deferred, &sink, syn.wg ? &syn : nullptr,
                       (d->clip_all && ae_is_wide(d)) ? w.norm_e : nullptr, &w.n_norm_e, kg, true, !(stages & ST_STAGE_AE_DINPUT)));      // the forward left its AE state in w.aews
    if (!deferred) return ST_OK;                       // wide geometries: the gradient-finish launch summed the partials (and the synthesis slabs), and the polar backward ran inside wide_dv_polar_kernel
    stm::PostAeArgs a;
    a.ws = w.aews + 2 * ae_h4_floats(d); a.nparts = ae_use_split(d) ? ae_split_grid(d) : ae_bwd_grid(d); a.PG = L.PG; a.g_m = grads + L.offs[4]; a.g_p = grads + L.offs[22];
    a.n_red_x = (L.PG + 63) / 64; a.n_red = 2 * a.n_red_x;
    a.re = w.re; a.im = w.im; a.dmag = w.dmag; a.dphs = w.dphs; a.g_mag = g_mag; a.dG = w.dG; a.F = d->F; a.KP = L.KP;
    a.gx = (L.KP / 2 + 255) / 256; a.sat = gemm_ht(d->prec) == 2 ? 65504.0f : 0.0f;
    a.n_polar = a.gx * d->B * d->T;
    a.polar_total = 0; a.polar_magic = 0;
    if (stm::polar_flat_ok((long long)d->B * d->T, L.KP / 2)) {
        a.polar_total = (unsigned)((long long)d->B * d->T * (L.KP / 2)); a.polar_magic = stm::polar_magic(L.KP / 2);
        a.n_polar = (int)((a.polar_total + 256 * stm::POLAR_EPT - 1) / (256 * stm::POLAR_EPT));
    }
    a.wg = syn_plan ? syn_plan->area : w.wg; a.wg_nz = syn_slabs; a.gSr = grads + L.offs[2]; a.gSi = grads + L.offs[3]; a.norm_s = w.norm_s; a.N = d->N;
    a.nyq = stm::NyqJob{}; a.nyq.on = 0; if (syn_plan) a.nyq = syn_plan->nyq();
    a.dG16 = nullptr; a.ht = 0;
    if (w.g16) { a.dG16 = w.dG16; a.ht = gemm_ht(d->prec); a.dG = nullptr; }      // the analysis weight-gradient GEMM is the only consumer on this path
    a.norm_e = nullptr;
    if (d->clip_all && a.n_red <= NORM_E_MAX) { a.norm_e = w.norm_e; w.n_norm_e = a.n_red; }
    if (!(stages & ST_STAGE_AE_DINPUT)) a.n_polar = 0;      // the reduction blocks, then (if any) the synthesis slab blocks: the kernel's block arithmetic admits an empty polar role
    hipLaunchKernelGGL(stm::post_ae_kernel, dim3(a.n_red + a.n_polar + (syn_slabs > 0 ? norm_partials(d) : 0)), dim3(256), 0, st_stream(stream), a);
    if (!(stages & ST_STAGE_AE_DINPUT)) { ST_LAUNCHED("post_ae_reduce"); return ST_OK; }
    ST_LAUNCHED("post_ae");
    return ST_OK;
}
static int backward_p1(Call& c, const float* params, float* grads, const float* g_mag_hat, const float* g_mag, float reg_coef, float* kg = nullptr, int stages = ST_STAGE_EVERY)
{
    if (!(stages & ST_STAGE_AE_BWD)) return backward_syn(c, grads, nullptr, stages);      // only the synthesis bases train: their GEMM and its own slab reduce
    const WgradPlan sp = step_wgrad_plan(c.d, c.w, 1);
    ST_TRY(backward_syn(c, grads, &sp, stages));      // the slab sum rides in a later launch: post_ae_kernel (fused geometries) / wide_grad_finish_kernel (wide ones)
    return backward_ae(c, params, grads, g_mag_hat, g_mag, reg_coef, (stages & ST_STAGE_SYN_WGRAD) ? &sp : nullptr, kg, stages);
}
// The analysis weight gradient: the whole tensor, or ONE basis (half 0 = real, 1 = imaginary: gradient rows and packed stage rows [half * F, half * F + F))
static int backward_p2(Call& c, float* grads, float* stage = nullptr, int stage_bf16 = 0, int half = -1, int more = 0)
{
    return wgrad_gemm_and_sum(step_wgrad_plan(c.d, c.w, 0, half, nullptr, more), grads + c.L.offs[0], grads + c.L.offs[1], c.w.norm_a, stage, stage_bf16, c.stream);
}
// Both weight-gradient GEMMs of the fp32 step in ONE launch (stg::gemm_tn128_pair_kernel), then ONE launch that sums both sets of slabs.  Nothing between the two
// GEMMs of the per-GEMM schedule needs the synthesis weight gradient (its slabs are only summed, and the sum is first read by the optimizer), and its operands
// (the spectra, the padded d syn) are still in place when d G is ready.  Analysis slabs in w.wg, synthesis slabs in w.wg2, each with its Nyquist partials behind them.
// The pair applies to: fp32 operands, the fused autoencoder geometries, both GEMMs on the 128 x 128 kernel, g_tn128 == 1.  false from make: per-GEMM launches.
struct WgradPair { WgradPlan p[2]; stg::TNPair pair; bool on; };      // p[0] the analysis plan, p[1] the synthesis plan
static void wgrad_pair_make(WgradPair& q, const st_dims* d, const WS& w, int ncus = 0)
{
    q.on = false;
    if (g_tn128 != 1 || w.g16 || gemm_ht(d->prec) != 0 || ae_is_wide(d)) return;
    q.p[0] = step_wgrad_plan(d, w, 0, -1, w.wg, 0, ncus); q.p[1] = step_wgrad_plan(d, w, 1, -1, w.wg2, 0, ncus);
    if (q.p[0].form != WG_TN128 || q.p[1].form != WG_TN128) return;
    q.on = stg::tn128_pair_make(q.pair, q.p[0].tn, q.p[1].tn, 32);
}
static int wgrad_pair(Call& c, const WgradPair& q, float* grads)
{
    const st_dims* d = c.d; const Layout& L = c.L; void* stream = c.stream;
    ST_TRY(stg::launch_tn128_pair<32>(q.pair, q.p[0].tn, q.p[1].tn, st_stream(stream)));
    ST_LAUNCHED("wgrad_pair");
    stm::WgradPairArgs a;
    for (int i = 0; i < 2; ++i) {
        a.ws[i] = q.p[i].area; a.nz[i] = q.p[i].ns; a.gRe[i] = grads + L.offs[2 * i]; a.gIm[i] = grads + L.offs[2 * i + 1]; a.norm[i] = i ? c.w.norm_s : c.w.norm_a;
        a.nyq[i] = q.p[i].nyq();
    }
    a.N = d->N; a.F = d->F; a.KP = L.KP;
    hipLaunchKernelGGL(stm::wgrad_pair_reduce_kernel, dim3(2 * norm_partials(d)), dim3(256), 0, st_stream(stream), a);
    ST_LAUNCHED("wgrad_pair_reduce");
    return ST_OK;
}
// Host-side view of the pair launch (no device work; the CPU suite checks it): ten ints per workgroup slot, see stg::tn128_pair_describe -- (tile row, tile column,
// k-slice, k_begin, k_end) of the analysis entry, then of the synthesis entry, -1 five times where the slot has none; k ranges in reduction rows of the
// frame-major order, k-tiles of 32.  ncus <= 0: the current device's CU count.  Returns the slot count, 0 where the step does not take the pair launch at these
// dims (and tuning state), < 0 on bad arguments.
extern "C" int st_wgrad_pair_plan(const st_dims* d, int ncus, int* out, int cap)
{
    Layout L;
    if (make_layout(d, &L) != ST_OK || cap < 0 || (cap > 0 && !out)) return -1;
    WS w; carve(d, L, reinterpret_cast<void*>(sizeof(float)), &w);       // a non-null dummy base (as st_workspace_offsets): only pointer differences are used
    WgradPair q; wgrad_pair_make(q, d, w, ncus);
    if (!q.on) return 0;
    return stg::tn128_pair_describe(q.pair, d->N / 128, d->N / 128, 32, out, cap);
}
// Host-side view of ONE weight-gradient launch (no device work): the plan the launches themselves ask for, as ST_WGRAD_PLAN_INTS ints (signaltrain_hip.h).
// which 0 / 1: analysis / synthesis bases; half -1 / 0 / 1 (one basis: analysis only); flags: ST_WGPLAN_*; ncus <= 0: the current device's CU count -- then the
// answer is what a launch on this device does under the current tuning state.  Fills min(cap, count) ints and returns the count; < 0 on bad arguments.
extern "C" int st_wgrad_plan(const st_dims* d, int which, int half, int flags, int ncus, int* out, int cap)
{
    static_assert(ST_WGPLAN_PADDED == WGP_PADDED && ST_WGPLAN_G16 == WGP_G16 && ST_WGPLAN_STAGED == WGP_HALVES_96, "st_wgrad_plan: flag values");
    Layout L;
    if (make_layout(d, &L) != ST_OK || cap < 0 || (cap > 0 && !out)) return -1;
    if (which < 0 || which > 1 || half < -1 || half > 1 || (half >= 0 && which) || (flags & ~(WGP_PADDED | WGP_G16 | WGP_HALVES_96)) ||
        ((flags & WGP_G16) && !(flags & WGP_PADDED))) return -1;
    WS w; carve(d, L, reinterpret_cast<void*>(sizeof(float)), &w);       // a non-null dummy base: only pointer differences are used
    w.g16 = (flags & WGP_G16) && stft_family(d, GEMM_ANALYSIS, SGP_PADDED | SGP_G16) == GF_G16;      // as call_begin: the pipeline is taken where the precision admits it
    const WgradPlan p = (flags & WGP_PADDED) ? step_wgrad_plan(d, w, which, half, nullptr, flags & WGP_HALVES_96, ncus)
                                             : wgrad_plan(d, which, half, flags, WgOps{w.dG, w.xp, nullptr, nullptr, 1.0f}, w.wg, ncus);
    const int v[ST_WGRAD_PLAN_INTS] = {p.form, p.R, p.ns, p.m0, p.M, p.frame_major ? 1 : 0, p.trim.on ? 1 : 0, p.nyq_P, (int)p.nyq_off, p.nyq_write ? 1 : 0, (int)p.used()};
    for (int i = 0; i < ST_WGRAD_PLAN_INTS && i < cap; ++i) out[i] = v[i];
    return ST_WGRAD_PLAN_INTS;
}
static int backward_impl(Call& c, const float* params, float* grads, const float* g_mag_hat, const float* g_mag, float reg_coef, float* kg = nullptr)
{
    WgradPair q; wgrad_pair_make(q, c.d, c.w);
    if (q.on) {      // the data gradient alone, the autoencoders with post_ae_kernel free of slab blocks, then the pair
        ST_TRY(backward_p1(c, params, grads, g_mag_hat, g_mag, reg_coef, kg, ST_STAGE_EVERY & ~ST_STAGE_SYN_WGRAD));
        return wgrad_pair(c, q, grads);
    }
    ST_TRY(backward_p1(c, params, grads, g_mag_hat, g_mag, reg_coef, kg));
    return backward_p2(c, grads);
}

extern "C" int st_model_fwd(const st_dims* d, const float* params, const float* x, const float* knobs,
                            float* y_hat, float* mag, float* mag_hat, void* ws, int save_for_backward, void* stream)
{
    Call c; ST_TRY(call_begin(&c, d, params, knobs, ws, stream, FP32_OPERANDS));
    ST_REQ(params && x && (knobs || d->K == 0) && ws, "st_model_fwd: null pointer");
    return forward_impl(c, params, x, nullptr, y_hat, mag, mag_hat, save_for_backward != 0);
}

extern "C" int st_model_bwd(const st_dims* d, const float* params, float* grads, const float* x, const float* knobs,
                            const float* g_y_hat, const float* g_mag_hat, const float* g_mag, void* ws, void* stream)
{
    Call c; ST_TRY(call_begin(&c, d, params, knobs, ws, stream, FP32_OPERANDS));
    ST_REQ(params && grads && x && (knobs || d->K == 0) && g_y_hat && ws, "st_model_bwd: null pointer");
    ST_TRY(pad_scale(g_y_hat, c.w.dsyn, d->B, d->y, d->N, 2.0f, stream));     // dsyn = 2 * g_y_hat, padded for the framed loaders
    return backward_impl(c, params, grads, g_mag_hat, g_mag, 0.0f);
}

// d (anything downstream) / d knobs for arbitrary upstream gradients -- what autograd hands to a knobs tensor that requires grad (nn_proc.py:92-93: the
// knob settings are repeated over the rows of a window and concatenated in front of fnn_addknobs of BOTH autoencoders, nn_proc.py:332-333).  With
// d a5 the gradient at that layer's pre-activation, d knobs[b][k] = sum over nets, rows of window b, outputs o of  W5[o][16 + k] * d a5[row][o]: the row sum is
// exactly the layer's BIAS gradient of a batch that holds window b alone.  So: one forward + backward per window (B = 1), then 16 x K multiply-adds
// on the two bias gradients.  Deliberately the slow, exact route (B launch-bound passes, ~0.3 ms each): the reference's training never asks for this
// gradient (knobs are data), so the hot kernels carry no per-window reduction for it.  grads_scratch: L.total floats, overwritten; the saved-for-backward
// state of `ws` afterwards belongs to the LAST window -- run the forward again before st_model_bwd.  At geometries where a single window cannot take
// the requested 16-bit arithmetic (st_effective_prec: the wide autoencoder path, odd batch) these passes run the autoencoder layers in fp32.
// One workgroup (64 threads) per window: workgroup w reads ng rows of 16 floats of either net from gbm / gbp + w * ng * 16 and sums them in ascending row
// order (bit-repeatable), then the 16 x K multiply-adds with the fp32 W5 of both nets -> out[w][K].  ng = 1, one workgroup: the rows ARE the two bias
// gradients (st_model_knob_grad); ng = groups per window: the per-group column sums of d a5 the backward kernels wrote (st_model_bwd_knobs).
__global__ void knob_grad_kernel(const float* __restrict__ Wm, const float* __restrict__ gbm, const float* __restrict__ Wp, const float* __restrict__ gbp,
                                 const int K, float* __restrict__ out, const int ng)
{
    __shared__ float gb[32];
    const int k = threadIdx.x;
    if (k < 32) {
        const float* p = (k < 16 ? gbm : gbp) + (size_t)blockIdx.x * ng * 16 + (k & 15);
        float a = p[0];
        for (int j = 1; j < ng; ++j) a += p[j * 16];
        gb[k] = a;
    }
    __syncthreads();
    if (k >= K) return;
    float s = 0.f, t = 0.f;
    for (int o = 0; o < 16; ++o) { s += Wm[o * (16 + K) + 16 + k] * gb[o]; t += Wp[o * (16 + K) + 16 + k] * gb[16 + o]; }
    out[(size_t)blockIdx.x * K + k] = s + t;
}
extern "C" int st_model_knob_grad(const st_dims* d, const float* params, float* grads_scratch, const float* x, const float* knobs,
                                  const float* g_y_hat, const float* g_mag_hat, const float* g_mag, void* ws, float* g_knobs, void* stream)
{
    Layout L; ST_TRY(make_layout(d, &L));
    ST_REQ(params && grads_scratch && x && knobs && g_y_hat && ws && g_knobs, "st_model_knob_grad: null pointer");
    ST_REQ(d->K >= 1 && d->K <= 64, "st_model_knob_grad: K = %d", d->K);
    st_dims d1 = *d; d1.B = 1;
    Layout L1; ST_TRY(make_layout(&d1, &L1));
    const size_t w5 = (size_t)L1.offs[4] + (size_t)L1.go.w[4], b5 = (size_t)L1.offs[4] + (size_t)L1.go.b[4];
    for (int b = 0; b < d->B; ++b) {
        const float* xb = x + (size_t)b * d->L; const float* kb = knobs + (size_t)b * d->K;
        ST_TRY(st_model_fwd(&d1, params, xb, kb, nullptr, nullptr, nullptr, ws, 1, stream));
        ST_TRY(st_model_bwd(&d1, params, grads_scratch, xb, kb, g_y_hat + (size_t)b * d->y, g_mag_hat ? g_mag_hat + (size_t)b * d->OT * d->F : nullptr,
                            g_mag ? g_mag + (size_t)b * d->T * d->F : nullptr, ws, stream));
        hipLaunchKernelGGL(knob_grad_kernel, dim3(1), dim3(64), 0, st_stream(stream), params + w5, grads_scratch + b5, params + w5 + L1.PG, grads_scratch + b5 + L1.PG,
                           d->K, g_knobs + (size_t)b * d->K, 1);
    }
    ST_LAUNCHED("knob_grad");
    return ST_OK;
}

// The same gradient in ONE backward pass of the batch: the autoencoder backward kernels also write the per-group column sums of d a5 (16 floats per 16-row
// group; a group never straddles a window) into the caller's scratch, and one small launch -- one workgroup per window -- sums a window's groups in
// ascending order and applies W5.  Every scratch element that launch reads was written by this call: no clearing.
extern "C" int st_knob_grad_fused_supported(const st_dims* d)
{
    if (check_dims(d) != ST_OK) return 0;
    if (d->K < 1) { (void)st_fail(ST_ERR_ARG, "st_model_bwd_knobs: K = %d (a model without knobs has no knob gradient)", d->K); return 0; }
    if (!ae_kg_route(d)) { (void)st_fail(ST_ERR_UNSUPPORTED, "st_model_bwd_knobs: no per-group d a5 output on this autoencoder backward route (%s)", ae_kg_why(d)); return 0; }
    return 1;
}
extern "C" size_t st_model_bwd_knobs_ws_floats(const st_dims* d)
{
    if (check_dims(d) != ST_OK) return 0;
    return (size_t)2 * ae_fwd_groups(d) * 16;
}
extern "C" int st_model_bwd_knobs(const st_dims* d, const float* params, float* grads, const float* x, const float* knobs,
                                  const float* g_y_hat, const float* g_mag_hat, const float* g_mag, void* ws, float* scratch, float* g_knobs, void* stream)
{
    Call c; ST_TRY(call_begin(&c, d, params, knobs, ws, stream, FP32_OPERANDS));
    const Layout& L = c.L;
    ST_REQ(params && grads && x && knobs && g_y_hat && ws && scratch && g_knobs, "st_model_bwd_knobs: null pointer");
    ST_REQ(d->K >= 1, "st_model_bwd_knobs: K = %d (a model without knobs has no knob gradient)", d->K);
    if (!ae_kg_route(d)) return st_fail(ST_ERR_UNSUPPORTED, "st_model_bwd_knobs: no per-group d a5 output on this autoencoder backward route (%s)", ae_kg_why(d));
    ST_TRY(pad_scale(g_y_hat, c.w.dsyn, d->B, d->y, d->N, 2.0f, stream));     // as st_model_bwd
    ST_TRY(backward_impl(c, params, grads, g_mag_hat, g_mag, 0.0f, scratch));
    const size_t w5 = (size_t)L.offs[4] + (size_t)L.go.w[4];
    const int gpw = L.KP / 32;
    hipLaunchKernelGGL(knob_grad_kernel, dim3(d->B), dim3(64), 0, st_stream(stream), params + w5, (const float*)scratch, params + w5 + L.PG,
                       (const float*)scratch + (size_t)ae_fwd_groups(d) * 16, d->K, g_knobs, gpw);
    ST_LAUNCHED("knob_grad");
    return ST_OK;
}

extern "C" int st_loss_backward(const st_dims* d, const float* params, float* grads, const float* x, const float* knobs,
                                const float* y_true, float* y_hat, float* mag, float* mag_hat, void* ws,
                                float* scalars, void* stream)
{
    Call c; ST_TRY(call_begin(&c, d, params, knobs, ws, stream, G16_PIPELINE));
    ST_REQ(params && grads && x && (knobs || d->K == 0) && y_true && ws && scalars, "st_loss_backward: null pointer");
    prof_mark("begin", stream);
    ST_TRY(forward_impl(c, params, x, y_true, y_hat, mag, mag_hat, true));
    ST_TRY(backward_impl(c, params, grads, nullptr, nullptr, reg_coef_of(d)));
    // grads carry the loss scale (if any); the published norm is that of the unscaled gradient
    return finalize_scalars(d, c.w.loss_p, c.w.reg_p, c.w.norm_a, c.w.norm_s, 1.0f / loss_scale_of(d), scalars, stream);
}

// One validation batch of train.py:28-42: the forward of the training step at this st_dims.prec (16-bit levels: the pre-rounded operand GEMMs), nothing kept
// for a backward, the log-cosh / MAE / L1 partials and one finalize that updates the caller's accumulator on the device.  The log-cosh and MAE partials
// (2 * st_ola_loss_partials floats) take the place of d syn, which a forward without a backward never writes: the workspace does not grow.
extern "C" int st_eval_step(const st_dims* d, const float* params, const float* x, const float* knobs, const float* y_true,
                            float* y_hat, void* ws, double* acc, double beta, void* stream)
{
    Call c; ST_TRY(call_begin(&c, d, params, knobs, ws, stream, G16_PIPELINE));
    ST_REQ(params, "st_eval_step: null pointer (params)"); ST_REQ(x, "st_eval_step: null pointer (x)");
    ST_REQ(knobs || d->K == 0, "st_eval_step: null pointer (knobs, K = %d)", d->K);
    ST_REQ(y_true, "st_eval_step: null pointer (y_true)"); ST_REQ(ws, "st_eval_step: null pointer (ws)"); ST_REQ(acc, "st_eval_step: null pointer (acc)");
    prof_mark("begin", stream);
    float* const eval_p = c.w.dsyn;      // two arrays of B * ceil(y / 256) partials (the second at stm::mae_partial_offset) out of B * (y + 2N) floats
    ST_TRY(forward_impl(c, params, x, y_true, y_hat, nullptr, nullptr, false, eval_p));
    const stm::FinArgs f = fin_args(d, eval_p, c.w.reg_p, nullptr, nullptr, 1.0f);
    hipLaunchKernelGGL(stm::eval_finalize_kernel, dim3(1), dim3(256), 0, st_stream(stream), f, beta, acc);
    ST_LAUNCHED("eval_finalize"); return ST_OK;
}

// ae_knob_bwd_kernel (st_fit.h): 12-wave workgroups, three waves per SIMD, one workgroup per CU: grid.y = 2 nets -> up to half the CUs per net
static const int AE_KNOB_NW = 12;
static int ae_knob_grid(const st_dims* d) { int g = (ae_fwd_groups(d) + AE_KNOB_NW - 1) / AE_KNOB_NW; int c = num_cus() / 2; if (c < 1) c = 1; return g < c ? g : c; }
// ------------------------------------------------------------------------------ whole-signal inference (st_predict.h)
// utils/predict_long.py:30-79 in one call.  The workspace is [head | batch workspace]: the head holds what depends on the parameters only -- both orientations of the
// folded synthesis bases in the form this level's GEMMs read (fp32, 16-bit, or three bfloat16 planes), the 16-bit / plane copies of the analysis rows, the forward
// part of the autoencoders' LDS weight images -- and the batch's knob rows; it is built once per call and sized for every level, so it lies at the same place whatever
// the batch, the level and the tuning state.  The batch workspace behind it is carved per batch exactly as the fused entries carve theirs.
struct PredictWS {
    float *Sfold, *SfoldT, *img, *knobs;
    unsigned short *Sfold16, *SfoldT16, *W16, *pl_W, *pl_Sfold, *pl_SfoldT;
    size_t head_bytes;
};
// the ready-made forward images do not depend on the batch here (they have a place of their own): wherever the fp32 forward kernel can take them (ae_img_level's rules but the room)
static bool predict_img(const st_dims* d) { return g_ae_save != 2 && !ae_is_wide(d) && ae_ht(d->prec) == 0 && !ae_use_split(d) && st_kp_of(d->F) / 2 <= sta::CL::FWD_TOTAL; }
static void predict_carve(const st_dims* d, void* base, PredictWS* p)
{
    const size_t F = d->F, KP = st_kp_of(d->F), N = d->N;
    size_t off = 0;
    auto take = [&](size_t n) { float* q = base ? reinterpret_cast<float*>(base) + off : nullptr; off += (n + 63) / 64 * 64; return q; };
    auto take16 = [&](size_t n) { return reinterpret_cast<unsigned short*>(take((n + 1) / 2)); };
    p->Sfold = take(KP * N); p->SfoldT = take(KP * N);
    p->Sfold16 = take16(KP * N); p->SfoldT16 = take16(KP * N); p->W16 = take16(2 * F * N);
    p->pl_W = take16(3 * 2 * F * N); p->pl_Sfold = take16(3 * KP * N); p->pl_SfoldT = take16(3 * KP * N);
    p->img = take((size_t)sta::ae_img_fwd_floats((int)(KP / 2)));
    p->knobs = take((size_t)d->B * (d->K > 0 ? d->K : 1));
    p->head_bytes = off * sizeof(float);
}
static bool predict_ok(const st_dims* d) { return check_dims(d) == ST_OK && !ae_is_wide(d); }
extern "C" int st_predict_supported(const st_dims* d) { return predict_ok(d) ? 1 : 0; }
static long long predict_windows(const st_dims* d, long long n) { return n < d->L ? 1 : (n - d->L + d->y - 1) / d->y + 1; }      // audio.sliding_window with overlap L - y
extern "C" long long st_predict_windows(const st_dims* d, long long n) { return (check_dims(d) != ST_OK || n <= 0) ? 0 : predict_windows(d, n); }
extern "C" long long st_predict_out_samples(const st_dims* d, long long n)
{
    if (check_dims(d) != ST_OK) return 0;
    const long long r = n - ((long long)d->L - d->y);
    return r > 0 ? r : 0;
}
extern "C" size_t st_predict_ws_bytes(const st_dims* d)
{
    Layout L; if (make_layout(d, &L) != ST_OK || ae_is_wide(d)) return 0;
    PredictWS p; predict_carve(d, nullptr, &p);
    size_t best = 0;
    st_dims q = *d;
    for (int b = 1; b <= d->B; ++b) { q.B = b; WS w; carve(&q, L, nullptr, &w); if (w.bytes > best) best = w.bytes; }      // not monotonic in the batch (st_workspace_bytes_max)
    return p.head_bytes + best;
}
// One optimiser step of st_fit_knobs rides on the same batch loop (fit != NULL): the forward keeps h4, and behind the frames GEMM come fit_ola, the synthesis
// data-gradient GEMM, ae_knob_bwd, knob_grad and the per-batch tail instead of predict_ola.  batch_off: where the batch workspace starts (behind the head, and for
// the fit behind its own rows and scratch).
struct FitJob {
    const void* target; float *kg, *rows, *acc;      // per-group scratch [2][groups of a batch][16], per-window rows [d->B][K], the one-row accumulator [K]
    float *knobs, *m, *v, *grad; double* loss;       // grad: this step's row(s) of grad_hist, or NULL
    stf::TailArgs hyper;                             // inv_n, inv_n_d and Adam's scalars of this step
};
// The coded routes ride on it too (cj != NULL, st_decode.h).  code_out: st_encode_long -- the knob-independent half of every batch (stage kernel, analysis GEMM, the
// forward kernel's code-only pass) and the pack kernel, nothing else.  code: the forward of a batch is ae_dec_fwd_kernel from the code -- st_decode_long runs it, the
// frames GEMM and predict_ola once per knob setting INSIDE the batch (settings 2..S find the batch's code in L2 / Infinity Cache), st_fit_knobs_coded once, with
// mag_hat / phs_hat and the batch-layout h4, magnitude tail and knob rows ae_knob_bwd_kernel reads written through.  cj == NULL: the launches of st_predict_long and
// st_fit_knobs, unchanged.
struct CodeJob { float* code_out; const float* code; int n_settings; long long out_pitch; size_t set_stride; };      // set_stride: floats between two settings' knob rows
// ae_dec_fwd_kernel: 8-wave workgroups, four waves per SIMD, two workgroups per CU
static int ae_dec_grid(const st_dims* d) { int g = (ae_fwd_groups(d) + sta::AE_DEC_NW - 1) / sta::AE_DEC_NW; int c = num_cus() * sta::AE_DEC_WGS; return g < c ? g : c; }

// ---- the batch of the whole-signal entries, stated once: st_predict_long, the coded routes, the fits, the predict session and st_eval_pool all build theirs from these
// the head's parameter-side operands, where the GEMM plans look for them
static void ws_head(WS& w, const PredictWS& p)
{
    w.Sfold = p.Sfold; w.SfoldT = p.SfoldT; w.Sfold16 = p.Sfold16; w.SfoldT16 = p.SfoldT16; w.W16 = p.W16;
    w.pl_W = p.pl_W; w.pl_Sfold = p.pl_Sfold; w.pl_SfoldT = p.pl_SfoldT;
}
struct InferBatch {
    st_dims q; WS w;                           // the dims at this batch's row count, its workspace (carved as the fused entries carve theirs, the head's operands in place)
    bool g16, img;                             // the 16-bit pipeline wherever the precision admits it, as the training entries; ready-made forward images
    const Layout* L; const PredictWS* p; const float *params, *Wr, *Wi, *ae_m, *ae_p;
    int ht() const { return g16 ? gemm_ht(q.prec) : 0; }
    const float* resident_knobs() const { return q.K == 0 ? params : p->knobs; }      // K == 0: any resident float (call_begin)
};
static InferBatch infer_batch(const st_dims* d, const Layout& L, const PredictWS& p, const float* params, void* ws, size_t batch_off, long long rows)
{
    InferBatch b;
    b.q = *d; b.q.B = (int)rows;
    carve(&b.q, L, reinterpret_cast<char*>(ws) + batch_off, &b.w);
    b.g16 = stft_family(d, GEMM_ANALYSIS, SGP_PADDED | SGP_G16) == GF_G16; b.img = predict_img(d);
    b.w.g16 = b.g16;
    ws_head(b.w, p);
    b.L = &L; b.p = &p; b.params = params;
    b.Wr = params + L.offs[0]; b.Wi = params + L.offs[1]; b.ae_m = params + L.offs[4]; b.ae_p = params + L.offs[22];
    return b;
}
// what every stage kernel is told about the batch; fill_knobs: its knob blocks write the batch's knob rows into the head
static stp::StageCommon stage_common(const InferBatch& b, bool fill_knobs)
{
    const st_dims& q = b.q;
    const stg::RowMap map = stg::live_frames(q.T, q.H, q.N, q.N, q.L);
    stp::StageCommon c;
    c.y = q.y; c.L = q.L; c.pad = q.N; c.nb = q.B;
    c.xp = b.w.xp; c.xp16 = b.w.xp16; c.ht = b.ht();
    c.nbx = ((q.L + 2 * q.N) / 4 + 255) / 256; c.n_pad = c.nbx * q.B;
    c.mag = b.w.mag; c.phs = b.w.phs; c.T = q.T; c.F = q.F; c.t_lo = map.t_lo; c.Tv = map.Tv; c.n_dead = q.B * (q.T - map.Tv);
    c.knobs = b.p->knobs; c.K = q.K; c.n_kn = fill_knobs && q.K > 0 ? (q.B * q.K + 255) / 256 : 0;
    return c;
}
static int infer_analysis(const InferBatch& b, void* stream)
{
    return stft_gemm(step_stft_plan(&b.q, b.w, GEMM_ANALYSIS, b.Wr, b.Wi), GemmOut{nullptr, nullptr, b.w.mag, b.w.phs, nullptr, nullptr}, stream);
}
static int infer_frames(const InferBatch& b, void* stream) { return stft_gemm(step_stft_plan(&b.q, b.w, GEMM_FRAMES), slabs_at(b.w.frs), stream); }
// staged rows -> frames: analysis GEMM, the autoencoders at knob rows kn, frames GEMM.  keep_h4 (the fits): the code h4 stays at the head of the autoencoder workspace
static int infer_forward(const InferBatch& b, const float* kn, bool keep_h4, void* stream)
{
    ST_TRY(infer_analysis(b, stream));
    ST_TRY(ae_fwd_body(&b.q, *b.L, b.w.mag, b.w.phs, kn, b.ae_m, b.ae_p, b.w.mag_hat, b.w.phs_hat, b.w.AA, b.w.reg_p, keep_h4 ? b.w.aews : nullptr, stream,
                       b.g16 ? b.w.AA16 : nullptr, false, nullptr, b.img ? b.p->img : nullptr));
    return infer_frames(b, stream);
}
// The launch shape of every overlap-add kernel of the family (st_predict.h: ola_frame_sum): launch(NS, NF, grid, slab) names the kernel and its arguments.
// NF = 3: the rule of ola_loss_impl for the four-sample form with all loads up front.
template <class F> static void ola_launch(const InferBatch& b, F&& launch)
{
    const st_dims& q = b.q;
    const int ns = frame_slabs(&q);
    const dim3 grid((q.y / 4 + 255) / 256, q.B);
    const size_t slab = (size_t)q.B * q.OT * q.N;
    const bool three = (q.N + q.H - 1) / q.H <= 3;
    with_bool(three, [&](auto NF3) { with_slabs(ns, [&](auto NS) { launch(NS, ic<NF3() ? 3 : 0>{}, grid, slab); }); });
}
// d J / d knobs of a batch whose fit_ola has written d syn: data-gradient GEMM -> ae_knob_bwd_kernel (knob rows kn) -> knob_grad_kernel, into fit.rows [rows][K]
// The offset guard is st_fit_knobs' and st_fit_knobs_coded's (their wording); st_fit_knobs_multi_coded never reaches it: multi_args has refused these sizes, at the
// plan's largest batch and under its own name, before the first launch.
static int knob_backward(const InferBatch& b, const float* kn, const FitJob& fit, void* stream)
{
    const st_dims& q = b.q; const Layout& L = *b.L; const WS& w = b.w;
    ST_REQ((size_t)synth_slabs(&q) * q.B * q.OT * L.KP < ((size_t)1 << 30) && (size_t)q.B * q.T * L.KP < ((size_t)1 << 30),
           "st_fit_knobs: batch too large for the kernel's 32-bit element offsets (B=%d)", q.B);
    ST_TRY(stft_gemm(step_stft_plan(&q, w, GEMM_DGRAD), slabs_at(w.dAA), stream));
    const stg::RowMap live = synth_live(&q);
    const int groups = ae_fwd_groups(&q), kgrid = ae_knob_grid(&q);
    ST_TRY(with_ht(ae_ht(q.prec), [&](auto HT) {
        return launch_lds("ae_knob_bwd_kernel", sta::ae_knob_bwd_kernel<AE_KNOB_NW, HT()>, dim3(kgrid, 2), dim3(AE_KNOB_NW * 64),
                          (size_t)sta::ae_knob_lds_floats(AE_KNOB_NW) * sizeof(float), st_stream(stream),
                          w.mag, kn, b.ae_m, b.ae_p, L.go, w.mag_hat, w.phs_hat, w.dAA, w.aews, fit.kg, q.B, q.T, q.OT, q.F, q.K, L.KP,
                          live.t_lo, live.t_lo + live.Tv - 1, synth_slabs(&q), (size_t)q.B * q.OT * L.KP); }));
    ST_LAUNCHED("ae_knob_bwd");
    const size_t w5 = (size_t)L.offs[4] + (size_t)L.go.w[4];
    hipLaunchKernelGGL(knob_grad_kernel, dim3(q.B), dim3(64), 0, st_stream(stream), b.params + w5, (const float*)fit.kg, b.params + w5 + L.PG,
                       (const float*)fit.kg + (size_t)groups * 16, q.K, fit.rows, L.KP / 32);
    ST_LAUNCHED("knob_grad");
    return ST_OK;
}
// the decoder forward of a batch from the code (st_decode.h): no stage kernel, no analysis GEMM, no encoder.  fit: mag_hat / phs_hat and the batch-layout h4, magnitude
// tail and knob rows ae_knob_bwd_kernel reads are written through.  STK: rows are (setting, window) pairs, nw windows each, the settings set_stride floats apart.
template <bool STK>
static int dec_forward(const InferBatch& b, const float* code, const float* kn, int kn_pitch, bool fit, void* stream, int nw = 0, unsigned set_stride = 0u)
{
    const st_dims& q = b.q; const WS& w = b.w;
    ST_TRY(with_ht(ae_ht(q.prec), [&](auto HT) {
        return launch_lds("ae_dec_fwd_kernel", sta::ae_dec_fwd_kernel<sta::AE_DEC_NW, HT(), STK>, dim3(ae_dec_grid(&q)), dim3(sta::AE_DEC_NW * 64),
                          (size_t)sta::ae_dec_lds_floats() * sizeof(float), st_stream(stream),
                          code, kn, kn_pitch, b.ae_m, b.ae_p, b.L->go,
                          fit ? w.mag_hat : nullptr, fit ? w.phs_hat : nullptr, w.AA, b.g16 ? w.AA16 : nullptr, b.ht(),
                          fit ? w.aews : nullptr, fit ? w.mag : nullptr, fit ? b.p->knobs : nullptr, q.B, q.T, q.OT, q.F, q.K, b.L->KP, nw, set_stride); }));
    ST_LAUNCHED("ae_dec_fwd");
    return ST_OK;
}
template <typename T>
static int predict_batches(const st_dims* d, const Layout& L, const PredictWS& p, const float* params, const void* signal_v, long long n,
                           const float* knobs, long long knob_rows, float* out, long long n_out, void* ws, void* stream,
                           const FitJob* fit = nullptr, size_t batch_off = 0, const CodeJob* cj = nullptr)
{
    const T* signal = reinterpret_cast<const T*>(signal_v);
    if (!batch_off) batch_off = p.head_bytes;
    const bool enc = cj && cj->code_out, dec = cj && cj->code;
    const int nset = dec && !fit ? cj->n_settings : 1;
    const size_t CW = stc::code_window_floats(L.KP / 2, d->OT);
    const long long nwin = (n_out + d->y - 1) / d->y;      // == predict_windows(d, n) wherever n_out > 0
    for (long long w0 = 0; w0 < nwin; w0 += d->B) {
        const InferBatch b = infer_batch(d, L, p, params, ws, batch_off, nwin - w0 < d->B ? nwin - w0 : d->B);
        const st_dims& q = b.q; const WS& w = b.w;
        const long long s0 = w0 * q.y;
        const bool fill = knob_rows == 1 && q.K > 0;
        const float* kn = q.K == 0 ? params : fill ? p.knobs : knobs + (size_t)w0 * q.K;      // K == 0: any resident float (call_begin)
        if (!dec) {
            stp::StageArgs a;
            a.c = stage_common(b, fill && !enc);      // the code does not depend on the knobs: the code-only pass loads a knob row (any resident floats) and drops it
            a.signal = signal; a.n = n; a.s0 = s0; a.knob_row = knobs;
            hipLaunchKernelGGL(stp::predict_stage_kernel<T>, dim3(a.c.n_pad + a.c.n_dead + a.c.n_kn), dim3(256), 0, st_stream(stream), a);
            ST_LAUNCHED("predict_stage");
        }
        if (enc) {      // st_encode_long: the knob-independent half, then the batch's h4 and tails to their windows of the code
            ST_TRY(infer_analysis(b, stream));
            ST_TRY(ae_fwd_body(&q, L, w.mag, w.phs, b.resident_knobs(), b.ae_m, b.ae_p, nullptr, nullptr, nullptr, nullptr, w.aews, stream, nullptr, false, nullptr,
                               b.img ? p.img : nullptr));
            const int n4 = (int)(CW / 4);
            hipLaunchKernelGGL(stc::code_pack_kernel, dim3((n4 + 1023) / 1024, q.B), dim3(256), 0, st_stream(stream),
                               (const float*)w.aews, (const float*)w.mag, (const float*)w.phs, cj->code_out + (size_t)w0 * CW, q.B, q.T, q.OT, q.F, L.KP / 2);
            ST_LAUNCHED("code_pack");
            continue;
        }
        for (int s = 0; s < nset; ++s) {
            if (dec) {
                ST_REQ((size_t)q.B * CW < ((size_t)1 << 30) && (size_t)q.B * q.T * q.F < ((size_t)1 << 30) && (size_t)q.B * q.OT * L.KP < ((size_t)1 << 30) &&
                       (size_t)q.B * q.T < ((size_t)1 << 24),      // the last: the 24-bit products b * T and b * OT of the row offsets
                       "st_decode_long / st_fit_knobs_coded: batch too large for the kernel's 32-bit element offsets (B=%d)", q.B);
                const bool one = knob_rows == 1;
                const float* ks = q.K == 0 ? params : knobs + (size_t)s * cj->set_stride + (one ? 0 : (size_t)w0 * q.K);
                ST_TRY(dec_forward<false>(b, cj->code + (size_t)w0 * CW, ks, (one || q.K == 0) ? 0 : q.K, fit != nullptr, stream));
                ST_TRY(infer_frames(b, stream));
            }
            else ST_TRY(infer_forward(b, kn, fit != nullptr, stream));
            if (!fit) {
                ola_launch(b, [&](auto NS, auto NF, dim3 grid, size_t slab) {
                    hipLaunchKernelGGL((stp::predict_ola_kernel<T, NS(), NF()>), grid, dim3(256), 0, st_stream(stream),
                                       w.frs, slab, signal, dec ? out + (size_t)s * cj->out_pitch : out, s0, n_out, q.L, q.N, q.H, q.OT, q.y); });
                ST_LAUNCHED("predict_ola");
                continue;
            }
            const int nslot = (q.y + 255) / 256;
            ola_launch(b, [&](auto NS, auto NF, dim3 grid, size_t slab) {
                hipLaunchKernelGGL((stf::fit_ola_kernel<T, NS(), NF()>), grid, dim3(256), 0, st_stream(stream),
                                   w.frs, slab, signal, reinterpret_cast<const T*>(fit->target), w.dsyn, b.g16 ? w.dsyn16 : nullptr, b.ht(), w.loss_p, nslot,
                                   s0, n_out, q.L, q.N, q.H, q.OT, q.y, 0); });
            ST_LAUNCHED("fit_ola");
            ST_TRY(knob_backward(b, kn, *fit, stream));
            stf::TailArgs t = fit->hyper;
            t.loss_p = w.loss_p; t.n_lp = q.B * nslot; t.loss = fit->loss;
            t.rows = fit->rows; t.nb = q.B; t.K = q.K; t.acc = fit->acc;
            t.per_window = knob_rows != 1; t.first = w0 == 0; t.last = w0 + q.B >= nwin;
            const size_t ro = t.per_window ? (size_t)w0 * q.K : 0;
            t.knobs = fit->knobs + ro; t.m = fit->m + ro; t.v = fit->v + ro; t.grad = fit->grad ? fit->grad + ro : nullptr;
            hipLaunchKernelGGL(stf::fit_tail_kernel, dim3(1), dim3(256), 0, st_stream(stream), t);
            ST_LAUNCHED("fit_tail");
        }
    }
    return ST_OK;
}
// once per call: the parameter side of prep_kernel (its per-batch jobs have no blocks here) into the head of the workspace
static int predict_prep(const st_dims* d, const Layout& L, const PredictWS& p, const float* params, void* stream)
{
    {
        const int family = stft_family(d, GEMM_ANALYSIS, SGP_PADDED | SGP_G16);      // as predict_batches
        const bool g16 = family == GF_G16;
        stm::PrepArgs a;
        a.x = nullptr; a.xp = nullptr; a.Ls = d->L; a.pad = d->N; a.scale = 0.5f; a.nbx = 1; a.n_pad = 0;
        a.Sr = params + L.offs[2]; a.Si = params + L.offs[3]; a.Sfold = p.Sfold; a.SfoldT = p.SfoldT; a.N = d->N; a.F = d->F; a.KP = L.KP; a.n_fold = (L.KP / 32) * (d->N / 32);
        a.re = a.im = a.mag = a.phs = nullptr; a.T = d->T; a.t_lo = 0; a.Tv = d->T; a.n_dead = 0;
        a.ht = g16 ? gemm_ht(d->prec) : 0; a.n_w16 = 0;
        a.xp16 = nullptr; a.Sfold16 = p.Sfold16; a.SfoldT16 = p.SfoldT16; a.W16 = p.W16; a.Wr = params + L.offs[0]; a.Wi = params + L.offs[1];
        if (a.ht) a.n_w16 = (int)(((size_t)2 * d->F * (d->N / 4) + 255) / 256);
        a.wd = stm::PrepWide{}; a.wd.n_vpad = a.wd.n_kn = a.wd.n_pj = 0;
        a.ai = sta::AEImgJob{}; a.ai.n_blk = 0;
        if (predict_img(d)) {
            a.ai.ae[0] = params + L.offs[4]; a.ai.ae[1] = params + L.offs[22]; a.ai.img = p.img; a.ai.go = L.go;
            a.ai.T = d->T; a.ai.OT = d->OT; a.ai.K = d->K; a.ai.F = d->F; a.ai.FP = L.KP / 2; a.ai.expfac = expfac_of(d);
            a.ai.n = sta::ae_img_fwd_floats(L.KP / 2); a.ai.n_blk = (a.ai.n + 255) / 256;
        }
        hipLaunchKernelGGL(stm::prep_kernel, dim3(a.n_fold + a.ai.n_blk + a.n_w16), dim3(256), 0, st_stream(stream), a);
        ST_LAUNCHED("predict_prep");
        if (family == GF_PLANES) {
            WS w; ws_head(w, p);
            ST_TRY(planes_prepare(d, a.Wr, a.Wi, w, stream));
        }
    }
    return ST_OK;
}
// ---- what the whole-signal entries ask of their arguments, each rule and its wording in one place, under the entry's name
// the dims rule that failed, under this entry's name
static int layout_named(const char* name, const st_dims* d, Layout* L)
{
    if (make_layout(d, L) == ST_OK) return ST_OK;
    char rule[400]; snprintf(rule, sizeof(rule), "%s", st_last_error());
    return st_fail(ST_ERR_ARG, "%s: %s", name, rule);
}
static int refuse_wide(const char* name, const char* hint, const st_dims* d)
{
    ST_REQ(!ae_is_wide(d), "%s: not supported for the wide autoencoder geometries (T = %d > 32 or OT = %d > 16): %s", name, d->T, d->OT, hint);
    return ST_OK;
}
static int pcm_align(int fmt) { return fmt == ST_PCM_S16 ? 8 : 16; }      // one quad of samples is one aligned access
// a pointer the entry needs: present, and aligned to `align` bytes (1: any address)
static int check_ptr(const char* name, const char* what, const void* p, int align)
{
    ST_REQ(p, "%s: null pointer (%s)", name, what);
    ST_REQ((reinterpret_cast<uintptr_t>(p) & (uintptr_t)(align - 1)) == 0, "%s: %s must be %d-byte aligned", name, what, align);
    return ST_OK;
}
// the recording and the workspace: parameters, a positive length, a known format, bases a quad access can take
static int check_recording(const char* name, const float* params, int fmt, const void* signal, long long n, const void* ws)
{
    ST_TRY(check_ptr(name, "params", params, 1));
    ST_REQ(n > 0, "%s: n must be positive (n = %lld)", name, n);
    ST_REQ(fmt == ST_PCM_F32 || fmt == ST_PCM_S16, "%s: fmt = %d is neither ST_PCM_F32 nor ST_PCM_S16", name, fmt);
    ST_TRY(check_ptr(name, "signal", signal, pcm_align(fmt)));
    return check_ptr(name, "ws", ws, 16);
}
static int check_knob_rows(const char* name, const st_dims* d, long long n, long long knob_rows)
{
    const long long nwin = predict_windows(d, n);
    ST_REQ(knob_rows == 1 || knob_rows == nwin, "%s: knob_rows = %lld must be 1 or the window count (%lld windows for n = %lld)", name, knob_rows, nwin, n);
    return ST_OK;
}
// Adam's scalars of a fit entry, and what one step makes of them for the tail kernels (inv_n, inv_n_d and torch.optim.Adam's step constants)
struct AdamArgs { long long first_step; int steps; float lr, beta1, beta2, eps; };
static int check_adam(const char* name, const AdamArgs& h)
{
    ST_REQ(h.steps >= 1, "%s: steps = %d must be at least 1", name, h.steps);
    ST_REQ(h.first_step >= 1, "%s: first_step = %lld must be at least 1 (Adam's step number is 1-based)", name, h.first_step);
    ST_REQ(std::isfinite(h.lr) && h.lr >= 0.f, "%s: lr = %g must be finite and not negative", name, (double)h.lr);
    ST_REQ(std::isfinite(h.beta1) && h.beta1 >= 0.f && h.beta1 < 1.f, "%s: beta1 = %g must lie in [0, 1)", name, (double)h.beta1);
    ST_REQ(std::isfinite(h.beta2) && h.beta2 >= 0.f && h.beta2 < 1.f, "%s: beta2 = %g must lie in [0, 1)", name, (double)h.beta2);
    ST_REQ(std::isfinite(h.eps) && h.eps > 0.f, "%s: eps = %g must be finite and positive", name, (double)h.eps);
    return ST_OK;
}
static stf::TailArgs adam_step(const AdamArgs& h, int s, long long n_out)
{
    const double t = (double)(h.first_step + s);
    const double bc1 = 1.0 - pow((double)h.beta1, t), bc2 = 1.0 - pow((double)h.beta2, t);
    stf::TailArgs a{};
    a.inv_n_d = 1.0 / (double)n_out; a.inv_n = (float)(1.0 / (double)n_out);
    a.neg_step = (float)(-(double)h.lr / bc1); a.bc2_sqrt = (float)sqrt(bc2);
    a.w1 = (float)(1.0 - (double)h.beta1); a.b2 = h.beta2; a.w2 = (float)(1.0 - (double)h.beta2); a.eps = h.eps;
    return a;
}
extern "C" int st_predict_long(const st_dims* d, const float* params, int fmt, const void* signal, long long n,
                               const float* knobs, long long knob_rows, float* out, void* ws, void* stream)
{
    static const char* const name = "st_predict_long";
    Layout L; ST_TRY(make_layout(d, &L));
    ST_TRY(check_recording(name, params, fmt, signal, n, ws));
    ST_REQ(knobs || d->K == 0, "%s: null pointer (knobs, K = %d)", name, d->K);
    ST_TRY(check_ptr(name, "out", out, 16));
    ST_TRY(check_knob_rows(name, d, n, knob_rows));
    ST_TRY(refuse_wide(name, "st_predict_supported", d));
    const long long n_out = n - ((long long)d->L - d->y);
    if (n_out <= 0) return ST_OK;      // shorter than the first window's lookback: nothing to predict, nothing launched
    PredictWS p; predict_carve(d, ws, &p);
    prof_mark("begin", stream);
    ST_TRY(predict_prep(d, L, p, params, stream));
    return with_pcm(fmt, [&](auto z) { return predict_batches<decltype(z)>(d, L, p, params, signal, n, knobs, knob_rows, out, n_out, ws, stream); });
}

// ------------------------------------------------------------------------------ predict session: inference fed block by block (st_predict_stream.h)
// st_predict_long's batch -- its staging, forward and overlap-add -- on rows that are (channel, window) pairs, read from (history | block) instead of a resident
// signal.  The workspace is st_predict_long's, [head | one batch's workspace]; the head is built by st_predict_stream_open and only read afterwards.  The schedule
// (which windows a push completes, what it emits, what stays held) is host arithmetic in stream_plan, shared by st_predict_stream_plan and the push.
static long long stream_wc(const st_dims* d, long long n) { return n < d->L ? 0 : (n - d->L) / d->y + 1; }      // complete windows in n samples
static void stream_plan(const st_dims* d, long long n_in, long long m, int final, long long out4[4])
{
    const long long n1 = n_in + m, first = stream_wc(d, n_in), wc1 = stream_wc(d, n1);
    out4[0] = first; out4[1] = wc1 - first; out4[2] = (wc1 - first) * d->y; out4[3] = n1 - wc1 * d->y;
    if (final) {      // the zero-padded last window as well, clipped as st_predict_long clips it; nothing stays held
        const long long n_out = n1 > (long long)d->L - d->y ? n1 - ((long long)d->L - d->y) : 0;
        out4[1] = (n_out + d->y - 1) / d->y - first; out4[2] = n_out - first * d->y; out4[3] = 0;
    }
}
extern "C" int st_predict_stream_plan(const st_dims* d, long long n_in, long long m, int final, long long out4[4])
{
    ST_TRY(check_dims(d));
    ST_REQ(out4, "st_predict_stream_plan: null pointer (out4)");
    ST_REQ(n_in >= 0 && m >= 0, "st_predict_stream_plan: n_in = %lld and m = %lld must not be negative", n_in, m);
    stream_plan(d, n_in, m, final, out4);
    return ST_OK;
}
extern "C" size_t st_predict_stream_state_bytes(const st_dims* d, int channels)
{
    return (predict_ok(d) && channels >= 1) ? (size_t)2 * channels * d->L * sizeof(float) : 0;
}
extern "C" size_t st_predict_stream_ws_bytes(const st_dims* d) { return st_predict_ws_bytes(d); }
static const int STREAM_MAX_CHANNELS = 65535;      // the carry kernel's grid.y
extern "C" int st_predict_stream_open(const st_dims* d, const float* params, int channels, st_predict_stream* s, void* state, void* ws, void* stream)
{
    Layout L; ST_TRY(make_layout(d, &L));
    ST_TRY(refuse_wide("st_predict_stream_open", "st_predict_supported", d));
    ST_REQ(channels >= 1 && channels <= STREAM_MAX_CHANNELS, "st_predict_stream_open: channels = %d must lie in 1 .. %d", channels, STREAM_MAX_CHANNELS);
    ST_REQ(params, "st_predict_stream_open: null pointer (params)"); ST_REQ(s, "st_predict_stream_open: null pointer (s)");
    ST_REQ(state, "st_predict_stream_open: null pointer (state)"); ST_REQ(ws, "st_predict_stream_open: null pointer (ws)");
    ST_REQ((reinterpret_cast<uintptr_t>(state) & 15) == 0, "st_predict_stream_open: state must be 16-byte aligned");
    ST_REQ((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "st_predict_stream_open: ws must be 16-byte aligned");
    *s = st_predict_stream{};
    s->channels = channels;
    s->L = d->L; s->N = d->N; s->H = d->H; s->T = d->T; s->OT = d->OT; s->F = d->F; s->K = d->K; s->y = d->y; s->prec = d->prec; s->B = d->B;
    PredictWS p; predict_carve(d, ws, &p);
    prof_mark("begin", stream);
    return predict_prep(d, L, p, params, stream);
}
extern "C" int st_predict_stream_reset(st_predict_stream* s)
{
    ST_REQ(s, "st_predict_stream_reset: null pointer (s)");
    ST_REQ(s->channels >= 1, "st_predict_stream_reset: the session was never opened (channels = %d)", s->channels);
    s->received = s->emitted = 0; s->held = 0; s->half = 0; s->closed = 0;
    return ST_OK;
}
// One push's batches: st_predict_long's batch with the stream's stage and overlap-add kernels around the forward.
template <typename T>
static int stream_batches(const st_dims* d, const Layout& L, const PredictWS& p, const float* params, const sts::Src& src, int channels,
                          const long long plan[4], const float* knobs, long long knob_rows, float* out, long long out_pitch, void* ws, void* stream)
{
    const long long rows = plan[1] * channels;
    for (long long r0 = 0; r0 < rows; r0 += d->B) {
        const InferBatch b = infer_batch(d, L, p, params, ws, p.head_bytes, rows - r0 < d->B ? rows - r0 : d->B);
        const st_dims& q = b.q;
        sts::StageArgs a;
        a.c = stage_common(b, true);
        a.s = src; a.first = plan[0]; a.nw = plan[1]; a.r0 = r0;
        a.knob_src = knobs; a.knob_stride = knob_rows == 1 ? 0 : q.K;
        hipLaunchKernelGGL(sts::stream_stage_kernel<T>, dim3(a.c.n_pad + a.c.n_dead + a.c.n_kn), dim3(256), 0, st_stream(stream), a);
        ST_LAUNCHED("stream_stage");
        ST_TRY(infer_forward(b, b.resident_knobs(), false, stream));
        ola_launch(b, [&](auto NS, auto NF, dim3 grid, size_t slab) {
            hipLaunchKernelGGL((sts::stream_ola_kernel<T, NS(), NF()>), grid, dim3(256), 0, st_stream(stream),
                               b.w.frs, slab, src, out, out_pitch, plan[0], plan[1], r0, plan[2], q.L, q.N, q.H, q.OT, q.y); });
        ST_LAUNCHED("stream_ola");
    }
    return ST_OK;
}
extern "C" int st_predict_stream_push(const st_dims* d, const float* params, st_predict_stream* s, int fmt, const void* block, long long m, long long block_pitch,
                                      int final, const float* knobs, long long knob_rows, float* out, long long out_pitch, void* state, void* ws, void* stream)
{
    Layout L; ST_TRY(make_layout(d, &L));
    ST_TRY(refuse_wide("st_predict_stream_push", "st_predict_supported", d));
    ST_REQ(s, "st_predict_stream_push: null pointer (s)");
    ST_REQ(s->channels >= 1 && s->channels <= STREAM_MAX_CHANNELS, "st_predict_stream_push: channels = %d: the session was not opened by st_predict_stream_open", s->channels);
    ST_REQ(s->L == d->L && s->N == d->N && s->H == d->H && s->T == d->T && s->OT == d->OT && s->F == d->F && s->K == d->K && s->y == d->y,
           "st_predict_stream_push: dims differ from the ones the session was opened with (L = %d, N = %d, H = %d, K = %d at open)", s->L, s->N, s->H, s->K);
    ST_REQ(s->prec == d->prec, "st_predict_stream_push: prec = %d differs from the one the session was opened with (%d)", d->prec, s->prec);
    ST_REQ(s->B == d->B, "st_predict_stream_push: B = %d differs from the one the session was opened with (%d)", d->B, s->B);
    ST_REQ(!s->closed, "st_predict_stream_push: the session is closed (a final push came before): st_predict_stream_reset");
    ST_REQ(params, "st_predict_stream_push: null pointer (params)");
    ST_REQ(knobs || d->K == 0, "st_predict_stream_push: null pointer (knobs, K = %d)", d->K);
    ST_REQ(state, "st_predict_stream_push: null pointer (state)"); ST_REQ(ws, "st_predict_stream_push: null pointer (ws)");
    ST_REQ(m >= 0 && m <= (1ll << 30), "st_predict_stream_push: m = %lld must lie in 0 .. 2^30", m);
    ST_REQ(final || m % 4 == 0, "st_predict_stream_push: m = %lld of a non-final push must be a multiple of 4", m);
    ST_REQ(fmt == ST_PCM_F32 || fmt == ST_PCM_S16, "st_predict_stream_push: fmt = %d is neither ST_PCM_F32 nor ST_PCM_S16", fmt);
    ST_REQ(knob_rows == 1 || knob_rows == s->channels, "st_predict_stream_push: knob_rows = %lld must be 1 or the channel count (%d)", knob_rows, s->channels);
    ST_REQ(block || m == 0, "st_predict_stream_push: null pointer (block, m = %lld)", m);
    ST_REQ(block_pitch >= m && block_pitch % 4 == 0, "st_predict_stream_push: block_pitch = %lld must be a multiple of 4 and at least m = %lld", block_pitch, m);
    const long long n0 = s->received;
    ST_REQ(n0 >= 0 && s->held >= 0 && s->held < d->L && s->held <= n0 && n0 % 4 == 0 && s->held % 4 == 0 && (s->half == 0 || s->half == 1),
           "st_predict_stream_push: the session's counters are inconsistent (received = %lld, held = %d)", n0, s->held);
    long long plan[4]; stream_plan(d, n0, m, final, plan);
    ST_REQ(s->held == n0 - plan[0] * d->y, "st_predict_stream_push: the session's counters are inconsistent (received = %lld, held = %d)", n0, s->held);
    ST_REQ(out || plan[2] == 0, "st_predict_stream_push: null pointer (out, %lld samples per channel to emit)", plan[2]);
    ST_REQ(out_pitch >= plan[2] && out_pitch % 4 == 0, "st_predict_stream_push: out_pitch = %lld must be a multiple of 4 and at least the emitted count (%lld)", out_pitch, plan[2]);
    const uintptr_t ba = fmt == ST_PCM_S16 ? 7 : 15;
    ST_REQ((reinterpret_cast<uintptr_t>(block) & ba) == 0, "st_predict_stream_push: block must be %d-byte aligned", (int)ba + 1);
    ST_REQ((reinterpret_cast<uintptr_t>(out) & 15) == 0, "st_predict_stream_push: out must be 16-byte aligned");
    ST_REQ((reinterpret_cast<uintptr_t>(state) & 15) == 0, "st_predict_stream_push: state must be 16-byte aligned");
    ST_REQ((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "st_predict_stream_push: ws must be 16-byte aligned");
    const size_t half = (size_t)s->channels * d->L;
    float* hist = reinterpret_cast<float*>(state);
    sts::Src src{hist + s->half * half, block, n0 - s->held, n0, m, block_pitch, d->L};
    prof_mark("begin", stream);
    if (plan[1] > 0) {
        PredictWS p; predict_carve(d, ws, &p);
        ST_TRY(with_pcm(fmt, [&](auto z) { return stream_batches<decltype(z)>(d, L, p, params, src, s->channels, plan, knobs, knob_rows, out, out_pitch, ws, stream); }));
    }
    if (!final && m > 0) {      // what no complete window has consumed, to the other half; a final push keeps nothing
        const int held1 = (int)plan[3];
        if (held1 > 0) {
            const dim3 grid((held1 / 4 + 255) / 256, s->channels);
            float* next = hist + (s->half ^ 1) * half;
            with_pcm(fmt, [&](auto z) { hipLaunchKernelGGL(sts::stream_carry_kernel<decltype(z)>, grid, dim3(256), 0, st_stream(stream), src, next, n0 + m - held1, held1); });
            ST_LAUNCHED("stream_carry");
        }
        s->half ^= 1;
    }
    s->received = n0 + m; s->emitted += plan[2]; s->held = (int)plan[3]; s->closed = final ? 1 : 0;
    return ST_OK;
}

// ------------------------------------------------------------------------------ a folder of recordings in one call (st_eval_pool.h)
// st_predict_long's batch on rows that are (file, window) pairs of the feeds' pool, every file at its own knob row, with the per-file error statistics left on the
// device.  The workspace is [st_predict_long's head | the batch's partials [POOL_PART][d->B * ceil(y / 256)] | one batch's workspace].
static size_t pool_part_plane(const st_dims* d) { return ((size_t)d->B * ((d->y + 255) / 256) + 63) / 64 * 64; }
static size_t pool_part_bytes(const st_dims* d) { return (size_t)stq::POOL_PART * pool_part_plane(d) * sizeof(float); }
static long long pool_windows(const st_dims* d, long long len) { return len > (long long)d->L - d->y ? predict_windows(d, len) : 0; }      // no output sample, no row
extern "C" int st_eval_pool_supported(const st_dims* d) { return st_predict_supported(d); }
extern "C" long long st_eval_pool_rows(const st_dims* d, const long long* file_len_host, int nfiles, long long* win_off_host)
{
    if (check_dims(d) != ST_OK || !file_len_host || nfiles < 1) return 0;
    long long rows = 0;
    for (int f = 0; f < nfiles; ++f) {
        if (win_off_host) win_off_host[f] = rows;
        rows += pool_windows(d, file_len_host[f]);
    }
    if (win_off_host) win_off_host[nfiles] = rows;
    return rows;
}
extern "C" size_t st_eval_pool_ws_bytes(const st_dims* d)
{
    const size_t pb = st_predict_ws_bytes(d);
    return pb ? pb + pool_part_bytes(d) : 0;
}
template <typename T>
static int pool_batches(const st_dims* d, const Layout& L, const PredictWS& p, const float* params, const void* pool_x_v, const void* pool_y_v, const stq::Tables& tb,
                        long long total_rows, const float* file_knobs, double* stats, float* out, void* ws, void* stream)
{
    const T* pool_x = reinterpret_cast<const T*>(pool_x_v); const T* pool_y = reinterpret_cast<const T*>(pool_y_v);
    float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + p.head_bytes);
    const size_t batch_off = p.head_bytes + pool_part_bytes(d);
    const size_t plane = pool_part_plane(d);
    const int nslot = (d->y + 255) / 256;
    const int n_zero = tb.nfiles < 1024 ? tb.nfiles : 1024;
    if (total_rows == 0) {      // nothing to predict: the side role alone (the zero spans and the zero statistics)
        stq::StageArgs a{};
        a.t = tb; a.c.L = d->L; a.c.y = d->y; a.out = out; a.stats = stats; a.n_zero = n_zero;
        hipLaunchKernelGGL(stq::pool_stage_kernel<T>, dim3(n_zero), dim3(256), 0, st_stream(stream), a);
        ST_LAUNCHED("pool_stage");
        return ST_OK;
    }
    for (long long r0 = 0; r0 < total_rows; r0 += d->B) {
        const InferBatch b = infer_batch(d, L, p, params, ws, batch_off, total_rows - r0 < d->B ? total_rows - r0 : d->B);
        const st_dims& q = b.q;
        stq::StageArgs a;
        a.c = stage_common(b, true);
        a.pool_x = pool_x; a.t = tb; a.r0 = r0; a.file_knobs = file_knobs;
        a.out = out; a.stats = stats; a.n_zero = r0 == 0 ? n_zero : 0;
        hipLaunchKernelGGL(stq::pool_stage_kernel<T>, dim3(a.c.n_pad + a.c.n_dead + a.c.n_kn + a.n_zero), dim3(256), 0, st_stream(stream), a);
        ST_LAUNCHED("pool_stage");
        ST_TRY(infer_forward(b, b.resident_knobs(), false, stream));
        ola_launch(b, [&](auto NS, auto NF, dim3 grid, size_t slab) {
            hipLaunchKernelGGL((stq::pool_ola_kernel<T, NS(), NF()>), grid, dim3(256), 0, st_stream(stream),
                               b.w.frs, slab, pool_x, pool_y, out, part, plane, nslot, tb, r0, q.L, q.N, q.H, q.OT, q.y); });
        ST_LAUNCHED("pool_ola");
        if (stats) {
            hipLaunchKernelGGL(stq::pool_tail_kernel, dim3(q.B), dim3(256), 0, st_stream(stream), (const float*)part, plane, nslot, tb, r0, q.B, q.L, q.y, stats);
            ST_LAUNCHED("pool_tail");
        }
    }
    return ST_OK;
}
extern "C" int st_eval_pool(const st_dims* d, const float* params, int fmt, const void* pool_x, const void* pool_y,
                            const long long* file_off, const long long* file_len, const long long* win_off, int nfiles,
                            long long total_rows, long long pool_samples, const float* file_knobs, double* stats, float* out, void* ws, void* stream)
{
    Layout L; ST_TRY(make_layout(d, &L));
    ST_TRY(refuse_wide("st_eval_pool", "st_eval_pool_supported", d));
    ST_REQ(params, "st_eval_pool: null pointer (params)"); ST_REQ(pool_x, "st_eval_pool: null pointer (pool_x)");
    ST_REQ(file_off, "st_eval_pool: null pointer (file_off)"); ST_REQ(file_len, "st_eval_pool: null pointer (file_len)"); ST_REQ(win_off, "st_eval_pool: null pointer (win_off)");
    ST_REQ(file_knobs || d->K == 0, "st_eval_pool: null pointer (file_knobs, K = %d)", d->K);
    ST_REQ(ws, "st_eval_pool: null pointer (ws)");
    ST_REQ(fmt == ST_PCM_F32 || fmt == ST_PCM_S16, "st_eval_pool: fmt = %d is neither ST_PCM_F32 nor ST_PCM_S16", fmt);
    ST_REQ(nfiles >= 1, "st_eval_pool: nfiles = %d must be at least 1", nfiles);
    ST_REQ(total_rows >= 0, "st_eval_pool: total_rows = %lld must not be negative", total_rows);
    ST_REQ(pool_samples >= 1, "st_eval_pool: pool_samples = %lld must be at least 1", pool_samples);
    ST_REQ((stats != nullptr) == (pool_y != nullptr), "st_eval_pool: stats and pool_y come together (stats %s, pool_y %s)", stats ? "given" : "null", pool_y ? "given" : "null");
    ST_REQ(out || stats, "st_eval_pool: out and stats are both null: nothing to compute");
    const uintptr_t pa = fmt == ST_PCM_S16 ? 7 : 15;
    ST_REQ((reinterpret_cast<uintptr_t>(pool_x) & pa) == 0, "st_eval_pool: pool_x must be %d-byte aligned", (int)pa + 1);
    ST_REQ((reinterpret_cast<uintptr_t>(pool_y) & pa) == 0, "st_eval_pool: pool_y must be %d-byte aligned", (int)pa + 1);
    ST_REQ((reinterpret_cast<uintptr_t>(out) & 15) == 0, "st_eval_pool: out must be 16-byte aligned");
    ST_REQ((reinterpret_cast<uintptr_t>(stats) & 15) == 0, "st_eval_pool: stats must be 16-byte aligned");
    ST_REQ((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "st_eval_pool: ws must be 16-byte aligned");
    {   // the kernels' 32-bit element offsets at the largest batch: the frame slabs and the synthesis operand (check_dims holds the rest at d->B)
        const size_t rows = (size_t)(total_rows < d->B ? total_rows : d->B);
        ST_REQ((size_t)frame_slabs(d) * rows * d->OT * d->N < ((size_t)1 << 30) && (size_t)synth_slabs(d) * rows * d->OT * L.KP < ((size_t)1 << 30),
               "st_eval_pool: batch too large for the kernels' 32-bit element offsets (%zu rows)", rows);
    }
    PredictWS p; predict_carve(d, ws, &p);
    const stq::Tables tb{file_off, file_len, win_off, nfiles, pool_samples};
    prof_mark("begin", stream);
    if (total_rows > 0) { ST_TRY(predict_prep(d, L, p, params, stream)); }
    return with_pcm(fmt, [&](auto z) { return pool_batches<decltype(z)>(d, L, p, params, pool_x, pool_y, tb, total_rows, file_knobs, stats, out, ws, stream); });
}

// ------------------------------------------------------------------------------ knob fit on the device (st_fit.h)
// predict.fit_knobs in one call: every batch of every optimiser step is enqueued here.  The workspace is [st_predict_long's head | the fit's own rows and scratch |
// one batch's workspace]: per-window gradient rows [d->B][K] (a batch's windows; one knob row: summed into the accumulator batch by batch in ascending window
// order, one row per window: consumed by the batch's own tail launch), the accumulator [64] and the per-group column sums of d a5 [2][d->B * KP / 32][16].
struct FitWS { float *rows, *acc, *kg; size_t bytes; };
static void fit_carve(const st_dims* d, void* base, FitWS* f)
{
    size_t off = 0;
    auto take = [&](size_t n) { float* q = base ? reinterpret_cast<float*>(base) + off : nullptr; off += (n + 63) / 64 * 64; return q; };
    f->rows = take((size_t)d->B * (d->K > 0 ? d->K : 1)); f->acc = take(64); f->kg = take((size_t)2 * ae_fwd_groups(d) * 16);
    f->bytes = off * sizeof(float);
}
extern "C" int st_fit_knobs_supported(const st_dims* d) { return (predict_ok(d) && d->K >= 1) ? 1 : 0; }
extern "C" size_t st_fit_knobs_ws_bytes(const st_dims* d)
{
    if (!st_fit_knobs_supported(d)) return 0;
    const size_t pb = st_predict_ws_bytes(d);
    if (!pb) return 0;
    FitWS f; fit_carve(d, nullptr, &f);
    return pb + f.bytes;
}
static int fit_knobs_impl(const char* name, const bool coded, const st_dims* d, const float* params, const float* code, int fmt, const void* signal, const void* target, long long n,
                          float* knobs, long long knob_rows, float* adam_m, float* adam_v, const AdamArgs& h,
                          double* loss_hist, float* grad_hist, void* ws, void* stream)
{
    Layout L; ST_TRY(layout_named(name, d, &L));
    ST_REQ(d->K >= 1, "%s: K = %d (a model without knobs has no knobs to fit)", name, d->K);
    ST_TRY(check_recording(name, params, fmt, signal, n, ws));
    ST_TRY(check_ptr(name, "target", target, pcm_align(fmt)));
    ST_TRY(check_ptr(name, "knobs", knobs, 16)); ST_TRY(check_ptr(name, "adam_m", adam_m, 16)); ST_TRY(check_ptr(name, "adam_v", adam_v, 16));
    ST_TRY(check_ptr(name, "loss_hist", loss_hist, 1));
    if (coded) ST_TRY(check_ptr(name, "code", code, 16));
    ST_TRY(check_knob_rows(name, d, n, knob_rows));
    ST_TRY(check_adam(name, h));
    ST_TRY(refuse_wide(name, "st_fit_knobs_supported", d));
    const long long n_out = n - ((long long)d->L - d->y);
    if (n_out <= 0) return ST_OK;      // no output sample, no objective: nothing launched, every buffer left alone
    PredictWS p; predict_carve(d, ws, &p);
    FitWS f; fit_carve(d, reinterpret_cast<char*>(ws) + p.head_bytes, &f);
    const size_t batch_off = p.head_bytes + f.bytes;
    prof_mark("begin", stream);
    ST_TRY(predict_prep(d, L, p, params, stream));
    const size_t row_floats = (size_t)knob_rows * d->K;
    for (int s = 0; s < h.steps; ++s) {
        FitJob job;
        job.target = target; job.kg = f.kg; job.rows = f.rows; job.acc = f.acc;
        job.knobs = knobs; job.m = adam_m; job.v = adam_v; job.grad = grad_hist ? grad_hist + (size_t)s * row_floats : nullptr; job.loss = loss_hist + s;
        job.hyper = adam_step(h, s, n_out);
        const CodeJob cj{nullptr, code, 1, 0, 0};
        ST_TRY(with_pcm(fmt, [&](auto z) {
            return predict_batches<decltype(z)>(d, L, p, params, signal, n, knobs, knob_rows, nullptr, n_out, ws, stream, &job, batch_off, coded ? &cj : nullptr); }));
    }
    return ST_OK;
}
extern "C" int st_fit_knobs(const st_dims* d, const float* params, int fmt, const void* signal, const void* target, long long n,
                            float* knobs, long long knob_rows, float* adam_m, float* adam_v,
                            long long first_step, int steps, float lr, float beta1, float beta2, float eps,
                            double* loss_hist, float* grad_hist, void* ws, void* stream)
{
    return fit_knobs_impl("st_fit_knobs", false, d, params, nullptr, fmt, signal, target, n, knobs, knob_rows, adam_m, adam_v,
                          AdamArgs{first_step, steps, lr, beta1, beta2, eps}, loss_hist, grad_hist, ws, stream);
}
// st_fit_knobs from the code of the recording (st_encode_long): every step's forward is the decoder forward; everything behind the frames GEMM is st_fit_knobs'.
extern "C" int st_fit_knobs_coded(const st_dims* d, const float* params, const void* code, int fmt, const void* signal, const void* target, long long n,
                                  float* knobs, long long knob_rows, float* adam_m, float* adam_v,
                                  long long first_step, int steps, float lr, float beta1, float beta2, float eps,
                                  double* loss_hist, float* grad_hist, void* ws, void* stream)
{
    return fit_knobs_impl("st_fit_knobs_coded", true, d, params, reinterpret_cast<const float*>(code), fmt, signal, target, n, knobs, knob_rows, adam_m, adam_v,
                          AdamArgs{first_step, steps, lr, beta1, beta2, eps}, loss_hist, grad_hist, ws, stream);
}

// ------------------------------------------------------------------------------ encode once, decode at any knob setting (st_decode.h)
// Every ae_dec_fwd_kernel instantiation passes the ISA scan (tools/check_mfma_hazards.py), so every arithmetic level of the fused geometries is served.
static bool decode_ok(const st_dims* d) { return predict_ok(d); }
extern "C" int st_decode_supported(const st_dims* d) { return decode_ok(d) ? 1 : 0; }
extern "C" size_t st_decode_ws_bytes(const st_dims* d) { return decode_ok(d) ? st_predict_ws_bytes(d) : 0; }
extern "C" size_t st_code_bytes(const st_dims* d, long long n)
{
    if (!decode_ok(d) || n <= 0) return 0;
    return (size_t)predict_windows(d, n) * stc::code_window_floats(st_kp_of(d->F) / 2, d->OT) * sizeof(float);
}
// what st_encode_long and st_decode_long ask of the recording and the workspace, under the entry's name
static int coded_args(const char* name, const st_dims* d, Layout* L, const float* params, const void* code, int fmt, const void* signal, long long n, const void* ws)
{
    ST_TRY(layout_named(name, d, L));
    ST_TRY(check_recording(name, params, fmt, signal, n, ws));
    ST_TRY(check_ptr(name, "code", code, 16));
    return refuse_wide(name, "st_decode_supported", d);
}
extern "C" int st_encode_long(const st_dims* d, const float* params, int fmt, const void* signal, long long n, void* code, void* ws, void* stream)
{
    Layout L; ST_TRY(coded_args("st_encode_long", d, &L, params, code, fmt, signal, n, ws));
    const long long n_out = n - ((long long)d->L - d->y);
    if (n_out <= 0) return ST_OK;      // as st_predict_long: no output sample, nothing launched
    PredictWS p; predict_carve(d, ws, &p);
    prof_mark("begin", stream);
    ST_TRY(predict_prep(d, L, p, params, stream));
    const CodeJob cj{reinterpret_cast<float*>(code), nullptr, 1, 0, 0};
    return with_pcm(fmt, [&](auto z) { return predict_batches<decltype(z)>(d, L, p, params, signal, n, nullptr, 1, nullptr, n_out, ws, stream, nullptr, 0, &cj); });
}
extern "C" int st_decode_long(const st_dims* d, const float* params, const void* code, int fmt, const void* signal, long long n,
                              const float* knobs, long long knob_rows, int n_settings, float* out, long long out_pitch, void* ws, void* stream)
{
    Layout L; ST_TRY(coded_args("st_decode_long", d, &L, params, code, fmt, signal, n, ws));
    ST_REQ(knobs || d->K == 0, "st_decode_long: null pointer (knobs, K = %d)", d->K);
    ST_TRY(check_ptr("st_decode_long", "out", out, 16));
    ST_TRY(check_knob_rows("st_decode_long", d, n, knob_rows));
    ST_REQ(n_settings >= 1, "st_decode_long: n_settings = %d must be at least 1", n_settings);
    const long long n_out = n - ((long long)d->L - d->y);
    ST_REQ(out_pitch >= n_out && out_pitch >= 0 && out_pitch % 4 == 0,
           "st_decode_long: out_pitch = %lld must be a multiple of 4 and at least the %lld output samples of a setting", out_pitch, n_out > 0 ? n_out : 0);
    if (n_out <= 0) return ST_OK;
    PredictWS p; predict_carve(d, ws, &p);
    prof_mark("begin", stream);
    ST_TRY(predict_prep(d, L, p, params, stream));      // the parameter-only head (folded synthesis bases, their 16-bit / plane copies), once per call
    const CodeJob cj{nullptr, reinterpret_cast<const float*>(code), n_settings, out_pitch, (size_t)knob_rows * d->K};
    return with_pcm(fmt, [&](auto z) { return predict_batches<decltype(z)>(d, L, p, params, signal, n, knobs, knob_rows, out, n_out, ws, stream, nullptr, 0, &cj); });
}

// ------------------------------------------------------------------------------ many knob settings from one code (st_multi.h)
// st_score_knobs_coded and st_fit_knobs_multi_coded walk the batches of st_knob_multi_plan: rows of a batch are (setting, window) pairs.  The workspace is
// st_fit_knobs' with the per-setting gradient accumulators [S][16] and the score's per-setting loss partials [S][partials of a batch of d->B] in front of the batch
// workspace: [head | the fit's rows and scratch | acc | partials | one batch's workspace].
static size_t multi_acc_bytes(int S) { return ((size_t)S * 16 + 63) / 64 * 64 * sizeof(float); }
static size_t multi_extra_bytes(const st_dims* d, int S) { return multi_acc_bytes(S) + ((size_t)S * ola_loss_partials(d) + 63) / 64 * 64 * sizeof(float); }
static bool multi_plan_of(const st_dims* d, long long n, int n_settings, stx::MultiPlan* mp)
{
    if (!st_fit_knobs_supported(d) || n <= 0 || n_settings < 1) return false;
    const long long nwin = predict_windows(d, n);
    if (nwin > 0x7fffffffLL) return false;
    *mp = stx::multi_plan(nwin, d->B, n_settings);
    return mp->count() <= 0x7fffffffLL;
}
extern "C" int st_knob_multi_plan(const st_dims* d, long long n, int n_settings, int* out, int cap)
{
    stx::MultiPlan mp;
    if (!multi_plan_of(d, n, n_settings, &mp)) return 0;
    const long long cnt = mp.count();
    for (long long i = 0; out && i < cnt && i < cap; ++i) {
        const stx::MultiBatch b = mp.at(i);
        out[4 * i] = b.w0; out[4 * i + 1] = b.nw; out[4 * i + 2] = b.s0; out[4 * i + 3] = b.ns;
    }
    return (int)cnt;
}
extern "C" size_t st_knob_multi_ws_bytes(const st_dims* d, int n_settings)
{
    if (n_settings < 1) return 0;
    const size_t fb = st_fit_knobs_ws_bytes(d);
    return fb ? fb + multi_extra_bytes(d, n_settings) : 0;
}
// what both entries ask of the recording, the code, the knob rows and the workspace, under the entry's name (st_fit_knobs_coded's rules and wording)
static int multi_args(const char* name, const st_dims* d, Layout* L, const float* params, const void* code, int fmt, const void* signal, const void* target, long long n,
                      const float* knobs, long long knob_rows, int n_settings, const void* ws)
{
    ST_TRY(layout_named(name, d, L));
    ST_REQ(d->K >= 1, "%s: K = %d (a model without knobs has no knobs to fit)", name, d->K);
    ST_TRY(check_recording(name, params, fmt, signal, n, ws));
    ST_TRY(check_ptr(name, "code", code, 16));
    ST_TRY(check_ptr(name, "target", target, pcm_align(fmt)));
    ST_TRY(check_ptr(name, "knobs", knobs, 16));
    ST_TRY(check_knob_rows(name, d, n, knob_rows));
    ST_REQ(n_settings >= 1, "%s: n_settings = %d must be at least 1", name, n_settings);
    ST_TRY(refuse_wide(name, "st_fit_knobs_supported", d));
    const long long nwin = predict_windows(d, n);
    stx::MultiPlan mp;
    ST_REQ(multi_plan_of(d, n, n_settings, &mp), "%s: the plan of %lld windows x %d settings does not fit (st_knob_multi_plan)", name, nwin, n_settings);
    // the 32-bit element offsets of the kernels (predict_batches' guards) at the plan's largest batch: its rows are the stacked (setting, window) pairs
    const size_t rows = mp.stacked ? (size_t)mp.per * (size_t)nwin : (size_t)(nwin < d->B ? nwin : d->B);
    const size_t CW = stc::code_window_floats(L->KP / 2, d->OT);
    ST_REQ(rows * CW < ((size_t)1 << 30) && rows * d->T * d->F < ((size_t)1 << 30) && rows * d->OT * L->KP < ((size_t)1 << 30) && rows * d->T < ((size_t)1 << 24) &&
           (size_t)synth_slabs(d) * rows * d->OT * L->KP < ((size_t)1 << 30) && rows * d->T * L->KP < ((size_t)1 << 30) &&
           (size_t)knob_rows * d->K * (mp.stacked ? (size_t)mp.per : 1) < ((size_t)1 << 30),
           "%s: batch too large for the kernels' 32-bit element offsets (%zu stacked rows)", name, rows);
    return ST_OK;
}
struct MultiJob {
    const float* code; const void* target; long long nwin; int S;
    float* knobs; long long knob_rows;      // [S][knob_rows][K]
    const FitJob* fit;                      // NULL: score
    double* loss; float* win_loss;          // loss[S] of this step (or of the score); win_loss [S][nwin] or NULL
    double inv_n_d; float *acc, *lp_all;    // lp_all: [S][ola_loss_partials(d)], the score's partials of every setting of a window batch
};
template <typename T>
static int multi_batches(const st_dims* d, const Layout& L, const PredictWS& p, const float* params, const void* signal_v, long long n_out, const MultiJob& j,
                         void* ws, size_t batch_off, void* stream)
{
    const T* signal = reinterpret_cast<const T*>(signal_v);
    const FitJob* const fit = j.fit;
    const size_t CW = stc::code_window_floats(L.KP / 2, d->OT);
    const bool one = j.knob_rows == 1;
    const size_t set_stride = (size_t)j.knob_rows * d->K;
    const stx::MultiPlan mp = stx::multi_plan(j.nwin, d->B, j.S);
    const long long cnt = mp.count();
    const bool defer = !fit && !mp.stacked;      // the score of a recording that is not stacked: one tail launch per window batch, behind its last setting
    const size_t lpn = (size_t)ola_loss_partials(d);
    for (long long bi = 0; bi < cnt; ++bi) {
        const stx::MultiBatch mb = mp.at(bi);
        const InferBatch b = infer_batch(d, L, p, params, ws, batch_off, (long long)mb.nw * mb.ns);
        const st_dims& q = b.q; const WS& w = b.w;
        const size_t ro = (size_t)mb.s0 * set_stride + (one ? 0 : (size_t)mb.w0 * q.K);      // the batch's first knob row
        ST_TRY(dec_forward<true>(b, j.code + (size_t)mb.w0 * CW, (const float*)j.knobs + ro, one ? 0 : q.K, fit != nullptr, stream, mb.nw, (unsigned)set_stride));
        ST_TRY(infer_frames(b, stream));
        const int nslot = (q.y + 255) / 256;
        const long long s0 = (long long)mb.w0 * q.y;
        float* const lp = defer ? j.lp_all + (size_t)mb.s0 * lpn : w.loss_p;
        with_bool(fit != nullptr, [&](auto FIT) { ola_launch(b, [&](auto NS, auto NF, dim3 grid, size_t slab) {
            hipLaunchKernelGGL((stf::fit_ola_kernel<T, NS(), NF(), FIT() ? 1 : 2>), grid, dim3(256), 0, st_stream(stream),
                               w.frs, slab, signal, reinterpret_cast<const T*>(j.target), w.dsyn, b.g16 ? w.dsyn16 : nullptr, b.ht(), lp, nslot,
                               s0, n_out, q.L, q.N, q.H, q.OT, q.y, mb.nw); }); });
        ST_LAUNCHED("fit_ola");
        if (defer && mb.s0 + 1 < j.S) continue;
        const int ts0 = defer ? 0 : mb.s0, tns = defer ? j.S : mb.ns;      // the settings this tail launch folds
        stx::MultiTailArgs m;
        m.t = fit ? fit->hyper : stf::TailArgs{};
        m.t.inv_n_d = j.inv_n_d;
        m.t.loss_p = defer ? j.lp_all : w.loss_p; m.lp_stride = defer ? lpn : (size_t)mb.nw * nslot; m.t.n_lp = mb.nw * nslot; m.t.loss = nullptr; m.t.acc = nullptr;
        m.t.rows = nullptr; m.t.nb = mb.nw; m.t.K = q.K;
        m.t.per_window = !one; m.t.first = mb.w0 == 0; m.t.last = mb.w0 + mb.nw >= j.nwin;
        m.t.knobs = m.t.m = m.t.v = m.t.grad = nullptr;
        if (fit) {
            ST_TRY(knob_backward(b, p.knobs, *fit, stream));
            m.t.rows = fit->rows;
            m.t.knobs = fit->knobs + ro; m.t.m = fit->m + ro; m.t.v = fit->v + ro; m.t.grad = fit->grad ? fit->grad + ro : nullptr;
        }
        m.nw = mb.nw; m.nslot = nslot; m.set_stride = set_stride;
        m.loss = j.loss + ts0;
        m.win_loss = j.win_loss ? j.win_loss + (size_t)ts0 * j.nwin + mb.w0 : nullptr; m.win_pitch = j.nwin;
        m.acc = j.acc + (size_t)ts0 * 16;
        hipLaunchKernelGGL(stx::multi_tail_kernel, dim3(tns), dim3(256), 0, st_stream(stream), m);
        ST_LAUNCHED("multi_tail");
    }
    return ST_OK;
}
// what both entries' jobs have in common; acc: the per-setting accumulators behind the fit's rows and scratch (st_knob_multi_ws_bytes).  fit, loss, win_loss and
// lp_all (the score's alone) stay null for the entry to set.
static MultiJob multi_job(const st_dims* d, const void* code, const void* target, long long n, int S, float* knobs, long long knob_rows, float* acc)
{
    MultiJob j{};
    j.code = reinterpret_cast<const float*>(code); j.target = target; j.nwin = predict_windows(d, n); j.S = S; j.knobs = knobs; j.knob_rows = knob_rows;
    j.inv_n_d = 1.0 / (double)(n - ((long long)d->L - d->y));
    j.acc = acc;
    return j;
}
extern "C" int st_score_knobs_coded(const st_dims* d, const float* params, const void* code, int fmt, const void* signal, const void* target, long long n,
                                    const float* knobs, long long knob_rows, int n_settings, double* loss, float* win_loss, void* ws, void* stream)
{
    static const char* const name = "st_score_knobs_coded";
    Layout L; ST_TRY(multi_args(name, d, &L, params, code, fmt, signal, target, n, knobs, knob_rows, n_settings, ws));
    ST_REQ(loss, "%s: null pointer (loss)", name);
    const long long n_out = n - ((long long)d->L - d->y);
    if (n_out <= 0) return ST_OK;      // no output sample, no objective: nothing launched, every buffer left alone
    PredictWS p; predict_carve(d, ws, &p);
    FitWS f; fit_carve(d, reinterpret_cast<char*>(ws) + p.head_bytes, &f);
    char* const extra = reinterpret_cast<char*>(ws) + p.head_bytes + f.bytes;
    MultiJob j = multi_job(d, code, target, n, n_settings, const_cast<float*>(knobs), knob_rows, reinterpret_cast<float*>(extra));
    j.loss = loss; j.win_loss = win_loss; j.lp_all = reinterpret_cast<float*>(extra + multi_acc_bytes(n_settings));
    const size_t batch_off = p.head_bytes + f.bytes + multi_extra_bytes(d, n_settings);
    prof_mark("begin", stream);
    ST_TRY(predict_prep(d, L, p, params, stream));
    return with_pcm(fmt, [&](auto z) { return multi_batches<decltype(z)>(d, L, p, params, signal, n_out, j, ws, batch_off, stream); });
}
extern "C" int st_fit_knobs_multi_coded(const st_dims* d, const float* params, const void* code, int fmt, const void* signal, const void* target, long long n,
                                        float* knobs, long long knob_rows, int n_settings, float* adam_m, float* adam_v,
                                        long long first_step, int steps, float lr, float beta1, float beta2, float eps,
                                        double* loss_hist, float* grad_hist, void* ws, void* stream)
{
    static const char* const name = "st_fit_knobs_multi_coded";
    Layout L; ST_TRY(multi_args(name, d, &L, params, code, fmt, signal, target, n, knobs, knob_rows, n_settings, ws));
    const AdamArgs h{first_step, steps, lr, beta1, beta2, eps};
    ST_TRY(check_ptr(name, "adam_m", adam_m, 16)); ST_TRY(check_ptr(name, "adam_v", adam_v, 16)); ST_TRY(check_ptr(name, "loss_hist", loss_hist, 1));
    ST_TRY(check_adam(name, h));
    const long long n_out = n - ((long long)d->L - d->y);
    if (n_out <= 0) return ST_OK;
    PredictWS p; predict_carve(d, ws, &p);
    FitWS f; fit_carve(d, reinterpret_cast<char*>(ws) + p.head_bytes, &f);
    const size_t batch_off = p.head_bytes + f.bytes + multi_extra_bytes(d, n_settings);
    prof_mark("begin", stream);
    ST_TRY(predict_prep(d, L, p, params, stream));      // once per call, whatever the number of starts and steps
    const size_t all_floats = (size_t)n_settings * knob_rows * d->K;
    for (int s = 0; s < steps; ++s) {
        FitJob job;
        job.target = target; job.kg = f.kg; job.rows = f.rows; job.acc = nullptr;
        job.knobs = knobs; job.m = adam_m; job.v = adam_v; job.grad = grad_hist ? grad_hist + (size_t)s * all_floats : nullptr; job.loss = nullptr;
        job.hyper = adam_step(h, s, n_out);      // st_fit_knobs' scalars of this step
        MultiJob j = multi_job(d, code, target, n, n_settings, knobs, knob_rows, reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + p.head_bytes + f.bytes));
        j.fit = &job; j.loss = loss_hist + (size_t)s * n_settings;
        ST_TRY(with_pcm(fmt, [&](auto z) { return multi_batches<decltype(z)>(d, L, p, params, signal, n_out, j, ws, batch_off, stream); }));
    }
    return ST_OK;
}

// Data-parallel split of st_loss_backward: after phase 1 the synthesis + autoencoder gradients
// (grads[offs[2] ..)) are final and can be all-reduced while phase 2 (analysis wgrad) runs.
extern "C" int st_loss_backward_p1(const st_dims* d, const float* params, float* grads, const float* x, const float* knobs,
                                   const float* y_true, void* ws, void* stream)
{
    Call c; ST_TRY(call_begin(&c, d, params, knobs, ws, stream, G16_PIPELINE));
    ST_REQ(params && grads && x && (knobs || d->K == 0) && y_true && ws, "st_loss_backward_p1: null pointer");
    prof_mark("begin", stream);
    ST_TRY(forward_impl(c, params, x, y_true, nullptr, nullptr, nullptr, true));
    return backward_p1(c, params, grads, nullptr, nullptr, reg_coef_of(d));
}
extern "C" int st_loss_backward_p2(const st_dims* d, float* grads, const float* x, void* ws, float* scalars, void* stream)
{
    Call c; ST_TRY(call_begin(&c, d, nullptr, nullptr, ws, stream, G16_PIPELINE));
    ST_REQ(grads && x && ws && scalars, "st_loss_backward_p2: null pointer");
    ST_TRY(backward_p2(c, grads));
    return finalize_scalars(d, c.w.loss_p, c.w.reg_p, c.w.norm_a, c.w.norm_s, 1.0f / loss_scale_of(d), scalars, stream);
}

// As st_loss_backward_p2, and the 2F live rows of the two analysis gradients are ALSO written packed into `stage` [2F][N]:
// the data-parallel all-reduce then moves 4.2 MB instead of the 6.3 MB contiguous range that spans the dead rows of the
// first tensor (st_unstage_analysis copies the reduced rows back).
extern "C" int st_loss_backward_p2_staged(const st_dims* d, float* grads, float* stage, const float* x, void* ws, float* scalars, void* stream)
{
    Call c; ST_TRY(call_begin(&c, d, nullptr, nullptr, ws, stream, G16_PIPELINE));
    ST_REQ(grads && stage && x && ws && scalars, "st_loss_backward_p2_staged: null pointer");
    (void)scalars;      // the loss scalars are published by st_dp_clip_adam (no single-block finalize between this GEMM and the all-reduce)
    return backward_p2(c, grads, stage);
}
extern "C" int st_unstage_analysis(const st_dims* d, float* grads, const float* stage, void* stream)
{
    Layout L; ST_TRY(make_layout(d, &L));
    ST_REQ(grads && stage, "st_unstage_analysis: null pointer");
    const size_t live = (size_t)d->F * d->N * sizeof(float);
    if (hipMemcpyAsync(grads + L.offs[0], stage, live, hipMemcpyDeviceToDevice, st_stream(stream)) != hipSuccess ||
        hipMemcpyAsync(grads + L.offs[1], stage + (size_t)d->F * d->N, live, hipMemcpyDeviceToDevice, st_stream(stream)) != hipSuccess)
        return st_fail(ST_ERR_LAUNCH, "st_unstage_analysis: copy failed");
    return ST_OK;
}

// Finer data-parallel split (dp.DataParallel): stage s leaves one gradient range final, in the order
//   0: forward + loss + synthesis dgrad/wgrad   -> the two synthesis bases           grads[offs[2], offs[4])
//   1: autoencoders + polar backward             -> both autoencoders                 grads[offs[4], total)
//   2: analysis weight gradient, real basis      -> rows [0,F) of the first tensor    grads[offs[0], +F*N)
//   3: analysis weight gradient, imaginary basis -> rows [0,F) of the second tensor   grads[offs[1], +F*N)  + scalars
// so each all-reduce runs under the next stage and only the last, smallest range (2.1 MB) is exposed.
extern "C" int st_loss_backward_stage(const st_dims* d, const float* params, float* grads, const float* x, const float* knobs,
                                      const float* y_true, void* ws, float* scalars, int stage, void* stream)
{
    Call c; ST_TRY(call_begin(&c, d, params, knobs, ws, stream, FP32_OPERANDS));
    WS& w = c.w;
    ST_REQ(params && grads && x && (knobs || d->K == 0) && y_true && ws && scalars, "st_loss_backward_stage: null pointer");
    ST_REQ(stage >= 0 && stage < 4, "st_loss_backward_stage: stage %d not in 0..3", stage);
    switch (stage) {
    case 0:
        prof_mark("begin", stream);
        ST_TRY(forward_impl(c, params, x, y_true, nullptr, nullptr, nullptr, true));
        return backward_syn(c, grads);
    case 1:
        return backward_ae(c, params, grads, nullptr, nullptr, reg_coef_of(d));
    case 2:
        return backward_p2(c, grads, nullptr, 0, 0, WGP_HALVES_96);
    default:
        ST_TRY(backward_p2(c, grads, nullptr, 0, 1, WGP_HALVES_96));
        return finalize_scalars(d, w.loss_p, w.reg_p, w.norm_a, w.norm_s, 1.0f / loss_scale_of(d), scalars, stream);
    }
}

static int train_step_impl(const st_dims* d, float* params, float* grads, float* m, float* v, const float* x,
                           const float* knobs, const float* y_true, void* ws, float* scalars,
                           float lr, float beta1, float beta2, float eps, int step, void* stream, bool dev_hyper)
{
    Call c; ST_TRY(call_begin(&c, d, params, knobs, ws, stream, G16_PIPELINE));
    const Layout& L = c.L; WS& w = c.w;
    ST_REQ(params && grads && x && (knobs || d->K == 0) && y_true && ws && scalars, "st_train_step: null pointer");
    prof_mark("begin", stream);
    ST_TRY(forward_impl(c, params, x, y_true, nullptr, nullptr, nullptr, true));
    ST_TRY(backward_impl(c, params, grads, nullptr, nullptr, reg_coef_of(d)));
    // loss scalars + clip coefficient inside the optimizer kernel (st_loss_backward + st_clip_adam minus one launch)
    const float inv_s = 1.0f / loss_scale_of(d);            // the gradients carry the loss scale: unscale inside the optimizer
    stm::FinArgs f = fin_args(d, w.loss_p, w.reg_p, w.norm_a, w.norm_s, inv_s);
    if (d->clip_all) {                                       // train.py:136: the norm runs over every parameter
        if (w.n_norm_e > 0) { f.norm_e = w.norm_e; f.n_ne = w.n_norm_e; }      // the kernels that summed the autoencoder gradients left their |g| partials
        else {
            hipLaunchKernelGGL(stm::l1_partial_kernel, dim3(NORM_E_PARTIALS), dim3(256), 0, st_stream(stream),
                               grads + L.n_stft, L.total - L.n_stft, 1.0f, w.norm_e);
            ST_LAUNCHED("l1_partial_ae");
            f.norm_e = w.norm_e; f.n_ne = NORM_E_PARTIALS;
        }
    }
    return clip_adam_impl(params, grads, m, v, L.total, d->clip_all ? L.total : L.n_stft, scalars, inv_s, lr, beta1, beta2, eps, step, &f, stream, dev_hyper);
}
extern "C" int st_train_step(const st_dims* d, float* params, float* grads, float* m, float* v, const float* x,
                             const float* knobs, const float* y_true, void* ws, float* scalars,
                             float lr, float beta1, float beta2, float eps, int step, void* stream)
{
    return train_step_impl(d, params, grads, m, v, x, knobs, y_true, ws, scalars, lr, beta1, beta2, eps, step, stream, false);
}

// ------------------------------------------------------------------------------ the step with frozen parameter groups
extern "C" int st_step_groups_stages(int trainable)
{
    if (trainable < 1 || trainable > ST_GROUP_ALL) return -1;
    int s = 0;
    if (trainable & ST_GROUP_SYNTHESIS) s |= ST_STAGE_SYN_WGRAD;
    if (trainable & (ST_GROUP_AE_MAG | ST_GROUP_AE_PHS | ST_GROUP_ANALYSIS)) s |= ST_STAGE_AE_BWD | ST_STAGE_SYN_DGRAD;
    if (trainable & ST_GROUP_ANALYSIS) s |= ST_STAGE_AE_DINPUT | ST_STAGE_ANA_WGRAD;
    return s;
}
// The optimizer launch of a step is marked with the groups it updates (st_profile_report): bit g of the number = group g
static const char* const CLIP_ADAM_GROUPS[16] = {"", "clip_adam_g1", "clip_adam_g2", "clip_adam_g3", "clip_adam_g4", "clip_adam_g5", "clip_adam_g6", "clip_adam_g7",
                                                 "clip_adam_g8", "clip_adam_g9", "clip_adam_g10", "clip_adam_g11", "clip_adam_g12", "clip_adam_g13", "clip_adam_g14", "clip_adam_g15"};
extern "C" int st_train_step_groups(const st_dims* d, float* params, float* grads, float* m, float* v, const float* x,
                                    const float* knobs, const float* y_true, void* ws, float* scalars,
                                    float lr, float beta1, float beta2, float eps, const int step[4], int trainable, void* stream)
{
    ST_REQ(trainable >= 1 && trainable <= ST_GROUP_ALL, "st_train_step_groups: trainable = %d is not a non-empty set of the four ST_GROUP_* bits (1..15)", trainable);
    ST_REQ(step, "st_train_step_groups: null pointer (step)");
    for (int g = 0; g < 4; ++g)
        ST_REQ(!((trainable >> g) & 1) || step[g] >= 1, "st_train_step_groups: step[%d] = %d, the Adam step number of a trainable group must be at least 1", g, step[g]);
    if (trainable == ST_GROUP_ALL && step[0] == step[1] && step[1] == step[2] && step[2] == step[3])      // nothing frozen, one step number: the plain step, launch for launch
        return train_step_impl(d, params, grads, m, v, x, knobs, y_true, ws, scalars, lr, beta1, beta2, eps, step[0], stream, false);
    Call c; ST_TRY(call_begin(&c, d, params, knobs, ws, stream, G16_PIPELINE));
    const Layout& L = c.L; WS& w = c.w;
    ST_REQ(params && grads && m && v && x && (knobs || d->K == 0) && y_true && ws && scalars, "st_train_step_groups: null pointer");
    const int stages = st_step_groups_stages(trainable);
    prof_mark("begin", stream);
    ST_TRY(forward_impl(c, params, x, y_true, nullptr, nullptr, nullptr, true));
    ST_TRY(backward_p1(c, params, grads, nullptr, nullptr, reg_coef_of(d), nullptr, stages));
    if (stages & ST_STAGE_ANA_WGRAD) ST_TRY(backward_p2(c, grads));
    const float inv_s = 1.0f / loss_scale_of(d);
    // the clip norm: |g| partials of the trainable tensors of the clip scope only
    stm::FinArgs f = fin_args(d, w.loss_p, w.reg_p, (trainable & ST_GROUP_ANALYSIS) ? w.norm_a : nullptr, (trainable & ST_GROUP_SYNTHESIS) ? w.norm_s : nullptr, inv_s);
    const int ae_bits = trainable & (ST_GROUP_AE_MAG | ST_GROUP_AE_PHS);
    if (d->clip_all && ae_bits) {
        if (ae_bits == (ST_GROUP_AE_MAG | ST_GROUP_AE_PHS) && w.n_norm_e > 0) { f.norm_e = w.norm_e; f.n_ne = w.n_norm_e; }      // left by the kernel that summed both nets' gradients
        else {
            const int64_t b = (ae_bits & ST_GROUP_AE_MAG) ? L.offs[4] : L.offs[22], e = (ae_bits & ST_GROUP_AE_PHS) ? L.total : L.offs[22];
            hipLaunchKernelGGL(stm::l1_partial_kernel, dim3(NORM_E_PARTIALS), dim3(256), 0, st_stream(stream), grads + b, e - b, 1.0f, w.norm_e);
            ST_LAUNCHED("l1_partial_ae");
            f.norm_e = w.norm_e; f.n_ne = NORM_E_PARTIALS;
        }
    }
    // one range per run of adjacent trainable groups with one step number and one clip rule
    const int64_t gb[5] = {L.offs[0], L.offs[2], L.offs[4], L.offs[22], L.total};
    const float w1 = (float)(1.0 - (double)beta1), w2 = (float)(1.0 - (double)beta2);
    stm::AdamRanges tab; tab.n = 0;
    int64_t n4 = 0;
    for (int g = 0; g < 4; ++g) {
        if (!((trainable >> g) & 1)) continue;
        const int clipped = (g < 2 || d->clip_all) ? 1 : 0;
        const bool joins = tab.n > 0 && ((trainable >> (g - 1)) & 1) && step[g - 1] == step[g] && tab.r[tab.n - 1].clipped == clipped;
        if (joins) tab.r[tab.n - 1].e4 = gb[g + 1] / 4;
        else {
            const double bc1 = 1.0 - pow((double)beta1, step[g]), bc2 = 1.0 - pow((double)beta2, step[g]);      // as clip_adam_impl forms them
            tab.r[tab.n++] = stm::AdamRange{gb[g] / 4, gb[g + 1] / 4, clipped, (float)(-(double)lr / bc1), (float)sqrt(bc2)};
        }
        n4 += (gb[g + 1] - gb[g]) / 4;
    }
    for (int k = tab.n; k < 4; ++k) tab.r[k] = stm::AdamRange{0, 0, 0, 0.f, 1.f};
    int grid = (int)((n4 + 255) / 256); if (grid > 2048) grid = 2048; if (grid < 1) grid = 1;
    hipLaunchKernelGGL(stm::clip_adam_ranges_kernel, dim3(grid), dim3(256), 0, st_stream(stream), params, grads, m, v, tab, scalars, inv_s, w1, beta2, w2, eps, f);
    ST_LAUNCHED(CLIP_ADAM_GROUPS[trainable]); return ST_OK;
}

extern "C" int st_dp_clip_adam(const st_dims* d, float* params, float* grads, float* m, float* v, void* ws,
                               float* scalars, float grad_scale, float lr, float beta1, float beta2, float eps,
                               int step, void* stream)
{
    Call c; ST_TRY(call_begin(&c, d, nullptr, nullptr, ws, stream, G16_PIPELINE));
    const Layout& L = c.L; WS& w = c.w;
    ST_REQ(params && grads && m && v && ws && scalars, "st_dp_clip_adam: null pointer");
    // L1 norm of the all-reduced, 1/world-scaled STFT gradient: identical on every rank, no second collective
    const int np = norm_partials(d);
    const int64_t n_clip = d->clip_all ? L.total : L.n_stft;
    const float gs = grad_scale / loss_scale_of(d);          // 1/world and the loss scale leave the gradient together
    hipLaunchKernelGGL(stm::l1_partial_kernel, dim3(np), dim3(256), 0, st_stream(stream),
                       grads, n_clip, gs, w.norm_a);
    ST_LAUNCHED("l1_partial");
    stm::FinArgs f = fin_args(d, w.loss_p, w.reg_p, w.norm_a, nullptr, 1.0f);     // this rank's loss terms + the norm of the REDUCED gradient (l1 partials above)
    f.n_na = np;
    return clip_adam_impl(params, grads, m, v, L.total, n_clip, scalars, gs, lr, beta1, beta2, eps, step, &f, stream);
}

// ------------------------------------------------------------------------------ device-side data feed
extern "C" int st_compressor_4c(const float* x, const float* knobs_wc, float sr, int B, int L, int ysz, float* y, void* stream)
{
    ST_REQ(x && knobs_wc && y, "st_compressor_4c: null pointer");
    ST_REQ(B > 0 && L > 0 && ysz > 0 && ysz <= L && sr > 0.f, "st_compressor_4c: bad sizes (B=%d L=%d ysz=%d)", B, L, ysz);
    hipLaunchKernelGGL(stm::compressor_4c_kernel, dim3(B), dim3(256), 0, st_stream(stream), x, knobs_wc, sr, L, ysz, y);
    ST_LAUNCHED("compressor_4c"); return ST_OK;
}

extern "C" int st_compressor(const float* x, const float* knobs_wc, float sr, int B, int L, int ysz, float* y, void* stream)
{
    ST_REQ(x && knobs_wc && y, "st_compressor: null pointer");
    ST_REQ(B > 0 && L > 0 && ysz > 0 && ysz <= L && sr > 0.f, "st_compressor: bad sizes (B=%d L=%d ysz=%d)", B, L, ysz);
    hipLaunchKernelGGL(stm::compressor_env_kernel, dim3(B), dim3(256), 0, st_stream(stream), x, nullptr, knobs_wc, 3, sr, L, ysz, y);
    ST_LAUNCHED("compressor_env"); return ST_OK;
}

// audio.LowPass (audio.py:610-625): the third-order Butterworth low-pass as a scan over the filter's modes (st_filter.h), one workgroup per window
extern "C" int st_lowpass(const float* x, const float* knobs_wc, float sr, int B, int L, int ysz, float* y, void* stream)
{
    ST_REQ(x && knobs_wc && y, "st_lowpass: null pointer");
    ST_REQ(B > 0 && L > 0 && ysz > 0 && ysz <= L && sr > 0.f, "st_lowpass: bad sizes (B=%d L=%d ysz=%d): 0 < ysz <= L and sr > 0 are required", B, L, ysz);
    ST_REQ(L % 4 == 0, "st_lowpass: L = %d is not a multiple of 4", L);
    hipLaunchKernelGGL(stm::lowpass_kernel, dim3(B), dim3(256), 0, st_stream(stream), x, knobs_wc, sr, L, ysz, y);
    ST_LAUNCHED("lowpass"); return ST_OK;
}
// audio.Echo (audio.py:430-443, :539-547): delayed, attenuated copies of the window added to it (st_echo.h); sr is not used
extern "C" int st_echo(const float* x, const float* knobs_wc, float sr, int B, int L, int ysz, float* y, void* stream)
{
    (void)sr;
    ST_REQ(x && knobs_wc && y, "st_echo: null pointer");
    ST_REQ(B > 0 && L > 0 && ysz > 0 && ysz <= L, "st_echo: bad sizes (B=%d L=%d ysz=%d): B > 0 and 0 < ysz <= L are required", B, L, ysz);
    const int ECHO_SUB = 32768;                              // windows per launch: the grid stays far below 2^31 workgroups
    const int tiles = (ysz + 2047) / 2048;                   // eight 256-sample trips per workgroup: the taps' float64 powers are worked out once for them
    for (int b0 = 0; b0 < B; b0 += ECHO_SUB) {
        const int nb = B - b0 < ECHO_SUB ? B - b0 : ECHO_SUB;
        hipLaunchKernelGGL(stm::echo_kernel, dim3(nb, tiles < 65535 ? tiles : 65535), dim3(256), 0, st_stream(stream),
                           x + (size_t)b0 * L, knobs_wc + (size_t)b0 * 3, L, ysz, y + (size_t)b0 * ysz);
    }
    ST_LAUNCHED("echo"); return ST_OK;
}
// audio.Denoise's input (audio.py:571) for clean windows the caller brings: the noise stream of the feed (stf::denoise_add)
extern "C" int st_denoise_input(unsigned seed, unsigned long long first_window, const float* x, const float* knobs_wc, int B, int L, float* x_noisy, void* stream)
{
    ST_REQ(x && knobs_wc && x_noisy, "st_denoise_input: null pointer");
    ST_REQ(B > 0 && L > 0, "st_denoise_input: bad sizes (B=%d L=%d)", B, L);
    ST_REQ(L % 4 == 0, "st_denoise_input: L = %d is not a multiple of 4", L);
    const int chunks = (L / 4 + 255) / 256;
    hipLaunchKernelGGL(stf::denoise_input_kernel, dim3(B, chunks < 65535 ? chunks : 65535), dim3(256), 0, st_stream(stream), seed, first_window, x, knobs_wc, L, x_noisy);
    ST_LAUNCHED("denoise_input"); return ST_OK;
}

// scratch of st_synth_effect for the full-featured path: [gain curve (ST_FX_COMP: dB signal) B * L | world knobs 4 B] and, for power-of-two windows beyond the in-LDS FFT
// (8192 < L <= 65536), [1/f noise B * L | per-window peaks | four-step FFT buffer 2 * min(B, 1024) * L]
static const int FEED_FFT_SUB = 1024;      // windows per pass-1 / pass-2 launch pair of the long-window noise (a launch pair costs ~50 us whatever its size: few, large ones)
static bool feed_long_fft(int L) { return L > stf::FFT_MAX && (L & (L - 1)) == 0 && L / stf::PL_N1 <= 256; }
static bool feed_effect_ok(int effect) { return effect >= ST_FX_COMP4C && effect <= ST_FX_DECOMP4C; }
static bool feed_effect_splits(int effect) { return effect == ST_FX_COMP4C || effect == ST_FX_COMP || effect == ST_FX_DECOMP4C; }      // has a lane-per-window / second-launch form through the scratch
// The compressors' form through the scratch, the head of every feed's scratch: [gain curve or dB signal B * L | world knobs 4 B].  It is taken when the caller
// brings scratch and L % 64 == 0 (comp_smooth_kernel's tiles); the floats are part of the scratch size whatever L is.  ST_FX_LOWPASS / ST_FX_DENOISE / ST_FX_ECHO: none.
struct FeedSplit { float* gc; float* kw; explicit operator bool() const { return gc != nullptr; } };      // both NULL: the effect runs inside the feed kernel
static size_t feed_split_floats(int effect, int B, int L) { return feed_effect_splits(effect) ? (size_t)B * (L + 4) : 0; }
static FeedSplit feed_split(int effect, int B, int L, float* scratch)
{
    return scratch && L % 64 == 0 && feed_effect_splits(effect) ? FeedSplit{scratch, scratch + (size_t)B * L} : FeedSplit{nullptr, nullptr};
}
// at most 32768 windows per launch (a grid's y dimension stays below 65536): f(b0, nb) for every run of windows [b0, b0 + nb) of B
template <class F> static inline int feed_window_runs(int B, F&& f)
{
    const int SUB = 32768;
    for (int b0 = 0; b0 < B; b0 += SUB) ST_TRY(f(b0, B - b0 < SUB ? B - b0 : SUB));
    return ST_OK;
}
extern "C" size_t st_synth_effect_scratch_floats(int effect, int B, int L)
{
    if (!feed_effect_ok(effect) || B <= 0 || L <= 0) return 0;
    size_t n = feed_split_floats(effect, B, L);
    if (feed_long_fft(L)) n += (size_t)B * L + (size_t)st_round_up(B, 64) + (size_t)2 * (B < FEED_FFT_SUB ? B : FEED_FFT_SUB) * L;
    return n;
}
extern "C" size_t st_synth_comp4c_scratch_floats(int B, int L) { return st_synth_effect_scratch_floats(ST_FX_COMP4C, B, L); }
template <int FX, bool EXT>
static int feed_launch(const stf::FeedArgs& a, int B, size_t lds, void* stream)
{
    if (lds >= 65536) {      // exactly 64 KB of dynamic LDS beside a few static bytes: ask for it explicitly (the 160 KB request of ensure_dyn_lds is refused for a kernel with static LDS)
        static std::mutex mu; static std::set<int> done;
        int dev = 0; (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lk(mu);
        if (!done.count(dev)) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&stf::synth_feed_kernel<FX, EXT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return st_fail(ST_ERR_LAUNCH, "hipFuncSetAttribute(synth_feed_kernel, %zu B dynamic LDS): %s", lds, hipGetErrorString(e));
            done.insert(dev);
        }
    }
    hipLaunchKernelGGL((stf::synth_feed_kernel<FX, EXT>), dim3(B), dim3(256), lds, st_stream(stream), a);
    ST_LAUNCHED(FX == ST_FX_COMP ? "synth_comp" : FX == ST_FX_LOWPASS ? "synth_lowpass" : FX == ST_FX_DENOISE ? "synth_denoise" : FX == ST_FX_ECHO ? "synth_echo" :
                FX == ST_FX_DECOMP4C ? "synth_decomp4c" : "synth_comp4c"); return ST_OK;
}
// what every feed refuses about the effect, its knob count and (host arrays, checked as soon as they are there) its knob ranges
static int feed_effect_check(const char* who, int effect, int K, float sr, const float* knob_lo, const float* knob_hi)
{
    ST_REQ(feed_effect_ok(effect), "%s: effect %d is not an ST_FX_* id (ST_FX_COMP4C = 0, ST_FX_COMP = 1, ST_FX_LOWPASS = 2, ST_FX_DENOISE = 3, ST_FX_ECHO = 4, ST_FX_DECOMP4C = 5)", who, effect);
    ST_REQ(effect != ST_FX_COMP4C || (K >= 1 && K <= 4), "%s: ST_FX_COMP4C takes 1 to 4 knobs, not K=%d", who, K);
    ST_REQ(effect != ST_FX_COMP || K == 3, "%s: ST_FX_COMP takes 3 knobs (threshold, ratio, attack/release), not K=%d", who, K);
    ST_REQ(effect != ST_FX_LOWPASS || K == 1, "%s: ST_FX_LOWPASS takes 1 knob (cutoff Hz), not K=%d", who, K);
    ST_REQ(effect != ST_FX_DENOISE || K == 1, "%s: ST_FX_DENOISE takes 1 knob (strength), not K=%d", who, K);
    ST_REQ(effect != ST_FX_ECHO || K == 3, "%s: ST_FX_ECHO takes 3 knobs (delay in samples, ratio, echoes), not K=%d", who, K);
    ST_REQ(effect != ST_FX_DECOMP4C || (K >= 1 && K <= 4), "%s: ST_FX_DECOMP4C takes 1 to 4 knobs, not K=%d", who, K);
    // the one-knob effects' and the echo's ranges (host arrays): checked as soon as they are there, before the device pointers
    ST_REQ(effect != ST_FX_LOWPASS || !knob_lo || !knob_hi || (knob_lo[0] > 0.f && knob_lo[0] <= knob_hi[0] && knob_hi[0] < 0.5f * sr),
           "%s: ST_FX_LOWPASS needs a cutoff range with 0 < lo <= hi < sr / 2 (lo=%g hi=%g sr=%g)", who, knob_lo[0], knob_hi[0], sr);
    ST_REQ(effect != ST_FX_DENOISE || !knob_lo || !knob_hi || (knob_lo[0] >= 0.f && knob_lo[0] <= knob_hi[0]),
           "%s: ST_FX_DENOISE needs a strength range with 0 <= lo <= hi (lo=%g hi=%g)", who, knob_lo[0], knob_hi[0]);
    if (effect == ST_FX_ECHO && knob_lo && knob_hi) {      // the delay and the echo count are rounded half to even (Echo.go_wc), so the rounded ends decide
        ST_REQ(rintf(knob_lo[0]) >= 1.f && knob_lo[0] <= knob_hi[0] && knob_hi[0] <= 3.402823466e38f,
               "%s: ST_FX_ECHO needs a delay range with 1 <= rint(lo), lo <= hi, finite (lo=%g hi=%g)", who, knob_lo[0], knob_hi[0]);
        ST_REQ(fabsf(knob_lo[1]) <= 3.402823466e38f && fabsf(knob_hi[1]) <= 3.402823466e38f && knob_lo[1] <= knob_hi[1],
               "%s: ST_FX_ECHO needs a finite ratio range with lo <= hi (lo=%g hi=%g)", who, knob_lo[1], knob_hi[1]);
        ST_REQ(rintf(knob_lo[2]) >= 0.f && rintf(knob_hi[2]) <= (float)ST_ECHO_MAX && knob_lo[2] <= knob_hi[2],
               "%s: ST_FX_ECHO needs an echoes range with 0 <= rint(lo), rint(hi) <= ST_ECHO_MAX = %d, lo <= hi (lo=%g hi=%g)", who, (int)ST_ECHO_MAX, knob_lo[2], knob_hi[2]);
    }
    return ST_OK;
}
// the second launches of the compressors' form through the scratch (gc [B][L] gain curve or dB signal, kw [B][4] world knobs): once per row, comp_smooth_kernel works in place
static int feed_effect_finish(int effect, int B, int L, int ysz, float sr, float* x, float* y, float* gc, const float* kw, void* stream)
{
    if (effect == ST_FX_DECOMP4C) {      // the target, the clean tail, is out; the window in x becomes the compressed one
        hipLaunchKernelGGL(stm::comp_smooth_kernel, dim3((B + 63) / 64), dim3(64), 0, st_stream(stream), gc, kw, sr, B, L);
        ST_LAUNCHED("comp_smooth");
        hipLaunchKernelGGL(stm::comp_apply_inplace_kernel, dim3((L + 2047) / 2048 < 65535 ? (L + 2047) / 2048 : 65535, B), dim3(256), 0, st_stream(stream), x, gc, L);
        ST_LAUNCHED("comp_apply_inplace");
    } else if (effect == ST_FX_COMP) {
        hipLaunchKernelGGL(stm::compressor_env_kernel, dim3(B), dim3(256), 0, st_stream(stream), x, gc, kw, 4, sr, L, ysz, y);
        ST_LAUNCHED("compressor_env");
    } else if (effect == ST_FX_COMP4C) {
        hipLaunchKernelGGL(stm::comp_smooth_kernel, dim3((B + 63) / 64), dim3(64), 0, st_stream(stream), gc, kw, sr, B, L);
        ST_LAUNCHED("comp_smooth");
        hipLaunchKernelGGL(stm::comp_apply_kernel, dim3((ysz + 255) / 256, B), dim3(256), 0, st_stream(stream), x, gc, L, ysz, y);
        ST_LAUNCHED("comp_apply");
    }
    return ST_OK;
}
// st_synth_effect (families = the compressor's set, today's family rule) and st_synth_effect_families (who names the entry in the messages).
// finish = false (st_live_feed): the generator only -- the caller runs feed_effect_finish after it has replaced rows
static int synth_effect_run(const char* who, int effect, unsigned families, bool any_family, unsigned seed, unsigned long long first_window, int B, int L, int ysz,
                            int K, float sr, const float* knob_lo, const float* knob_hi, int augment, int chooser, const float* pink_in,
                            float* x, float* y, float* knobs, float* scratch, void* stream, bool finish = true)
{
    ST_TRY(feed_effect_check(who, effect, K, sr, knob_lo, knob_hi));
    ST_REQ(x && y && knobs && knob_lo && knob_hi, "%s: null pointer", who);
    ST_REQ(B > 0 && L > 0 && ysz > 0 && ysz <= L && sr > 0.f, "%s: bad sizes (B=%d L=%d ysz=%d K=%d)", who, B, L, ysz, K);
    ST_REQ(any_family || chooser == -1 || chooser == 0 || chooser == 1 || chooser == 2 || chooser == 4 || chooser == 6 || chooser == 7 || chooser == 100, "%s: signal family %d is not built (the compressor's set is 0,1,2,4,6,7)", who, chooser);
    // the kernel it always was unless a family beyond the compressor's set can come out
    const bool ext = chooser >= 0 ? (chooser != 100 && !((stf::FAMILIES_COMPRESSOR >> chooser) & 1u)) : families != stf::FAMILIES_COMPRESSOR;
    const bool fft_ok = L <= stf::FFT_MAX && (L & (L - 1)) == 0;
    const bool long_fft = !fft_ok && !pink_in && scratch && feed_long_fft(L);      // scratch is then st_synth_effect_scratch_floats(effect, B, L) floats (contract)
    ST_REQ(fft_ok || pink_in || long_fft, "%s: a %d-sample window needs either the 1/f noise from the caller (pink_in) or -- powers of two up to 65536 -- "
           "st_synth_effect_scratch_floats() floats of scratch for the library's own transform", who, L);
    stf::FeedArgs a;
    a.x = x; a.y = y; a.knobs = knobs; a.pink_in = pink_in; a.pink_peak = nullptr; a.seed = seed; a.first = first_window;
    a.L = L; a.ysz = ysz; a.K = K; a.sr = sr; a.augment = augment; a.chooser = chooser; a.families = families;
    for (int k = 0; k < 4; ++k) { a.lo[k] = knob_lo[k]; a.hi[k] = knob_hi[k]; }
    const FeedSplit split = feed_split(effect, B, L, scratch);
    a.gc = split.gc; a.kw = split.kw;
    if (long_fft) {
        // the window's 1/f noise by the library's own four-step inverse FFT (st_feed.h pink_long_pass1 / 2), 1024 windows at a time through the FFT buffer
        float* pink = scratch + feed_split_floats(effect, B, L);
        float* peak = pink + (size_t)B * L;
        float2* fbuf = reinterpret_cast<float2*>(peak + st_round_up(B, 64));
        const int N2 = L / stf::PL_N1;
        for (int b0 = 0; b0 < B; b0 += FEED_FFT_SUB) {
            const int nb = B - b0 < FEED_FFT_SUB ? B - b0 : FEED_FFT_SUB;
            hipLaunchKernelGGL(stf::pink_long_pass1_kernel, dim3(stf::PL_N1 / stf::PL_G, nb), dim3(256), 0, st_stream(stream), seed, first_window + (unsigned long long)b0, L, chooser, families, fbuf, peak + b0);
            hipLaunchKernelGGL(stf::pink_long_pass2_kernel, dim3(N2 / stf::PL_G, nb), dim3(256), 0, st_stream(stream), seed, first_window + (unsigned long long)b0, L, chooser, families,
                               (const float2*)fbuf, pink + (size_t)b0 * L, peak + b0);
        }
        ST_LAUNCHED("pink_long");
        a.pink_in = pink; a.pink_peak = peak;
    }
    // dynamic LDS: the in-LDS FFT's buffer, else the in-kernel effect's (compressor_window's float[COMP_CH] holds the envelope scan's EnvLds as well)
    static_assert(sizeof(stm::EnvLds) <= (size_t)stm::COMP_CH * sizeof(float), "the envelope scan's LDS must fit the in-kernel effect's buffer");
    static_assert(sizeof(stm::LpLds) <= (size_t)stm::COMP_CH * sizeof(float), "the low-pass scan's LDS must fit the in-kernel effect's buffer");
    static_assert(sizeof(stm::EchoLds) <= (size_t)stm::COMP_CH * sizeof(float), "the echo's taps must fit the in-kernel effect's buffer");
    const size_t lds = a.pink_in ? (split ? 0 : (size_t)stm::COMP_CH * sizeof(float)) : (size_t)stf::FFT_MAX * sizeof(float2);
    ST_TRY(with_fx(effect, [&](auto FX) { return with_bool(ext, [&](auto EXT) { return feed_launch<FX(), EXT()>(a, B, lds, stream); }); }));
    return split && finish ? feed_effect_finish(effect, B, L, ysz, sr, x, y, a.gc, a.kw, stream) : ST_OK;
}
extern "C" int st_synth_effect(int effect, unsigned seed, unsigned long long first_window, int B, int L, int ysz, int K, float sr,
                               const float* knob_lo, const float* knob_hi, int augment, int chooser, const float* pink_in,
                               float* x, float* y, float* knobs, float* scratch, void* stream)
{
    return synth_effect_run("st_synth_effect", effect, stf::FAMILIES_COMPRESSOR, false, seed, first_window, B, L, ysz, K, sr, knob_lo, knob_hi, augment, chooser, pink_in,
                            x, y, knobs, scratch, stream);
}
static int family_mask_check(const char* who, unsigned family_mask)
{
    ST_REQ(family_mask != 0u, "%s: family_mask is empty (bit f allows signal family f, f in 0..11; ST_FAMILIES_COMPRESSOR = 0xD7)", who);
    ST_REQ((family_mask & ~stf::FAMILIES_ALL) == 0u, "%s: family_mask 0x%X has bits past family 11 (the superposition, chooser >= 12, is not built)", who, family_mask);
    return ST_OK;
}
// The same feed over a caller-chosen set of signal families (all twelve of audio.synth_input_sample are built; the superposition is not)
extern "C" int st_synth_effect_families(int effect, unsigned family_mask, unsigned seed, unsigned long long first_window, int B, int L, int ysz, int K, float sr,
                                        const float* knob_lo, const float* knob_hi, int augment, int chooser, const float* pink_in,
                                        float* x, float* y, float* knobs, float* scratch, void* stream)
{
    ST_TRY(family_mask_check("st_synth_effect_families", family_mask));
    ST_REQ(chooser == -1 || chooser == 100 || chooser < 12, "st_synth_effect_families: the superposition of two signals (chooser %d >= 12) is not built; "
           "a forced family is 0..11, or 100 for the bare 1/f noise, or -1 to draw from family_mask", chooser);
    ST_REQ(chooser >= -1, "st_synth_effect_families: forced family %d: 0..11, or 100 for the bare 1/f noise, or -1 to draw from family_mask", chooser);
    return synth_effect_run("st_synth_effect_families", effect, family_mask, true, seed, first_window, B, L, ysz, K, sr, knob_lo, knob_hi, augment, chooser, pink_in,
                            x, y, knobs, scratch, stream);
}
extern "C" int st_synth_comp4c(unsigned seed, unsigned long long first_window, int B, int L, int ysz, int K, float sr,
                               const float* knob_lo, const float* knob_hi, int augment, int chooser, const float* pink_in,
                               float* x, float* y, float* knobs, float* scratch, void* stream)
{
    ST_REQ(K == 4, "st_synth_comp4c: bad sizes (B=%d L=%d ysz=%d K=%d)", B, L, ysz, K);
    return st_synth_effect(ST_FX_COMP4C, seed, first_window, B, L, ysz, K, sr, knob_lo, knob_hi, augment, chooser, pink_in, x, y, knobs, scratch, stream);
}

// what every feed of recorded input refuses about its window sizes, and about the pool it cuts them from
static int feed_window_check(const char* who, int B, int L, int ysz, int nfiles)
{
    ST_REQ(B > 0 && L > 0 && ysz > 0 && nfiles > 0, "%s: bad sizes: B, L, ysz and nfiles must be positive (B=%d L=%d ysz=%d nfiles=%d)", who, B, L, ysz, nfiles);
    ST_REQ(ysz <= L, "%s: ysz = %d exceeds L = %d (the target is the last ysz samples of the window)", who, ysz, L);
    ST_REQ(L % 4 == 0 && ysz % 4 == 0, "%s: L = %d and ysz = %d must be multiples of 4 (the st_dims rule: 16-byte rows)", who, L, ysz);
    return ST_OK;
}
static int feed_pool_check(const char* who, int fmt, int L, long long min_len, long long pool_samples)
{
    ST_REQ(fmt == ST_PCM_F32 || fmt == ST_PCM_S16, "%s: fmt = %d is not an ST_PCM_* id (ST_PCM_F32 = 0, ST_PCM_S16 = 1)", who, fmt);
    ST_REQ(min_len > (long long)L, "%s: min_len = %lld: every file must be longer than the window L = %d", who, min_len, L);
    ST_REQ(pool_samples >= min_len, "%s: pool_samples = %lld is below min_len = %lld", who, pool_samples, min_len);
    return ST_OK;
}
// The feed of recorded input / target pairs (st_feed_files.h): B windows cut out of the device-resident audio pool in one launch.
extern "C" int st_file_feed(unsigned seed, unsigned long long first_window, int B, int L, int ysz, int K, int fmt,
                            const void* pool_x, const void* pool_y, const long long* file_off, const long long* file_len, int nfiles,
                            long long min_len, long long pool_samples, const float* file_knobs, int augment,
                            float* x, float* y, float* knobs, long long* meta, void* stream)
{
    ST_REQ(pool_x && file_off && file_len && x, "st_file_feed: null pointer (pool_x, file_off, file_len and x are required)");
    ST_REQ(!y || pool_y, "st_file_feed: null pointer (pool_y is required when y is asked for)");
    ST_TRY(feed_window_check("st_file_feed", B, L, ysz, nfiles));
    ST_REQ(K >= 0 && K <= 16, "st_file_feed: K = %d knobs is outside [0, 16]", K);
    ST_REQ(K == 0 || (file_knobs && knobs), "st_file_feed: null pointer (file_knobs and knobs are required when K = %d > 0)", K);
    ST_REQ(K > 0 || !file_knobs, "st_file_feed: file_knobs must be NULL when K = 0");
    ST_TRY(feed_pool_check("st_file_feed", fmt, L, min_len, pool_samples));
    stf::FileFeedArgs a;
    a.pool_x = pool_x; a.pool_y = pool_y; a.file_off = file_off; a.file_len = file_len; a.file_knobs = file_knobs;
    a.pool_samples = pool_samples; a.seed = seed; a.L = L; a.ysz = ysz; a.K = K; a.nfiles = nfiles; a.augment = augment ? 1 : 0;
    a.nsx = (L + stf::FILE_SEG - 1) / stf::FILE_SEG;
    const int nsy = y ? (ysz + stf::FILE_SEG - 1) / stf::FILE_SEG : 0;
    return feed_window_runs(B, [&](int b0, int nb) -> int {
        a.first = first_window + (unsigned long long)b0;
        a.x = x + (size_t)b0 * L; a.y = y ? y + (size_t)b0 * ysz : nullptr; a.knobs = knobs ? knobs + (size_t)b0 * K : nullptr;
        a.meta = meta ? meta + (size_t)b0 * 3 : nullptr;
        with_pcm(fmt, [&](auto T) { hipLaunchKernelGGL(stf::file_feed_kernel<decltype(T)>, dim3(a.nsx + nsy, nb), dim3(256), 0, st_stream(stream), a); });
        ST_LAUNCHED(fmt == ST_PCM_S16 ? "file_feed_s16" : "file_feed_f32"); return ST_OK;
    });
}

// The feed of recorded input through a live effect (st_feed_live.h): per window a span of the audio pool, fresh knobs and the effect on the spot; a
// share synth_prob of the windows are st_synth_effect_families' instead.
extern "C" size_t st_live_feed_scratch_floats(int effect, int B, int L, float synth_prob)
{
    if (synth_prob > 0.f) return st_synth_effect_scratch_floats(effect, B, L);      // the synthetic rows' generator shares the scratch
    if (!feed_effect_ok(effect) || B <= 0 || L <= 0) return 0;
    return feed_split_floats(effect, B, L);
}
// what st_live_feed and st_live_feed_stream refuse alike, before any launch, and the kernel arguments they share (gc / kw stay NULL: st_live_feed sets them)
static int live_feed_prepare(const char* who, int effect, unsigned family_mask, float synth_prob, unsigned seed, unsigned long long first_window,
                             int B, int L, int ysz, int K, float sr, const float* knob_lo, const float* knob_hi, int augment,
                             int fmt, const void* pool_x, const long long* file_off, const long long* file_len, int nfiles, long long min_len, long long pool_samples,
                             float* x, float* y, float* knobs, long long* meta, stf::LiveFeedArgs& a)
{
    ST_REQ(knob_lo && knob_hi, "%s: null pointer (knob_lo and knob_hi, four host floats each, are required)", who);
    ST_TRY(feed_effect_check(who, effect, K, sr, knob_lo, knob_hi));
    ST_TRY(feed_window_check(who, B, L, ysz, nfiles));
    ST_REQ(sr > 0.f, "%s: sr = %g must be positive", who, sr);
    ST_REQ(synth_prob >= 0.f && synth_prob <= 1.f, "%s: synth_prob = %g is not a probability in [0, 1]", who, synth_prob);      // refuses NaN as well
    ST_TRY(feed_pool_check(who, fmt, L, min_len, pool_samples));
    ST_REQ(pool_x && file_off && file_len, "%s: null pointer (pool_x, file_off and file_len are required)", who);
    ST_REQ(x && y && knobs, "%s: null pointer (x, y and knobs are required)", who);
    if (synth_prob > 0.f) ST_TRY(family_mask_check(who, family_mask));
    a.pool = pool_x; a.file_off = file_off; a.file_len = file_len; a.x = x; a.y = y; a.knobs = knobs; a.meta = meta; a.gc = nullptr; a.kw = nullptr;
    a.pool_samples = pool_samples; a.seed = seed; a.first = first_window; a.L = L; a.ysz = ysz; a.K = K; a.nfiles = nfiles; a.augment = augment ? 1 : 0;
    a.sr = sr; a.synth_prob = synth_prob;
    for (int k = 0; k < 4; ++k) { a.lo[k] = knob_lo[k]; a.hi[k] = knob_hi[k]; }
    return ST_OK;
}
extern "C" int st_live_feed(int effect, unsigned family_mask, float synth_prob, unsigned seed, unsigned long long first_window,
                            int B, int L, int ysz, int K, float sr, const float* knob_lo, const float* knob_hi, int augment,
                            int fmt, const void* pool_x, const long long* file_off, const long long* file_len, int nfiles,
                            long long min_len, long long pool_samples,
                            float* x, float* y, float* knobs, long long* meta, float* scratch, void* stream)
{
    const char* who = "st_live_feed";
    stf::LiveFeedArgs a;
    ST_TRY(live_feed_prepare(who, effect, family_mask, synth_prob, seed, first_window, B, L, ysz, K, sr, knob_lo, knob_hi, augment, fmt, pool_x, file_off, file_len, nfiles,
                             min_len, pool_samples, x, y, knobs, meta, a));
    const FeedSplit split = feed_split(effect, B, L, scratch);
    a.gc = split.gc; a.kw = split.kw;
    // synthetic rows: the generator of st_synth_effect_families over the whole batch (its checks, the long windows' scratch contract among them, come before its
    // first launch); the recorded rows are overwritten below and the scratch form's second launches run once, after both
    if (synth_prob > 0.f)
        ST_TRY(synth_effect_run(who, effect, family_mask, true, seed, first_window, B, L, ysz, K, sr, knob_lo, knob_hi, augment, -1, nullptr, x, y, knobs, scratch, stream, false));
    if (synth_prob < 1.f || meta) {
        const size_t lds = split || effect == ST_FX_DENOISE ? 0 : (size_t)stm::COMP_CH * sizeof(float);      // the in-workgroup effect's buffer (synth_effect_run's static_asserts)
        with_fx(effect, [&](auto FX) { with_pcm(fmt, [&](auto T) {
            hipLaunchKernelGGL((stf::live_feed_kernel<FX(), decltype(T)>), dim3(B), dim3(256), lds, st_stream(stream), a); }); });
        ST_LAUNCHED(fmt == ST_PCM_S16 ? "live_feed_s16" : "live_feed_f32");
    }
    return split ? feed_effect_finish(effect, B, L, ysz, sr, x, y, split.gc, split.kw, stream) : ST_OK;
}

// st_live_feed with the effect's history (st_feed_stream.h).  Scratch of the pre-roll form, P = round_up(preroll + L, 64):
// [world knobs 4 B | R per row (int32; -1: synthetic) round_up(B, 4) | B * P rows, right-aligned (not ST_FX_DENOISE) | st_live_feed's scratch (synth_prob > 0)]
static const char* stream_limit(int B, int L, int preroll)
{
    if (preroll < 0) return "preroll is negative";
    if (preroll % 4 != 0) return "preroll is not a multiple of 4 (the history keeps the 4-sample rule of the rows)";
    if (preroll > (int)ST_LIVE_PREROLL_MAX) return "preroll exceeds ST_LIVE_PREROLL_MAX = 4194304 samples";
    const long long P = ((long long)preroll + (long long)(L > 0 ? L : 0) + 63) / 64 * 64;
    if (P >= 0x7fffffffLL - 64) return "preroll + L leaves the 32-bit row index (preroll + L < 2^31 - 64 is required)";
    if ((long long)(B > 0 ? B : 0) * P >= (1ll << 40)) return "B * (preroll + L) leaves the offset arithmetic (below 2^40 elements is required)";
    return nullptr;
}
static int stream_pitch(int L, int preroll) { return (int)(((long long)preroll + L + 63) / 64 * 64); }
extern "C" size_t st_live_feed_stream_scratch_floats(int effect, int B, int L, int preroll, float synth_prob)
{
    if (preroll == 0) return st_live_feed_scratch_floats(effect, B, L, synth_prob);
    if (!feed_effect_ok(effect) || B <= 0 || L <= 0 || L % 4 != 0 || stream_limit(B, L, preroll)) return 0;
    size_t n = (size_t)4 * B + (size_t)st_round_up(B, 4);
    if (effect != ST_FX_DENOISE) n += (size_t)B * stream_pitch(L, preroll);
    return n + (synth_prob > 0.f ? st_live_feed_scratch_floats(effect, B, L, synth_prob) : 0);
}
extern "C" int st_live_feed_stream(int effect, unsigned family_mask, float synth_prob, int preroll, unsigned seed, unsigned long long first_window,
                                   int B, int L, int ysz, int K, float sr, const float* knob_lo, const float* knob_hi, int augment,
                                   int fmt, const void* pool_x, const long long* file_off, const long long* file_len, int nfiles,
                                   long long min_len, long long pool_samples,
                                   float* x, float* y, float* knobs, long long* meta, float* scratch, void* stream)
{
    const char* who = "st_live_feed_stream";
    if (preroll == 0)      // today's feed: the same launches, the same scratch contract
        return st_live_feed(effect, family_mask, synth_prob, seed, first_window, B, L, ysz, K, sr, knob_lo, knob_hi, augment, fmt, pool_x, file_off, file_len, nfiles,
                            min_len, pool_samples, x, y, knobs, meta, scratch, stream);
    const char* why = stream_limit(B, L, preroll);
    ST_REQ(!why, "%s: %s (preroll=%d B=%d L=%d)", who, why, preroll, B, L);
    ST_REQ(scratch, "%s: null pointer (scratch, st_live_feed_stream_scratch_floats() floats, is required with preroll = %d > 0)", who, preroll);
    stf::StreamFeedArgs s;
    ST_TRY(live_feed_prepare(who, effect, family_mask, synth_prob, seed, first_window, B, L, ysz, K, sr, knob_lo, knob_hi, augment, fmt, pool_x, file_off, file_len, nfiles,
                             min_len, pool_samples, x, y, knobs, meta, s.live));
    const int P = stream_pitch(L, preroll);
    const bool gain = effect == ST_FX_COMP4C || effect == ST_FX_DECOMP4C;
    s.kw = scratch; s.rr = reinterpret_cast<int*>(scratch + (size_t)4 * B);
    float* rest = scratch + (size_t)4 * B + (size_t)st_round_up(B, 4);
    s.buf = effect == ST_FX_DENOISE ? nullptr : rest;
    if (effect != ST_FX_DENOISE) rest += (size_t)B * P;
    s.P = P; s.preroll = preroll;
    // synthetic rows: the generator of st_synth_effect_families over the whole batch and, where it left the compressors' chain to second launches, that chain at
    // pitch L over its own part of the scratch -- all before the recorded rows are written, so no row passes an in-place stage twice
    if (synth_prob > 0.f) {
        float* scr_l = st_live_feed_scratch_floats(effect, B, L, synth_prob) ? rest : nullptr;
        ST_TRY(synth_effect_run(who, effect, family_mask, true, seed, first_window, B, L, ysz, K, sr, knob_lo, knob_hi, augment, -1, nullptr, x, y, knobs, scr_l, stream, false));
        if (const FeedSplit sp = feed_split(effect, B, L, scr_l)) ST_TRY(feed_effect_finish(effect, B, L, ysz, sr, x, y, sp.gc, sp.kw, stream));
    }
    const size_t lds = gain || effect == ST_FX_DENOISE ? 0 : (size_t)stm::COMP_CH * sizeof(float);      // the in-workgroup effect's buffer (synth_effect_run's static_asserts)
    with_fx(effect, [&](auto FX) { with_pcm(fmt, [&](auto T) {
        hipLaunchKernelGGL((stf::stream_feed_kernel<FX(), decltype(T)>), dim3(B), dim3(256), lds, st_stream(stream), s); }); });
    ST_LAUNCHED(fmt == ST_PCM_S16 ? "stream_feed_s16" : "stream_feed_f32");
    if (!gain) return ST_OK;
    // the recorded rows' chain at pitch P: history tiles advance the state, only the tiles the apply kernel reads are stored
    const int keep0 = (P - (effect == ST_FX_DECOMP4C ? L : ysz)) & ~63;
    hipLaunchKernelGGL(stf::stream_smooth_kernel, dim3((B + 63) / 64), dim3(64), 0, st_stream(stream), s.buf, (const float*)s.kw, (const int*)s.rr, sr, B, L, P, keep0);
    ST_LAUNCHED("stream_smooth");
    feed_window_runs(B, [&](int b0, int nb) -> int {
        if (effect == ST_FX_DECOMP4C)
            hipLaunchKernelGGL(stf::stream_apply_inplace_kernel, dim3((L + 2047) / 2048 < 65535 ? (L + 2047) / 2048 : 65535, nb), dim3(256), 0, st_stream(stream),
                               x + (size_t)b0 * L, (const float*)s.buf + (size_t)b0 * P, (const int*)s.rr + b0, L, P);
        else
            hipLaunchKernelGGL(stf::stream_apply_kernel, dim3((ysz + 255) / 256, nb), dim3(256), 0, st_stream(stream),
                               (const float*)x + (size_t)b0 * L, (const float*)s.buf + (size_t)b0 * P, (const int*)s.rr + b0, L, P, ysz, y + (size_t)b0 * ysz);
        return ST_OK;
    });
    ST_LAUNCHED(effect == ST_FX_DECOMP4C ? "stream_apply_inplace" : "stream_apply");
    return ST_OK;
}

// ------------------------------------------------------------------------------ a folder of recordings through an effect (st_render_pool.h)
// gen_dataset.py's render in one call: every file of the pool whole through the effect at its own knob setting.  The scratch is [row_off int64 [nfiles + 1], padded
// to 64 floats | one row of round_up(len, 64) floats per file]; ST_FX_DENOISE streams from the pool to out and needs none.
static const long long RENDER_LEN_LIMIT = (1ll << 31) - 64;      // a file's length and every row index stay inside 32 bits
static size_t render_head_floats(int nfiles) { return ((size_t)2 * ((size_t)nfiles + 1) + 63) / 64 * 64; }
extern "C" size_t st_render_pool_scratch_floats(int effect, const long long* file_len_host, int nfiles)
{
    if (!feed_effect_ok(effect) || !file_len_host || nfiles < 1) return 0;
    size_t n = 0;
    for (int f = 0; f < nfiles; ++f) {
        const long long len = file_len_host[f];
        if (len < 0 || len >= RENDER_LEN_LIMIT) return 0;
        n += (size_t)((len + 63) & ~63ll);
    }
    return effect == ST_FX_DENOISE ? 0 : render_head_floats(nfiles) + n;
}
extern "C" int st_render_pool(int effect, float sr, int fmt, const void* pool_x, const long long* file_off, const long long* file_len, int nfiles,
                              long long max_len, long long pool_samples, const float* knobs_wc, unsigned seed, unsigned long long first_file,
                              float* out, float* scratch, void* stream)
{
    const char* who = "st_render_pool";
    ST_REQ(feed_effect_ok(effect), "%s: effect = %d is not an ST_FX_* id", who, effect);
    ST_REQ(fmt == ST_PCM_F32 || fmt == ST_PCM_S16, "%s: fmt = %d is neither ST_PCM_F32 nor ST_PCM_S16", who, fmt);
    ST_REQ(nfiles >= 1, "%s: nfiles = %d must be at least 1", who, nfiles);
    ST_REQ(pool_samples >= 1, "%s: pool_samples = %lld must be at least 1", who, pool_samples);
    ST_REQ(max_len >= 0 && max_len < RENDER_LEN_LIMIT, "%s: max_len = %lld must lie in [0, 2^31 - 64)", who, max_len);
    ST_REQ(sr > 0.f, "%s: sr = %g must be positive", who, (double)sr);
    ST_TRY(check_ptr(who, "pool_x", pool_x, pcm_align(fmt)));
    ST_TRY(check_ptr(who, "file_off", file_off, 1)); ST_TRY(check_ptr(who, "file_len", file_len, 1));
    ST_TRY(check_ptr(who, "knobs_wc", knobs_wc, 1));
    ST_TRY(check_ptr(who, "out", out, 16));
    const bool needs_scratch = effect != ST_FX_DENOISE;
    ST_REQ(scratch || !needs_scratch, "%s: null pointer (scratch, st_render_pool_scratch_floats() floats, is required for effect %d)", who, effect);
    ST_REQ((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    if (max_len == 0) return ST_OK;      // every file is empty: nothing is written
    str::Pool p{pool_x, file_off, file_len, nfiles, pool_samples, max_len, knobs_wc, nullptr, nullptr, out};
    const long long tl = (max_len + str::TILE - 1) / str::TILE;
    const dim3 tiled((unsigned)nfiles, (unsigned)(tl < 65535 ? tl : 65535));      // (file, 2048-sample tile); the kernels stride over the tiles beyond 65535
    prof_mark("begin", stream);
    if (effect == ST_FX_DENOISE) {
        with_pcm(fmt, [&](auto z) { hipLaunchKernelGGL(str::render_denoise_kernel<decltype(z)>, tiled, dim3(256), 0, st_stream(stream), p, seed, first_file); });
        ST_LAUNCHED("render_denoise"); return ST_OK;
    }
    p.row_off = reinterpret_cast<long long*>(scratch); p.rows = scratch + render_head_floats(nfiles);
    hipLaunchKernelGGL(str::render_rows_kernel, dim3(1), dim3(256), 0, st_stream(stream), p);
    ST_LAUNCHED("render_rows");
    const bool gain = effect == ST_FX_COMP4C || effect == ST_FX_DECOMP4C;
    with_pcm(fmt, [&](auto z) {
        if (gain) hipLaunchKernelGGL((str::render_stage_kernel<decltype(z), true>), tiled, dim3(256), 0, st_stream(stream), p);
        else hipLaunchKernelGGL((str::render_stage_kernel<decltype(z), false>), tiled, dim3(256), 0, st_stream(stream), p); });
    ST_LAUNCHED("render_stage");
    if (gain) {
        hipLaunchKernelGGL(str::render_smooth_kernel, dim3((unsigned)(((long long)nfiles + 63) / 64)), dim3(64), 0, st_stream(stream), p, sr);
        ST_LAUNCHED("render_smooth");
        with_pcm(fmt, [&](auto z) { hipLaunchKernelGGL(str::render_apply_kernel<decltype(z)>, tiled, dim3(256), 0, st_stream(stream), p); });
        ST_LAUNCHED("render_apply");
    } else if (effect == ST_FX_ECHO) {
        hipLaunchKernelGGL(str::render_echo_kernel, tiled, dim3(256), 0, st_stream(stream), p);
        ST_LAUNCHED("render_echo");
    } else if (effect == ST_FX_COMP) {
        hipLaunchKernelGGL(str::render_scan_kernel<ST_FX_COMP>, dim3((unsigned)nfiles), dim3(256), 0, st_stream(stream), p, sr);
        ST_LAUNCHED("render_scan_comp");
    } else {
        hipLaunchKernelGGL(str::render_scan_kernel<ST_FX_LOWPASS>, dim3((unsigned)nfiles), dim3(256), 0, st_stream(stream), p, sr);
        ST_LAUNCHED("render_scan_lowpass");
    }
    return ST_OK;
}

// ------------------------------------------------------------------------------ generic learned-basis front end (a15)
// cls_fe_dct_bases.Analysis / Synthesis: Conv1d(1 -> C, k = KW, stride = hop, padding = pad, bias) and
// ConvTranspose1d(C -> 1, k = KW, stride = hop) + crop, forward and backward, on the same framed GEMM family.
// The one host-side gate of the family: the limit a shape violates, by name, or NULL where the kernels may run it.  Everything in 64-bit host arithmetic.
//  - rows: the loaders index rows and padded signals with 24-bit multiplies (__umul24): B * T and L + 2 pad + 2 KW stay below 2^24;
//  - elements: ldg128 shifts a 32-bit ELEMENT offset left by 2 in 32 bits, so every operand addressed that way stays below 2^30 elements;
//  - the row split: RowMap::split divides a compact row r < B * T by T with a multiply-high by floor(2^32 / T) + 1, exact while r * T < 2^32.  The quotient
//    fails first at r = T - 1 (mod T), so the largest row B * T - 1 decides.  A wrong quotient is a frame index of -1: an address, not a rounding error.
static const char* fe_limit(int B, int L, int C, int KW, int hop, int pad)
{
    if (!(B > 0 && L > 0 && C > 0 && KW > 0 && hop > 0 && pad >= 0)) return "non-positive dimension";
    if (!(KW % 16 == 0 && C % 16 == 0 && hop % 4 == 0 && pad % 4 == 0 && L % 4 == 0)) return "KW%16, C%16, hop%4, pad%4, L%4 required";
    const long long span = (long long)L + 2ll * pad;
    if (KW > span) return "window longer than the padded signal (no frame)";
    const long long T = (span - KW) / hop + 1, R = (long long)B * T, wide = span + 2ll * KW;
    const long long r24 = 1ll << 24, e30 = 1ll << 30;
    if (R >= r24) return "B*T rows leave the 24-bit row index";
    if (wide >= r24) return "L + 2 pad + 2 KW leaves the 24-bit sample index";
    if ((long long)B * L >= e30) return "B*L leaves the 32-bit element offsets (2^30 elements)";
    if ((long long)B * wide >= e30) return "B*(L + 2 pad + 2 KW) leaves the 32-bit element offsets (2^30 elements)";
    if (R * KW >= e30) return "B*T*KW leaves the 32-bit element offsets (2^30 elements)";
    if (R * C >= e30) return "B*T*C leaves the 32-bit element offsets (2^30 elements)";
    if ((long long)C * KW >= e30) return "C*KW leaves the 32-bit element offsets (2^30 elements)";
    if (!fm_div_exact((int)(R - 1), (int)T)) return "row split inexact: (B*T - 1)*T must stay below 2^32";
    return nullptr;
}
extern "C" int st_fe_supported(int B, int L, int C, int KW, int hop, int pad) { return fe_limit(B, L, C, KW, hop, pad) ? 0 : 1; }
static int fe_check(const char* who, int B, int L, int C, int KW, int hop, int pad)
{
    const char* why = fe_limit(B, L, C, KW, hop, pad);
    ST_REQ(!why, "%s: %s (B=%d L=%d C=%d KW=%d hop=%d pad=%d)", who, why, B, L, C, KW, hop, pad);
    return ST_OK;
}
// the synthesis entries take (B, T, C, KW, hop, crop): the same gate at the analysis geometry of the same model, L = the output length and pad = crop
// (st_fe_frames(len, KW, hop, crop) is T again)
static int fe_check_synth(const char* who, int B, int T, int C, int KW, int hop, int crop, int* len)
{
    ST_REQ(B > 0 && T > 0 && C > 0 && KW > 0 && hop > 0 && crop >= 0, "%s: non-positive dimension", who);
    const long long n = ((long long)T - 1) * hop + KW - 2ll * crop;
    ST_REQ(n > 0, "%s: nothing left after the crop", who);
    ST_REQ(n < (1ll << 24), "%s: output length leaves the 24-bit sample index", who);
    *len = (int)n;
    return fe_check(who, B, (int)n, C, KW, hop, crop);      // len % 4 is the gate's L % 4
}
extern "C" int st_fe_frames(int L, int KW, int hop, int pad) { return (L + 2 * pad - KW) / hop + 1; }
extern "C" size_t st_fe_ws_floats(int B, int L, int C, int KW, int hop, int pad)
{
    if (!st_fe_supported(B, L, C, KW, hop, pad)) return 0;
    const int T = st_fe_frames(L, KW, hop, pad);
    const size_t R = (size_t)B * T;
    // frames [R][KW] + padded gradient signal [B][L + 2 KW] + split-K slabs of the weight gradient
    return R * KW + (size_t)B * ((size_t)L + 2 * (size_t)KW + 2 * (size_t)pad) + (size_t)wgrad_split((int)R) * C * KW + 1024;
}
extern "C" int st_fe_analysis_fwd(const float* x, int B, int L, const float* W, const float* bias, int C, int KW, int hop, int pad,
                                  float* out, void* stream)
{
    ST_TRY(fe_check("st_fe_analysis_fwd", B, L, C, KW, hop, pad)); ST_REQ(x && W && out, "st_fe_analysis_fwd: null pointer");
    const int T = st_fe_frames(L, KW, hop, pad), R = B * T;
    stg::FramedNT<false> al{x, L, hop, pad, R, KW, 1.0f, stg::all_frames(T)};
    stg::PlainNT bl{W, C, KW, KW, stg::all_frames(1)};
    stg::BiasStore ep{out, bias, R, C, C};
    stg::launch<2, 16>(al, bl, ep, R, C, KW, 1, st_stream(stream));
    ST_LAUNCHED("fe_analysis_fwd"); return ST_OK;
}
static int fe_frames_ola(const float* xft, int B, int T, const float* W, int C, int KW, int hop, int crop, int len,
                         float* frs, float* out, void* stream)
{
    const int R = B * T;
    stg::PlainNT al{xft, R, C, C, stg::all_frames(1)};
    stg::PlainTN bl{W, C, KW, KW, stg::all_frames(1)};
    stg::StoreC ep{frs, R, KW, KW, 0, stg::all_frames(1)};
    stg::launch<2, 16>(al, bl, ep, R, KW, C, 1, st_stream(stream));
    hipLaunchKernelGGL(stm::ola_crop_kernel, dim3((len + 255) / 256, B), dim3(256), 0, st_stream(stream), frs, out, T, KW, hop, crop, len);
    return ST_OK;
}
extern "C" int st_fe_synthesis_fwd(const float* xft, int B, int T, const float* W, int C, int KW, int hop, int crop,
                                   float* ws, float* out, void* stream)
{
    int len = 0;
    ST_TRY(fe_check_synth("st_fe_synthesis_fwd", B, T, C, KW, hop, crop, &len));
    ST_REQ(xft && W && ws && out, "st_fe_synthesis_fwd: null pointer");
    ST_TRY(fe_frames_ola(xft, B, T, W, C, KW, hop, crop, len, ws, out, stream));
    ST_LAUNCHED("fe_synthesis_fwd"); return ST_OK;
}
// d loss / d (x/2) of the whole model, for callers with something trainable UPSTREAM of st_model (the reference's autograd gives it for
// free; its own training never asks: x is data).  Must follow st_model_bwd on the same workspace: the analysis output gradient dG
// [B*T][KP] is still there.  gxh[b][n] = sum_t sum_k dG[b,t,k] W[k][n - (H t - N)]  (conv-transpose of both Conv1d's, cropped by the
// padding); the caller scales by the 1/2 of nn_proc.py:307 and adds the skip term of :340.  scratch: st_model_input_grad_ws_floats().
__global__ void __launch_bounds__(256)
wcat_kernel(const float* __restrict__ Wr, const float* __restrict__ Wi, float* __restrict__ out, const int F, const int N, const int KP)
{
    const int row = blockIdx.x, half = KP / 2;
    const bool is_im = row >= half; const int k = is_im ? row - half : row;
    for (int n = threadIdx.x; n < N; n += 256) out[(size_t)row * N + n] = k < F ? (is_im ? Wi : Wr)[(size_t)k * N + n] : 0.f;
}
extern "C" size_t st_model_input_grad_ws_floats(const st_dims* d)
{
    if (check_dims(d) != ST_OK) return 0;
    return (size_t)st_kp_of(d->F) * d->N + (size_t)d->B * d->T * d->N + 64;
}
extern "C" int st_model_input_grad(const st_dims* d, const float* params, void* ws, float* scratch, float* gxh, void* stream)
{
    Layout L; ST_TRY(make_layout(d, &L));
    ST_REQ(params && ws && scratch && gxh, "st_model_input_grad: null pointer");
    ST_REQ(d->L % 4 == 0 && d->H % 4 == 0, "st_model_input_grad: L %% 4 and hop %% 4 required");
    WS w; carve(d, L, ws, &w);
    float* Wc = scratch; float* frs = scratch + (size_t)L.KP * d->N;
    hipLaunchKernelGGL(wcat_kernel, dim3(L.KP), dim3(256), 0, st_stream(stream), params + L.offs[0], params + L.offs[1], Wc, d->F, d->N, L.KP);
    ST_TRY(fe_frames_ola(w.dG, d->B, d->T, Wc, L.KP, d->N, d->H, d->N, d->L, frs, gxh, stream));
    ST_LAUNCHED("model_input_grad");
    return ST_OK;
}
// autograd of st_fe_analysis_fwd: gW [C][KW], gbias [C] (may be null), gx [B][L] (may be null)
extern "C" int st_fe_analysis_bwd(const float* x, int B, int L, const float* W, int C, int KW, int hop, int pad, const float* g_out,
                                  float* ws, float* gW, float* gbias, float* gx, void* stream)
{
    ST_TRY(fe_check("st_fe_analysis_bwd", B, L, C, KW, hop, pad)); ST_REQ(x && W && g_out && ws && gW, "st_fe_analysis_bwd: null pointer");
    const int T = st_fe_frames(L, KW, hop, pad), R = B * T;
    const int ns = wgrad_split(R);
    float* slabs = ws;                                       // [ns][C][KW]
    float* frs = ws + (size_t)ns * C * KW;                   // [R][KW]
    {
        stg::PlainTN al{g_out, R, C, C, stg::all_frames(1)};
        stg::FramedTN<false> bl{x, L, hop, pad, R, KW, 1.0f, stg::all_frames(T)};
        stg::StoreC ep{slabs, C, KW, KW, (size_t)C * KW, stg::all_frames(1)};
        stg::launch<3, 16>(al, bl, ep, C, KW, R, ns, st_stream(stream));
        const size_t n = (size_t)C * KW;
        hipLaunchKernelGGL(stm::sum_slabs_flat_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st_stream(stream), slabs, ns, n, gW);
    }
    if (gbias) hipLaunchKernelGGL(stm::col_sum_kernel, dim3((C + 255) / 256), dim3(256), 0, st_stream(stream), g_out, R, C, gbias);
    if (gx) ST_TRY(fe_frames_ola(g_out, B, T, W, C, KW, hop, pad, L, frs, gx, stream));   // conv-transpose of the output gradient, cropped by the padding
    ST_LAUNCHED("fe_analysis_bwd"); return ST_OK;
}
// autograd of st_fe_synthesis_fwd: gW [C][KW], g_xft [B][T][C] (may be null)
extern "C" int st_fe_synthesis_bwd(const float* xft, int B, int T, const float* W, int C, int KW, int hop, int crop, const float* g_wave,
                                   float* ws, float* gW, float* g_xft, void* stream)
{
    int len = 0;
    ST_TRY(fe_check_synth("st_fe_synthesis_bwd", B, T, C, KW, hop, crop, &len));
    ST_REQ(xft && W && g_wave && ws && gW, "st_fe_synthesis_bwd: null pointer");
    const int R = B * T;
    const int ns = wgrad_split(R);
    float* slabs = ws;                                       // [ns][C][KW]
    float* gp = ws + (size_t)ns * C * KW;                    // padded gradient signal [B][crop + len + crop]: its frames are d(frames)
    ST_TRY(pad_scale(g_wave, gp, B, len, crop, 1.0f, stream));
    if (g_xft) {
        stg::FramedNT<true> al{gp, len, hop, crop, R, KW, 1.0f, stg::all_frames(T)};
        stg::PlainNT bl{W, C, KW, KW, stg::all_frames(1)};
        stg::StoreC ep{g_xft, R, C, C, 0, stg::all_frames(1)};
        stg::launch<2, 16>(al, bl, ep, R, C, KW, 1, st_stream(stream));
    }
    {
        stg::PlainTN al{xft, R, C, C, stg::all_frames(1)};
        stg::FramedTN<true> bl{gp, len, hop, crop, R, KW, 1.0f, stg::all_frames(T)};
        stg::StoreC ep{slabs, C, KW, KW, (size_t)C * KW, stg::all_frames(1)};
        stg::launch<3, 16>(al, bl, ep, C, KW, R, ns, st_stream(stream));
        const size_t n = (size_t)C * KW;
        hipLaunchKernelGGL(stm::sum_slabs_flat_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st_stream(stream), slabs, ns, n, gW);
    }
    ST_LAUNCHED("fe_synthesis_bwd"); return ST_OK;
}

// ------------------------------------------------------------------------------ data parallel (st_dp.h): RCCL inside the library
extern "C" int st_dp_unique_id(void* id128)
{
    ST_REQ(id128, "st_dp_unique_id: null buffer");
    st_dp tmp; memset(&tmp, 0, sizeof(tmp));
    ST_TRY(stdp::bind(&tmp));
    ncclUniqueId id;
    ST_NCCL(&tmp, tmp.GetUniqueId(&id), "ncclGetUniqueId");
    static_assert(sizeof(id) == 128, "RCCL unique id is 128 bytes");
    memcpy(id128, &id, sizeof(id));
    return ST_OK;
}

extern "C" int st_dp_init(const void* id128, int rank, int world, st_dp** out)
{
    ST_REQ(id128 && out && world >= 1 && rank >= 0 && rank < world, "st_dp_init: bad arguments (rank %d of %d)", rank, world);
    st_dp* p = new st_dp; memset(p, 0, sizeof(*p));
    int rc = stdp::bind(p);
    if (rc != ST_OK) { delete p; return rc; }
    ncclUniqueId id; memcpy(&id, id128, sizeof(id));
    p->rank = rank; p->world = world;
    const ncclResult_t r = p->CommInitRank(&p->comm, world, id, rank);       // collective over all ranks: every rank must call this
    if (r != ncclSuccess) { rc = st_fail(ST_ERR_LAUNCH, "st_dp ncclCommInitRank(rank %d of %d): %s", rank, world, p->GetErrorString(r)); delete p; return rc; }
    hipError_t e = hipStreamCreateWithFlags(&p->cs, hipStreamNonBlocking);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&p->ready[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->wgfree, hipEventDisableTiming);
    if (e != hipSuccess) { rc = st_fail(ST_ERR_LAUNCH, "st_dp_init: stream/event creation: %s", hipGetErrorString(e)); (void)p->CommDestroy(p->comm); delete p; return rc; }
    *out = p;
    return ST_OK;
}

extern "C" int st_dp_destroy(st_dp* p)
{
    if (!p) return ST_OK;
    (void)hipStreamSynchronize(p->cs);
    if (p->comm) (void)p->CommDestroy(p->comm);
    for (int i = 0; i < 4; ++i) if (p->ready[i]) (void)hipEventDestroy(p->ready[i]);
    if (p->done) (void)hipEventDestroy(p->done);
    if (p->wgfree) (void)hipEventDestroy(p->wgfree);
    if (p->cs) (void)hipStreamDestroy(p->cs);
    delete p;
    return ST_OK;
}
extern "C" int st_dp_rank(const st_dp* p) { return p ? p->rank : -1; }
extern "C" int st_dp_world(const st_dp* p) { return p ? p->world : -1; }
// ncclGetVersion of the library the communicator is bound to (e.g. 22606), 0 if it does not export one: bench.py prints it beside the world size every
// rank reports, so that a multi-GPU line carries its own evidence of what the ranks met on
extern "C" int st_dp_rccl_version(const st_dp* p) { int v = 0; if (p && p->GetVersion && p->GetVersion(&v) == ncclSuccess) return v; return 0; }

// buf (n floats, in place, SUM) is all-reduced on the communicator stream once everything issued so far on `stream` has
// finished; returns at once.  st_dp_sync makes `stream` wait for all collectives issued since the last sync.
extern "C" int st_dp_allreduce(st_dp* p, float* buf, int64_t n, void* stream)
{
    ST_REQ(p && buf && n > 0, "st_dp_allreduce: bad arguments");
    hipEvent_t ev = p->ready[p->n_issued & 3]; p->n_issued++;
    ST_HIP(hipEventRecord(ev, st_stream(stream)), "event record");
    ST_HIP(hipStreamWaitEvent(p->cs, ev, 0), "stream wait");
    ST_NCCL(p, p->AllReduce(buf, buf, (size_t)n, ncclFloat32, ncclSum, p->comm, p->cs), "ncclAllReduce");
    return ST_OK;
}
// ... of `n` elements of `dt` on the communicator stream WITHOUT a new compute -> comm dependency (the caller has ordered the stream already)
static int dp_allreduce_on_cs(st_dp* p, void* buf, int64_t n, ncclDataType_t dt)
{
    ST_NCCL(p, p->AllReduce(buf, buf, (size_t)n, dt, ncclSum, p->comm, p->cs), "ncclAllReduce");
    return ST_OK;
}
// compute -> comm: everything issued so far on `stream` precedes what is issued on the communicator stream from here on
static int dp_fork(st_dp* p, void* stream)
{
    hipEvent_t ev = p->ready[p->n_issued & 3]; p->n_issued++;
    ST_HIP(hipEventRecord(ev, st_stream(stream)), "event record");
    ST_HIP(hipStreamWaitEvent(p->cs, ev, 0), "stream wait");
    return ST_OK;
}
extern "C" int st_dp_broadcast(st_dp* p, float* buf, int64_t n, int root, void* stream)
{
    ST_REQ(p && buf && n > 0 && root >= 0 && root < p->world, "st_dp_broadcast: bad arguments");
    hipEvent_t ev = p->ready[p->n_issued & 3]; p->n_issued++;
    ST_HIP(hipEventRecord(ev, st_stream(stream)), "event record");
    ST_HIP(hipStreamWaitEvent(p->cs, ev, 0), "stream wait");
    ST_NCCL(p, p->Broadcast(buf, buf, (size_t)n, ncclFloat32, root, p->comm, p->cs), "ncclBroadcast");
    return ST_OK;
}
extern "C" int st_dp_sync(st_dp* p, void* stream)
{
    ST_REQ(p, "st_dp_sync: null communicator");
    ST_HIP(hipEventRecord(p->done, p->cs), "event record");
    ST_HIP(hipStreamWaitEvent(st_stream(stream), p->done, 0), "stream wait");
    return ST_OK;
}

// One data-parallel optimisation step (train.py:112-151 on this rank's shard + the exchange of SURVEY.md 8e), all from C:
//   phase 1 (forward ... autoencoder / polar backward)            -> all-reduce grads[offs[2], total)  (8.45 MB)  || phase 2
//   phase 2 (analysis weight gradient, live rows packed in stage) -> all-reduce stage [2F][N]          (4.2 MB, exposed)
//   copy the reduced rows back, L1 norm of the reduced gradient, clip, Adam with grad_scale = 1/world.
// `stage`: caller-owned 2*F*N floats.  p == NULL or world == 1 falls through to st_train_step (no exchange).
extern "C" int st_dp_train_step(st_dp* p, const st_dims* d, float* params, float* grads, float* m, float* v, float* stage,
                                const float* x, const float* knobs, const float* y_true, void* ws, float* scalars,
                                float lr, float beta1, float beta2, float eps, int step, int force_exchange, void* stream)
{
    if (!p || (p->world == 1 && !(force_exchange & 1)))
        return st_train_step(d, params, grads, m, v, x, knobs, y_true, ws, scalars, lr, beta1, beta2, eps, step, stream);
    Call c; ST_TRY(call_begin(&c, d, params, knobs, ws, stream, G16_PIPELINE));
    const Layout& L = c.L; WS& w = c.w;
    ST_REQ(stage, "st_dp_train_step: null staging buffer");
    ST_REQ(params && grads && x && (knobs || d->K == 0) && y_true && ws, "st_dp_train_step: null pointer");
    const float gs = (1.0f / (float)p->world) / loss_scale_of(d);          // 1/world and the loss scale leave the gradient together
    // force_exchange is a bit set: 1 = run the exchange even with one rank; 2 = split the LAST exchange by basis (real rows under the GEMM of the imaginary
    // ones: 2.1 MB exposed instead of 4.2); 4 = that exchange on bfloat16 values (only where the autoencoder layers already run in 16 bits: *_ALL)
    const bool split_last = (force_exchange & 2) != 0;
    const int pack16 = ((force_exchange & 4) != 0 && ae_ht(d->prec) != 0) ? 1 : 0;
    // Exchanges, each issued the moment its gradients are final (the communicator stream orders them):
    //   synthesis bases (8.4 MB)  -- after their weight-gradient GEMM, BEFORE the autoencoder backward: hidden behind the longest
    //                                kernels of the step (autoencoder backward + polar backward + analysis weight gradient); the sum of
    //                                the GEMM's split-K slabs itself runs ON the communicator stream, beside the autoencoder backward
    //                                (round 3 ran it in line: a 9 us launch on the critical path that the single-GPU step folds into post_ae_kernel);
    //   autoencoders (67 KB)      -- after the autoencoder backward;
    //   analysis bases            -- the 2F live rows, packed (4.2 MB), after the last GEMM of the step: the exposed one (split / packed: see the flags).
    {
        prof_mark("begin", stream);
        ST_TRY(forward_impl(c, params, x, y_true, nullptr, nullptr, nullptr, true));
        const WgradPlan sp = step_wgrad_plan(d, w, 1, -1, g_dp_inline ? w.wg2 : w.wg);  // round 6: the synthesis slabs in their own area (no wait before the analysis GEMM reuses the first)
        ST_TRY(backward_syn(c, grads, &sp));                                            // GEMMs only; the slabs are summed on the communicator stream
        ST_TRY(dp_fork(p, stream));
        wgrad_reduce(sp, grads + L.offs[2], grads + L.offs[3], w.norm_s, nullptr, 0, p->cs);
        if (!g_dp_inline) ST_HIP(hipEventRecord(p->wgfree, p->cs), "event record");     // the analysis weight-gradient GEMM reuses the slab buffer
        ST_TRY(dp_allreduce_on_cs(p, grads + L.offs[2], L.offs[4] - L.offs[2], ncclFloat32));
        // The clip norm is that of the REDUCED, 1/world-scaled gradient.  The two ranges whose exchange is hidden get their |g| partials on the communicator
        // stream right behind their collective (hidden as well); only the analysis rows' share is formed after the exposed collective, in the pass that
        // copies them back (unstage_l1_kernel).  Same kernels, same order, same data on every rank: the norm is bit-identical across ranks.
        hipLaunchKernelGGL(stm::l1_partial_kernel, dim3(norm_partials(d)), dim3(256), 0, p->cs, grads + L.offs[2], L.offs[4] - L.offs[2], gs, w.norm_s);
        ST_TRY(backward_ae(c, params, grads, nullptr, nullptr, reg_coef_of(d)));
        ST_TRY(st_dp_allreduce(p, grads + L.offs[4], L.total - L.offs[4], stream));
        if (d->clip_all) hipLaunchKernelGGL(stm::l1_partial_kernel, dim3(NORM_E_PARTIALS), dim3(256), 0, p->cs, grads + L.n_stft, L.total - L.n_stft, gs, w.norm_e);
        if (!g_dp_inline) ST_HIP(hipStreamWaitEvent(st_stream(stream), p->wgfree, 0), "stream wait");
    }
    const int64_t half_n = (int64_t)d->F * d->N;
    bool last_in_line = false;
    if (!split_last && g_dp_inline) {
        // Round 6: the LAST exchange is exposed whatever stream it runs on (nothing is left to run beside it), so it is issued IN LINE on the compute stream:
        // the two cross-stream hand-offs around it (compute -> communicator before, communicator -> compute after: ~10 us each on this stack, measured with one
        // rank as a 21 us hole in front of the optimizer kernel) become ONE join that is recorded HERE, behind the last hidden collective, and has fired long
        // before the GEMM below ends.  RCCL serialises the collectives of one communicator in issue order across streams; every rank issues the same order.
        ST_HIP(hipEventRecord(p->done, p->cs), "event record");
        ST_TRY(backward_p2(c, grads, stage, pack16));
        ST_HIP(hipStreamWaitEvent(st_stream(stream), p->done, 0), "stream wait");
        ST_NCCL(p, p->AllReduce(stage, stage, (size_t)(2 * half_n), pack16 ? ncclBfloat16 : ncclFloat32, ncclSum, p->comm, st_stream(stream)), "ncclAllReduce");
        last_in_line = true;
    } else if (!split_last) {
        ST_TRY(backward_p2(c, grads, stage, pack16));
        ST_TRY(dp_fork(p, stream));
        ST_TRY(dp_allreduce_on_cs(p, stage, 2 * half_n, pack16 ? ncclBfloat16 : ncclFloat32));
    } else {
        for (int h = 0; h < 2; ++h) {
            ST_TRY(backward_p2(c, grads, stage, pack16, h));
            void* part = pack16 ? (void*)(reinterpret_cast<unsigned short*>(stage) + (size_t)h * half_n) : (void*)(stage + (size_t)h * half_n);
            if (h == 1 && g_dp_inline) {        // the second half's exchange is the exposed one: in line, behind the join recorded when the first half's was issued
                ST_HIP(hipStreamWaitEvent(st_stream(stream), p->done, 0), "stream wait");
                ST_NCCL(p, p->AllReduce(part, part, (size_t)half_n, pack16 ? ncclBfloat16 : ncclFloat32, ncclSum, p->comm, st_stream(stream)), "ncclAllReduce");
                last_in_line = true;
                break;
            }
            ST_TRY(dp_fork(p, stream));
            ST_TRY(dp_allreduce_on_cs(p, part, half_n, pack16 ? ncclBfloat16 : ncclFloat32));
            if (g_dp_inline) ST_HIP(hipEventRecord(p->done, p->cs), "event record");
        }
    }
    if (!last_in_line) ST_TRY(st_dp_sync(p, stream));
    {
        const int np = norm_partials(d);
        hipLaunchKernelGGL(stm::unstage_l1_kernel, dim3(2 * d->F), dim3(256), 0, st_stream(stream), stage, grads + L.offs[0], grads + L.offs[1], d->F, d->N, gs, w.norm_a, np, pack16);
        ST_LAUNCHED("unstage_l1");
        stm::FinArgs f = fin_args(d, w.loss_p, w.reg_p, w.norm_a, w.norm_s, 1.0f);
        if (d->clip_all) { f.norm_e = w.norm_e; f.n_ne = NORM_E_PARTIALS; }
        return clip_adam_impl(params, grads, m, v, L.total, d->clip_all ? L.total : L.n_stft, scalars, gs, lr, beta1, beta2, eps, step, &f, stream);
    }
}


// ------------------------------------------------------------------------------ the whole step as one HIP graph
// st_train_step captured once and replayed: 11 kernel nodes + the step-tick head.  What changes from iteration to iteration --
// the step number (Adam's bias corrections) and the learning rate (1-cycle table, train.py:108,150) -- lives on the device
// (scalars[6], scalars[7]; the table is a caller-owned device array), so the graph needs no per-step update; the minibatch is read
// from the fixed device buffers x / knobs / y_true the graph was captured with (the caller refills them, e.g. by an index gather
// from a device-resident dataset).  On this path the launch work of a step is one hipGraphLaunch; the GPU-side cost of the
// kernel boundaries themselves is the same as for eager launches (MI355X_MICROARCH.md "boundary": eager == hipGraph).
struct st_graph { hipGraph_t graph; hipGraphExec_t exec; };

static int attr_prepare(const st_dims* d)
{
    // hipFuncSetAttribute is not a capturable call: make sure every >64 KB-LDS kernel this geometry / precision uses has its
    // attribute before the capture starts (ensure_dyn_lds is then a table hit inside the captured calls)
    auto prep = [](auto* kernel, const char* name) { return ensure_dyn_lds(reinterpret_cast<const void*>(kernel), name); };
    const int ht = ae_ht(d->prec);
    if (ae_is_wide(d))
        ST_TRY(with_ht(ht, [&](auto HT) -> int {
            ST_TRY(prep(sta::ae_inner_fwd_kernel<AE_FWD_NW, HT()>, "ae_inner_fwd_kernel")); ST_TRY(prep(sta::ae_inner_fwd_kernel<9, HT()>, "ae_inner_fwd_kernel"));
            ST_TRY(prep(sta::ae_inner_fwd_kernel<12, HT()>, "ae_inner_fwd_kernel"));
            ST_TRY(prep(sta::ae_bwd_kernel<AE_BWD_NW, true, HT(), 0>, "ae_bwd_kernel"));
            return prep(stw::wide_dv_polar_kernel<HT()>, "wide_dv_polar_kernel"); }));
    else {
        ST_TRY(with_ht(ht, [&](auto HT) -> int {
            ST_TRY(prep(sta::ae_fwd_kernel<AE_FWD_NW, HT()>, "ae_fwd_kernel"));
            ST_TRY(prep(sta::ae_bwd_part_kernel<AE_SPLIT_NW, 1, HT(), false>, "ae_bwd_part_kernel")); ST_TRY(prep(sta::ae_bwd_part_kernel<AE_SPLIT_NW, 2, HT(), false>, "ae_bwd_part_kernel"));
            return d->T - d->OT == 16 ? prep(sta::ae_bwd_kernel<AE_BWD_NW, false, HT(), 2>, "ae_bwd_kernel") : prep(sta::ae_bwd_kernel<AE_BWD_NW, false, HT(), 0>, "ae_bwd_kernel"); }));
        if (ht != 0) ST_TRY(with_ht16(ht, [&](auto HT) { return prep(sta::ae_fwd32_kernel<AE_FWD_NW, HT()>, "ae_fwd32_kernel"); }));
        else {      // fp32 layers: the 11-wave forward, the kept-activation forms of both, with and without the ready-made images
            ST_TRY(prep(sta::ae_fwd_kernel<11, 0>, "ae_fwd_kernel")); ST_TRY(prep(sta::ae_fwd_kernel<11, 0, true>, "ae_fwd_kernel")); ST_TRY(prep(sta::ae_fwd_kernel<AE_FWD_NW, 0, true>, "ae_fwd_kernel"));
            for (int var = 0; var < 3; ++var)
                ST_TRY(with_var(var, [&](auto VAR) -> int {
                    ST_TRY(prep(sta::ae_bwd_kernel<AE_BWD_NW, false, 0, VAR(), true>, "ae_bwd_kernel"));
                    return prep(sta::ae_bwd_kernel<AE_BWD_NW, false, 0, VAR(), true, false, true>, "ae_bwd_kernel"); }));
        }
    }
    if (g_nt128 && gemm_ht(d->prec) == 0) ST_TRY(prep(stg::gemm_nt128_kernel, "gemm_nt128_kernel"));
    if (use_g16(d))             // st_gemm16.h: 72 / 80 KB of LDS with 64-deep k-tiles
        ST_TRY(with_ht16(gemm_ht(d->prec), [&](auto HT) -> int {
            ST_TRY(prep(stg::gemm16_nt256_kernel<HT(), stg::PolarStore>, "gemm16_nt256_kernel")); ST_TRY(prep(stg::gemm16_nt256_kernel<HT(), stg::StoreC>, "gemm16_nt256_kernel"));
            ST_TRY(prep(stg::gemm16_nt_kernel<HT(), 64, stg::PolarStore>, "gemm16_nt_kernel")); ST_TRY(prep(stg::gemm16_nt_kernel<HT(), 64, stg::StoreC>, "gemm16_nt_kernel"));
            return prep(stg::gemm16_tn_kernel<HT(), 64>, "gemm16_tn_kernel"); }));
    if (use_planes(d)) {        // the 4-wave plane GEMM carries 67 KB of LDS (st_gemm_planes.h)
        ST_TRY(prep(stg::gemm_planes_kernel<4, 3, stg::FramedNT<true>, stg::ChunkP, stg::PolarStore>, "gemm_planes_kernel"));
        ST_TRY(prep(stg::gemm_planes_kernel<8, 3, stg::FramedNT<true>, stg::ChunkP, stg::PolarStore>, "gemm_planes_kernel"));
        ST_TRY(prep(stg::gemm_planes_kernel<4, 3, stg::PlainNT, stg::ChunkP, stg::StoreC>, "gemm_planes_kernel"));
        ST_TRY(prep(stg::gemm_planes_kernel<4, 3, stg::FramedNT<true>, stg::ChunkP, stg::StoreC>, "gemm_planes_kernel"));
    }
    (void)num_cus();
    return ST_OK;
}

extern "C" int st_graph_create(const st_dims* d, float* params, float* grads, float* m, float* v, const float* x,
                               const float* knobs, const float* y_true, void* ws, float* scalars,
                               const float* lr_table, int n_lr, float beta1, float beta2, float eps, void* stream, st_graph** out)
{
    ST_TRY(check_dims(d));
    ST_REQ(params && grads && m && v && x && (knobs || d->K == 0) && y_true && ws && scalars && lr_table && n_lr > 0 && out, "st_graph_create: bad arguments");
    ST_REQ(!g_prof, "st_graph_create: switch the event profiling off first (event records would be captured)");
    ST_TRY(attr_prepare(d));
    hipStream_t s = st_stream(stream);
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) return st_fail(ST_ERR_LAUNCH, "st_graph_create: hipStreamBeginCapture failed (is `stream` the legacy default stream?)");
    hipLaunchKernelGGL(stm::step_tick_kernel, dim3(1), dim3(64), 0, s, scalars, lr_table, n_lr);
    int rc = train_step_impl(d, params, grads, m, v, x, knobs, y_true, ws, scalars, 0.f, beta1, beta2, eps, 1, stream, true);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(s, &g);
    if (rc != ST_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess || !g) return st_fail(ST_ERR_LAUNCH, "st_graph_create: capture failed: %s", hipGetErrorString(e));
    hipGraphExec_t ex = nullptr;
    if (hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess) { (void)hipGraphDestroy(g); return st_fail(ST_ERR_LAUNCH, "st_graph_create: hipGraphInstantiate failed"); }
    st_graph* p = new st_graph{g, ex};
    *out = p;
    return ST_OK;
}
extern "C" int st_graph_launch(st_graph* g, void* stream)
{
    ST_REQ(g && g->exec, "st_graph_launch: null graph");
    const hipError_t e = hipGraphLaunch(g->exec, st_stream(stream));
    if (e != hipSuccess) return st_fail(ST_ERR_LAUNCH, "hipGraphLaunch: %s", hipGetErrorString(e));
    return ST_OK;
}
extern "C" int st_graph_destroy(st_graph* g)
{
    if (!g) return ST_OK;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
    return ST_OK;
}
