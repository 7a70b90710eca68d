/* signaltrain_hip.h -- C ABI of libsignaltrain_hip.so (MI355X / gfx950).
 *
 * The reference (drscotthawley/signaltrain) has no FFI / operator registry: its hot path is
 * plain PyTorch modules.  This header is therefore the boundary a maintainer
 * would bind (ctypes stub in INTEGRATION.md); every entry point names the reference code it
 * replaces.  Conventions:
 *   - all pointers are DEVICE pointers to contiguous fp32 unless stated; the caller (PyTorch)
 *     owns every buffer, including workspaces and saved activations;
 *   - every compute entry is asynchronous on `stream` (a hipStream_t passed as void*), does
 *     no allocation and no host synchronisation;
 *   - return value: 0 = ok, <0 = error; message via st_last_error();
 *   - shapes use the reference's names: B windows, L samples/window, N=ft_size, H=hop,
 *     T input frames, OT output frames, F=N/2+1 bins, K knobs, y output samples.
 */
#ifndef SIGNALTRAIN_HIP_H
#define SIGNALTRAIN_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ST_OK 0
#define ST_ERR_ARG (-1)      /* bad dimension / null pointer / misalignment */
#define ST_ERR_LAUNCH (-2)   /* HIP launch error */
#define ST_ERR_UNSUPPORTED (-3)

/* Arithmetic of a call (st_dims.prec).  Carried per call: two engines of different precision can share a process.
 *   ST_PREC_F32       fp32 MFMA everywhere -- the parity path (<= 1e-4 of the fp32 reference).
 *   ST_PREC_BF16      bf16 operands, fp32 accumulation in the analysis / synthesis GEMMs and their data / weight gradients
 *                     (BASELINE.json configs[2], [3]); operands are rounded (RNE) as they are staged, parameters,
 *                     activations, gradients, autoencoders, loss and Adam stay fp32.
 *   ST_PREC_BF16_ALL  additionally the nine Linear layers of both autoencoders (nn_proc.py:84-117 and their autograd):
 *                     weights and layer inputs / incoming gradients rounded to bf16, fp32 accumulation; bias, ELU, ELU',
 *                     skip / residual epilogue fp32.
 *   ST_PREC_F16, ST_PREC_F16_ALL   the same two levels with IEEE float16 operands (BASELINE.json configs[4], the
 *                     reference's Apex amp path, train.py:254-255), meant to run with st_dims.loss_scale > 1
 *                     (train.py:134-135 amp.scale_loss).  Conversion is IEEE: an out-of-range operand becomes inf, the
 *                     gradient norm turns non-finite and st_train_step / st_dp_clip_adam SKIP the update and count it in
 *                     scalars[5] (Apex's overflow handling; the host lowers the scale).  The polar backward (fp32, 1e7-sized
 *                     sub-gradients on silent frames) saturates its output to the fp16 range; loss and Adam fp32.
 *   ST_PREC_F32X3     fp32 results from the bf16 MATRIX pipe: every operand of the analysis / synthesis GEMMs (forward, data and
 *                     weight gradients) is split as it is staged into three bfloat16 planes x = x1 + x2 + x3 (24 significand bits,
 *                     both remainders exact) and each product is the sum of the six partial products of order >= 2^-16, accumulated
 *                     in fp32.  Accuracy is that of an fp32 GEMM (measured against float64: not worse than ST_PREC_F32); it is a
 *                     different ROUNDING of the same arithmetic, so it is held to the fp32 reference with the fp32 tolerance.  On
 *                     gfx950 the fp32 MFMA runs at the vector-ALU rate and does not overlap vector work; six bf16 MFMAs cost 3/8 of
 *                     its cycles and run beside the VALU.  Autoencoders, polar maps, loss and Adam are as in ST_PREC_F32.
 * Each 16-bit level equals the reference computed with those operands rounded the same way (the oracle has the same switches),
 * not the fp32 reference. */
#define ST_PREC_F32 0
#define ST_PREC_BF16 1
#define ST_PREC_BF16_ALL 2
#define ST_PREC_F16 3
#define ST_PREC_F16_ALL 4
#define ST_PREC_F32X3 5

/* Geometry (nn_proc.py:357-385) and arithmetic of one call.
 * The supported family is wider than what st_geometry produces (N = 1024, H = 384 and the legacy multiples); every entry refuses anything outside it
 * with ST_ERR_ARG and a message in st_last_error() that names the rule, before any launch, and every size or count function below that takes an st_dims
 * then returns 0 (st_param_offsets and st_workspace_offsets: -1):
 *   - B, L, N, H, T, OT > 0, 0 <= K <= 16, F == N/2 + 1;
 *   - N % 32 == 0, H % 4 == 0, L % 4 == 0, y % 4 == 0 (H > N, H == N and L < N are inside the family);
 *   - y == (OT - 1) * H - N, 0 < y <= L, OT <= T;
 *   - H * T >= L + N: frame t starts at sample H t - N, so T frames must reach the end of the signal.  The reference's Conv1d yields (L + N) / H + 1 frames
 *     and its first Linear layer accepts no other count; here a larger T only adds all-padding frames (st_geometry's ceil(L/H) + ceil(N/H) does that for some
 *     L) and the one frame that starts exactly at L may be left out, but a T that drops a frame overlapping the signal is refused;
 *   - B * T < 2^24, B * T * KP < 2^30, B * (L + 2 N) < 2^30 (32-bit element offsets) and (B * T - 1) * T < 2^32 (the row split by a multiply-high).
 * Sizes away from 1024 / 384 run the general kernels (no 128-row tiles below N % 256 == 0, no 16-bit operand pipeline below N % 128 == 0): correct, not tuned. */
typedef struct st_dims {
    int B;   /* windows in this (per-GPU) minibatch                         */
    int L;   /* samples per input window  (8192*scale)                      */
    int N;   /* ft_size (1024)                                              */
    int H;   /* hop (384)                                                   */
    int T;   /* input STFT frames  = ceil(L/H)+ceil(N/H)                    */
    int OT;  /* output STFT frames = ceil(out/H)+ceil(N/H)                  */
    int F;   /* N/2+1                                                       */
    int K;   /* knobs                                                       */
    int y;   /* output samples = (OT-1)*H - N                               */
    int prec;          /* ST_PREC_* (0 = fp32)                                                                   */
    float loss_scale;  /* static loss scale S of the mixed-precision step (0 or 1: none).  The fused entry points
                          multiply d loss by S before the backward and divide the gradients by S in the optimizer
                          (train.py:134-135); the per-op backward entries are linear and simply pass S through.   */
    int clip_all;      /* 0: L1 clip over the 4 STFT tensors only (nn_proc.py:299-302, the default path);
                          1: over ALL parameters (train.py:136, what the reference does when Apex amp is on)      */
} st_dims;

/* Internal padded spectral pitch: re bins at [0,F), im bins at [KP/2, KP/2+F). */
int st_kp(int F);

const char* st_last_error(void);
int st_version(void);

/* Diagnostic switches (process-wide; NEVER set by the product path): st_set_tuning(code) selects a kernel variant that the test-suite keeps as
 * an A/B reference or an agreement case.  ONE table in st_api.hip (k_tuning_codes) is the whole interface: it lists every accepted code with the
 * switch it sets and the value it stores; any other code returns ST_ERR_ARG, names the code in st_last_error() and changes nothing.  The 20
 * switches are one readable state: st_get_tuning / st_tuning_defaults fill out[0..n) in a fixed order and return the number of switches (out
 * may be NULL), st_reset_tuning restores the shipped defaults; the test-suite asserts the state is at the defaults after every test.
 * Timing-only ablations (results invalid) are not switches: they exist only as -D constants that the Makefile never sets. */
int st_set_tuning(int code);
int st_get_tuning(int* out, int n);
int st_tuning_defaults(int* out, int n);
int st_reset_tuning(void);
/* The arithmetic a call with these dims ACTUALLY runs (an ST_PREC_* code).  Since round 5 that is d->prec for every geometry and batch (until round 4 the
 * wide autoencoder path -- T > 32 or OT > 16, e.g. the 65536-sample window -- ran fp32 Linear layers for odd batches; its weight-gradient GEMMs now take
 * 16-deep k-tiles when B * 528 is 16 mod 32).  Kept so that callers assert the arithmetic instead of assuming it (StepEngine.effective_dtype). */
int st_effective_prec(const st_dims* d);
/* The library has no run-time ablations (build one with EXTRA=-DST_GEMM_ABLATE=<bits>, -DST_AE_ABLATE=..., -DST_PL_ABLATE=..., -DST_G128_ABLATE=...):
 * accepts 0, anything else is ST_ERR_ARG.  Kept for callers that pass an ablation argument through. */
int st_set_debug(int v);

/* Optional per-kernel HIP-event profiling of the fused entry points (off by default; used by
 * bench.py's roofline leg outside the timed region).  st_profile_report fills buf with
 * "kernel_name total_ms launches\n" lines; synchronise the stream first. */
int st_profile_enable(int on);
int st_profile_report(char* buf, int buflen);

/* nn_proc.py:357-385 (st_model.__init__ geometry); lean scheme when legacy==0. Host only. */
int st_geometry(double scale_factor, double shrink_factor, int legacy, int K, int B, st_dims* out);

/* Flat parameter buffer layout: the 40 state_dict tensors in registration order,
 * each start aligned to 4 floats.  st_param_offsets fills offs[40] (in floats) and returns the
 * total length in floats (or <0). */
int64_t st_param_offsets(const st_dims* d, int64_t* offs /*[40]*/);

/* Workspace sizes in bytes for st_model_fwd / st_train_step (pure functions of dims).
 * Contract on its contents: the library never reads a workspace element that the same step has not written -- but it does not write every element.
 * Regions the trimmed kernels skip stay as the caller left them: the padding columns [F, FP) of both halves of every dAA slab (the data gradient
 * covers the F spectral columns only; the autoencoder backward masks f >= F) and the 128-tap tile columns of frs that hold only cropped taps
 * (st_ola_loss reads live taps only).  Zero-fill the buffer once after allocating it (signaltrain_amd.engine does: torch.zeros) if anything
 * other than the library -- a debug dump, a new consumer -- is going to look at those regions; stale bytes there may read as NaN. */
size_t st_workspace_bytes(const st_dims* d);
/* st_workspace_bytes answers for EXACTLY the dims it is given, and it is monotonic neither in the batch (the split-K slab counts of the weight-gradient /
 * synthesis GEMMs are picked per batch: 585 windows of 8192 samples need 85.6 MB more than 586) nor in the arithmetic level (fp32 autoencoder layers keep
 * their activations for the backward).  A host that allocates ONE workspace and then runs other batches or levels in it -- a last partial batch, an inference
 * remainder, a change of st_dims.prec on a live model -- sizes it with this: the maximum over every batch 1 .. d->B, every ST_PREC_* level and both clip
 * scopes (host arithmetic only; ~20 ms for 1024 windows).  0 for bad dims. */
size_t st_workspace_bytes_max(const st_dims* d);
/* The knobs pointer of every entry below: [B][K] fp32; with K == 0 (a model without knobs: nn_proc.py:92-93 concatenates an empty tensor) it may be NULL. */

/* ---------------------------------------------------------------- per-op entry points --- */
/* cls_fe_dft.py:50-58 Analysis.forward fused with nn_proc.py:309-310 (mag, phs).
 * x[B,L]; Wr,Wi[N,N] (rows >= F unused); in_scale multiplies x (0.5, nn_proc.py:307).
 * Outputs [B,T,F] each; any of re/im/mag/phs may be NULL. */
int st_analysis_fwd(const st_dims* d, const float* x, const float* Wr, const float* Wi, float in_scale,
                    float* re, float* im, float* mag, float* phs, void* stream);

/* nn_proc.py:77-126 AsymAutoEncoder.forward for both nets + nn_proc.py:322-326 polar->rect.
 * ae_m / ae_p: the 18 tensors of one autoencoder, packed contiguously in state_dict order with
 * the 4-float alignment of st_param_offsets (i.e. pointer into the flat parameter buffer).
 * Outputs: mag_hat, phs_hat [B,OT,F]; AA [B*OT, KP] (an_real | an_imag, padded);
 * reg_partial: per-wave partial sums of |mag_hat * exp(7 f/F)| (st_ae_fwd_partials() floats). */
int st_ae_fwd(const st_dims* d, const float* mag, const float* phs, const float* knobs,
              const float* ae_m, const float* ae_p, float* mag_hat, float* phs_hat, float* AA,
              float* reg_partial, float* ws, void* stream);
int st_ae_fwd_partials(const st_dims* d);
/* Floats of workspace st_ae_fwd uses in `ws`.  Fused kernels (T <= 32 and OT <= 16): OPTIONAL - when ws is given the
 * forward keeps each net's 16-wide code h4 there ([net][group][lane] float4) so that a following st_ae_bwd on the SAME
 * workspace starts its decoder half from it; ws may be NULL (h4 is then not kept and the backward recomputes it).  Wide
 * geometries (e.g. the 65536-sample window: T = 174, OT = 46) run the layers as feature-major GEMMs, keep their
 * activations there and REQUIRE it.  st_ae_bwd_ws_floats() covers the backward of either path (and contains the forward's
 * part at offset 0). */
size_t st_ae_fwd_ws_floats(const st_dims* d);

/* Hermitian fold of the synthesis bases (cls_fe_dft.py:109-110 expressed on the weights):
 * Sfold[KP,N]: rows [0,F) = Sr[k]+Sr[N-k], rows [KP/2,KP/2+F) = Si[k]-Si[N-k]; other rows 0. */
int st_synth_fold(const st_dims* d, const float* Sr, const float* Si, float* Sfold, void* stream);

/* Number of split-K slabs the two small-M synthesis GEMMs write: st_synth_frame_slabs() for st_synthesis_frames'
 * output frs (slabs x [B*OT,N], summed by st_ola_loss) and st_synth_slabs() for st_synthesis_dgrad's output dAA
 * (slabs x [B*OT,KP], summed by st_ae_bwd). */
int st_synth_slabs(const st_dims* d);
int st_synth_frame_slabs(const st_dims* d);

/* cls_fe_dft.py:112 ConvTranspose1d as a GEMM: frs[B*OT,N] = AA[B*OT,KP] * Sfold[KP,N] -- only what survives the crop of cls_fe_dft.py:113: frames that
 * lie wholly in the cropped margins are not computed, and (round 5, 128 x 128-tile path) of the partly cropped frames only the 128-tap tile columns that hold
 * a tap n with N <= H t + n < N + y.  st_ola_loss reads exactly those taps; everything else in frs is left as it was. */
int st_synthesis_frames(const st_dims* d, const float* AA, const float* Sfold, float* frs, void* stream);

/* Diagnostics, host only (no device work): the work list of the 128 x 128-tile synthesis GEMMs -- which = 0 st_synthesis_frames, 1 st_synthesis_dgrad's
 * padded form inside the fused step -- after the structural zeros of the cropped transposed convolution (cls_fe_dft.py:112-113) are dropped.
 * out[i] = tile row (8 bits) | tile column (6) << 8 | slab (2) << 14 | first zero-filled slab (2; 0 = none) << 16 | kind (1; 1: the two Nyquist columns of a
 * tile row) << 18 | first k unit (6) << 19 | k units (7) << 25; rows are the live frames enumerated frame-major (row = (t' - t'_lo) * B + b);
 * head6 = {slabs, col_h, col_stride, B, k-tiles (of 32) per k unit, k-tiles of the whole reduction} (tile column c covers output columns
 * (128 c % col_h) + (128 c / col_h) * col_stride ... + 128; col_h = 0: 128 c).  ncus <= 0: the current device's CU count; with ncus > 0 the result
 * is a pure function of (d, which, ncus) -- no device query.
 * Returns the entry count (one workgroup each; more than ncus = several rounds), 0 if the geometry does not use this kernel. */
int st_nt128_worklist(const st_dims* d, int which, int ncus, unsigned* out, int cap, int* head6);

/* Diagnostics, host only (no device work): the plan of the fp32 step's pair launch, which runs both 128 x 128-tile weight-gradient GEMMs (analysis and
 * synthesis bases) in one launch -- every workgroup slot runs one k-slice of an analysis tile and then one of a synthesis tile, the tile columns paired so that
 * the longest analysis slices meet the shortest synthesis slices.  out holds ten ints per slot, slots in the order (k-slice, tile row, tile column):
 * {tile row, tile column, k-slice, k_begin, k_end} of the analysis entry, then the same of the synthesis entry; -1 five times where the slot has no entry of
 * that GEMM (the GEMMs may have different k-slice counts).  k ranges are reduction rows of the frame-major order (row = (t - t_lo) * B + b) and are run in
 * k-tiles of 32 rows; k_end <= k_begin is an empty slice whose tile is stored as zeros.  ncus <= 0: the current device's CU count; with ncus > 0 the result is
 * a pure function of (d, ncus) and the tuning state.  Returns the slot count (cap only limits what is written), 0 where the step keeps one launch per GEMM
 * at these dims (16-bit or split operands, wide autoencoder geometries, N % 256 != 0, st_set_tuning(9582)), < 0 on bad arguments. */
int st_wgrad_pair_plan(const st_dims* d, int ncus, int* out, int cap);

/* Diagnostics, host only: what ONE weight-gradient GEMM and the sum of its k-slice slabs do at these dims -- the plan the launches themselves ask for, so with
 * ncus <= 0 (the current device's CU count) exactly what a launch on this device does under the current tuning state; with ncus > 0 a pure function of its
 * arguments and the tuning state.  which: 0 = the analysis bases, 1 = the synthesis bases.  half: -1 = the whole tensor, 0 / 1 = the real / imaginary basis alone
 * (analysis only: the split exchange of st_dp_train_step, stages 2 / 3 of st_loss_backward_stage).  flags: ST_WGPLAN_PADDED = operands in the padded workspace
 * layout (every fused entry; 0 = st_analysis_wgrad / st_synthesis_wgrad), ST_WGPLAN_G16 = the entry asks for the 16-bit operand pipeline (the training and
 * validation entries; taken where the precision admits it; needs ST_WGPLAN_PADDED), ST_WGPLAN_STAGED = st_loss_backward_stage, whose one-basis launches keep
 * the 96 x 96 kernel.  out receives min(cap, ST_WGRAD_PLAN_INTS) ints in the order of the ST_WGP_* indices:
 *   FORM      0 = the 128 x 128 fp32 kernel, 1 = the 96 x 96 three-wave kernel, 2 = the 16-bit kernel
 *   R         live reduction rows: B x the frames with a tap inside the unpadded signal
 *   SLICES    k-slices = slabs [KP][N] written at the start of the area
 *   M0, M     output rows [M0, M0 + M) of each slab (KP rows for the whole tensor, KP / 2 for one basis)
 *   FRAME_MAJOR, TRIM   reduction rows enumerated frame-major; per tile column only the rows that carry a tap inside the signal
 *   NYQ_P, NYQ_OFF, NYQ_WRITE   the slab sum reads NYQ_P Nyquist partials [2][N] at float offset NYQ_OFF of the area (0: the slabs hold those rows); 1 = this
 *             launch writes them (the real basis' launch writes them for both)
 *   USED      floats of the area the launch and its slab sum touch: never more than st_wgrad_ws_floats(d)
 * Returns ST_WGRAD_PLAN_INTS; < 0 on bad arguments (unsupported dims, which / half / flags out of range, one basis of the synthesis pair, cap < 0). */
enum { ST_WGPLAN_PADDED = 1, ST_WGPLAN_G16 = 2, ST_WGPLAN_STAGED = 4 };
enum { ST_WGP_FORM = 0, ST_WGP_R, ST_WGP_SLICES, ST_WGP_M0, ST_WGP_M, ST_WGP_FRAME_MAJOR, ST_WGP_TRIM, ST_WGP_NYQ_P, ST_WGP_NYQ_OFF, ST_WGP_NYQ_WRITE, ST_WGP_USED,
       ST_WGRAD_PLAN_INTS };
int st_wgrad_plan(const st_dims* d, int which, int half, int flags, int ncus, int* out, int cap);

/* Diagnostics, host only: what ONE of the other three STFT GEMMs does at these dims -- which: ST_STFT_ANALYSIS = the analysis forward (st_analysis_fwd),
 * ST_STFT_FRAMES = the synthesis frames (st_synthesis_frames), ST_STFT_DGRAD = the synthesis data gradient (st_synthesis_dgrad) -- the plan the launches
 * themselves ask for; ncus as in st_wgrad_plan.  flags: 0 = the per-op entry; ST_STFTPLAN_PADDED = operands in the padded workspace layout (every fused entry),
 * ST_STFTPLAN_SFOLDT = the transposed fold is there (every fused entry), ST_STFTPLAN_G16 = the entry asks for the 16-bit operand pipeline (the training,
 * validation and prediction entries; taken where the precision admits it); the last two need ST_STFTPLAN_PADDED.  out receives min(cap, ST_STFT_PLAN_INTS)
 * ints in the order of the ST_SGP_* indices:
 *   FAMILY    operands: 0 = fp32 on the fp32 MFMA, 1 = fp32 converted while staged (bf16 / f16 / the in-kernel three-plane split of ST_PREC_F32X3),
 *             2 = bfloat16 planes of the once-per-step operands, 3 = the 16-bit operand pipeline
 *   FORM      kernel: 0 = the small-tile kernel ((32 WAVES) x 96), 1 = the 128 x 128 work-list kernel (st_nt128_worklist is its list), 2 = the plane kernel
 *             ((32 WAVES) x 96), 3 = the 16-bit 128 x 128 kernel, 4 = the 16-bit LDS-DMA kernel (256 x 128)
 *   WAVES     waves per workgroup of forms 0 and 2 (0 elsewhere: fixed by the kernel)
 *   BK, XT    family 0 on form 0: k-tile depth (16 / 32) and 1 = k-quad-major staging; 0 elsewhere
 *   R, M, NC, K   live rows (B x the frames with a tap inside the signal resp. the crop); the GEMM is M = R rows x NC columns over K
 *   SLABS     split-K slabs: 1 for the analysis forward, st_synth_frame_slabs(d) / st_synth_slabs(d) for the other two, whatever the family
 *   FRAME_MAJOR, CROP   rows enumerated frame-major (only where st_fm_div_exact(R, B)); structural zeros of the crop skipped: 0 none, 1 the dead tile columns of
 *             the frames GEMM, 2 the dead taps per tile row of the data gradient
 *   WORK      entries of the work list (form 1; 0 elsewhere)
 *   T_LO, TV  the live frames [T_LO, T_LO + TV)
 * Returns ST_STFT_PLAN_INTS; < 0 on bad arguments (unsupported dims, which / flags out of range, cap < 0). */
enum { ST_STFT_ANALYSIS = 0, ST_STFT_FRAMES = 1, ST_STFT_DGRAD = 2 };
enum { ST_STFTPLAN_PADDED = 1, ST_STFTPLAN_G16 = 2, ST_STFTPLAN_SFOLDT = 4 };
enum { ST_SGP_FAMILY = 0, ST_SGP_FORM, ST_SGP_WAVES, ST_SGP_BK, ST_SGP_XT, ST_SGP_R, ST_SGP_M, ST_SGP_NC, ST_SGP_K, ST_SGP_SLABS, ST_SGP_FRAME_MAJOR, ST_SGP_CROP,
       ST_SGP_WORK, ST_SGP_T_LO, ST_SGP_TV, ST_STFT_PLAN_INTS };
int st_stft_plan(const st_dims* d, int which, int flags, int ncus, int* out, int cap);

/* Diagnostics, host only: 1 if the frame-major row order may be used for a GEMM with R = (live frames) * B compact rows, i.e. if the kernels' division of a
 * row index r < R by B through a multiply-high with floor(2^32 / B) + 1 is exact (r * B < 2^32 for every r); 0: those launches keep the window-major order
 * and the untrimmed / uncropped tile sets.  (cls_fe_dft.py:28-31, :112-113: the trimming is an optimisation of the padded / cropped frames, never a
 * change of results.) */
int st_fm_div_exact(int R, int B);

/* cls_fe_dft.py:112-113 overlap-add + crop, nn_proc.py:332,340 residual and x2,
 * loss_functions.py:9-10 log-cosh partial sums and d loss/d syn.
 * y_true may be NULL (inference): then only y_hat is produced.
 * loss_partial[b * st_ola_loss_partials() + s] = the sum over samples [256 s, 256 s + 256) of window b, always by the same summation tree
 * (quads in sample order, then a balanced binary tree over the quad sums): the bits do not depend on the pointers' alignment, which only
 * selects between the 16-byte and the 4-byte access form of the kernel. */
int st_ola_loss(const st_dims* d, const float* frs, const float* x, const float* y_true,
                float* y_hat, float* dsyn, float* loss_partial, void* stream);
int st_ola_loss_partials(const st_dims* d);

/* Backward of the synthesis GEMM wrt its input: dAA[B*OT,KP] = frames(dsyn) * Sfold^T.  Columns [F, KP/2) and [KP/2 + F, KP) (the padding of the
 * spectral pitch) are written as zeros by the small-tile kernels and LEFT AS THEY WERE by the work-list kernel (see st_workspace_bytes). */
int st_synthesis_dgrad(const st_dims* d, const float* dsyn, const float* Sfold, float* dAA, void* stream);

/* Weight gradient of the synthesis bases (folded then unfolded to Sr/Si [N,N]); also emits
 * partial sums of |g| for the L1 clip (nn_proc.py:299-302).  ws: split-K scratch. */
int st_synthesis_wgrad(const st_dims* d, const float* AA, const float* dsyn, float* ws,
                       float* gSr, float* gSi, float* norm_partial, void* stream);

/* Backward of both autoencoders (recomputes activations) incl. nn_proc.py:322-326 and the
 * L1 term of loss_functions.py:36.  Outputs dmag, dphs [B,T,F]; per-wave partial weight grads
 * in ws (st_ae_bwd_ws_floats()), reduced into g_m / g_p (same packing as ae_m / ae_p). */
int st_ae_bwd(const st_dims* d, const float* mag, const float* phs, const float* knobs,
              const float* ae_m, const float* ae_p, const float* mag_hat, const float* phs_hat,
              const float* dAA, const float* g_mag_hat /* optional extra d/d mag_hat */, float reg_coef,
              float* dmag, float* dphs, float* ws, float* g_m, float* g_p, void* stream);
size_t st_ae_bwd_ws_floats(const st_dims* d);
/* Round 6.  In the fused step (st_model_fwd with save_for_backward / st_loss_backward / st_train_step) of the fused geometries with fp32 autoencoder
 * layers, the forward kernel KEEPS the post-ELU activations of both nets -- what the reference's autograd keeps (nn_proc.py:77-126) -- in the
 * autoencoder workspace behind the gradient partials, and the backward reads them instead of recomputing the forward chain.  Returns the bytes the
 * forward writes (and the backward reads back) per call: 2 nets x B * ceil(F / 16) row groups x 17 KB (294 MB at B = 256); 0 where the path is not
 * taken (16-bit autoencoder layers, wide geometries, the recompute switch g_ae_save = 0).  st_ae_bwd on its own (no forward in the same workspace) recomputes. */
size_t st_ae_kept_activation_bytes(const st_dims* d);
/* Round 10.  On the same configurations every fused forward (training step, st_model_fwd, st_eval_step) also leaves the autoencoders' LDS weight images --
 * both nets' forward and data-gradient fragment images with their zero padding, and the per-bin frequency weights of the L1 term -- at the head of the
 * autoencoder workspace, in the h4 / d a4 exchange areas that only the split backward uses (no size changes): its first launch builds them once, and the
 * autoencoder kernels copy them into LDS instead of rebuilding them in each of their 512 workgroups.  A part that does not fit there (the backward's below
 * 38 row groups, the forward's below 20 at the default geometry) is built in the kernel as before, as in st_ae_fwd / st_ae_bwd on their own and in the
 * whole step under st_set_tuning(8202) (the A/B reference of tests/test_gpu_ae_weight_images.py: identical bits). */

/* Backward of nn_proc.py:309-310: dG[B*T,KP] (d re | d im) from (re,im,dmag,dphs). */
int st_polar_bwd(const st_dims* d, const float* re, const float* im, const float* dmag, const float* dphs,
                 const float* g_mag /* optional extra d/d mag */, float* dG, void* stream);

/* Weight gradient of the analysis bases: gWr/gWi[N,N] rows [0,F) written, rows >= F untouched
 * (they are structurally zero).  Emits |g| partial sums. */
int st_analysis_wgrad(const st_dims* d, const float* dG, const float* x, float in_scale, float* ws,
                      float* gWr, float* gWi, float* norm_partial, void* stream);
size_t st_wgrad_ws_floats(const st_dims* d);
int st_norm_partials(const st_dims* d);

/* nn_proc.py:299-302 L1 clip (STFT tensors = first 4 tensors of the flat buffer) fused with
 * torch.optim.Adam.step (train.py:147).  scalars: device float[8] written by st_finalize_scalars.
 * st_clip_adam refuses, before any launch: a NULL pointer, n_total <= 0, n_stft < 0, either not a multiple of 4, n_stft > n_total, step < 1. */
int st_finalize_scalars(const st_dims* d, const float* loss_partial, const float* reg_partial,
                        const float* norm_partial_a, const float* norm_partial_s, float inv_world,
                        float* scalars /* [0]=loss [1]=logcosh [2]=reg [3]=l1norm [4]=clip_coef [5]=overflow */, void* stream);
int st_clip_adam(float* params, float* grads, float* m, float* v, int64_t n_total, int64_t n_stft,
                 const float* scalars, float grad_scale, float lr, float beta1, float beta2, float eps, int step,
                 void* stream);

/* ---------------------------------------------------------------- fused entry points ----- */
/* st_model.forward (nn_proc.py:392 -> :305-340), inference/validation: y_hat[B,y], mag[B,T,F],
 * mag_hat[B,OT,F].  params = flat parameter buffer; ws = st_workspace_bytes(). */
int st_model_fwd(const st_dims* d, const float* params, const float* x, const float* knobs,
                 float* y_hat, float* mag, float* mag_hat, void* ws, int save_for_backward, void* stream);

/* Autograd backward of st_model_fwd(save_for_backward=1) for arbitrary upstream gradients
 * g_y_hat[B,y] (required), g_mag_hat[B,OT,F], g_mag[B,T,F] (optional): fills the flat `grads`
 * (rows >= F of the analysis tensors are never written: keep them zero). */
int st_model_bwd(const st_dims* d, const float* params, float* grads, const float* x, const float* knobs,
                 const float* g_y_hat, const float* g_mag_hat, const float* g_mag, void* ws, void* stream);

/* One optimisation step of train.py:112-151 WITHOUT the optimiser: forward, loss, backward.
 * grads (flat, same layout as params) are overwritten; scalars[0..3] receive loss terms and the
 * STFT L1 norm (before any all-reduce).  y_hat/mag/mag_hat may be NULL. */
int st_loss_backward(const st_dims* d, const float* params, float* grads, const float* x, const float* knobs,
                     const float* y_true, float* y_hat, float* mag, float* mag_hat, void* ws,
                     float* scalars, void* stream);

/* One validation batch of train.py:28-80 on the device: forward, calc_loss with scale_by_freq (loss_functions.py:26-36) and mae
 * (loss_functions.py:19-20).  The forward is the one st_train_step takes at this st_dims.prec (the 16-bit levels run the GEMMs on pre-rounded 16-bit
 * operands, which st_model_fwd does not); nothing is kept for a backward -- the saved state of `ws` is gone afterwards -- no gradient is written, no
 * mag / mag_hat copy is made, and there is no host synchronisation and no allocation.  st_dims.loss_scale and clip_all are ignored: the reported
 * values never carry the loss scale.  y_hat[B,y] may be NULL; knobs may be NULL for K == 0.
 * acc: 8 doubles on the device, updated by the last kernel of the call:
 *   [0] running average beta * acc[0] + (1 - beta) * loss, formed in double as train.py:33 forms vl_avg (the caller seeds it: train.py carries
 *       vl_avg from epoch to epoch)                        [1] this batch's loss        [2] its mean log-cosh      [3] its L1 term
 *   [4] this batch's MAE (train.py:34 logs the last one)   [5] batches accumulated      [6], [7] running sums of loss and MAE
 * The caller resets by writing acc.  [1..3] are formed exactly as st_finalize_scalars forms scalars[0..2]; the MAE partials (one per 256 samples, by the
 * summation tree of st_ola_loss's loss partials, bits independent of pointer alignment) live in the workspace's d syn area: st_workspace_bytes is unchanged. */
int st_eval_step(const st_dims* d, const float* params, const float* x, const float* knobs, const float* y_true,
                 float* y_hat /* may be NULL */, void* ws, double* acc /* device, 8 doubles */, double beta, void* stream);

/* Whole-signal inference, utils/predict_long.py:30-79, as ONE call: a recording of n samples resident on the device goes through the model window by window
 * without a copy of the windows, of the knob matrix or of the concatenated output.
 * Windows (audio.sliding_window, audio.py:23-49, with overlap L - y): n < L gives one window, otherwise ceil((n - L) / y) + 1; window w reads
 * signal[w y, w y + L) with zeros from sample n on -- no padded copy of the signal is made.  Output: st_predict_out_samples = max(n - (L - y), 0) floats; sample i
 * belongs to window i / y at position i % y and to input sample (L - y) + i (the first window's lookback has no prediction, as in the reference); the last window
 * is clipped inside the kernel, nothing at or past out + n_out is written and nothing at or past signal + n is read.
 *   fmt         ST_PCM_F32 or ST_PCM_S16 (the pool formats of st_file_feed); an int16 sample converts as (float)((double)s / 32767.0), so an int16 recording gives,
 *               bit for bit, the result of its float32 image.
 *   knobs       [knob_rows][K], knob_rows == 1 (one setting for the whole signal) or == the window count (one row per window: knob automation); NULL for K == 0.
 *   d->B        windows per internal batch: all batches are enqueued on `stream` by the one call -- no host synchronisation, no allocation, no hipMemcpy.
 *   ws          st_predict_ws_bytes(d) bytes, 16-byte aligned: [what depends on the parameters only | the workspace of one batch].  The first part -- the folded
 *               synthesis bases, the 16-bit (or three-plane) copies of the bases where st_dims.prec runs on them, the autoencoders' LDS weight images where the
 *               fp32 forward kernel takes them -- is built ONCE per call (st_model_fwd / st_eval_step rebuild it per batch) and does not move when the last batch is
 *               smaller than d->B; the second covers st_workspace_bytes of every batch 1 .. d->B.  Its saved-for-backward state is gone afterwards.
 * Per batch: one staging launch (x / 2 with the Conv1d padding as the analysis GEMM's operand, fp32 or 16-bit, straight from the signal; the all-padding frames;
 * the knob rows where knob_rows == 1), the forward st_eval_step takes at this st_dims.prec (the 16-bit levels run the pre-rounded operand GEMMs) with nothing kept
 * for a backward and no mag / mag_hat copies, and one overlap-add launch that sums the synthesis frames in st_ola_loss's order, takes the residual from the signal
 * and writes 2 (s + x / 2) to its place in out.  Parameters are only read; st_dims.loss_scale and clip_all are ignored.
 * st_predict_supported (host only): 1 for every geometry of the fused autoencoder kernels (T <= 32 and OT <= 16) at every ST_PREC_* level; 0 for bad dims and for the
 * wide geometries (e.g. the 65536-sample window), which stay on st_model_fwd batch by batch.  st_predict_windows / st_predict_out_samples (host only): 0 for bad
 * dims (st_predict_windows: also for n <= 0).  st_predict_ws_bytes: 0 for bad or unsupported dims.
 * Refused before any launch (ST_ERR_ARG, the rule in st_last_error()): bad dims; a null pointer (knobs only where K > 0); n <= 0; an unknown fmt; knob_rows neither 1
 * nor the window count; signal or out not 16-byte aligned (ST_PCM_S16: signal 8-byte); ws not 16-byte aligned; dims st_predict_supported rejects.
 * An n with no output sample (n <= L - y) returns ST_OK without a launch. */
long long st_predict_windows(const st_dims* d, long long n);
long long st_predict_out_samples(const st_dims* d, long long n);
int       st_predict_supported(const st_dims* d);
size_t    st_predict_ws_bytes(const st_dims* d);
int st_predict_long(const st_dims* d, const float* params, int fmt, const void* signal, long long n,
                    const float* knobs, long long knob_rows, float* out, void* ws, void* stream);

/* Predict session: st_predict_long's inference fed block by block, `channels` signals in lockstep (st_predict_stream.h).  The model has no look-ahead -- output
 * sample i belongs to input sample (L - y) + i -- so a session emits every output sample as soon as its window is complete and keeps only the samples no complete
 * window has consumed yet.  That history stays on the device, the parameter-only head of the workspace is built once at open, and a batch's rows are (channel,
 * window) pairs, so many channels fill a batch even at one window per push.
 *   st_predict_stream   plain data in HOST memory, owned by the caller, written by open / push / reset only: samples received and emitted per channel, channels,
 *               samples held, which history half is current, the closed flag, and the geometry, prec and B the session was opened with.
 *   state       st_predict_stream_state_bytes(d, channels) = 2 * channels * L * sizeof(float) bytes on the device, 16-byte aligned: two history halves
 *               [2][channels][L] float32 (float32 whatever the block format, so an int16 stream equals its float image bit for bit).  Need not be initialised.
 *   ws          st_predict_stream_ws_bytes(d) bytes (>= st_predict_ws_bytes(d)) on the device, 16-byte aligned: [parameter-only head | one batch's workspace].
 *               It belongs to the session from open to its last push: st_predict_stream_open builds the head (what st_predict_long builds once per call), the
 *               pushes only read it.  That the parameters have not changed since open is the caller's precondition.
 *   push        m new samples per channel, block[c][0 .. m) at pitch block_pitch (elements), ST_PCM_F32 or ST_PCM_S16 ((float)s / 32767.0f, as everywhere).  With
 *               n0 samples received before the push, n1 = n0 + m after it, and Wc(n) = n < L ? 0 : (n - L) / y + 1 complete windows in n samples, a non-final push
 *               computes windows Wc(n0) .. Wc(n1) - 1 of every channel and writes their y samples each, concatenated, to out[c][0 .. nw y) at pitch out_pitch.  A
 *               final push (any m >= 0) also computes the one zero-padded last window where st_predict_windows(d, n1) > Wc(n1), clipped as st_predict_long clips
 *               it: over its life a session emits exactly st_predict_out_samples(d, n) samples per channel, the ones st_predict_long gives for the concatenated
 *               channel.  After a final push the session is closed until st_predict_stream_reset (host only: zero samples received, same geometry and channels).
 *   plan        st_predict_stream_plan (host arithmetic only; the push uses the same function): out4 = {first window, window count, samples emitted per channel,
 *               samples held afterwards} for a push of m at n_in samples received.  Held after a non-final push: [Wc(n1) y, n1), at most L - 1 samples
 *               (L - y + (n1 - L) % y once n1 >= L); after a final push nothing.
 *   alignment   a non-final push needs m % 4 == 0, so the held count and every window start stay multiples of four: every quad of the pair (history | block) is
 *               one aligned access and none straddles the join.  block: 16-byte aligned (ST_PCM_S16: 8-byte), block_pitch >= m and % 4 == 0; out: 16-byte
 *               aligned, out_pitch >= the emitted count and % 4 == 0.  Nothing at or past block[c] + m is read and nothing outside out[c][0 .. emitted) is written.
 *   knobs       [knob_rows][K], knob_rows == 1 (all channels) or == channels (one setting per channel), held for every window of the push; NULL only for K == 0.
 *               Finer automation means smaller pushes.
 *   rows        a push that computes nw windows of C channels has C * nw rows; row r = c * nw + k is window Wc(n0) + k of channel c.  d->B is the most rows per
 *               batch; a push with more rows runs its batches one after the other inside the call.  No allocation, no hipMemcpy, no host synchronisation, no float
 *               atomics, no captured graph: the host struct is advanced by host arithmetic when the push is enqueued.
 * Per batch: one staging launch (st_predict_long's, reading the pair; the knob rows always filled, per channel), st_predict_long's analysis GEMM, autoencoder
 * forward and frames GEMM at this st_dims.prec, one overlap-add launch in st_predict_long's summation order with the residual from the pair.  After the last
 * batch of a non-final push one carry launch copies the samples to keep into the other history half and the halves swap; it is the only launch of a push that
 * completes no window.  Equal bits: a batch whose rows are the windows of one st_predict_long batch (same d->B, same row count) gives that batch's bits; an int16
 * stream its float image's; knob_rows == 1 the row repeated.  Other partitions into pushes give other row counts per batch: equal to 1e-6 of max|y|, as between
 * two batch sizes of st_predict_long.
 * The fused autoencoder geometries only (st_predict_supported), at every ST_PREC_* level.  The size functions give 0 for bad or unsupported dims (state: also for
 * channels < 1).
 * Refused before any launch (ST_ERR_ARG, the rule in st_last_error(), naming the entry): bad or unsupported dims; dims, prec or B that differ from the ones the
 * session was opened with; channels < 1 (or above 65535); a null pointer, named (knobs only where K > 0; block only where m > 0; out only where the plan emits
 * something); m < 0 or m > 2^30; a non-final m % 4 != 0; an unknown fmt; knob_rows neither 1 nor channels; block_pitch < m or % 4 != 0; out_pitch below the
 * emitted count or % 4 != 0; block misaligned; out, state or ws not 16-byte aligned; a push on a closed session. */
typedef struct st_predict_stream {
    long long received, emitted;        /* samples per channel so far */
    int channels, held, half, closed;   /* held: samples [received - held, received) of every channel lie in history half `half` */
    int L, N, H, T, OT, F, K, y, prec, B;
} st_predict_stream;
size_t st_predict_stream_state_bytes(const st_dims* d, int channels);
size_t st_predict_stream_ws_bytes(const st_dims* d);
int    st_predict_stream_plan(const st_dims* d, long long n_in, long long m, int final, long long out4[4]);
int    st_predict_stream_open(const st_dims* d, const float* params, int channels, st_predict_stream* s, void* state, void* ws, void* stream);
int    st_predict_stream_push(const st_dims* d, const float* params, st_predict_stream* s, int fmt, const void* block, long long m, long long block_pitch,
                              int final, const float* knobs, long long knob_rows, float* out, long long out_pitch, void* state, void* ws, void* stream);
int    st_predict_stream_reset(st_predict_stream* s);

/* Knob fit on the device: the knob settings for which the model turns `signal` into `target` (predict.fit_knobs), every batch of every optimiser step enqueued by
 * ONE call.  Windows, lengths and formats are st_predict_long's: nwin = st_predict_windows(d, n); window w reads signal[w y, w y + L) with zeros from sample n on;
 * fmt (ST_PCM_F32 / ST_PCM_S16, an int16 sample converts as (float)((double)s / 32767.0)) applies to both recordings; target holds the same n samples, aligned with
 * signal, and the target of output sample i, 0 <= i < n_out = st_predict_out_samples(d, n), is target[(L - y) + i].  Nothing at or past signal + n or target + n is read.
 * Objective: J(knobs) = (1 / n_out) * sum_{i < n_out} logcosh(y_hat_i - target_i), y_hat as st_predict_long forms it at this st_dims.prec.  Output positions of the last
 * window that lie behind the end of the recording carry no loss and no gradient (the host route of predict.fit_knobs counts its zero-padded tail; the two objectives
 * coincide when n = L + k y).
 *   knobs       [knob_rows][K], start values in, fitted values out.  knob_rows == 1: one setting, its gradient the sum over all windows in ascending window order;
 *               knob_rows == nwin: one row per window (knob automation), row w receives window w's own gradient of the same J.
 *   adam_m, adam_v  [knob_rows][K] Adam moments, updated in place (zeros before the first step).
 *   per step s = 0 .. steps - 1: loss_hist[s] = J at the knobs BEFORE the update; grad_hist[s] ([knob_rows][K], skipped where grad_hist is NULL) that gradient; then
 *               torch.optim.Adam's update at step number first_step + s (1-based, bias-corrected, denom = sqrt(v) / sqrt(1 - beta2^t) + eps) and a clamp to
 *               [-0.5, 0.5].  `steps` calls of one step chained through first_step are, bit for bit, one call of `steps` steps.
 *   loss_hist   device, [steps] doubles;  grad_hist  device, [steps][knob_rows][K] floats or NULL.
 *   ws          st_fit_knobs_ws_bytes(d) bytes (>= st_predict_ws_bytes(d)), 16-byte aligned: [st_predict_long's parameter-only head, built once per call | the
 *               per-window gradient rows of a batch, the one-row accumulator and the per-group scratch | one batch's workspace].
 * Per batch: st_predict_long's staging launch, analysis GEMM and autoencoder forward (the 16-wide code h4 kept), the frames GEMM; one overlap-add launch that also
 * writes 2 tanh(y_hat - target) as the padded operand of the synthesis data-gradient GEMM (zeros in the padding and behind the recording's end) and the log-cosh
 * partials in st_ola_loss's formula; that GEMM; the knob-only autoencoder backward (data gradients of layers 9..6 and ELU' at layer 5: no weight or bias gradient,
 * no encoder half, no polar backward); the per-window reduce that applies W5; one tail launch (loss partials into loss_hist[s] in double; after the step's last batch
 * the window sum, 1 / n_out, grad_hist[s], Adam and the clamp).  1 / n_out is applied in fp32 BEHIND the reduce that applies W5: the operand of the data-gradient GEMM
 * is unscaled, so the 16-bit levels do not lose it to the fp16 subnormal range however long the recording.  st_dims.loss_scale and clip_all are ignored.
 * No float atomics: every reduction has a fixed order and a repeated call repeats its bits.  No allocation, no hipMemcpy, no host synchronisation; parameters are only read.
 * st_fit_knobs_supported (host only): st_predict_supported(d) && d->K >= 1.  st_fit_knobs_ws_bytes: 0 for bad or unsupported dims.
 * Refused before any launch (ST_ERR_ARG, the rule in st_last_error(), naming st_fit_knobs): bad dims; K < 1; a null pointer, named (grad_hist may be NULL); n <= 0; an
 * unknown fmt; knob_rows neither 1 nor the window count; steps < 1; first_step < 1; lr, beta1, beta2 or eps not finite, lr < 0, a beta outside [0, 1), eps <= 0;
 * signal or target not 16-byte aligned (ST_PCM_S16: 8-byte); knobs, adam_m, adam_v or ws not 16-byte aligned; dims st_fit_knobs_supported rejects (the wide geometries).
 * An n with no output sample (n <= L - y) returns ST_OK without a launch and leaves every buffer alone. */
int    st_fit_knobs_supported(const st_dims* d);
size_t st_fit_knobs_ws_bytes(const st_dims* d);
int    st_fit_knobs(const st_dims* d, const float* params, int fmt, const void* signal, const void* target, long long n,
                    float* knobs, long long knob_rows, float* adam_m, float* adam_v,
                    long long first_step, int steps, float lr, float beta1, float beta2, float eps,
                    double* loss_hist /* device, [steps] */, float* grad_hist /* device, [steps][knob_rows][K], may be NULL */,
                    void* ws, void* stream);

/* Encode a recording once, decode it at any knob setting.  The knobs enter at layer 5 of 9: window staging, the analysis GEMM, the polar form and encoder layers
 * 1..4 of both autoencoders do not depend on them.  st_encode_long runs that half over the recording (windows, lengths and formats are st_predict_long's) and
 * leaves the recording's CODE in device memory; st_decode_long and st_fit_knobs_coded then run only layers 5..9, the polar epilogue, the frames GEMM and the
 * overlap-add per knob setting / optimiser step.  The fused autoencoder geometries only (st_decode_supported == st_predict_supported).
 *   code        st_code_bytes(d, n) bytes, 16-byte aligned, opaque.  Per window of st_predict_windows(d, n): the 16-wide code h4 of both nets and the last OT frames
 *               of the window's mag and phs, rows padded to KP / 2 bins:
 *                   st_code_bytes(d, n) = st_predict_windows(d, n) * (st_kp(d->F) / 2) * (32 + 2 * d->OT) * sizeof(float)
 *               and 0 for bad dims, the wide geometries and n <= 0.  Window-major: it does not depend on d->B, so a code built at one batch size decodes at another.
 *               It is valid for the st_dims.prec, the parameters and the recording it was built from; that none of them changed since the encode is the caller's
 *               precondition (nothing detects it).
 *   ws          st_decode_ws_bytes(d) bytes (== st_predict_ws_bytes(d)), 16-byte aligned, for st_encode_long and st_decode_long; st_fit_knobs_coded takes
 *               st_fit_knobs_ws_bytes(d).  Scratch: nothing in it is read before it is written.
 * st_decode_long: knobs [n_settings][knob_rows][K] on the device, knob_rows = 1 (one setting for the whole recording) or the window count (one row per window),
 *   n_settings >= 1.  Row s of the result -- the n_out = n - (L - y) samples st_predict_long gives at setting s at this st_dims.prec, up to the order of a few sums --
 *   goes to out + s * out_pitch; out_pitch >= n_out, out_pitch % 4 == 0, out 16-byte aligned; nothing outside [0, n_out) of a row is written.  The recording is an
 *   argument because the overlap-add takes the residual x / 2 from it; nothing at or past signal + n is read.  Settings run inside the batch loop: settings 2..S of a
 *   batch read its code from the caches.
 * st_fit_knobs_coded: st_fit_knobs with the code after params; every argument, result and refusal is st_fit_knobs' (named st_fit_knobs_coded), plus: code NULL or
 *   not 16-byte aligned.  Every step's forward is the decoder forward from the code -- no staging launch, no analysis GEMM, no encoder; everything behind the frames
 *   GEMM is st_fit_knobs'.
 * No float atomics, fixed summation orders, no allocation, no hipMemcpy, no host synchronisation; parameters, the code (decode, fit) and the recording are only read.
 * Refused before any launch (ST_ERR_ARG, the rule in st_last_error(), naming the entry): bad dims; a null pointer, named; n <= 0; an unknown fmt; signal not 16-byte
 * aligned (ST_PCM_S16: 8-byte); code, out or ws not 16-byte aligned; knob_rows neither 1 nor the window count; n_settings < 1; out_pitch < n_out or not a multiple of
 * 4; dims st_decode_supported rejects (the wide geometries).  An n with no output sample (n <= L - y) returns ST_OK without a launch. */
int    st_decode_supported(const st_dims* d);
size_t st_decode_ws_bytes(const st_dims* d);
size_t st_code_bytes(const st_dims* d, long long n);
int    st_encode_long(const st_dims* d, const float* params, int fmt, const void* signal, long long n, void* code, void* ws, void* stream);
int    st_decode_long(const st_dims* d, const float* params, const void* code, int fmt, const void* signal, long long n,
                      const float* knobs, long long knob_rows, int n_settings, float* out, long long out_pitch, void* ws, void* stream);
int    st_fit_knobs_coded(const st_dims* d, const float* params, const void* code, int fmt, const void* signal, const void* target, long long n,
                          float* knobs, long long knob_rows, float* adam_m, float* adam_v,
                          long long first_step, int steps, float lr, float beta1, float beta2, float eps,
                          double* loss_hist /* device, [steps] */, float* grad_hist /* device, [steps][knob_rows][K], may be NULL */,
                          void* ws, void* stream);

/* Many knob settings of one recording from its code: a loss-only SCORE of S settings and a FIT of S starts at once.  J is not convex in the knobs, so a search scores
 * many candidates, keeps the best few and refines them together; both steps read the code st_encode_long left (valid as stated there).  Windows, lengths, formats
 * and the objective J are st_fit_knobs_coded's.  The fused autoencoder geometries only, K >= 1 (st_fit_knobs_supported).
 * Rows of an internal batch are (setting, window) pairs, so that a recording shorter than a batch still fills it.  st_knob_multi_plan (host arithmetic only) gives
 * the batches both entries walk, as 4-tuples (w0, nw, s0, ns) in out[4 i .. 4 i + 3], i < min(count, cap): windows w0 .. w0 + nw - 1 at settings s0 .. s0 + ns - 1,
 * nw * ns <= d->B rows, row r of the batch being setting s0 + r / nw at window w0 + r % nw.  The rule, with nwin = st_predict_windows(d, n):
 *     2 * nwin > d->B    st_decode_long's batches: ns == 1, nw = min(d->B, nwin - w0), the settings loop inside the window batch;
 *     otherwise          every batch holds the whole recording ns = min(d->B / nwin, n_settings - s0) times (stacked).
 * Every (setting, window) pair appears exactly once; the windows of any one setting appear in ascending order.  Returns the tuple count -- also when cap is too
 * small or out is NULL -- and 0 for bad or unsupported dims, n <= 0 and n_settings < 1.
 *   knobs       [n_settings][knob_rows][K] on the device, knob_rows == 1 or the window count.  Only the base pointer needs 16-byte alignment: the settings' rows are
 *               read with scalar loads, whatever K.
 *   ws          st_knob_multi_ws_bytes(d, n_settings) bytes (>= st_fit_knobs_ws_bytes(d), not decreasing in n_settings; 0 for bad or unsupported dims and
 *               n_settings < 1), 16-byte aligned: st_fit_knobs' workspace with the per-setting gradient accumulators and the score's per-setting loss partials
 *               of one window batch in front of the batch's.  Scratch: nothing in it is read before it is written.
 * st_score_knobs_coded: loss[s] = J at setting s; win_loss[s][w] (may be NULL) = the sum of log-cosh over window w's valid output samples times 1 / n_out -- the rows
 *   sum to loss[s] up to rounding; with knob_rows == nwin that is the per-window best of a grid.  Per plan batch: the decoder forward, the frames GEMM, ONE
 *   overlap-add launch that forms st_fit_knobs' sums and log-cosh partials (the same formula, the same per-slot tree, the same validity rule behind the recording's
 *   end) and writes no output sample and no gradient operand; a tail launch of one workgroup per setting then folds the partials into loss / win_loss in
 *   double, in a fixed order -- behind every stacked batch, and once per window batch, behind its last setting, where the recording is not stacked.  No
 *   [S][n_out] buffer exists.
 * st_fit_knobs_multi_coded: S independent runs of st_fit_knobs_coded -- setting s has its own rows of knobs / adam_m / adam_v ([n_settings][knob_rows][K], in place),
 *   loss_hist[step][s] and grad_hist[step][s][knob_rows][K] (may be NULL).  Per plan batch it runs what st_fit_knobs_coded runs, over the stacked rows; the tail, per
 *   setting: the loss partials in st_fit_knobs' order, the setting's rows summed in ascending window order (or taken row by row for knob_rows == nwin), and after the
 *   setting's last batch of the step 1 / n_out, grad_hist, Adam and the clamp, in st_fit_knobs' arithmetic.  The parameter-only head is built once per call.
 *   `steps` calls of one step chained through first_step are, bit for bit, one call of `steps` steps; n_settings == 1 is st_fit_knobs_coded bit for bit.
 * No float atomics: every sum has a fixed order and a repeated call repeats its bits.  No allocation, no hipMemcpy, no host synchronisation; parameters, the code and
 * the recordings are only read.
 * Refused before any launch (ST_ERR_ARG, the rule in st_last_error(), naming the entry): everything st_fit_knobs_coded refuses (the optimiser's arguments: the fit
 * only), n_settings < 1, a null loss / loss_hist, and a plan batch whose stacked row count exceeds the kernels' 32-bit element offsets.  An n with no output sample
 * (n <= L - y) returns ST_OK without a launch. */
int    st_knob_multi_plan(const st_dims* d, long long n, int n_settings, int* out, int cap);
size_t st_knob_multi_ws_bytes(const st_dims* d, int n_settings);
int    st_score_knobs_coded(const st_dims* d, const float* params, const void* code, int fmt, const void* signal, const void* target, long long n,
                            const float* knobs /* [n_settings][knob_rows][K] */, long long knob_rows, int n_settings,
                            double* loss /* device, [n_settings] */, float* win_loss /* device, [n_settings][nwin], may be NULL */, void* ws, void* stream);
int    st_fit_knobs_multi_coded(const st_dims* d, const float* params, const void* code, int fmt, const void* signal, const void* target, long long n,
                                float* knobs /* [n_settings][knob_rows][K], in / out */, long long knob_rows, int n_settings, float* adam_m, float* adam_v,
                                long long first_step, int steps, float lr, float beta1, float beta2, float eps,
                                double* loss_hist /* device, [steps][n_settings] */, float* grad_hist /* device, [steps][n_settings][knob_rows][K], may be NULL */,
                                void* ws, void* stream);

/* ---- a folder of recordings in one call: st_eval_pool (csrc/st_eval_pool.h) ----------------------------------------------------
 * Reporting a model on a SignalTrain test set: every file of the folder (input_N_.wav / target_N_<effect>__k1__k2....wav, datasets.py:64-259) WHOLE through the
 * network at the knob setting in its name (utils/predict_long.py:30-79 per file), and the error per file.  The folder is the pool the device feeds keep
 * (st_file_feed): pool_x / pool_y, the files' audio concatenated (fmt as there), file_off / file_len (device int64, in samples) and one knob row per file.
 * Batch rows are (file, window) pairs: row r is window r - win_off[f] of file f, win_off[f] <= r < win_off[f + 1] (file-major, windows ascending), so short clips
 * share a batch of up to d->B rows and a long file spans several.  Windows of a file of `len` samples: st_predict_windows(d, len) if len > L - y, else 0 (no
 * output sample, no row).  st_eval_pool_rows is host arithmetic: it returns the total and, if win_off_host != NULL, fills the prefix sums [nfiles + 1] the
 * caller uploads as win_off (0 for bad dims, a null file_len_host or nfiles < 1).
 *
 * One call enqueues every batch: the parameter-only head of the workspace once (as st_predict_long), then per batch the forward at st_dims.prec (every level).
 * No allocation, no hipMemcpy, no host synchronisation; parameters and pools are only read.
 *   out    (may be NULL: the score form) pool-shaped, [pool_samples]: the prediction for output sample i of file f at out[file_off[f] + (L - y) + i] --
 *          time-aligned with the input (predict_long.py:222-223) -- clipped at the file's end; the first min(L - y, len) samples of every file's span are
 *          written as 0.  Every sample of out inside some file's span is written by the call: out needs no initialisation; what lies between spans is not touched.
 *   stats  (NULL iff pool_y == NULL: predict only) device double [nfiles][ST_POOL_STATS], with e = y_hat - t over the file's n_out = max(len - (L - y), 0)
 *          output samples:  n_out, sum log cosh e, sum |e|, sum e^2, max |e|, sum t^2, sum y_hat^2, 0.  Per-sample terms and the sums of 256 samples are
 *          float32 (st_ola_loss's formula and tree), everything above that double in ascending row order.  Every row of stats is written by the call (all
 *          zeros for a file without a window): no initialisation.  No float atomics; a repeated call repeats its bits.
 * file_off need not be a multiple of four (such files are read and written sample by sample where a 16-byte access would be misaligned: same values).  Whatever
 * the tables hold, no address outside [0, pool_samples) of the pools and of out is formed (offsets and lengths are clamped, as st_file_feed clamps).
 * ws: st_eval_pool_ws_bytes(d) bytes (>= st_predict_ws_bytes(d); 0 for bad or unsupported dims), 16-byte aligned.
 * Refused before any launch (ST_ERR_ARG, the rule in st_last_error()): bad dims, dims st_eval_pool_supported rejects (= st_predict_supported: the wide
 * autoencoder geometries), a null required pointer (named), an unknown fmt, nfiles < 1, total_rows < 0, pool_samples < 1, stats and pool_y not both null or both
 * given, out and stats both null, out / stats / ws not 16-byte aligned, pools not 16-byte aligned (int16: 8-byte), a batch whose offsets would exceed the
 * kernels' 32-bit element offsets.  total_rows == 0 returns ST_OK and writes only the zero spans and the zero statistics. */
enum { ST_POOL_STATS = 8 };  /* per file: n_out, S logcosh(e), S |e|, S e^2, max |e|, S t^2, S y_hat^2, 0 */
int       st_eval_pool_supported(const st_dims* d);              /* = st_predict_supported */
long long st_eval_pool_rows(const st_dims* d, const long long* file_len_host, int nfiles, long long* win_off_host /* [nfiles+1], may be NULL */);
size_t    st_eval_pool_ws_bytes(const st_dims* d);               /* >= st_predict_ws_bytes(d); 0 for bad / unsupported dims */
int st_eval_pool(const st_dims* d, const float* params, int fmt, const void* pool_x, const void* pool_y /* NULL: predict only */,
                 const long long* file_off, const long long* file_len, const long long* win_off /* device */, int nfiles,
                 long long total_rows, long long pool_samples, const float* file_knobs /* [nfiles][K]; NULL iff K == 0 */,
                 double* stats /* device [nfiles][ST_POOL_STATS]; NULL iff pool_y == NULL */, float* out /* [pool_samples], may be NULL */,
                 void* ws, void* stream);

/* Data-parallel split of st_loss_backward.  After p1 the gradients of the synthesis bases and both
 * autoencoders (grads[offs[2]..end)) are final: all-reduce them while p2 computes the analysis
 * weight gradient (rows [0,F) of tensors 0 and 1) and the loss scalars. */
int st_loss_backward_p1(const st_dims* d, const float* params, float* grads, const float* x, const float* knobs,
                        const float* y_true, void* ws, void* stream);
int st_loss_backward_p2(const st_dims* d, float* grads, const float* x, void* ws, float* scalars, void* stream);
/* p2 with a packed copy of the 2F live analysis rows in `stage` [2F][N] (caller-owned): the buffer the data-parallel
 * all-reduce moves instead of the contiguous range spanning the structurally-zero rows; st_unstage_analysis copies the
 * reduced rows back into grads (rows [0,F) of tensors 0 and 1).  The loss scalars are NOT written here: st_dp_clip_adam
 * publishes them together with the norm of the reduced gradient.  No reference counterpart (see st_loss_backward_stage). */
int st_loss_backward_p2_staged(const st_dims* d, float* grads, float* stage, const float* x, void* ws, float* scalars, void* stream);
int st_unstage_analysis(const st_dims* d, float* grads, const float* stage, void* stream);

/* Finer split of the same step for data parallel (no reference counterpart: train.py:259-263 is a disabled
 * nn.DataParallel stub).  Call stage = 0, 1, 2, 3 in order on one stream; after stage s one gradient range is final
 * and can be all-reduced while the next stage runs:
 *   0  forward (nn_proc.py:304-340) + loss (loss_functions.py:26-36) + synthesis backward -> grads[offs[2], offs[4])
 *   1  autoencoder + polar backward                                                       -> grads[offs[4], total)
 *   2  analysis weight gradient, real basis      (cls_fe_dft.py:50-58 autograd)           -> grads[offs[0], offs[0] + F*N)
 *   3  analysis weight gradient, imaginary basis + loss scalars                           -> grads[offs[1], offs[1] + F*N)
 * Rows >= F of the analysis tensors are structurally zero and never need to move. */
int st_loss_backward_stage(const st_dims* d, const float* params, float* grads, const float* x, const float* knobs,
                           const float* y_true, void* ws, float* scalars, int stage, void* stream);

/* Full single-GPU step: st_loss_backward + L1 clip + Adam (train.py:131-151). */
int st_train_step(const st_dims* d, float* params, float* grads, float* m, float* v, const float* x,
                  const float* knobs, const float* y_true, void* ws, float* scalars,
                  float lr, float beta1, float beta2, float eps, int step, void* stream);

/* ---- the step with frozen parameter groups ------------------------------------------------------------------------------
 * st_train_step for a model some of whose parameters have requires_grad = False (the reference's nn_proc.freeze_layers, nn_proc.py:17-26, and the
 * st_model.freeze() it sketches for the two STFT bases, :395-401), with torch's semantics under clip_grad_norm_ + torch.optim.Adam (train.py:131-151).
 * The 40 tensors form four groups, frozen or trainable as a whole; `trainable` is the OR of the trainable ones. */
#define ST_GROUP_ANALYSIS  1   /* params[offs[0],  offs[2])   dft_analysis  real | imag  */
#define ST_GROUP_SYNTHESIS 2   /* params[offs[2],  offs[4])   dft_synthesis real | imag  */
#define ST_GROUP_AE_MAG    4   /* params[offs[4],  offs[22])  aenc                        */
#define ST_GROUP_AE_PHS    8   /* params[offs[22], total)     phs_aenc                    */
#define ST_GROUP_ALL      15

/* stages of one step, as st_step_groups_stages() reports them */
#define ST_STAGE_SYN_DGRAD  1
#define ST_STAGE_SYN_WGRAD  2
#define ST_STAGE_AE_BWD     4
#define ST_STAGE_AE_DINPUT  8   /* d mag / d phs out of the autoencoder backward + the polar backward */
#define ST_STAGE_ANA_WGRAD 16

/* The backward stages a step with this mask launches (host arithmetic, no state; < 0 for a mask outside 1..15):
 *   SYN_WGRAD  iff SYNTHESIS is trainable;   AE_BWD iff any of AE_MAG, AE_PHS, ANALYSIS is;   SYN_DGRAD iff AE_BWD;
 *   AE_DINPUT and ANA_WGRAD  iff ANALYSIS is trainable.
 * A stage outside the set issues NO launch: neither its GEMM, nor its slab reduce, nor its share of the launch behind the autoencoder backward.  The
 * autoencoder backward, when it runs, runs both nets.  Without AE_DINPUT the fused geometries' autoencoder backward is the instantiation that forms no
 * input gradient (csrc/st_ae.h, NOIN); the split 16-bit backward and the wide path keep forming it, and nothing reads it.  The polar backward runs on no route. */
int st_step_groups_stages(int trainable);

/* Forward, loss and st_dims.prec handling are st_train_step's at every level and geometry.  Frozen groups: their ranges of params, m and v are not
 * written (bit for bit as the caller left them, whatever they hold -- they are not read either); what their ranges of grads hold afterwards is
 * unspecified.  The L1 clip norm runs over the TRAINABLE tensors of the clip scope (the four STFT tensors, or everything with st_dims.clip_all); with
 * none the norm is 0 and the coefficient 1, as clip_grad_norm_ over parameters without gradients.  scalars[3], [4] report exactly that norm and
 * coefficient; scalars[0..2] and [5] are as in st_train_step, and the overflow skip of the f16 levels holds back every trainable group at once.
 * step[g] (g = 0..3, order of the bits): the Adam step number of group g, >= 1 for a trainable group, ignored for a frozen one -- torch's
 * per-parameter state['step']: a group unfrozen after k steps takes its bias corrections from step 1 while the others are at k + 1.
 * ST_ERR_ARG before any launch: trainable outside 1..15, a trainable group with step[g] < 1, a null pointer.  trainable == ST_GROUP_ALL with four
 * equal steps IS st_train_step with that step (same launches, same bits).  Not for the captured step or the data-parallel step. */
int st_train_step_groups(const st_dims* d, float* params, float* grads, float* m, float* v,
                         const float* x, const float* knobs, const float* y_true, void* ws, float* scalars,
                         float lr, float beta1, float beta2, float eps,
                         const int step[4],   /* Adam step number per group, order of the bits above */
                         int trainable, void* stream);

/* After an external all-reduce of `grads` (data parallel): recompute the L1 norm of the reduced, scaled gradient (over the
 * STFT tensors, or over everything with st_dims.clip_all), clip and Adam.  grad_scale = 1/world (the loss scale of
 * st_dims.loss_scale, if any, is removed here as well). */
int st_dp_clip_adam(const st_dims* d, float* params, float* grads, float* m, float* v, void* ws,
                    float* scalars, float grad_scale, float lr, float beta1, float beta2, float eps,
                    int step, void* stream);

/* ---- data parallel inside the library: RCCL over xGMI -------------------------------------------
 * Replaces the reference's disabled nn.DataParallel stub (train.py:259-263) by one process per GPU + an explicit exchange
 * step.  The communicator handle is the only state the library owns; RCCL is bound with dlopen at st_dp_init (a process
 * that already carries librccl -- PyTorch-ROCm does -- shares that copy).
 *   st_dp_unique_id   rank 0: fills 128 bytes; the host hands them to every rank (any bootstrap channel).
 *   st_dp_init        collective over all ranks (ncclCommInitRank); creates the communicator stream and ordering events.
 *   st_dp_allreduce   in-place SUM of n floats on the communicator stream, ordered after the work issued so far on `stream`;
 *                     returns at once, so the caller's next kernels overlap the collective.
 *   st_dp_broadcast   same ordering, root's buffer to all (initial parameters).
 *   st_dp_sync        `stream` waits for every collective issued so far.
 *   st_dp_train_step  one whole data-parallel optimisation step driven from C (no host code between the buckets):
 *                     st_loss_backward_p1 -> all-reduce grads[offs[2]..) || st_loss_backward_p2_staged -> all-reduce the
 *                     packed live analysis rows (`stage`, 2*F*N floats, caller-owned) -> st_unstage_analysis ->
 *                     st_dp_clip_adam(1/world).  p == NULL or world == 1 (and bit 0 of force_exchange clear): plain st_train_step.
 *                     force_exchange is a bit set: 1 = run the exchange even with one rank (tests, overhead measurements);
 *                     2 = split the LAST exchange by basis -- the real rows' all-reduce runs under the weight-gradient GEMM of the imaginary
 *                         rows, so F*N values (2.1 MB) stay exposed instead of 2*F*N;
 *                     4 = the last exchange on bfloat16 values (ncclBfloat16; first half of `stage`), honoured only where the autoencoder
 *                         layers already run in 16 bits (ST_PREC_*_ALL): half the exposed bytes.
 *                     The sum of the synthesis weight-gradient slabs runs on the communicator stream, beside the autoencoder backward
 *                     (round 6: from a slab area of its own, so the analysis weight-gradient GEMM waits for nothing).  Round 6: without bit 1 the
 *                     LAST exchange -- exposed whatever stream it runs on -- is issued in line on `stream` behind one join with the communicator
 *                     stream (recorded behind the last hidden collective): two cross-stream hand-offs of ~10 us each less on the critical path
 *                     (one rank, --force-dp: +44 -> +16 us over the plain step); every rank issues the collectives of the communicator in the same order.
 *   st_dp_rccl_version  ncclGetVersion of the bound library (0 if it exports none): evidence for multi-GPU bench lines. */
typedef struct st_dp st_dp;
int st_dp_unique_id(void* id128);
int st_dp_init(const void* id128, int rank, int world, st_dp** out);
int st_dp_destroy(st_dp* p);
int st_dp_rank(const st_dp* p);
int st_dp_world(const st_dp* p);
int st_dp_rccl_version(const st_dp* p);
int st_dp_allreduce(st_dp* p, float* buf, int64_t n, void* stream);
int st_dp_broadcast(st_dp* p, float* buf, int64_t n, int root, void* stream);
int st_dp_sync(st_dp* p, void* stream);
int st_dp_train_step(st_dp* p, const st_dims* d, float* params, float* grads, float* m, float* v, float* stage,
                     const float* x, const float* knobs, const float* y_true, void* ws, float* scalars,
                     float lr, float beta1, float beta2, float eps, int step, int force_exchange, void* stream);

/* ---- the whole optimisation step as ONE HIP graph -----------------------------------------------------------------------
 * st_graph_create captures st_train_step (every kernel of train.py:112-151) on `stream` -- which must not be the legacy
 * default stream -- with the per-iteration quantities on the device: scalars[6] = step counter (0 before the first step;
 * restore it together with m / v when resuming), scalars[7] = learning rate of the step, looked up by the graph's head
 * node in lr_table (device float[n_lr] = the 1-cycle table, learningrate.py:14-52) as lr_sched[max(i - 1, 0)] for the
 * 0-based iteration i (train.py:150).  The graph reads the minibatch from the x / knobs / y_true buffers it was captured
 * with: refill them before each st_graph_launch.  All pointers must stay valid for the graph's lifetime. */
typedef struct st_graph st_graph;
int st_graph_create(const st_dims* d, float* params, float* grads, float* m, float* v, const float* x,
                    const float* knobs, const float* y_true, void* ws, float* scalars,
                    const float* lr_table, int n_lr, float beta1, float beta2, float eps, void* stream, st_graph** out);
int st_graph_launch(st_graph* g, void* stream);
int st_graph_destroy(st_graph* g);

/* ---- diagnostics: the activations st_model.forward(return_acts=True) returns (nn_proc.py:311-338, plotted by utils/viz.py:135) ----
 * st_workspace_offsets: float offsets, inside a workspace carved for d, of the forward state st_model_fwd(save_for_backward = 1) left:
 *   offs8 = { re, im, mag, phs [B][T][F], mag_hat, phs_hat [B][OT][F], AA [B*OT][KP] (an_real | an_imag halves), y_hat [B][y] }.
 * st_ae_acts: the ten activation tensors of ONE autoencoder (nn_proc.py:77-126 with return_acts), [B][F][width] each, concatenated
 *   (widths 64, 32, 16, 16, 16 + K, 16, 16, 32, 64, OT = st_ae_acts_floats(d) floats); v = its [B][T][F] input, ae = its packed parameters,
 *   sf != 0 for the magnitude net's skip-filter output (nn_proc.py:115), 0 for the phase net's bare output (nn_proc.py:117). */
int st_workspace_offsets(const st_dims* d, int64_t* offs8);
size_t st_ae_acts_floats(const st_dims* d);
int st_ae_acts(const st_dims* d, const float* v, const float* knobs, const float* ae, int sf, float* acts, void* stream);

/* ---- device-side data feed -------------------------------------------------------------------
 * audio.compressor_4controls (signaltrain/audio.py:380-426), the effect of the synthetic comp_4c task
 * (SynthAudioDataSet, datasets.py:312-334), for a batch of device-resident windows:
 *   x [B][L] fp32, knobs_wc [B][4] = (threshold dB, ratio, attack s, release s) in WORLD coordinates
 *   (Effect.knobs_wc, audio.py:455), y [B][ysz] = the last ysz samples of the processed window (datasets.py:327-330). */
int st_compressor_4c(const float* x, const float* knobs_wc, float sr, int B, int L, int ysz, float* y, void* stream);
/* audio.compressor (signaltrain/audio.py:349-371), the effect of the reference's `comp` task (audio.Compressor): a dB envelope
 * (20 log10(|x| + 1e-6)) smoothed by a first-order Butterworth low-pass at 1 / (attackrel sr) of Nyquist, started at its first sample,
 * then the static curve on the smoothed envelope; float64 envelope and gain, y rounded to fp32 (y == x where the envelope stays at or
 * below the threshold).  The envelope is a linear recurrence and runs as a parallel scan in one workgroup per window.
 *   x [B][L] fp32, knobs_wc [B][3] = (threshold dB, ratio, attack / release s) in WORLD coordinates, y [B][ysz] = the last ysz samples. */
int st_compressor(const float* x, const float* knobs_wc, float sr, int B, int L, int ysz, float* y, void* stream);
/* audio.LowPass (signaltrain/audio.py:610-625): scipy's butter(3, cutoff / (sr / 2)) low-pass run by lfilter from a zero state.  The
 * recurrence is linear, so the window is a parallel scan in one workgroup per window -- over the three MODES of the filter (parallel form
 * d + sum r_k / (1 - p_k z^-1) with the poles and residues in closed form from K = tan(pi cutoff / sr)), not over lfilter's direct-form state,
 * whose maps are too ill-conditioned to compose near z = 1 (st_filter.h).  float64 states, y rounded to fp32; within 1e-5 of
 * max(1e-3, max |y|) of scipy's float64 lfilter (measured: 3.5e-7; scipy itself is 7.5e-8 away from a long-double run at 10 Hz).
 *   x [B][L] fp32, knobs_wc [B][1] = the cutoff in Hz (WORLD coordinates), y [B][ysz] = the last ysz samples of the filtered window.
 * Asynchronous, no allocation.  Refused before any launch (ST_ERR_ARG, the rule in st_last_error()): a null pointer; B, L, ysz <= 0; ysz > L;
 * sr <= 0; L % 4.  The cutoff is device data and cannot be checked on the host: a cutoff that is not inside (0, sr / 2), or is NaN, makes that
 * row of y all NaN and nothing else. */
int st_lowpass(const float* x, const float* knobs_wc, float sr, int B, int L, int ysz, float* y, void* stream);
/* audio.Echo (signaltrain/audio.py:539-547 over echo(), :430-443): y = x plus rint(echoes) delayed copies of it, copy i delayed by i * delay samples
 * and scaled by ratio^i.  A fractional delay is the reference's two-tap interpolation: with dl = i * delay in float64, D = floor(dl), diff = dl - D,
 *   y[n] += (float)pow(ratio, i) * ((float)(1 - diff) * x[n - D] + (float)diff * x[n - D - 1]),   x[m] = 0 for m < 0,
 * in float32 with every product and sum rounded on its own -- what numpy computes on a float32 window (audio.echo is the host restatement, bit for
 * bit the reference's under numpy 2).  No recurrence: one workgroup per (window, 2048 samples of the tail), reads of the window through L2.
 *   x [B][L] fp32, knobs_wc [B][3] = (delay in samples, ratio, echoes) in WORLD coordinates, y [B][ysz] = the last ysz samples.  sr is accepted
 *   (the signature is st_lowpass's and st_compressor_4c's) and not used.  Any L: a delayed read is unaligned anyway.
 * Asynchronous, no allocation.  Refused before any launch (ST_ERR_ARG, the rule in st_last_error()): a null pointer; B, L, ysz <= 0; ysz > L.  The
 * knobs are device data and cannot be checked on the host: a delay that is not a finite number >= 1 (the reference raises at 0), rint(echoes)
 * (half to even) outside 0 .. ST_ECHO_MAX, or a NaN knob makes that row of y all NaN and nothing else. */
enum { ST_ECHO_MAX = 8 };
int st_echo(const float* x, const float* knobs_wc, float sr, int B, int L, int ysz, float* y, void* stream);
/* The input of audio.Denoise (signaltrain/audio.py:558-571: the clean signal is the target, the noisy one the input) for callers that bring
 * their own clean windows:  x_noisy[b][n] = x[b][n] + knobs_wc[b] * (2 u - 1),  u = value n of per-sample stream 11 of window
 * first_window + b of the stream `seed` (the counter-based generator of st_synth_effect), the noise formed and added in float32.  The same
 * stream as ST_FX_DENOISE's: identical bits for the same (seed, window, clean x, strength).
 *   x, x_noisy [B][L] fp32 (x_noisy may alias x), knobs_wc [B][1] = the strength (WORLD coordinates).
 * Asynchronous, no allocation.  Refused before any launch (ST_ERR_ARG, the rule in st_last_error()): a null pointer; B, L <= 0; L % 4. */
int st_denoise_input(unsigned seed, unsigned long long first_window, const float* x, const float* knobs_wc, int B, int L, float* x_noisy, void* stream);
/* One training minibatch of the synthetic comp_4c task made on the device in ONE launch (st_feed.h; replaces
 * SynthAudioDataSet.gen_single_chunk, datasets.py:312-334, over audio.synth_input_sample, audio.py:296-334, chooser set
 * {0,1,2,4,6,7}, and compressor_4controls): per window the test signal, knobs = Beta(0.8, 0.8) - 0.5 (audio.py:20-21,
 * datasets.py:325), the target (last ysz samples of the compressed window) and, if `augment`, the random polarity flip of
 * the pair (datasets.py:27-29).  Counter-based generator: window i of the stream `seed` is the same whatever the batching;
 * `first_window` = index of window 0 of this call.  K must be 4; knob_lo / knob_hi = Effect.knob_ranges (host arrays of 4).
 * chooser: -1 = drawn per window (the training feed); 0,1,2,4,6,7 force one signal family (tests).
 * pink_in: optional caller-made [B][L] unit-peak 1/f noise for windows longer than 8192 samples (the in-LDS FFT's limit); NULL: the library makes it --
 * in LDS up to 8192 samples, by its own four-step inverse FFT through `scratch` for powers of two up to 65536 (BASELINE configs[4]'s window), both
 * keyed by (seed, window index) like everything else of the window.
 * scratch: st_synth_comp4c_scratch_floats(B, L) floats (B * (L + 4) up to 8192 samples; may be NULL there): with it (and L % 64 == 0) the effect's
 * sequential attack / release stage runs one LANE per window in a second, tiny launch (64 windows per wave) instead of one workgroup per window --
 * the form that runs beside the training step.
 * Outputs x [B][L], y [B][ysz], knobs [B][4] (fp32, normalised to [-0.5, 0.5]). */
size_t st_synth_comp4c_scratch_floats(int B, int L);
int st_synth_comp4c(unsigned seed, unsigned long long first_window, int B, int L, int ysz, int K, float sr,
                    const float* knob_lo, const float* knob_hi, int augment, int chooser, const float* pink_in,
                    float* x, float* y, float* knobs, float* scratch, void* stream);
/* The same feed for every synthetic effect the library generates on the device; `effect` is an ST_FX_* id, the other arguments are
 * st_synth_comp4c's (which is st_synth_effect(ST_FX_COMP4C, ...) with K == 4):
 *   ST_FX_COMP4C  compressor_4controls, 1 <= K <= 4: knobs with index >= K are fixed at knob_lo[k] (knob_lo / knob_hi always carry 4
 *                 entries) -- e.g. Comp_Just_Thresh (K = 1: threshold, then ratio 3, attack 0.05 s, release 1 s) and Compressor_4c_OneSetting;
 *                 for K == 4 the window stream is st_synth_comp4c's, bit for bit;
 *   ST_FX_COMP    the envelope compressor of st_compressor, K == 3 (threshold, ratio, attack / release s); with scratch (and L % 64 == 0)
 *                 the generator leaves the dB signal there and a second launch runs the envelope scan.
 *   ST_FX_LOWPASS the low-pass of st_lowpass, K == 1 (cutoff Hz): x is the clean window, y the last ysz samples of the filtered one.  The filter is
 *                 odd in x, so the polarity flip is the compressors'.  knob_lo[0] / knob_hi[0] must satisfy 0 < lo <= hi < sr / 2;
 *   ST_FX_DENOISE audio.Denoise (audio.py:558-571), K == 1 (strength): y is the last ysz samples of the CLEAN window and x leaves with the noise
 *                 of st_denoise_input added (the same bits for the same seed, window, clean x and strength).  0 <= lo <= hi is required.
 *   ST_FX_ECHO    audio.Echo (audio.py:539-547), K == 3 (delay in samples, ratio, echoes): x is the clean window, y the last ysz samples of st_echo's
 *                 result.  All three world knobs are float32 Effect.knobs_wc with every step rounded; the delay and the echo count are then rounded to
 *                 integers, half to even, as Echo.go_wc does: st_echo on the feed's x and those knobs reproduces the feed's y bit for bit.  The ranges
 *                 must satisfy rint(lo) >= 1 and lo <= hi (delay), finite lo <= hi (ratio), 0 <= rint(lo), rint(hi) <= ST_ECHO_MAX and lo <= hi (echoes).
 *   ST_FX_DECOMP4C audio.DeCompressor_4c (audio.py:573-583), the inverse problem of ST_FX_COMP4C with its knobs and ranges (1 <= K <= 4): y is the last
 *                 ysz samples of the CLEAN window and x leaves as compressor_4controls of the clean window over all L samples -- bit for bit
 *                 st_compressor_4c(clean x, the window's world knobs, ysz = L), and its tail ST_FX_COMP4C's y.  With scratch (ST_FX_COMP4C's size, and
 *                 L % 64 == 0) the attack / release stage runs one lane per window and a third launch applies the gain over the whole of x; the two forms
 *                 agree bit for bit.
 * Both are odd in x like the others, so the polarity flip of the pair stays where it is.
 * The window's draws do not depend on the effect: all four knob draws are made whatever K is, so the clean signal of window w of the stream `seed`
 * is, bit for bit, the x ST_FX_COMP4C produces for the same (seed, w, chooser, augment).  ST_FX_LOWPASS, ST_FX_DENOISE and ST_FX_ECHO have no second-launch
 * form: st_synth_effect_scratch_floats answers for them only what the 1/f noise of windows beyond 8192 samples needs (0 up to 8192 samples,
 * where scratch may be NULL).  Their world knob is lo + (knob + 0.5) * (hi - lo) in float32 with every step rounded (what Effect.knobs_wc gives
 * in float32): st_lowpass / st_denoise_input on the feed's x (clean x) and that knob reproduce the feed's y (x) bit for bit.
 * Every window is a function of (seed, window index) only; knobs [B][K].  Wrong ids, knob counts and (for the two one-knob effects and ST_FX_ECHO; the ranges
 * are host arrays) knob ranges are refused before any launch (ST_ERR_ARG, the rule in st_last_error()). */
enum { ST_FX_COMP4C = 0, ST_FX_COMP = 1, ST_FX_LOWPASS = 2, ST_FX_DENOISE = 3, ST_FX_ECHO = 4, ST_FX_DECOMP4C = 5 };
size_t st_synth_effect_scratch_floats(int effect, int B, int L);
int st_synth_effect(int effect, unsigned seed, unsigned long long first_window, int B, int L, int ysz, int K, float sr,
                    const float* knob_lo, const float* knob_hi, int augment, int chooser, const float* pink_in,
                    float* x, float* y, float* knobs, float* scratch, void* stream);
/* st_synth_effect over a caller-chosen set of signal families: all twelve of audio.synth_input_sample (audio.py:296-334) are built -- beyond the
 * compressor's set 3 (triangle + 1/f noise), 5 (spikes + normal noise), 8 (ampexpstepup from -30 dB), 9 (frequency sweep), 10 (box + white + 1/f
 * noise) and 11 (scaled 1/f noise); the datasets of the reference use e.g. {0,1,3,4,6,10,2,7,9} and {1,3,5,6,7} (datasets.py:317-320).
 *   family_mask   bit f allows family f, f in 0..11.  With ST_FAMILIES_COMPRESSOR the call IS st_synth_effect: the same kernel, the same bits.
 *   chooser       -1: per window a uniform member of the set (the draw law is written out in st_feed.h; datasets.synth_feed_draw replicates the
 *                 part of it the new families use); 0..11 force one family whatever the mask holds, 100 is the bare 1/f noise (tests).
 * The other arguments, the effects, the scratch and the long-window rules are st_synth_effect's; a window stays a function of (seed, window index,
 * family set) only, and its knobs, polarity and the signals of the compressor's families do not depend on the set.  Refused before any launch
 * (ST_ERR_ARG, the rule in st_last_error()): an empty mask; bits >= 12; a forced family outside 0..11 / 100 -- the superposition of two signals
 * (chooser >= 12 in the reference, which none of its datasets draws) is not built -- and everything st_synth_effect refuses. */
enum { ST_FAMILIES_COMPRESSOR = 0xD7, ST_FAMILIES_ALL = 0xFFF };
int st_synth_effect_families(int effect, unsigned family_mask, unsigned seed, unsigned long long first_window, int B, int L, int ysz, int K, float sr,
                             const float* knob_lo, const float* knob_hi, int augment, int chooser, const float* pink_in,
                             float* x, float* y, float* knobs, float* scratch, void* stream);

/* One training minibatch of RECORDED input / target pairs cut out of device-resident audio in ONE launch (st_feed_files.h; replaces
 * AudioFileDataSet.get_single_chunk, datasets.py:225-253).  pool_x / pool_y hold all files concatenated (float32, or the int16 of the wav
 * files: fmt), file f at samples [file_off[f], file_off[f] + file_len[f]).  Window b of the call is window w = first_window + b of the stream
 * `seed`, a function of (seed, w) only, with integer draws (the law is written out in st_feed_files.h; datasets.file_feed_draw replicates it):
 * a file uniformly over the files, a start uniformly in [0, len - L), and with `augment` one polarity flip of the pair.
 *   x [B][L] = the window of pool_x, y [B][ysz] = the last ysz samples of the same span of pool_y (NULL: not made),
 *   knobs [B][K] = the file's row of file_knobs [nfiles][K] (normalised settings; K == 0: both NULL), meta [B][3] = (file, start, flipped), or NULL.
 * ST_PCM_S16 samples convert as (float)((double)s / 32767.0): a window out of the int16 pool equals the one out of the float32 pool bit for bit.
 * min_len: the smallest file length, pool_samples: the pool's length (host values).  Refused before any launch (ST_ERR_ARG, the rule in
 * st_last_error()): a null required pointer; B, L, ysz, nfiles <= 0; ysz > L; L % 4 or ysz % 4; K outside [0, 16]; file_knobs == NULL with K > 0
 * (or not NULL with K == 0); an unknown fmt; min_len <= L; pool_samples < min_len.  No address outside the pools is formed even from wrong tables. */
enum { ST_PCM_F32 = 0, ST_PCM_S16 = 1 };
int st_file_feed(unsigned seed, unsigned long long first_window, int B, int L, int ysz, int K, int fmt,
                 const void* pool_x, const void* pool_y, const long long* file_off, const long long* file_len, int nfiles,
                 long long min_len, long long pool_samples, const float* file_knobs, int augment,
                 float* x, float* y, float* knobs, long long* meta, void* stream);

/* One training minibatch of RECORDED input through a LIVE effect (st_feed_live.h): per window a span of st_file_feed's audio pool (pool_x, file_off,
 * file_len, nfiles, min_len, pool_samples and fmt as there; no target pool), knobs drawn for that window, and the effect `effect` (an ST_FX_* id; K, knob_lo /
 * knob_hi, sr, ysz as st_synth_effect) applied on the spot.  Window b of the call is window w = first_window + b of the stream `seed`; its four scalar
 * draws -- the law is written out in st_feed_live.h, datasets.live_feed_draw replicates it -- decide
 *   synthetic  with probability synth_prob (0: never, 1: always): the row is then, bit for bit, row w of st_synth_effect_families(effect, family_mask, seed, ...);
 *   file, start, flipped   else: x = +-pool_x[file_off[file] + start .. + L) (minus where `augment` and flipped; no 1e-8 noise, no random polarity),
 *              knobs = Beta(0.8, 0.8) - 0.5 per window, y / x by the effect as in st_synth_effect (ST_FX_DENOISE, ST_FX_DECOMP4C: y is the clean tail and x
 *              leaves with the noise on it / compressed), so the library's effect entries on (x, world knobs) reproduce the row.
 * x [B][L], y [B][ysz], knobs [B][K]; meta [B][4] = (synthetic, file, start, flipped) of every window, or NULL.  Every row is a function of (seed, w) and
 * the pool only, whatever the batching and the other rows.  scratch: st_live_feed_scratch_floats(effect, B, L, synth_prob) floats, or NULL.  With it
 * (and L % 64 == 0) the compressor effects run their sequential stage through the scratch, as st_synth_effect does, with the same bits as without:
 * [gain curve or dB signal B * L | world knobs 4 B] are left there.  With synth_prob == 0 no synthetic kernel is launched and no window length needs a
 * scratch; with synth_prob > 0 the scratch is st_synth_effect_scratch_floats(effect, B, L) and windows beyond 8192 samples require it.
 * Refused before any launch (ST_ERR_ARG, the rule in st_last_error()): everything st_synth_effect refuses about the effect, K, the knob ranges and the
 * sizes; everything st_file_feed refuses about the pool (fmt, nfiles, min_len <= L, pool_samples < min_len, null tables, L % 4, ysz % 4); synth_prob outside
 * [0, 1] or NaN; and with synth_prob > 0 what st_synth_effect_families refuses about family_mask.  No address outside the pool is formed even from wrong tables. */
size_t st_live_feed_scratch_floats(int effect, int B, int L, float synth_prob);
int st_live_feed(int effect, unsigned family_mask, float synth_prob, unsigned seed, unsigned long long first_window,
                 int B, int L, int ysz, int K, float sr, const float* knob_lo, const float* knob_hi, int augment,
                 int fmt, const void* pool_x, const long long* file_off, const long long* file_len, int nfiles,
                 long long min_len, long long pool_samples,
                 float* x, float* y, float* knobs, long long* meta /* [B][4] kind, file, start, flipped; may be NULL */,
                 float* scratch, void* stream);

/* st_live_feed with the effect's HISTORY: the streamed target (st_feed_stream.h, where the law is written out).  Every argument of st_live_feed keeps its
 * meaning and every window its draws, knobs, world knobs and meta.  For a recorded window the effect runs over up to `preroll` samples of the window's own
 * file in front of it, the pre-roll, and only the window and the effect's tail leave:
 *   R  = min(preroll, start & ~3)      (start: meta[2]; preroll % 4 == 0; at most three samples at a file's head stay out of the history)
 *   xe = +-pool_x[file_off[file] + start - R .. + R + L)   (the flip covers the whole span),   x = xe[R:]
 *   y  = the last ysz samples of st_compressor_4c / st_compressor / st_lowpass / st_echo on (xe, the window's world knobs), bit for bit;
 *   ST_FX_DENOISE: st_live_feed's row (no state; the noise index is relative to the window);  ST_FX_DECOMP4C: y is the clean tail, x the last L samples of
 *   st_compressor_4c(xe).
 * With a pre-roll that reaches the head of the file, y is the streamed render of the file at the window's knob setting.  A synthetic row (synth_prob > 0) has
 * no history: st_live_feed's row.  A recorded row depends on (seed, w), the pool and preroll only.
 * How a state forgets its start: the 4-control compressor's gain in dB contracts by max(alphaA, alphaR)^n, alpha = exp(-ln 9 / (sr T)), so n ~ 7.6 T sr samples
 * bring a difference down to 2^-24 of its start (T = 1 s at 44.1 kHz, Comp_Just_Thresh's release: 335 000 samples).  ST_LIVE_PREROLL_MAX = 2^22 samples is
 * twelve times that (95 s at 44.1 kHz) and keeps preroll + L, every row index, inside 32 bits.
 * preroll == 0: the call IS st_live_feed (same launches, same scratch contract, same size).  preroll > 0: scratch is REQUIRED,
 * st_live_feed_stream_scratch_floats(effect, B, L, preroll, synth_prob) floats, and on return holds, with P = round_up(preroll + L, 64):
 *   [ world knobs [B][4] (recorded rows) | R per row as int32, -1 for a synthetic row, round_up(B, 4) words |
 *     B * P floats (not for ST_FX_DENOISE), rows right-aligned: ST_FX_COMP / LOWPASS / ECHO the float image of xe, ST_FX_COMP4C / DECOMP4C its gain curve,
 *     smoothed over the samples that were applied | st_live_feed's scratch, st_live_feed_scratch_floats(effect, B, L, synth_prob) floats, when synth_prob > 0 ]
 * Refused before any launch (ST_ERR_ARG, the rule in st_last_error()): everything st_live_feed refuses; preroll < 0; preroll % 4 != 0; preroll >
 * ST_LIVE_PREROLL_MAX; a NULL scratch with preroll > 0; preroll + L >= 2^31 - 64 or B * P >= 2^40 elements (the offsets are 64-bit, a row index 32-bit).
 * The size function returns 0 for such arguments.  Asynchronous, no allocation, no host sync. */
enum { ST_LIVE_PREROLL_MAX = 1 << 22 };
size_t st_live_feed_stream_scratch_floats(int effect, int B, int L, int preroll, float synth_prob);
int st_live_feed_stream(int effect, unsigned family_mask, float synth_prob, int preroll, unsigned seed, unsigned long long first_window,
                        int B, int L, int ysz, int K, float sr, const float* knob_lo, const float* knob_hi, int augment,
                        int fmt, const void* pool_x, const long long* file_off, const long long* file_len, int nfiles,
                        long long min_len, long long pool_samples,
                        float* x, float* y, float* knobs, long long* meta, float* scratch, void* stream);

/* ---- a folder of recordings through an effect in one call: st_render_pool (csrc/st_render_pool.h) --------------------------------
 * gen_dataset.py's step: every file of the folder WHOLE through the effect `effect` (an ST_FX_* id) at ONE knob setting per file.  The folder is the pool of
 * st_file_feed / st_eval_pool: fmt, pool_x, file_off / file_len (device int64, in samples), pool_samples.  knobs_wc: device [nfiles][4], WORLD coordinates in the
 * order of the effect's entry (4-control compressor: threshold dB, ratio, attack s, release s; ST_FX_COMP: threshold, ratio, attack / release s; ST_FX_LOWPASS:
 * cutoff Hz; ST_FX_ECHO: delay in samples, ratio, echoes; ST_FX_DENOISE: strength); entries past the effect's count are not read.
 * THE LAW.  For file f, after the offset and length clamps st_eval_pool applies (and len <= max_len), let xe be the float32 image of pool_x[file_off[f] .. + len)
 * (ST_PCM_S16 converts as in st_file_feed) and len' = len rounded up to the multiple the effect's own entry demands, zeros appended.  Then out[file_off[f] + n],
 * n in [0, len), is bit for bit sample n of
 *   ST_FX_COMP4C    st_compressor_4c(xe, row f of knobs_wc, B = 1, L = ysz = len')        ST_FX_COMP     st_compressor(...), same arguments
 *   ST_FX_LOWPASS   st_lowpass(...)                                                        ST_FX_ECHO     st_echo(...)
 *   ST_FX_DENOISE   st_denoise_input(seed, first_file + f, xe, strength, 1, len') -- the noisy input; the target is the pool itself
 *   ST_FX_DECOMP4C  as ST_FX_COMP4C -- the compressed input; the target is the pool itself
 * seed / first_file: ST_FX_DENOISE only (file f is window first_file + f of the noise stream `seed`), ignored otherwise.
 * Every sample of out inside a file's span is written; what lies between spans is not touched; a file of length 0 writes nothing.  The per-row NaN rules of the
 * entries carry over per file: a cutoff outside (0, sr / 2) or an echo count outside 0 .. ST_ECHO_MAX makes that file's span NaN and nothing else.  file_off need
 * not be a multiple of four.  Whatever the tables hold, no address outside [0, pool_samples) of the pool or of out is formed.  max_len: the longest file (host
 * value); a longer device length is cut to it.
 * scratch: st_render_pool_scratch_floats(effect, file_len_host, nfiles) floats, 16-byte aligned; its layout is the library's own ([per-file row offsets, built on
 * the device from file_len | one row of round_up(len, 64) floats per file]; sized from the HOST lengths, which the device lengths must not exceed).  The size is 0
 * for ST_FX_DENOISE (scratch may be NULL) and for bad arguments: a null table, nfiles < 1, a length < 0 or >= 2^31 - 64, an unknown effect.
 * The 4-control compressor's attack / release chain is sequential per file: it runs one lane per file, 64 files per wave, each wave to the longest of its files.
 * Asynchronous; no allocation, no hipMemcpy, no host synchronisation, no float atomics: a repeated call repeats its bits.
 * Refused before any launch (ST_ERR_ARG, the rule in st_last_error()): a null required pointer (named); an unknown effect or fmt; nfiles < 1; pool_samples < 1;
 * max_len < 0 or >= 2^31 - 64; sr <= 0; out or scratch not 16-byte aligned; pool_x not 16-byte aligned (int16: 8-byte); a null scratch where the size function
 * is non-zero. */
size_t st_render_pool_scratch_floats(int effect, const long long* file_len_host, int nfiles);   /* 0 for bad arguments */
int st_render_pool(int effect, float sr, int fmt, const void* pool_x,
                   const long long* file_off, const long long* file_len /* device int64 */, int nfiles,
                   long long max_len /* host: the longest file */, long long pool_samples,
                   const float* knobs_wc /* device [nfiles][4], world coordinates */,
                   unsigned seed, unsigned long long first_file /* ST_FX_DENOISE only */,
                   float* out /* [pool_samples] float32 */, float* scratch, void* stream);

/* Gradient of the loss w.r.t. the (halved) input waveform, for callers with something trainable upstream of the model (the reference's
 * autograd provides it; nn_proc.py:307, cls_fe_dft.py:55-56).  Call right after st_model_bwd on the SAME workspace:
 *   gxh[b][n] = conv-transpose of the analysis output gradient with both bases, cropped by the Conv1d padding   [B][L]
 * The caller multiplies by 1/2 (nn_proc.py:307) and adds g_y_hat on the last y samples (the skip of nn_proc.py:340).
 * scratch: st_model_input_grad_ws_floats(d) floats. */
size_t st_model_input_grad_ws_floats(const st_dims* d);
int st_model_input_grad(const st_dims* d, const float* params, void* ws, float* scratch, float* gxh, void* stream);

/* Gradient w.r.t. the knob settings for arbitrary upstream gradients (same meaning as st_model_bwd's): what the reference's autograd hands to a
 * knobs tensor that requires grad -- nn_proc.py:92-93 repeats the settings over the rows of a window and concatenates them in front of
 * fnn_addknobs of both autoencoders (nn_proc.py:332-333).  g_knobs [B][K].  The exact, SLOW route: one forward + backward per window, whose
 * fnn_addknobs bias gradients are that window's row sums of d a5; the reference's training never asks for this gradient (knobs are data), so
 * the training step's kernels carry nothing for it (st_model_bwd_knobs below is the opt-in one-pass form).  grads_scratch: st_param_offsets() floats, overwritten.  The saved-for-backward state of `ws` belongs
 * to the last window afterwards: run st_model_fwd(save_for_backward = 1) again before st_model_bwd.  The per-window passes run in the arithmetic of
 * d->prec like the batch itself (round 5: a single window takes 16-bit layers on every geometry, st_effective_prec). */
int st_model_knob_grad(const st_dims* d, const float* params, float* grads_scratch, const float* x, const float* knobs,
                       const float* g_y_hat, const float* g_mag_hat, const float* g_mag, void* ws, float* g_knobs, void* stream);

/* The same gradient in ONE backward pass of the batch (opt-in; st_model_knob_grad above stays the exact reference route and the fallback).
 * st_model_bwd_knobs is st_model_bwd -- same contract: asynchronous, no allocation, no host sync, same meaning of the upstream gradients, `grads`
 * receives exactly what st_model_bwd writes, bit for bit -- and in the same pass g_knobs[B][K]: the autoencoder backward kernel that holds d a5 (the
 * gradient at fnn_addknobs' pre-activation, fp32 also with 16-bit layers) also stores its column sums per 16-row group (a group never straddles a
 * window) into `scratch` ([net][group][16] floats), and one small launch, one workgroup per window, sums a window's groups in ascending order
 * (bit-repeatable) and applies the fp32 W5 of both nets.  Call it where st_model_bwd would be called, after st_model_fwd(save_for_backward = 1); the
 * saved-for-backward state of `ws` is still that of the batch afterwards.  scratch: st_model_bwd_knobs_ws_floats(d) floats of the caller's, every
 * element read is written by the same call (no clearing); st_workspace_bytes does not change.
 * Refusals, before any launch, with the rule in st_last_error(): dims outside the family, a null pointer, K < 1 (ST_ERR_ARG); ST_ERR_UNSUPPORTED where
 * a diagnostic switch away from its default (st_set_tuning 8000 / 8001 / 8200) routes the autoencoder backward to a kernel form that has no per-group
 * output -- st_knob_grad_fused_supported (host only, no device work) then answers 0, as it does for K == 0 and for bad dims. */
int    st_knob_grad_fused_supported(const st_dims* d);
size_t st_model_bwd_knobs_ws_floats(const st_dims* d);      /* 2 nets x B x (KP/32) groups x 16 floats; 0 for bad dims */
int    st_model_bwd_knobs(const st_dims* d, const float* params, float* grads, const float* x, const float* knobs,
                          const float* g_y_hat, const float* g_mag_hat, const float* g_mag, void* ws, float* scratch, float* g_knobs, void* stream);

/* ---- generic learned-basis front end: SURVEY.md row a15, signaltrain/cls_fe_dct_bases.py ------------------------------
 * Analysis.forward (:129-136)  = Conv1d(1 -> C, kernel KW, stride hop, padding pad, bias) transposed to [B][T][C];
 * Synthesis.forward (:174-179) = ConvTranspose1d(C -> 1, kernel KW, stride hop) with `crop` samples cut from both ends.
 * W is the [C][1][KW] Conv weight seen as [C][KW].  T = st_fe_frames(L, KW, hop, pad).  The *_bwd entries are the
 * autograd of the forward ones (weight, bias and input gradients).  ws: st_fe_ws_floats() floats (for synthesis pass
 * L = the output length (T - 1) * hop + KW - 2 * crop and pad = crop, i.e. call it with the analysis geometry of the same model).
 * Every entry refuses a shape st_fe_supported() refuses with ST_ERR_ARG and a message that names the limit, before any launch; st_fe_ws_floats()
 * then returns 0. */
int st_fe_frames(int L, int KW, int hop, int pad);
/* Host only (no device work): 1 if the front-end kernels may run this shape, else 0.  The rules: positive sizes, KW%16, C%16, hop%4, pad%4, L%4 and at least
 * one frame (KW <= L + 2 pad); rows B * T and samples L + 2 pad + 2 KW below 2^24 (24-bit multiplies); B * L, B * (L + 2 pad + 2 KW), B * T * KW, B * T * C
 * and C * KW below 2^30 elements (32-bit element offsets); and (B * T - 1) * T < 2^32, up to where the kernels' division of a row index r < B * T by T through
 * a multiply-high with floor(2^32 / T) + 1 is exact (the same rule st_fm_div_exact states for the frame-major order).  The synthesis entries apply it with
 * L = (T - 1) * hop + KW - 2 * crop and pad = crop. */
int st_fe_supported(int B, int L, int C, int KW, int hop, int pad);
size_t st_fe_ws_floats(int B, int L, int C, int KW, int hop, int pad);
int st_fe_analysis_fwd(const float* x, int B, int L, const float* W, const float* bias, int C, int KW, int hop, int pad,
                       float* out, void* stream);
int st_fe_synthesis_fwd(const float* xft, int B, int T, const float* W, int C, int KW, int hop, int crop,
                        float* ws, float* out, void* stream);
int st_fe_analysis_bwd(const float* x, int B, int L, const float* W, int C, int KW, int hop, int pad, const float* g_out,
                       float* ws, float* gW, float* gbias, float* gx, void* stream);
int st_fe_synthesis_bwd(const float* xft, int B, int T, const float* W, int C, int KW, int hop, int crop, const float* g_wave,
                        float* ws, float* gW, float* g_xft, void* stream);

#ifdef __cplusplus
}
#endif
#endif
