"""Round 10, host side: the ready-made LDS weight images prep_kernel builds (csrc/st_ae.h ae_img_build, one float per thread, gathered) are, float for float, what
the in-kernel build leaves in LDS (ae_params_issue + zero fill + ae_params_scatter).  Both are plain index arithmetic, compiled here for the CPU: a small program
runs the scatter for every thread of a 256-thread (backward) and a 704-thread (forward) workgroup into zeroed arrays, runs the gather over a block poisoned with NaN
bit patterns, and compares bytes -- forward images and biases of both nets, the frequency-weight table, the data-gradient images of both nets.
Also on the host: the scatter into the two compact layouts of the split backward (st_ae_split.h CP<1>, CP<2>) against the matching regions of the full-layout
scatter, with the 256 and 512 threads of the backward kernels, and the workgroup store pass (ae_partials_store) against a plain loop over (layer, o, i).
The layer shapes are typed out here on purpose: this file is the independent statement of the table in st_ae.h.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r'''
#include <stdio.h>
#include <string.h>
#include <vector>
#include "st_ae_split.h"
using namespace sta;

template <int NT>
static void scatter_all(float* lds, const AETab& tab, const float* ae, const AEOffsets& go, int T, int OT, int K, bool dgrad, int l0 = 0, int l1 = NL)
{
    for (int tid = 0; tid < NT; ++tid) {
        AEParamRegs<NT> r;
        ae_params_issue<NT>(r, ae, go, T, OT, K, tid, l0, l1);
        ae_params_scatter<NT, 0>(lds, tab, r, T, OT, K, tid, l0, l1, dgrad);
    }
}
// (a) the scatter into a compact layout is, region by region, the full-layout scatter: forward images, biases, dgrad images of the layers [l0, l1)
template <int NT, int PART>
static int compact_case(const float* ae, const AEOffsets& go, int T, int OT, int K, const std::vector<float>& full)
{
    typedef CP<PART> P;
    const int l0 = P::L0, l1 = P::L1;
    const int outp[NL] = {64, 32, 16, 16, 16, 16, 32, 64, 16}, inp[NL] = {32, 64, 32, 16, 32, 16, 16, 32, 64};
    int nw = 0, nb = 0;
    for (int l = l0; l < l1; ++l) { nw += outp[l] * inp[l]; nb += outp[l]; }
    if (P::TOTAL != 2 * nw + nb || P::FWD_END != nw + nb) { printf("CP<%d>: sizes differ from the sum over its layers\n", PART); return 1; }
    std::vector<float> c(P::TOTAL + 64, 0.f);
    memset(c.data() + P::TOTAL, 0xFF, 64 * sizeof(float));
    scatter_all<NT>(c.data(), P::tab(), ae, go, T, OT, K, true, l0, l1);
    for (int i = P::TOTAL; i < P::TOTAL + 64; ++i) { unsigned u; memcpy(&u, &c[i], 4); if (u != 0xFFFFFFFFu) { printf("CP<%d>: written past the layout\n", PART); return 1; } }
    const int a0[NL] = {CL::A0, CL::A1, CL::A2, CL::A3, CL::A4, CL::A5, CL::A6, CL::A7, CL::A8}, b0[NL] = {CL::B0, CL::B1, CL::B2, CL::B3, CL::B4, CL::B5, CL::B6, CL::B7, CL::B8};
    if (memcmp(c.data(), full.data() + a0[l0], nw * sizeof(float)) || memcmp(c.data() + nw, full.data() + b0[l0], nb * sizeof(float)) ||
        memcmp(c.data() + nw + nb, full.data() + CL::G0 + a0[l0], nw * sizeof(float))) {
        printf("T=%d OT=%d K=%d NT=%d: the compact scatter of CP<%d> differs from the full one\n", T, OT, K, NT, PART); return 1;
    }
    return 0;
}
// (b) the store pass over four images of distinct values against a plain loop: exactly PG floats, (0 + 1) + (2 + 3), pads zero
template <int NT>
static int store_case(const AETab& tab, int stride, const AEOffsets& go, int PG, int T, int OT, int K, int l0, int l1, unsigned have, const char* what)
{
    const int out[NL] = {64, 32, 16, 16, 16, 16, 32, 64, OT}, in[NL] = {T, 64, 32, 16, 16 + K, 16, 16, 32, 64};
    const int inp[NL] = {32, 64, 32, 16, 32, 16, 16, 32, 64};
    std::vector<float> lds(4 * stride);
    for (int i = 0; i < 4 * stride; ++i) lds[i] = (float)(i % 8191) * 0.37f + (float)(i / stride) * 1e-3f + 1.0f;
    std::vector<float> got(PG + 64), want(PG, 0.f);
    memset(got.data(), 0xFF, got.size() * sizeof(float));
    for (int tid = 0; tid < NT; ++tid) ae_partials_store<NT>(got.data(), lds.data(), stride, tab, go, PG, T, OT, K, tid, l0, l1, have);
    std::vector<char> mine(PG, 0);
    for (int l = l0; l < l1; ++l) {
        const int bend = l + 1 < NL ? go.w[l + 1] : PG;
        for (int e = go.w[l]; e < bend; ++e) mine[e] = 1;                      // the tensors of the layer and the pads behind them
        if (!((have >> l) & 1)) continue;
        for (int o = 0; o < out[l]; ++o)
            for (int i = 0; i < in[l]; ++i) {
                const int x = tab.ao[l] + o * inp[l] + i;
                want[go.w[l] + o * in[l] + i] = (lds[x] + lds[stride + x]) + (lds[2 * stride + x] + lds[3 * stride + x]);
            }
        for (int o = 0; o < out[l]; ++o) { const int x = tab.bo[l] + o; want[go.b[l] + o] = (lds[x] + lds[stride + x]) + (lds[2 * stride + x] + lds[3 * stride + x]); }
    }
    for (int e = 0; e < PG + 64; ++e) {
        unsigned u; memcpy(&u, &got[e], 4);
        const bool untouched = u == 0xFFFFFFFFu;
        if (e >= PG || !mine[e]) { if (!untouched) { printf("%s T=%d OT=%d K=%d: float %d written outside the layers' block\n", what, T, OT, K, e); return 1; } }
        else if (untouched || memcmp(&got[e], &want[e], 4)) { printf("%s T=%d OT=%d K=%d: float %d differs\n", what, T, OT, K, e); return 1; }
    }
    return 0;
}
static int run_case(int T, int OT, int K, int F)
{
    const int out[NL] = {64, 32, 16, 16, 16, 16, 32, 64, OT}, in[NL] = {T, 64, 32, 16, 16 + K, 16, 16, 32, 64};
    AEOffsets go; int off = 0;
    for (int l = 0; l < NL; ++l) { go.w[l] = off; off += (out[l] * in[l] + 3) / 4 * 4; go.b[l] = off; off += (out[l] + 3) / 4 * 4; }      // st_param_offsets: 4-float alignment
    const int PG = off, FP = (F + 15) / 16 * 16;
    std::vector<float> ae[2];
    unsigned s = 12345u + 977u * (unsigned)(T + 32 * OT + 1024 * K);
    for (int a = 0; a < 2; ++a) { ae[a].resize(PG); for (int i = 0; i < PG; ++i) { s = s * 1664525u + 1013904223u; ae[a][i] = (float)(int)(s >> 8) * (1.0f / 8388608.0f) - 1.0f + 1e-3f; } }
    std::vector<float> lf(2 * CL::FWD_TOTAL, 0.f), lb[2];
    scatter_all<704>(lf.data(), CL::tab(), ae[0].data(), go, T, OT, K, false);
    scatter_all<704>(lf.data() + CL::FWD_TOTAL, CL::tab(), ae[1].data(), go, T, OT, K, false);
    for (int a = 0; a < 2; ++a) { lb[a].assign(CL::BWD_TOTAL, 0.f); scatter_all<256>(lb[a].data(), CL::tab(), ae[a].data(), go, T, OT, K, true); }
    const int n = ae_img_floats(FP);
    std::vector<float> img(n + 64);
    memset(img.data(), 0xFF, img.size() * sizeof(float));
    AEImgJob j; j.ae[0] = ae[0].data(); j.ae[1] = ae[1].data(); j.img = img.data(); j.go = go; j.T = T; j.OT = OT; j.K = K; j.F = F; j.FP = FP; j.expfac = (float)(7.0 / F);
    j.n = n; j.n_blk = (n + 255) / 256;
    for (int p = 0; p < j.n_blk * 256; ++p) ae_img_build(j, p);
    int bad = 0;
    for (int i = n; i < n + 64; ++i) { unsigned u; memcpy(&u, &img[i], 4); bad += u != 0xFFFFFFFFu; }                       // nothing written past the block
    if (bad) { printf("T=%d OT=%d K=%d F=%d: %d floats written past the block\n", T, OT, K, F, bad); return 1; }
    if (memcmp(img.data(), lf.data(), 2 * CL::FWD_TOTAL * sizeof(float))) { printf("T=%d OT=%d K=%d F=%d: forward images differ\n", T, OT, K, F); return 1; }
    for (int i = 0; i < FP; ++i) { const float w = i < F ? ae_freq_weight(j.expfac, i) : 0.f; if (memcmp(&w, &img[2 * CL::FWD_TOTAL + i], 4)) { printf("table entry %d differs\n", i); return 1; } }
    for (int a = 0; a < 2; ++a) {
        if (memcmp(lb[a].data(), lf.data() + a * CL::FWD_TOTAL, CL::FWD_TOTAL * sizeof(float))) { printf("net %d: the 256- and 704-thread scatters disagree\n", a); return 1; }
        if (memcmp(img.data() + 2 * CL::FWD_TOTAL + FP + a * AE_IMG_DG, lb[a].data() + CL::G0, AE_IMG_DG * sizeof(float))) { printf("T=%d OT=%d K=%d F=%d: dgrad images of net %d differ\n", T, OT, K, F, a); return 1; }
    }
    for (int a = 0; a < 2; ++a)
        if (compact_case<256, 1>(ae[a].data(), go, T, OT, K, lb[a]) || compact_case<256, 2>(ae[a].data(), go, T, OT, K, lb[a]) ||
            compact_case<512, 1>(ae[a].data(), go, T, OT, K, lb[a]) || compact_case<512, 2>(ae[a].data(), go, T, OT, K, lb[a])) return 1;
    const unsigned all = 0x1FFu;      // one bit per layer
    if (store_case<256>(CL::tab(), CL::FWD_TOTAL, go, PG, T, OT, K, 0, NL, all, "ae_bwd") ||
        store_case<256>(CL::tab(), CL::FWD_TOTAL, go, PG, T, OT, K, 0, NL, 0x0FEu, "ae_bwd INNER") ||
        store_case<512>(CP<1>::tab(), CP<1>::FWD_END, go, PG, T, OT, K, CP<1>::L0, CP<1>::L1, all, "ae_bwd_part 1") ||
        store_case<512>(CP<2>::tab(), CP<2>::FWD_END, go, PG, T, OT, K, CP<2>::L0, CP<2>::L1, all, "ae_bwd_part 2")) return 1;
    return 0;
}
int main()
{
    const int cases[][4] = {{25, 9, 4, 513}, {25, 9, 0, 513}, {25, 9, 2, 513}, {11, 6, 4, 513}, {32, 16, 16, 129}, {1, 1, 1, 17}, {24, 8, 3, 49}, {16, 16, 5, 81}, {4, 4, 4, 129}};
    for (const auto& c : cases) if (run_case(c[0], c[1], c[2], c[3])) return 1;
    printf("ok %d\n", (int)(sizeof(cases) / sizeof(cases[0])));
    return 0;
}
'''


def test_gathered_images_equal_the_scattered_ones_on_the_host(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.isfile(hipcc):
        pytest.skip("no hipcc")
    src = tmp_path / "ae_images_host.hip"
    src.write_text(PROG)
    exe = tmp_path / "ae_images_host"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "signaltrain_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok 9", (r.returncode, r.stdout[-1000:], r.stderr[-500:])
