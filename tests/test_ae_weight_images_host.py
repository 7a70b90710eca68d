"""Round 10, host side: the ready-made LDS weight images prep_kernel builds (csrc/st_ae.h ae_img_build, one float per thread, gathered) are, float for float, what
the in-kernel build leaves in LDS (ae_params_issue + zero fill + ae_params_scatter).  Both are plain index arithmetic, compiled here for the CPU: a small program
runs the scatter for every thread of a 256-thread (backward) and a 704-thread (forward) workgroup into zeroed arrays, runs the gather over a block poisoned with NaN
bit patterns, and compares bytes -- forward images and biases of both nets, the frequency-weight table, the data-gradient images of both nets.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r'''
#include <stdio.h>
#include <string.h>
#include <vector>
#include "st_ae.h"
using namespace sta;

template <int NT>
static void scatter_all(float* lds, const float* ae, const AEOffsets& go, int T, int OT, int K, bool dgrad)
{
    for (int tid = 0; tid < NT; ++tid) {
        AEParamRegs<NT> r;
        ae_params_issue<NT>(r, ae, go, T, OT, K, tid, 0, NL);
        ae_params_scatter<NT, 0>(lds, r, T, OT, K, tid, 0, NL, dgrad);
    }
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
    scatter_all<704>(lf.data(), ae[0].data(), go, T, OT, K, false);
    scatter_all<704>(lf.data() + CL::FWD_TOTAL, ae[1].data(), go, T, OT, K, false);
    for (int a = 0; a < 2; ++a) { lb[a].assign(CL::BWD_TOTAL, 0.f); scatter_all<256>(lb[a].data(), ae[a].data(), go, T, OT, K, true); }
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
