// Correctness + timing harness for the P16 (pre-split activation) variants of the split16 kernels (csrc/p16.hpp):
//   conv3  conv3_h8<.., P16> against conv3_h8 on float32 tensors: the P16 output must be split(float32 output) BIT FOR BIT
//          (same MFMAs on the same operands in the same order; only where the split happens moves), plus timing of both.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -Xclang -target-feature -Xclang -packed-fp32-ops tools/p16_tune.hip -o tools/p16_tune
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../dcscn-super-resolution_amd/csrc/conv3_h8.hpp"
#include "../dcscn-super-resolution_amd/csrc/split16_pack.hpp"

using namespace dcscn;

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            exit(1);                                                                       \
        }                                                                                  \
    } while (0)

static std::vector<float> rand_vec(size_t n, unsigned seed, float scale) {
    std::vector<float> h(n);
    unsigned s = seed;
    for (auto& v : h) { s = s * 1664525u + 1013904223u; v = (((s >> 8) & 0xffff) / 65536.0f - 0.5f) * scale; }
    return h;
}

__global__ void fill_act(float* p, size_t n, unsigned seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned s = (unsigned)(i * 2654435761u) ^ seed;
        float acc = 0.0f;
        for (int k = 0; k < 4; ++k) { s = s * 1664525u + 1013904223u; acc += ((s >> 8) & 0xffff) / 65536.0f - 0.5f; }
        float v = acc * 90.0f;
        s = s * 1664525u + 1013904223u;
        const unsigned sel = (s >> 10) & 1023;
        if (sel == 0) v *= 8.0f;
        else if (sel < 8) v *= 1e-4f;
        p[i] = v > 0.0f ? v : 0.2f * v;
    }
}

static void group_plan(int cout, int max_nt, int* n_groups, int* nt, int* n_full) {
    const int tiles16 = (cout + 15) / 16;
    *n_groups = (tiles16 + max_nt - 1) / max_nt;
    *nt = (tiles16 + *n_groups - 1) / *n_groups;
    *n_full = tiles16 - *n_groups * (*nt - 1);
}
static int padded_col(int cc, int nt, int n_full) {
    const int t = cc / 16, wide = n_full * nt;
    const int g = t < wide ? t / nt : n_full + (t - wide) / (nt - 1);
    const int tg = t < wide ? t % nt : (t - wide) % (nt - 1);
    return (g * nt + tg) * 16 + cc % 16;
}

struct P16Buf { P16Desc d; size_t bytes; };
static P16Buf p16_alloc(long long npix, int channels) {
    P16Buf b{};
    b.d.octs = (channels + 7) / 8;
    b.d.plane = p16_plane_bytes(npix);
    b.bytes = (size_t)p16_tensor_bytes(npix, b.d.octs);
    CK(hipMalloc((void**)&b.d.base, b.bytes));
    CK(hipMemset(b.d.base, 0, b.bytes));
    return b;
}

struct Layer3 { const char* name; int cin, cout; };
struct R { float ms32, ms16; int bad; };
static int g_wgs = 256;

template <typename F>
static float time_it(F launch, int reps, bool warm) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < (warm ? 2 : 0); ++i) launch();
    CK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int i = 0; i < reps; ++i) {
        CK(hipEventRecord(e0, 0));
        launch();
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        best = ms < best ? ms : best;
    }
    CK(hipGetLastError());
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    return best;
}

static R run_conv3(const Layer3& L, int N, int H, int W, bool timing, int overflow, bool quiet) {
    const int cin_phys = (L.cin + 3) & ~3, in_stride = cin_phys, out_stride = (L.cout + 3) & ~3;
    const long long npix = (long long)N * H * W;
    const size_t in_floats = (size_t)npix * in_stride, out_floats = (size_t)npix * out_stride;
    float *d_in, *d_o32;
    CK(hipMalloc(&d_in, in_floats * 4 + 256)); CK(hipMalloc(&d_o32, out_floats * 4)); CK(hipMemset(d_o32, 0, out_floats * 4));
    hipLaunchKernelGGL(fill_act, dim3(4096), dim3(256), 0, 0, d_in, in_floats, 99u + L.cin);
    if (overflow) {
        const float big = -3.0e5f;
        CK(hipMemcpy(d_in + ((size_t)((N - 1) * H + H / 2) * W + W / 3) * in_stride + 2, &big, 4, hipMemcpyHostToDevice));
    }
    std::vector<float> w = rand_vec((size_t)9 * L.cin * L.cout, 777 + L.cin, 2.0f * std::sqrt(6.0f / (9 * L.cin)));
    std::vector<float> bias = rand_vec(L.cout, 5, 0.4f), alpha = rand_vec(L.cout, 6, 0.25f);
    for (auto& v : alpha) v += 0.175f;
    int ng, nt, nfull;
    group_plan(L.cout, 6, &ng, &nt, &nfull);
    R r{};
    if (ng > 2) { printf("%s: %d groups, skipped\n", L.name, ng); return r; }
    const int n_chunks = (cin_phys + 31) / 32, ctot = ng * nt * 16;
    std::vector<float> dense((size_t)9 * n_chunks * 32 * ctot, 0.0f), bp(ctot, 0.0f), ap(ctot, 0.0f);
    for (int t = 0; t < 9; ++t)
        for (int c = 0; c < L.cin; ++c)
            for (int o = 0; o < L.cout; ++o) dense[((size_t)t * n_chunks * 32 + c) * ctot + padded_col(o, nt, nfull)] = w[((size_t)t * L.cin + c) * L.cout + o];
    for (int o = 0; o < L.cout; ++o) { bp[padded_col(o, nt, nfull)] = bias[o]; ap[padded_col(o, nt, nfull)] = alpha[o]; }
    const int e = split16_scale_exp(dense.data(), dense.size());
    const int tail_octs = c3h_tail_octs(cin_phys);
    std::vector<uint16_t> p16 = pack_conv16(dense, 9, n_chunks * 32, ctot, ng, nt, n_chunks, e, tail_octs);
    void* d_p16; float *d_bp, *d_ap;
    CK(hipMalloc(&d_p16, p16.size() * 2)); CK(hipMalloc(&d_bp, ctot * 4)); CK(hipMalloc(&d_ap, ctot * 4));
    CK(hipMemcpy(d_p16, p16.data(), p16.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_bp, bp.data(), ctot * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(d_ap, ap.data(), ctot * 4, hipMemcpyHostToDevice));
    const long long n_tiles = (long long)N * ((H + 15) / 16) * ((W + 15) / 16);
    int *d_redo, *d_redo16;
    CK(hipMalloc(&d_redo, n_tiles * 4)); CK(hipMemset(d_redo, 0, n_tiles * 4));
    CK(hipMalloc(&d_redo16, (N + 1) * 4)); CK(hipMemset(d_redo16, 0, (N + 1) * 4));
    ConvArgs a{};
    a.in = d_in; a.in_stride = in_stride; a.cin_phys = cin_phys; a.act = ACT_ALPHA;
    a.N = N; a.H = H; a.W = W; a.split = 1 << 30; a.ps = 1; a.ps_c = 1; a.vec4 = 1; a.res_stride = 1;
    a.tiles_x = (W + 15) / 16; a.tiles_y = (H + 15) / 16;
    a.wpack16 = d_p16; a.inv_scale = std::ldexp(1.0f, -e); a.n_chunks = n_chunks; a.n_full = nfull; a.bias = d_bp; a.alpha = d_ap; a.redo = d_redo; a.tail_octs = tail_octs;
    a.out0 = OutDesc{d_o32, out_stride, 0, out_stride}; a.out1 = a.out0;
    a.nt_pack = nt; a.n_groups = ng;
    // P16 tensors: input = pack(float32 input), expected output = pack(float32 output)
    P16Buf in16 = p16_alloc(npix, L.cin), out16 = p16_alloc(npix, L.cout), exp16 = p16_alloc(npix, L.cout);
    hipLaunchKernelGGL(p16_pack_kernel, dim3((unsigned)((npix * in16.d.octs + 255) / 256)), dim3(256), 0, 0, d_in, in_stride, L.cin, npix, in16.d);
    ConvArgs b = a;
    b.in = nullptr; b.in16 = in16.d;
    b.out0 = OutDesc{nullptr, 0, 0, out_stride, out16.d}; b.out1 = b.out0;
    b.redo = d_redo16;
    const int c0 = ng >= 2 ? nt : (nt + 1) / 2, c1 = ng >= 2 ? (nfull >= 2 ? nt : nt - 1) : nt - c0;
    const long long n_units = n_tiles * ((ng + 1) / 2);
    const dim3 g8((unsigned)std::min<long long>(n_units, g_wgs));
    auto launch = [&](bool p16v) {
        auto go = [&](auto c0_c, auto c1_c) {
            constexpr int C0 = decltype(c0_c)::value, C1c = decltype(c1_c)::value;
            if (p16v) {
                auto k = conv3_h8<C0, C1c, (C0 >= 4 ? C0 : 0), true>;
                CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, C3EGeom<C0>::LDS_BYTES));
                hipLaunchKernelGGL(k, g8, dim3(512), C3EGeom<C0>::LDS_BYTES, 0, b);
            } else {
#ifdef P16_TUNE_WIDE_ONLY
                return;
#endif
                auto k = conv3_h8<C0, C1c, (C0 >= 4 ? C0 : 0), false>;
                CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, C3EGeom<C0>::LDS_BYTES));
                hipLaunchKernelGGL(k, g8, dim3(512), C3EGeom<C0>::LDS_BYTES, 0, a);
            }
        };
#define H8_CASE(A, B) if (c0 == A && c1 == B) { go(std::integral_constant<int, A>{}, std::integral_constant<int, B>{}); return; }
        H8_CASE(6, 5) H8_CASE(5, 5) H8_CASE(5, 4) H8_CASE(4, 4) H8_CASE(4, 3)
#ifndef P16_TUNE_WIDE_ONLY                  // (tuning builds: the five variants of the bench model's wide layers only -- a third of the compile time)
        H8_CASE(6, 6) H8_CASE(3, 3) H8_CASE(3, 2) H8_CASE(2, 2) H8_CASE(2, 1) H8_CASE(1, 1) H8_CASE(1, 0)
#endif
#undef H8_CASE
        printf("no conv3_h8<%d, %d>\n", c0, c1); exit(1);
    };
    const int reps = timing ? 5 : 1;
    r.ms32 = time_it([&] { launch(false); }, reps, timing);
    r.ms16 = time_it([&] { launch(true); }, reps, timing);
    CK(hipDeviceSynchronize());
    hipLaunchKernelGGL(p16_pack_kernel, dim3((unsigned)((npix * exp16.d.octs + 255) / 256)), dim3(256), 0, 0, d_o32, out_stride, L.cout, npix, exp16.d);
    CK(hipDeviceSynchronize());
    std::vector<unsigned char> got(out16.bytes), want(exp16.bytes);
    CK(hipMemcpy(got.data(), out16.d.base, out16.bytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(want.data(), exp16.d.base, exp16.bytes, hipMemcpyDeviceToHost));
    size_t ndiff = 0, first = 0;
    for (size_t i = 0; i < got.size(); ++i)
        if (got[i] != want[i]) { if (!ndiff) first = i; ++ndiff; }
    std::vector<int> redo(N + 1);
    CK(hipMemcpy(redo.data(), d_redo16, (N + 1) * 4, hipMemcpyDeviceToHost));
    int nflag = 0;
    for (int i = 1; i <= N; ++i) nflag += redo[i] != 0;
    if (overflow) {
        // the poked input is beyond f16: (the float32 kernel flags its tile;) the P16 kernel flags the image only if an OUTPUT leaves the f16 range
        // or is non-finite -- with hi = -inf in the input the accumulators are non-finite: the last image and the pass flag must be set
        if (!redo[0] || !redo[N] || nflag != 1) { printf("  ** redo flags wrong: pass %d, image %d, %d images flagged\n", redo[0], redo[N], nflag); ++r.bad; }
        ndiff = 0;                                   // non-finite outputs: NaN payloads need not agree
    } else if (redo[0] || nflag) { printf("  ** redo flags set without an overflow (pass %d, %d images)\n", redo[0], nflag); ++r.bad; }
    if (ndiff) {
        ++r.bad;
        const size_t plane = (size_t)out16.d.plane;
        printf("  ** %zu bytes differ; first at byte %zu (chunk %zu, offset %zu in the plane)\n", ndiff, first, first / plane, first % plane);
    }
    const double flop = 2.0 * 9 * L.cin * (double)L.cout * npix;
    if (!quiet || r.bad)
        printf("%-8s %4d->%-4d %dx%dx%d  groups %d NT%d (%d wide) halves %d+%d chunks %d tail %d  f32 tensors %7.3f ms %6.1f TF  |  P16 %7.3f ms %6.1f TF  (%+.1f %%)%s\n", L.name, L.cin, L.cout,
               N, H, W, ng, nt, nfull, c0, c1, n_chunks, tail_octs, r.ms32, flop / r.ms32 * 1e-9, r.ms16, flop / r.ms16 * 1e-9, 100.0 * (r.ms16 / r.ms32 - 1.0), r.bad ? "  ** FAIL **" : "");
    fflush(stdout);
    CK(hipFree(d_in)); CK(hipFree(d_o32)); CK(hipFree(d_p16)); CK(hipFree(d_bp)); CK(hipFree(d_ap)); CK(hipFree(d_redo)); CK(hipFree(d_redo16));
    CK(hipFree(in16.d.base)); CK(hipFree(out16.d.base)); CK(hipFree(exp16.d.base));
    return r;
}

int main(int argc, char** argv) {
    const char* what = argc > 1 ? argv[1] : "all";
    if (getenv("C3E_WGS")) g_wgs = atoi(getenv("C3E_WGS"));
    int bad = 0;
    if (!strcmp(what, "edge") || !strcmp(what, "all")) {
        int n = 0;
        const int sizes[][2] = {{1, 1}, {2, 3}, {15, 17}, {16, 16}, {17, 33}, {31, 5}, {48, 48}, {50, 21}};
        const int cins[] = {24, 32, 36, 57, 64, 100, 196};
        const int couts[] = {20, 33, 48, 64, 80, 97, 112, 166};
        for (auto& sz : sizes)
            for (int cin : cins)
                for (int cout : couts) {
                    R r = run_conv3(Layer3{"edge", cin, cout}, 3, sz[0], sz[1], false, 0, true);
                    ++n; bad += r.bad;
                }
        { R r = run_conv3(Layer3{"overflow", 57, 48}, 3, 40, 50, false, 1, false); ++n; bad += r.bad; }
        { R r = run_conv3(Layer3{"overflow", 133, 120}, 3, 40, 50, false, 1, false); ++n; bad += r.bad; }
        printf("p16 conv3 edge: %d cases, %d failures\n", n, bad);
    }
    if (!strcmp(what, "wide")) {             // tuning builds (-DP16_TUNE_WIDE_ONLY): the P16 kernel on CNN2 .. CNN7 only, no comparison
        const Layer3 layers[] = {{"CNN2", 196, 166}, {"CNN3", 166, 148}, {"CNN4", 148, 133}, {"CNN5", 133, 120}, {"CNN6", 120, 108}, {"CNN7", 108, 97}};
        double w16 = 0;
        for (const Layer3& L : layers) { R r = run_conv3(L, 1024, 48, 48, true, 0, true); w16 += r.ms16; printf("%s %.3f  ", L.name, r.ms16); }
        printf("\nCNN2-7 P16: %.3f ms\n", w16);
        return 0;
    }
    if (!strcmp(what, "bench") || !strcmp(what, "all")) {
        const Layer3 layers[] = {{"CNN2", 196, 166}, {"CNN3", 166, 148}, {"CNN4", 148, 133}, {"CNN5", 133, 120}, {"CNN6", 120, 108}, {"CNN7", 108, 97},
                                 {"CNN8", 97, 86},   {"CNN9", 86, 76},   {"CNN10", 76, 66},  {"CNN11", 66, 57},  {"CNN12", 57, 48},  {"B2", 32, 32}};
        double s32 = 0, s16 = 0, w32 = 0, w16 = 0;
        int i = 0;
        for (const Layer3& L : layers) {
            R r = run_conv3(L, 1024, 48, 48, true, 0, false);
            bad += r.bad;
            s32 += r.ms32; s16 += r.ms16;
            if (i++ < 6) { w32 += r.ms32; w16 += r.ms16; }
        }
        printf("CNN2-7: f32 tensors %.3f ms, P16 %.3f ms (%+.1f %%);  all 12: %.3f -> %.3f ms\n", w32, w16, 100.0 * (w16 / w32 - 1.0), s32, s16);
    }
    printf("p16_tune: %d failures\n", bad);
    return bad != 0;
}
