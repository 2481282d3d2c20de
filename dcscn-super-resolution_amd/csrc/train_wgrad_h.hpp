// Option "train_split16_wgrad" (include/dcscn.h): the weight gradient of the training plan's wide layers on v_mfma_f32_16x16x32_f16 at f32
// accuracy.   part[s][tap][ci][co] = sum over the pixels of split s of in[p + tap][ci] * dz[p][co]   as split16.hpp's three products
// ah*bh + ah*bl + al*bh per k-chunk of 32 pixels, accumulated in f32.  Both operands are scaled by train_h.hpp's power of two (max-abs into
// [2^13, 2^14); the exponents are read from device memory) before they are split, and the epilogue undoes the scale with ldexpf (exact).
//
// The contract is tconv_wgrad's (train_kernels.hpp): SAME padding, stride 1, ks 1 / 3 / 5 / 7, arbitrary in_stride and slice offset, ragged pixel,
// row and column counts masked to zero, a fixed partition of the pixels summed in a fixed order (no atomics: two runs give the same bits), a
// non-finite input gives a non-finite result.  The partition differs from wgrad_splits': the unit is a TILE of tr rows x tc columns of one
// image, tiles are numbered image-major, then row block, then column block, and split s sums tiles [s * tps, (s + 1) * tps) in that order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dcscn_impl {

struct TWgradHArgs {
    const float* in; int in_stride; int cin;
    int n, H, W, ks;
    const float* dz; int cout;      // dense [pixels][cout]
    const int* e_in;                // exponent of the input slice's scale (device memory)
    const int* e_dz;                // ... of dz's
    float* part;                    // [splits][ks*ks][cin][cout]
};

constexpr int kWgHBlock = 64;            // channels (rows) and columns of a workgroup's block of the gradient
constexpr int kWgHPitch = 288;           // bytes of one LDS position: 64 hi halves | 64 lo halves | 32 bytes that spread the rows over the banks
constexpr size_t kWgHLdsBudget = 144 * 1024;
constexpr size_t kWgHLdsMax = 160 * 1024;

// the tiling and the split of one layer: fixed by the shape alone (tests/test_train_split16_wgrad_host.py restates it)
struct TWgradHPlan {
    int tr, tc, tcp;          // tile rows and columns; LDS positions per tile row = tc + ks - 1
    int kpad;                 // dz positions of a tile: tr * tcp rounded up to a multiple of 32 (the k-chunks)
    int in_cap;               // input positions: kpad + the largest tap offset, rounded up to a multiple of 16
    int tiles_y, tiles_x;
    int64_t tiles;            // n * tiles_y * tiles_x
    int tg, groups;           // taps per workgroup (all 9 of a 3x3, else one filter row) and tap groups
    int64_t tps;              // tiles per split
    int splits;
    size_t lds_bytes;
};

inline TWgradHPlan twgrad_h_plan(int ks, int cin, int cout, int n, int H, int W) {
    TWgradHPlan p;
    const int tc_max = ks <= 3 ? 64 : 32;
    p.tc = W < tc_max ? W : tc_max;
    p.tcp = p.tc + ks - 1;
    const int slack = (ks - 1) * (p.tcp + 1);
    auto positions = [&](int tr, int* kpad, int* in_cap) {
        *kpad = (tr * p.tcp + 31) / 32 * 32;
        *in_cap = (*kpad + slack + 15) / 16 * 16;
        return (size_t)(*kpad + *in_cap);
    };
    p.tr = 1;
    for (int tr = 2; tr <= 8 && tr <= H; ++tr) {
        int k, c;
        if (positions(tr, &k, &c) * kWgHPitch > kWgHLdsBudget) break;
        p.tr = tr;
    }
    p.lds_bytes = positions(p.tr, &p.kpad, &p.in_cap) * kWgHPitch;
    p.tiles_y = (H + p.tr - 1) / p.tr;
    p.tiles_x = (W + p.tc - 1) / p.tc;
    p.tiles = (int64_t)n * p.tiles_y * p.tiles_x;
    p.tg = ks == 3 ? 9 : ks;
    p.groups = ks * ks / p.tg;
    const int64_t blocks = (int64_t)((cin + kWgHBlock - 1) / kWgHBlock) * p.groups * ((cout + kWgHBlock - 1) / kWgHBlock);
    int64_t s = (256 + blocks - 1) / blocks;
    s = s < 1 ? 1 : s > p.tiles ? p.tiles : s;
    p.tps = (p.tiles + s - 1) / s;
    p.splits = (int)((p.tiles + p.tps - 1) / p.tps);
    return p;
}

// hipErrorInvalidValue (nothing launched) when the plan's LDS image is over 160 KB
hipError_t launch_tconv_wgrad_h(const TWgradHArgs& a, const TWgradHPlan& p, hipStream_t st);

}  // namespace dcscn_impl
