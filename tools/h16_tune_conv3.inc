// conv3 part of tools/h16_tune.hip: conv3_h (direct 3x3 on the f16 pipe) vs conv_wino2 (f32 Winograd) vs a float64 naive conv.

#ifndef C3H_MAX_NT
#define C3H_MAX_NT 6
#endif

struct Layer3 { const char* name; int cin, cout, ps; };

// naive reference: one thread per (pixel, channel), float64 accumulation, HWIO weights, bias + PReLU, optional depth_to_space
__global__ void naive_conv3(const float* in, int in_stride, int cin, const float* w, int cout, const float* bias, const float* alpha, int n, int H,
                            int W, float* out, int out_stride, int ps) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)n * H * W * cout;
    if (idx >= total) return;
    const int co = (int)(idx % cout);
    long long p = idx / cout;
    const int x = (int)(p % W); p /= W;
    const int y = (int)(p % H);
    const int img = (int)(p / H);
    double s = 0.0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int yy = y + dy, xx = x + dx;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const float* ip = in + ((size_t)(img * H + yy) * W + xx) * in_stride;
            const float* wp = w + ((size_t)((dy + 1) * 3 + (dx + 1)) * cin) * cout + co;
            for (int c = 0; c < cin; ++c) s += (double)ip[c] * (double)wp[(size_t)c * cout];
        }
    float v = (float)(s + bias[co]);
    v = v > 0.0f ? v : alpha[co] * v;
    if (ps == 1) out[((size_t)(img * H + y) * W + x) * out_stride + co] = v;
    else {
        const int psc = cout / (ps * ps);
        const int sub = co / psc, ch = co - sub * psc, ay = sub / ps, bx = sub - ay * ps;
        out[((size_t)(img * H * ps + y * ps + ay) * (W * ps) + (x * ps + bx)) * out_stride + ch] = v;
    }
}

// conv_wino2 image (api: finalize_op): [group][chunk of 8][f][(c & 1) * 4 + (c >> 1)][NS]
static std::vector<float> pack_wino2(const std::vector<float>& w, int cin, int cout, int cin_phys, int nt, int n_groups, int n_full, int* n_chunks) {
    const int kc = 8, ns = conv_ns(nt);
    *n_chunks = (cin_phys + kc - 1) / kc;
    const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    std::vector<float> p((size_t)n_groups * *n_chunks * 16 * kc * ns, 0.0f);
    for (int c = 0; c < cin; ++c)
        for (int o = 0; o < cout; ++o) {
            double g[3][3];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) g[i][j] = w[((size_t)(i * 3 + j) * cin + c) * cout + o];
            const int pc = padded_col(o, nt, n_full);
            const int grp = pc / (nt * 16), jn = pc % (nt * 16);
            const int cc = c % kc, row = (cc & 1) * 4 + (cc >> 1);
            for (int xi = 0; xi < 4; ++xi)
                for (int nu = 0; nu < 4; ++nu) {
                    double u = 0;
                    for (int i = 0; i < 3; ++i)
                        for (int j = 0; j < 3; ++j) u += G[xi][i] * g[i][j] * G[nu][j];
                    p[(((size_t)grp * *n_chunks + c / kc) * 16 + xi * 4 + nu) * kc * ns + (size_t)row * ns + jn] = (float)u;
                }
        }
    return p;
}

static dim3 tiles_grid(ConvArgs& a, int n_groups) { return dim3((unsigned)xcd_grid_ids(a, n_groups)); }

struct R3 { double e32, e16, maxv; float ms32, ms16, mshp, msh8; int bad; };
static int g_h8_wgs = 256;        // persistent workgroups of conv3_h8 (env C3E_WGS)
static int g_hp_wgs = 512;        // persistent workgroups of conv3_hp (argv: conv3 <mode> ... or env C3P_WGS)
static int g_det_runs = 0;        // > 0: after the timing, run conv3_h this many more times and compare every output bit with the first run

__global__ void count_diff(const float* a, const float* b, size_t n, unsigned long long* cnt, float* maxd) {
    unsigned long long c = 0;
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float d = fabsf(a[i] - b[i]);
        if (__float_as_uint(a[i]) != __float_as_uint(b[i])) { ++c; m = fmaxf(m, d); }
    }
    if (c) { atomicAdd(cnt, c); atomicMax(reinterpret_cast<unsigned*>(maxd), __float_as_uint(m)); }
}

static R3 run_conv3(const Layer3& L, int N, int H, int W, int n_check, bool timing, int overflow_test, bool quiet) {
    const int cin_phys = (L.cin + 3) & ~3, in_stride = cin_phys;
    const int cstore = L.ps == 1 ? L.cout : L.cout / (L.ps * L.ps);
    const int out_stride = (cstore + 3) & ~3;
    const size_t in_floats = (size_t)N * H * W * in_stride, out_floats = (size_t)N * H * L.ps * W * L.ps * out_stride;
    float *d_in, *d_ref, *d_o32, *d_o16, *d_wraw, *d_bias, *d_alpha;
    CK(hipMalloc(&d_in, in_floats * 4 + 256)); CK(hipMalloc(&d_ref, out_floats * 4)); CK(hipMalloc(&d_o32, out_floats * 4)); CK(hipMalloc(&d_o16, out_floats * 4));
    hipLaunchKernelGGL(fill_act, dim3(4096), dim3(256), 0, 0, d_in, in_floats, 99u + L.cin);
    std::vector<float> w = rand_vec((size_t)9 * L.cin * L.cout, 777 + L.cin, 2.0f * std::sqrt(6.0f / (9 * L.cin)));
    std::vector<float> bias = rand_vec(L.cout, 5, 0.4f), alpha = rand_vec(L.cout, 6, 0.25f);
    for (auto& v : alpha) v += 0.175f;
    CK(hipMalloc(&d_wraw, w.size() * 4)); CK(hipMalloc(&d_bias, L.cout * 4)); CK(hipMalloc(&d_alpha, L.cout * 4));
    CK(hipMemcpy(d_wraw, w.data(), w.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_bias, bias.data(), L.cout * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(d_alpha, alpha.data(), L.cout * 4, hipMemcpyHostToDevice));
    CK(hipMemset(d_ref, 0, out_floats * 4)); CK(hipMemset(d_o32, 0, out_floats * 4)); CK(hipMemset(d_o16, 0, out_floats * 4));
    long long poke_tile = -1;
    ConvArgs a{};
    a.in = d_in; a.in_stride = in_stride; a.in_off = 0; a.cin_phys = cin_phys; a.act = ACT_ALPHA;
    a.N = N; a.H = H; a.W = W; a.split = 1 << 30; a.ps = L.ps; a.ps_c = L.ps == 1 ? 1 : cstore; a.vec4 = 1; a.res = nullptr; a.res_stride = 1;
    a.tiles_x = (W + 15) / 16; a.tiles_y = (H + 15) / 16;
    const long long n_tiles = (long long)N * a.tiles_y * a.tiles_x;
    int* d_redo;
    CK(hipMalloc(&d_redo, n_tiles * 4)); CK(hipMemset(d_redo, 0, n_tiles * 4));
    if (overflow_test) {
        const int py = H / 2, px = W / 3, pimg = N - 1;
        const float big = -3.0e5f;
        CK(hipMemcpy(d_in + ((size_t)(pimg * H + py) * W + px) * in_stride + 2, &big, 4, hipMemcpyHostToDevice));
        poke_tile = ((long long)pimg * a.tiles_y + py / 16) * a.tiles_x + px / 16;
    }
    CK(hipDeviceSynchronize());
    {
        const long long total = (long long)n_check * H * W * L.cout;
        hipLaunchKernelGGL(naive_conv3, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, d_in, in_stride, L.cin, d_wraw, L.cout, d_bias, d_alpha, n_check, H, W,
                           d_ref, out_stride, L.ps);
        CK(hipDeviceSynchronize());
    }
    R3 r{};
    const int owidth = L.ps == 1 ? out_stride : L.cout;
    const int reps = timing ? 5 : 1;
    // ---- f32 Winograd ----
    float *d_p32 = nullptr, *d_bp32 = nullptr, *d_ap32 = nullptr;
    ConvArgs a32 = a;
    dim3 grid32;
    int nt32;
    {
        int ng, nfull, nch;
        group_plan(L.cout, 3, &ng, &nt32, &nfull);
        std::vector<float> p = pack_wino2(w, L.cin, L.cout, cin_phys, nt32, ng, nfull, &nch);
        const int ctot = ng * nt32 * 16;
        std::vector<float> bp(ctot, 0.0f), ap(ctot, 0.0f);
        for (int o = 0; o < L.cout; ++o) { bp[padded_col(o, nt32, nfull)] = bias[o]; ap[padded_col(o, nt32, nfull)] = alpha[o]; }
        CK(hipMalloc(&d_p32, p.size() * 4)); CK(hipMalloc(&d_bp32, ctot * 4)); CK(hipMalloc(&d_ap32, ctot * 4));
        CK(hipMemcpy(d_p32, p.data(), p.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(d_bp32, bp.data(), ctot * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(d_ap32, ap.data(), ctot * 4, hipMemcpyHostToDevice));
        a32.wpack = d_p32; a32.n_chunks = nch; a32.n_full = nfull; a32.bias = d_bp32; a32.alpha = d_ap32;
        a32.out0 = OutDesc{d_o32, out_stride, 0, owidth}; a32.out1 = a32.out0;
        a32.redo = d_redo;
        grid32 = tiles_grid(a32, ng);
    }
    auto run32 = [&](const ConvArgs& b, int nrep) {
        switch (nt32) {
            case 1: { auto k = conv_wino2<1>; CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, Wino2Geom<1>::LDS_BYTES)); return time_kernel(k, grid32, Wino2Geom<1>::LDS_BYTES, b, nrep); }
            case 2: { auto k = conv_wino2<2>; CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, Wino2Geom<2>::LDS_BYTES)); return time_kernel(k, grid32, Wino2Geom<2>::LDS_BYTES, b, nrep); }
            default: { auto k = conv_wino2<3>; CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, Wino2Geom<3>::LDS_BYTES)); return time_kernel(k, grid32, Wino2Geom<3>::LDS_BYTES, b, nrep); }
        }
    };
    r.ms32 = run32(a32, reps);
    // ---- f16 x 3 direct ----
    int ng, nt, nfull;
    group_plan(L.cout, C3H_MAX_NT, &ng, &nt, &nfull);
    const int n_chunks = (cin_phys + 31) / 32, ctot = ng * nt * 16;
    std::vector<float> dense((size_t)9 * n_chunks * 32 * ctot, 0.0f), bp(ctot, 0.0f), ap(ctot, 0.0f);
    for (int t = 0; t < 9; ++t)
        for (int c = 0; c < L.cin; ++c)
            for (int o = 0; o < L.cout; ++o) dense[((size_t)t * n_chunks * 32 + c) * ctot + padded_col(o, nt, nfull)] = w[((size_t)t * L.cin + c) * L.cout + o];
    for (int o = 0; o < L.cout; ++o) { bp[padded_col(o, nt, nfull)] = bias[o]; ap[padded_col(o, nt, nfull)] = alpha[o]; }
    const int e = split16_scale_exp(dense.data(), dense.size());
    static const int no_tail = getenv("C3H_NO_TAIL") ? atoi(getenv("C3H_NO_TAIL")) : 0;       // A/B aid: 1 = plain last chunk
    const int tail_octs = no_tail ? 0 : c3h_tail_octs(cin_phys);
    std::vector<uint16_t> p16 = pack_conv16(dense, 9, n_chunks * 32, ctot, ng, nt, n_chunks, e, tail_octs);
    void* d_p16; float *d_bp, *d_ap;
    CK(hipMalloc(&d_p16, p16.size() * 2)); CK(hipMalloc(&d_bp, ctot * 4)); CK(hipMalloc(&d_ap, ctot * 4));
    CK(hipMemcpy(d_p16, p16.data(), p16.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_bp, bp.data(), ctot * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(d_ap, ap.data(), ctot * 4, hipMemcpyHostToDevice));
    ConvArgs b = a;
    b.wpack16 = d_p16; b.inv_scale = std::ldexp(1.0f, -e); b.n_chunks = n_chunks; b.n_full = nfull; b.bias = d_bp; b.alpha = d_ap; b.redo = d_redo; b.tail_octs = tail_octs;
    b.out0 = OutDesc{d_o16, out_stride, 0, owidth}; b.out1 = b.out0;
    const dim3 grid = tiles_grid(b, ng);
    auto run16 = [&](auto nt_c) {
        constexpr int NTc = decltype(nt_c)::value;
        auto k = conv3_h<NTc>;
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, C3HGeom<NTc>::LDS_BYTES));
        return time_kernel(k, grid, C3HGeom<NTc>::LDS_BYTES, b, reps);
    };
    // ---- the one-product form (option "fast16": NP = 1) first, into the same buffer; read back before the three-product launch overwrites it ----
    std::vector<float> o1;
    float ms1 = 0;
    if (!overflow_test) {
        auto run1 = [&](auto nt_c) {
            constexpr int NTc = decltype(nt_c)::value;
            auto k = conv3_h<NTc, 2, false, 1>;
            CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, C3HGeom<NTc>::LDS_BYTES));
            return time_kernel(k, grid, C3HGeom<NTc>::LDS_BYTES, b, reps);
        };
        switch (nt) {
            case 1: ms1 = run1(std::integral_constant<int, 1>{}); break;
            case 2: ms1 = run1(std::integral_constant<int, 2>{}); break;
            case 3: ms1 = run1(std::integral_constant<int, 3>{}); break;
            case 4: ms1 = run1(std::integral_constant<int, 4>{}); break;
#if C3H_MAX_NT >= 5
            case 5: ms1 = run1(std::integral_constant<int, 5>{}); break;
#endif
#if C3H_MAX_NT >= 6
            case 6: ms1 = run1(std::integral_constant<int, 6>{}); break;
#endif
            default: printf("no conv3_h<%d>\n", nt); exit(1);
        }
        o1.resize((size_t)n_check * H * L.ps * W * L.ps * out_stride);
        CK(hipMemcpy(o1.data(), d_o16, o1.size() * 4, hipMemcpyDeviceToHost));
        CK(hipMemset(d_redo, 0, n_tiles * 4));
    }
    switch (nt) {
        case 1: r.ms16 = run16(std::integral_constant<int, 1>{}); break;
        case 2: r.ms16 = run16(std::integral_constant<int, 2>{}); break;
        case 3: r.ms16 = run16(std::integral_constant<int, 3>{}); break;
        case 4: r.ms16 = run16(std::integral_constant<int, 4>{}); break;
#if C3H_MAX_NT >= 5
        case 5: r.ms16 = run16(std::integral_constant<int, 5>{}); break;
#endif
#if C3H_MAX_NT >= 6
        case 6: r.ms16 = run16(std::integral_constant<int, 6>{}); break;
#endif
        default: printf("no conv3_h<%d>\n", nt); exit(1);
    }
    // ---- conv3_hp: the same arithmetic, persistent workgroups (bit-identical to conv3_h by construction) ----
    unsigned long long hp_diff = 0;
    float* d_ohp = nullptr;
    int* d_work = nullptr;
    // ---- conv3_h8: persistent 8-wave workgroups, one input image for all channel groups (bit-identical to conv3_h by construction) ----
    unsigned long long h8_diff = 0;
#ifdef H16_H8
    {
        float* d_o8;
        CK(hipMalloc(&d_o8, out_floats * 4)); CK(hipMemset(d_o8, 0, out_floats * 4));
        ConvArgs b8 = b;
        b8.out0 = OutDesc{d_o8, out_stride, 0, owidth}; b8.out1 = b8.out0;
        b8.nt_pack = nt;
        b8.n_groups = ng;
        CK(hipMemset(d_redo, 0, n_tiles * 4));
        // tiles of half 0 / half 1 (launch constants of the kernel): two groups -> one each; one group -> its tiles split
        const int full0 = nt, full1 = ng >= 2 ? (nfull >= 2 ? nt : nt - 1) : 0;
        const int c0 = ng >= 2 ? full0 : (nt + 1) / 2, c1 = ng >= 2 ? full1 : nt - c0;
        const bool h8_ok = ng == 1 || (ng == 2) || (ng % 2 == 0 && nfull == ng);
        const long long n_units = n_tiles * ((ng + 1) / 2);
        const dim3 g8((unsigned)std::min<long long>(n_units, g_h8_wgs));
        auto launch8 = [&]() {
            const ConvArgs c = b8;
            auto go = [&](auto c0_c, auto c1_c) {
                constexpr int C0 = decltype(c0_c)::value, C1c = decltype(c1_c)::value;
                auto k = conv3_h8<C0, C1c, (C0 >= 4 ? C0 : 0)>;       // two groups: nt = C0 >= 4 in the image; one group split: run time
                CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, C3EGeom<C0>::LDS_BYTES));
                hipLaunchKernelGGL(k, g8, dim3(512), C3EGeom<C0>::LDS_BYTES, 0, c);
            };
            auto go_nt = [&]() {
#define H8_CASE(A, B) if (c0 == A && c1 == B) { go(std::integral_constant<int, A>{}, std::integral_constant<int, B>{}); return; }
                H8_CASE(6, 6) H8_CASE(6, 5) H8_CASE(5, 5) H8_CASE(5, 4) H8_CASE(4, 4) H8_CASE(4, 3)
                H8_CASE(3, 3) H8_CASE(3, 2) H8_CASE(2, 2) H8_CASE(2, 1) H8_CASE(1, 1) H8_CASE(1, 0)
#undef H8_CASE
                printf("no conv3_h8<%d, %d>\n", c0, c1); exit(1);
            };
            if (!h8_ok) return;
            go_nt();
        };
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        for (int i = 0; i < (timing ? 2 : 0); ++i) launch8();
        CK(hipDeviceSynchronize());
        float best = 1e30f;
        for (int i = 0; i < reps; ++i) {
            CK(hipEventRecord(e0, 0));
            launch8();
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            best = ms < best ? ms : best;
        }
        CK(hipGetLastError());
        r.msh8 = best;
        unsigned long long* d_cnt; float* d_max;
        CK(hipMalloc(&d_cnt, 8)); CK(hipMalloc(&d_max, 4)); CK(hipMemset(d_cnt, 0, 8)); CK(hipMemset(d_max, 0, 4));
        hipLaunchKernelGGL(count_diff, dim3(2048), dim3(256), 0, 0, d_o16, d_o8, out_floats, d_cnt, d_max);
        CK(hipMemcpy(&h8_diff, d_cnt, 8, hipMemcpyDeviceToHost));
        CK(hipFree(d_cnt)); CK(hipFree(d_max));
        if (!h8_ok) h8_diff = 0;
        if (h8_diff) ++r.bad;
        CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
        CK(hipFree(d_o8));
    }
#endif
    if (g_det_runs > 0) {
        float* d_first;
        unsigned long long* d_cnt; float* d_max;
        CK(hipMalloc(&d_first, out_floats * 4)); CK(hipMalloc(&d_cnt, 8)); CK(hipMalloc(&d_max, 4));
        CK(hipMemcpy(d_first, d_o16, out_floats * 4, hipMemcpyDeviceToDevice));
        int bad_runs = 0; unsigned long long total = 0; float worst = 0;
        for (int it = 0; it < g_det_runs; ++it) {
            CK(hipMemset(d_cnt, 0, 8)); CK(hipMemset(d_max, 0, 4));
            if (getenv("DET_REWRITE")) {       // producer -> consumer: the input is rewritten (garbage first, then the same data) right before the conv
                hipLaunchKernelGGL(fill_act, dim3(4096), dim3(256), 0, 0, d_in, in_floats, 12345u + it);
                hipLaunchKernelGGL(fill_act, dim3(4096), dim3(256), 0, 0, d_in, in_floats, 99u + L.cin);
            }
            switch (nt) {
                case 1: { auto k = conv3_h<1>; hipLaunchKernelGGL(k, grid, dim3(256), C3HGeom<1>::LDS_BYTES, 0, b); break; }
                case 2: { auto k = conv3_h<2>; hipLaunchKernelGGL(k, grid, dim3(256), C3HGeom<2>::LDS_BYTES, 0, b); break; }
                case 3: { auto k = conv3_h<3>; hipLaunchKernelGGL(k, grid, dim3(256), C3HGeom<3>::LDS_BYTES, 0, b); break; }
                default: { auto k = conv3_h<4>; hipLaunchKernelGGL(k, grid, dim3(256), C3HGeom<4>::LDS_BYTES, 0, b); break; }
            }
            hipLaunchKernelGGL(count_diff, dim3(2048), dim3(256), 0, 0, d_first, d_o16, out_floats, d_cnt, d_max);
            unsigned long long c; float m;
            CK(hipMemcpy(&c, d_cnt, 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(&m, d_max, 4, hipMemcpyDeviceToHost));
            if (c) { ++bad_runs; total += c; worst = std::fmax(worst, m); }
        }
        printf("  determinism %s: %d of %d re-runs differ from the first (%llu elements in total, max |diff| %.3g)\n", L.name, bad_runs, g_det_runs, total, worst);
        CK(hipFree(d_first)); CK(hipFree(d_cnt)); CK(hipFree(d_max));
    }
    std::vector<int> redo(n_tiles);
    CK(hipMemcpy(redo.data(), d_redo, n_tiles * 4, hipMemcpyDeviceToHost));
    long long nflag = 0;
    for (int v : redo) nflag += v != 0;
    if (overflow_test) {
        // the poked pixel feeds its own tile and, on a tile edge, the neighbours: every flagged tile must be one of those
        if (nflag < 1 || nflag > 4 || !redo[poke_tile]) { printf("  ** redo flags wrong: %lld set, tile of the poked pixel %d\n", nflag, redo[poke_tile]); ++r.bad; }
        ConvArgs f = a32;
        f.out0 = OutDesc{d_o16, out_stride, 0, owidth}; f.out1 = f.out0;
        f.redo_check = 1;
        run32(f, 1);
    } else if (nflag) { printf("  ** %lld redo flags set without an overflow\n", nflag); ++r.bad; }

    const size_t cnt = (size_t)n_check * H * L.ps * W * L.ps * out_stride;
    std::vector<float> rf(cnt), o32(cnt), o16(cnt);
    CK(hipMemcpy(rf.data(), d_ref, cnt * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(o32.data(), d_o32, cnt * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(o16.data(), d_o16, cnt * 4, hipMemcpyDeviceToHost));
    double s32 = 0, s16 = 0, stray = 0;
    long long nn = 0;
    for (size_t px = 0; px < cnt / out_stride; ++px)
        for (int c = 0; c < out_stride; ++c) {
            const size_t i = px * out_stride + c;
            if (c >= cstore) { stray = std::fmax(stray, std::fabs((double)o16[i])); continue; }
            const double a32e = std::fabs((double)o32[i] - rf[i]), a16e = std::fabs((double)o16[i] - rf[i]);
            if (!(a32e <= r.e32)) r.e32 = a32e;
            if (!(a16e <= r.e16)) r.e16 = a16e;
            s32 += a32e * a32e; s16 += a16e * a16e; ++nn;
            r.maxv = std::fmax(r.maxv, std::fabs((double)rf[i]));
        }
    const bool ok = r.e16 <= 2.0 * r.e32 + 2e-6 * r.maxv && r.e16 <= 1e-5 * r.maxv && std::isfinite(r.e16) && stray == 0.0;
    r.bad += !ok;
    const double flop = 2.0 * 9 * L.cin * (double)L.cout * N * H * W;
    if (h8_diff) printf("  ** conv3_h8 differs from conv3_h in %llu elements\n", h8_diff);
    if (hp_diff) printf("  ** conv3_hp differs from conv3_h in %llu elements\n", hp_diff);
    if (!quiet || !ok || r.bad)
        printf("%-8s %4d->%-4d %dx%dx%d ps%d  wino2 f32 NT%d %7.3f ms %6.1f TF  |  conv3_h NT%d groups %d (%d wide) chunks %d %7.3f ms %6.1f TF  |  conv3_hp %7.3f ms %6.1f TF%s  |  conv3_h8 %7.3f ms %6.1f TF%s  "
               "max err f32 %.3g f16x3 %.3g (rms %.3g / %.3g, max|ref| %.4g)%s%s\n",
               L.name, L.cin, L.cout, N, H, W, L.ps, nt32, r.ms32, flop / r.ms32 * 1e-9, nt, ng, nfull, n_chunks, r.ms16, flop / r.ms16 * 1e-9, r.mshp, flop / r.mshp * 1e-9,
               hp_diff ? "  ** hp != conv3_h **" : "", r.msh8, r.msh8 > 0 ? flop / r.msh8 * 1e-9 : 0.0, h8_diff ? "  ** h8 != conv3_h **" : "", r.e32, r.e16,
               std::sqrt(s32 / nn), std::sqrt(s16 / nn), r.maxv, ok ? "" : "  ** MISMATCH **", stray != 0 ? "  ** STRAY WRITE **" : "");
    if (!o1.empty() && (!quiet || !ok || r.bad)) {
        double e1 = 0, s1 = 0;
        for (size_t px = 0; px < cnt / out_stride; ++px)
            for (int c = 0; c < cstore; ++c) {
                const double a1 = std::fabs((double)o1[px * out_stride + c] - rf[px * out_stride + c]);
                if (!(a1 <= e1)) e1 = a1;
                s1 += a1 * a1;
            }
        printf("%-8s   one product (fast16): %7.3f ms (%.3f of f16x3)  max err %.3g  rms %.3g  (%.0f x the f16x3 rms)\n", L.name, ms1, ms1 / r.ms16, e1, std::sqrt(s1 / nn),
               std::sqrt(s1 / nn) / std::sqrt(s16 / nn));
    }
    fflush(stdout);
    CK(hipFree(d_in)); CK(hipFree(d_ref)); CK(hipFree(d_o32)); CK(hipFree(d_o16)); CK(hipFree(d_wraw)); CK(hipFree(d_bias)); CK(hipFree(d_alpha));
    if (d_ohp) CK(hipFree(d_ohp)); if (d_work) CK(hipFree(d_work)); CK(hipFree(d_p32)); CK(hipFree(d_bp32)); CK(hipFree(d_ap32)); CK(hipFree(d_p16)); CK(hipFree(d_bp)); CK(hipFree(d_ap)); CK(hipFree(d_redo));
    return r;
}

static int conv3_main(int argc, char** argv) {
    const char* what = argc > 2 ? argv[2] : "all";
    int bad = 0;
    if (getenv("C3P_WGS")) g_hp_wgs = atoi(getenv("C3P_WGS"));
    if (getenv("C3E_WGS")) g_h8_wgs = atoi(getenv("C3E_WGS"));
    if (!strcmp(what, "edge") || !strcmp(what, "all")) {
        int n = 0;
        const int sizes[][2] = {{1, 1}, {2, 3}, {15, 17}, {16, 16}, {17, 33}, {31, 5}, {48, 48}, {50, 21}};
        const int cins[] = {24, 32, 36, 57, 64, 100};
        const int couts[] = {20, 33, 48, 64, 80, 97, 112, 166};
        for (auto& sz : sizes)
            for (int cin : cins)
                for (int cout : couts) {
                    const Layer3 L{"edge", cin, cout, 1};
                    R3 r = run_conv3(L, 3, sz[0], sz[1], 3, false, 0, true);
                    ++n; bad += r.bad;
                }
        for (int ps : {2, 3}) {
            const Layer3 L{"edge-ps", 40, ps * ps * 8, ps};
            R3 r = run_conv3(L, 2, 19, 23, 2, false, 0, true);
            ++n; bad += r.bad;
        }
        {   // overflow -> redo -> f32 fallback, poked pixel in the interior and the result compared everywhere
            const Layer3 L{"overflow", 57, 48, 1};
            R3 r = run_conv3(L, 3, 40, 50, 3, false, 1, false);
            ++n; bad += r.bad;
        }
        printf("conv3 edge: %d cases, %d failures\n", n, bad);
    }
    if (!strcmp(what, "det")) {
        g_det_runs = argc > 3 ? atoi(argv[3]) : 20;
        const int N = argc > 4 ? atoi(argv[4]) : 96;
        const Layer3 layers[] = {{"CNN2", 196, 166, 1}, {"CNN5", 133, 120, 1}, {"CNN9", 86, 76, 1}, {"CNN12", 57, 48, 1}, {"B2", 32, 32, 1}};
        for (const Layer3& L : layers) run_conv3(L, N, 48, 48, 1, false, 0, false);
        return 0;
    }
    if (!strcmp(what, "bench") || !strcmp(what, "all")) {
        const Layer3 layers[] = {{"CNN2", 196, 166, 1}, {"CNN3", 166, 148, 1}, {"CNN4", 148, 133, 1}, {"CNN5", 133, 120, 1}, {"CNN6", 120, 108, 1},
                                 {"CNN7", 108, 97, 1},  {"CNN8", 97, 86, 1},   {"CNN9", 86, 76, 1},   {"CNN10", 76, 66, 1},  {"CNN11", 66, 57, 1},
                                 {"CNN12", 57, 48, 1},  {"B2", 32, 32, 1},     {"Up-PS", 96, 384, 2}};
        double s32 = 0, s16 = 0, shp = 0, sh8 = 0;
        for (const Layer3& L : layers) {
            R3 r = run_conv3(L, 1024, 48, 48, 2, true, 0, false);
            bad += r.bad;
            if (strcmp(L.name, "Up-PS")) { s32 += r.ms32; s16 += r.ms16; shp += r.mshp; sh8 += r.msh8; }
        }
        printf("sum of the 12 feature / B2 3x3 layers: f32 Winograd %.3f ms   f16x3 direct %.3f ms   persistent %.3f ms   conv3_h8 %.3f ms\n", s32, s16, shp, sh8);
    }
    printf("conv3: %d failures\n", bad);
    return bad;
}
