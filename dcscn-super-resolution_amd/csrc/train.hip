// Single-GPU f32 training of the pixel-shuffler DCSCN nets (DCSCN.py:334-425, tf_graph.py:117-177); the depthwise-separable ones behind
// option "train_separable", the transposed-conv upsampler (pixel_shuffler = false) behind option "train_transposed".
//
// The training plan is its own list of layers over its own arena (TrainState); it shares only the variables with the inference
// plan.  Every conv runs as one launch of tconv_gemm (implicit GEMM on v_mfma_f32_16x16x4_f32, rows = output pixels, columns =
// output channels, k = (tap, input channel)); the data gradient is the same kernel on the filter flipped in space with Cin <-> Cout
// transposed (tpack_dgrad, repacked on the device every step) accumulating into the gradient of the layer's input; the weight
// gradient is tconv_wgrad (rows = (tap, cin), columns = cout, k = pixels) over a fixed split of the pixels, reduced in a fixed order
// by treduce_wgrad.  Concat (H_concat, Concat2 = [B2 | A1]) is a strided slice of one tensor and its gradient one of the same
// layout, so neither direction copies.  Every reduction is a fixed partition summed in a fixed order: no atomics anywhere, two
// identical runs give identical bits.
//
// A separable conv layer (tf.nn.separable_conv2d) is two stages: the depthwise k x k conv into a dense tensor d kept for the backward
// (tdw_fwd, train_dw.hpp), then all of the above with ks = 1 on d and the pointwise filter.  Backward: the pointwise weight gradient from d,
// dd = dz . P^T into a scratch by the data-gradient filter, the depthwise weight gradient from the layer's input and dd (tdw_wgrad over a fixed
// pixel split, summed by treduce_wgrad), and tdw_dgrad accumulating into the gradient of the layer's input.  Neither filter of a separable
// layer is in the l2 term (the reference sums l2_loss over the layer's unused conv_W instead): no decay in their gradients.
//
// The transposed-conv upsampler Up-TCNN (train_tconv.hpp) takes the place of the Up-PS stages: tup_fwd writes the HR activation buffer
// (no bias, no activator, no z, no depth_to_space), the gradient of that buffer is the layer's dz as it stands, tup_wgrad + treduce_wgrad
// give Tconv_W's gradient (with the l2 decay: the reference appends Tconv_W to self.Weights, tf_graph.py:235) and tup_dgrad accumulates
// into the gradient of the layer's input.  The layer is never separable and never on the split16 kernels.
//
// Variables, their gradients and the optimizer slots live in flat f32 buffers in the checkpoint (HWIO) layout, in the order of
// the graph's variable list (dcscn_tensor_info), so the update is one elementwise launch.
#include "plan.h"
#include "train_h.hpp"
#include "train_wgrad_h.hpp"
#include "train_kernels.hpp"   // the kernels, and fp contract(off) for them and everything below
#include "train_dw.hpp"
#include "train_tconv.hpp"
#include "summary.hpp"

namespace dcscn_impl {

// ---------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------
struct TBuf { int stride = 0; int res = 1; float* h = nullptr; float* g = nullptr; };

struct TLayer {
    std::string name;
    int index = 0;                 // position in the graph's layer list (dcscn_layer_info order): the dropout layer number
    int ks = 3, cin = 0, cout = 0, res = 1;
    int act = ACT_NONE; float calpha = 0.0f;
    bool dropout = false;          // has an activator (DCSCN.py: dropout follows exactly those convs)
    int in_buf = -1, in_off = 0;   // -1: the network input x
    int out_buf = -1, out_off = 0; // activation destination (act layers) / depth_to_space destination (ps > 0); -1: y_ (last layer)
    int ps = 0;                    // > 0: Up-PS conv followed by depth_to_space with this factor
    int w_t = -1, b_t = -1, a_t = -1;
    bool ds = false;               // a separable layer: ks is the depthwise filter's, w_t the pointwise filter [cin][cout], and the convs run with ks = 1 on d
    int dw_t = -1;                 // ... its depthwise filter [ks][ks][cin][1]
    int up = 0;                    // > 0: the transposed conv Up-TCNN of this stride: ks = 2 up - up % 2, cin = cout, w_t = Tconv_W [ks][ks][oc][ic], res the
                                   // input's, out_buf the HR activation buffer at res * up; no bias, no activator, no z (train_tconv.hpp)
    float* z = nullptr;            // pre-activation, dense [px, cout]
    float* d = nullptr;            // separable: the depthwise stage's output, dense [px, cin]
    // ---- the launch plan of the current carve: all that the batch shape and the two options fix (plan_layer); run_gradients only reads it ----
    int Hr = 0, Wr = 0;            // the batch's H and W at the layer's resolution
    int64_t px = 0;                // n Hr Wr pixels
    int64_t zcount = 0, wcount = 0;   // elements of z (px cout) and of the filter (ks ks cin cout; separable: the pointwise filter's cin cout)
    int64_t dcount = 0, dwcount = 0;  // separable: elements of d (px cin) and of the depthwise filter (ks ks cin)
    int dws = 0, dcw = 0; int64_t dchunk = 0;   // dw_splits: the depthwise weight gradient
    // option "train_split16" (train_h.hpp): h16 = the layer's forward and data-gradient convs run on tconv_gemm_h
    bool h16 = false;
    void *w16 = nullptr, *wd16 = nullptr;   // tpack_h images: forward, data gradient (null for a layer on the network input)
    int* e = nullptr;                       // exponents of the scales: [0] filter, [1] input slice, [2] dz
    // option "train_split16_wgrad" (train_wgrad_h.hpp): the layer's weight gradient runs on tconv_wgrad_h; it reads e[1] and e[2], which the
    // forward and the data gradient have found already when h16 is set as well
    bool wg16 = false;
    int splits = 0;                // of the weight gradient: wp's (wg16), else wgrad_splits' with `chunk` pixels each
    int64_t chunk = 0;
    TWgradHPlan wp{};
    int cs = 0; int64_t cchunk = 0;   // col_splits: the bias and PReLU-slope gradients
    int gks() const { return ds ? 1 : ks; }   // the kernel size of the layer's GEMM convs
};

// the variables the l2 term sums over: the filters, not biases or prelu slopes
// (Tconv_W as well: tf_graph.py:235 appends it to self.Weights, which DCSCN.py:350 sums)
static bool ends_with(const std::string& name, const char* tail) { const size_t n = strlen(tail); return name.size() >= n && name.compare(name.size() - n, n, tail) == 0; }
static bool is_conv_w(const std::string& name) { return ends_with(name, "/conv_W") || ends_with(name, "/Tconv_W"); }

static constexpr int kLossBlocks = 256, kNormBlocks = 256, kW2Blocks = 32;   // (kW2Blocks: per conv_W tensor, for the l2 term)

struct TrainState {
    dcscn_train_config tc{};
    std::vector<TBuf> bufs;
    std::vector<TLayer> layers;
    std::vector<int64_t> off;      // flat offset of every variable (h->tensors order)
    int64_t count = 0;
    float *d_w = nullptr, *d_g = nullptr, *d_m = nullptr, *d_v = nullptr, *d_wd = nullptr, *d_pw = nullptr;
    float h_pw[2] = {0.0f, 0.0f};
    // arena for the current batch shape
    void* arena = nullptr; size_t arena_bytes = 0;
    int n = 0, H = 0, W = 0;
    bool h16 = false;              // the carve holds the filter images and exponents of option "train_split16"
    bool wg16 = false;             // ... the exponents and the partial sums of option "train_split16_wgrad"
    unsigned* absmax = nullptr;    // kAbsMaxBlocks partial maxima (launch_texp)
    float *dz = nullptr, *at = nullptr, *part = nullptr, *col = nullptr, *zlast = nullptr, *clip = nullptr;
    float* dd = nullptr;           // separable layers: the gradient of d (the largest px cin of them)
    float *io_x = nullptr, *io_x2 = nullptr, *io_y = nullptr;
    double *dpart = nullptr, *d_stats = nullptr;
    int w2_blocks = 0;
    std::vector<double> stats_host;
    bool stepped = false;          // a step has changed the variables since the inference plan was last packed
    // dcscn_train_apply_records: [kNormBlocks] norm partials | 4 stats | clip (float) | ok (int) | [world] rank weights, as doubles
    double* d_red = nullptr; size_t red_cap = 0;
    hipEvent_t join_ev = nullptr;  // join_stream's event, made on first use
    // dcscn_train_log_pass (the end of this file): the summarised tensors by name, their records as the last pass left them on the host
    // ([names] dcscn_summary | [names][kSummaryBuckets] int64), and the device buffer they are reduced into (the same, then the scratch)
    std::vector<std::string> sum_names;
    std::map<std::string, int> sum_index;
    std::vector<char> sum_host;
    char* sum_dev = nullptr; size_t sum_cap = 0;
    bool sum_valid = false;        // a log pass has filled sum_host
    bool acts_valid = false;       // the arena holds that pass's activations and y_ (in `at`): until the next prepare_step
};

static int grid1(int64_t n) { return (int)((n + 255) / 256); }

static int tensor_of(dcscn_ctx* h, const std::string& name) {
    auto it = h->tensor_index.find(name);
    return it == h->tensor_index.end() ? -1 : it->second;
}

// the training graph of build_graph (graph.hip), without the launch-level rewrites
static int build_train_plan(dcscn_ctx* h, TrainState* t) {
    const dcscn_config& c = h->cfg;
    float ca = 0.0f;
    const int act = kernel_act(c.activator, &ca);
    const bool ds = c.depthwise_separable != 0;
    auto add_buf = [&](int stride, int res) { TBuf b; b.stride = stride; b.res = res; t->bufs.push_back(b); return (int)t->bufs.size() - 1; };
    auto add_layer = [&](const std::string& var, const std::string& short_name, int in_buf, int in_off, int cin, int ks, int cout, bool has_act,
                         int out_buf, int out_off, int ps, int res, bool ds) -> int {
        TLayer L;
        L.name = var; L.index = (int)t->layers.size(); L.ks = ks; L.cin = cin; L.cout = cout; L.res = res;
        L.act = has_act ? act : ACT_NONE; L.calpha = has_act ? ca : 0.0f; L.dropout = has_act;
        L.in_buf = in_buf; L.in_off = in_off; L.out_buf = out_buf; L.out_off = out_off; L.ps = ps;
        L.ds = ds;
        L.w_t = tensor_of(h, var + (ds ? "/pointwise_W" : "/conv_W"));
        if (ds && (L.dw_t = tensor_of(h, var + "/depthwise_W")) < 0)
            return fail(h, DCSCN_ERR_UNSUPPORTED, "training: layer %s has no depthwise_W variable", var.c_str());
        L.b_t = tensor_of(h, var + "/conv_B");
        if (has_act && c.activator == DCSCN_ACT_PRELU) L.a_t = tensor_of(h, var + "/prelu/" + short_name + "_prelu");
        if (L.w_t < 0 || (has_act && c.activator == DCSCN_ACT_PRELU && L.a_t < 0))
            return fail(h, DCSCN_ERR_UNSUPPORTED, "training: layer %s has no conv_W (pointwise_W) / prelu variable", var.c_str());
        t->layers.push_back(L);
        return DCSCN_OK;
    };
    int rc;
    int total = 0;
    std::vector<int> off(c.layers);
    for (int i = 0; i < c.layers; ++i) { off[i] = total; total += h->sched[i]; }
    const int cat = add_buf(total, 1);
    int in_buf = -1, in_off = 0, cin = c.channels;
    for (int i = 0; i < c.layers; ++i) {
        const std::string nm = "CNN" + std::to_string(i + 1);
        if ((rc = add_layer(nm, nm, in_buf, in_off, cin, c.cnn_size, h->sched[i], true, cat, off[i], 0, 1, ds))) return rc;
        in_buf = cat; in_off = off[i]; cin = h->sched[i];
    }
    if (c.use_nin) {
        const int na = c.nin_filters, nb = c.nin_filters2;
        const int t1 = add_buf(nb, 1), t2 = add_buf(nb + na, 1);
        if ((rc = add_layer("A1", "A1", cat, 0, total, 1, na, true, t2, nb, 0, 1, ds))) return rc;
        if ((rc = add_layer("B1", "B1", cat, 0, total, 1, nb, true, t1, 0, 0, 1, ds))) return rc;
        if ((rc = add_layer("B2", "B2", t1, 0, nb, 3, nb, true, t2, 0, 0, 1, ds))) return rc;       // (3x3 whatever cnn_size); Concat2 = [B2 | A1]
        in_buf = t2; in_off = 0; cin = nb + na;
    } else if (c.legacy_no_c) {
        in_buf = cat; in_off = 0; cin = total;
    } else {
        const int tc = add_buf(c.filters, 1);
        if ((rc = add_layer("C", "C", cat, 0, total, 1, c.filters, true, tc, 0, 0, 1, ds))) return rc;
        in_buf = tc; in_off = 0; cin = c.filters;
    }
    const int ps_out = c.pixel_shuffler_filters != 0 ? c.pixel_shuffler_filters : cin;
    struct Stage { const char* name; int s; int cout; };
    std::vector<Stage> stages;
    if (c.pixel_shuffler) {   // (else: no stages, Up-TCNN below)
        if (c.scale == 4) { stages.push_back({"Up-PS", 2, cin}); stages.push_back({"Up-PS2", 2, ps_out}); }
        else stages.push_back({"Up-PS", c.scale, ps_out});
    }
    int res = 1;
    if (!c.pixel_shuffler) {
        // build_transposed_conv("Up-TCNN", H[-1], scale, channels): one stage for any scale, C -> C, in place of the Up-PS stages
        TLayer L;
        L.name = "Up-TCNN"; L.index = (int)t->layers.size(); L.up = c.scale; L.ks = 2 * c.scale - c.scale % 2; L.cin = L.cout = cin; L.res = res;
        L.in_buf = in_buf; L.in_off = in_off; L.out_buf = add_buf(cin, res * c.scale);
        if ((L.w_t = tensor_of(h, "Up-TCNN/Tconv_W")) < 0) return fail(h, DCSCN_ERR_UNSUPPORTED, "training: layer Up-TCNN has no Tconv_W variable");
        t->layers.push_back(L);
        in_buf = L.out_buf; in_off = 0; res *= c.scale;
    }
    for (const Stage& st : stages) {
        const int ub = add_buf(st.cout, res * st.s);
        const std::string var = std::string(st.name) + "/" + st.name + "_CNN";
        if ((rc = add_layer(var, std::string(st.name) + "_CNN", in_buf, in_off, cin, c.cnn_size, st.s * st.s * st.cout, false, ub, 0, st.s, res, ds))) return rc;
        in_buf = ub; in_off = 0; cin = st.cout; res *= st.s;
    }
    const int rl = std::max(c.reconstruct_layers, 1);
    for (int i = 0; i < rl - 1; ++i) {
        const std::string nm = "R-CNN" + std::to_string(i + 1);
        const int rb = add_buf(c.reconstruct_filters, res);
        if ((rc = add_layer(nm, nm, in_buf, in_off, cin, c.cnn_size, c.reconstruct_filters, true, rb, 0, 0, res, false))) return rc;   // (plain convs even in a separable net, DCSCN.py:313-316)
        in_buf = rb; in_off = 0; cin = c.reconstruct_filters;
    }
    const std::string nm = "R-CNN" + std::to_string(rl);
    if ((rc = add_layer(nm, nm, in_buf, in_off, cin, c.cnn_size, 1, false, -1, 0, 0, res, ds))) return rc;
    if (t->layers.size() != h->layers.size()) return fail(h, DCSCN_ERR_UNSUPPORTED, "training: internal layer count mismatch");
    return DCSCN_OK;
}

// wgrad split of a layer: fixed by the shape alone
static int wgrad_splits(const TLayer& L, int64_t P, int64_t* chunk) {
    const int64_t tiles = (int64_t)((L.gks() * L.gks() * L.cin + 31) / 32) * ((L.cout + 31) / 32);
    int64_t s = std::max<int64_t>(1, std::min<int64_t>((2048 + tiles - 1) / tiles, (P + 1023) / 1024));
    // a separable layer's pointwise filter is a tile or a few: half the pixels per split, so that twice the workgroups share the k loop, and
    // at most 256 splits for treduce_wgrad to sum
    if (L.ds) s = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((2048 + tiles - 1) / tiles, 256), (P + 511) / 512));
    int64_t ch = ((P + s - 1) / s + 15) / 16 * 16;
    s = (P + ch - 1) / ch;
    *chunk = ch;
    return (int)s;
}
static int col_splits(int64_t P, int64_t* chunk) {
    int64_t s = std::max<int64_t>(1, std::min<int64_t>(64, (P + 4095) / 4096));
    *chunk = (P + s - 1) / s;
    return (int)s;
}

// Where a layer's kernels and splits are decided: once per carve, from the batch shape and the two options.
static void plan_layer(TLayer& L, int n, int H, int W, bool h16, bool wg16) {
    L.Hr = H * L.res; L.Wr = W * L.res;
    L.px = (int64_t)n * L.Hr * L.Wr;
    L.zcount = L.up > 0 ? 0 : L.px * L.cout;                      // (Up-TCNN writes its output buffer: no z)
    L.wcount = (int64_t)L.gks() * L.gks() * L.cin * L.cout;
    const bool wide = !L.ds && L.up == 0 && tconv_h_eligible(L.cin, L.cout);   // separable layers and Up-TCNN stay on the f32 kernels
    L.h16 = h16 && wide;
    L.wg16 = wg16 && wide;
    if (L.wg16) { L.wp = twgrad_h_plan(L.ks, L.cin, L.cout, n, L.Hr, L.Wr); L.splits = L.wp.splits; }
    else L.splits = wgrad_splits(L, L.px, &L.chunk);
    L.cs = col_splits(L.px, &L.cchunk);
    if (L.ds) {
        L.dcount = L.px * L.cin;
        L.dwcount = (int64_t)L.ks * L.ks * L.cin;
        L.dws = dw_splits(L.cin, L.px, &L.dcw, &L.dchunk);
    }
}

// Walks the arena in its order: every take rounds `words` 4-byte words up to 256 bytes.  Without a base it only sizes; with one it binds
// the slot as well.  A buffer that is not present takes nothing and binds null.
struct Carver {
    char* base;
    size_t bytes = 0;
    template <class T>
    void take(T*& slot, size_t words, bool present = true) {
        if (base) slot = present ? (T*)(base + bytes) : nullptr;
        if (present) bytes += (words * 4 + 255) / 256 * 256;
    }
};

static int carve(dcscn_ctx* h, TrainState* t, int n, int H, int W) {
    const bool h16 = h->train_split16, wg16 = h->train_split16_wgrad;
    if (t->arena && t->n == n && t->H == H && t->W == W && t->h16 == h16 && t->wg16 == wg16) return DCSCN_OK;
    // the plan goes into a copy, committed with the new arena: a carve refused for its size leaves the present one as it is
    std::vector<TLayer> layers = t->layers;
    size_t dz_max = 0, part_max = 0, col_max = 0, dd_max = 0;
    for (TLayer& L : layers) {
        plan_layer(L, n, H, W, h16, wg16);
        dz_max = std::max(dz_max, (size_t)L.zcount);
        part_max = std::max({part_max, (size_t)L.splits * L.wcount, (size_t)L.dws * L.dwcount});
        dd_max = std::max(dd_max, (size_t)L.dcount);
        col_max = std::max(col_max, (size_t)L.cs * L.cout);
    }
    const size_t P = (size_t)n * H * W, hr = P * h->cfg.scale * h->cfg.scale;
    // the arena: every buffer once, in arena order
    auto lay_out = [&](Carver c) {
        for (TBuf& b : t->bufs) {
            const size_t count = P * b.res * b.res * b.stride;
            c.take(b.h, count);
            c.take(b.g, count);
        }
        for (TLayer& L : layers) c.take(L.z, (size_t)L.zcount, L.zcount > 0);
        for (TLayer& L : layers) c.take(L.d, (size_t)L.dcount, L.ds);
        c.take(t->dd, dd_max, dd_max > 0);
        c.take(t->dz, dz_max); c.take(t->at, dz_max); c.take(t->part, part_max); c.take(t->col, col_max);
        c.take(t->io_x, P); c.take(t->io_x2, hr); c.take(t->io_y, hr); c.take(t->clip, 4);
        c.take(t->dpart, 2 * (2 * kLossBlocks + (size_t)t->w2_blocks + kNormBlocks) + 16);   // doubles: the partials, then d_stats
        // option "train_split16": both filter images of every layer on tconv_gemm_h
        for (TLayer& L : layers) {
            c.take(L.w16, tpack_h_bytes(L.ks * L.ks, L.cin, L.cout) / 4, L.h16);
            c.take(L.wd16, tpack_h_bytes(L.ks * L.ks, L.cout, L.cin) / 4, L.h16 && L.in_buf >= 0);
        }
        // either option reads exponents: three per layer, and the partial maxima behind them
        int* e = nullptr;
        c.take(e, 3 * layers.size(), h16 || wg16);
        c.take(t->absmax, kAbsMaxBlocks, h16 || wg16);
        for (size_t l = 0; l < layers.size(); ++l) layers[l].e = e && (layers[l].h16 || layers[l].wg16) ? e + 3 * l : nullptr;
        return c.bytes;
    };
    const size_t bytes = lay_out(Carver{nullptr});
    if ((int64_t)bytes > h->workspace_budget)
        return fail(h, DCSCN_ERR_NOMEM, "training batch %d x %d x %d needs %zu bytes of workspace, over the budget of %lld (training does not tile)",
                    n, H, W, bytes, (long long)h->workspace_budget);
    if (t->arena) { (void)hipStreamSynchronize(h->stream); HIP_TRY(h, hipFree(t->arena)); t->arena = nullptr; }
    hipError_t e = hipMalloc(&t->arena, bytes);
    if (e != hipSuccess) { t->arena = nullptr; return fail(h, DCSCN_ERR_NOMEM, "training workspace of %zu bytes: %s", bytes, hipGetErrorString(e)); }
    t->arena_bytes = bytes;
    lay_out(Carver{static_cast<char*>(t->arena)});
    t->layers.swap(layers);
    t->h16 = h16; t->wg16 = wg16;
    t->d_stats = t->dpart + 2 * kLossBlocks + t->w2_blocks + kNormBlocks;
    t->zlast = t->layers.back().z;
    t->n = n; t->H = H; t->W = W;
    return DCSCN_OK;
}

#define KTRY(h, launch)                                                                                \
    do {                                                                                               \
        launch;                                                                                        \
        hipError_t e_ = hipGetLastError();                                                             \
        if (e_ != hipSuccess) return fail(h, DCSCN_ERR_HIP, "%s: %s", #launch, hipGetErrorString(e_)); \
    } while (0)

// One conv of layer L: the forward (dgrad = false: dst = conv of src by the filter, + bias) or the data gradient (dst += conv of src = dz by
// the filter flipped in space with cin <-> cout swapped), on tconv_gemm or, for L.h16, on tconv_gemm_h.  tconv_gemm_h reads the exponent of
// src's scale: it is found here first, except dz's when the layer's weight gradient (wg16, which runs before) has found it already.
static int launch_layer_conv(dcscn_ctx* h, TrainState* t, const TLayer& L, bool dgrad, const float* src, int src_stride, float* dst, int dst_stride,
                             hipStream_t st) {
    const int K = dgrad ? L.cout : L.cin, N = dgrad ? L.cin : L.cout;
    const float* bias = !dgrad && L.b_t >= 0 ? t->d_w + t->off[L.b_t] : nullptr;
    if (L.h16) {
        int* e_src = L.e + (dgrad ? 2 : 1);
        if (!(dgrad && L.wg16)) KTRY(h, launch_texp(src, src_stride, K, L.px, t->absmax, e_src, st));
        TConvHArgs a{src, src_stride, K, t->n, L.Hr, L.Wr, L.ks, dgrad ? L.wd16 : L.w16, N, bias, dst, dst_stride, e_src, L.e};
        KTRY(h, launch_tconv_gemm_h(a, dgrad ? 1 : 0, st));
        return DCSCN_OK;
    }
    TConvArgs a{src, src_stride, K, t->n, L.Hr, L.Wr, L.gks(), (dgrad ? t->d_wd : t->d_w) + t->off[L.w_t], N, bias, dst, dst_stride};
    dim3 grid((unsigned)((L.px + 127) / 128), (unsigned)((N + 31) / 32));
    if (dgrad && L.ds) KTRY(h, hipLaunchKernelGGL(tconv_gemm<0>, grid, dim3(256), 0, st, a));   // dd = dz . P^T: written, not accumulated
    else if (dgrad) KTRY(h, hipLaunchKernelGGL(tconv_gemm<1>, grid, dim3(256), 0, st, a));
    else KTRY(h, hipLaunchKernelGGL(tconv_gemm<0>, grid, dim3(256), 0, st, a));
    return DCSCN_OK;
}

// grad_dst[co] = the sum over the layer's pixels of src[p][co] (bias gradient from dz, PReLU-slope gradient from at): a fixed split, then its sum
static int launch_col_grad(dcscn_ctx* h, TrainState* t, const TLayer& L, const float* src, float* grad_dst, hipStream_t st) {
    KTRY(h, hipLaunchKernelGGL(tcol_partial, dim3(L.cout, L.cs), dim3(256), 0, st, src, L.cout, L.px, L.cchunk, t->col));
    KTRY(h, hipLaunchKernelGGL(tcol_final, dim3(grid1(L.cout)), dim3(256), 0, st, (const float*)t->col, L.cout, L.cs, grad_dst));
    return DCSCN_OK;
}

// the global norm's partial sums of d_g (tsumsq over kNormBlocks blocks) into g2p
static int launch_grad_norm(dcscn_ctx* h, TrainState* t, double* g2p, hipStream_t st) {
    KTRY(h, hipLaunchKernelGGL(tsumsq, dim3(kNormBlocks), dim3(256), 0, st, (const float*)t->d_g, t->count, (t->count + kNormBlocks - 1) / kNormBlocks, g2p));
    return DCSCN_OK;
}

// forward + backward of one step (gradients into d_g, stats into d_stats); no host synchronisation
// (dropout_on = false: the log pass, which runs the graph with dropout = 1.0 whatever keep_prob the handle trains with)
static int run_gradients(dcscn_ctx* h, TrainState* t, const float* x, const float* x2, const float* yt, uint64_t key, hipStream_t st,
                         int64_t first_index = 0, bool dropout_on = true) {
    const dcscn_train_config& tc = t->tc;
    const int n = t->n;
    const int64_t P = (int64_t)n * t->H * t->W;
    const bool drop = dropout_on && tc.keep_prob < 1.0;
    const float keep = (float)tc.keep_prob;
    const uint32_t thresh = drop ? (uint32_t)std::min(16777216.0, std::floor(tc.keep_prob * 16777216.0)) : 0u;
    auto in_ptr = [&](const TLayer& L, float** g) -> const float* {
        if (L.in_buf < 0) { *g = nullptr; return x; }
        const TBuf& b = t->bufs[L.in_buf];
        *g = b.g + L.in_off;
        return b.h + L.in_off;
    };
    auto in_stride = [&](const TLayer& L) { return L.in_buf < 0 ? 1 : t->bufs[L.in_buf].stride; };
    auto var = [&](int tensor) -> float* { return tensor >= 0 ? t->d_w + t->off[tensor] : nullptr; };   // a variable in d_w; null: the layer has none
    // the index of the layer's first activation within the global batch's (the dropout mask is the whole batch's)
    auto idx0 = [&](const TLayer& L) { return (uint64_t)first_index * (uint64_t)(L.px / n * L.cout); };
    int rc;

    // dgrad filters of the current weights
    for (const TLayer& L : t->layers) {
        if (L.h16) {   // the scaled f16 images of both directions instead
            KTRY(h, launch_texp(var(L.w_t), 1, 1, L.wcount, t->absmax, L.e, st));
            KTRY(h, launch_tpack_h(var(L.w_t), L.ks * L.ks, L.cin, L.cout, L.e, L.w16, L.wd16, st));
            continue;
        }
        KTRY(h, hipLaunchKernelGGL(tpack_dgrad, dim3(grid1(L.wcount)), dim3(256), 0, st, var(L.w_t), L.gks() * L.gks(), L.cin, L.cout, t->d_wd + t->off[L.w_t]));
    }
    // ---- forward ----
    for (const TLayer& L : t->layers) {
        float* gdummy;
        const float* in = in_ptr(L, &gdummy);
        if (L.up > 0) {   // Up-TCNN: one GEMM per output phase, straight into the HR activation buffer
            const TUpArgs ua{const_cast<float*>(in), in_stride(L), L.cin, n, L.Hr, L.Wr, L.up, L.ks, t->d_wd + t->off[L.w_t], t->bufs[L.out_buf].h, 0, nullptr};
            KTRY(h, hipLaunchKernelGGL(tup_fwd, dim3((unsigned)((L.px + 127) / 128), (L.cout + 31) / 32, L.up * L.up), dim3(256), 0, st, ua));
            continue;
        }
        if (L.ds) {   // the depthwise stage into d; the pointwise conv reads d
            const TDwArgs da{in, in_stride(L), L.cin, n, L.Hr, L.Wr, L.ks, var(L.dw_t)};
            KTRY(h, hipLaunchKernelGGL(tdw_fwd, dim3(grid1(L.dcount)), dim3(256), 0, st, da, L.d));
            if ((rc = launch_layer_conv(h, t, L, false, L.d, L.cin, L.z, L.cout, st))) return rc;
        } else if ((rc = launch_layer_conv(h, t, L, false, in, in_stride(L), L.z, L.cout, st))) return rc;
        if (L.dropout) {
            const TBuf& ob = t->bufs[L.out_buf];
            KTRY(h, hipLaunchKernelGGL(tact_fwd, dim3(grid1(L.zcount)), dim3(256), 0, st, L.z, L.cout, L.px, var(L.a_t), L.calpha, L.act, ob.h + L.out_off,
                                       ob.stride, dropout_layer_key(key, L.index), idx0(L), thresh, keep, drop ? 1 : 0));
        } else if (L.ps > 0) {
            const TBuf& ob = t->bufs[L.out_buf];
            const int C = L.cout / (L.ps * L.ps);
            KTRY(h, hipLaunchKernelGGL(td2s, dim3(grid1(L.zcount)), dim3(256), 0, st, (const float*)L.z, ob.h, n, L.Hr, L.Wr, L.ps, C, 0));
        }
    }
    // ---- loss ----
    const int64_t cnt = P * h->cfg.scale * h->cfg.scale;
    for (const TBuf& b : t->bufs) HIP_TRY(h, hipMemsetAsync(b.g, 0, (size_t)P * b.res * b.res * b.stride * 4, st));
    const int64_t lchunk = (cnt + kLossBlocks - 1) / kLossBlocks;
    KTRY(h, hipLaunchKernelGGL(tloss, dim3(kLossBlocks), dim3(256), 0, st, (const float*)t->zlast, x2, yt, cnt, lchunk, tc.use_l1_loss, t->dz, t->dpart));
    // ---- backward, layers in reverse ----
    for (int l = (int)t->layers.size() - 1; l >= 0; --l) {
        const TLayer& L = t->layers[l];
        float* gin;
        const float* in = in_ptr(L, &gin);
        const bool prelu = L.a_t >= 0;
        if (L.up > 0) {
            // Up-TCNN: dz is the gradient of its output buffer as it stands; Tconv_W's gradient (+ l2_decay * W), then the data gradient
            float* dout = t->bufs[L.out_buf].g;
            const TUpArgs wa{const_cast<float*>(in), in_stride(L), L.cin, n, L.Hr, L.Wr, L.up, L.ks, nullptr, dout, L.chunk, t->part};
            KTRY(h, hipLaunchKernelGGL(tup_wgrad, dim3((L.ks * L.ks * L.cout + 31) / 32, (L.cin + 31) / 32, L.splits), dim3(256), 0, st, wa));
            KTRY(h, hipLaunchKernelGGL(treduce_wgrad, dim3(grid1(L.wcount)), dim3(256), 0, st, (const float*)t->part, L.splits, L.wcount, (const float*)var(L.w_t),
                                       (float)tc.l2_decay, t->d_g + t->off[L.w_t]));
            const TUpArgs ga{gin, in_stride(L), L.cin, n, L.Hr, L.Wr, L.up, L.ks, var(L.w_t), dout, 0, nullptr};
            KTRY(h, hipLaunchKernelGGL(tup_dgrad, dim3((unsigned)((L.px + 127) / 128), (L.cin + 31) / 32), dim3(256), 0, st, ga));
            continue;
        }
        if (L.dropout) {
            const TBuf& ob = t->bufs[L.out_buf];
            KTRY(h, hipLaunchKernelGGL(tact_bwd, dim3(grid1(L.zcount)), dim3(256), 0, st, (const float*)(ob.g + L.out_off), ob.stride, (const float*)L.z, L.cout,
                                       L.px, var(L.a_t), L.calpha, L.act, dropout_layer_key(key, L.index), idx0(L), thresh, keep, drop ? 1 : 0, t->dz,
                                       prelu ? t->at : nullptr));
        } else if (L.ps > 0) {
            const TBuf& ob = t->bufs[L.out_buf];
            const int C = L.cout / (L.ps * L.ps);
            KTRY(h, hipLaunchKernelGGL(td2s, dim3(grid1(L.zcount)), dim3(256), 0, st, (const float*)t->dz, (float*)ob.g, n, L.Hr, L.Wr, L.ps, C, 1));
        }   // (the last layer: dz is the loss gradient already)
        // weight gradient (+ l2_decay * W)
        if (L.wg16) {
            // e[1] is the forward's when the layer's convs run on tconv_gemm_h; e[2] is found here, once, for this launch and the data gradient's
            if (!L.h16) KTRY(h, launch_texp(in, in_stride(L), L.cin, L.px, t->absmax, L.e + 1, st));
            KTRY(h, launch_texp(t->dz, L.cout, L.cout, L.px, t->absmax, L.e + 2, st));
            const TWgradHArgs wa{in, in_stride(L), L.cin, n, L.Hr, L.Wr, L.ks, t->dz, L.cout, L.e + 1, L.e + 2, t->part};
            const hipError_t we = launch_tconv_wgrad_h(wa, L.wp, st);
            if (we != hipSuccess) return fail(h, DCSCN_ERR_HIP, "tconv_wgrad_h (%s, %zu bytes of LDS): %s", L.name.c_str(), L.wp.lds_bytes, hipGetErrorString(we));
        } else {
            // (separable: the pointwise filter's, from d)
            TWgradArgs wa{L.ds ? L.d : in, L.ds ? L.cin : in_stride(L), L.cin, n, L.Hr, L.Wr, L.gks(), t->dz, L.cout, L.chunk, t->part};
            KTRY(h, hipLaunchKernelGGL(tconv_wgrad, dim3((L.gks() * L.gks() * L.cin + 31) / 32, (L.cout + 31) / 32, L.splits), dim3(256), 0, st, wa));
        }
        KTRY(h, hipLaunchKernelGGL(treduce_wgrad, dim3(grid1(L.wcount)), dim3(256), 0, st, (const float*)t->part, L.splits, L.wcount, (const float*)var(L.w_t),
                                   L.ds ? 0.0f : (float)tc.l2_decay, t->d_g + t->off[L.w_t]));
        // bias and PReLU-alpha gradients
        if (L.b_t >= 0 && (rc = launch_col_grad(h, t, L, t->dz, t->d_g + t->off[L.b_t], st))) return rc;
        if (prelu && (rc = launch_col_grad(h, t, L, t->at, t->d_g + t->off[L.a_t], st))) return rc;
        // data gradient, accumulated into the input's gradient (none for the network input)
        if (L.ds) {
            // dd = dz . P^T, the depthwise filter's gradient from the input and dd (no decay), then the depthwise data gradient into gin
            if ((rc = launch_layer_conv(h, t, L, true, t->dz, L.cout, t->dd, L.cin, st))) return rc;
            const TDwArgs wa{in, in_stride(L), L.cin, n, L.Hr, L.Wr, L.ks, var(L.dw_t)};
            KTRY(h, hipLaunchKernelGGL(tdw_wgrad, dim3(L.ks * L.ks, (L.cin + L.dcw - 1) / L.dcw, L.dws), dim3(256), 0, st, wa, (const float*)t->dd, L.dcw,
                                       L.dchunk, t->part));
            KTRY(h, hipLaunchKernelGGL(treduce_wgrad, dim3(grid1(L.dwcount)), dim3(256), 0, st, (const float*)t->part, L.dws, L.dwcount,
                                       (const float*)var(L.dw_t), 0.0f, t->d_g + t->off[L.dw_t]));
            if (gin) {
                const TDwArgs ga{gin, in_stride(L), L.cin, n, L.Hr, L.Wr, L.ks, var(L.dw_t)};
                KTRY(h, hipLaunchKernelGGL(tdw_dgrad, dim3(grid1(L.dcount)), dim3(256), 0, st, ga, (const float*)t->dd));
            }
        } else if (gin && (rc = launch_layer_conv(h, t, L, true, t->dz, L.cout, gin, in_stride(L), st))) return rc;
    }
    // ---- l2 term, global norm, stats ----
    double* w2p = t->dpart + 2 * kLossBlocks;
    int slot = 0;
    for (size_t i = 0; i < h->tensors.size(); ++i) {
        if (!is_conv_w(h->tensors[i].name)) continue;
        const int64_t c = (int64_t)h->tensors[i].data.size();
        KTRY(h, hipLaunchKernelGGL(tsumsq, dim3(kW2Blocks), dim3(256), 0, st, (const float*)(t->d_w + t->off[i]), c, (c + kW2Blocks - 1) / kW2Blocks,
                                   w2p + slot));
        slot += kW2Blocks;
    }
    double* g2p = w2p + t->w2_blocks;
    if ((rc = launch_grad_norm(h, t, g2p, st))) return rc;
    KTRY(h, hipLaunchKernelGGL(tstats, dim3(1), dim3(256), 0, st, (const double*)t->dpart, kLossBlocks, (const double*)w2p, slot, (const double*)g2p, kNormBlocks,
                               cnt, tc.use_l1_loss, tc.l2_decay, tc.clipping_norm, t->d_stats, t->clip));
    return DCSCN_OK;
}

// the three optimizers behind option "train_optimizers" (topt_more)
static bool more_optimizer(int kind) { return kind == DCSCN_OPTIMIZER_ADADELTA || kind == DCSCN_OPTIMIZER_ADAGRAD || kind == DCSCN_OPTIMIZER_RMSPROP; }

// the optimizer step on d_g scaled by clip[0]; ok: null, or a reduction's device flag that gates it (topt, topt_more)
static int apply_update(dcscn_ctx* h, TrainState* t, double lr, const float* clip, const int* ok, hipStream_t st) {
    const dcscn_train_config& tc = t->tc;
    if (more_optimizer(tc.optimizer)) {   // option "train_optimizers": adadelta, adagrad, rmsprop
        KTRY(h, hipLaunchKernelGGL(topt_more, dim3(grid1(t->count)), dim3(256), 0, st, ok, tc.optimizer, t->d_w, (const float*)t->d_g, t->d_m, t->d_v, t->count,
                                   clip, (float)lr, (float)tc.momentum));
        t->stepped = true;
        return DCSCN_OK;
    }
    KTRY(h, hipLaunchKernelGGL(topt, dim3(grid1(t->count)), dim3(256), 0, st, ok, tc.optimizer, t->d_w, (const float*)t->d_g, t->d_m, t->d_v, t->count, clip,
                               (const float*)t->d_pw, (float)lr, (float)tc.beta1, (float)tc.beta2, (float)tc.epsilon, (float)tc.momentum));
    if (tc.optimizer == DCSCN_OPTIMIZER_ADAM) KTRY(h, hipLaunchKernelGGL(tpowers, dim3(1), dim3(1), 0, st, ok, t->d_pw, (float)tc.beta1, (float)tc.beta2));
    t->stepped = true;
    return DCSCN_OK;
}

static int check_step(dcscn_ctx* h, const void* x, const void* x2, const void* y, int n, int H, int W) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    if (!h->finalized) return fail(h, DCSCN_ERR_STATE, "training step before dcscn_finalize");
    if (!h->train) return fail(h, DCSCN_ERR_STATE, "training step before dcscn_train_begin");
    if (!x || !x2 || !y) return fail(h, DCSCN_ERR_INVALID_ARG, "training step: null buffer");
    if (n < 1 || H < 1 || W < 1) return fail(h, DCSCN_ERR_INVALID_ARG, "training step: bad shape %d x %d x %d", n, H, W);
    return DCSCN_OK;
}

// the four doubles of a step's stats (tstats) to the caller, who asked for them: synchronises `st`; stats == nullptr: nothing, the step stays enqueued
static int read_stats(dcscn_ctx* h, TrainState* t, double* stats, hipStream_t st) {
    if (!stats) return DCSCN_OK;
    HIP_TRY(h, hipMemcpyAsync(stats, t->d_stats, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return DCSCN_OK;
}

// The one step sequence.  Every gradient entry point reads: validate -> prepare_step -> its inputs -> run_gradients -> finish_update (a step) or
// write_record (a data-parallel rank).
//
// prepare_step, behind the validation: the device, the arena of the batch shape, the stream the step runs on (null: the handle's)
static int prepare_step(dcscn_ctx* h, int n, int H, int W, void* stream, TrainState** t, hipStream_t* st) {
    *t = h->train;
    (*t)->acts_valid = false;   // (whatever runs next overwrites the last log pass's activations)
    HIP_TRY(h, hipSetDevice(h->device));
    *st = stream ? (hipStream_t)stream : h->stream;
    return carve(h, *t, n, H, W);
}

// the ending of a step: the update (update = false: dcscn_train_gradients stops at d_g), then the stats for a caller who asked
static int finish_update(dcscn_ctx* h, TrainState* t, bool update, double lr, double* stats, hipStream_t st) {
    int rc;
    if (update && (rc = apply_update(h, t, lr, t->clip, nullptr, st))) return rc;
    return read_stats(h, t, stats, st);
}

// later host-buffer steps, forwards and tensor reads run on the handle's stream: order it behind the caller's
static int join_stream(dcscn_ctx* h, hipStream_t st) {
    if (st == h->stream) return DCSCN_OK;
    TrainState* t = h->train;
    if (!t->join_ev) HIP_TRY(h, hipEventCreateWithFlags(&t->join_ev, hipEventDisableTiming));
    HIP_TRY(h, hipEventRecord(t->join_ev, st));
    HIP_TRY(h, hipStreamWaitEvent(h->stream, t->join_ev, 0));
    return DCSCN_OK;
}

// steps in host memory: upload, step, read the stats back
static int host_step(dcscn_ctx* h, const float* x, const float* x2, const float* y, int n, int H, int W, double lr, uint64_t key, double* stats, bool update) {
    int rc = check_step(h, x, x2, y, n, H, W);
    if (rc) return rc;
    TrainState* t;
    hipStream_t st;
    if ((rc = prepare_step(h, n, H, W, nullptr, &t, &st))) return rc;
    const int s = h->cfg.scale;
    const size_t lr_b = (size_t)n * H * W * 4, hr_b = lr_b * s * s;
    HIP_TRY(h, hipMemcpyAsync(t->io_x, x, lr_b, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(t->io_x2, x2, hr_b, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(t->io_y, y, hr_b, hipMemcpyHostToDevice, st));
    if ((rc = run_gradients(h, t, t->io_x, t->io_x2, t->io_y, key, st))) return rc;
    if ((rc = finish_update(h, t, update, lr, stats, st))) return rc;
    // only here: the uploads read the caller's buffers, so the step is done with them on return, stats (read_stats has synchronised) or not
    if (!stats) HIP_TRY(h, hipStreamSynchronize(st));
    return DCSCN_OK;
}

static int check_record(dcscn_ctx* h, const void* rec, int64_t first_index, const char* what) {
    if (!rec) return fail(h, DCSCN_ERR_INVALID_ARG, "%s: null record buffer", what);
    if ((uintptr_t)rec % 16 != 0) return fail(h, DCSCN_ERR_INVALID_ARG, "%s: the record buffer is not 16-byte aligned", what);
    if (first_index < 0) return fail(h, DCSCN_ERR_INVALID_ARG, "%s: first_index %lld < 0", what, (long long)first_index);
    return DCSCN_OK;
}

// the gradient of the batch just run (d_g) and its stats as a record at `rec`, on `st`
static int write_record(dcscn_ctx* h, TrainState* t, int n, float* rec, hipStream_t st) {
    HIP_TRY(h, hipMemcpyAsync(rec, t->d_g, (size_t)t->count * 4, hipMemcpyDeviceToDevice, st));
    KTRY(h, hipLaunchKernelGGL(trecord_tail, dim3(1), dim3(1), 0, st, rec, t->count, (const double*)t->d_stats, (double)n));
    return join_stream(h, st);
}

// dcscn_train_step_patches and dcscn_train_step_patches_aug: the batch built on the device (train_data.hip), then the step
static int step_patches(dcscn_ctx* h, PatchList patches, int n, int lr_size, double max_value, double lr, uint64_t dropout_key, double* stats) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    int rc = check_patches(h, patches, n, lr_size, max_value);
    if (rc) return rc;
    TrainState* t;
    hipStream_t st;
    if ((rc = prepare_step(h, n, lr_size, lr_size, nullptr, &t, &st))) return rc;   // the handle's stream only: nothing to join
    if ((rc = build_batch_device(h, patches, n, lr_size, max_value, t->io_x, t->io_x2, t->io_y, st))) return rc;
    if ((rc = run_gradients(h, t, t->io_x, t->io_x2, t->io_y, dropout_key, st))) return rc;
    return finish_update(h, t, true, lr, stats, st);
}

// dcscn_train_local_gradients_patches and dcscn_train_local_gradients_patches_aug
static int local_gradients_patches(dcscn_ctx* h, PatchList patches, int n, int lr_size, double max_value, uint64_t dropout_key,
                                   int64_t first_index, float* record_out, void* stream, const char* who) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    int rc = check_patches(h, patches, n, lr_size, max_value);
    if (rc) return rc;
    if ((rc = check_record(h, record_out, first_index, who))) return rc;
    TrainState* t;
    hipStream_t st;
    if ((rc = prepare_step(h, n, lr_size, lr_size, stream, &t, &st))) return rc;
    if ((rc = build_batch_device(h, patches, n, lr_size, max_value, t->io_x, t->io_x2, t->io_y, st))) return rc;
    if ((rc = run_gradients(h, t, t->io_x, t->io_x2, t->io_y, dropout_key, st, first_index))) return rc;
    return write_record(h, t, n, record_out, st);
}

// ---------------------------------------------------------------------------------------------
// log pass (include/dcscn.h: dcscn_train_log_pass)
// ---------------------------------------------------------------------------------------------
// y_ = the last layer + x2 (DCSCN.py:325); a step never stores it (tloss forms it on the fly)
__global__ void tadd_out(const float* z, const float* x2, int64_t count, float* y) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count) y[e] = z[e] + x2[e];
}

// What the reference appends to self.H for the layer: the activator's output (with dropout off: exactly that) in the layer's slice of its
// output buffer; Up-TCNN's output buffer; else the conv's output z -- for an Up-PS conv the tensor before depth_to_space.
static SummaryView output_view(const TrainState* t, const TLayer& L) {
    if (L.dropout || L.up > 0) {
        const TBuf& ob = t->bufs[L.out_buf];
        const int64_t px = L.up > 0 ? L.px * L.up * L.up : L.px;
        return SummaryView{ob.h + L.out_off, px * L.cout, L.cout, ob.stride};
    }
    return flat_view(L.z, L.zcount);
}

// "x", "y_" and "<layer>/output" of the current carve; false: no such activation
static bool activation_view(dcscn_ctx* h, const std::string& name, SummaryView* v) {
    const TrainState* t = h->train;
    if (!t) return false;
    const int64_t P = (int64_t)t->n * t->H * t->W, hr = P * h->cfg.scale * h->cfg.scale;
    if (name == "x") { *v = flat_view(t->io_x, P); return true; }
    if (name == "y_") { *v = flat_view(t->at, hr); return true; }   // (tadd_out's destination: `at` is free behind the backward pass)
    if (!ends_with(name, "/output")) return false;
    const std::string layer = name.substr(0, name.size() - 7);
    for (const TLayer& L : t->layers)
        if (L.name == layer) { *v = output_view(t, L); return true; }
    return false;
}

static int log_pass(dcscn_ctx* h, const float* x, const float* x2, const float* y, int n, int H, int W, double* stats) {
    int rc = check_step(h, x, x2, y, n, H, W);
    if (rc) return rc;
    TrainState* t;
    hipStream_t st;
    if ((rc = prepare_step(h, n, H, W, nullptr, &t, &st))) return rc;
    t->sum_valid = false;
    const int s = h->cfg.scale;
    const int64_t P = (int64_t)n * H * W, hr = P * s * s;
    HIP_TRY(h, hipMemcpyAsync(t->io_x, x, (size_t)P * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(t->io_x2, x2, (size_t)hr * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(t->io_y, y, (size_t)hr * 4, hipMemcpyHostToDevice, st));
    if ((rc = run_gradients(h, t, t->io_x, t->io_x2, t->io_y, 0, st, 0, false))) return rc;
    KTRY(h, hipLaunchKernelGGL(tadd_out, dim3(grid1(hr)), dim3(256), 0, st, (const float*)t->zlast, (const float*)t->io_x2, hr, t->at));
    if (t->sum_names.empty()) {
        for (const TensorSpec& ts : h->tensors) { t->sum_names.push_back(ts.name); t->sum_names.push_back(ts.name + "/grad"); }
        for (const TLayer& L : t->layers) t->sum_names.push_back(L.name + "/output");
        t->sum_names.push_back("x");
        t->sum_names.push_back("y_");
        for (size_t i = 0; i < t->sum_names.size(); ++i) t->sum_index[t->sum_names[i]] = (int)i;
    }
    const size_t names = t->sum_names.size(), head = names * (sizeof(dcscn_summary) + sizeof(int64_t) * kSummaryBuckets);
    if ((rc = grow(h, &t->sum_dev, &t->sum_cap, head + summary_scratch_bytes(), st))) return rc;
    HIP_TRY(h, summary_prepare_device(h->device));
    dcscn_summary* recs = reinterpret_cast<dcscn_summary*>(t->sum_dev);
    int64_t* counts = reinterpret_cast<int64_t*>(t->sum_dev + names * sizeof(dcscn_summary));
    HIP_TRY(h, hipMemsetAsync(t->sum_dev, 0, head, st));
    size_t r = 0;
    auto reduce = [&](const SummaryView& v) {
        const hipError_t e = launch_summary(v, t->sum_dev + head, recs + r, counts + r * kSummaryBuckets, st);
        ++r;
        return e;
    };
    for (size_t i = 0; i < h->tensors.size(); ++i) {   // (the order of sum_names)
        const int64_t c = (int64_t)h->tensors[i].data.size();
        HIP_TRY(h, reduce(flat_view(t->d_w + t->off[i], c)));
        HIP_TRY(h, reduce(flat_view(t->d_g + t->off[i], c)));
    }
    for (const TLayer& L : t->layers) HIP_TRY(h, reduce(output_view(t, L)));
    HIP_TRY(h, reduce(flat_view(t->io_x, P)));
    HIP_TRY(h, reduce(flat_view(t->at, hr)));
    t->sum_host.resize(head);
    HIP_TRY(h, hipMemcpyAsync(t->sum_host.data(), t->sum_dev, head, hipMemcpyDeviceToHost, st));
    if (stats) HIP_TRY(h, hipMemcpyAsync(stats, t->d_stats, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));   // the pass's one synchronisation
    t->sum_valid = true;
    t->acts_valid = true;
    return DCSCN_OK;
}

void train_free(dcscn_ctx* h) {
    TrainState* t = h->train;
    if (!t) return;
    for (float* p : {t->d_w, t->d_g, t->d_m, t->d_v, t->d_wd, t->d_pw})
        if (p) (void)hipFree(p);
    if (t->d_red) (void)hipFree(t->d_red);
    if (t->join_ev) (void)hipEventDestroy(t->join_ev);
    if (t->sum_dev) (void)hipFree(t->sum_dev);
    if (t->arena) (void)hipFree(t->arena);
    delete t;
    h->train = nullptr;
}

// Before a forward on a handle whose variables a training step changed: bring them to the host copies and repack the inference plan.
int train_sync_inference(dcscn_ctx* h) {
    TrainState* t = h->train;
    if (!t || !t->stepped) return DCSCN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<float> host((size_t)t->count);
    HIP_TRY(h, hipMemcpy(host.data(), t->d_w, host.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h->tensors.size(); ++i) {
        TensorSpec& ts = h->tensors[i];
        std::copy(host.begin() + t->off[i], host.begin() + t->off[i] + ts.data.size(), ts.data.begin());
    }
    int rc = repack_weights(h);
    if (rc) return rc;
    t->stepped = false;
    return DCSCN_OK;
}

}  // namespace dcscn_impl

extern "C" {

int dcscn_train_begin(dcscn_handle h, const dcscn_train_config* tc) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    if (!tc) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_train_begin: null config");
    if (tc->struct_size != (int32_t)sizeof(dcscn_train_config))
        return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_train_begin: struct_size %d != %zu", tc->struct_size, sizeof(dcscn_train_config));
    if (!h->finalized) return fail(h, DCSCN_ERR_STATE, "dcscn_train_begin before dcscn_finalize");
    if (h->train) return fail(h, DCSCN_ERR_STATE, "dcscn_train_begin called twice on one handle");
    const dcscn_config& c = h->cfg;
    if (c.depthwise_separable && !h->train_separable) return fail(h, DCSCN_ERR_UNSUPPORTED, "training of depthwise separable nets is not implemented");
    if (!c.pixel_shuffler && !h->train_transposed) return fail(h, DCSCN_ERR_UNSUPPORTED, "training of the transposed-conv upsampler (pixel_shuffler = false) is not implemented");
    if (c.batch_norm) return fail(h, DCSCN_ERR_UNSUPPORTED, "batch_norm is not implemented");
    if (!(h->train_optimizers && more_optimizer(tc->optimizer))) switch (tc->optimizer) {   // option "train_optimizers" lifts the three refusals
        case DCSCN_OPTIMIZER_ADAM: case DCSCN_OPTIMIZER_GD: case DCSCN_OPTIMIZER_MOMENTUM: break;
        case DCSCN_OPTIMIZER_ADADELTA: return fail(h, DCSCN_ERR_UNSUPPORTED, "optimizer adadelta is not implemented (supported: adam, gd, momentum)");
        case DCSCN_OPTIMIZER_ADAGRAD: return fail(h, DCSCN_ERR_UNSUPPORTED, "optimizer adagrad is not implemented (supported: adam, gd, momentum)");
        case DCSCN_OPTIMIZER_RMSPROP: return fail(h, DCSCN_ERR_UNSUPPORTED, "optimizer rmsprop is not implemented (supported: adam, gd, momentum)");
        default: return fail(h, DCSCN_ERR_INVALID_ARG, "unknown optimizer %d", tc->optimizer);
    }
    if (!(tc->keep_prob > 0.0 && tc->keep_prob <= 1.0)) return fail(h, DCSCN_ERR_INVALID_ARG, "keep_prob must be in (0, 1]");
    if (tc->l2_decay < 0.0 || tc->clipping_norm < 0.0) return fail(h, DCSCN_ERR_INVALID_ARG, "l2_decay and clipping_norm must be >= 0");
    TrainState* t = new (std::nothrow) TrainState();
    if (!t) return fail(h, DCSCN_ERR_NOMEM, "out of host memory");
    t->tc = *tc;
    h->train = t;
    int rc = build_train_plan(h, t);
    if (rc) { train_free(h); return rc; }
    for (const TensorSpec& ts : h->tensors) {
        t->off.push_back(t->count);
        t->count += (int64_t)ts.data.size();
        if (is_conv_w(ts.name)) t->w2_blocks += kW2Blocks;
    }
    std::vector<float> flat((size_t)t->count);
    for (size_t i = 0; i < h->tensors.size(); ++i) std::copy(h->tensors[i].data.begin(), h->tensors[i].data.end(), flat.begin() + t->off[i]);
    const size_t bytes = (size_t)t->count * 4;
    hipError_t e = hipSetDevice(h->device);
    for (float** p : {&t->d_w, &t->d_g, &t->d_m, &t->d_v, &t->d_wd})
        if (e == hipSuccess) e = hipMalloc(p, bytes);
    if (e == hipSuccess) e = hipMalloc(&t->d_pw, 2 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(t->d_w, flat.data(), bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(t->d_g, 0, bytes);
    if (e == hipSuccess) e = hipMemset(t->d_m, 0, bytes);
    if (e == hipSuccess) e = hipMemset(t->d_v, 0, bytes);
    // TF's non-zero initial slots: <var>/Adagrad = initial_accumulator_value, <var>/RMSProp = ones (the other three start at 0)
    if (e == hipSuccess && (tc->optimizer == DCSCN_OPTIMIZER_ADAGRAD || tc->optimizer == DCSCN_OPTIMIZER_RMSPROP)) {
        std::fill(flat.begin(), flat.end(), tc->optimizer == DCSCN_OPTIMIZER_ADAGRAD ? kAdagradInitialAccumulator : kRmsPropInitialMs);
        e = hipMemcpy(t->d_m, flat.data(), bytes, hipMemcpyHostToDevice);
    }
    t->h_pw[0] = (float)tc->beta1; t->h_pw[1] = (float)tc->beta2;      // TF: beta1_power / beta2_power start at beta1 / beta2
    if (e == hipSuccess) e = hipMemcpy(t->d_pw, t->h_pw, sizeof t->h_pw, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        train_free(h);
        return fail(h, DCSCN_ERR_HIP, "dcscn_train_begin: %s", hipGetErrorString(e));
    }
    return DCSCN_OK;
}

int dcscn_train_step(dcscn_handle h, const float* x, const float* x2, const float* y_true, int n, int height, int width, double lr,
                     uint64_t dropout_key, double* stats) {
    return host_step(h, x, x2, y_true, n, height, width, lr, dropout_key, stats, true);
}

int dcscn_train_gradients(dcscn_handle h, const float* x, const float* x2, const float* y_true, int n, int height, int width,
                          uint64_t dropout_key, double* stats) {
    return host_step(h, x, x2, y_true, n, height, width, 0.0, dropout_key, stats, false);
}

int dcscn_train_log_pass(dcscn_handle h, const float* x, const float* x2, const float* y_true, int n, int height, int width, double* stats) {
    return log_pass(h, x, x2, y_true, n, height, width, stats);
}

int dcscn_summary_get(dcscn_handle h, const char* name, dcscn_summary* out, int64_t* buckets, int capacity) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    if (!name || !out) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_summary_get: null argument");
    if (buckets && capacity < kSummaryBuckets)
        return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_summary_get: room for %d bucket counts, %d needed", capacity, kSummaryBuckets);
    const TrainState* t = h->train;
    if (!t || !t->sum_valid) return fail(h, DCSCN_ERR_STATE, "dcscn_summary_get before dcscn_train_log_pass");
    const auto it = t->sum_index.find(name);
    if (it == t->sum_index.end()) return fail(h, DCSCN_ERR_SHAPE, "no summary '%s'", name);
    const size_t names = t->sum_names.size();
    memcpy(out, t->sum_host.data() + (size_t)it->second * sizeof(dcscn_summary), sizeof(dcscn_summary));
    if (buckets)
        memcpy(buckets, t->sum_host.data() + names * sizeof(dcscn_summary) + (size_t)it->second * kSummaryBuckets * sizeof(int64_t),
               kSummaryBuckets * sizeof(int64_t));
    return DCSCN_OK;
}

int dcscn_train_step_device(dcscn_handle h, const float* x, const float* x2, const float* y_true, int n, int height, int width, double lr,
                            uint64_t dropout_key, double* stats, void* stream) {
    int rc = check_step(h, x, x2, y_true, n, height, width);
    if (rc) return rc;
    TrainState* t;
    hipStream_t st;
    if ((rc = prepare_step(h, n, height, width, stream, &t, &st))) return rc;
    if ((rc = run_gradients(h, t, x, x2, y_true, dropout_key, st))) return rc;
    if ((rc = finish_update(h, t, true, lr, stats, st))) return rc;
    return join_stream(h, st);   // the step ran on the caller's stream
}

int dcscn_train_step_patches(dcscn_handle h, const dcscn_patch* patches, int n, int lr_size, double max_value, double lr, uint64_t dropout_key,
                             double* stats) {
    return step_patches(h, patches, n, lr_size, max_value, lr, dropout_key, stats);
}

int dcscn_train_step_patches_aug(dcscn_handle h, const dcscn_patch_aug* patches, int n, int lr_size, double max_value, double lr,
                                 uint64_t dropout_key, double* stats) {
    return step_patches(h, patches, n, lr_size, max_value, lr, dropout_key, stats);
}

int64_t dcscn_train_record_floats(dcscn_handle h) {
    if (!h) return 0;
    int64_t count = 0;
    for (const TensorSpec& ts : h->tensors) count += (int64_t)ts.data.size();
    return record_pad(count) + kRecordTrailer;
}

int dcscn_train_local_gradients_device(dcscn_handle h, const float* x, const float* x2, const float* y_true, int n, int height, int width,
                                       uint64_t dropout_key, int64_t first_index, float* record_out, void* stream) {
    int rc = check_step(h, x, x2, y_true, n, height, width);
    if (rc) return rc;
    if ((rc = check_record(h, record_out, first_index, "dcscn_train_local_gradients_device"))) return rc;
    TrainState* t;
    hipStream_t st;
    if ((rc = prepare_step(h, n, height, width, stream, &t, &st))) return rc;
    if ((rc = run_gradients(h, t, x, x2, y_true, dropout_key, st, first_index))) return rc;
    return write_record(h, t, n, record_out, st);
}

int dcscn_train_local_gradients_patches(dcscn_handle h, const dcscn_patch* patches, int n, int lr_size, double max_value, uint64_t dropout_key,
                                        int64_t first_index, float* record_out, void* stream) {
    return local_gradients_patches(h, patches, n, lr_size, max_value, dropout_key, first_index, record_out, stream,
                                   "dcscn_train_local_gradients_patches");
}

int dcscn_train_local_gradients_patches_aug(dcscn_handle h, const dcscn_patch_aug* patches, int n, int lr_size, double max_value,
                                            uint64_t dropout_key, int64_t first_index, float* record_out, void* stream) {
    return local_gradients_patches(h, patches, n, lr_size, max_value, dropout_key, first_index, record_out, stream,
                                   "dcscn_train_local_gradients_patches_aug");
}

int dcscn_train_apply_records(dcscn_handle h, const float* records, int world, double lr, double* stats, void* stream) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    if (!h->finalized) return fail(h, DCSCN_ERR_STATE, "dcscn_train_apply_records before dcscn_finalize");
    if (!h->train) return fail(h, DCSCN_ERR_STATE, "dcscn_train_apply_records before dcscn_train_begin");
    if (world < 1) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_train_apply_records: world %d < 1", world);
    int rc = check_record(h, records, 0, "dcscn_train_apply_records");
    if (rc) return rc;
    TrainState* t = h->train;
    const dcscn_train_config& tc = t->tc;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if ((rc = grow(h, &t->d_red, &t->red_cap, (size_t)kNormBlocks + 8 + (size_t)world, st))) return rc;
    double *g2p = t->d_red, *d_stats = g2p + kNormBlocks, *w = d_stats + 8;
    float* clip = reinterpret_cast<float*>(d_stats + 4);
    int* ok = reinterpret_cast<int*>(d_stats + 5);
    const int64_t pad = record_pad(t->count), rf = pad + kRecordTrailer;
    KTRY(h, hipLaunchKernelGGL(trank_weights, dim3(1), dim3(1), 0, st, records, world, rf, pad, w, ok));
    KTRY(h, hipLaunchKernelGGL(treduce_ranks, dim3(grid1(pad / 4)), dim3(256), 0, st, records, world, rf, t->count, (const double*)w, t->d_g));
    if ((rc = launch_grad_norm(h, t, g2p, st))) return rc;
    KTRY(h, hipLaunchKernelGGL(tstats_ranks, dim3(1), dim3(256), 0, st, records, world, rf, pad, (const double*)w, (const double*)g2p, kNormBlocks,
                               tc.clipping_norm, d_stats, clip));
    if ((rc = apply_update(h, t, lr, clip, ok, st))) return rc;   // nothing moves unless ok[0]
    if ((rc = join_stream(h, st))) return rc;
    if (!stats) return DCSCN_OK;
    double host[6];
    HIP_TRY(h, hipMemcpyAsync(host, d_stats, sizeof host, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    int good;
    memcpy(&good, &host[5], sizeof good);
    if (!good) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_train_apply_records: a patch count of the %d records is not > 0, or their sum is not finite; nothing was updated", world);
    std::copy(host, host + 4, stats);
    return DCSCN_OK;
}

// "<var>", "<var>/grad", "<var>/Adam", "<var>/Adam_1", "<var>/Momentum", "<var>/Adagrad", "<var>/Adadelta", "<var>/Adadelta_1", "<var>/RMSProp",
// "<var>/RMSProp_1", "beta1_power", "beta2_power"
static int train_tensor(dcscn_ctx* h, const char* name, float** dev, int64_t* count, bool* is_var) {
    TrainState* t = h->train;
    *is_var = false;
    if (!strcmp(name, "beta1_power") || !strcmp(name, "beta2_power")) {
        if (!t || t->tc.optimizer != DCSCN_OPTIMIZER_ADAM) return fail(h, DCSCN_ERR_SHAPE, "'%s' exists only while training with adam", name);
        *dev = t->d_pw + (name[4] == '1' ? 0 : 1);
        *count = 1;
        return DCSCN_OK;
    }
    std::string nm = name, suffix;
    auto it = h->tensor_index.find(nm);
    if (it == h->tensor_index.end()) {
        const size_t slash = nm.rfind('/');
        if (slash == std::string::npos) return fail(h, DCSCN_ERR_SHAPE, "unknown tensor '%s'", name);
        suffix = nm.substr(slash + 1);
        it = h->tensor_index.find(nm.substr(0, slash));
        if (it == h->tensor_index.end()) return fail(h, DCSCN_ERR_SHAPE, "unknown tensor '%s'", name);
    }
    const int i = it->second;
    *count = (int64_t)h->tensors[i].data.size();
    if (suffix.empty()) {
        *is_var = true;
        *dev = t ? t->d_w + t->off[i] : nullptr;
        return DCSCN_OK;
    }
    if (!t) return fail(h, DCSCN_ERR_STATE, "'%s' exists only after dcscn_train_begin", name);
    const int opt = t->tc.optimizer;
    if (suffix == "grad") *dev = t->d_g + t->off[i];
    else if (suffix == "Adam" && opt == DCSCN_OPTIMIZER_ADAM) *dev = t->d_m + t->off[i];
    else if (suffix == "Adam_1" && opt == DCSCN_OPTIMIZER_ADAM) *dev = t->d_v + t->off[i];
    else if (suffix == "Momentum" && opt == DCSCN_OPTIMIZER_MOMENTUM) *dev = t->d_m + t->off[i];
    else if (suffix == "Adagrad" && opt == DCSCN_OPTIMIZER_ADAGRAD) *dev = t->d_m + t->off[i];
    else if (suffix == "Adadelta" && opt == DCSCN_OPTIMIZER_ADADELTA) *dev = t->d_m + t->off[i];
    else if (suffix == "Adadelta_1" && opt == DCSCN_OPTIMIZER_ADADELTA) *dev = t->d_v + t->off[i];
    else if (suffix == "RMSProp" && opt == DCSCN_OPTIMIZER_RMSPROP) *dev = t->d_m + t->off[i];
    else if (suffix == "RMSProp_1" && opt == DCSCN_OPTIMIZER_RMSPROP) *dev = t->d_v + t->off[i];
    else return fail(h, DCSCN_ERR_SHAPE, "unknown tensor '%s' for this optimizer", name);
    return DCSCN_OK;
}

int dcscn_get_tensor(dcscn_handle h, const char* name, float* out, int64_t count) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    if (!name || !out) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_get_tensor: null argument");
    float* dev = nullptr;
    int64_t n = 0;
    bool is_var;
    SummaryView av;
    if (activation_view(h, name, &av)) {   // "x", "y_", "<layer>/output": what the last log pass left in the arena
        if (!h->train->acts_valid) return fail(h, DCSCN_ERR_STATE, "'%s' is readable only between dcscn_train_log_pass and the next training call", name);
        if (count != av.count) return fail(h, DCSCN_ERR_SHAPE, "tensor '%s' has %lld values, not %lld", name, (long long)av.count, (long long)count);
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (av.C == av.stride) HIP_TRY(h, hipMemcpy(out, av.p, (size_t)av.count * 4, hipMemcpyDeviceToHost));
        else HIP_TRY(h, hipMemcpy2D(out, (size_t)av.C * 4, av.p, (size_t)av.stride * 4, (size_t)av.C * 4, (size_t)(av.count / av.C), hipMemcpyDeviceToHost));
        return DCSCN_OK;
    }
    int rc = train_tensor(h, name, &dev, &n, &is_var);
    if (rc) return rc;
    if (count != n) return fail(h, DCSCN_ERR_SHAPE, "tensor '%s' has %lld values, not %lld", name, (long long)n, (long long)count);
    if (!dev) {   // a variable of a handle that is not training: the host copy
        const TensorSpec& ts = h->tensors[h->tensor_index[name]];
        if (!ts.set) return fail(h, DCSCN_ERR_MISSING_TENSOR, "variable '%s' was never set", name);
        std::copy(ts.data.begin(), ts.data.end(), out);
        return DCSCN_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(out, dev, (size_t)n * 4, hipMemcpyDeviceToHost));
    return DCSCN_OK;
}

int dcscn_set_train_tensor(dcscn_handle h, const char* name, const float* data, int64_t count) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    if (!name || !data) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_set_train_tensor: null argument");
    if (!h->train) return fail(h, DCSCN_ERR_STATE, "dcscn_set_train_tensor before dcscn_train_begin");
    if (strlen(name) > 5 && !strcmp(name + strlen(name) - 5, "/grad")) return fail(h, DCSCN_ERR_SHAPE, "gradients are not settable");
    float* dev = nullptr;
    int64_t n = 0;
    bool is_var;
    int rc = train_tensor(h, name, &dev, &n, &is_var);
    if (rc) return rc;
    if (count != n) return fail(h, DCSCN_ERR_SHAPE, "tensor '%s' has %lld values, not %lld", name, (long long)n, (long long)count);
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(data[i])) return fail(h, DCSCN_ERR_INVALID_ARG, "tensor '%s' holds a non-finite value", name);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(dev, data, (size_t)n * 4, hipMemcpyHostToDevice));
    if (is_var) h->train->stepped = true;
    return DCSCN_OK;
}

}  // extern "C"
