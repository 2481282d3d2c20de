// Weight repack: every launch's filters in the exact LDS image of the kernel that consumes them (dcscn_finalize).
#include "plan.h"
#include "split16_pack.hpp"

#pragma clang fp contract(off)

namespace dcscn_impl {

// ---- weight repack -----------------------------------------------------------------------------

int upload(dcscn_ctx* h, const void* host, size_t bytes, void** dev) {
    HIP_TRY(h, hipMalloc(dev, bytes));
    h->device_allocs.push_back(*dev);
    HIP_TRY(h, hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
    return DCSCN_OK;
}

// ---- what the packers share ---------------------------------------------------------------------
static const std::vector<float>& tens(const dcscn_ctx* h, int id) { return h->tensors[id].data; }
static int tens_cols(const dcscn_ctx* h, int id) { return (int)h->tensors[id].shape.back(); }

// filters, bias and slope of one launch
template <class T, class P>
static int upload3(dcscn_ctx* h, const std::vector<T>& w, P** d_w, const std::vector<float>& bias, float** d_bias, const std::vector<float>& alpha, float** d_alpha) {
    int rc = upload_vec(h, w, d_w);
    if (!rc) rc = upload_vec(h, bias, d_bias);
    if (!rc) rc = upload_vec(h, alpha, d_alpha);
    return rc;
}

// Channel groups of a launch: `tiles16` 16-channel tiles spread over the fewest groups of at most max_nt tiles; the first n_full groups
// hold nt tiles, the others nt - 1.  Bias, slope and filter columns live in the padded [group][nt * 16] layout.
struct ChanGroups {
    int n_tiles, nt, n_full;
    ChanGroups(int tiles16, int max_nt) {
        n_tiles = (tiles16 + max_nt - 1) / max_nt;
        nt = (tiles16 + n_tiles - 1) / n_tiles;
        n_full = tiles16 - n_tiles * (nt - 1);
    }
    int ctot() const { return n_tiles * nt * 16; }
    int slot(int cc) const {                         // conv channel -> slot of the padded layout
        const int t = cc / 16;
        const int wide = n_full * nt;                // tiles held by the wide groups
        const int g = t < wide ? t / nt : n_full + (t - wide) / (nt - 1);
        const int tg = t < wide ? t % nt : (t - wide) % (nt - 1);
        return (g * nt + tg) * 16 + cc % 16;
    }
};

// bias and slope of a column segment: conv channel dst + co goes to its slot of `groups` (none: slot = conv channel);
// bias_override[co] takes the place of the segment's bias tensor
static void seg_bias_alpha(const dcscn_ctx* h, const Op& op, const ColSeg& sg, const ChanGroups* groups, std::vector<float>& bias, std::vector<float>& alpha,
                           const std::vector<float>* bias_override = nullptr) {
    for (int co = 0; co < sg.cout; ++co) {
        const int pc = groups ? groups->slot(sg.dst + co) : sg.dst + co;
        if (bias_override) bias[pc] = (*bias_override)[co];
        else if (sg.b >= 0) bias[pc] = tens(h, sg.b)[sg.col0 + co];
        alpha[pc] = sg.alpha >= 0 ? tens(h, sg.alpha)[sg.col0 + co] : op.const_alpha;
    }
}

// the streamed kernels' pair of the first `cout` columns of a segment: ba[co] = bias * 2^e, ba[32 + co] = slope - 1 (stream_prelu wants alpha - 1)
static void stream_bias_slope(const dcscn_ctx* h, const Op& o, const ColSeg& sg, int cout, float* ba, int e = 0) {
    for (int co = 0; co < cout; ++co) {
        ba[co] = std::ldexp(sg.b >= 0 ? tens(h, sg.b)[sg.col0 + co] : 0.0f, e);
        ba[32 + co] = (sg.alpha >= 0 ? tens(h, sg.alpha)[sg.col0 + co] : o.const_alpha) - 1.0f;
    }
}

// depthwise filter [taps][cin] -> rows of `stride` floats (zero past cin)
static void depthwise_rows(float* dst, int stride, const std::vector<float>& dw, int taps, int cin) {
    for (int k = 0; k < taps; ++k)
        for (int ci = 0; ci < cin; ++ci) dst[(size_t)k * stride + ci] = dw[(size_t)k * cin + ci];
}

// dense [tap][physical input channel][ctot] form of one column segment, the input of pack_conv16: w = [taps][cin][wcols] from column col0
static std::vector<float> dense_image(const Op& op, const ColSeg& sg, int taps, const std::vector<float>& w, int wcols, int col0, const ChanGroups* groups, int ctot) {
    const int cin = (int)op.chan_map.size();
    std::vector<float> dense((size_t)taps * op.cin_phys * ctot, 0.0f);
    for (int t = 0; t < taps; ++t)
        for (int ci = 0; ci < cin; ++ci)
            for (int co = 0; co < sg.cout; ++co)
                dense[((size_t)t * op.cin_phys + op.chan_map[ci]) * ctot + (groups ? groups->slot(sg.dst + co) : sg.dst + co)] = w[((size_t)t * cin + ci) * wcols + col0 + co];
    return dense;
}

// parameter blob of a streamed kernel, region by region; `lds` = LDS byte address of the next region where the blob is an LDS image
struct BlobBuilder {
    std::vector<float> v;
    int lds = 0;
    size_t region(size_t floats, int32_t* lds_off = nullptr) {
        const size_t base = v.size();
        v.resize(base + floats, 0.0f);
        if (lds_off) *lds_off = lds;
        lds += (int)floats * 4;
        return base;
    }
};

// conv3_h's image of a 3x3 layer (one column segment): direct form on the f16 pipe with its own channel groups (up to kC3hMaxNT tiles),
// untransformed filters as (hi, lo) fragments scaled by 2^e, bias and slopes in the padded group layout
static int pack_conv3_h16(dcscn_ctx* h, Op& op, const std::vector<float>& w, int wcols, int tiles16) {
    const ColSeg& sg = op.segs[0];
    const ChanGroups g(tiles16, kC3hMaxNT);
    Op::Split16& s16 = op.h16;
    s16.n_tiles = g.n_tiles; s16.nt = g.nt; s16.n_full = g.n_full;
    s16.n_chunks = (op.cin_phys + kC3hKC - 1) / kC3hKC;
    const std::vector<float> dense = dense_image(op, sg, 9, w, wcols, sg.col0, &g, g.ctot());
    std::vector<float> b16(g.ctot(), 0.0f), a16(g.ctot(), 0.0f);
    seg_bias_alpha(h, op, sg, &g, b16, a16);
    const int e = split16_scale_exp(dense.data(), dense.size());
    s16.inv_scale = std::ldexp(1.0f, -e);
    s16.tail_octs = c3h_tail_octs(op.cin_phys);
    const int rc = upload3(h, pack_conv16(dense, 9, op.cin_phys, g.ctot(), g.n_tiles, g.nt, s16.n_chunks, e, s16.tail_octs), &s16.d_w, b16, &s16.d_bias, a16, &s16.d_alpha);
    s16.on = rc == DCSCN_OK;
    return rc;
}

// ---- fold_whole_tail (graph.hip): the composite 5x5 kernels of the whole tail, one set per border-position class -------------------------
namespace {
struct FoldStage {                  // one pixel-shuffler stage as a dense 3x3 conv: w [9][cin][s * s * c], b [s * s * c]
    int s = 1, cin = 0, c = 0;
    std::vector<double> w, b;
};

// the dense equivalent [9][cin][cout] of the 3x3 conv variable `var` (tf_graph.py build_conv / build_depthwise_separable_conv:
// tf.nn.separable_conv2d with channel_multiplier 1 is the dense conv w[t][ci][co] = depthwise[t][ci] * pointwise[ci][co])
bool foldx_dense(const dcscn_ctx* h, const std::string& var, int cin, int cout, bool bias, std::vector<double>& w, std::vector<double>& b) {
    auto find = [&](const std::string& n) -> const TensorSpec* {
        auto it = h->tensor_index.find(n);
        return it == h->tensor_index.end() ? nullptr : &h->tensors[it->second];
    };
    w.assign((size_t)9 * cin * cout, 0.0);
    b.assign(cout, 0.0);
    if (const TensorSpec* t = find(var + "/conv_W")) {
        if (t->data.size() != w.size()) return false;
        for (size_t i = 0; i < w.size(); ++i) w[i] = t->data[i];
    } else {
        const TensorSpec* dw = find(var + "/depthwise_W");
        const TensorSpec* pw = find(var + "/pointwise_W");
        if (!dw || !pw || dw->data.size() != (size_t)9 * cin || pw->data.size() != (size_t)cin * cout) return false;
        for (int t = 0; t < 9; ++t)
            for (int ci = 0; ci < cin; ++ci)
                for (int co = 0; co < cout; ++co) w[((size_t)t * cin + ci) * cout + co] = (double)dw->data[(size_t)t * cin + ci] * (double)pw->data[(size_t)ci * cout + co];
    }
    if (bias) {
        const TensorSpec* bt = find(var + "/conv_B");
        if (!bt || bt->data.size() != (size_t)cout) return false;
        for (int co = 0; co < cout; ++co) b[co] = bt->data[co];
    }
    return true;
}

// position classes of a pixel along one axis: 0 interior, 1 first row, 2 last row, 3 both (a one-pixel axis) -- as (size of a virtual image, the
// pixel's coordinate in it).  The padding of the intermediate maps reaches one LR pixel deep, the composite's support two: 5 / 3 / 3 / 1 pixels.
const int kFoldHv[4] = {5, 3, 3, 1}, kFoldYv[4] = {2, 0, 2, 0};

// Which (last-conv tap, stage taps ...) chains of HR row S y + a survive the zero padding of the intermediate maps, with the LR offset each
// ends at: two position classes with the same list have the same kernel (the LR map's own padding multiplies taps by zero: not part of it)
std::vector<int> foldx_axis_sig(const std::vector<FoldStage>& up, int S, int a, int variant) {
    const int Hv = kFoldHv[variant], y = kFoldYv[variant];
    std::vector<std::pair<int, int>> cur, nxt;       // (position, path code)
    for (int e = -1; e <= 1; ++e) {
        const int Y = S * y + a + e;
        if (Y >= 0 && Y < S * Hv) cur.push_back({Y, e + 1});
    }
    int res = S;
    for (int k = (int)up.size() - 1; k >= 0; --k) {
        res /= up[k].s;
        nxt.clear();
        for (const auto& p : cur)
            for (int f = -1; f <= 1; ++f) {
                const int q = p.first / up[k].s + f;
                if (k > 0 && (q < 0 || q >= res * Hv)) continue;
                nxt.push_back({q, p.second * 3 + f + 1});
            }
        cur.swap(nxt);
    }
    std::vector<int> sig;
    for (const auto& p : cur) { sig.push_back(p.second); sig.push_back(p.first - y); }
    return sig;
}

// d y(S y + a, S x + b) / d X(y + dy, x + dx, ci) for a pixel of position class (vy, vx), and the constant term: the adjoint of the chain, from the
// output pixel back through the last conv, and per stage depth_to_space and the 3x3 conv, dropping every tap that leaves an intermediate map
void foldx_kernel(const std::vector<FoldStage>& up, const std::vector<double>& r, int S, int a, int b, int vy, int vx, std::vector<double>& kw, double& kb) {
    const int Hv = kFoldHv[vy], y = kFoldYv[vy], Wv = kFoldHv[vx], x = kFoldYv[vx];
    const int n = (int)up.size(), c_last = up[n - 1].c;
    typedef std::map<std::pair<int, int>, std::vector<double>> Adj;
    Adj g;
    for (int ey = -1; ey <= 1; ++ey)
        for (int ex = -1; ex <= 1; ++ex) {
            const int Y = S * y + a + ey, X = S * x + b + ex;
            if (Y < 0 || Y >= S * Hv || X < 0 || X >= S * Wv) continue;          // the last conv's SAME padding of the HR map
            std::vector<double>& v = g[{Y, X}];
            v.assign(c_last, 0.0);
            for (int c = 0; c < c_last; ++c) v[c] = r[(size_t)((ey + 1) * 3 + (ex + 1)) * c_last + c];
        }
    kb = 0.0;
    int res = S;
    for (int k = n - 1; k >= 0; --k) {
        const FoldStage& st = up[k];
        const int s = st.s, co = s * s * st.c;
        res /= s;                                    // resolution of the stage's input map
        Adj gp;
        for (const auto& kv : g) {
            const int Y = kv.first.first, X = kv.first.second;
            const int py = Y / s, px = X / s;
            const int ch0 = ((Y - py * s) * s + (X - px * s)) * st.c;            // depth_to_space: conv channel of (sub-pixel, c)
            const std::vector<double>& gv = kv.second;
            for (int c = 0; c < st.c; ++c) kb += gv[c] * st.b[ch0 + c];
            for (int fy = -1; fy <= 1; ++fy)
                for (int fx = -1; fx <= 1; ++fx) {
                    const int qy = py + fy, qx = px + fx;
                    if (k > 0 && (qy < 0 || qy >= res * Hv || qx < 0 || qx >= res * Wv)) continue;     // SAME padding of an intermediate map
                    std::vector<double>& d = gp[{qy, qx}];
                    if (d.empty()) d.assign(st.cin, 0.0);
                    const double* wt = &st.w[(size_t)((fy + 1) * 3 + (fx + 1)) * st.cin * co];
                    for (int ci = 0; ci < st.cin; ++ci) {
                        const double* wr = wt + (size_t)ci * co + ch0;
                        double sum = 0.0;
                        for (int c = 0; c < st.c; ++c) sum += gv[c] * wr[c];
                        d[ci] += sum;
                    }
                }
        }
        g.swap(gp);
    }
    const int cin0 = up[0].cin;
    kw.assign((size_t)25 * cin0, 0.0);
    for (const auto& kv : g) {
        const int dy = kv.first.first - y, dx = kv.first.second - x;
        if (dy < -2 || dy > 2 || dx < -2 || dx > 2) continue;                    // (cannot happen: the chain's support is 5 x 5)
        for (int ci = 0; ci < cin0; ++ci) kw[(size_t)((dy + 2) * 5 + (dx + 2)) * cin0 + ci] = kv.second[ci];
    }
}
}  // namespace

int pack_foldx(dcscn_ctx* h, Op& op) {
    for (Op& sub : op.fused) {                       // the launches it replaces: the float32 plan of a flagged image, and split16 = 0
        const int rc = finalize_op(h, sub);
        if (rc) return rc;
    }
    const dcscn_config& c = h->cfg;
    const int S = op.fold_s, cin = (int)op.chan_map.size();
    const int ps_out = c.pixel_shuffler_filters != 0 ? c.pixel_shuffler_filters : cin;
    std::vector<FoldStage> up;
    if (S == 4) {
        up.resize(2);
        up[0].s = 2; up[0].cin = cin; up[0].c = cin;
        up[1].s = 2; up[1].cin = cin; up[1].c = ps_out;
    } else {
        up.resize(1);
        up[0].s = S; up[0].cin = cin; up[0].c = ps_out;
    }
    const char* names[2] = {"Up-PS/Up-PS_CNN", "Up-PS2/Up-PS2_CNN"};
    for (size_t k = 0; k < up.size(); ++k)
        if (!foldx_dense(h, names[k], up[k].cin, up[k].s * up[k].s * up[k].c, true, up[k].w, up[k].b))
            return fail(h, DCSCN_ERR_UNSUPPORTED, "internal: fold_whole_tail does not find the variables of %s", names[k]);
    std::vector<double> r, r_b;
    if (!foldx_dense(h, "R-CNN1", ps_out, 1, false, r, r_b)) return fail(h, DCSCN_ERR_UNSUPPORTED, "internal: fold_whole_tail does not find the variables of R-CNN1");
    // position classes along an axis that share a kernel for phase a (the first class with the same surviving chains)
    int eff[4][4];
    for (int a = 0; a < S; ++a) {
        std::vector<int> sig[4];
        for (int v = 0; v < 4; ++v) {
            sig[v] = foldx_axis_sig(up, S, a, v);
            eff[a][v] = v;
            for (int u = 0; u < v; ++u)
                if (sig[u] == sig[v]) { eff[a][v] = u; break; }
        }
    }
    std::map<std::vector<int>, std::pair<std::vector<double>, double>> memo;
    const int ncols = 16;
    std::vector<std::vector<float>> dense(kFoldVariants, std::vector<float>((size_t)25 * op.cin_phys * ncols, 0.0f));
    std::vector<float> b16((size_t)kFoldVariants * ncols, 0.0f);
    for (int vy = 0; vy < 4; ++vy)
        for (int vx = 0; vx < 4; ++vx)
            for (int a = 0; a < S; ++a)
                for (int b = 0; b < S; ++b) {
                    const std::vector<int> key = {a, eff[a][vy], b, eff[b][vx]};
                    auto it = memo.find(key);
                    if (it == memo.end()) {
                        std::pair<std::vector<double>, double> kk;
                        foldx_kernel(up, r, S, a, b, eff[a][vy], eff[b][vx], kk.first, kk.second);
                        it = memo.emplace(key, std::move(kk)).first;
                    }
                    const int v = vy * 4 + vx, p = a * S + b;
                    const std::vector<double>& kw = it->second.first;
                    for (int t = 0; t < 25; ++t)
                        for (int ci = 0; ci < cin; ++ci) dense[v][((size_t)t * op.cin_phys + op.chan_map[ci]) * ncols + p] = (float)kw[(size_t)t * cin + ci];
                    b16[(size_t)v * ncols + p] = (float)it->second.second;
                }
    Op::Split16& s16 = op.h16;
    s16.nt = 1; s16.n_tiles = 1; s16.n_full = 1;
    s16.n_chunks = (op.cin_phys + kC3hKC - 1) / kC3hKC;
    int e = 0;
    {
        float m = 0.0f;
        for (const auto& d : dense)
            for (float w : d) m = std::fmax(m, std::fabs(w));
        e = split16_scale_exp(&m, 1);
    }
    s16.inv_scale = std::ldexp(1.0f, -e);
    std::vector<uint16_t> img;
    for (int v = 0; v < kFoldVariants; ++v) {
        const std::vector<uint16_t> one = pack_conv16(dense[v], 25, op.cin_phys, ncols, 1, 1, s16.n_chunks, e);
        img.insert(img.end(), one.begin(), one.end());
    }
    int rc = upload_vec(h, img, &s16.d_w);
    if (!rc) rc = upload_vec(h, b16, &s16.d_bias);
    s16.on = rc == DCSCN_OK;
    return rc;
}

// ---- the launches of the layer-by-layer plan, one packer per kind ----------------------------------------------------------------------
static int pack_depthwise(dcscn_ctx* h, Op& op) {
    const int rc = upload_vec(h, tens(h, op.dw_w), &op.d_w);            // [k, k, cin, 1] -> [taps][cin]
    if (rc) return rc;
    return upload_vec(h, std::vector<int32_t>(op.chan_map.begin(), op.chan_map.end()), &op.d_map);
}

static int pack_cout1(dcscn_ctx* h, Op& op) {
    const ColSeg& s = op.segs[0];
    const bool separable = op.dw_w >= 0;
    const std::vector<float>& tw = tens(h, separable ? op.dw_w : s.w);  // [k, k, cin, 1]
    if (separable) op.out_scale = tens(h, s.w)[0];                      // pointwise [1, 1, 1, 1]
    const int taps = op.ks * op.ks, cin = (int)op.chan_map.size();
    std::vector<float> w((size_t)taps * op.cin_phys, 0.0f);
    for (int t = 0; t < taps; ++t)
        for (int ci = 0; ci < cin; ++ci) {
            float v = tw[(size_t)t * cin + ci];
            if (s.dw1 >= 0) v = tens(h, s.dw1)[ci] * v;                  // folded 1x1 depthwise half (ColSeg::dw1)
            w[(size_t)t * op.cin_phys + op.chan_map[ci]] = v;
        }
    return upload_vec(h, w, &op.d_w);
}

static int pack_cin1(dcscn_ctx* h, Op& op) {
    const ColSeg& s = op.segs[0];
    const int taps = op.ks * op.ks, cs = op.out_width[0];
    std::vector<float> w((size_t)taps * cs, 0.0f), b(cs, 0.0f), al(cs, op.const_alpha);
    const std::vector<float>& tw = tens(h, s.w);            // [k, k, 1, cout]
    for (int t = 0; t < taps; ++t)
        for (int c = 0; c < s.cout; ++c) w[(size_t)t * cs + c] = tw[(size_t)t * s.cout + c];
    if (s.b >= 0) std::copy(tens(h, s.b).begin(), tens(h, s.b).end(), b.begin());
    if (s.alpha >= 0) std::copy(tens(h, s.alpha).begin(), tens(h, s.alpha).end(), al.begin());
    for (int c = s.cout; c < cs; ++c) al[c] = 0.0f;
    return upload3(h, w, &op.d_w, b, &op.d_bias, al, &op.d_alpha);
}

// transposed conv [k, k, out C, in C] of stride sc: the equivalent 3x3 filter [3][3][C][sc * sc * C] (see add_tconv)
static std::vector<float> tconv_filter3(const TensorSpec& t, int sc) {
    const int kk = (int)t.shape[0], C = (int)t.shape[2], pt = (kk - sc) / 2, co = sc * sc * C;
    std::vector<float> w((size_t)9 * C * co, 0.0f);
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx)
            for (int a2 = 0; a2 < sc; ++a2)
                for (int b2 = 0; b2 < sc; ++b2) {
                    const int ky = a2 + pt - sc * dy, kx = b2 + pt - sc * dx;
                    if (ky < 0 || ky >= kk || kx < 0 || kx >= kk) continue;
                    for (int ic = 0; ic < C; ++ic)
                        for (int oc = 0; oc < C; ++oc)
                            w[(((size_t)(dy + 1) * 3 + (dx + 1)) * C + ic) * co + (size_t)(a2 * sc + b2) * C + oc] = t.data[(((size_t)ky * kk + kx) * C + oc) * C + ic];
                }
    return w;
}

// folded linear tail: the composite 5x5 filter [5][5][cin][phase * 4 + variant] of the pixel-shuffler conv wu [3, 3, cin, sc * sc * C] (bias bu or
// null) and the last reconstruction conv wr [3, 3, C, 1], and its bias, in float64
static void fold_tail_filter5(const std::vector<float>& wu, const float* bu, const std::vector<float>& wr, int sc, int C, int cin, std::vector<float>& w, std::vector<float>& bias) {
    const int V = 4 * sc * sc, UC = sc * sc * C;
    std::vector<double> wacc((size_t)25 * cin * V, 0.0), bacc(V, 0.0);
    auto fdiv = [](int x, int d) { return x >= 0 ? x / d : -((-x + d - 1) / d); };
    for (int pa = 0; pa < sc; ++pa)
        for (int pb = 0; pb < sc; ++pb)
            for (int var = 0; var < 4; ++var) {
                const int v = (pa * sc + pb) * 4 + var;
                const bool rbit = var & 2, cbit = var & 1;
                for (int dy = -1; dy <= 1; ++dy) {
                    if (rbit && ((pa == 0 && dy == -1) || (pa == sc - 1 && dy == 1))) continue;   // tap above / below the image
                    const int oy = fdiv(pa + dy, sc), a2 = pa + dy - oy * sc;
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (cbit && ((pb == 0 && dx == -1) || (pb == sc - 1 && dx == 1))) continue;
                        const int ox = fdiv(pb + dx, sc), b2 = pb + dx - ox * sc;
                        for (int cc = 0; cc < C; ++cc) {
                            const double wrv = wr[((size_t)(dy + 1) * 3 + (dx + 1)) * C + cc];
                            const int ch = (a2 * sc + b2) * C + cc;
                            if (bu) bacc[v] += wrv * bu[ch];
                            for (int ey = -1; ey <= 1; ++ey)
                                for (int ex = -1; ex <= 1; ++ex) {
                                    const size_t tap5 = (size_t)(oy + ey + 2) * 5 + (ox + ex + 2);
                                    const float* wsrc = &wu[((size_t)(ey + 1) * 3 + (ex + 1)) * cin * UC + ch];
                                    double* wdst = &wacc[tap5 * cin * V + v];
                                    for (int k = 0; k < cin; ++k) wdst[(size_t)k * V] += wrv * wsrc[(size_t)k * UC];
                                }
                        }
                    }
                }
            }
    w.assign(wacc.begin(), wacc.end());
    bias.assign(bacc.begin(), bacc.end());
}

// conv_nin (wide 1x1 GEMM) and, over the same channel groups, conv_nin_h: dense [k_phys][conv channel] -> [group][chunk][kk][NS]
static int pack_nin(dcscn_ctx* h, Op& op, int tiles16) {
    const ChanGroups g(tiles16, kNinMaxNT);
    const int nt = g.nt, kc = kNinKC, cin = (int)op.chan_map.size();
    op.n_tiles = g.n_tiles; op.n_full = g.n_full; op.ctot = g.ctot();
    op.shape = ConvShape{1, 4, nt, kNinKC, 0, 1, 0};
    op.n_chunks = (op.cin_phys + kc - 1) / kc;
    const int ns = conv_ns(nt);
    const size_t chunk_floats = (size_t)kc * ns;
    std::vector<float> pack((size_t)op.n_tiles * op.n_chunks * chunk_floats, 0.0f);
    std::vector<float> bias(op.ctot, 0.0f), alpha(op.ctot, 0.0f);
    std::vector<float> dense((size_t)op.cin_phys * op.ctot, 0.0f);          // [physical input channel][padded output channel], for the split16 image
    for (const ColSeg& sg : op.segs) {
        const std::vector<float>& tw = tens(h, sg.w);                       // [1, 1, cin, cout]
        const int wcols = tens_cols(h, sg.w);
        for (int ci = 0; ci < cin; ++ci) {
            const int kp = op.chan_map[ci];
            const int chunk = kp / kc, c16 = kp % kc;
            const int row = (c16 & 3) * 4 + (c16 >> 2);                   // k-step c16 & 3, MFMA k index c16 >> 2
            const float dscale = sg.dw1 >= 0 ? tens(h, sg.dw1)[ci] : 1.0f;     // folded 1x1 depthwise
            const float* wrow = &tw[(size_t)ci * wcols + sg.col0];
            for (int co = 0; co < sg.cout; ++co) {
                const int pc = g.slot(sg.dst + co);
                const int grp = pc / (nt * 16), jn = pc % (nt * 16);
                const float wv = sg.dw1 >= 0 ? dscale * wrow[co] : wrow[co];
                pack[((size_t)grp * op.n_chunks + chunk) * chunk_floats + (size_t)row * ns + jn] = wv;
                dense[(size_t)kp * op.ctot + pc] = wv;
            }
        }
        seg_bias_alpha(h, op, sg, &g, bias, alpha);
    }
    int rc = upload3(h, pack, &op.d_w, bias, &op.d_bias, alpha, &op.d_alpha);
    if (rc) return rc;
    // conv_nin_h: the same channel groups, 32-channel chunks, f16 (hi, lo) fragments of the filters scaled by 2^e
    Op::Split16& s16 = op.h16;
    s16.nt = nt; s16.n_tiles = op.n_tiles; s16.n_full = op.n_full;
    s16.n_chunks = (op.cin_phys + kNinHKC - 1) / kNinHKC;
    const int e = split16_scale_exp(dense.data(), dense.size());
    s16.inv_scale = std::ldexp(1.0f, -e);
    rc = upload_vec(h, pack_conv16(dense, 1, op.cin_phys, op.ctot, op.n_tiles, nt, s16.n_chunks, e), &s16.d_w);
    s16.on = rc == DCSCN_OK;
    return rc;
}

// conv_wino2 (one column segment): w = [3, 3, cin, wcols] as G g G^T -> [group][chunk][f][kk][NS], and conv3_h's image of the same layer
static int pack_wino(dcscn_ctx* h, Op& op, const std::vector<float>& w, int wcols, int tiles16) {
    const ChanGroups g(tiles16, kWinoMaxNT);
    const int nt = g.nt, kc = kWinoKC, cin = (int)op.chan_map.size();
    op.n_tiles = g.n_tiles; op.n_full = g.n_full; op.ctot = g.ctot();
    op.shape = ConvShape{3, 4, nt, kWinoKC, 0, 0, 1};
    op.n_chunks = (op.cin_phys + kc - 1) / kc;
    const int ns = conv_ns(nt);
    const size_t chunk_floats = (size_t)16 * kc * ns;
    std::vector<float> pack((size_t)op.n_tiles * op.n_chunks * chunk_floats, 0.0f);
    std::vector<float> bias(op.ctot, 0.0f), alpha(op.ctot, 0.0f);
    const ColSeg& sg = op.segs[0];
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    for (int ci = 0; ci < cin; ++ci) {
        const int kp = op.chan_map[ci];
        const int chunk = kp / kc, c8 = kp % kc;
        const int row = (c8 & 1) * 4 + (c8 >> 1);                          // k-step c8 & 1, MFMA k index c8 >> 1
        for (int co = 0; co < sg.cout; ++co) {
            double f[3][3], gg[4][3];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) f[i][j] = w[((size_t)(i * 3 + j) * cin + ci) * wcols + sg.col0 + co];
            for (int xi = 0; xi < 4; ++xi)                      // G g
                for (int j = 0; j < 3; ++j) gg[xi][j] = G[xi][0] * f[0][j] + G[xi][1] * f[1][j] + G[xi][2] * f[2][j];
            const int pc = g.slot(sg.dst + co);
            const int grp = pc / (nt * 16), jn = pc % (nt * 16);
            for (int xi = 0; xi < 4; ++xi)
                for (int nu = 0; nu < 4; ++nu) {                // (G g) G^T, float64, rounded once
                    const double u = gg[xi][0] * G[nu][0] + gg[xi][1] * G[nu][1] + gg[xi][2] * G[nu][2];
                    pack[((size_t)grp * op.n_chunks + chunk) * chunk_floats + ((size_t)(xi * 4 + nu) * kc + row) * ns + jn] = (float)u;
                }
        }
    }
    seg_bias_alpha(h, op, sg, &g, bias, alpha);
    int rc = upload3(h, pack, &op.d_w, bias, &op.d_bias, alpha, &op.d_alpha);
    if (!rc) rc = pack_conv3_h16(h, op, w, wcols, tiles16);
    return rc;
}

// conv_igemm with equal-width channel groups: dense [tap][k_phys][conv channel] -> [n_tile][chunk][tap][kk][NS]; in front of it the filter of
// a fused depthwise conv.  w_override ([taps][cin][cout] per segment) / bias_override: the derived filter of a transposed conv or a folded tail
static int pack_igemm(dcscn_ctx* h, Op& op, int tiles16, const std::vector<float>* w_override, const std::vector<float>* bias_override) {
    const int taps = op.ks * op.ks, cin = (int)op.chan_map.size();
    const int max_nt = op.dwk ? conv_max_fused_dw_nt() : conv_max_nt(op.ks);
    op.n_tiles = (tiles16 + max_nt - 1) / max_nt;
    const int nt = (tiles16 + op.n_tiles - 1) / op.n_tiles;
    op.shape = conv_pick_shape(op.ks, nt, op.dwk);
    if (op.dwk) {
        std::vector<float> dww((size_t)op.dwk * op.dwk * op.cin_phys, 0.0f);   // [k, k, cin, 1] -> [taps][cin_phys] physical
        for (int t = 0; t < op.dwk * op.dwk; ++t)
            for (int ci = 0; ci < cin; ++ci) dww[(size_t)t * op.cin_phys + op.chan_map[ci]] = tens(h, op.dw_w)[(size_t)t * cin + ci];
        const int rc0 = upload_vec(h, dww, &op.d_dww);
        if (rc0) return rc0;
    }
    op.ctot = op.n_tiles * nt * 16;
    const int kc = op.shape.kc;
    op.n_chunks = (op.cin_phys + kc - 1) / kc;
    const int ns = conv_ns(nt);
    const size_t chunk_floats = (size_t)taps * kc * ns;
    std::vector<float> pack((size_t)op.n_tiles * op.n_chunks * chunk_floats, 0.0f);
    std::vector<float> bias(op.ctot, 0.0f), alpha(op.ctot, 0.0f);
    for (const ColSeg& s : op.segs) {
        const std::vector<float>& tw = w_override ? *w_override : tens(h, s.w);   // [ks, ks, cin, cout] (or [1,1,cin,cout])
        const int wcols = w_override ? s.cout : tens_cols(h, s.w);
        for (int t = 0; t < taps; ++t)
            for (int ci = 0; ci < cin; ++ci) {
                const int kp = op.chan_map[ci];
                const int chunk = kp / kc, kk = kp % kc;
                const float* wrow = &tw[((size_t)t * cin + ci) * wcols + s.col0];
                const float dscale = s.dw1 >= 0 ? tens(h, s.dw1)[ci] : 1.0f;     // folded 1x1 depthwise
                for (int co = 0; co < s.cout; ++co) {
                    const int cc = s.dst + co;
                    const int tile = cc / (nt * 16), j = cc % (nt * 16);
                    pack[((size_t)tile * op.n_chunks + chunk) * chunk_floats + ((size_t)t * kc + kk) * ns + j] =
                        s.dw1 >= 0 ? dscale * wrow[co] : wrow[co];
                }
            }
        seg_bias_alpha(h, op, s, nullptr, bias, alpha, bias_override);
    }
    return upload3(h, pack, &op.d_w, bias, &op.d_bias, alpha, &op.d_alpha);
}

// conv5_h: the folded tail (composite filter w [25][cin][cout], its bias) on the f16 pipe -- one channel group of ceil(4 s^2 / 16) tiles;
// conv_igemm<5, 4, ...> with the same 16x16 pixel tiles stays behind it as the f32 fallback of flagged tiles
static int pack_conv5_h16(dcscn_ctx* h, Op& op, const std::vector<float>& w, const std::vector<float>& bias) {
    Op::Split16& s16 = op.h16;
    const ColSeg& sg = op.segs[0];
    const int nt16 = (sg.dst + sg.cout + 15) / 16;
    if (nt16 != 1 && nt16 != 3 && nt16 != 4) return DCSCN_OK;
    s16.nt = nt16; s16.n_tiles = 1; s16.n_full = 1;
    s16.n_chunks = (op.cin_phys + kC3hKC - 1) / kC3hKC;
    const int ctot16 = nt16 * 16;
    const std::vector<float> dense = dense_image(op, sg, 25, w, sg.cout, 0, nullptr, ctot16);
    std::vector<float> b16(ctot16, 0.0f);
    for (int co = 0; co < sg.cout; ++co) b16[sg.dst + co] = bias[co];
    const int e = split16_scale_exp(dense.data(), dense.size());
    s16.inv_scale = std::ldexp(1.0f, -e);
    int rc = upload_vec(h, pack_conv16(dense, 25, op.cin_phys, ctot16, 1, nt16, s16.n_chunks, e), &s16.d_w);
    if (!rc) rc = upload_vec(h, b16, &s16.d_bias);
    s16.on = rc == DCSCN_OK;
    return rc;
}

int finalize_op(dcscn_ctx* h, Op& op) {
    switch (op.kind) {
        case OP_FOLDX: return pack_foldx(h, op);
        case OP_STREAM3: return pack_feat3_stream(h, op);
        case OP_STREAM: return pack_feat_stream(h, op);
        case OP_TAIL: return pack_tail_stream(h, op);
        case OP_DW: return pack_depthwise(h, op);
        case OP_COUT1: return pack_cout1(h, op);
        case OP_CIN1: return pack_cin1(h, op);
        case OP_CONV: break;
    }
    const ColSeg& s0 = op.segs[0];
    std::vector<float> derived, derived_bias;          // the filter of a transposed conv / a folded linear tail takes the variable's place
    if (op.tconv_s > 0) derived = tconv_filter3(h->tensors[s0.w], op.tconv_s);
    if (op.fold_s > 0)
        fold_tail_filter5(tens(h, s0.w), s0.b >= 0 ? tens(h, s0.b).data() : nullptr, tens(h, op.fold_rw), op.fold_s, op.fold_c, (int)op.chan_map.size(), derived, derived_bias);
    const bool is_derived = op.tconv_s > 0 || op.fold_s > 0;
    int ctot = 0;
    for (const ColSeg& s : op.segs) ctot = std::max(ctot, s.dst + s.cout);
    const int tiles16 = (ctot + 15) / 16;
    if (nin_eligible(h, op)) return pack_nin(h, op, tiles16);
    if (wino_eligible(h, op)) return is_derived ? pack_wino(h, op, derived, s0.cout, tiles16) : pack_wino(h, op, tens(h, s0.w), tens_cols(h, s0.w), tiles16);
    int rc = pack_igemm(h, op, tiles16, is_derived ? &derived : nullptr, op.fold_s > 0 ? &derived_bias : nullptr);
    if (!rc && op.fold_s > 0 && op.ks == 5 && op.shape.mt == 4 && op.segs.size() == 1 && op.dwk == 0) rc = pack_conv5_h16(h, op, derived, derived_bias);
    // one-tile / scalar-store 3x3 layers: conv3_h in front of the conv_igemm kernel packed above (graph.hip: h16_direct_eligible)
    if (!rc && h16_direct_eligible(h, op)) rc = pack_conv3_h16(h, op, tens(h, s0.w), tens_cols(h, s0.w), tiles16);
    return rc;
}

// ---- the streamed kernels -----------------------------------------------------------------------------------------------------------------
// float32 image of one pointwise GEMM of the streamed kernels (feat_stream.hpp: stream_dw_pw): [chunk][tile][64 lanes] float4 -- lane (output
// column 16 n + (lane & 15), q = lane >> 4) holds in k-step st the channel stream_chunk_channel gives it (zero where it gives none).
// get(ci, co) = the weight (0 past the real channels)
template <typename Get>
static void stream_f32_image(float* dst, int quads, int chunks, int tiles, const Get& get) {
    for (int ch = 0; ch < chunks; ++ch)
        for (int n = 0; n < tiles; ++n)
            for (int lane = 0; lane < 64; ++lane)
                for (int st = 0; st < 4; ++st) {
                    const int ci = stream_chunk_channel(quads, ch, lane >> 4, st);
                    if (ci >= 0) dst[((size_t)(ch * tiles + n) * 64 + lane) * 4 + st] = get(ci, 16 * n + (lane & 15));
                }
}

// f16 image of the same GEMM (F16 kernels), written over its float32 image's slots
// (same size): `quads` input channel quads in 16-channel chunks, `tiles` output tiles; per chunk PAIR and tile two 1 KB fragments --
// lane (i = lane & 15: output column 16 n + i, q = lane >> 4) holds k = 8 q + t: t < 4 channel 16 (2p) + 4 q + t, else 16 (2p + 1) + 4 q + t - 4 --
// hi at slot (2p * tiles + 2n), lo right behind it; an odd last chunk keeps one slot per tile: [hi t 0-3 | lo t 0-3].  get(ci, co) as above;
// the weights are multiplied by 2^e.
template <typename Get>
static void stream_f16_image(float* dst, int quads, int tiles, const Get& get, int e) {
    const int chunks = (quads + 3) / 4;
    uint16_t* d16 = reinterpret_cast<uint16_t*>(dst);
    auto chan = [&](int ch, int q, int t) { return q < std::min(4, quads - 4 * ch) ? 16 * ch + 4 * q + t : -1; };
    for (int n = 0; n < tiles; ++n)
        for (int lane = 0; lane < 64; ++lane) {
            const int q = lane >> 4, co = 16 * n + (lane & 15);
            for (int p = 0; 2 * p + 1 < chunks; ++p) {
                uint16_t* hi = d16 + ((size_t)(2 * p * tiles + 2 * n) * 64 + lane) * 8;
                uint16_t* lo = hi + 64 * 8;
                for (int t = 0; t < 8; ++t) {
                    const int ci = chan(2 * p + (t >> 2), q, t & 3);
                    split16_host(std::ldexp(ci >= 0 ? get(ci, co) : 0.0f, e), &hi[t], &lo[t]);
                }
            }
            if (chunks & 1) {
                const int ch = chunks - 1;
                uint16_t* s = d16 + ((size_t)(ch * tiles + n) * 64 + lane) * 8;
                for (int t = 0; t < 4; ++t) {
                    const int ci = chan(ch, q, t);
                    split16_host(std::ldexp(ci >= 0 ? get(ci, co) : 0.0f, e), &s[t], &s[4 + t]);
                }
            }
        }
}

// feat3_stream's fragment of v_mfma_f32_16x16x32_f16 (its layout differs from stream_f16_image's): [hi | lo][64 lanes][8 halfs] at d16 --
// lane (i = lane & 15, q = lane >> 4) holds get(q, t, i) * 2^e for t < 8
template <typename Get>
static void s3_f16_fragment(uint16_t* d16, const Get& get, int e) {
    for (int lane = 0; lane < 64; ++lane) {
        uint16_t* hi = d16 + (size_t)lane * 8;
        uint16_t* lo = hi + 64 * 8;
        for (int t = 0; t < 8; ++t) split16_host(std::ldexp(get(lane >> 4, t, lane & 15), e), &hi[t], &lo[t]);
    }
}

// A1 || B1 of the streamed kernels as one 32-column GEMM over the K axis of all feature layers: column v < pad4(nb) is B1 channel v
// (segment sb), the others A1 channel v - pad4(nb) (segment sa), zero past the real channels; with the folded 1x1 depthwise half, as pack_nin
static float nin_column(const dcscn_ctx* h, const ColSeg& sb, const ColSeg& sa, int nb, int na, int k, int v) {
    const bool is_b = v < pad4(nb);
    const ColSeg& sg = is_b ? sb : sa;
    const int co = is_b ? v : v - pad4(nb);
    if (co >= (is_b ? nb : na)) return 0.0f;
    float w = tens(h, sg.w)[(size_t)k * tens_cols(h, sg.w) + sg.col0 + co];
    if (sg.dw1 >= 0) w = tens(h, sg.dw1)[k] * w;
    return w;
}

int pack_tail_stream(dcscn_ctx* h, Op& op) {
    const Op& u1 = op.fused[0];
    const Op& u2 = op.fused[1];
    const Op& rc = op.fused[2];
    const int cin = u1.cin, C = u1.ps_c;
    TailArgs& a = op.tail;
    a = TailArgs{};
    BlobBuilder bb;
    a.in.quads = cin / 4; a.in.units = a.in.quads | 1; a.in.slots = 3; a.in.off = bb.lds;
    bb.lds += 3 * kStreamRowPx * a.in.units * 16;
    a.u.quads = C / 4; a.u.units = a.u.quads | 1; a.u.slots = 6; a.u.off = bb.lds;
    bb.lds += 6 * (2 * kStreamPX + 2) * a.u.units * 16;
    a.v_off = bb.lds;
    bb.lds += 12 * (4 * kStreamPX + 4) * 4;
    a.ring_bytes = bb.lds;
    // Up-PS: depthwise [3, 3, cin, 1]; pointwise [1, 1, cin, 4C] (column phase * C + c) as [chunk][channel tile 0..7][lane] float4 over the 4C conv
    // channels (tile = 2 * phase + half when C > 16); bias [channel tile][16]
    const std::vector<float>& pw1 = tens(h, u1.segs[0].w);
    const int tiles = C > 16 ? 2 : 1;
    auto get1 = [&](int ci, int co) {
        const int n = co / 16, ph = n / tiles, cc = 16 * (n % tiles) + co % 16;
        return ci < cin && ph < 4 && cc < C ? pw1[(size_t)ci * 4 * C + ph * C + cc] : 0.0f;
    };
    const size_t a_dww_base = bb.region((size_t)9 * a.in.quads * 4, &a.a_dww);
    depthwise_rows(&bb.v[a_dww_base], a.in.quads * 4, tens(h, u1.dw_w), 9, cin);
    const size_t a_wp_base = bb.region((size_t)2 * 8 * 64 * 4, &a.a_wp);
    stream_f32_image(&bb.v[a_wp_base], cin / 4, 2, 8, get1);
    const size_t a_bias_base = bb.region(8 * 16, &a.a_bias);
    for (int ph = 0; ph < 4; ++ph)
        for (int cc = 0; cc < C; ++cc) bb.v[a_bias_base + (ph * tiles + cc / 16) * 16 + cc % 16] = u1.segs[0].b >= 0 ? tens(h, u1.segs[0].b)[ph * C + cc] : 0.0f;
    // Up-PS2: depthwise [3, 3, C, 1]; pointwise [1, 1, C, 4] as [chunk][lane] float4; bias [4]
    const std::vector<float>& pw2 = tens(h, u2.segs[0].w);
    auto get2 = [&](int ci, int co) { return ci < C && co < 4 ? pw2[(size_t)ci * 4 + co] : 0.0f; };
    const size_t b_dww_base = bb.region((size_t)9 * a.u.quads * 4, &a.b_dww);
    depthwise_rows(&bb.v[b_dww_base], a.u.quads * 4, tens(h, u2.dw_w), 9, C);
    const size_t b_wp_base = bb.region((size_t)2 * 64 * 4, &a.b_wp);
    stream_f32_image(&bb.v[b_wp_base], C / 4, 2, 1, get2);
    const size_t b_bias_base = bb.region(4, &a.b_bias);
    for (int co = 0; co < 4; ++co) bb.v[b_bias_base + co] = u2.segs[0].b >= 0 ? tens(h, u2.segs[0].b)[co] : 0.0f;
    a.ldsw_bytes = bb.lds - a.ring_bytes;
    if (bb.lds > 160 * 1024) return fail(h, DCSCN_ERR_UNSUPPORTED, "internal: tail_stream needs %d bytes of LDS", bb.lds);
    for (int k = 0; k < 9; ++k) a.c_w[k] = tens(h, rc.dw_w)[k];      // [3, 3, 1, 1]
    a.c_scale = tens(h, rc.segs[0].w)[0];                            // [1, 1, 1, 1]
    int urc = upload_vec(h, bb.v, &op.d_w);
    if (urc) return urc;
    // the F16 kernel's image: the pointwise filters as f16 fragments scaled by 2^e per GEMM over the float32 image's slots, the biases times 2^e
    std::vector<float> blob16 = bb.v;
    auto f16_gemm = [&](const std::vector<float>& pw, size_t wp_base, int quads, int n_tiles, auto& get, size_t bias_base, int n_bias, float* inv) {
        const int e = split16_scale_exp(pw.data(), pw.size());
        stream_f16_image(&blob16[wp_base], quads, n_tiles, get, e);
        for (int k = 0; k < n_bias; ++k) blob16[bias_base + k] = std::ldexp(bb.v[bias_base + k], e);
        *inv = std::ldexp(1.0f, -e);
    };
    f16_gemm(pw1, a_wp_base, cin / 4, 8, get1, a_bias_base, 8 * 16, &a.a_inv);
    f16_gemm(pw2, b_wp_base, C / 4, 1, get2, b_bias_base, 4, &a.b_inv);
    urc = upload_vec(h, blob16, &op.h16.d_w);
    op.h16.on = urc == DCSCN_OK;
    return urc;
}

// feat_stream's wave -> role table.  Wave w runs on SIMD w & 3, and on a SIMD the MFMAs and the VALU instructions of all its waves execute
// one after the other (tools/mfma_valu_overlap.hip), so a SIMD's time per row is the SUM of its roles' estimated cycles.  Exhaustive search
// for the assignment with the smallest maximum: roles 0 .. L (CNN1 and the L convs, cost[r]) are tried on every SIMD (4^(L+1) <= 65536), the L
// interchangeable A1 || B1 roles (nin_cost each, codes 16 + slot) always go onto the least loaded SIMD with a free wave.  False: no placement
static bool feat_stream_roles(const std::vector<int>& cost, int nin_cost, int L, int8_t role[16]) {
    const int waves = 2 * L + 1;
    int cap[4];
    for (int sd = 0; sd < 4; ++sd) cap[sd] = (waves - sd + 3) / 4;      // waves sd, sd + 4, ... below `waves`
    long best_key = -1;
    std::vector<int> best_sd(1 + L, 0);
    int best_nin[4] = {0, 0, 0, 0};
    const int combos = 1 << (2 * (L + 1));
    for (int m = 0; m < combos; ++m) {
        int load[4] = {0, 0, 0, 0}, used[4] = {0, 0, 0, 0};
        for (int r = 0; r <= L; ++r) { const int sd = (m >> (2 * r)) & 3; load[sd] += cost[r]; used[sd] += 1; }
        if (used[0] > cap[0] || used[1] > cap[1] || used[2] > cap[2] || used[3] > cap[3]) continue;
        // (the interchangeable roles only add load, so a maximum that is already past the best key's cannot become the smaller key)
        if (best_key >= 0 && (long)std::max(std::max(load[0], load[1]), std::max(load[2], load[3])) * 1000000 > best_key) continue;
        int nin[4] = {0, 0, 0, 0};
        bool ok = true;
        for (int k = 0; k < L && ok; ++k) {
            int pick = -1;
            for (int sd = 0; sd < 4; ++sd)
                if (used[sd] + nin[sd] < cap[sd] && (pick < 0 || load[sd] < load[pick])) pick = sd;
            if (pick < 0) { ok = false; break; }
            nin[pick] += 1;
            load[pick] += nin_cost;
        }
        if (!ok) continue;
        const long mx = std::max(std::max(load[0], load[1]), std::max(load[2], load[3]));
        long sq = 0;
        for (int sd = 0; sd < 4; ++sd) sq += (long)(load[sd] / 16) * (load[sd] / 16);
        const long key = mx * 1000000 + sq / 16;
        if (best_key < 0 || key < best_key) {
            best_key = key;
            for (int r = 0; r <= L; ++r) best_sd[r] = (m >> (2 * r)) & 3;
            for (int sd = 0; sd < 4; ++sd) best_nin[sd] = nin[sd];
        }
    }
    if (best_key < 0) return false;
    int used[4] = {0, 0, 0, 0};
    for (int w = 0; w < 16; ++w) role[w] = 0;
    for (int r = 0; r <= L; ++r) { const int sd = best_sd[r]; role[sd + 4 * used[sd]] = (int8_t)r; used[sd] += 1; }
    int slot = 0;
    for (int sd = 0; sd < 4; ++sd)
        for (int k = 0; k < best_nin[sd]; ++k) { role[sd + 4 * used[sd]] = (int8_t)(16 + slot); used[sd] += 1; slot += 1; }
    return true;
}

int pack_feat_stream(dcscn_ctx* h, Op& op) {
    const dcscn_config& c = h->cfg;
    const int L = c.layers, nb = c.nin_filters2, na = c.nin_filters;
    StreamArgs& a = op.stream;
    a = StreamArgs{};
    a.L = L;
    a.n_conv = L;                      // CNN2 .. CNNL and B2
    a.total_lag = 2 * L + 1;
    a.nb_quads = pad4(nb) / 4;
    BlobBuilder bb;
    auto ring = [&](int ch, int slots) {
        StreamRing r;
        r.quads = pad4(ch) / 4;
        r.units = r.quads | 1;
        r.slots = slots;
        r.off = bb.lds;
        bb.lds += slots * kStreamRowPx * r.units * 16;
        return r;
    };
    std::vector<StreamRing> fr(L);
    for (int i = 0; i < L; ++i) fr[i] = ring(h->sched[i], 3);
    a.b1 = ring(nb, 4);
    a.first_out = fr[0];
    a.ring_bytes = bb.lds;

    std::vector<size_t> nin_base(L), wp_base(L), ba_base(L);        // blob offsets (floats) of the regions the f16 image rewrites
    const Op& nin = op.fused[L + 1];
    const ColSeg& sb = nin.segs[0];
    const ColSeg& sa = nin.segs[1];
    // conv i: CNN(i+2) for i < L-1, B2 for i == L-1; get(ci, co) of its pointwise filter [1, 1, cin, cout] and of layer i's K-slice of A1 || B1
    auto conv_src = [&](int i) -> const Op& { return i == L - 1 ? op.fused[L + 2] : op.fused[2 + i]; };
    auto conv_cin = [&](int i) { return i == L - 1 ? nb : h->sched[i]; };
    auto pw_get = [&](int i) {
        const ColSeg& sg = conv_src(i).segs[0];
        const float* pw = tens(h, sg.w).data();
        const int cin = conv_cin(i), cout = sg.cout;
        return [=](int ci, int co) { return ci < cin && co < cout ? pw[(size_t)ci * cout + co] : 0.0f; };
    };
    std::vector<int> k0(L + 1, 0);                                  // first row of layer i on the K axis of A1 || B1
    for (int i = 0; i < L; ++i) k0[i + 1] = k0[i] + h->sched[i];
    auto nin_get = [&](int i) {
        const int C = h->sched[i], kb = k0[i];
        return [=, &sb, &sa](int ci, int v) { return ci < C ? nin_column(h, sb, sa, nb, na, kb + ci, v) : 0.0f; };
    };
    // --- LDS image: A1 || B1 slices, then the depthwise filters ---
    for (int i = 0; i < L; ++i) {
        StreamNinSrc& s = a.nin[i];
        s.ring = fr[i];
        s.chunks = (h->sched[i] + 15) / 16;
        s.last_ql = s.ring.quads - 4 * (s.chunks - 1);
        nin_base[i] = bb.region((size_t)s.chunks * 2 * 64 * 4, &s.w);
        stream_f32_image(&bb.v[nin_base[i]], s.ring.quads, s.chunks, 2, nin_get(i));
    }
    for (int i = 0; i < L; ++i) {
        const bool is_b2 = i == L - 1;
        StreamConv& cv = a.conv[i];
        cv.in = is_b2 ? a.b1 : fr[i];
        cv.lag = is_b2 ? 2 * L + 1 : 2 * (i + 1);
        cv.to_global = is_b2 ? 1 : 0;
        if (is_b2) { cv.out = StreamRing{-1, 0, pad4(nb) / 4, 0}; }
        else cv.out = fr[i + 1];
        const int quads = pad4(conv_cin(i)) / 4;
        const size_t base = bb.region((size_t)9 * quads * 4, &cv.dww);
        depthwise_rows(&bb.v[base], quads * 4, tens(h, conv_src(i).dw_w), 9, conv_cin(i));   // [3, 3, cin, 1]
    }
    // --- pointwise filters [chunk][tile][lane] float4, bias, slope of the streamed convs ---
    for (int i = 0; i < L; ++i) {
        const Op& src = conv_src(i);
        const int cin = conv_cin(i), chunks = (cin + 15) / 16, tiles = (src.segs[0].cout + 15) / 16;
        StreamConv& cv = a.conv[i];
        wp_base[i] = bb.region((size_t)chunks * tiles * 64 * 4, &cv.wp);
        stream_f32_image(&bb.v[wp_base[i]], pad4(cin) / 4, chunks, tiles, pw_get(i));
        ba_base[i] = bb.region(64, &cv.ba);
        stream_bias_slope(h, src, src.segs[0], src.segs[0].cout, &bb.v[ba_base[i]]);
    }
    {
        const size_t base = bb.region(64, &a.nin_ba);
        stream_bias_slope(h, nin, sb, sb.cout, &bb.v[base]);
        stream_bias_slope(h, nin, sa, sa.cout, &bb.v[base + pad4(nb)]);
    }
    const int lds = bb.lds;
    a.ldsw_src = 0;
    a.ldsw_bytes = lds - a.ring_bytes;
    if ((size_t)a.ldsw_bytes != bb.v.size() * sizeof(float)) return fail(h, DCSCN_ERR_UNSUPPORTED, "internal: feat_stream LDS image size");
    {
        // estimated cycles per row of the roles: 32 per MFMA + 4.5 per other VALU instruction
        auto ksteps = [](int quads) { const int ch = (quads + 3) / 4, ql = quads - 4 * (ch - 1); return 4 * (ch - 1) + (ql >= 3 ? 4 : ql); };
        std::vector<int> cost(1 + L);
        cost[0] = (int)(4.5 * 180);                               // CNN1
        int nin_mfma = 0;
        for (int i = 0; i < L; ++i) {
            const int chunks = (a.conv[i].in.quads + 3) / 4, tiles = (a.conv[i].out.quads + 3) / 4;
            cost[1 + i] = 32 * 3 * tiles * ksteps(a.conv[i].in.quads) + (int)(4.5 * (54 * chunks + 36 * tiles + 100));
            nin_mfma += 6 * ksteps(fr[i].quads);
        }
        if (!feat_stream_roles(cost, 32 * nin_mfma / L + (int)(4.5 * 85), L, a.role)) return fail(h, DCSCN_ERR_UNSUPPORTED, "internal: feat_stream role placement");
    }
    if (lds > 160 * 1024) return fail(h, DCSCN_ERR_UNSUPPORTED, "internal: feat_stream needs %d bytes of LDS", lds);

    // --- CNN1 (global, read once into registers): depthwise[9] (+3 pad), pointwise[32], bias[32], slope[32] ---
    {
        const ColSeg& sg = op.fused[1].segs[0];
        a.first_w = (int)bb.region(12 + 96);
        for (int k = 0; k < 9; ++k) bb.v[a.first_w + k] = tens(h, op.fused[0].dw_w)[k];
        for (int co = 0; co < sg.cout; ++co) bb.v[a.first_w + 12 + co] = tens(h, sg.w)[co];      // [1, 1, 1, C1]
        stream_bias_slope(h, op.fused[1], sg, sg.cout, &bb.v[a.first_w + 44]);
    }
    int rc = upload_vec(h, bb.v, &op.d_w);
    if (rc) return rc;
    // --- the F16 kernel's image: the same blob with the pointwise and A1 || B1 filters as f16 (hi, lo) fragments scaled by 2^e per GEMM,
    // the convs' biases times 2^e (they are the first MFMA's C operand); 2^-e goes to the kernel arguments ---
    std::vector<float> blob16 = bb.v;
    for (int i = 0; i < L; ++i) {
        const ColSeg& sg = conv_src(i).segs[0];
        const int cin = conv_cin(i);
        const int e = split16_scale_exp(tens(h, sg.w).data(), (size_t)cin * sg.cout);
        stream_f16_image(&blob16[wp_base[i]], pad4(cin) / 4, (sg.cout + 15) / 16, pw_get(i), e);
        for (int k = 0; k < 32; ++k) blob16[ba_base[i] + k] = std::ldexp(bb.v[ba_base[i] + k], e);
        a.conv[i].inv = std::ldexp(1.0f, -e);
    }
    {
        std::vector<float> all;
        for (int k = 0; k < k0[L]; ++k)
            for (int v = 0; v < 32; ++v) all.push_back(nin_column(h, sb, sa, nb, na, k, v));
        const int e = split16_scale_exp(all.data(), all.size());
        for (int i = 0; i < L; ++i) stream_f16_image(&blob16[nin_base[i]], a.nin[i].ring.quads, 2, nin_get(i), e);
        a.nin_inv = std::ldexp(1.0f, -e);
    }
    rc = upload_vec(h, blob16, &op.h16.d_w);
    op.h16.on = rc == DCSCN_OK;
    return rc;
}

// feat3_stream's wave -> SIMD placement (wave w runs on SIMD w & 3): deal the `waves` roles, heaviest first by cost (MFMAs per row), onto the
// least loaded SIMD that has a wave slot left; role_conv[i] = the role of cost[i] on entry, the role of wave i on return (-1: no such wave)
static void feat3_stream_roles(const std::vector<int>& cost, int waves, int8_t role_conv[kS3MaxWaves]) {
    std::vector<int> order(waves);
    for (int i = 0; i < waves; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return cost[x] > cost[y]; });
    int load[4] = {0, 0, 0, 0}, used[4] = {0, 0, 0, 0};
    int8_t rc[kS3MaxWaves];
    for (int w = 0; w < kS3MaxWaves; ++w) rc[w] = -1;
    for (int idx : order) {
        int pick = -1;
        for (int sd = 0; sd < 4; ++sd) {
            const int cap = (waves - sd + 3) / 4;
            if (used[sd] < cap && (pick < 0 || load[sd] < load[pick])) pick = sd;
        }
        rc[pick + 4 * used[pick]] = role_conv[idx];
        used[pick] += 1;
        load[pick] += cost[idx] + 20;
    }
    for (int w = 0; w < kS3MaxWaves; ++w) role_conv[w] = rc[w];
}

// ---- feat3_stream (feat3_stream.hpp): rings, role table and filter fragments of the fused CNN1 .. CNNL launch ---------------------
int pack_feat3_stream(dcscn_ctx* h, Op& op) {
    const bool nin_on = op.stream3.nin.on != 0;                 // fuse_feat3_stream: B1+A1 and B2 are part of the launch (op.fused[L], op.fused[L + 1])
    const int L = (int)op.fused.size() - (nin_on ? 2 : 0);
    for (Op& sub : op.fused) {                      // the layers' own launches: the float32 plan of a flagged image, and split16 = 0
        const int rc = finalize_op(h, sub);
        if (rc) return rc;
    }
    Stream3Args& a = op.stream3;
    a = Stream3Args{};
    a.L = L;
    a.nin.on = nin_on ? 1 : 0;
    a.total_lag = nin_on ? 2 * L + 1 : 2 * (L - 1);             // (B2 computes stream row t - (2 L + 1): two behind the row A1 || B1 finishes at step g + 2 L - 1)
    int lds = 0;
    std::vector<S3Ring> ring(L);
    for (int i = 0; i < L; ++i) {
        const int octs = (h->sched[i] + 7) / 8;
        const bool has = i + 1 < L || nin_on;                    // the last layer's rows are read by the A1 || B1 waves only
        ring[i] = S3Ring{lds, has ? (2 * octs + 1) * 16 : 0, octs};
        if (has) lds += 4 * kStreamRowPx * ring[i].px;           // four slots (feat3_stream.hpp)
    }
    if (nin_on) {
        a.nin.b1 = S3Ring{lds, 3 * 16, 1};
        lds += 4 * kStreamRowPx * a.nin.b1.px;
    }
    a.ring_bytes = lds;
    if (lds > 160 * 1024) return fail(h, DCSCN_ERR_UNSUPPORTED, "internal: feat3_stream needs %d bytes of LDS", lds);
    a.first_out = ring[0];
    BlobBuilder bb;                                 // (global memory: the kernel reads its fragments from there)
    {   // CNN1: filter [9][32] (tap major), bias [32], slope - 1 [32]
        const ColSeg& sg = op.fused[0].segs[0];
        const int C = h->sched[0];
        a.first_w = (int)bb.region(288 + 64);
        const std::vector<float>& w = tens(h, sg.w);           // [3, 3, 1, C]
        for (int t = 0; t < 9; ++t)
            for (int co = 0; co < C; ++co) bb.v[(size_t)t * 32 + co] = w[(size_t)t * C + sg.col0 + co];
        stream_bias_slope(h, op.fused[0], sg, C, &bb.v[288]);
    }
    // a 3x3 conv of the stream: conv[ci] computes `cout` channels from the `cin` channels of ring `in`; fragments [step][tile][hi | lo][64 lanes][8 halfs]
    auto pack_conv = [&](int ci, const Op& o, int cin, int cout, const S3Ring& in, const S3Ring& out, int lag) {
        const ColSeg& sg = o.segs[0];
        const int octs = in.octs, steps = (9 * octs + 3) / 4, tiles = (cout + 15) / 16;
        S3Conv& cv = a.conv[ci];
        cv.in = in;
        cv.out = out;
        cv.lag = lag;
        cv.tiles = tiles;
        const std::vector<float>& w = tens(h, sg.w);           // [3, 3, cin, cout_total]
        const int wcols = tens_cols(h, sg.w);
        std::vector<float> all((size_t)9 * cin * cout);
        for (int t = 0; t < 9; ++t)
            for (int c0 = 0; c0 < cin; ++c0)
                for (int co = 0; co < cout; ++co) all[((size_t)t * cin + c0) * cout + co] = w[((size_t)t * cin + c0) * wcols + sg.col0 + co];
        const int e = split16_scale_exp(all.data(), all.size());
        cv.inv = std::ldexp(1.0f, -e);
        cv.w_off = (int)bb.region((size_t)steps * tiles * 2 * 64 * 4);
        uint16_t* d16 = reinterpret_cast<uint16_t*>(&bb.v[cv.w_off]);
        for (int s = 0; s < steps; ++s)
            for (int n = 0; n < tiles; ++n)
                s3_f16_fragment(d16 + (size_t)(s * tiles + n) * 2 * 64 * 8, [&](int q, int t8, int i) {
                    const int p = 4 * s + q, tap = p / octs, c0 = 8 * (p - tap * octs) + t8, co = 16 * n + i;
                    return tap < 9 && c0 < cin && co < cout ? all[((size_t)tap * cin + c0) * cout + co] : 0.0f;
                }, e);
        cv.ba_off = (int)bb.region(64);
        stream_bias_slope(h, o, sg, cout, &bb.v[cv.ba_off], e);
        return 9 * steps * tiles;                               // MFMAs per row
    };
    int waves = 0;
    std::vector<int> cost;                          // MFMAs per row of each wave
    a.role_conv[waves] = -1; cost.push_back(0); ++waves;
    int pair_cost[2] = {0, 0};
    for (int i = 1; i < L; ++i) {
        const int mf = pack_conv(i - 1, op.fused[i], h->sched[i - 1], h->sched[i], ring[i - 1], ring[i], 2 * i);
        if (nin_on && i >= L - 2) { pair_cost[0] += mf; continue; }             // conv[L - 3], conv[L - 2] share a wave
        if (nin_on && i == L - 3) { pair_cost[1] += mf; continue; }             // conv[L - 4] shares one with B2
        if (waves >= kS3MaxWaves) return fail(h, DCSCN_ERR_UNSUPPORTED, "internal: feat3_stream needs more than %d waves", kS3MaxWaves);
        a.role_conv[waves] = (int8_t)(i - 1); cost.push_back(mf); ++waves;
    }
    if (nin_on) {
        const dcscn_config& c = h->cfg;
        const int nb = c.nin_filters2, na = c.nin_filters;      // 8, 24 (fuse_feat3_stream)
        const Op& nin = op.fused[L];
        pair_cost[1] += pack_conv(L - 1, op.fused[L + 1], nb, nb, a.nin.b1, S3Ring{0, 0, 1}, 2 * L + 1);
        if (waves + 4 > kS3MaxWaves) return fail(h, DCSCN_ERR_UNSUPPORTED, "internal: feat3_stream with A1 || B1 needs more than %d waves", kS3MaxWaves);
        for (int k = 0; k < 2; ++k) { a.role_conv[waves] = (int8_t)(kS3RolePair + k); cost.push_back(pair_cost[k] + 60); ++waves; }   // (+ a second conv's fixed work)
        // A1 || B1: conv channel c < nb = B1 channel c, else A1 channel c - nb; the K axis layer by layer, one K = 32 fragment per (layer, tile)
        const ColSeg& sb = nin.segs[0];
        const ColSeg& sa = nin.segs[1];
        int ktot = 0;
        for (int i = 0; i < L; ++i) ktot += h->sched[i];
        std::vector<float> all((size_t)ktot * 32, 0.0f);
        for (int k = 0; k < ktot; ++k)
            for (int v = 0; v < 32; ++v) all[(size_t)k * 32 + v] = nin_column(h, sb, sa, nb, na, k, v);
        const int e = split16_scale_exp(all.data(), all.size());
        a.nin.inv = std::ldexp(1.0f, -e);
        a.nin.w_off = (int)bb.region((size_t)L * 2 * 2 * 64 * 4);
        uint16_t* d16 = reinterpret_cast<uint16_t*>(&bb.v[a.nin.w_off]);
        int k0 = 0;
        for (int i = 0; i < L; ++i) {
            for (int n = 0; n < 2; ++n)
                s3_f16_fragment(d16 + (size_t)(i * 2 + n) * 2 * 64 * 8, [&](int q, int t8, int col) {
                    const int c0 = 8 * q + t8;                     // (a lane group past the layer's last octet re-reads that octet: zero rows here)
                    return c0 < h->sched[i] && 8 * q < 8 * ring[i].octs ? all[(size_t)(k0 + c0) * 32 + 16 * n + col] : 0.0f;
                }, e);
            k0 += h->sched[i];
        }
        a.nin.ba_off = (int)bb.region(64);
        stream_bias_slope(h, nin, sb, nb, &bb.v[a.nin.ba_off], e);
        stream_bias_slope(h, nin, sa, na, &bb.v[a.nin.ba_off + nb], e);
        for (int n = 0; n < 2; ++n) { a.role_conv[waves] = (int8_t)(kS3RoleNin + n); cost.push_back(9 * L); ++waves; }
    }
    a.n_waves = waves;
    feat3_stream_roles(cost, waves, a.role_conv);
    const int rc = upload_vec(h, bb.v, &op.d_w);
    op.h16.on = rc == DCSCN_OK;
    return rc;
}

}  // namespace dcscn_impl
