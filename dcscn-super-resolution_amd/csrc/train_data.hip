// Training batches on the device (helper/loader.py DynamicDataSets.load_batch_image, loader.py:278-355 of the reference):
// per patch a crop of HR = L s pixels of an image kept on the device -- or of one of its eight flipped / rotated variants
// (the files augmentation.py writes, DCSCN_AUG_*: an index map over the same pixels, so one upload serves all eight) --
// its Y (RGB) or its pixels (grey), fliplr, then
// LR = bicubic 1/s and x2 = bicubic s of LR as Pillow computes them -- mode "F" for the float Y of RGB images, mode "L" (8-bit
// fixed point) for grey images -- and the max_value / float32 cast rules of load_batch_image + train_batch (include/dcscn.h).
//
// A batch is, on one stream and without a host synchronisation:
//   batch_gather  (1 launch per 32 patches)  variant + crop + Y / grey + fliplr into compact HR planes (float32 for RGB patches, uint8
//                                            for grey ones, numbered in batch order per kind); writes y_true
//   resize_device (4 launches, RGB patches)  resample.hip's mode-"F" kernels: HR -> LR -> x2
//   resize_device_bytes (4 launches, grey patches) resample.hip's 8-bpc kernels: HR -> LR -> x2 through uint8 intermediates
//   batch_finish  (1 launch per 32 patches)  max_value and float32 cast of LR and x2 into x, x2
// Everything here is a few hundred KB of elementwise work per batch; the kernels are the plain one-thread-per-pixel form.
#include "plan.h"

#pragma clang fp contract(off)

namespace dcscn_impl {

struct TrainImage {
    uint8_t* px = nullptr;
    int H = 0, W = 0, C = 0;
};

struct TrainBatches {
    std::vector<TrainImage> images;
    float* planes = nullptr; size_t planes_cap = 0;   // the HR / LR / x2 planes of one batch (capacity in floats)
    float* out = nullptr; size_t out_cap = 0;         // dcscn_train_build_batch: x, x2, y_true before the copy to the host
};

namespace {

constexpr int kChunk = 32;          // patches per gather / finish launch (their descriptors travel as kernel arguments)

struct PatchDesc {
    const uint8_t* px;              // the image, [h, w, c] uint8
    int32_t h, w, c, top, left, flip;   // top, left: in the image as `code` transforms it ([w, h] for codes 4 .. 7)
    int32_t code;                   // DCSCN_AUG_*
    int32_t slot;                   // index among the batch's patches of the same kind (c == 3: float planes, c == 1: uint8 planes)
};
struct PatchChunk {
    PatchDesc p[kChunk];
};

// convert_rgb_to_y: numpy's image.dot(M.T) + 16 in float64, the FMA chain of color.hip's dot3 (bit-identical to the host)
__device__ __forceinline__ double luma(double r, double g, double b) {
    return __fma_rn(b, 25.064 / 256.0, __fma_rn(g, 129.057 / 256.0, r * (65.738 / 256.0))) + 16.0;
}

// Pixel (r, c) of the image as `code` transforms it -> its offset in the stored image [h, w]: the index maps of numpy's flipud,
// fliplr and rot90 in augmentation.py's order (include/dcscn.h, DCSCN_AUG_*).  `code` is uniform over a workgroup.
__device__ __forceinline__ size_t source_pixel(int code, int h, int w, int r, int c) {
    int sr, sc;
    switch (code) {
        case DCSCN_AUG_V: sr = h - 1 - r; sc = c; break;
        case DCSCN_AUG_H: sr = r; sc = w - 1 - c; break;
        case DCSCN_AUG_HV: sr = h - 1 - r; sc = w - 1 - c; break;
        case DCSCN_AUG_R1: sr = c; sc = w - 1 - r; break;
        case DCSCN_AUG_R2: sr = h - 1 - c; sc = r; break;
        case DCSCN_AUG_R1_V: sr = c; sc = r; break;
        case DCSCN_AUG_R2_V: sr = h - 1 - c; sc = w - 1 - r; break;
        default: sr = r; sc = c; break;
    }
    return (size_t)sr * w + sc;
}

// grid (ceil(HR^2 / 256), patches of the chunk); y_true is offset to the chunk's first patch
__global__ __launch_bounds__(256) void batch_gather_kernel(PatchChunk pc, int hr, int mul, double scale, float* __restrict__ yf,
                                                           uint8_t* __restrict__ y8, float* __restrict__ y_true) {
    const long long hr2 = (long long)hr * hr;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= hr2) return;
    const PatchDesc& d = pc.p[blockIdx.y];
    const int i = (int)(idx / hr), j = (int)(idx % hr);
    const size_t src = source_pixel(d.code, d.h, d.w, d.top + i, d.left + (d.flip ? hr - 1 - j : j));
    double v;
    if (d.c == 1) {
        const uint8_t u = d.px[src];
        y8[(size_t)d.slot * hr2 + idx] = u;
        v = (double)u;
    } else {
        const uint8_t* p = d.px + 3 * src;
        v = luma((double)p[0], (double)p[1], (double)p[2]);
        yf[(size_t)d.slot * hr2 + idx] = (float)v;          // Image.fromarray(float64): mode "F" holds float32(Y)
    }
    y_true[(size_t)blockIdx.y * hr2 + idx] = (float)(mul ? v * scale : v);
}

// load_batch_image's max_value rule and train_batch's float32 cast: float32 planes (RGB) times float32(scale); uint8 planes
// (grey) times scale in float64 (numpy: uint8 array * Python float -> float64)
__device__ __forceinline__ float cast_rgb(float v, int mul, double scale) { return mul ? v * (float)scale : v; }
__device__ __forceinline__ float cast_grey(uint8_t u, int mul, double scale) { return mul ? (float)((double)u * scale) : (float)u; }

// grid (ceil(HR^2 / 256), patches of the chunk); x, x2 offset to the chunk's first patch
__global__ __launch_bounds__(256) void batch_finish_kernel(PatchChunk pc, int lr, int hr, int mul, double scale, const float* __restrict__ f_lr,
                                                           const float* __restrict__ f_x2, const uint8_t* __restrict__ g_lr,
                                                           const uint8_t* __restrict__ g_x2, float* __restrict__ x, float* __restrict__ x2) {
    const long long hr2 = (long long)hr * hr, lr2 = (long long)lr * lr;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= hr2) return;
    const PatchDesc& d = pc.p[blockIdx.y];
    const size_t s_hr = (size_t)d.slot * hr2 + idx, s_lr = (size_t)d.slot * lr2 + idx;
    x2[(size_t)blockIdx.y * hr2 + idx] = d.c == 1 ? cast_grey(g_x2[s_hr], mul, scale) : cast_rgb(f_x2[s_hr], mul, scale);
    if (idx < lr2) x[(size_t)blockIdx.y * lr2 + idx] = d.c == 1 ? cast_grey(g_lr[s_lr], mul, scale) : cast_rgb(f_lr[s_lr], mul, scale);
}

static unsigned blocks(long long n) { return (unsigned)((n + 255) / 256); }

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

int check_patches(dcscn_ctx* h, PatchList p, int n, int lr_size, double max_value) {
    if (!h->train) return fail(h, DCSCN_ERR_STATE, "training batch before dcscn_train_begin");
    if (!p || n < 1) return fail(h, DCSCN_ERR_INVALID_ARG, "training batch: %d patches (need >= 1 and a patch array)", n);
    if (lr_size < 1) return fail(h, DCSCN_ERR_INVALID_ARG, "training batch: lr_size %d < 1", lr_size);
    if (!(max_value > 0.0) || !std::isfinite(max_value)) return fail(h, DCSCN_ERR_INVALID_ARG, "training batch: max_value %g is not > 0", max_value);
    const int64_t hr = (int64_t)lr_size * h->cfg.scale;
    const int count = h->batches ? (int)h->batches->images.size() : 0;
    for (int i = 0; i < n; ++i) {
        const dcscn_patch_aug q = p[i];
        if (q.image < 0 || q.image >= count) return fail(h, DCSCN_ERR_INVALID_ARG, "patch %d: unknown image %d (%d added)", i, q.image, count);
        if (q.fliplr != 0 && q.fliplr != 1) return fail(h, DCSCN_ERR_INVALID_ARG, "patch %d: fliplr %d is not 0 or 1", i, q.fliplr);
        if (q.transform < 0 || q.transform >= DCSCN_AUG_COUNT)
            return fail(h, DCSCN_ERR_INVALID_ARG, "patch %d: transform %d is not one of 0 .. %d", i, q.transform, DCSCN_AUG_COUNT - 1);
        const TrainImage& im = h->batches->images[q.image];
        const bool turned = q.transform >= DCSCN_AUG_R1;      // the rotated variants are [W, H]
        const int th = turned ? im.W : im.H, tw = turned ? im.H : im.W;
        if (q.top < 0 || q.left < 0 || q.top + hr > th || q.left + hr > tw) {
            if (q.transform == DCSCN_AUG_NONE)
                return fail(h, DCSCN_ERR_INVALID_ARG, "patch %d: the %lld x %lld crop at (top %d, left %d) is outside image %d (%d x %d)", i,
                            (long long)hr, (long long)hr, q.top, q.left, q.image, im.H, im.W);
            return fail(h, DCSCN_ERR_INVALID_ARG,
                        "patch %d: the %lld x %lld crop at (top %d, left %d) is outside image %d under transform %d (%d x %d)", i, (long long)hr,
                        (long long)hr, q.top, q.left, q.image, q.transform, th, tw);
        }
    }
    return DCSCN_OK;
}

// after check_patches; x [n, L, L], x2 and y_true [n, HR, HR] device buffers
int build_batch_device(dcscn_ctx* h, PatchList p, int n, int L, double max_value, float* x, float* x2, float* y_true, hipStream_t st) {
    TrainBatches* b = h->batches;
    const int s = h->cfg.scale, HR = L * s;
    const size_t hr2 = (size_t)HR * HR, lr2 = (size_t)L * L;
    int n_f = 0, n_g = 0;
    for (int i = 0; i < n; ++i) (b->images[p[i].image].C == 1 ? n_g : n_f) += 1;
    // planes: float32 HR, LR, x2 of the RGB patches, then uint8 HR, LR, x2 of the grey ones
    size_t off[6], bytes = 0;
    const size_t sizes[6] = {(size_t)n_f * hr2 * 4, (size_t)n_f * lr2 * 4, (size_t)n_f * hr2 * 4, (size_t)n_g * hr2, (size_t)n_g * lr2,
                             (size_t)n_g * hr2};
    for (int k = 0; k < 6; ++k) { off[k] = bytes; bytes += align256(sizes[k]); }
    int rc = grow(h, &b->planes, &b->planes_cap, bytes / 4, st);
    if (rc) return rc;
    char* base = reinterpret_cast<char*>(b->planes);
    float *f_hr = (float*)(base + off[0]), *f_lr = (float*)(base + off[1]), *f_x2 = (float*)(base + off[2]);
    uint8_t *g_hr = (uint8_t*)(base + off[3]), *g_lr = (uint8_t*)(base + off[4]), *g_x2 = (uint8_t*)(base + off[5]);
    // ordered behind a forward / resize of this handle on another stream (resize_device's row buffer rs_tmp is shared)
    if (h->has_last && h->last_stream != st) HIP_TRY(h, hipStreamWaitEvent(st, h->done_ev, 0));

    const int mul = max_value != 255.0;        // load_batch_image scales only when max_value != 255
    const double scale = max_value / 255.0;
    std::vector<PatchChunk> chunks((n + kChunk - 1) / kChunk);
    for (int i = 0, nf = 0, ng = 0; i < n; ++i) {
        const dcscn_patch_aug q = p[i];
        const TrainImage& im = b->images[q.image];
        chunks[i / kChunk].p[i % kChunk] = PatchDesc{im.px, im.H, im.W, im.C, q.top, q.left, q.fliplr, q.transform, im.C == 1 ? ng++ : nf++};
    }
    for (size_t c = 0; c < chunks.size(); ++c) {
        const int cnt = std::min(kChunk, n - (int)c * kChunk);
        hipLaunchKernelGGL(batch_gather_kernel, dim3(blocks((long long)hr2), cnt), dim3(256), 0, st, chunks[c], HR, mul, scale, f_hr, g_hr,
                           y_true + c * kChunk * hr2);
        HIP_TRY(h, hipGetLastError());
    }
    if ((rc = resize_device(h, f_hr, f_lr, n_f, HR, HR, L, L, st))) return rc;
    if ((rc = resize_device(h, f_lr, f_x2, n_f, L, L, HR, HR, st))) return rc;
    if ((rc = resize_device_bytes(h, g_hr, g_lr, n_g, HR, HR, 1, L, L, st))) return rc;
    if ((rc = resize_device_bytes(h, g_lr, g_x2, n_g, L, L, 1, HR, HR, st))) return rc;
    for (size_t c = 0; c < chunks.size(); ++c) {
        const int cnt = std::min(kChunk, n - (int)c * kChunk);
        hipLaunchKernelGGL(batch_finish_kernel, dim3(blocks((long long)hr2), cnt), dim3(256), 0, st, chunks[c], L, HR, mul, scale, f_lr, f_x2,
                           g_lr, g_x2, x + c * kChunk * lr2, x2 + c * kChunk * hr2);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipEventRecord(h->done_ev, st));
    h->last_stream = st;
    h->has_last = true;
    return DCSCN_OK;
}

void train_batches_free(dcscn_ctx* h) {
    TrainBatches* b = h->batches;
    if (!b) return;
    for (TrainImage& im : b->images) (void)hipFree(im.px);
    if (b->planes) (void)hipFree(b->planes);
    if (b->out) (void)hipFree(b->out);
    delete b;
    h->batches = nullptr;
}

// dcscn_train_build_batch and dcscn_train_build_batch_aug
static int build_batch_host(dcscn_ctx* h, PatchList patches, int n, int lr_size, double max_value, float* x, float* x2, float* y_true,
                            const char* who) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    int rc = check_patches(h, patches, n, lr_size, max_value);
    if (rc) return rc;
    if (!x || !x2 || !y_true) return fail(h, DCSCN_ERR_INVALID_ARG, "%s: null output buffer", who);
    HIP_TRY(h, hipSetDevice(h->device));
    TrainBatches* b = h->batches;
    const int s = h->cfg.scale;
    const size_t lr_n = (size_t)n * lr_size * lr_size, hr_n = lr_n * s * s;
    hipStream_t st = h->stream;
    if ((rc = grow(h, &b->out, &b->out_cap, lr_n + 2 * hr_n, st))) return rc;
    float *dx = b->out, *dx2 = dx + lr_n, *dy = dx2 + hr_n;
    if ((rc = build_batch_device(h, patches, n, lr_size, max_value, dx, dx2, dy, st))) return rc;
    HIP_TRY(h, hipMemcpyAsync(x, dx, lr_n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(x2, dx2, hr_n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(y_true, dy, hr_n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return DCSCN_OK;
}

}  // namespace dcscn_impl

extern "C" {

int dcscn_train_add_image(dcscn_handle h, const uint8_t* pixels, int height, int width, int channels, int32_t* image_id) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    if (!h->train) return fail(h, DCSCN_ERR_STATE, "dcscn_train_add_image before dcscn_train_begin");
    if (!pixels || !image_id) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_train_add_image: null pointer");
    if (height < 1 || width < 1) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_train_add_image: bad size %d x %d", height, width);
    if (channels != 1 && channels != 3)
        return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_train_add_image: %d channels (images have 1 (grey) or 3 (RGB))", channels);
    if (!h->batches) {
        h->batches = new (std::nothrow) TrainBatches();
        if (!h->batches) return fail(h, DCSCN_ERR_NOMEM, "out of host memory");
    }
    HIP_TRY(h, hipSetDevice(h->device));
    TrainImage im;
    im.H = height; im.W = width; im.C = channels;
    const size_t bytes = (size_t)height * width * channels;
    hipError_t e = hipMalloc((void**)&im.px, bytes);
    if (e != hipSuccess) return fail(h, DCSCN_ERR_NOMEM, "training image of %zu bytes: %s", bytes, hipGetErrorString(e));
    e = hipMemcpy(im.px, pixels, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(im.px);
        return fail(h, DCSCN_ERR_HIP, "dcscn_train_add_image: %s", hipGetErrorString(e));
    }
    h->batches->images.push_back(im);
    *image_id = (int32_t)(h->batches->images.size() - 1);
    return DCSCN_OK;
}

int dcscn_train_build_batch(dcscn_handle h, const dcscn_patch* patches, int n, int lr_size, double max_value, float* x, float* x2, float* y_true) {
    return build_batch_host(h, patches, n, lr_size, max_value, x, x2, y_true, "dcscn_train_build_batch");
}

int dcscn_train_build_batch_aug(dcscn_handle h, const dcscn_patch_aug* patches, int n, int lr_size, double max_value, float* x, float* x2,
                                float* y_true) {
    return build_batch_host(h, patches, n, lr_size, max_value, x, x2, y_true, "dcscn_train_build_batch_aug");
}

}  // extern "C"
