/*
 * dcscn.h -- C ABI of the MI355X-native DCSCN forward pass (libdcscn_hip.so).
 *
 * The reference (jiny2001/dcscn-super-resolution) has no FFI of its own: its forward pass is a
 * TensorFlow session call.  This header is the drop-in seam for that call; every entry point cites
 * the reference interface it stands in for (file:line into the reference tree).
 *
 *   reference                                                      this library
 *   ------------------------------------------------------------   ---------------------------
 *   SuperResolution.__init__ + build_graph  (DCSCN.py:29-106,222)   dcscn_create
 *   tf.train.Saver.restore by variable name (tf_graph.py:263-280)   dcscn_set_tensor (+ tensor_info)
 *   init_all_variables / first sess.run     (tf_graph.py:73-75)     dcscn_finalize
 *   sess.run(self.y_, {x, x2, dropout:1.0, is_training:0})          dcscn_forward / dcscn_forward_device
 *                                           (DCSCN.py:565-569,575-578)
 *   self-ensemble loop of do()              (DCSCN.py:559-573)      dcscn_forward_ensemble
 *   logging "Complexity" / layer list       (DCSCN.py:331-332)      dcscn_layer_info
 *   sess.close()                                                    dcscn_destroy
 *   build_optimizer                         (DCSCN.py:379-413)      dcscn_train_begin
 *   sess.run(training_optimizer, ...)       (DCSCN.py:727-769)      dcscn_train_step / dcscn_train_step_device
 *   DynamicDataSets.load_batch_image        (loader.py:278-355)     dcscn_train_add_image + dcscn_train_step_patches
 *   the same on augmentation.py's copies    (augmentation.py:36-70) dcscn_train_step_patches_aug (dcscn_patch_aug.transform)
 *   Saver.save / restore of the slots       (tf_graph.py:251-280)   dcscn_get_tensor / dcscn_set_train_tensor
 *
 * Conventions: plain C types only; all image tensors are dense NHWC float32 with C == 1
 * (x: [n, h, w, 1], x2 / y: [n, s*h, s*w, 1], s = scale).  Weights are passed exactly as the
 * checkpoint stores them (conv filters HWIO) under the checkpoint's variable names.  Every call
 * returns a dcscn_status; nothing aborts the process.  A handle owns one device, one HIP stream and
 * its workspace, and must not be used from two threads at once.  There is no CPU fallback: on a
 * machine without a usable HIP device dcscn_create fails with DCSCN_ERR_HIP.
 */
#ifndef DCSCN_H_
#define DCSCN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCSCN_ABI_VERSION 4
#define DCSCN_MAX_NAME 128

typedef struct dcscn_ctx* dcscn_handle;

typedef enum dcscn_status {
    DCSCN_OK = 0,
    DCSCN_ERR_INVALID_ARG = 1,    /* null pointer, bad size, bad enum */
    DCSCN_ERR_UNSUPPORTED = 2,    /* a flag combination the HIP path does not implement */
    DCSCN_ERR_MISSING_TENSOR = 3, /* finalize(): a variable the graph needs was never set
                                     (reference: Saver.restore raises NotFoundError) */
    DCSCN_ERR_SHAPE = 4,          /* set_tensor(): unknown name or shape mismatch */
    DCSCN_ERR_HIP = 5,            /* HIP runtime error / no device */
    DCSCN_ERR_STATE = 6,          /* call order violated (e.g. forward before finalize) */
    DCSCN_ERR_NOMEM = 7
} dcscn_status;

/* helper/tf_graph.py:77-102 build_activator */
typedef enum dcscn_activator {
    DCSCN_ACT_NONE = 0,
    DCSCN_ACT_PRELU = 1,
    DCSCN_ACT_RELU = 2,
    DCSCN_ACT_LEAKY_RELU = 3,
    DCSCN_ACT_SIGMOID = 4,
    DCSCN_ACT_TANH = 5,
    DCSCN_ACT_SELU = 6
} dcscn_activator;

/* Model flags of helper/args.py:17-36 as consumed by DCSCN.py:33-48 and build_graph. */
typedef struct dcscn_config {
    int32_t struct_size;            /* = sizeof(dcscn_config), ABI guard */
    int32_t scale;                  /* 2, 3 or 4 */
    int32_t layers;                 /* feature-extraction layers */
    int32_t filters;
    int32_t min_filters;
    double  filters_decay_gamma;
    int32_t cnn_size;               /* 3 (1 is accepted) */
    int32_t use_nin;
    int32_t nin_filters;            /* A1 */
    int32_t nin_filters2;           /* B1, B2 */
    int32_t reconstruct_layers;     /* max(flag, 1) applied inside, DCSCN.py:42 */
    int32_t reconstruct_filters;
    int32_t activator;              /* dcscn_activator */
    int32_t pixel_shuffler;         /* 1: pixel shuffler (tf_graph.py:238-249); 0: transposed conv "Up-TCNN"
                                       (tf_graph.py:219-236), run as its equivalent 3x3 conv + depth_to_space */
    int32_t pixel_shuffler_filters; /* 0 = same as input channels */
    int32_t depthwise_separable;
    int32_t channels;               /* must be 1 */
    int32_t legacy_no_c;            /* 1: graph of the shipped dcscn_L2_* checkpoints (use_nin=0 and
                                       no 1x1 "C" layer between H_concat and the upsampler) */
    int32_t batch_norm;             /* must be 0 */
    int32_t reserved[8];
} dcscn_config;

/* One conv layer of the graph, in build order (CNN1.., A1, B1, B2 | C, Up-PS.., R-CNN..). */
typedef struct dcscn_layer_info {
    char    name[DCSCN_MAX_NAME];   /* checkpoint scope, e.g. "CNN3", "Up-PS/Up-PS_CNN" */
    int32_t kernel_size;
    int32_t in_channels;
    int32_t out_channels;
    int32_t depthwise_separable;
    int32_t has_bias;
    int32_t activator;
    int32_t resolution;             /* pixels per LR pixel along one axis where the conv runs */
    int64_t macs_per_lr_pixel;      /* multiply-accumulates per LR pixel */
} dcscn_layer_info;

/* Library / ABI version (DCSCN_ABI_VERSION). */
int dcscn_abi_version(void);

/* Message of the last failing call on this thread that had no usable handle (e.g. dcscn_create). */
const char* dcscn_last_global_error(void);

/* Number of visible HIP devices, or a negative dcscn_status. */
int dcscn_device_count(void);

/* Feature-extraction filter schedule of DCSCN.py:232,240-244; writes `layers` ints. */
int dcscn_filter_schedule(int layers, int filters, int min_filters, double gamma, int32_t* out);

/* Build the graph for `cfg` on HIP device `device` (SuperResolution.__init__ + build_graph). */
int dcscn_create(const dcscn_config* cfg, int device, dcscn_handle* out);

/* Variables the graph expects, in checkpoint naming (tf_graph.py:117-216). shape has 4 slots. */
int dcscn_num_tensors(dcscn_handle h);
int dcscn_tensor_info(dcscn_handle h, int index, char* name, int name_capacity, int64_t* shape, int* rank);

/* Copy one variable in (Saver.restore); `shape`/`rank` must match the graph. Host memory. */
int dcscn_set_tensor(dcscn_handle h, const char* name, const float* data, const int64_t* shape, int rank);

/* Repack weights for the MFMA kernels and upload them.  All variables must have been set. */
int dcscn_finalize(dcscn_handle h);

/* Conv layers of the graph (for logging / FLOP accounting). */
int dcscn_num_layers(dcscn_handle h);
int dcscn_layer_info_get(dcscn_handle h, int index, dcscn_layer_info* out);

/* Kernel launches one forward pass is made of, in stream order (valid after dcscn_finalize).
 * A launch covers one graph layer, or two when they are fused (A1 and B1 share one GEMM). */
typedef struct dcscn_op_info {
    char    name[DCSCN_MAX_NAME];   /* e.g. "CNN2", "B1+A1", "CNN3/depthwise" */
    char    kernel[32];             /* "conv_igemm", "conv_wino", "conv_cin1", "conv_cout1", "depthwise" */
    int32_t kernel_size;
    int32_t in_channels;            /* logical */
    int32_t out_channels;           /* logical */
    int32_t resolution;
    int32_t mt, nt, kc, n_tiles;    /* conv_igemm variant (0 for the other kernels) */
    int64_t macs_per_lr_pixel;      /* algorithmic multiply-accumulates per LR pixel */
    int64_t bytes_per_lr_pixel;     /* algorithmic activation bytes read + written per LR pixel */
    int64_t executed_macs_per_lr_pixel; /* multiply-accumulates the kernel really issues: channel padding
                                       included, 16/36 of the direct form for the Winograd kernel */
} dcscn_op_info;
int dcscn_num_ops(dcscn_handle h);
int dcscn_op_info_get(dcscn_handle h, int index, dcscn_op_info* out);

/* Tunables: "sub_batch_pixels" (LR pixels processed per pass through the layer chain, default 4 Mi),
 * "workspace_budget_bytes" (caps the pass size so the activation workspace stays below it, default
 * 48 GiB; an image whose workspace alone exceeds it is cut into equally shaped windows overlapping by twice
 * the network's receptive-field radius, run as a batch and stitched -- "spatial_tiling" 0 disables that and
 * lets the allocation fail instead), "profile" (1: time every launch with HIP events, read back with dcscn_get_profile),
 * "winograd" (default 1; before dcscn_finalize only: 0 keeps every 3x3 conv on the direct
 * implicit-GEMM kernel instead of the Winograd F(2x2,3x3) kernel), "nin_gemm" (default 1; before dcscn_finalize only: 0 sends
 * the wide 1x1 convs -- A1 || B1 over the skip-concat -- to the generic implicit-GEMM kernel instead of conv_nin_h / conv_nin),
 * "fold_linear_tail" (default 1; before dcscn_finalize only): the last pixel-shuffler conv, depth_to_space and the last
 * reconstruction conv -- all linear, no activator between them, DCSCN.py:293-323 -- run as ONE 5x5 conv of the
 * low-resolution map with per-phase / per-border kernels composed in float64 from the checkpoint tensors; the same
 * function, f32 results differ from the layer-by-layer graph by re-association only (parity-tested against the float64
 * oracle at the same 1e-4 bar).  0 = the escape hatch: execute the reference's layers one by one.  Ignored where the
 * graph has no such tail: separable convs, transposed-conv upsampler, reconstruct_layers > 1, cnn_size != 3 -- and,
 * with the default value 1, where the composite would be MORE work than the layers (pixel shufflers to fewer than 12
 * channels at x2: the c-DCSCN nets); 2 folds there too.  The work rule is evaluated ONCE, in dcscn_finalize, for the "split16"
 * value in force then (a one-tile composite is cheap on conv5_h and folds; on the f32 kernel it would not): a handle whose
 * split16 option is flipped afterwards keeps the plan it was finalized with.
 * "fold_whole_tail" (default 1; before dcscn_finalize only; needs fold_linear_tail != 0 and split16 = 1 at finalize): at x3 and x4 EVERY
 * pixel-shuffler stage is built without an activator (tf_graph.py:238-249 as called from DCSCN.py:300-311), so the whole tail -- Up-PS,
 * depth_to_space, (Up-PS2, depth_to_space,) the last reconstruction conv, dense or depthwise separable -- is one affine map of the LR tensor:
 * a 5x5 conv to scale^2 <= 16 sub-pixel phases (ONE channel tile) whose kernel differs only on the first / last row and column of the
 * image, where the reference zero-pads the SHUFFLED maps.  One launch computes the interior with the interior kernels, a second one the
 * border ring with the kernels of its 15 (row, column) position classes, all composed in float64 (csrc/pack.hip: pack_foldx); the launches it
 * replaces -- the shuffler conv(s), the r05 fold of the last stage, tail_stream -- remain the float32 plan of a flagged image and the
 * split16 = 0 path.  Same function, same parity bars.  0 = the r05 plans.
 * "dense_features" (default 1; before dcscn_finalize only): every feature layer stores into its own dense NHWC buffer and
 * the 1x1 layer(s) that consume tf.concat (DCSCN.py:234) walk the list of buffers, instead of all layers sharing one
 * [n, h, w, sum C_i] tensor -- same bits, full cache lines.  0 = one concat tensor.  Ignored where a consumer of the
 * concat is not a 1x1 GEMM launch (cnn_size > 1 reconstruction without NIN).
 * "stream_features" / "stream_tail" (default 1; before dcscn_finalize only): the separable narrow nets (depthwise_separable,
 * <= 7 feature layers of <= 32 filters, NIN of <= 32 channels) run CNN1 .. CNNL, A1 || B1 and B2 as ONE row-streamed launch
 * with every intermediate tensor in LDS, and -- x4 models with a 32-channel pixel shuffler -- Up-PS, Up-PS2, the last
 * reconstruction conv and the residual add as a second one.  0 = the layer-by-layer launches (same function, f32 results
 * differ by accumulation order only).
 * "stream_dense" (default 1; before dcscn_finalize only): the NON-separable narrow nets (plain 3x3 feature layers of <= 32 filters --
 * the c-DCSCN checkpoints) run CNN1 .. CNNL as one row-streamed launch on the f16 matrix pipe (csrc/feat3_stream.hpp: three-row rings of
 * pre-split units in LDS, filter fragments in registers, every layer's rows written once for A1 || B1); with split16 = 0, and for a
 * flagged image, the layers run one by one.  0 = always layer by layer.
 * "stream_nin" (default 1; before dcscn_finalize only): in that launch also A1 || B1 -- accumulated in registers as the layers' rows appear in
 * their LDS rings -- and B2, where the net has the c-DCSCN shape (7 feature layers, nin_filters 24, nin_filters2 8): no feature map is
 * written to device memory, Concat2 [B2 | A1] is the launch's only output (DCSCN.py:258-291).  0 = every layer's rows go to device memory
 * and the 1x1 GEMM reads them back (the r05 plan; same function, f32 results differ by accumulation order only).
 * "split16" (default 1; any time): the 3x3 convs the Winograd kernel would take and the wide 1x1 convs run their contraction
 * on the f16 matrix pipe at f32 accuracy -- every f32 operand as an f16 (hi, lo) pair, three products per MAC, f32
 * accumulation; measured error at the f32 kernels' level (profiles/r03_f16x3_numerics.txt).  Weights are scaled
 * by a power of two per layer before the split; activations are split unscaled, so below |x| ~ 2^-3 their `lo` piece is an f16
 * subnormal and the pair carries an ABSOLUTE error floor of ~3e-8 per element instead of a relative 2^-22 -- immaterial for the
 * network's data (tested: inputs in [0, 1] as --max_value=1 feeds them meet the same 5e-6 bar on the bare branch,
 * test_small_magnitude_inputs_on_split16), but not "f32 accuracy for any input".  Per layer the split16 kernels are about twice
 * as far from the float64 value as the f32 Winograd kernel (max error 2.9e-4 against 1.4e-4 on outputs of magnitude 260, rms 1.8e-5
 * against 1.6e-5: profiles/r04_h16_conv3_harness.txt); end to end both families meet the same bars.  An activation beyond the f16
 * range (|x| >= 65520) cannot be carried as a pair: the launch that meets it (a non-finite accumulator) or produces it (a P16 output,
 * see "p16") raises the IMAGE's redo flag, and behind every pass the float32 launches of all layers run once more, gated by those
 * flags: a flagged image is recomputed from the first layer on by the float32 kernels (bit-identical to a split16 = 0 run of
 * that image), every other image of the batch keeps its split16 bits -- results never depend on what else is in the batch.  With no
 * flag set (always, for image data) the gated launches exit at once.
 * 0 = the pure f32 kernels (conv_wino2 / conv_nin).
 * "p16" (default 1; any time, the next forward re-carves the workspace): tensors that only split16 launches write and read (the
 * feature maps, B1, Concat2) are kept PRE-SPLIT in the workspace -- per pixel and 32-channel chunk one aligned 128-byte record of
 * f16 (hi | lo) units instead of float32 values, same 4 bytes per value (csrc/p16.hpp) -- so the split happens once, in the producer's
 * epilogue, and the consumers stage their input tiles by LDS-DMA.  Same split, same products in the same order: results are
 * bit-identical to p16 = 0.  Needs split16 = 1 (both kernel families); otherwise the float32 tensors of r04 are used.
 * "conv3_h8" (default 1; any time): 3x3 layers whose output channels form two channel groups (7 .. 12 tiles of 16) run on
 * conv3_h8 -- one persistent 8-wave workgroup per CU that stages a pixel tile's input once for both groups -- instead of two
 * conv3_h workgroups per tile; same filter image, bit-identical results.
 * "nin_h8" (default 1; any time): the split16 1x1 GEMMs with K >= 1024 input channels, P16 sources and six full output tiles
 * (A1 || B1 of the L12 nets) run on 256-pixel workgroups of conv_nin_h -- half the filter traffic per pixel -- instead of 128-pixel
 * ones; same filter image, same products in the same order, bit-identical results.  0 = 128-pixel workgroups everywhere.
 * "fast16" (default 0; any time, like "split16"): an opt-in LOWER-PRECISION inference mode.  With 1, every launch on conv3_h, conv3_h8
 * (float32 or P16 tensors), conv_nin_h (both workgroup sizes) and conv5_h with fold_border -- the layer kernels of "split16" -- takes each
 * contraction as the SINGLE product wh * xh: the activation rounded to f16, the weight (scaled by the layer's power of two) rounded to f16,
 * the product exact and accumulated in f32.  The two products that carry the last 11 bits of each operand are not issued and their `lo`
 * operands not read from LDS.  Everything else is split16's: the filter images and P16 records still hold (hi | lo) and epilogues still write
 * both (a later fast16 = 0, or a launch that keeps three products, reads them as before), the 2^-e scale, bias, activators and the residual
 * add run in f32, and the redo flags and the gated float32 plan work as described under "split16" -- a flagged image is still recomputed to
 * the bits of a split16 = 0 run, bystanders keep their fast16 bits.  The streamed kernels (feat_stream, tail_stream, feat3_stream) keep
 * three products under this option (feat3_stream has its own: "fast16_stream" below), so the narrow nets change only in their folded
 * tail; split16 = 0 ignores the option.
 * Error against the float64 oracle on the 0-255 scale (seeded weights, U(0, 255) input), CPU model of the mode: max-abs 2.2e-3, rms 5.6e-4
 * for L12 x2, 3.7e-3 / 9.4e-4 for L12 x4, 2.6e-3 / 8.3e-4 for L8 x2, 1.5e-3 / 4.4e-4 for c-DCSCN x2 -- about a hundred times split16's
 * 1.5e-5 and 1/200 of an 8-bit step.  Measured on an MI355X: 2.3e-3 / 6.2e-4 (L12 x2), 3.1e-3 / 8.0e-4 (L12 x4), 3.5e-3 / 8.7e-4 (L8 x2);
 * with the shipped c-DCSCN x2 weights, layer by layer, 1.3e-2 / 1.5e-3.  A 1024-patch pass of L12 x2 takes 0.667 of its time (DESIGN.md
 * 3.13).  Not f32 accuracy, not bf16 / fp8, not for training.
 * "fast16_stream" (default 0; any time, like "fast16", and independent of it: all four combinations are legal): the same mode for the
 * feat3_stream launch of the non-separable narrow nets (c-DCSCN), which "fast16" leaves on three products.  With 1, every matrix
 * contraction inside that launch -- CNN2 .. CNNL and, where "stream_nin" puts them there, A1 || B1 and B2 -- is the single product
 * wh * xh: the `hi` piece of the ring unit, which is f16(x), times the `hi` piece of the scaled filter image, accumulated in f32; the
 * `lo` filter fragments are not loaded, the `lo` ring units not read and their two products not issued.  CNN1 stays f32 VALU work, the
 * filter blob still holds (hi | lo), epilogues still write (hi | lo) units to the rings and to global memory (conv_nin_h behind
 * stream_nin = 0, the tail kernels and a later fast16_stream = 0 read what they always read), and scale, bias, PReLU, the redo flags and
 * the gated float32 plan are split16's.  Ignored where the plan has no feat3_stream launch: split16 = 0, stream_dense = 0, the wide nets,
 * and the separable nets' feat_stream / tail_stream, which keep three products.  Error and speed: DESIGN.md 3.13.
 * "fast16_separable" (default 0; any time, like "fast16", and independent of it and of "fast16_stream": every combination is legal): the
 * same mode for the feat_stream and tail_stream launches of the depthwise-separable narrow nets, which the two options above leave on
 * three products.  With 1, every matrix contraction inside such a launch -- the pointwise stage of CNN2 .. CNNL and B2, A1 || B1, and in
 * tail_stream Up-PS and Up-PS2 -- is the single product wh * xh: xh = f16 (round to nearest even) of the f32 value the lane holds (the
 * depthwise output; for A1 || B1 the ring value), wh = the `hi` half of the scaled f16 filter image, accumulated in f32; the `lo` halves
 * of the activations are not computed, the `lo` filter fragments not loaded and the two cross products not issued.  CNN1 and R-CNN1 stay
 * f32 VALU work, the depthwise stage stays f32, the filter blob still holds (hi | lo) (a later fast16_separable = 0 reads what it always
 * read), and bias, the 2^-e scale, PReLU, the rings, the redo flags and the gated float32 plan are split16's -- a flagged image is still
 * recomputed to the bits of a split16 = 0 run.  Ignored where the plan has no such launch: split16 = 0, stream_features = 0 /
 * stream_tail = 0, widths feat_stream does not take, every non-separable net, and the layer-by-layer separable kernels (depthwise,
 * conv_igemm with a fused depthwise stage).  Error and speed: DESIGN.md 3.13.
 * "train_split16" (default 0; any time, also before dcscn_train_begin; takes effect from the next gradient computation, which re-carves
 * the training workspace): an opt-in training mode at the f32 path's accuracy.  With 1, every layer of the training plan with
 * min(cin, cout) >= 16 -- a rule of the layer's shape alone, the same for both directions -- takes its forward conv and its data-gradient
 * conv on the f16 matrix pipe (tconv_gemm_h) as three f16 products wh * xh + wh * xl + wl * xh per multiply-accumulate, accumulated in
 * f32; narrower layers (CNN1, the last R-CNN), the weight gradients, activators, dropout, loss, clipping, the optimizers and the record
 * calls are the f32 path's, and the weight gradient consumes the dz the split16 data gradient produced.  Unlike the inference "split16",
 * EVERY operand is scaled before it is split: the layer's input slice, dz and the filter are multiplied by 2^e, e chosen on the device
 * (a max reduction: no atomics, no host synchronisation) so that the tensor's largest magnitude lies in [2^13, 2^14); e = 0 for an
 * all-zero tensor and |e| <= 126.  Gradients of 1e-6 and below therefore keep their lo pieces normal, no operand can leave the f16 range,
 * and the mode has no redo flags and no float32 fallback; the epilogue undoes both scales with ldexp (exact).  A non-finite value in an
 * operand gives non-finite results, as on the f32 path.  Same parity bars as the default mode (1e-4 * max|g| per gradient tensor),
 * deterministic, but not the default mode's bits.  0 allocates and launches exactly what a handle that never set the option does.
 * "train_split16_wgrad" (default 0; any time, also before dcscn_train_begin; takes effect from the next gradient computation, which
 * re-carves the training workspace; independent of "train_split16": all four combinations are legal): with 1, every layer of the training
 * plan with min(cin, cout) >= 16 -- the same rule of the shape -- takes its WEIGHT gradient on the f16 matrix pipe (tconv_wgrad_h): the sum
 * over the pixels of in[p + tap][ci] * dz[p][co] as three f16 products ah * bh + ah * bl + al * bh per multiply-accumulate in chunks of 32
 * pixels, accumulated in f32, both operands scaled by the power of two described above (found once per layer and step and shared with the
 * "train_split16" convs when both options are on) and the scale undone with ldexp.  The pixels are summed over a fixed partition into tiles
 * in a fixed order and the partial sums in split order, without atomics: deterministic, though not in the f32 kernel's order.  Narrower
 * layers, the bias and PReLU-slope gradients, the l2 term and everything else are untouched: only the conv_W gradients of eligible layers
 * (and with them the gradient norm) change bits.  Same parity bars as the default mode; a non-finite operand gives a non-finite result;
 * 0 computes every bit of what a handle that never set the option computes, for either setting of "train_split16".
 * "train_separable" (default 0; read by dcscn_train_begin alone): with 1, dcscn_train_begin builds the training plan of a
 * depthwise-separable net instead of refusing it ("Training" below: the semantics and the known departure); with 0 the refusal, its
 * status and its text are unchanged.  No effect on non-separable configs, and none after dcscn_train_begin.
 * "train_transposed" (default 0; read by dcscn_train_begin alone): with 1, dcscn_train_begin builds the training plan of a net with the
 * transposed-conv upsampler (pixel_shuffler = 0, layer Up-TCNN) instead of refusing it ("Training" below); with 0 the refusal, its status
 * and its text are unchanged.  No effect on pixel-shuffler configs, and none after dcscn_train_begin.  A net that is both separable and
 * transposed needs this option and "train_separable"; with one of them set the refusal names the other.
 * "train_optimizers" (default 0; read by dcscn_train_begin alone): with 1, dcscn_train_begin accepts DCSCN_OPTIMIZER_ADADELTA, _ADAGRAD and
 * _RMSPROP ("Training" below: the rules, the fixed constants, the slots) instead of refusing them; with 0 the refusal, its status and its
 * text are unchanged.  No effect on adam, gd or momentum, whose kernel is not the one these three run, and none after dcscn_train_begin.
 * "graph_replay" (default 0; any time): a dcscn_forward_device call whose arguments repeat (same x / x2 / y pointers, shape and
 * stream) is captured into a hipGraph the second time it is seen and replayed from then on: one graph launch instead of the
 * pass's ~30 kernel launches (the launch gaps are 0.4 % of a 1024-patch pass of the L12 model, 3 % for the narrow nets).  The
 * data in the buffers may change between calls, the pointers may not; any other call falls back to plain launches. */
int dcscn_set_option(dcscn_handle h, const char* key, int64_t value);

/* Forward pass on host buffers: H2D, kernels, D2H, synchronous. */
int dcscn_forward(dcscn_handle h, const float* x, const float* x2, float* y, int n, int height, int width);

/* Bicubic resize of `n` single-channel float images [height, width] -> [out_height, out_width], bit-compatible
 * with Pillow's Image.resize(BICUBIC) on mode-"F" images (a = -0.5 cubic, antialiased when shrinking, float64
 * accumulation, horizontal pass first): replaces util.resize_image_by_pil (helper/utilty.py:211-239) for the
 * single-channel images of the path.  Host buffers, synchronous; the _device form takes device pointers and a
 * hipStream_t (NULL = the handle's stream) and does not synchronise.  Usable before dcscn_finalize. */
int dcscn_resize_bicubic(dcscn_handle h, const float* in, float* out, int n, int height, int width,
                         int out_height, int out_width);
/* The per-axis tables the resize uses (Pillow's precompute_coeffs for BICUBIC over the whole axis): for output
 * index i, `bounds[2i]` = first input index, `bounds[2i+1]` = taps, `weights[i * ksize + t]` = normalised float64
 * weight of tap t.  Host only, needs no device.  Call with bounds = weights = NULL to get `ksize`; `capacity` is
 * the number of doubles `weights` can hold (>= out_size * ksize). */
int dcscn_resample_table(int in_size, int out_size, int* ksize, int* bounds, double* weights, int capacity);
int dcscn_resize_bicubic_device(dcscn_handle h, const float* in, float* out, int n, int height, int width,
                                int out_height, int out_width, void* stream);

/* The 8-bit form of dcscn_resample_table (Pillow's normalize_coeffs_8bpc: the weights as int32 with 22 fraction bits,
 * rounded half away from zero): bounds as there, `coeffs[i * ksize + t]`.  Host only, needs no device; NULL tables query
 * `ksize`; `capacity` is the number of int32 values `coeffs` can hold. */
int dcscn_resample_table_bytes(int in_size, int out_size, int* ksize, int* bounds, int32_t* coeffs, int capacity);
/* Image.resize(BICUBIC) of `n` uint8 images of mode "L" (channels = 1) or "RGB" (channels = 3, interleaved), bit-identical
 * to Pillow (int32 fixed point, horizontal pass into a uint8 intermediate, then the vertical pass): replaces
 * util.resize_image_by_pil for the 8-bit images of sr.py / evaluate.py.  Host buffers, synchronous; the _device form takes
 * device pointers of any alignment and a hipStream_t (NULL = the handle's stream) and does not synchronise.  Usable before
 * dcscn_finalize.  Other channel counts: DCSCN_ERR_INVALID_ARG. */
int dcscn_resize_bicubic_bytes(dcscn_handle h, const uint8_t* in, uint8_t* out, int n, int height, int width, int channels,
                               int out_height, int out_width);
int dcscn_resize_bicubic_bytes_device(dcscn_handle h, const uint8_t* in, uint8_t* out, int n, int height, int width, int channels,
                                      int out_height, int out_width, void* stream);

/* do(input_image, bicubic_input_image=None) (DCSCN.py:547-554): x2 is the bicubic upscale of x, computed on the
 * device with dcscn_resize_bicubic; otherwise as dcscn_forward. */
int dcscn_forward_lr(dcscn_handle h, const float* x, float* y, int n, int height, int width);

/* Forward pass on device buffers, enqueued on `stream` (a hipStream_t, NULL = the handle's own
 * stream, see dcscn_get_stream) without synchronising.  Workspace growth (first call / larger shape) does
 * synchronise.  Consecutive calls on DIFFERENT streams are ordered by the library (they share the workspace): the
 * later call waits, on the device, for the earlier one.  The reference analogue is a second sess.run on the same
 * session (DCSCN.py:565-569): it simply runs after the first. */
int dcscn_forward_device(dcscn_handle h, const float* x, const float* x2, float* y,
                         int n, int height, int width, void* stream);

/* The handle's own hipStream_t (created non-blocking: it does NOT synchronise with the legacy default stream), so a
 * caller that passes stream = NULL above can order its own work against it (hipStreamWaitEvent / hipStreamSynchronize). */
int dcscn_get_stream(dcscn_handle h, void** stream);

/* Blocks until every forward / resize enqueued through this handle has finished, whatever stream it ran on
 * (sess.run is synchronous; this is the explicit form for the _device entry points). */
int dcscn_synchronize(dcscn_handle h);

/* do() with self_ensemble = n_ensemble in [1, 8] for ONE image (DCSCN.py:559-573): the flipped /
 * rotated copies (utilty.py:595-617) run as two batches on the device; the mean over copies is
 * accumulated in float64 in the reference's order.  x: [h, w], x2: [s*h, s*w], y: float64 [s*h, s*w]. */
int dcscn_forward_ensemble(dcscn_handle h, const float* x, const float* x2, double* y,
                           int height, int width, int n_ensemble);

/* Colour conversions of helper/utilty.py:142-193 on the device, float64 like the reference's numpy (host buffers,
 * synchronous; usable before dcscn_finalize).  rgb: uint8 [n_pixels, 3] interleaved.
 *   dcscn_convert_rgb_to_y            utilty.py:142-149   y     float64 [n_pixels]     = [65.738 129.057 25.064]/256 . rgb + 16
 *   dcscn_convert_rgb_to_ycbcr        utilty.py:152-165   ycbcr float64 [n_pixels, 3]
 *   dcscn_convert_y_and_cbcr_to_rgb   utilty.py:168-193   y float64 [n_pixels], cbcr float64 [n_pixels, 2] -> rgb float64 [n_pixels, 3] */
int dcscn_convert_rgb_to_y(dcscn_handle h, const uint8_t* rgb, double* y, int64_t n_pixels);
int dcscn_convert_rgb_to_ycbcr(dcscn_handle h, const uint8_t* rgb, double* ycbcr, int64_t n_pixels);
int dcscn_convert_y_and_cbcr_to_rgb(dcscn_handle h, const double* y, const double* cbcr, double* rgb, int64_t n_pixels);

/* do_for_evaluate's image pipeline (DCSCN.py:672-703, loader.py:42-67) with ONE upload: the aligned true image
 * (uint8 RGB [height, width, 3], both multiples of the scale) -> Y in float64 (convert_rgb_to_y) -> LR = Pillow BICUBIC
 * of the mode-'F' Y at 1/scale -> x2 = BICUBIC of LR at scale -> do() with self_ensemble = n_ensemble.
 * Outputs (host): y float64 [height, width] (n_ensemble == 1: the float32 network output, widened), and optionally
 * true_y float64 [height, width] (what the PSNR is measured against) and lr float32 [height/s, width/s]. */
int dcscn_evaluate_rgb(dcscn_handle h, const uint8_t* rgb, int height, int width, int n_ensemble,
                       double* true_y, float* lr, double* y);

/* PSNR and SSIM as evaluate.py reports them (compute_psnr_and_ssim, utilty.py:509-536), computed on the device.  Both images are
 * trimmed like a saved file (rint, half to even, then clipped to [0, 255]) and shaved by border_size pixels on every side.
 *   sq_err_sum, n_pixels   exact integers over the shaved pixels; psnr = 10 log10(255^2 / (sq_err_sum / n_pixels)), formed on the
 *                          host from the two, +inf when sq_err_sum is 0
 *   ssim                   what the reference's multichannel=True call on 2-D arrays yields: the mean over image columns of a
 *                          1-D SSIM down each column (11-tap Gaussian window, sigma 1.5, sample covariance), taken over the rows
 *                          whose window lies inside the shaved image.  float64; two calls give the same bits.
 * DCSCN_ERR_INVALID_ARG with "win_size" in the message: fewer than 11 rows or no column left after shaving, or a negative
 * border_size (the reference raises "win_size exceeds image extent").  Pixel values must be finite. */
typedef struct dcscn_metrics {
    double  psnr;
    double  ssim;
    int64_t sq_err_sum;
    int64_t n_pixels;
} dcscn_metrics;   /* 32 bytes */

/* Two single-channel float64 images [height, width] in host memory (synchronous; usable before dcscn_finalize). */
int dcscn_psnr_ssim(dcscn_handle h, const double* a, const double* b, int height, int width, int border_size, dcscn_metrics* out);

/* dcscn_evaluate_rgb with the metrics taken on the device from the images the pipeline already holds there: `model` = the
 * network output against the true Y (do_for_evaluate), `bicubic` (optional) = the bicubic of LR against the true Y
 * (evaluate_bicubic).  y (optional) receives the output like dcscn_evaluate_rgb's; when it is null no image is downloaded. */
int dcscn_evaluate_rgb_metrics(dcscn_handle h, const uint8_t* rgb, int height, int width, int n_ensemble, int border_size,
                               dcscn_metrics* model, dcscn_metrics* bicubic, double* y);

/* do_for_file's colour pipeline (sr.py; DCSCN.py:588-614): rgb uint8 [height, width, 3] is the input image,
 * rgb_upscaled uint8 [s*height, s*width, 3] its Pillow-upscaled copy (built by the caller, on the host or with
 * dcscn_resize_bicubic_bytes; dcscn_sr_rgb_bytes below builds it on the device itself).  Device: Y of the input
 * -> x, x2 = BICUBIC(x), do() -> y; CbCr of rgb_upscaled; rgb_out = convert_y_and_cbcr_to_rgb(y, cbcr), float64
 * [s*height, s*width, 3].  y (optional) receives the super-resolved luma, float64. */
int dcscn_sr_rgb(dcscn_handle h, const uint8_t* rgb, const uint8_t* rgb_upscaled, int height, int width, int n_ensemble,
                 double* y, double* rgb_out);

/* The same pipeline from ONE upload of the uint8 RGB input, every result as the bytes save_image would write (its cast is
 * numpy's astype(uint8): truncate toward zero to a 32-bit integer, keep the low 8 bits -- values outside 0..255 wrap).
 * Each output is optional (at least one non-null), uint8, of the upscaled size sh = s*height, sw = s*width:
 *   rgb_bicubic [sh, sw, 3]  resize_image_by_pil(rgb, s)                                      ("_bicubic")
 *   y_bicubic   [sh, sw]     cast(BICUBIC of float32(Y)) -- the x2 the forward consumes       ("_bicubic_y")
 *   y_out       [sh, sw]     cast(do(Y))                                                      ("_result_y")
 *   rgb_out     [sh, sw, 3]  cast(convert_y_and_cbcr_to_rgb(do(Y), CbCr of rgb_bicubic))      ("_result")
 * The network runs only when y_out or rgb_out is asked for. */
int dcscn_sr_rgb_bytes(dcscn_handle h, const uint8_t* rgb, int height, int width, int n_ensemble, uint8_t* rgb_bicubic,
                       uint8_t* y_bicubic, uint8_t* y_out, uint8_t* rgb_out);

/* Per-launch (dcscn_op_info order) device milliseconds, summed over sub-batches and averaged over
 * the forwards run with the profile option on since the previous call (which this call resets);
 * `ms` receives min(capacity, num_ops + 1) entries; entry num_ops is the float32 plan behind the split16 passes (the gated float32
 * launches, see "split16": microseconds unless an image left the f16 range).  Synchronises the device. */
int dcscn_get_profile(dcscn_handle h, double* ms, int capacity);

/* Debug aid (no reference counterpart): with dcscn_set_option("debug_digest", 1) every launch of a forward is followed by a
 * position-weighted checksum of the workspace tensor(s) it writes, and the pass ends with one of its output; `out` receives
 * min(capacity, num_ops + 1) values of the LAST pass.  Two runs of the same input must agree entry by entry -- the first entry
 * that differs names the launch whose result changed (tools/determinism_check.py).  "debug_poison" (1 LDS, 2 vector
 * registers, 3 both) fills those with NaN patterns in front of every launch: no kernel may depend on what they held. */
int dcscn_debug_digests(dcscn_handle h, uint64_t* out, int capacity);

/* Bytes of device workspace currently held. */
int64_t dcscn_workspace_bytes(dcscn_handle h);
/* How many workspace tensors the next forward keeps pre-split (option "p16"; 0 when the option, split16 or the graph rules it out).
 * The reference has no counterpart (sess.run hides its buffers); diagnostic for tests and benchmarks.  After dcscn_finalize. */
int dcscn_num_presplit_tensors(dcscn_handle h);

/* ---------------------------------------------------------------------------------------------------------------------
 * Training (DCSCN.py:334-425, 727-769): f32; the depthwise-separable nets behind option "train_separable" and the transposed-conv
 * upsampler (pixel_shuffler = 0) behind option "train_transposed" (both below); one device per handle, several handles (one per rank) train data-parallel through the record calls below.
 *
 * Forward in training mode = the inference graph run layer by layer in f32 (no tail fold, no Winograd, none of the inference split16
 * kernels; option "train_split16" moves the wide layers' forward and data-gradient convs to the f16 matrix pipe at f32 accuracy), with
 * dropout after the activator of every conv that has one (CNN1..L, A1, B1, B2, C, the non-final R-CNN layers; not the Up-PS
 * convs or Up-TCNN, not the last R-CNN): out = h / keep where the mask is 1, else 0.
 * Loss: diff = (R-CNN_last + x2) - y_true over the whole HR patch; mse = mean(diff^2); image_loss = mse, or mean(|diff|) with
 * use_l1_loss; loss = image_loss + l2_decay * sum over every conv_W (and Up-TCNN's Tconv_W) of 0.5 * ||W||^2 (biases and PReLU alphas not decayed).
 * Gradients of `loss` for every variable; clipping (clipping_norm > 0): g <- g * c / max(||g||_global, c) over all variables;
 * then TF's update rule:
 *   adam:     lr_t = lr * sqrt(1 - beta2_power) / (1 - beta1_power); m <- b1 m + (1 - b1) g; v <- b2 v + (1 - b2) g^2;
 *             w <- w - lr_t * m / (sqrt(v) + epsilon);  then beta1_power *= b1, beta2_power *= b2 (float32, start at b1, b2)
 *   gd:       w <- w - lr g
 *   momentum: a <- mu a + g; w <- w - lr a  (not Nesterov)
 * and, behind option "train_optimizers" (default 0, read by dcscn_train_begin alone: with 0 the three are refused as ever; no effect on
 * adam, gd or momentum), with the defaults TF 1.x gives the optimizers the reference constructs (DCSCN.py:383-392; the constants are
 * fixed, the layout of dcscn_train_config is unchanged), each line one float32 operation per operator, in this order:
 *   adagrad:  a = acc + g g; acc <- a; w <- w - lr g (1 / sqrt(a))                                    acc starts at 0.1
 *   adadelta: a = acc rho + g g (1 - rho); u = sqrt(upd + eps) (1 / sqrt(a + eps)) g; w <- w - u lr;
 *             upd <- upd rho + u u (1 - rho); acc <- a                        rho = 0.95, eps = 1e-8; acc, upd start at 0
 *   rmsprop:  s = ms + (g g - ms) (1 - decay); q = mom mu + (g lr) / sqrt(s + eps); w <- w - q; ms <- s; mom <- q
 *                                     decay = 0.9, eps = 1e-10, mu = the config's momentum, not centred; ms starts at 1, mom at 0
 * These three are written from knowledge of TF 1.x's ApplyAdagrad / ApplyAdadelta / ApplyRMSProp; they have not been run against TensorFlow.
 * Everything is deterministic: two identical sequences of calls give bit-identical variables and slots.
 *
 * Separable nets (depthwise_separable; option "train_separable", default 0, read by dcscn_train_begin: with 0 such a net is refused, the
 * option has no effect on a non-separable net and none after dcscn_train_begin).  A separable conv layer (tf.nn.separable_conv2d,
 * tf_graph.py:155-177) is d = depthwise k x k SAME (in; depthwise_W[k, k, cin, 1]), z = d . pointwise_W[1, 1, cin, cout] + conv_B, then the
 * activator and dropout as for a plain conv; the dropout layer number is still the layer's index in dcscn_layer_info order, one per
 * separable layer.  The extra reconstruction layers (R-CNN1 .. R-CNN(rl-1) with reconstruct_layers > 1) are plain convs even in a
 * separable net.  The trained variables are the handle's tensor list (depthwise_W, pointwise_W, conv_B, the PReLU slopes, conv_W of plain
 * layers), and the names follow from it: "<var>/depthwise_W/grad", "<var>/pointwise_W/Adam", ...  The l2 term covers conv_W of plain
 * layers only: the reference sums l2_loss over a list that holds, for a separable layer, the layer's UNUSED conv_W and never depthwise_W or
 * pointwise_W, so neither gets l2_decay * W in its gradient and neither enters the total loss.
 * Known departure: the library does not hold those unused conv_W tensors.  Missing are their l2 term in the reference's total loss
 * (stats[3]) and their l2_decay * |conv_W| in the global norm before clipping (stats[2]).  The gradients and updates of every variable the
 * library holds are the reference's, unless the clip is active and that term would move the norm.
 * Options "train_split16" / "train_split16_wgrad" leave separable layers on the f32 kernels; plain layers of a separable net keep their rule.
 *
 * Transposed-conv nets (pixel_shuffler = 0; option "train_transposed", default 0, read by dcscn_train_begin: with 0 such a net is refused,
 * the option has no effect on a pixel-shuffler net and none after dcscn_train_begin).  Layer Up-TCNN (build_transposed_conv,
 * tf_graph.py:219-236) takes the place of the Up-PS stages, one stage for any scale s: out = tf.nn.conv2d_transpose(in,
 * Tconv_W[k, k, out C, in C], stride s, SAME) with k = 2 s - s % 2 and C -> C channels, no bias, no activator and no dropout of its own.  It
 * runs as itself, k^2 C^2 multiply-adds per LR pixel in each of forward, data gradient and weight gradient, not as the derived 3x3 filter of
 * the inference plan.  Up-TCNN/Tconv_W is one more variable of the tensor list ("Up-TCNN/Tconv_W/grad", ".../Adam", ".../Adam_1",
 * ".../Momentum", the records of the data-parallel calls).  It IS in the l2 term (the reference appends it to its weight list,
 * tf_graph.py:235): l2_decay * W in its gradient, 0.5 ||W||^2 in the total loss.  A layer's dropout number stays its index in
 * dcscn_layer_info order, so Up-TCNN takes a number although it has no dropout: the layers behind it (R-CNN1 .. with reconstruct_layers > 1)
 * are numbered as dcscn_layer_info numbers them.  Options "train_split16" / "train_split16_wgrad" leave Up-TCNN on its f32 kernels; the other
 * layers of such a net take them as before.  A net that is also separable needs "train_separable" as well (Up-TCNN itself is never
 * separable).  After a step the inference plan's derived filter is rebuilt from the trained Tconv_W like every other packed filter.
 *
 * Ties.  At a pre-activation of exactly 0 the derivative of the activator is the one the reference's graph takes
 * (helper/tf_graph.py:82-96) under TensorFlow 1.x's registered gradients:
 *   prelu      = relu(z) + a (z - |z|) / 2   ReluGrad passes features > 0, Abs has the gradient sign(z) = 0       ->  a / 2
 *   leaky_relu = maximum(z, 0.1 z)           MaximumGrad sends x >= y to the first argument                      ->  1
 *   selu                                     SeluGrad: outputs < 0 ? g (outputs + scale alpha) : scale g         ->  1.0507009873554805
 *   relu                                     ReluGrad                                                             ->  0
 * and the gradient of a PReLU slope takes 0 from such an element.  The tie is an ordinary case: the reference initialises biases to
 * zero, and a black image region then gives pre-activations of exactly 0 in every layer.  This convention is derived from the
 * reference graph and those registrations; it has not been run against TensorFlow.
 *
 * Dropout mask (not stored; regenerated by the backward pass).  With splitmix64(z) = { z += 0x9E3779B97F4A7C15;
 * z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31); } on uint64:
 *   layer_key = splitmix64(dropout_key + 0x9E3779B97F4A7C15 * (layer + 1))   layer = index in dcscn_layer_info order
 *   idx       = ((n * H + y) * W + x) * C + c                                 the element's index in the layer's NHWC output
 *                                                                              (H, W at the layer's resolution, C = its filters)
 *   kept     <=> (splitmix64(layer_key ^ idx) >> 40) < floor(keep_prob * 2^24)
 * Reference values: splitmix64(0) = 0xE220A8397B1DCDAF; for dropout_key = 1, layer = 0: layer_key = 0xBEEB8DA1658EEC67 and
 * splitmix64(layer_key ^ 0) >> 40 = 0x778B1A, splitmix64(layer_key ^ 1) >> 40 = 0x3ED40B.
 * keep_prob = 1 turns dropout off.
 * A shard of a data-parallel step (dcscn_train_local_gradients_*, first_index = the index of the shard's first patch within the
 * global batch) counts n from first_index: idx = first_index * H * W * C + the shard-local idx above, H, W at the layer's
 * resolution.  The masks of a sharded batch are therefore the masks of the whole batch; first_index = 0 is the rule above.
 *
 * Variables, their gradients and the slots live on the device in flat f32 buffers, checkpoint (HWIO) layout.  Tensor names
 * (TF's, so checkpoints interoperate): "<var>", "<var>/grad" (gradient of the total loss BEFORE clipping, of the last step
 * or dcscn_train_gradients call), "<var>/Adam", "<var>/Adam_1", "<var>/Momentum", "beta1_power", "beta2_power"; with "train_optimizers"
 * "<var>/Adagrad" (acc), "<var>/Adadelta" (acc), "<var>/Adadelta_1" (upd), "<var>/RMSProp" (ms), "<var>/RMSProp_1" (mom).  A slot of
 * another optimizer than the running one is DCSCN_ERR_SHAPE; the beta powers exist under adam only.
 * The first forward (any dcscn_forward* / evaluate / sr call) after a step re-packs the inference plan from the device
 * variables (Training); forwards before any step are unchanged.
 * The training workspace is separate from the inference one, sized per batch shape and bounded by "workspace_budget_bytes":
 * a batch that does not fit returns DCSCN_ERR_NOMEM (training never tiles).
 * --------------------------------------------------------------------------------------------------------------------- */
typedef enum dcscn_optimizer {
    DCSCN_OPTIMIZER_ADAM = 0,
    DCSCN_OPTIMIZER_GD = 1,
    DCSCN_OPTIMIZER_MOMENTUM = 2,
    DCSCN_OPTIMIZER_ADADELTA = 3,   /* these three: option "train_optimizers"; without it refused, DCSCN_ERR_UNSUPPORTED */
    DCSCN_OPTIMIZER_ADAGRAD = 4,
    DCSCN_OPTIMIZER_RMSPROP = 5
} dcscn_optimizer;

/* Training flags of helper/args.py (optimizer, beta1, beta2, epsilon, momentum, l2_decay, clipping_norm, dropout_rate,
 * use_l1_loss). */
typedef struct dcscn_train_config {
    int32_t struct_size;            /* = sizeof(dcscn_train_config) */
    int32_t optimizer;              /* dcscn_optimizer */
    int32_t use_l1_loss;
    int32_t reserved0;
    double beta1, beta2, epsilon, momentum, l2_decay, clipping_norm;
    double keep_prob;               /* --dropout_rate: probability of KEEPING a unit, (0, 1] */
    int32_t reserved[8];
} dcscn_train_config;

/* build_optimizer: after dcscn_finalize; copies the variables to the device master copy and fills the slots with TF's initial values
 * (zeros, but 0.1 in "<var>/Adagrad" and 1 in "<var>/RMSProp").
 * Refused (DCSCN_ERR_UNSUPPORTED): depthwise_separable unless option "train_separable" was set to 1 before this call, pixel_shuffler = 0
 * unless option "train_transposed" was, adadelta / adagrad / rmsprop unless option "train_optimizers" was, batch_norm. */
int dcscn_train_begin(dcscn_handle h, const dcscn_train_config* tc);
/* One training step on host buffers (x [n, h, w], x2 and y_true [n, s*h, s*w]); synchronous.  stats (optional, 4 doubles):
 * image_loss, mse, global gradient norm before clipping, total loss (image_loss + the l2 term). */
int dcscn_train_step(dcscn_handle h, const float* x, const float* x2, const float* y_true, int n, int height, int width, double lr,
                     uint64_t dropout_key, double* stats);
/* The same on device buffers, enqueued on `stream` (NULL = the handle's); synchronises only when stats != NULL. */
int dcscn_train_step_device(dcscn_handle h, const float* x, const float* x2, const float* y_true, int n, int height, int width, double lr,
                            uint64_t dropout_key, double* stats, void* stream);
/* Forward and backward only (gradients readable as "<var>/grad"); no update, slots untouched.  Host buffers. */
int dcscn_train_gradients(dcscn_handle h, const float* x, const float* x2, const float* y_true, int n, int height, int width,
                          uint64_t dropout_key, double* stats);

/* Training batches built on the device from device-resident images (helper/loader.py DynamicDataSets.load_batch_image).
 * A patch is a crop of HR = lr_size * scale pixels per side at (top, left) of an image added with dcscn_train_add_image, mirrored
 * left-right when fliplr = 1.  Per patch, bit for bit what the host loader returns after the float32 cast of train_batch:
 *   RGB image:  y = Y of the crop (float64, color.hip's chain), x = Pillow mode-"F" bicubic of float32(y) to lr_size, x2 = mode "F"
 *               bicubic of x back to HR;  max_value != 255: y * (max_value / 255) in float64, x and x2 * float32(max_value / 255)
 *   grey image: y = the uint8 pixels, x and x2 = Pillow mode-"L" (8-bit fixed-point) bicubic;  max_value != 255: all three
 *               * (max_value / 255) in float64
 * then the float32 cast.  One batch may mix grey and RGB patches.  Bad input (an unknown image, a crop outside its image,
 * fliplr not 0 / 1, lr_size < 1, max_value <= 0) returns DCSCN_ERR_INVALID_ARG naming the patch; any of these calls before
 * dcscn_train_begin returns DCSCN_ERR_STATE. */
typedef struct dcscn_patch {
    int32_t image, top, left, fliplr;
} dcscn_patch;
/* Upload an image (uint8 [height, width, channels], channels 1 or 3) once; it stays on the device until the handle is destroyed.
 * *image_id receives its index for dcscn_patch.image (0, 1, 2, ... in call order). */
int dcscn_train_add_image(dcscn_handle h, const uint8_t* pixels, int height, int width, int channels, int32_t* image_id);
/* Build the batch of n patches into host buffers x [n, lr_size, lr_size], x2 and y_true [n, HR, HR]; synchronous. */
int dcscn_train_build_batch(dcscn_handle h, const dcscn_patch* patches, int n, int lr_size, double max_value, float* x, float* x2,
                            float* y_true);
/* Build the batch into the training workspace and take one step on it as dcscn_train_step does, on the handle's stream; no pixel
 * crosses PCIe.  Synchronises only when stats != NULL (the 4 doubles of dcscn_train_step). */
int dcscn_train_step_patches(dcscn_handle h, const dcscn_patch* patches, int n, int lr_size, double max_value, double lr,
                             uint64_t dropout_key, double* stats);
/* The 8-fold augmented dataset (augmentation.py: flipped and rotated copies of every image, files <stem><suffix><ext>) without
 * the copies: a patch names the variant of its image as an index map over the one uploaded image.  For a stored image in [H, W]
 * the variant out is [H, W] for codes 0 .. 3 and [W, H] for codes 4 .. 7 (numpy is the specification):
 *   code  suffix   numpy                      out[i, j]
 *   0     ""       m                          in[i, j]
 *   1     "_v"     flipud(m)                  in[H-1-i, j]
 *   2     "_h"     fliplr(m)                  in[i, W-1-j]
 *   3     "_hv"    flipud(fliplr(m))          in[H-1-i, W-1-j]
 *   4     "_r1"    rot90(m)                   in[j, W-1-i]
 *   5     "_r2"    rot90(m, -1)               in[H-1-j, i]
 *   6     "_r1_v"  flipud(rot90(m))           in[j, i]
 *   7     "_r2_v"  flipud(rot90(m, -1))       in[H-1-j, W-1-i]
 * augmentation.py --augment_level N writes codes 0 .. N-1.  top and left are coordinates in the VARIANT (so the crop must lie inside
 * [W, H] for codes 4 .. 7), and fliplr mirrors the crop afterwards, as the loader's random flip does:
 *   patch = fliplr?( variant(image)[top : top + HR, left : left + HR] )
 * and from there everything is dcscn_patch's pipeline, bit for bit what the host loader cuts from the file augmentation.py writes
 * (for a lossless format; a JPEG copy is re-encoded, the variant here is cut from the original decode).  The three calls have the
 * semantics of their namesakes, which are their transform = 0 case; a transform outside 0 .. 7 is DCSCN_ERR_INVALID_ARG. */
enum { DCSCN_AUG_NONE = 0, DCSCN_AUG_V = 1, DCSCN_AUG_H = 2, DCSCN_AUG_HV = 3, DCSCN_AUG_R1 = 4, DCSCN_AUG_R2 = 5, DCSCN_AUG_R1_V = 6,
       DCSCN_AUG_R2_V = 7, DCSCN_AUG_COUNT = 8 };
typedef struct dcscn_patch_aug {
    int32_t image, top, left, fliplr, transform;
} dcscn_patch_aug;
int dcscn_train_build_batch_aug(dcscn_handle h, const dcscn_patch_aug* patches, int n, int lr_size, double max_value, float* x, float* x2,
                                float* y_true);
int dcscn_train_step_patches_aug(dcscn_handle h, const dcscn_patch_aug* patches, int n, int lr_size, double max_value, double lr,
                                 uint64_t dropout_key, double* stats);
/* Data-parallel training: every rank holds a full replica (variables, slots, beta powers) on its own handle.  Per step each
 * rank computes the gradient of its shard of the global batch into a RECORD, the ranks exchange the records (any all-gather:
 * the library does not communicate), and every rank reduces all records in rank order and applies the same update -- the
 * replicas stay bit-identical without ever exchanging weights, and two runs give the same bits.
 * A record is dcscn_train_record_floats(h) float32 values in device memory, 16-byte aligned:
 *   [0, count)            the flat gradient of the shard's loss (local mean image loss + the l2 term, what dcscn_train_gradients
 *                         computes), variables in dcscn_tensor_info order, each in checkpoint layout
 *   [count, pad)          zeros, pad = count rounded up to a multiple of 4
 *   [pad, pad + 8)        4 doubles, bit for bit: image_loss, mse, n_local (the shard's patch count), total loss
 * dcscn_train_apply_records takes `world` records laid out [world][record_floats] and computes, on the device, with no atomics:
 *   w_r = n_r / sum n_r (double);  g[e] = (float) sum over r = 0 .. world-1, in that order, of w_r * (double) g_r[e]
 * (uneven shards give the exact mean over the global batch; the l2 term every rank added comes out once), the global norm of g
 * in the order dcscn_train_step sums it, the stats as the same weighted sums of the trailers (stats[2] = the norm of g), the
 * clip factor, and then the update rule above.  With world = 1 and first_index = 0 the two calls give dcscn_train_step's bits.
 * Both kinds of call enqueue on `stream` (NULL = the handle's) and do not synchronise, except apply_records with stats != NULL.
 * "<var>/grad" reads the shard's gradient after a local_gradients call and the reduced one after apply_records.
 * Refused: before dcscn_train_begin DCSCN_ERR_STATE; world < 1, first_index < 0, null or misaligned pointers, n < 1
 * DCSCN_ERR_INVALID_ARG.  Records of which one n_local is not > 0, or whose n_local sum to a non-finite value (so also a sum of
 * zero), leave variables, slots and powers untouched; the call reports that as DCSCN_ERR_INVALID_ARG when stats != NULL (without
 * stats it does not read the device back).  "<var>/grad" reads zeros after such a call, not the last local gradient. */
int64_t dcscn_train_record_floats(dcscn_handle h);
int dcscn_train_local_gradients_device(dcscn_handle h, const float* x, const float* x2, const float* y_true, int n, int height, int width,
                                       uint64_t dropout_key, int64_t first_index, float* record_out, void* stream);
/* The same with the shard built on the device from dcscn_patch descriptors, as dcscn_train_step_patches builds its batch. */
int dcscn_train_local_gradients_patches(dcscn_handle h, const dcscn_patch* patches, int n, int lr_size, double max_value,
                                        uint64_t dropout_key, int64_t first_index, float* record_out, void* stream);
/* The same from dcscn_patch_aug descriptors (above). */
int dcscn_train_local_gradients_patches_aug(dcscn_handle h, const dcscn_patch_aug* patches, int n, int lr_size, double max_value,
                                            uint64_t dropout_key, int64_t first_index, float* record_out, void* stream);
int dcscn_train_apply_records(dcscn_handle h, const float* records, int world, double lr, double* stats, void* stream);
/* Read a variable (any time after its dcscn_set_tensor; the trained value while training), a gradient or a slot: `count`
 * must equal its number of values. */
int dcscn_get_tensor(dcscn_handle h, const char* name, float* out, int64_t count);
/* Write a variable or a slot of a training handle (resume from a checkpoint). */
int dcscn_set_train_tensor(dcscn_handle h, const char* name, const float* data, int64_t count);

/* ---------------------------------------------------------------------------------------------------------------------
 * TensorBoard summaries (util.add_summaries, helper/utilty.py:427-443; log_to_tensorboard, DCSCN.py:427-479), reduced on the device.
 *
 * A record summarises `count` float32 values:
 *   num, nonfinite     the finite values, and the NaN / +Inf / -Inf ones: those are counted and left out of everything else
 *                      (TensorFlow's histogram op refuses them; the caller decides what to do with a tensor that has some)
 *   min, max           of the finite values
 *   sum, sum_squares   double sums of (double)v and (double)v * (double)v
 *   mean               sum / num                                    (tf.reduce_mean)
 *   stddev             sqrt(mean((v - mean)^2)), a second pass over the data in double with the first pass's mean   (utilty.py:430-436)
 *   buckets            DCSCN_SUMMARY_BUCKETS dense int64 counts: v is counted in bucket upper_bound(limits, (double)v), `limits` the
 *                      table of dcscn_summary_bucket_limits
 * num == 0 (no finite value, or count == 0 values in a view): min = max = sum = sum_squares = mean = stddev = 0.
 * The limit table is TensorFlow's default histogram table as its histogram.cc builds it: for (v = 1e-12; v < 1e20; v *= 1.1) in double gives
 * 774 positive limits p; limits = -DBL_MAX, -p reversed, 0.0, p, DBL_MAX.  It is built once on the host by exactly that loop and uploaded; the
 * device searches the uploaded table (a binary search in LDS), it never recomputes a limit.  The table is written from memory of
 * TensorFlow's source, not checked against it.
 * Determinism: the values are cut into a fixed number of contiguous chunks, a function of `count` alone; every double sum runs over one chunk
 * in a fixed order, and the chunks' sums are added in chunk order.  The counts use integer atomics, which commute exactly.  No floating-point
 * atomic anywhere: two calls give the same bits.  The data pointer needs float alignment only; count may be 1.
 * --------------------------------------------------------------------------------------------------------------------- */
#define DCSCN_SUMMARY_BUCKETS 1551
typedef struct dcscn_summary {
    int64_t num, nonfinite;
    double  min, max, sum, sum_squares, mean, stddev;
} dcscn_summary;   /* 64 bytes */

/* The bucket limits (host only, needs no device): writes min(capacity, DCSCN_SUMMARY_BUCKETS) doubles to `out` (may be NULL with
 * capacity 0) and returns DCSCN_SUMMARY_BUCKETS. */
int dcscn_summary_bucket_limits(double* out, int capacity);
/* The record of `count` >= 1 float32 values at the DEVICE pointer `data`, reduced on `stream` (a hipStream_t, NULL = the handle's);
 * `out` and `buckets` (optional; `capacity` >= DCSCN_SUMMARY_BUCKETS int64 values when given) are host memory, and the call returns
 * after the stream has finished.  Needs neither dcscn_finalize nor dcscn_train_begin. */
int dcscn_summarize_device(dcscn_handle h, const float* data, int64_t count, dcscn_summary* out, int64_t* buckets, int capacity,
                           void* stream);
/* What sess.run([summary_op, loss], {x, x2, y, dropout: 1.0, is_training: 0}) computes (DCSCN.py:446-471): forward and backward of the
 * batch in host buffers as dcscn_train_gradients runs them -- the same launches, so whatever kernels the current "train_split16" options
 * give a step -- but with dropout OFF whatever keep_prob the handle trains with; no update: variables, slots and beta powers are untouched.
 * Then every summarised tensor is reduced on the handle's stream and the call synchronises once.  stats (optional): the 4 doubles of
 * dcscn_train_step.  Afterwards, until the next gradient computation of any kind on the handle,
 *   "<var>/grad"        reads THIS pass's gradients (dropout off), not the last step's;
 *   dcscn_summary_get   returns the record of: every variable "<var>" and every "<var>/grad"; "<layer>/output" for each layer of
 *                       dcscn_layer_info, the tensor the reference appends to self.H for it: the activator's output where the layer
 *                       has one, else the conv's (for an Up-PS conv that is before depth_to_space), for Up-TCNN the transposed conv's;
 *                       "x", the input; "y_", the last layer + x2;
 *   dcscn_get_tensor    also reads "<layer>/output" (NHWC at the layer's resolution, n * H r * W r * out_channels values), "x" and "y_".
 * The summaries stay readable after later steps; the three kinds of activations do not (DCSCN_ERR_STATE).
 * The backward pass overwrites no activation (every layer keeps its own pre-activation and output in the training arena), so all
 * records are taken behind it.  DCSCN_ERR_STATE before dcscn_train_begin; DCSCN_ERR_NOMEM as for a step (training never tiles). */
int dcscn_train_log_pass(dcscn_handle h, const float* x, const float* x2, const float* y_true, int n, int height, int width, double* stats);
/* The record `name` of the last dcscn_train_log_pass; buckets optional as above.  Before any log pass DCSCN_ERR_STATE; an unknown
 * name DCSCN_ERR_SHAPE. */
int dcscn_summary_get(dcscn_handle h, const char* name, dcscn_summary* out, int64_t* buckets, int capacity);

const char* dcscn_last_error(dcscn_handle h);
int dcscn_destroy(dcscn_handle h);

#ifdef __cplusplus
}
#endif
#endif /* DCSCN_H_ */
