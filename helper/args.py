"""Flag surface of the reference (helper/args.py:13-107): same names, types and defaults, hosted on
the absl-like registry of ``dcscn-super-resolution_amd/flags.py`` instead of ``tf.app.flags``.

Usage is unchanged:  ``from helper import args``; ``args.flags.DEFINE_string(...)``;
``FLAGS = args.get()``; and ``args.run(main)`` where the reference calls ``tf.app.run()``.
The training flags drive train.py (SuperResolution.build_optimizer / train_batch on the engine's training plan).
"""

import sys

import numpy as np

import dcscn_amd
from dcscn_amd import flags as flags          # noqa: F401  (the reference exposes args.flags)

FLAGS = flags.FLAGS
run = flags.run

_I, _F, _B, _S = flags.DEFINE_integer, flags.DEFINE_float, flags.DEFINE_boolean, flags.DEFINE_string

_TABLE = [
    # ---- model (args.py:17-36)
    (_I, "scale", 2, "super-resolution factor: 2, 3 or 4"),
    (_I, "layers", 12, "feature-extraction conv layers"),
    (_I, "filters", 196, "filters of the first feature layer"),
    (_I, "min_filters", 48, "filters of the last feature layer"),
    (_F, "filters_decay_gamma", 1.5, "decay exponent of the filter count from filters to min_filters"),
    (_B, "use_nin", True, "network-in-network reconstruction (A1 / B1 / B2)"),
    (_I, "nin_filters", 64, "filters of A1"),
    (_I, "nin_filters2", 32, "filters of B1 and B2"),
    (_I, "cnn_size", 3, "conv kernel size"),
    (_I, "reconstruct_layers", 1, "reconstruction conv layers (0 behaves as 1)"),
    (_I, "reconstruct_filters", 32, "filters of the extra reconstruction layers"),
    (_F, "dropout_rate", 0.8, "keep probability while training; inference always keeps everything"),
    (_S, "activator", "prelu", "relu, leaky_relu, prelu, sigmoid, tanh or selu"),
    (_B, "pixel_shuffler", True, "pixel-shuffler upsampling; false = transposed-conv upsampler (Up-TCNN, tf_graph.py:219-236)"),
    (_I, "pixel_shuffler_filters", 0, "pixel-shuffler output channels, 0 = as many as its input"),
    (_I, "self_ensemble", 8, "flipped / rotated copies averaged per image, 1 to 8"),
    (_B, "batch_norm", False, "batch normalisation (not implemented)"),
    (_B, "depthwise_separable", False, "depthwise-separable convs in place of every conv"),
    # ---- training (args.py:39-59)
    (_B, "bicubic_init", True, "unused (the reference defines it but never reads it)"),
    (_F, "clipping_norm", 5, "clip the gradients by their global norm to this value; 0 = no clipping"),
    (_S, "initializer", "he", "weight initialiser used before a checkpoint is loaded: he, xavier, uniform, stddev, identity (any other name: zeros)"),
    (_F, "weight_dev", 0.01, "stddev of the initialiser when --initializer is stddev; half the range when it is uniform"),
    (_F, "l2_decay", 0.0001, "weight of the l2 loss of the conv filters"),
    (_S, "optimizer", "adam", "adam, momentum, gd, adadelta, adagrad or rmsprop (the last three with TF 1.x's default constants; rmsprop takes --momentum)"),
    (_F, "beta1", 0.9, "beta1 of adam"),
    (_F, "beta2", 0.999, "beta2 of adam"),
    (_F, "epsilon", 1e-8, "epsilon of adam (TF placement: added to sqrt(v))"),
    (_F, "momentum", 0.9, "momentum of the momentum and rmsprop optimizers"),
    (_I, "batch_num", 20, "patches per training step"),
    (_I, "batch_image_size", 48, "LR size of a training patch"),
    (_I, "stride_size", 0, "patch stride of --build_batch (not supported)"),
    (_I, "training_images", 24000, "patches per training epoch"),
    (_B, "use_l1_loss", False, "train on mean |diff| instead of the mse"),
    (_F, "initial_lr", 0.002, "initial learning rate"),
    (_F, "lr_decay", 0.5, "learning rate factor every lr_decay_epoch epochs"),
    (_I, "lr_decay_epoch", 9, "epochs between learning rate decays"),
    (_F, "end_lr", 2e-5, "training stops when the learning rate falls to this"),
    # ---- datasets (args.py:62-65)
    (_S, "dataset", "bsd200", "training image directory under data_dir"),
    (_S, "test_dataset", "set5", "directory under data_dir to evaluate: set5, set14, bsd100, ... or all"),
    (_I, "tests", 1, "number of trained models (trials) to evaluate"),
    (_B, "do_benchmark", False, "after training, also evaluate set5, set14 and bsd100"),
    # ---- image processing (args.py:68-74)
    (_F, "max_value", 255, "pixel value range the network works in"),
    (_I, "channels", 1, "image channels fed to the network; only 1 (Y of YCbCr) is supported"),
    (_I, "psnr_calc_border_size", -1, "border shaved before PSNR; negative means the scale factor"),
    (_B, "build_batch", False, "pre-cut training patches (BatchDataSets): not supported"),
    # ---- environment (args.py:77-85)
    (_S, "checkpoint_dir", "models", "directory of the TF checkpoints"),
    (_S, "graph_dir", "graphs", "unused"),
    (_S, "data_dir", "data", "directory of the image datasets"),
    (_S, "batch_dir", "batch_data", "directory of --build_batch patches (not supported)"),
    (_S, "output_dir", "output", "directory result images are written to"),
    (_S, "tf_log_dir", "tf_log", "Directory for tensorboard log (written with --tensorboard)"),
    (_S, "log_filename", "log.txt", "log file"),
    (_S, "model_name", "", "explicit model name instead of the one derived from the flags"),
    (_S, "load_model_name", "", "checkpoint to load: a file stem or 'default'"),
    # ---- logging / device (args.py:88-94)
    (_B, "initialize_tf_log", True, "Clear all tensorboard log before start (with --tensorboard)"),
    (_B, "enable_log", True, "Enables tensorboard-log. Save loss. (with --tensorboard)"),
    (_B, "save_weights", True, "Save weights and biases/gradients (with --tensorboard)"),
    (_B, "save_images", False, "unused"),
    (_I, "save_images_num", 20, "unused"),
    (_B, "save_meta_data", False, "unused"),
    (_I, "gpu_device_id", 0, "HIP device the engine runs on"),
    # ---- extension (not a reference flag): PSNR / SSIM of evaluated images on the device instead of numpy / scipy
    (_B, "device_metrics", False, "compute the PSNR and SSIM of evaluated images on the device"),
    # ---- extension (not a reference flag): inference with ONE f16 product per multiply-accumulate (engine option "fast16", include/dcscn.h)
    (_B, "fast16", False, "inference at f16 operand accuracy: one matrix product per MAC instead of three (training is unaffected)"),
    # ---- extension (not a reference flag): the same inside the narrow nets' streamed feature extractor (engine option "fast16_stream", include/dcscn.h)
    (_B, "fast16_stream", False, "inference with one f16 product per MAC inside the streamed feature extractor of the narrow nets (c-DCSCN); independent of --fast16"),
    # ---- extension (not a reference flag): the same inside the separable narrow nets' streamed kernels (engine option "fast16_separable", include/dcscn.h)
    (_B, "fast16_separable", False, "inference with one f16 product per MAC inside the streamed kernels of the depthwise-separable narrow nets (feat_stream, tail_stream); independent of --fast16 and --fast16_stream"),
    # ---- extension (not a reference flag): training's wide forward / data-gradient convs on the f16 matrix pipe (engine option "train_split16", include/dcscn.h)
    (_B, "train_split16", False, "training at f32 accuracy with the forward and data-gradient convs of layers with min(cin, cout) >= 16 as three scaled f16 products"),
    # ---- extension (not a reference flag): the weight gradients of the same layers on the f16 matrix pipe (engine option "train_split16_wgrad", include/dcscn.h)
    (_B, "train_split16_wgrad", False, "training at f32 accuracy with the weight gradients of layers with min(cin, cout) >= 16 as three scaled f16 products"),
    # ---- extension (not a reference flag): write the reference's TensorBoard log under <tf_log_dir>/train, summaries reduced on the device (dcscn_train_log_pass, include/dcscn.h)
    (_B, "tensorboard", False, "write the TensorBoard event file of the reference's training log once per epoch (needs enable_log)"),
    # ---- extension (not a reference flag): train on the copies augmentation.py --augment_level N would write of --dataset, cut from the one uploaded
    # image per file (dcscn_patch_aug, include/dcscn.h).  Not "augment_level": augmentation.py defines that flag itself, with another default
    (_I, "train_augment_level", 0, "train on the flipped / rotated copies augmentation.py --augment_level N would write, without writing them: 0 .. 8 (0 and 1: the images as they are)"),
    # ---- frozen graphs (args.py:97-98): weights from the Const nodes of a frozen GraphDef (dcscn-super-resolution_amd/frozen.py)
    (_B, "frozenInference", False, "Flag for whether the model to evaluate is frozen."),
    (_S, "frozen_graph_path", "./model_to_freeze/frozen_model_optimized.pb", "the path to a frozen model if performing inference from it"),
]
for _define, _name, _default, _help in _TABLE:
    _define(_name, _default, _help)


def get():
    print("Python Interpreter version:%s" % sys.version[:3])
    print("dcscn_amd engine: %s" % dcscn_amd.engine.library_path())
    print("numpy version:%s" % np.__version__)
    return FLAGS
