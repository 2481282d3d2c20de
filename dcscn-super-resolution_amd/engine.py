"""ctypes binding of libdcscn_hip.so (include/dcscn.h): the device side of ``sess.run(self.y_, ...)``.

There is deliberately no fallback: if the shared library is missing or no gfx950 device is usable,
constructing an :class:`Engine` raises :class:`EngineError`.
"""

import ctypes
import os

import numpy as np

from . import build as _build

ABI_VERSION = 4
MAX_NAME = 128

ACTIVATORS = {None: 0, "": 0, "none": 0, "prelu": 1, "relu": 2, "leaky_relu": 3, "sigmoid": 4, "tanh": 5, "selu": 6}

STATUS_NAMES = {0: "OK", 1: "INVALID_ARG", 2: "UNSUPPORTED", 3: "MISSING_TENSOR", 4: "SHAPE", 5: "HIP", 6: "STATE",
                7: "NOMEM"}

# every symbol include/dcscn.h declares (tests check the library exports exactly these)
EXPORTED_SYMBOLS = (
    "dcscn_abi_version", "dcscn_last_global_error", "dcscn_device_count", "dcscn_filter_schedule", "dcscn_create",
    "dcscn_num_tensors", "dcscn_tensor_info", "dcscn_set_tensor", "dcscn_finalize", "dcscn_num_layers",
    "dcscn_layer_info_get", "dcscn_num_ops", "dcscn_op_info_get", "dcscn_set_option", "dcscn_forward",
    "dcscn_forward_device", "dcscn_forward_ensemble", "dcscn_get_profile", "dcscn_debug_digests", "dcscn_workspace_bytes", "dcscn_num_presplit_tensors",
    "dcscn_last_error", "dcscn_destroy", "dcscn_resize_bicubic", "dcscn_resize_bicubic_device", "dcscn_forward_lr",
    "dcscn_resample_table", "dcscn_get_stream", "dcscn_synchronize", "dcscn_convert_rgb_to_y", "dcscn_convert_rgb_to_ycbcr",
    "dcscn_convert_y_and_cbcr_to_rgb", "dcscn_evaluate_rgb", "dcscn_sr_rgb",
    "dcscn_train_begin", "dcscn_train_step", "dcscn_train_step_device", "dcscn_train_gradients", "dcscn_get_tensor",
    "dcscn_set_train_tensor", "dcscn_train_add_image", "dcscn_train_build_batch", "dcscn_train_step_patches",
    "dcscn_psnr_ssim", "dcscn_evaluate_rgb_metrics",
    "dcscn_train_record_floats", "dcscn_train_local_gradients_device", "dcscn_train_local_gradients_patches",
    "dcscn_train_apply_records",
    "dcscn_train_build_batch_aug", "dcscn_train_step_patches_aug", "dcscn_train_local_gradients_patches_aug",
    "dcscn_resample_table_bytes", "dcscn_resize_bicubic_bytes", "dcscn_resize_bicubic_bytes_device", "dcscn_sr_rgb_bytes",
    "dcscn_summary_bucket_limits", "dcscn_summarize_device", "dcscn_train_log_pass", "dcscn_summary_get",
)

SUMMARY_BUCKETS = 1551

# dcscn_optimizer; the names of helper/args.py --optimizer (the last three train behind option "train_optimizers")
OPTIMIZERS = {"adam": 0, "gd": 1, "momentum": 2, "adadelta": 3, "adagrad": 4, "rmsprop": 5}
MORE_OPTIMIZERS = ("adadelta", "adagrad", "rmsprop")


class EngineError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("dcscn: %s (%s)" % (message, STATUS_NAMES.get(status, status)))
        self.status = status
        self.message = message


class Config(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_int32),
        ("scale", ctypes.c_int32),
        ("layers", ctypes.c_int32),
        ("filters", ctypes.c_int32),
        ("min_filters", ctypes.c_int32),
        ("filters_decay_gamma", ctypes.c_double),
        ("cnn_size", ctypes.c_int32),
        ("use_nin", ctypes.c_int32),
        ("nin_filters", ctypes.c_int32),
        ("nin_filters2", ctypes.c_int32),
        ("reconstruct_layers", ctypes.c_int32),
        ("reconstruct_filters", ctypes.c_int32),
        ("activator", ctypes.c_int32),
        ("pixel_shuffler", ctypes.c_int32),
        ("pixel_shuffler_filters", ctypes.c_int32),
        ("depthwise_separable", ctypes.c_int32),
        ("channels", ctypes.c_int32),
        ("legacy_no_c", ctypes.c_int32),
        ("batch_norm", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 8),
    ]


class TrainConfig(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_int32),
        ("optimizer", ctypes.c_int32),
        ("use_l1_loss", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
        ("beta1", ctypes.c_double),
        ("beta2", ctypes.c_double),
        ("epsilon", ctypes.c_double),
        ("momentum", ctypes.c_double),
        ("l2_decay", ctypes.c_double),
        ("clipping_norm", ctypes.c_double),
        ("keep_prob", ctypes.c_double),
        ("reserved", ctypes.c_int32 * 8),
    ]


class LayerInfo(ctypes.Structure):
    _fields_ = [
        ("name", ctypes.c_char * MAX_NAME),
        ("kernel_size", ctypes.c_int32),
        ("in_channels", ctypes.c_int32),
        ("out_channels", ctypes.c_int32),
        ("depthwise_separable", ctypes.c_int32),
        ("has_bias", ctypes.c_int32),
        ("activator", ctypes.c_int32),
        ("resolution", ctypes.c_int32),
        ("macs_per_lr_pixel", ctypes.c_int64),
    ]


class OpInfo(ctypes.Structure):
    _fields_ = [
        ("name", ctypes.c_char * MAX_NAME),
        ("kernel", ctypes.c_char * 32),
        ("kernel_size", ctypes.c_int32),
        ("in_channels", ctypes.c_int32),
        ("out_channels", ctypes.c_int32),
        ("resolution", ctypes.c_int32),
        ("mt", ctypes.c_int32),
        ("nt", ctypes.c_int32),
        ("kc", ctypes.c_int32),
        ("n_tiles", ctypes.c_int32),
        ("macs_per_lr_pixel", ctypes.c_int64),
        ("bytes_per_lr_pixel", ctypes.c_int64),
        ("executed_macs_per_lr_pixel", ctypes.c_int64),
    ]


class Metrics(ctypes.Structure):
    """dcscn_metrics: PSNR / SSIM of one image pair and the exact integers the PSNR is formed from."""
    _fields_ = [
        ("psnr", ctypes.c_double),
        ("ssim", ctypes.c_double),
        ("sq_err_sum", ctypes.c_int64),
        ("n_pixels", ctypes.c_int64),
    ]


class Summary(ctypes.Structure):
    """dcscn_summary: the record of one summarised tensor ("TensorBoard summaries" in include/dcscn.h)."""
    _fields_ = [
        ("num", ctypes.c_int64),
        ("nonfinite", ctypes.c_int64),
        ("min", ctypes.c_double),
        ("max", ctypes.c_double),
        ("sum", ctypes.c_double),
        ("sum_squares", ctypes.c_double),
        ("mean", ctypes.c_double),
        ("stddev", ctypes.c_double),
    ]

    def as_dict(self, buckets=None):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        if buckets is not None:
            d["buckets"] = buckets
        return d


_lib = None


def library_path():
    return _build.LIB_PATH


def load_library():
    """dlopen libdcscn_hip.so (built in-tree by build.py / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.isfile(path):
        raise EngineError(5, "HIP extension %s is missing; run `python __graft_entry__.py` (or "
                             "dcscn-super-resolution_amd/build.py) to compile it with hipcc" % path)
    try:
        lib = ctypes.CDLL(path)
    except OSError as exc:
        raise EngineError(5, "cannot load %s: %s" % (path, exc))
    c = ctypes
    fp, dp, vp = c.POINTER(c.c_float), c.POINTER(c.c_double), c.c_void_p
    lib.dcscn_abi_version.restype = c.c_int
    lib.dcscn_last_global_error.restype = c.c_char_p
    lib.dcscn_device_count.restype = c.c_int
    lib.dcscn_filter_schedule.argtypes = [c.c_int, c.c_int, c.c_int, c.c_double, c.POINTER(c.c_int32)]
    lib.dcscn_create.argtypes = [c.POINTER(Config), c.c_int, c.POINTER(vp)]
    lib.dcscn_num_tensors.argtypes = [vp]
    lib.dcscn_tensor_info.argtypes = [vp, c.c_int, c.c_char_p, c.c_int, c.POINTER(c.c_int64), c.POINTER(c.c_int)]
    lib.dcscn_set_tensor.argtypes = [vp, c.c_char_p, fp, c.POINTER(c.c_int64), c.c_int]
    lib.dcscn_finalize.argtypes = [vp]
    lib.dcscn_num_layers.argtypes = [vp]
    lib.dcscn_layer_info_get.argtypes = [vp, c.c_int, c.POINTER(LayerInfo)]
    lib.dcscn_num_ops.argtypes = [vp]
    lib.dcscn_op_info_get.argtypes = [vp, c.c_int, c.POINTER(OpInfo)]
    lib.dcscn_set_option.argtypes = [vp, c.c_char_p, c.c_int64]
    lib.dcscn_forward.argtypes = [vp, fp, fp, fp, c.c_int, c.c_int, c.c_int]
    lib.dcscn_forward_device.argtypes = [vp, vp, vp, vp, c.c_int, c.c_int, c.c_int, vp]
    lib.dcscn_forward_ensemble.argtypes = [vp, fp, fp, dp, c.c_int, c.c_int, c.c_int]
    lib.dcscn_resize_bicubic.argtypes = [vp, fp, fp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int]
    lib.dcscn_resize_bicubic_device.argtypes = [vp, vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp]
    lib.dcscn_forward_lr.argtypes = [vp, fp, fp, c.c_int, c.c_int, c.c_int]
    lib.dcscn_resample_table.argtypes = [c.c_int, c.c_int, c.POINTER(c.c_int), c.POINTER(c.c_int), dp, c.c_int]
    lib.dcscn_get_profile.argtypes = [vp, dp, c.c_int]
    lib.dcscn_debug_digests.argtypes = [vp, c.POINTER(c.c_uint64), c.c_int]
    lib.dcscn_workspace_bytes.argtypes = [vp]
    lib.dcscn_num_presplit_tensors.argtypes = [vp]
    lib.dcscn_get_stream.argtypes = [vp, c.POINTER(vp)]
    u8p = c.POINTER(c.c_uint8)
    lib.dcscn_convert_rgb_to_y.argtypes = [vp, u8p, dp, c.c_int64]
    lib.dcscn_convert_rgb_to_ycbcr.argtypes = [vp, u8p, dp, c.c_int64]
    lib.dcscn_convert_y_and_cbcr_to_rgb.argtypes = [vp, dp, dp, dp, c.c_int64]
    lib.dcscn_evaluate_rgb.argtypes = [vp, u8p, c.c_int, c.c_int, c.c_int, dp, fp, dp]
    lib.dcscn_sr_rgb.argtypes = [vp, u8p, u8p, c.c_int, c.c_int, c.c_int, dp, dp]
    lib.dcscn_resample_table_bytes.argtypes = [c.c_int, c.c_int, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_int32), c.c_int]
    lib.dcscn_resize_bicubic_bytes.argtypes = [vp, u8p, u8p, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int]
    lib.dcscn_resize_bicubic_bytes_device.argtypes = [vp, vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp]
    lib.dcscn_sr_rgb_bytes.argtypes = [vp, u8p, c.c_int, c.c_int, c.c_int, u8p, u8p, u8p, u8p]
    lib.dcscn_psnr_ssim.argtypes = [vp, dp, dp, c.c_int, c.c_int, c.c_int, c.POINTER(Metrics)]
    lib.dcscn_evaluate_rgb_metrics.argtypes = [vp, u8p, c.c_int, c.c_int, c.c_int, c.c_int, c.POINTER(Metrics), c.POINTER(Metrics), dp]
    lib.dcscn_synchronize.argtypes = [vp]
    lib.dcscn_workspace_bytes.restype = c.c_int64
    lib.dcscn_last_error.argtypes = [vp]
    lib.dcscn_last_error.restype = c.c_char_p
    lib.dcscn_destroy.argtypes = [vp]
    lib.dcscn_train_begin.argtypes = [vp, c.POINTER(TrainConfig)]
    lib.dcscn_train_step.argtypes = [vp, fp, fp, fp, c.c_int, c.c_int, c.c_int, c.c_double, c.c_uint64, dp]
    lib.dcscn_train_step_device.argtypes = [vp, vp, vp, vp, c.c_int, c.c_int, c.c_int, c.c_double, c.c_uint64, dp, vp]
    lib.dcscn_train_gradients.argtypes = [vp, fp, fp, fp, c.c_int, c.c_int, c.c_int, c.c_uint64, dp]
    lib.dcscn_get_tensor.argtypes = [vp, c.c_char_p, fp, c.c_int64]
    lib.dcscn_set_train_tensor.argtypes = [vp, c.c_char_p, fp, c.c_int64]
    lib.dcscn_train_add_image.argtypes = [vp, u8p, c.c_int, c.c_int, c.c_int, c.POINTER(c.c_int32)]
    lib.dcscn_train_build_batch.argtypes = [vp, vp, c.c_int, c.c_int, c.c_double, fp, fp, fp]
    lib.dcscn_train_step_patches.argtypes = [vp, vp, c.c_int, c.c_int, c.c_double, c.c_double, c.c_uint64, dp]
    lib.dcscn_train_record_floats.argtypes = [vp]
    lib.dcscn_train_record_floats.restype = c.c_int64
    lib.dcscn_train_local_gradients_device.argtypes = [vp, vp, vp, vp, c.c_int, c.c_int, c.c_int, c.c_uint64, c.c_int64, vp, vp]
    lib.dcscn_train_local_gradients_patches.argtypes = [vp, vp, c.c_int, c.c_int, c.c_double, c.c_uint64, c.c_int64, vp, vp]
    lib.dcscn_train_apply_records.argtypes = [vp, vp, c.c_int, c.c_double, dp, vp]
    # the dcscn_patch_aug twins take their namesakes' arguments (an older build of the library, timed through
    # tools/train_bench.py --library, has none of them: calling one there raises AttributeError)
    for name in ("dcscn_train_build_batch", "dcscn_train_step_patches", "dcscn_train_local_gradients_patches"):
        if hasattr(lib, name + "_aug"):
            getattr(lib, name + "_aug").argtypes = getattr(lib, name).argtypes
    i64p = c.POINTER(c.c_int64)
    lib.dcscn_summary_bucket_limits.argtypes = [dp, c.c_int]
    lib.dcscn_summarize_device.argtypes = [vp, vp, c.c_int64, c.POINTER(Summary), i64p, c.c_int, vp]
    lib.dcscn_train_log_pass.argtypes = [vp, fp, fp, fp, c.c_int, c.c_int, c.c_int, dp]
    lib.dcscn_summary_get.argtypes = [vp, c.c_char_p, c.POINTER(Summary), i64p, c.c_int]
    if lib.dcscn_abi_version() != ABI_VERSION:
        raise EngineError(5, "ABI mismatch: library %d, binding %d" % (lib.dcscn_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def filter_schedule(layers, filters, min_filters, gamma):
    lib = load_library()
    out = (ctypes.c_int32 * layers)()
    rc = lib.dcscn_filter_schedule(layers, filters, min_filters, gamma, out)
    if rc:
        raise EngineError(rc, lib.dcscn_last_global_error().decode())
    return list(out)


def device_count():
    return load_library().dcscn_device_count()


def make_config(cfg):
    """Translate a flags-style dict / object (names of helper/args.py) into the C struct."""
    get = cfg.get if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))
    c = Config()
    c.struct_size = ctypes.sizeof(Config)
    c.scale = int(get("scale", 2))
    c.layers = int(get("layers", 12))
    c.filters = int(get("filters", 196))
    c.min_filters = int(get("min_filters", 48))
    c.filters_decay_gamma = float(get("filters_decay_gamma", 1.5))
    c.cnn_size = int(get("cnn_size", 3))
    c.use_nin = int(bool(get("use_nin", True)))
    c.nin_filters = int(get("nin_filters", 64))
    c.nin_filters2 = int(get("nin_filters2", 32))
    c.reconstruct_layers = int(get("reconstruct_layers", 1))
    c.reconstruct_filters = int(get("reconstruct_filters", 32))
    act = get("activator", "prelu")
    if act not in ACTIVATORS:
        raise NameError("Not implemented activator:%s" % act)      # tf_graph.py:98
    c.activator = ACTIVATORS[act]
    c.pixel_shuffler = int(bool(get("pixel_shuffler", True)))
    c.pixel_shuffler_filters = int(get("pixel_shuffler_filters", 0))
    c.depthwise_separable = int(bool(get("depthwise_separable", False)))
    c.channels = int(get("channels", 1))
    c.legacy_no_c = int(bool(get("legacy_no_c", False)))
    c.batch_norm = int(bool(get("batch_norm", False)))
    return c


def make_train_config(flags):
    """Translate the training flags of helper/args.py (dict or object) into the C struct."""
    get = flags.get if isinstance(flags, dict) else (lambda k, d=None: getattr(flags, k, d))
    opt = get("optimizer", "adam")
    if opt not in OPTIMIZERS:
        raise EngineError(1, "unknown optimizer '%s'" % opt)
    c = TrainConfig()
    c.struct_size = ctypes.sizeof(TrainConfig)
    c.optimizer = OPTIMIZERS[opt]
    c.use_l1_loss = int(bool(get("use_l1_loss", False)))
    c.beta1 = float(get("beta1", 0.9))
    c.beta2 = float(get("beta2", 0.999))
    c.epsilon = float(get("epsilon", 1e-8))
    c.momentum = float(get("momentum", 0.9))
    c.l2_decay = float(get("l2_decay", 0.0001))
    c.clipping_norm = float(get("clipping_norm", 5))
    c.keep_prob = float(get("dropout_rate", 0.8))
    return c


def summary_bucket_limits():
    """The SUMMARY_BUCKETS float64 limits of the summary histograms (dcscn_summary_bucket_limits: TensorFlow's default table, built
    on the host by the library); needs no GPU."""
    lib = load_library()
    out = np.zeros(SUMMARY_BUCKETS, np.float64)
    n = lib.dcscn_summary_bucket_limits(out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out.size)
    if n != SUMMARY_BUCKETS:
        raise EngineError(5, "the library has %d summary buckets, the binding %d" % (n, SUMMARY_BUCKETS))
    return out


def resample_table(in_size, out_size):
    """(bounds [out, 2] int32, weights [out, ksize] float64) of the Pillow-compatible bicubic resize along one
    axis (dcscn_resample_table); host code of the library, needs no GPU."""
    lib = load_library()
    ks = ctypes.c_int(0)
    rc = lib.dcscn_resample_table(int(in_size), int(out_size), ctypes.byref(ks), None, None, 0)
    if rc:
        raise EngineError(rc, "dcscn_resample_table(%d, %d)" % (in_size, out_size))
    bounds = np.zeros((int(out_size), 2), np.int32)
    weights = np.zeros((int(out_size), ks.value), np.float64)
    rc = lib.dcscn_resample_table(int(in_size), int(out_size), ctypes.byref(ks),
                                  bounds.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                  weights.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), weights.size)
    if rc:
        raise EngineError(rc, "dcscn_resample_table(%d, %d)" % (in_size, out_size))
    return bounds, weights


def resample_table_bytes(in_size, out_size):
    """(bounds [out, 2] int32, coeffs [out, ksize] int32) of the Pillow-compatible 8-bit bicubic resize along one axis: the
    weights of resample_table with 22 fraction bits (dcscn_resample_table_bytes); host code of the library, needs no GPU."""
    lib = load_library()
    ks = ctypes.c_int(0)
    rc = lib.dcscn_resample_table_bytes(int(in_size), int(out_size), ctypes.byref(ks), None, None, 0)
    if rc:
        raise EngineError(rc, "dcscn_resample_table_bytes(%d, %d)" % (in_size, out_size))
    bounds = np.zeros((int(out_size), 2), np.int32)
    coeffs = np.zeros((int(out_size), ks.value), np.int32)
    rc = lib.dcscn_resample_table_bytes(int(in_size), int(out_size), ctypes.byref(ks),
                                        bounds.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                        coeffs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), coeffs.size)
    if rc:
        raise EngineError(rc, "dcscn_resample_table_bytes(%d, %d)" % (in_size, out_size))
    return bounds, coeffs


class Engine:
    """One DCSCN graph resident on one MI355X (``dcscn_handle``)."""

    def __init__(self, cfg, device=0):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        self.scale = int(cfg.get("scale", 2) if isinstance(cfg, dict) else getattr(cfg, "scale", 2))
        c = make_config(cfg)
        rc = self._lib.dcscn_create(ctypes.byref(c), int(device), ctypes.byref(self._h))
        if rc:
            self._h = ctypes.c_void_p()
            raise EngineError(rc, self._lib.dcscn_last_global_error().decode())
        self.device = int(device)
        self.finalized = False

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.dcscn_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc:
            raise EngineError(rc, self._lib.dcscn_last_error(self._h).decode())

    # -- graph description -------------------------------------------------------------------
    def tensor_specs(self):
        """[(checkpoint variable name, shape)] the graph expects."""
        out = []
        name = ctypes.create_string_buffer(256)
        shape = (ctypes.c_int64 * 4)()
        rank = ctypes.c_int()
        for i in range(self._lib.dcscn_num_tensors(self._h)):
            self._check(self._lib.dcscn_tensor_info(self._h, i, name, 256, shape, ctypes.byref(rank)))
            out.append((name.value.decode(), tuple(shape[j] for j in range(rank.value))))
        return out

    def layers(self):
        out = []
        info = LayerInfo()
        for i in range(self._lib.dcscn_num_layers(self._h)):
            self._check(self._lib.dcscn_layer_info_get(self._h, i, ctypes.byref(info)))
            out.append({f: (getattr(info, f).decode() if f == "name" else getattr(info, f)) for f, _ in info._fields_})
        return out

    def ops(self):
        out = []
        info = OpInfo()
        for i in range(self._lib.dcscn_num_ops(self._h)):
            self._check(self._lib.dcscn_op_info_get(self._h, i, ctypes.byref(info)))
            out.append({f: (getattr(info, f).decode() if f in ("name", "kernel") else getattr(info, f))
                        for f, _ in info._fields_})
        return out

    # -- weights -----------------------------------------------------------------------------
    def set_tensor(self, name, array):
        a = np.ascontiguousarray(array, dtype=np.float32)
        shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
        self._check(self._lib.dcscn_set_tensor(self._h, name.encode(), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                               shape, a.ndim))

    def load_weights(self, tensors, winograd=None, fold_tail=None, split16=None):
        """Feed every variable the graph needs from ``{name: ndarray}`` and finalize.
        ``split16=False`` (or DCSCN_SPLIT16=0) keeps every contraction on the f32 kernels; the library default runs the wide
        3x3 and 1x1 convs on the f16 matrix pipe at f32 accuracy (f16 hi/lo split, 3 products, f32 accumulate -- "split16"
        in include/dcscn.h; the option can also be flipped after finalize with ``set_option("split16", 0 / 1)``).
        ``winograd=False`` keeps every 3x3 conv on the direct implicit-GEMM kernel (default: library choice).
        ``fold_tail=False`` executes the reference's layers one by one; the library default runs the linear tail (last
        pixel-shuffler conv, depth_to_space, last reconstruction conv) as one 5x5 conv where that is less work;
        ``fold_tail=True`` (or the environment variable DCSCN_FOLD_TAIL=1; =0 for False) folds wherever the graph has
        such a tail -- see "fold_linear_tail" in include/dcscn.h."""
        if winograd is not None:
            self.set_option("winograd", 1 if winograd else 0)
        if split16 is None and os.environ.get("DCSCN_SPLIT16") in ("0", "1"):
            split16 = os.environ["DCSCN_SPLIT16"] == "1"
        if split16 is not None:
            self.set_option("split16", 1 if split16 else 0)
        if fold_tail is None and os.environ.get("DCSCN_FOLD_TAIL") in ("0", "1"):
            fold_tail = os.environ["DCSCN_FOLD_TAIL"] == "1"
        if fold_tail is not None:
            self.set_option("fold_linear_tail", 2 if fold_tail else 0)       # an explicit request folds wherever it is possible
        for name, _ in self.tensor_specs():
            if name not in tensors:
                raise EngineError(3, "variable '%s' is missing from the checkpoint" % name)
            self.set_tensor(name, tensors[name])
        self.finalize()

    def finalize(self):
        self._check(self._lib.dcscn_finalize(self._h))
        self.finalized = True

    def set_option(self, key, value):
        self._check(self._lib.dcscn_set_option(self._h, key.encode(), int(value)))

    # -- forward -----------------------------------------------------------------------------
    @staticmethod
    def _out_buffer(out, shape):
        if out is None:
            return np.empty(shape, dtype=np.float32)
        if out.dtype != np.float32 or not out.flags.c_contiguous or out.size != int(np.prod(shape)):
            raise EngineError(1, "out must be a C-contiguous float32 array of %s" % (shape,))
        return out.reshape(shape)

    def forward(self, x, x2, out=None):
        """x: [n, h, w, 1] (or [n, h, w]) float32 host array, x2: [n, s*h, s*w, 1]; returns y like x2 (``out``: reuse a
        result buffer -- a fresh 40 MB numpy array costs 2-3 ms of page faults under the download)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        x2 = np.ascontiguousarray(x2, dtype=np.float32)
        if x.ndim == 4:
            if x.shape[3] != 1:
                raise EngineError(1, "x must have one channel, got shape %s" % (x.shape,))
        elif x.ndim != 3:
            raise EngineError(1, "x must be [n, h, w, 1], got shape %s" % (x.shape,))
        n, h, w = x.shape[:3]
        s = self.scale
        if x2.size != n * h * s * w * s:
            raise EngineError(1, "x2 has %d elements, expected %d x %d x %d" % (x2.size, n, h * s, w * s))
        y = self._out_buffer(out, (n, h * s, w * s, 1))
        fp = ctypes.POINTER(ctypes.c_float)
        self._check(self._lib.dcscn_forward(self._h, x.ctypes.data_as(fp), x2.ctypes.data_as(fp),
                                            y.ctypes.data_as(fp), n, h, w))
        return y

    def forward_lr(self, x, out=None):
        """``do(input_image, bicubic_input_image=None)`` (DCSCN.py:547-554): x [n, h, w, 1] (or [n, h, w]); the bicubic
        x2 is computed on the device, bit-compatible with Pillow.  Returns y [n, s*h, s*w, 1]."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim == 4:
            x = x[..., 0]
        n, h, w = x.shape
        s = self.scale
        y = self._out_buffer(out, (n, h * s, w * s, 1))
        fp = ctypes.POINTER(ctypes.c_float)
        self._check(self._lib.dcscn_forward_lr(self._h, np.ascontiguousarray(x).ctypes.data_as(fp), y.ctypes.data_as(fp), n, h, w))
        return y

    def resize_bicubic(self, images, out_height, out_width):
        """Pillow-compatible (mode 'F', BICUBIC) resize of [n, h, w] float images on the device -> [n, oh, ow]."""
        a = np.ascontiguousarray(images, dtype=np.float32)
        single = a.ndim == 2
        if single:
            a = a[None]
        n, h, w = a.shape
        out = np.empty((n, int(out_height), int(out_width)), np.float32)
        fp = ctypes.POINTER(ctypes.c_float)
        self._check(self._lib.dcscn_resize_bicubic(self._h, a.ctypes.data_as(fp), out.ctypes.data_as(fp), n, h, w,
                                                   int(out_height), int(out_width)))
        return out[0] if single else out

    def resize_bicubic_bytes(self, images, out_height, out_width):
        """Pillow's Image.resize(BICUBIC) of uint8 images on the device, bit-identical: [h, w] (mode 'L'), [h, w, 3] ('RGB') or a
        batch [n, h, w, 1 | 3] -> the same layout at [out_height, out_width]."""
        a = np.ascontiguousarray(images)
        if a.dtype != np.uint8 or a.ndim not in (2, 3, 4):
            raise EngineError(1, "expected uint8 images [h, w], [h, w, 3] or [n, h, w, c], got %s %s" % (a.dtype, a.shape))
        n, h, w = (1,) + a.shape[:2] if a.ndim < 4 else a.shape[:3]
        ch = 1 if a.ndim == 2 else a.shape[-1]
        oh, ow = int(out_height), int(out_width)
        out = np.empty((oh, ow) if a.ndim == 2 else a.shape[:-3] + (oh, ow, ch), np.uint8)
        u8 = ctypes.POINTER(ctypes.c_uint8)
        self._check(self._lib.dcscn_resize_bicubic_bytes(self._h, a.ctypes.data_as(u8), out.ctypes.data_as(u8), n, h, w, ch, oh, ow))
        return out

    def resize_bicubic_bytes_device(self, in_ptr, out_ptr, n, h, w, channels, out_height, out_width, stream=None):
        """resize_bicubic_bytes on device pointers (ints), enqueued on ``stream`` (None / 0: the handle's own); does not synchronise."""
        self._check(self._lib.dcscn_resize_bicubic_bytes_device(self._h, ctypes.c_void_p(in_ptr), ctypes.c_void_p(out_ptr), int(n), int(h), int(w),
                                                                int(channels), int(out_height), int(out_width),
                                                                ctypes.c_void_p(stream) if stream else None))

    def stream(self):
        """The handle's own hipStream_t as an int (non-blocking: not ordered against the legacy default stream)."""
        out = ctypes.c_void_p()
        self._check(self._lib.dcscn_get_stream(self._h, ctypes.byref(out)))
        return int(out.value or 0)

    def synchronize(self):
        """Wait for everything enqueued through this handle (whatever stream it ran on)."""
        self._check(self._lib.dcscn_synchronize(self._h))

    def forward_device(self, x_ptr, x2_ptr, y_ptr, n, h, w, stream=None):
        """Enqueue on device pointers (ints, e.g. ``torch.Tensor.data_ptr()``); does not synchronise.

        ``stream``: a hipStream_t as an int; None / 0 means the handle's OWN stream (``self.stream()``), which is not
        ordered against the caller's default stream -- order with ``synchronize()`` or events, or pass a real stream."""
        self._check(self._lib.dcscn_forward_device(self._h, ctypes.c_void_p(x_ptr), ctypes.c_void_p(x2_ptr),
                                                   ctypes.c_void_p(y_ptr), n, h, w,
                                                   ctypes.c_void_p(stream) if stream else None))

    # ---- training (DCSCN.py:334-425; "Training" in include/dcscn.h) ----
    def train_begin(self, flags):
        """build_optimizer: ``flags`` holds the training flags of helper/args.py (optimizer, beta1, beta2, epsilon, momentum,
        l2_decay, clipping_norm, dropout_rate = keep probability, use_l1_loss).  adadelta, adagrad and rmsprop are accepted once
        ``set_option("train_optimizers", 1)`` was called on this handle, and refused without it."""
        c = make_train_config(flags)
        self._check(self._lib.dcscn_train_begin(self._h, ctypes.byref(c)))
        self.training = True

    def _train_arrays(self, x, x2, y_true):
        x = np.ascontiguousarray(x, dtype=np.float32)
        n, h, w = x.shape[0], x.shape[1], x.shape[2]
        s = self.scale
        x2 = np.ascontiguousarray(x2, dtype=np.float32)
        y_true = np.ascontiguousarray(y_true, dtype=np.float32)
        if x.size != n * h * w or x2.size != n * h * w * s * s or y_true.size != n * h * w * s * s:
            raise EngineError(4, "x %s, x2 %s, y_true %s do not match a [n, h, w] / [n, %dh, %dw] batch" % (x.shape, x2.shape, y_true.shape, s, s))
        return x, x2, y_true, n, h, w

    def train_step(self, x, x2, y_true, lr, dropout_key=0):
        """One optimizer step on host arrays; returns (image_loss, mse, gradient norm before clipping, total loss)."""
        x, x2, y_true, n, h, w = self._train_arrays(x, x2, y_true)
        fp = ctypes.POINTER(ctypes.c_float)
        stats = (ctypes.c_double * 4)()
        self._check(self._lib.dcscn_train_step(self._h, x.ctypes.data_as(fp), x2.ctypes.data_as(fp), y_true.ctypes.data_as(fp),
                                               n, h, w, float(lr), int(dropout_key) & (2 ** 64 - 1), stats))
        return tuple(stats)

    def train_gradients(self, x, x2, y_true, dropout_key=0):
        """Forward and backward only; the gradients are then readable as get_tensor("<var>/grad")."""
        x, x2, y_true, n, h, w = self._train_arrays(x, x2, y_true)
        fp = ctypes.POINTER(ctypes.c_float)
        stats = (ctypes.c_double * 4)()
        self._check(self._lib.dcscn_train_gradients(self._h, x.ctypes.data_as(fp), x2.ctypes.data_as(fp), y_true.ctypes.data_as(fp),
                                                    n, h, w, int(dropout_key) & (2 ** 64 - 1), stats))
        return tuple(stats)

    def train_step_device(self, x_ptr, x2_ptr, y_ptr, n, h, w, lr, dropout_key=0, stream=None, want_stats=True):
        """One step on device pointers (e.g. ``torch.Tensor.data_ptr()``); with want_stats the call synchronises and
        returns the stats of train_step, otherwise it only enqueues and returns None."""
        stats = (ctypes.c_double * 4)() if want_stats else None
        self._check(self._lib.dcscn_train_step_device(self._h, ctypes.c_void_p(x_ptr), ctypes.c_void_p(x2_ptr), ctypes.c_void_p(y_ptr),
                                                      int(n), int(h), int(w), float(lr), int(dropout_key) & (2 ** 64 - 1), stats,
                                                      ctypes.c_void_p(stream) if stream else None))
        return tuple(stats) if want_stats else None

    def train_add_image(self, image):
        """Upload a uint8 image [h, w, 1 | 3] (or [h, w]) for train_build_batch / train_step_patches; returns its image id.
        It stays on the device until the engine is closed."""
        a = np.ascontiguousarray(image)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.dtype != np.uint8 or a.ndim != 3:
            raise EngineError(1, "expected a uint8 image [h, w, 1] or [h, w, 3], got %s %s" % (a.dtype, a.shape))
        image_id = ctypes.c_int32()
        self._check(self._lib.dcscn_train_add_image(self._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), a.shape[0], a.shape[1],
                                                    a.shape[2], ctypes.byref(image_id)))
        return image_id.value

    @staticmethod
    def _patches(patches):
        """(rows, pointer, suffix of the entry point): a dcscn_patch array from (image id, top, left, fliplr) rows and "", or -- when
        any row has a fifth field, the transform (imaging.AUGMENT_SUFFIXES) -- a dcscn_patch_aug array (transform 0 where a row has
        none) and "_aug"."""
        rows = [tuple(r) for r in patches]
        fields = 5 if any(len(r) == 5 for r in rows) else 4
        if fields == 5:
            rows = [r + (0,) if len(r) == 4 else r for r in rows]
        p = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, fields))
        return p, ctypes.c_void_p(p.ctypes.data), "_aug" if fields == 5 else ""

    def train_build_batch(self, patches, lr_size, max_value=255.0):
        """The batch of (image id, top, left, fliplr) or (image id, top, left, fliplr, transform) patches as helper/loader.py's
        load_batch_image builds it, on the device: float32 (x [n, lr_size, lr_size, 1], x2 [n, hr, hr, 1], y_true [n, hr, hr, 1])
        with hr = lr_size * scale.  With a transform, top and left are coordinates in the transformed image."""
        p, ptr, aug = self._patches(patches)
        n, lr, hr = len(p), int(lr_size), int(lr_size) * self.scale
        x = np.empty((n, lr, lr, 1), np.float32)
        x2 = np.empty((n, hr, hr, 1), np.float32)
        y = np.empty((n, hr, hr, 1), np.float32)
        fp = ctypes.POINTER(ctypes.c_float)
        self._check(getattr(self._lib, "dcscn_train_build_batch" + aug)(self._h, ptr, n, lr, float(max_value), x.ctypes.data_as(fp), x2.ctypes.data_as(fp),
                                                      y.ctypes.data_as(fp)))
        return x, x2, y

    def train_step_patches(self, patches, lr_size, lr, max_value=255.0, dropout_key=0):
        """train_step on the batch train_build_batch would build, built on the device; returns the stats of train_step."""
        p, ptr, aug = self._patches(patches)
        stats = (ctypes.c_double * 4)()
        self._check(getattr(self._lib, "dcscn_train_step_patches" + aug)(self._h, ptr, len(p), int(lr_size), float(max_value), float(lr),
                                                       int(dropout_key) & (2 ** 64 - 1), stats))
        return tuple(stats)

    # ---- data-parallel training ("Data-parallel training" in include/dcscn.h): records in device memory, pointers as ints ----
    def train_record_floats(self):
        """Length in float32 values of a gradient record of this graph."""
        return int(self._lib.dcscn_train_record_floats(self._h))

    def train_local_gradients_device(self, x_ptr, x2_ptr, y_ptr, n, h, w, record_ptr, dropout_key=0, first_index=0, stream=None):
        """Gradient of the shard [n, h, w] (device pointers) whose first patch is patch ``first_index`` of the global batch, written
        as a record to ``record_ptr``; no update, no synchronisation.  ``stream``: a hipStream_t as an int, None / 0 = the handle's own."""
        self._check(self._lib.dcscn_train_local_gradients_device(
            self._h, ctypes.c_void_p(x_ptr), ctypes.c_void_p(x2_ptr), ctypes.c_void_p(y_ptr), int(n), int(h), int(w),
            int(dropout_key) & (2 ** 64 - 1), int(first_index), ctypes.c_void_p(record_ptr), ctypes.c_void_p(stream) if stream else None))

    def train_local_gradients_patches(self, patches, lr_size, record_ptr, max_value=255.0, dropout_key=0, first_index=0, stream=None):
        """train_local_gradients_device on the shard train_build_batch would build from ``patches``, built on the device."""
        p, ptr, aug = self._patches(patches)
        self._check(getattr(self._lib, "dcscn_train_local_gradients_patches" + aug)(
            self._h, ptr, len(p), int(lr_size), float(max_value), int(dropout_key) & (2 ** 64 - 1), int(first_index),
            ctypes.c_void_p(record_ptr), ctypes.c_void_p(stream) if stream else None))

    def train_apply_records(self, records_ptr, world, lr, stream=None, want_stats=True):
        """Reduce the ``world`` records at ``records_ptr`` ([world, train_record_floats()] float32 on the device) in rank order and
        take the optimizer step; with want_stats the call synchronises and returns the global batch's stats of train_step."""
        stats = (ctypes.c_double * 4)() if want_stats else None
        self._check(self._lib.dcscn_train_apply_records(self._h, ctypes.c_void_p(records_ptr), int(world), float(lr), stats,
                                                        ctypes.c_void_p(stream) if stream else None))
        return tuple(stats) if want_stats else None

    # ---- TensorBoard summaries ("TensorBoard summaries" in include/dcscn.h) ----
    def summarize_device(self, data_ptr, count, stream=None, want_buckets=True):
        """The summary record of ``count`` float32 values at the device pointer ``data_ptr`` (e.g. ``torch.Tensor.data_ptr()``), reduced
        on the device: a dict of num, nonfinite, min, max, sum, sum_squares, mean, stddev and, with want_buckets, "buckets", the
        SUMMARY_BUCKETS int64 counts over summary_bucket_limits().  Synchronises ``stream`` (None / 0 = the handle's own)."""
        rec = Summary()
        buckets = np.zeros(SUMMARY_BUCKETS, np.int64) if want_buckets else None
        self._check(self._lib.dcscn_summarize_device(
            self._h, ctypes.c_void_p(data_ptr), int(count), ctypes.byref(rec),
            buckets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if want_buckets else None, SUMMARY_BUCKETS if want_buckets else 0,
            ctypes.c_void_p(stream) if stream else None))
        return rec.as_dict(buckets)

    def train_log_pass(self, x, x2, y_true):
        """What the reference's summary run computes: forward and backward of the host batch with dropout off, no update, then every
        summarised tensor reduced on the device.  Returns the stats of train_step; afterwards summary(name) reads a record, and
        until the next training call get_tensor reads "<var>/grad" of this pass, "<layer>/output", "x" and "y_"."""
        x, x2, y_true, n, h, w = self._train_arrays(x, x2, y_true)
        fp = ctypes.POINTER(ctypes.c_float)
        stats = (ctypes.c_double * 4)()
        self._check(self._lib.dcscn_train_log_pass(self._h, x.ctypes.data_as(fp), x2.ctypes.data_as(fp), y_true.ctypes.data_as(fp), n, h, w, stats))
        self._log_shape = (n, h, w)
        return tuple(stats)

    def summary_names(self):
        """The names summary() knows after a log pass: every variable, its "/grad", "<layer>/output" per layer, "x", "y_"."""
        names = []
        for n, _ in self.tensor_specs():
            names += [n, n + "/grad"]
        return names + [l["name"] + "/output" for l in self.layers()] + ["x", "y_"]

    def summary(self, name, want_buckets=True):
        """The record of ``name`` from the last train_log_pass, as summarize_device returns it."""
        rec = Summary()
        buckets = np.zeros(SUMMARY_BUCKETS, np.int64) if want_buckets else None
        self._check(self._lib.dcscn_summary_get(self._h, name.encode(), ctypes.byref(rec),
                                                buckets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if want_buckets else None,
                                                SUMMARY_BUCKETS if want_buckets else 0))
        return rec.as_dict(buckets)

    def _activation_shape(self, name):
        """Shape of "x", "y_" or "<layer>/output" for the batch of the last log pass; None: not such a name."""
        shape = getattr(self, "_log_shape", None)
        if shape is None:
            return None
        n, h, w = shape
        s = self.scale
        if name == "x":
            return (n, h, w, 1)
        if name == "y_":
            return (n, h * s, w * s, 1)
        if name.endswith("/output"):
            for l in self.layers():
                if l["name"] == name[:-len("/output")]:
                    r = l["resolution"] * (s if l["name"] == "Up-TCNN" else 1)    # (the transposed conv's output is upscaled)
                    return (n, h * r, w * r, l["out_channels"])
        return None

    def _numel(self, name):
        act = self._activation_shape(name)
        if act is not None:
            return act
        base = name
        for suffix in ("/grad", "/Adam_1", "/Adam", "/Momentum", "/Adagrad", "/Adadelta_1", "/Adadelta", "/RMSProp_1", "/RMSProp"):
            if name.endswith(suffix):
                base = name[: -len(suffix)]
                break
        if base in ("beta1_power", "beta2_power"):
            return ()
        for n, shape in self.tensor_specs():
            if n == base:
                return shape
        raise EngineError(4, "unknown tensor '%s'" % name)

    def get_tensor(self, name):
        """A variable (the trained value while training), "<var>/grad", a slot ("<var>/Adam", "<var>/Adam_1",
        "<var>/Momentum"; behind option "train_optimizers" "<var>/Adagrad", "<var>/Adadelta", "<var>/Adadelta_1", "<var>/RMSProp",
        "<var>/RMSProp_1") or "beta1_power" / "beta2_power", shaped like the checkpoint variable; between a train_log_pass and the
        next training call also "<layer>/output" (NHWC), "x" and "y_" of that pass."""
        shape = self._numel(name)
        out = np.empty(shape, np.float32)
        self._check(self._lib.dcscn_get_tensor(self._h, name.encode(), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size))
        return out

    def set_train_tensor(self, name, array):
        """Write a variable or an optimizer slot of a training handle (resume)."""
        a = np.ascontiguousarray(array, dtype=np.float32)
        self._check(self._lib.dcscn_set_train_tensor(self._h, name.encode(), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), a.size))

    # ---- colour path (helper/utilty.py:142-193 and the RGB pipelines of evaluate.py / sr.py on the device) ----
    @staticmethod
    def _rgb8(image):
        a = np.ascontiguousarray(image)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise EngineError(1, "expected a uint8 RGB image [h, w, 3]")
        return a

    def convert_rgb_to_y(self, image):
        a = self._rgb8(image)
        out = np.empty(a.shape[:2] + (1,), np.float64)
        self._check(self._lib.dcscn_convert_rgb_to_y(self._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), a.shape[0] * a.shape[1]))
        return out

    def convert_rgb_to_ycbcr(self, image):
        a = self._rgb8(image)
        out = np.empty(a.shape, np.float64)
        self._check(self._lib.dcscn_convert_rgb_to_ycbcr(self._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), a.shape[0] * a.shape[1]))
        return out

    def convert_y_and_cbcr_to_rgb(self, y_image, cbcr_image):
        dp = ctypes.POINTER(ctypes.c_double)
        y = np.ascontiguousarray(np.asarray(y_image, np.float64).reshape(y_image.shape[0], y_image.shape[1], -1)[:, :, 0])
        cbcr = np.ascontiguousarray(np.asarray(cbcr_image, np.float64)[:, :, 0:2])
        out = np.empty(y.shape + (3,), np.float64)
        self._check(self._lib.dcscn_convert_y_and_cbcr_to_rgb(self._h, y.ctypes.data_as(dp), cbcr.ctypes.data_as(dp), out.ctypes.data_as(dp), y.size))
        return out

    def evaluate_rgb(self, true_image, n_ensemble=1, want_inputs=False):
        """do_for_evaluate's pipeline for an aligned uint8 RGB image: returns (true_y float64 [H, W, 1], y [H, W, 1]
        -- float32 for n_ensemble <= 1 like sess.run, float64 otherwise like do()'s mean) and, with want_inputs, the LR input."""
        a = self._rgb8(true_image)
        hh, ww = a.shape[:2]
        s = self.scale
        true_y = np.empty((hh, ww, 1), np.float64)
        y = np.empty((hh, ww, 1), np.float64)
        lr = np.empty((hh // s, ww // s, 1), np.float32) if want_inputs else None
        self._check(self._lib.dcscn_evaluate_rgb(self._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), hh, ww, max(1, int(n_ensemble)),
                                                 true_y.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                 lr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if want_inputs else None,
                                                 y.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        if n_ensemble <= 1:
            y = y.astype(np.float32)
        return (true_y, y, lr) if want_inputs else (true_y, y)

    # ---- metrics (helper/utilty.py:509-536 on the device: csrc/metrics.hip) ----
    def psnr_ssim(self, a, b, border_size=0, full=False):
        """compute_psnr_and_ssim(a, b, border_size) for two single-channel images [H, W] or [H, W, 1] of any real dtype:
        (psnr, ssim), or None when the shapes differ, like the host function; ``full``: the whole Metrics struct instead.
        An image with fewer than 11 rows left after shaving is an EngineError (INVALID_ARG, "win_size ...")."""
        a, b = np.asarray(a), np.asarray(b)
        if a.ndim == 2:
            a = a.reshape(a.shape[0], a.shape[1], 1)
        if b.ndim == 2:
            b = b.reshape(b.shape[0], b.shape[1], 1)
        if a.shape != b.shape:
            return None
        if a.ndim != 3 or a.shape[2] != 1:
            raise EngineError(1, "psnr_ssim expects single-channel images, got shape %s" % (a.shape,))
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        dp = ctypes.POINTER(ctypes.c_double)
        out = Metrics()
        self._check(self._lib.dcscn_psnr_ssim(self._h, a.ctypes.data_as(dp), b.ctypes.data_as(dp), a.shape[0], a.shape[1], int(border_size),
                                              ctypes.byref(out)))
        return out if full else (out.psnr, out.ssim)

    def evaluate_rgb_metrics(self, true_image, n_ensemble=1, border_size=0, want_bicubic=False, want_output=False, full=False):
        """evaluate_rgb's pipeline with PSNR / SSIM taken on the device: returns ((psnr, ssim) of the output against the true Y,
        (psnr, ssim) of the bicubic of LR against the true Y or None, the output like evaluate_rgb's or None).  Without
        want_output no image comes back to the host.  ``full``: Metrics structs in place of the pairs."""
        a = self._rgb8(true_image)
        hh, ww = a.shape[:2]
        model = Metrics()
        bicubic = Metrics() if want_bicubic else None
        y = np.empty((hh, ww, 1), np.float64) if want_output else None
        self._check(self._lib.dcscn_evaluate_rgb_metrics(self._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), hh, ww, max(1, int(n_ensemble)),
                                                         int(border_size), ctypes.byref(model), ctypes.byref(bicubic) if want_bicubic else None,
                                                         y.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if want_output else None))
        if want_output and n_ensemble <= 1:
            y = y.astype(np.float32)
        pair = (lambda m: m) if full else (lambda m: (m.psnr, m.ssim))
        return pair(model), pair(bicubic) if want_bicubic else None, y

    def sr_rgb(self, image, upscaled_image, n_ensemble=1):
        """do_for_file's colour branch: (super-resolved Y [s*h, s*w, 1], RGB float64 [s*h, s*w, 3])."""
        a, b = self._rgb8(image), self._rgb8(upscaled_image)
        h, w = a.shape[:2]
        s = self.scale
        if b.shape[:2] != (h * s, w * s):
            raise EngineError(1, "the upscaled image must be %d times the input" % s)
        y = np.empty((h * s, w * s, 1), np.float64)
        rgb = np.empty((h * s, w * s, 3), np.float64)
        u8 = ctypes.POINTER(ctypes.c_uint8)
        dp = ctypes.POINTER(ctypes.c_double)
        self._check(self._lib.dcscn_sr_rgb(self._h, a.ctypes.data_as(u8), b.ctypes.data_as(u8), h, w, max(1, int(n_ensemble)),
                                           y.ctypes.data_as(dp), rgb.ctypes.data_as(dp)))
        if n_ensemble <= 1:
            y = y.astype(np.float32)
        return y, rgb

    SR_BYTES_OUTPUTS = ("rgb_bicubic", "y_bicubic", "y_out", "rgb_out")

    def sr_rgb_bytes(self, image, n_ensemble=1, want=SR_BYTES_OUTPUTS):
        """do_for_file's colour branch from one upload of the uint8 RGB ``image``, every result as the uint8 array save_image
        would write: {"rgb_bicubic": [s*h, s*w, 3], "y_bicubic": [s*h, s*w, 1], "y_out": [s*h, s*w, 1], "rgb_out": [s*h, s*w, 3]},
        restricted to the names in ``want`` (dcscn_sr_rgb_bytes)."""
        a = self._rgb8(image)
        h, w = a.shape[:2]
        s = self.scale
        unknown = [k for k in want if k not in self.SR_BYTES_OUTPUTS]
        if unknown or not want:
            raise EngineError(1, "want must name some of %s, got %s" % (self.SR_BYTES_OUTPUTS, tuple(want)))
        out = {k: np.empty((h * s, w * s, 3 if k.startswith("rgb") else 1), np.uint8) for k in self.SR_BYTES_OUTPUTS if k in want}
        u8 = ctypes.POINTER(ctypes.c_uint8)
        ptrs = [out[k].ctypes.data_as(u8) if k in out else None for k in self.SR_BYTES_OUTPUTS]
        self._check(self._lib.dcscn_sr_rgb_bytes(self._h, a.ctypes.data_as(u8), h, w, max(1, int(n_ensemble)), *ptrs))
        return out

    def forward_ensemble(self, x, x2, n_ensemble):
        """One image [h, w(,1)] + bicubic [s*h, s*w(,1)] -> float64 [s*h, s*w, 1] (do(), DCSCN.py:559-573)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        x2 = np.ascontiguousarray(x2, dtype=np.float32)
        h, w = x.shape[:2]
        s = self.scale
        if x.size != h * w or x2.size != h * s * w * s:
            raise EngineError(1, "forward_ensemble expects single-channel images")
        y = np.empty((h * s, w * s, 1), dtype=np.float64)
        fp = ctypes.POINTER(ctypes.c_float)
        self._check(self._lib.dcscn_forward_ensemble(self._h, x.ctypes.data_as(fp), x2.ctypes.data_as(fp),
                                                     y.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), h, w,
                                                     int(n_ensemble)))
        return y

    def profile(self, with_float32_plan=False):
        """Per-launch milliseconds of the last forward (needs set_option('profile', 1)).  with_float32_plan: one more entry, the gated
        float32 launches behind every split16 pass (they exit at once unless an image left the f16 range; include/dcscn.h "split16")."""
        n = self._lib.dcscn_num_ops(self._h)
        ms = (ctypes.c_double * (n + 1))()
        self._check(self._lib.dcscn_get_profile(self._h, ms, n + 1))
        return list(ms) if with_float32_plan else list(ms)[:n]

    def debug_digests(self):
        """Workspace checksum behind every launch of the last pass + one of its output (needs set_option('debug_digest', 1))."""
        n = self._lib.dcscn_num_ops(self._h) + 1
        out = (ctypes.c_uint64 * n)()
        self._check(self._lib.dcscn_debug_digests(self._h, out, n))
        return [int(v) for v in out]

    def workspace_bytes(self):
        return int(self._lib.dcscn_workspace_bytes(self._h))

    def num_presplit_tensors(self):
        """Workspace tensors the next forward keeps pre-split (option "p16", csrc/p16.hpp)."""
        return int(self._lib.dcscn_num_presplit_tensors(self._h))
