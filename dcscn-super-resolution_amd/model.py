"""``SuperResolution``: the reference's model object (DCSCN.py:28-769) with its inference surface
re-hosted on the MI355X engine.

What stays identical for a caller (sr.py:38-47, evaluate.py:44-107): constructor arguments, the
model-name derivation, ``build_graph / build_optimizer / build_summary_saver / init_all_variables /
load_model``, ``do / do_for_file / do_for_evaluate / do_for_evaluate_with_output /
evaluate_bicubic / evaluate``, their return values, printed lines and output file layout.

What changes underneath: ``build_graph`` derives the layer list instead of a TF graph,
``load_model`` reads the TF checkpoint without TensorFlow (ckpt.py) and uploads it to the HIP
engine, and ``do`` calls the C ABI (engine.py) where the reference calls ``sess.run``.  The
self-ensemble copies run as two device batches instead of eight sequential batch-1 runs.
Training (train.py, DCSCN.py:334-425, 727-769) runs on the engine's training plan: ``build_optimizer`` records the flags,
the first ``train_batch`` after ``init_all_variables`` / ``load_model`` starts it (dcscn_train_begin), and
``save_model`` / ``load_model`` carry the optimizer slots under TF's names once training has begun.
"""

import logging
import math
import os
import shutil
import sys
import time

import numpy as np

from . import ckpt, engine, events, frozen, imaging as util, shard

BICUBIC_METHOD_STRING = "bicubic"


def transposed_conv_initial(scale, channels):
    """The initial value of ``Up-TCNN/Tconv_W`` (utilty.py:366-390): shape [k, k, channels, channels] with k = 2 scale - scale % 2, zero
    everywhere except ``W[:, :, i, i]`` = the bilinear upsampling filter of size k.  Pure numpy: needs neither the library nor a GPU."""
    k = 2 * scale - scale % 2
    factor = (k + 1) // 2
    center = factor - 1 if k % 2 == 1 else factor - 0.5
    row = 1 - np.abs(np.arange(k) - center) / factor
    w = np.zeros((k, k, channels, channels), np.float32)
    for i in range(channels):
        w[:, :, i, i] = np.outer(row, row)
    return w


def _truncated_normal(shape, stddev, rng):
    """Stands for ``tf.truncated_normal``: a standard normal draw clipped at 2 sigma, where TensorFlow redraws what falls outside
    (the one departure of every truncated normal here: a little mass sits exactly on +-2 sigma)."""
    return np.clip(rng.standard_normal(shape), -2.0, 2.0).astype(np.float32) * np.float32(stddev)


def initial_filter(shape, initializer, weight_dev, rng):
    """The initial value of a conv_W / depthwise_W / pointwise_W of HWIO ``shape`` under --initializer and --weight_dev (``utilty.weight``,
    utilty.py:393-413, as tf_graph.py calls it: ``stddev=weight_dev`` and ``uniform`` left False), drawn from the numpy Generator ``rng``."""
    shape = tuple(int(d) for d in shape)
    fan_in = shape[0] * shape[1] * shape[2]
    if initializer == "he":
        return _truncated_normal(shape, math.sqrt(2.0 / fan_in), rng)
    if initializer == "xavier":                                      # uniform=False: the truncated-normal branch (utilty.py:355-357)
        return _truncated_normal(shape, math.sqrt(3.0 / (fan_in + shape[0] * shape[1] * shape[3])), rng)
    if initializer == "uniform":
        return rng.uniform(-2.0 * weight_dev, 2.0 * weight_dev, shape).astype(np.float32)
    if initializer == "stddev":
        return _truncated_normal(shape, weight_dev, rng)
    if initializer == "identity":                                    # He, then 1 at the centre tap of the channel diagonal
        initial = _truncated_normal(shape, math.sqrt(2.0 / fan_in), rng)
        if len(shape) == 4:
            for k in range(min(shape[2], shape[3])):
                initial[shape[0] // 2, shape[1] // 2, k, k] = 1.0
        return initial
    return np.zeros(shape, np.float32)                               # the reference's else branch: any other name


def build_input_image(image, width=0, height=0, channels=1, scale=1, alignment=0, convert_ycbcr=True):
    """Crop / align / convert / downscale a loaded image into the network input (loader.py:42-67)."""
    if width != 0 and height != 0:
        if image.shape[0] != height or image.shape[1] != width:
            x = (image.shape[1] - width) // 2
            y = (image.shape[0] - height) // 2
            image = image[y: y + height, x: x + width, :]
    if alignment > 1:
        image = util.set_image_alignment(image, alignment)
    if channels == 1 and image.shape[2] == 3:
        if convert_ycbcr:
            image = util.convert_rgb_to_y(image)
    elif convert_ycbcr:
        image = util.convert_rgb_to_ycbcr(image)
    if scale != 1:
        image = util.resize_image_by_pil(image, 1.0 / scale)
    return image


class SuperResolution:
    def __init__(self, flags, model_name=""):
        # graph settings (helper/tf_graph.py:19-63)
        self.dropout_rate = flags.dropout_rate
        self.activator = flags.activator
        self.batch_norm = flags.batch_norm
        self.cnn_size = flags.cnn_size
        self.cnn_stride = 1
        self.initializer = flags.initializer
        self.weight_dev = flags.weight_dev
        self.enable_log = flags.enable_log
        self.checkpoint_dir = flags.checkpoint_dir
        self.tf_log_dir = flags.tf_log_dir
        self.gpu_device_id = flags.gpu_device_id

        # model parameters (DCSCN.py:33-48)
        self.scale = flags.scale
        self.layers = flags.layers
        self.filters = flags.filters
        self.min_filters = min(flags.filters, flags.min_filters)
        self.filters_decay_gamma = flags.filters_decay_gamma
        self.use_nin = flags.use_nin
        self.nin_filters = flags.nin_filters
        self.nin_filters2 = flags.nin_filters2
        self.reconstruct_layers = max(flags.reconstruct_layers, 1)
        self.reconstruct_filters = flags.reconstruct_filters
        self.resampling_method = BICUBIC_METHOD_STRING
        self.pixel_shuffler = flags.pixel_shuffler
        self.pixel_shuffler_filters = flags.pixel_shuffler_filters
        self.self_ensemble = flags.self_ensemble
        self.ensemble_group = None          # evaluate.py: a shard.Group when the ensemble transforms of an image are spread over ranks
        self.depthwise_separable = flags.depthwise_separable

        # image processing parameters (DCSCN.py:76-82)
        self.max_value = flags.max_value
        self.channels = flags.channels
        self.output_channels = 1
        self.psnr_calc_border_size = flags.psnr_calc_border_size
        if self.psnr_calc_border_size < 0:
            self.psnr_calc_border_size = self.scale
        # extension: PSNR / SSIM of evaluated images on the device (csrc/metrics.hip) instead of numpy / scipy; off = the host code
        self.device_metrics = bool(getattr(flags, "device_metrics", False))
        # extension: forwards take one f16 product per MAC (engine option "fast16"; set on every engine this model creates)
        self.fast16 = bool(getattr(flags, "fast16", False))
        # extension: ... and the streamed feature extractor of the narrow nets too (engine option "fast16_stream"), independently
        self.fast16_stream = bool(getattr(flags, "fast16_stream", False))
        # extension: ... and the streamed kernels of the separable narrow nets (engine option "fast16_separable"), independently of both
        self.fast16_separable = bool(getattr(flags, "fast16_separable", False))
        # extension: training takes the wide layers' forward / data-gradient convs on the f16 matrix pipe (engine option "train_split16")
        self.train_split16 = bool(getattr(flags, "train_split16", False))
        # extension: ... and their weight gradients (engine option "train_split16_wgrad"), independently
        self.train_split16_wgrad = bool(getattr(flags, "train_split16_wgrad", False))
        # extension: train on the dataset augmentation.py --augment_level N would write, without its files (helper/loader.py)
        self.train_augment_level = int(getattr(flags, "train_augment_level", 0))

        # training parameters (DCSCN.py:50-93)
        fget = lambda k, d: getattr(flags, k, d)
        self.dropout_rate = fget("dropout_rate", 0.8)
        self.l2_decay = fget("l2_decay", 0.0001)
        self.optimizer = fget("optimizer", "adam")
        self.beta1 = fget("beta1", 0.9)
        self.beta2 = fget("beta2", 0.999)
        self.epsilon = fget("epsilon", 1e-8)
        self.momentum = fget("momentum", 0.9)
        self.batch_num = fget("batch_num", 20)
        self.batch_image_size = fget("batch_image_size", 48)
        self.stride_size = fget("stride_size", 0) or self.batch_image_size // 2
        self.clipping_norm = fget("clipping_norm", 5)
        self.use_l1_loss = fget("use_l1_loss", False)
        self.initial_lr = fget("initial_lr", 0.002)
        self.lr_decay = fget("lr_decay", 0.5)
        self.lr_decay_epoch = fget("lr_decay_epoch", 9)
        self.training_images = int(math.ceil(fget("training_images", 24000) / self.batch_num) * self.batch_num)
        self.total_epochs = 0
        lr = self.initial_lr
        while lr > fget("end_lr", 2e-5):
            self.total_epochs += self.lr_decay_epoch
            lr *= self.lr_decay
        self.log_filename = fget("log_filename", "log.txt")
        # extension: write the reference's TensorBoard log (log_to_tensorboard); off = the no-op this model always had.  save_weights and
        # initialize_tf_log are the reference's flags (tf_graph.py:44, DCSCN.py:98-100) and take effect only with it
        self.tensorboard = bool(fget("tensorboard", False))
        self.save_weights = bool(fget("save_weights", True)) and bool(self.enable_log)
        self.initialize_tf_log = bool(fget("initialize_tf_log", True))
        self._train_writer = None           # events.EventWriter on <tf_log_dir>/train, opened by the first log_to_tensorboard that writes
        self._log_image_size = None         # the size of the logged image when it had to be cut to fit the training workspace
        self.train = None
        self.lr = self.initial_lr
        self.step = self.training_step = self.epochs_completed = self.epochs_completed_in_stage = 0
        self.training_loss_sum = self.training_psnr_sum = 0
        self.start_time = time.time()
        self.total_time = 0.0
        # dropout masks: dcscn_train_step's key = dropout_seed * 2^32 + step, so a resumed run given the same step has the same masks
        self.dropout_seed = 0
        self._train_flags = None            # build_optimizer
        self._train_engine = None           # the engine training was begun on
        self._device_images = {}            # filename -> image id of the images uploaded to _train_engine
        self._patches = None                # the batch build_input_batch drew, for the next train_batch
        self._pending_slots = None          # optimizer slots of a checkpoint loaded before training began
        # train.py under torch.distributed.run: a shard.Group whose ranks each train on their shard of every batch and apply the
        # same rank-ordered reduction of all shards' gradients (include/dcscn.h "Data-parallel training"); None: one process
        self.train_group = None
        self._train_stream = None           # the torch stream the data-parallel step is ordered on
        self._record = None                 # this rank's gradient record (a torch tensor on the device)

        self.name = self.get_model_name(model_name)

        # bookkeeping the reference logs from build_graph
        self.features = ""
        self.receptive_fields = 0
        self.complexity = 0
        self.legacy_no_c = False
        self._engine = None
        self._weights = None
        self._pending_init = None

        util.make_dir(self.checkpoint_dir)
        util.set_logging(flags.log_filename, stream_log_level=logging.INFO, file_log_level=logging.INFO)
        logging.info("\nDCSCN v2-------------------------------------")
        logging.info("%s [%s]" % (util.get_now_date(), self.name))

    # ---- naming (DCSCN.py:108-144) -----------------------------------------------------------
    def get_model_name(self, model_name, name_postfix=""):
        if model_name != "":
            return "dcscn_%s" % model_name
        name = "dcscn_L%d_F%d" % (self.layers, self.filters)
        if self.min_filters != 0:
            name += "to%d" % self.min_filters
        if self.filters_decay_gamma != 1.5:
            name += "_G%2.2f" % self.filters_decay_gamma
        if self.cnn_size != 3:
            name += "_C%d" % self.cnn_size
        if self.scale != 2:
            name += "_Sc%d" % self.scale
        if self.use_nin:
            name += "_NIN"
            if self.nin_filters != 0:
                name += "_A%d" % self.nin_filters
            if self.nin_filters2 != self.nin_filters // 2:
                name += "_B%d" % self.nin_filters2
        if self.pixel_shuffler:
            name += "_PS"
        if self.max_value != 255.0:
            name += "_M%2.1f" % self.max_value
        if self.activator != "prelu":
            name += "_%s" % self.activator
        if self.batch_norm:
            name += "_BN"
        if self.depthwise_separable:
            name += "_DS"
        if self.reconstruct_layers >= 1:
            name += "_R%d" % self.reconstruct_layers
            if self.reconstruct_filters != 1:
                name += "F%d" % self.reconstruct_filters
        if name_postfix != "":
            name += "_" + name_postfix
        return name

    # ---- graph -------------------------------------------------------------------------------
    def _engine_config(self):
        return dict(scale=self.scale, layers=self.layers, filters=self.filters, min_filters=self.min_filters,
                    filters_decay_gamma=self.filters_decay_gamma, cnn_size=self.cnn_size, use_nin=self.use_nin,
                    nin_filters=self.nin_filters, nin_filters2=self.nin_filters2,
                    reconstruct_layers=self.reconstruct_layers, reconstruct_filters=self.reconstruct_filters,
                    activator=self.activator, pixel_shuffler=self.pixel_shuffler,
                    pixel_shuffler_filters=self.pixel_shuffler_filters,
                    depthwise_separable=self.depthwise_separable, channels=self.channels,
                    legacy_no_c=self.legacy_no_c, batch_norm=self.batch_norm)

    def _create_engine(self):
        if self._engine is not None:
            self._engine.close()
        self._engine = engine.Engine(self._engine_config(), device=self.gpu_device_id)
        if self.fast16:
            self._engine.set_option("fast16", 1)
        if self.fast16_stream:
            self._engine.set_option("fast16_stream", 1)
        if self.fast16_separable:
            self._engine.set_option("fast16_separable", 1)
        self._weights = None
        return self._engine

    def build_graph(self):
        """Instantiate the layer plan on the device and log what the reference logs (DCSCN.py:331-332)."""
        eng = self._create_engine()
        self._log_graph(eng)

    def _log_graph(self, eng):
        layers = eng.layers()
        feats, total, rf, complexity = [], 0, 0, 0
        for i, li in enumerate(layers):
            cout, k, cin = li["out_channels"], li["kernel_size"], li["in_channels"]
            feats.append(cout)
            if i < self.layers:
                total += cout
            # "Complexity" counts every layer at LR resolution (tf_graph.py:100,106,110)
            complexity += (k * k * cin + cin * cout) if li["depthwise_separable"] else k * k * cin * cout
            complexity += cout if li["has_bias"] else 0
            complexity += cout if li["activator"] != 0 else 0
            rf = k if rf == 0 else rf + (k - 1)
        if self.use_nin:
            rf -= (self.cnn_size - 1)                         # DCSCN.py:275
        self.features = " ".join("%d" % f for f in feats[:self.layers]) + " Total: (%d) " % total \
                        + " ".join("%d" % f for f in feats[self.layers:]) + " "
        self.complexity = complexity
        self.receptive_fields = rf
        logging.info("Feature:%s Complexity:%s Receptive Fields:%d" % (
            self.features, "{:,}".format(self.complexity), self.receptive_fields))

    def build_optimizer(self):
        """DCSCN.py:334-413: loss (mse or l1, + l2_decay * sum of l2_loss over the filters), clip_by_global_norm, and the
        optimizer of --optimizer.  The engine's training plan is started on the first train_batch, after the variables
        are initialised or restored; adadelta / adagrad / rmsprop run with TF 1.x's default constants, as the reference
        constructs them (DCSCN.py:383-392), behind the engine's option "train_optimizers", which the first train_batch sets."""
        self._train_flags = dict(optimizer=self.optimizer, beta1=self.beta1, beta2=self.beta2, epsilon=self.epsilon,
                                 momentum=self.momentum, l2_decay=self.l2_decay, clipping_norm=self.clipping_norm,
                                 dropout_rate=self.dropout_rate, use_l1_loss=self.use_l1_loss)

    def build_summary_saver(self, with_saver=True):
        """TensorBoard writers / Saver in the reference (tf_graph.py:298-305); nothing to create: the event writer of --tensorboard is opened
        by the first log_to_tensorboard that writes."""

    def init_all_variables(self):
        """``tf.global_variables_initializer`` (tf_graph.py:73-75): filters drawn by --initializer (``initial_filter``; He
        truncated-normal by default, utilty.py:360-363), zero bias, PReLU slope 0.1, the bilinear Tconv_W of a transposed-conv net --
        replaced by ``load_model`` for real use."""
        if self._engine is None:
            self.build_graph()
        rng = np.random.default_rng()
        tensors = {}
        for name, shape in self._engine.tensor_specs():
            leaf = name.rsplit("/", 1)[-1]
            if leaf in ("conv_W", "depthwise_W", "pointwise_W"):
                tensors[name] = initial_filter(shape, self.initializer, self.weight_dev, rng)
            elif leaf == "conv_B":
                tensors[name] = np.zeros(shape, np.float32)
            elif leaf == "Tconv_W":
                tensors[name] = transposed_conv_initial(self.scale, shape[2])
            else:
                tensors[name] = np.full(shape, 0.1, np.float32)
        if self._data_parallel():
            tensors = self.train_group.broadcast_object(tensors)      # every replica starts from rank 0's draw
        self._pending_init = tensors
        print("Model initialized.")

    # ---- checkpoint (tf_graph.py:263-280) ------------------------------------------------------
    def load_model(self, name="", trial=0, output_log=False):
        if name == "" or name == "default":
            name = self.name
        if trial > 0:
            filename = self.checkpoint_dir + "/" + name + "_" + str(trial) + ".ckpt"
        else:
            filename = self.checkpoint_dir + "/" + name + ".ckpt"
        if not os.path.isfile(filename + ".index"):
            print("Error. [%s] is not exist!" % filename)
            sys.exit(-1)
        if not ckpt.has_data(filename):
            print("Error. [%s] has no data shard (.data-00000-of-00001)!" % filename)
            sys.exit(-1)
        if self._train_flags is not None:
            # a training run: the variables and, when the checkpoint has them, the optimizer slots (tf.train.Saver restores both)
            tensors = ckpt.load_checkpoint(filename, include_optimizer_slots=True)
            if self._data_parallel():
                tensors = self.train_group.broadcast_object(tensors)  # rank 0's variables and slots, whatever the other ranks read
            slots = {k: v for k, v in tensors.items() if ckpt.is_optimizer_slot(k)}
            self.load_weights({k: v for k, v in tensors.items() if k not in slots})
            self._pending_slots = slots or None
        else:
            tensors = ckpt.load_checkpoint(filename)
            self.load_weights(tensors)
        if output_log:
            logging.info("Model restored [ %s ]." % filename)
        else:
            print("Model restored [ %s ]." % filename)

    def save_model(self, name="", trial=0, output_log=False):
        """tf.train.Saver.save (tf_graph.py:282-296): the model's variables as a TF V2 checkpoint
        (``<checkpoint_dir>/<name>[_<trial>].ckpt.{index,data-00000-of-00001}`` + the ``checkpoint`` state file), written
        without TensorFlow (ckpt.save_checkpoint; byte-identical to what the reference's Saver writes for the same tensors)."""
        if name == "" or name == "default":
            name = self.name
        if trial > 0:
            filename = self.checkpoint_dir + "/" + name + "_" + str(trial) + ".ckpt"
        else:
            filename = self.checkpoint_dir + "/" + name + ".ckpt"
        if self._training_active():
            tensors = self._training_tensors()             # the trained variables and the optimizer slots, as TF's Saver writes them
        else:
            tensors = self._weights if self._weights is not None else self._pending_init
        if tensors is None:
            self.init_all_variables()
            tensors = self._pending_init
        ckpt.save_checkpoint(filename, tensors)
        if output_log:
            logging.info("Model saved [%s]." % filename)
        else:
            print("Model saved [%s]." % filename)

    def load_graph(self, frozen_graph_filename="./model_to_freeze/frozen_model_optimized.pb"):
        """--frozenInference (DCSCN.py:192-220): the weights come from the Const nodes of a frozen GraphDef (variables keep
        their checkpoint names through freeze_graph / optimize_for_inference); the topology is the one the flags describe,
        and a file that does not fit it is rejected by the engine (missing variable / shape mismatch)."""
        if not os.path.isfile(frozen_graph_filename):
            print("Error. [%s] is not exist!" % frozen_graph_filename)
            sys.exit(-1)
        tensors = frozen.read_frozen_graph(frozen_graph_filename)
        if not any(k.endswith(("/conv_W", "/pointwise_W")) for k in tensors):
            tensors = frozen.read_frozen_graph(frozen_graph_filename, prefix="prefix/")     # a re-exported import_graph_def copy
        self.load_weights({k: v for k, v in tensors.items() if not ckpt.is_optimizer_slot(k)})
        print("Frozen graph loaded [ %s ]." % frozen_graph_filename)

    def load_weights(self, tensors):
        """Upload ``{variable name: ndarray}``.  Checkpoints written by the reference's older graph
        (the shipped dcscn_L2_* files: use_nin=False and no 1x1 "C" layer) are recognised by their
        variable set and get the matching topology."""
        legacy = (not self.use_nin) and ("C/conv_W" not in tensors) and ("C/pointwise_W" not in tensors)
        if legacy != self.legacy_no_c or self._engine is None or self._engine.finalized:
            self.legacy_no_c = legacy
            self._create_engine()
        self._engine.load_weights(tensors)
        self._weights = tensors
        self._pending_init = None

    def _ready_engine(self):
        if self._engine is None:
            self.build_graph()
        if not self._engine.finalized:
            pending = self._pending_init
            if pending is None:
                self.init_all_variables()
                pending = self._pending_init
            self._engine.load_weights(pending)
            self._pending_init = None
        return self._engine

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None
        self._train_engine = None
        if self._train_writer is not None:
            self._train_writer.close()
            self._train_writer = None

    # ---- training (DCSCN.py:146-190, 426-532, 727-769) ---------------------------------------------
    def load_dynamic_datasets(self, data_dir, batch_image_size):
        """Opens an image directory as a dataset; patches are cut when build_input_batch() is called."""
        from helper import loader
        self.train = loader.DynamicDataSets(self.scale, batch_image_size, channels=self.channels,
                                            resampling_method=self.resampling_method, augment_level=self.train_augment_level)
        self.train.set_data_dir(data_dir)

    def load_datasets(self, data_dir, batch_dir, batch_image_size, stride_size=0):
        """BatchDataSets (--build_batch true) is not supported: train from the image directory (DynamicDataSets)."""
        print("Error. --build_batch true (BatchDataSets) is not supported; use --build_batch false.")
        sys.exit(-1)

    def _training_active(self):
        return self._train_engine is not None and self._train_engine is self._engine

    def _data_parallel(self):
        return self.train_group is not None and self.train_group.world > 1

    def _ready_training(self):
        if self._train_flags is None:
            raise RuntimeError("train_batch() before build_optimizer()")
        eng = self._ready_engine()
        if self._train_engine is not eng:
            if self._data_parallel():
                self.step = self.train_group.broadcast_object(self.step)   # the dropout key counts steps: rank 0's, when resuming
            if self.depthwise_separable:
                eng.set_option("train_separable", 1)             # read by train_begin: without it a separable net is refused
            if not self.pixel_shuffler:
                eng.set_option("train_transposed", 1)            # likewise for the transposed-conv upsampler
            if self.optimizer in engine.MORE_OPTIMIZERS:
                eng.set_option("train_optimizers", 1)            # likewise for adadelta, adagrad and rmsprop
            eng.train_begin(self._train_flags)
            if self.train_split16:
                eng.set_option("train_split16", 1)
            if self.train_split16_wgrad:
                eng.set_option("train_split16_wgrad", 1)
            self._train_engine = eng
            self._device_images = {}
            if self._pending_slots:
                for name, value in self._pending_slots.items():
                    eng.set_train_tensor(name, value)
            self._pending_slots = None
        return eng

    def _training_tensors(self):
        eng = self._engine
        names = [n for n, _ in eng.tensor_specs()]
        tensors = {n: eng.get_tensor(n) for n in names}
        for n in names:
            for slot in ckpt.OPTIMIZER_SLOTS[self.optimizer]:       # TF's slot names of --optimizer
                tensors[n + "/" + slot] = eng.get_tensor(n + "/" + slot)
        if self.optimizer == "adam":
            tensors["beta1_power"] = eng.get_tensor("beta1_power")
            tensors["beta2_power"] = eng.get_tensor("beta2_power")
        return tensors

    def init_epoch_index(self):
        self.batch_input = self.batch_num * [None]
        self.batch_input_bicubic = self.batch_num * [None]
        self.batch_true = self.batch_num * [None]
        self.training_psnr_sum = 0
        self.training_loss_sum = 0
        self.training_step = 0
        self.train.init_batch_index()

    def build_input_batch(self):
        """Draws the next batch_num patches (helper/loader.py next_patch); the next train_batch cuts them on the device, with
        the results load_batch_image gives on the host."""
        if self.channels != 1:
            raise NotImplementedError("training batches are built for channels = 1 (Y) only")
        self._patches = [self.train.next_patch() for _ in range(self.batch_num)]

    def training_digest(self):
        """sha256 over the variables, optimizer slots and beta powers of the running training, in name order: equal on two
        replicas exactly when they hold the same bits."""
        import hashlib
        digest = hashlib.sha256()
        for name, value in sorted(self._training_tensors().items()):
            digest.update(name.encode())
            digest.update(np.ascontiguousarray(value, dtype=np.float32).tobytes())
        return digest.hexdigest()

    def _train_shard_step(self, eng, descriptors, first_index):
        """The data-parallel step: this rank's shard of the batch (its patches, the first of them patch ``first_index`` of the
        batch) -> its record, all records gathered, the same rank-ordered reduction and update on every rank.  Returns the stats
        of the whole batch."""
        import torch
        group = self.train_group
        device = torch.device("cuda", eng.device)
        if self._record is None or self._record.device != device:
            self._train_stream = torch.cuda.Stream(device=device)
            self._record = torch.empty(eng.train_record_floats(), dtype=torch.float32, device=device)
        with torch.cuda.stream(self._train_stream):
            stream = self._train_stream.cuda_stream
            eng.train_local_gradients_patches(descriptors, self.train.batch_image_size, self._record.data_ptr(), max_value=self.max_value,
                                              dropout_key=self.dropout_key(), first_index=first_index, stream=stream)
            records = group.all_gather_records(self._record)
            return eng.train_apply_records(records.data_ptr(), group.world, self.lr, stream=stream)

    def dropout_key(self):
        return (int(self.dropout_seed) << 32) + int(self.step)

    def train_batch(self):
        """One optimizer step on the current batch (sess.run(training_optimizer, ...), DCSCN.py:426-436)."""
        eng = self._ready_training()
        if self._patches is not None:      # drawn by build_input_batch: built on the device from the uploaded images
            patches, self._patches = self._patches, None
            begin, end = 0, len(patches)
            if self._data_parallel():      # every rank drew the whole batch; it uploads and cuts only its own shard
                begin, end = shard.train_shard(len(patches), self.train_group.rank, self.train_group.world)
            descriptors = []
            for filename, *fields in patches[begin:end]:       # (top, left, fliplr), with train_augment_level >= 2 also the transform
                image_id = self._device_images.get(filename)    # one upload per base file: a variant is an index map over it
                if image_id is None:
                    image_id = self._device_images[filename] = eng.train_add_image(self.train.image(filename))
                descriptors.append((image_id, *fields))
            if self._data_parallel():
                image_loss, mse, _, _ = self._train_shard_step(eng, descriptors, begin)
            else:
                image_loss, mse, _, _ = eng.train_step_patches(descriptors, self.train.batch_image_size, self.lr, max_value=self.max_value,
                                                               dropout_key=self.dropout_key())
        else:                              # arrays assigned to batch_input, batch_input_bicubic, batch_true
            x = np.stack([np.asarray(a, np.float32).reshape(a.shape[0], a.shape[1], 1) for a in self.batch_input])
            x2 = np.stack([np.asarray(a, np.float32).reshape(a.shape[0], a.shape[1], 1) for a in self.batch_input_bicubic])
            y = np.stack([np.asarray(a, np.float32).reshape(a.shape[0], a.shape[1], 1) for a in self.batch_true])
            if self._data_parallel():
                raise NotImplementedError("data-parallel training takes the batches build_input_batch draws, not assigned arrays")
            image_loss, mse, _, _ = eng.train_step(x, x2, y, self.lr, dropout_key=self.dropout_key())
        self.training_loss_sum += image_loss
        self.training_psnr_sum += 0 if mse == 0 else 20 * math.log(self.max_value / math.sqrt(mse), 10)
        self.training_step += 1
        self.step += 1

    def log_to_tensorboard(self, test_filename, psnr, save_meta_data=True):
        """TensorBoard summaries (DCSCN.py:427-479), written only with --tensorboard (and enable_log); otherwise a no-op.

        One log pass of the engine on the test image (forward and backward with dropout off, every summary reduced on the device:
        dcscn_train_log_pass), then one Event at step = epochs_completed with every summary of events.summary_plan, and the scalars
        PSNR (the mean training PSNR; not with use_l1_loss or before any step) and LR, under <tf_log_dir>/train.  With save_weights
        false only the scalars (Loss, L2WeightDecayLoss, PSNR, LR) are written.  In a data-parallel run rank 0 writes, from the first step on.
        Departures: the reference's second writer (<tf_log_dir>/test: the graph and the test PSNR) is not written; an image that does
        not fit the training workspace (training never tiles) is cut to half its longer side, from the top left, until it fits."""
        if not (self.tensorboard and self.enable_log):
            return
        if self._data_parallel() and self.train_group.rank != 0:
            return
        if self._data_parallel() and not self._training_active():
            # train.py's log before the first step: beginning the training here would be rank 0 alone in _ready_training's broadcast
            logging.info("tensorboard: the log before the first step is not written in a data-parallel run")
            return
        eng = self._ready_training()
        org_image = util.set_image_alignment(util.load_image(test_filename, print_console=False), self.scale)
        if len(org_image.shape) >= 3 and org_image.shape[2] == 3 and self.channels == 1:
            org_image = util.convert_rgb_to_y(org_image)
        while True:
            input_image = util.resize_image_by_pil(org_image, 1.0 / self.scale, resampling_method=self.resampling_method)
            bicubic_image = util.resize_image_by_pil(input_image, self.scale, resampling_method=self.resampling_method)
            batch = [input_image, bicubic_image, org_image]
            if self.max_value != 255.0:
                batch = [np.multiply(a, self.max_value / 255.0) for a in batch]
            try:
                stats = eng.train_log_pass(*[np.asarray(a, np.float32).reshape((1,) + a.shape[:2] + (1,)) for a in batch])
                break
            except engine.EngineError as exc:
                if exc.status != 7:                                    # DCSCN_ERR_NOMEM
                    raise
                nomem = exc
            h, w = org_image.shape[:2]
            if h >= w:
                h = h // 2 // self.scale * self.scale
            else:
                w = w // 2 // self.scale * self.scale
            if h < self.scale or w < self.scale:
                raise nomem
            org_image = org_image[:h, :w]
            if self._log_image_size is None or (h, w) < self._log_image_size:
                self._log_image_size = (h, w)
                logging.info("tensorboard: the logged image is cut to %d x %d to fit the training workspace" % (w, h))
        values, records = [], {}
        variables = [n for n, _ in eng.tensor_specs()]
        for kind, tag, source, field in events.summary_plan(eng.layers(), variables, self.name, l2_decay=self.l2_decay, save_weights=self.save_weights):
            if source == "loss":
                values.append((tag, stats[3]))
                continue
            if source == "l2_loss":
                values.append((tag, stats[3] - stats[0]))
                continue
            rec = records.get(source)
            if rec is None:
                rec = records[source] = eng.summary(source)
            if rec["nonfinite"]:                                       # (TensorFlow's histogram op: "Nan in summary histogram for: ...")
                raise ValueError("Nan in summary histogram for: %s (%d non-finite values)" % (tag, rec["nonfinite"]))
            values.append((tag, rec[field] if kind == "scalar" else rec))
        if self._train_writer is None:
            util.make_dir(self.tf_log_dir)
            if self.initialize_tf_log:
                util.clean_dir(self.tf_log_dir)
            self._train_writer = events.EventWriter(os.path.join(self.tf_log_dir, "train"), limits=engine.summary_bucket_limits())
        writer = self._train_writer
        writer.add_summary(values, self.epochs_completed)
        if not self.use_l1_loss and self.training_step != 0:
            writer.add_scalar("PSNR", self.training_psnr_sum / self.training_step, self.epochs_completed)
        writer.add_scalar("LR", self.lr, self.epochs_completed)
        writer.flush()

    def update_epoch_and_lr(self):
        self.epochs_completed_in_stage += 1
        if self.epochs_completed_in_stage >= self.lr_decay_epoch:
            self.lr *= self.lr_decay
            self.epochs_completed_in_stage = 0
            return True
        return False

    def init_train_step(self):
        self.lr = self.initial_lr
        self.epochs_completed = 0
        self.epochs_completed_in_stage = 0
        self.min_validation_mse = -1
        self.min_validation_epoch = -1
        self.step = 0
        self.start_time = time.time()

    def end_train_step(self):
        self.total_time = time.time() - self.start_time

    def print_status(self, psnr, ssim, log=False):
        if self.step == 0:
            logging.info("Initial PSNR:%f SSIM:%f" % (psnr, ssim))
            return
        processing_time = (time.time() - self.start_time) / self.step
        if self.use_l1_loss:
            line_a = "%s Step:%s PSNR:%f SSIM:%f (Training Loss:%0.3f)" % (
                util.get_now_date(), "{:,}".format(self.step), psnr, ssim, self.training_loss_sum / max(self.training_step, 1))
        else:
            line_a = "%s Step:%s PSNR:%f SSIM:%f (Training PSNR:%0.3f)" % (
                util.get_now_date(), "{:,}".format(self.step), psnr, ssim, self.training_psnr_sum / max(self.training_step, 1))
        estimated = processing_time * (self.total_epochs - self.epochs_completed) * (self.training_images // self.batch_num)
        h = estimated // (60 * 60)
        estimated -= h * 60 * 60
        m = estimated // 60
        s = estimated - m * 60
        line_b = "Epoch:%d LR:%f (%2.3fsec/step) Estimated:%d:%d:%d" % (self.epochs_completed, self.lr, processing_time, h, m, s)
        if log:
            logging.info(line_a)
            logging.info(line_b)
        else:
            print(line_a)
            print(line_b)

    def print_steps_completed(self, output_to_logging=False):
        if self.step == 0:
            return
        processing_time = self.total_time / self.step
        h = self.total_time // (60 * 60)
        m = (self.total_time - h * 60 * 60) // 60
        s = (self.total_time - h * 60 * 60 - m * 60)
        status = "Finished at Total Epoch:%d Steps:%s Time:%02d:%02d:%02d (%2.3fsec/step) %d x %d x %d patches" % (
            self.epochs_completed, "{:,}".format(self.step), h, m, s, processing_time,
            self.batch_image_size, self.batch_image_size, self.training_images)
        if output_to_logging:
            logging.info(status)
        else:
            print(status)

    def copy_log_to_archive(self, archive_name):
        """tf_graph.py:251-261 archives the TensorBoard log directory; there is none here, so the text log is archived."""
        if not self.log_filename or not os.path.isfile(self.log_filename):
            return
        archive_directory = self.tf_log_dir + "_" + archive_name
        util.make_dir(archive_directory)
        target = os.path.join(archive_directory, self.name + "_" + os.path.basename(self.log_filename))
        try:
            shutil.copyfile(self.log_filename, target)
            print("log archived to [%s]." % target)
        except OSError as e:
            print(e)

    # ---- inference (DCSCN.py:547-586) ----------------------------------------------------------
    def do(self, input_image, bicubic_input_image=None):
        h, w = input_image.shape[:2]
        ch = input_image.shape[2] if len(input_image.shape) > 2 else 1
        if ch != 1:
            raise ValueError("do() expects a single-channel image, got %d channels" % ch)
        # the device bicubic reproduces Pillow's mode-'F' path (float images) here.  A uint8 single-channel image goes through
        # Pillow's mode 'L' in the reference (utilty.py:229-232: rounded and clipped to 0..255): _resize_bytes below
        if bicubic_input_image is None and self.resampling_method == "bicubic" and np.issubdtype(np.asarray(input_image).dtype, np.floating):
            # DCSCN.py:552-554 on the device: dcscn_resize_bicubic is bit-compatible with Pillow's mode-'F' BICUBIC
            # (tests/test_resize_hip.py), so x2 never has to be built or uploaded by the host
            eng = self._ready_engine()
            x = np.ascontiguousarray(input_image, dtype=np.float32).reshape(h, w)
            if self.max_value == 255.0 and self.self_ensemble <= 1:
                return eng.forward_lr(x[None])[0]
            bicubic_input_image = eng.resize_bicubic(x, self.scale * h, self.scale * w).reshape(self.scale * h, self.scale * w, 1)
        elif bicubic_input_image is None:
            bicubic_input_image = self._resize_bytes(input_image, self.scale)
        if self.max_value != 255.0:
            input_image = np.multiply(input_image, self.max_value / 255.0)
            bicubic_input_image = np.multiply(bicubic_input_image, self.max_value / 255.0)

        eng = self._ready_engine()
        x = np.ascontiguousarray(input_image, dtype=np.float32).reshape(h, w)
        x2 = np.ascontiguousarray(bicubic_input_image, dtype=np.float32).reshape(self.scale * h, self.scale * w)
        if self.self_ensemble > 1 and self.ensemble_group is not None:
            # (image, transform) work items sharded over the ranks (evaluate.py); float64 mean in the reference's order
            output = self.ensemble_group.ensemble_mean(
                x[:, :, None], x2[:, :, None], self.self_ensemble,
                lambda a, b: eng.forward(a[None], b[None])[0], util.flip)
            if output is None:
                return None                                   # not rank 0: the mean (and everything computed from it) lives there
        elif self.self_ensemble > 1:
            output = eng.forward_ensemble(x, x2, self.self_ensemble)            # float64, like np.zeros + +=
        else:
            output = eng.forward(x[None, :, :, None], x2[None, :, :, None])[0]   # float32, like sess.run
        if self.max_value != 255.0:
            return np.multiply(output, 255.0 / self.max_value)
        return output

    def do_batch(self, lr_batch, bicubic_batch):
        """Extension: [n, h, w, 1] + [n, s*h, s*w, 1] float32 -> [n, s*h, s*w, 1] in one device pass."""
        return self._ready_engine().forward(lr_batch, bicubic_batch)

    @util.with_deferred_saves                                # the PNGs are encoded on worker threads; on disk when this returns
    def do_for_file(self, file_path, output_folder="output"):
        """sr.py's work (DCSCN.py:588-614): writes the original, bicubic and SR images."""
        org_image = util.load_image(file_path)
        filename, extension = os.path.splitext(os.path.basename(file_path))
        output_folder += "/" + self.name + "/"
        util.save_image(output_folder + filename + extension, org_image)

        colour = len(org_image.shape) >= 3 and org_image.shape[2] == 3 and self.channels == 1
        if colour and self._device_colour_path(org_image):
            # both bicubic images, Y, the forward pass, the YCbCr -> RGB recombination and save_image's uint8 cast in one
            # device pipeline from one upload (dcscn_sr_rgb_bytes): the four arrays arrive as the bytes of their files
            out = self._ready_engine().sr_rgb_bytes(org_image, self.self_ensemble)
            util.save_image(output_folder + filename + "_bicubic" + extension, out["rgb_bicubic"])
            util.save_image(output_folder + filename + "_bicubic_y" + extension, out["y_bicubic"])
            util.save_image(output_folder + filename + "_result_y" + extension, out["y_out"])
            util.save_image(output_folder + filename + "_result" + extension, out["rgb_out"])
            return
        if colour:
            scaled_image = util.resize_image_by_pil(org_image, self.scale, resampling_method=self.resampling_method)
            util.save_image(output_folder + filename + "_bicubic" + extension, scaled_image)
            input_y_image = util.convert_rgb_to_y(org_image)
            scaled_image = util.resize_image_by_pil(input_y_image, self.scale, resampling_method=self.resampling_method)
            util.save_image(output_folder + filename + "_bicubic_y" + extension, scaled_image)
            output_y_image = self.do(input_y_image)
            util.save_image(output_folder + filename + "_result_y" + extension, output_y_image)
            scaled_ycbcr_image = util.convert_rgb_to_ycbcr(
                util.resize_image_by_pil(org_image, self.scale, self.resampling_method))
            image = util.convert_y_and_cbcr_to_rgb(output_y_image, scaled_ycbcr_image[:, :, 1:3])
        else:
            scaled_image = self._resize_bytes(org_image, self.scale)      # (the reference resizes twice: one image, two files)
            util.save_image(output_folder + filename + "_bicubic" + extension, scaled_image)
            util.save_image(output_folder + filename + "_bicubic_y" + extension, scaled_image)
            image = self.do(org_image)
        util.save_image(output_folder + filename + "_result" + extension, image)

    def _device_byte_resize(self, image):
        """A uint8 image of 1 or 3 channels through the device's 8-bit bicubic (Pillow's modes 'L' / 'RGB', bit-identical); it
        needs an engine but no weights.  Other resampling methods stay with Pillow."""
        return (self.resampling_method == BICUBIC_METHOD_STRING and self._engine is not None and image.dtype == np.uint8
                and (image.ndim == 2 or (image.ndim == 3 and image.shape[2] in (1, 3))))

    def _resize_bytes(self, image, scale):
        """util.resize_image_by_pil(image, scale, self.resampling_method), on the device where _device_byte_resize allows."""
        image = np.asarray(image)
        if not self._device_byte_resize(image):
            return util.resize_image_by_pil(image, scale, resampling_method=self.resampling_method)
        height, width = image.shape[0], image.shape[1]
        out = self._engine.resize_bicubic_bytes(image, int(height * scale), int(width * scale))
        return out.reshape(out.shape[0], out.shape[1], -1)

    def _device_colour_path(self, image):
        """uint8 RGB through the device colour / bicubic kernels: they reproduce the float64 numpy colour math and
        Pillow's mode-'F' BICUBIC only (other resampling methods, other value ranges stay on the host path)."""
        return (self.resampling_method == BICUBIC_METHOD_STRING and self.max_value == 255.0 and self.channels == 1
                and image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3
                and self.ensemble_group is None)              # the all-device pipeline runs the whole ensemble on this rank

    def _metrics(self, image1, image2):
        """compute_psnr_and_ssim at the model's border: on the host, or with device_metrics on the device (dcscn_psnr_ssim)."""
        if not self.device_metrics:
            return util.compute_psnr_and_ssim(image1, image2, border_size=self.psnr_calc_border_size)
        return self._on_device_metrics(self._ready_engine().psnr_ssim, image1, image2, border_size=self.psnr_calc_border_size)

    @staticmethod
    def _on_device_metrics(call, *args, **kwargs):
        """The engine's refusal of an image too small for the 11-row SSIM window, as the ValueError the host code raises."""
        try:
            return call(*args, **kwargs)
        except engine.EngineError as e:
            if e.status == 1 and "win_size" in e.message:
                raise ValueError("win_size exceeds image extent")
            raise

    def _evaluate_rgb_metrics(self, true_image, n_ensemble, want_bicubic=False):
        """(model pair, bicubic pair or None) of an RGB file wholly on the device: no image is downloaded (dcscn_evaluate_rgb_metrics)."""
        return self._on_device_metrics(self._ready_engine().evaluate_rgb_metrics, true_image, n_ensemble,
                                       border_size=self.psnr_calc_border_size, want_bicubic=want_bicubic)[:2]

    def _evaluation_inputs(self, file_path):
        """(true image aligned, true Y or grey, LR input, bicubic of LR) -- DCSCN.py:674-683."""
        true_image = util.set_image_alignment(util.load_image(file_path, print_console=False), self.scale)
        if true_image.shape[2] == 3 and self.channels == 1:
            input_image = build_input_image(true_image, channels=self.channels, scale=self.scale,
                                            alignment=self.scale, convert_ycbcr=True)
            true_y = util.convert_rgb_to_y(true_image)
        elif true_image.shape[2] == 1 and self.channels == 1:
            input_image = build_input_image(true_image, channels=self.channels, scale=self.scale, alignment=self.scale)
            true_y = true_image
        else:
            return true_image, None, None, None
        bicubic = self._resize_bytes(input_image, self.scale)              # uint8 for grey files; the float Y goes through Pillow
        return true_image, true_y, input_image, bicubic

    def do_for_evaluate(self, file_path, print_console=False):
        """(psnr, ssim) of one file (DCSCN.py:672-703)."""
        true_image = util.set_image_alignment(util.load_image(file_path, print_console=False), self.scale)
        if self._device_colour_path(true_image) and self.device_metrics:
            psnr, ssim = self._evaluate_rgb_metrics(true_image, self.self_ensemble)[0]     # ... and the metrics: nothing comes back but them
        else:
            if self._device_colour_path(true_image):
                # one upload: Y conversion, both bicubic resizes, the (ensemble of) forward pass on the device (dcscn_evaluate_rgb)
                true_y, output = self._ready_engine().evaluate_rgb(true_image, self.self_ensemble)
            else:
                true_image, true_y, input_image, bicubic = self._evaluation_inputs(file_path)
                if true_y is None:
                    return None, None
                output = self.do(input_image, bicubic)
                if output is None:
                    return 0.0, 0.0                           # split ensemble, not rank 0: the values are rank 0's (evaluate.py logs there)
            psnr, ssim = self._metrics(true_y, output)
        if print_console:
            print("[%s] PSNR:%f, SSIM:%f" % (file_path, psnr, ssim))
        return psnr, ssim

    def do_for_evaluate_many(self, file_paths, print_console=False):
        """[(psnr, ssim, seconds)] of do_for_evaluate over the files, in order, as a three-stage pipeline: the
        reference's loop (evaluate.py:89-107) is decode -> network -> PSNR / SSIM, strictly serial, and on this path the device is
        ~5 % of an image's time (profiles/r03_c4_eval_profile.txt).  Here the PNG decode of the NEXT files runs on one worker thread,
        the metric code (utilty.py:509-536, numpy / scipy: it releases the GIL) of the PREVIOUS ones on two more, and this thread
        alone drives the engine (the handle is not thread safe) in file order.  Every value is computed by the same functions on
        the same data as in do_for_evaluate: the results are identical.  `seconds` = wall clock of the whole call / number of files
        (what a caller waits per file; the reference's figure is the serial time of each file).
        With device_metrics the metric stage is part of the device stage and its two threads are not started."""
        import time
        from concurrent.futures import ThreadPoolExecutor
        from contextlib import nullcontext
        n = len(file_paths)
        if n == 0:
            return []
        t0 = time.time()

        def decode(path):
            return util.set_image_alignment(util.load_image(path, print_console=False), self.scale)

        class _Done:                                          # a value already computed, with a future's result()
            def __init__(self, value):
                self.value = value

            def result(self):
                return self.value

        def metrics(true_y, output):
            if self.device_metrics:                           # on this thread: the engine computes them (the handle is not thread safe)
                return _Done(self._metrics(true_y, output))
            return met.submit(self._metrics, true_y, output)

        with ThreadPoolExecutor(max_workers=1) as dec, (nullcontext() if self.device_metrics else ThreadPoolExecutor(max_workers=2)) as met:
            ahead = 2
            pending = {i: dec.submit(decode, file_paths[i]) for i in range(min(ahead, n))}
            results = []
            for i in range(n):
                true_image = pending.pop(i).result()
                if i + ahead < n:
                    pending[i + ahead] = dec.submit(decode, file_paths[i + ahead])
                if self._device_colour_path(true_image) and self.device_metrics:
                    results.append(_Done(self._evaluate_rgb_metrics(true_image, self.self_ensemble)[0]))
                    continue
                if self._device_colour_path(true_image):
                    true_y, output = self._ready_engine().evaluate_rgb(true_image, self.self_ensemble)
                else:
                    true_image, true_y, input_image, bicubic = self._evaluation_inputs(file_paths[i])
                    output = None if true_y is None else self.do(input_image, bicubic)
                results.append(None if true_y is None else metrics(true_y, output))
            values = [(None, None) if r is None else r.result() for r in results]
        per_file = (time.time() - t0) / n
        if print_console:
            for path, (psnr, ssim) in zip(file_paths, values):
                print("[%s] PSNR:%s, SSIM:%s" % (path, psnr, ssim))
        return [(psnr, ssim, per_file) for psnr, ssim in values]

    @util.with_deferred_saves
    def do_for_evaluate_with_output(self, file_path, output_directory, print_console=False):
        """As above, also writing the result images (DCSCN.py:616-670)."""
        filename, extension = os.path.splitext(file_path)
        output_directory += "/" + self.name + "/"
        util.make_dir(output_directory)

        true_image = util.set_image_alignment(util.load_image(file_path, print_console=False), self.scale)
        input_image = self._resize_bytes(true_image, 1.0 / self.scale)
        input_bicubic_image = self._resize_bytes(input_image, self.scale)
        util.save_image(output_directory + filename + "_input_bicubic" + extension, input_bicubic_image)

        if true_image.shape[2] == 3 and self.channels == 1:
            input_y_image = build_input_image(true_image, channels=self.channels, scale=self.scale,
                                              alignment=self.scale, convert_ycbcr=True)
            input_bicubic_y_image = util.resize_image_by_pil(input_y_image, self.scale,
                                                             resampling_method=self.resampling_method)
            true_ycbcr_image = util.convert_rgb_to_ycbcr(true_image)
            output_y_image = self.do(input_y_image, input_bicubic_y_image)
            psnr, ssim = self._metrics(true_ycbcr_image[:, :, 0:1], output_y_image)
            loss_image = util.get_loss_image(true_ycbcr_image[:, :, 0:1], output_y_image,
                                             border_size=self.psnr_calc_border_size)
            output_color_image = util.convert_y_and_cbcr_to_rgb(output_y_image, true_ycbcr_image[:, :, 1:3])
            util.save_image(output_directory + file_path, true_image)
            util.save_image(output_directory + filename + "_input" + extension, input_y_image)
            util.save_image(output_directory + filename + "_input_bicubic_y" + extension, input_bicubic_y_image)
            util.save_image(output_directory + filename + "_true_y" + extension, true_ycbcr_image[:, :, 0:1])
            util.save_image(output_directory + filename + "_result" + extension, output_y_image)
            util.save_image(output_directory + filename + "_result_c" + extension, output_color_image)
            util.save_image(output_directory + filename + "_loss" + extension, loss_image)
        elif true_image.shape[2] == 1 and self.channels == 1:
            input_image = build_input_image(true_image, channels=self.channels, scale=self.scale, alignment=self.scale)
            input_bicubic_y_image = self._resize_bytes(input_image, self.scale)
            output_image = self.do(input_image, input_bicubic_y_image)
            psnr, ssim = self._metrics(true_image, output_image)
            util.save_image(output_directory + file_path, true_image)
            util.save_image(output_directory + filename + "_result" + extension, output_image)
        else:
            return None, None

        if print_console:
            print("[%s] PSNR:%f, SSIM:%f" % (filename, psnr, ssim))
        return psnr, ssim

    def evaluate_bicubic(self, file_path, print_console=False):
        """PSNR / SSIM of plain bicubic upscaling (DCSCN.py:705-725)."""
        true_image = util.set_image_alignment(util.load_image(file_path, print_console=False), self.scale) if self.device_metrics else None
        if true_image is not None and self._device_colour_path(true_image):
            # the pipeline's own bicubic of LR against its true Y (one forward pass of ensemble 1 rides along)
            psnr, ssim = self._evaluate_rgb_metrics(true_image, 1, want_bicubic=True)[1]
        else:
            true_image, true_y, input_image, bicubic = self._evaluation_inputs(file_path)
            if true_y is None:
                return None, None
            psnr, ssim = self._metrics(true_y, bicubic)
        if print_console:
            print("PSNR:%f, SSIM:%f" % (psnr, ssim))
        return psnr, ssim

    def evaluate(self, test_filenames):
        """Mean (psnr, ssim) over files (DCSCN.py:534-545)."""
        if len(test_filenames) == 0:
            return 0, 0
        total_psnr = total_ssim = 0
        for filename in test_filenames:
            psnr, ssim = self.do_for_evaluate(filename, print_console=False)
            total_psnr += psnr
            total_ssim += ssim
        return total_psnr / len(test_filenames), total_ssim / len(test_filenames)
