"""TensorBoard event files without TensorFlow: the writer behind ``SuperResolution.log_to_tensorboard`` and the rules that name the
reference's summaries.

File format (TensorFlow's record_writer.cc / event.proto / summary.proto, restated from memory -- DESIGN.md 7.1 says what that means):

* a TFRecord stream: per record ``u64 length`` (little endian), ``u32 masked_crc32c(length bytes)``, the data, ``u32 masked_crc32c(data)``
  with ``mask(c) = ((c >> 15 | c << 17) + 0xa282ead8) mod 2^32`` over CRC-32C (Castagnoli);
* every record is an ``Event``: wall_time = 1 (double), step = 2 (int64), file_version = 3 (string), summary = 5 (Summary);
  the first record of a file carries file_version "brain.Event:2";
* ``Summary``: value = 1 (repeated Value); ``Value``: tag = 1, simple_value = 2 (float), histo = 5 (HistogramProto);
* ``HistogramProto``: min = 1, max = 2, num = 3, sum = 4, sum_squares = 5 (doubles), bucket_limit = 6, bucket = 7 (packed doubles),
  the buckets collapsed as Histogram::EncodeToProto does: a run of empty buckets is one entry with the run's last limit.

The records themselves come from the device (include/dcscn.h "TensorBoard summaries", Engine.train_log_pass / Engine.summary).
"""
import os
import re
import socket
import struct
import time

import numpy as np

# ---- crc32c ----
_CRC_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ (0x82F63B78 if _c & 1 else 0)
    _CRC_TABLE.append(_c)


def crc32c(data):
    crc = 0xFFFFFFFF
    for b in bytes(data):
        crc = _CRC_TABLE[(crc ^ b) & 0xFF] ^ (crc >> 8)
    return crc ^ 0xFFFFFFFF


def masked_crc32c(data):
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def record(data):
    """One TFRecord: length, its crc, the data, its crc."""
    header = struct.pack("<Q", len(data))
    return header + struct.pack("<I", masked_crc32c(header)) + data + struct.pack("<I", masked_crc32c(data))


# ---- protobuf wire format ----
def _varint(value):
    value &= (1 << 64) - 1            # (int64 as two's complement)
    out = bytearray()
    while value >= 0x80:
        out.append((value & 0x7F) | 0x80)
        value >>= 7
    out.append(value)
    return bytes(out)


def _key(field, wire):
    return _varint((field << 3) | wire)


def _double(field, value):
    return _key(field, 1) + struct.pack("<d", value)


def _float(field, value):
    return _key(field, 5) + struct.pack("<f", value)


def _bytes(field, data):
    return _key(field, 2) + _varint(len(data)) + data


def collapse_buckets(buckets, limits):
    """(bucket_limit, bucket) as Histogram::EncodeToProto writes them: a run of empty buckets becomes one entry that carries the
    run's last limit."""
    out_limits, out_counts = [], []
    i, n = 0, len(buckets)
    while i < n:
        end, count = limits[i], buckets[i]
        i += 1
        if count <= 0:
            while i < n and buckets[i] <= 0:
                end, count = limits[i], buckets[i]
                i += 1
        out_limits.append(float(end))
        out_counts.append(float(count))
    return out_limits, out_counts


def encode_histogram(rec, limits):
    """HistogramProto of a summary record (a dict with min, max, num, sum, sum_squares and dense "buckets" over ``limits``)."""
    lim, cnt = collapse_buckets(rec["buckets"], limits)
    return (_double(1, rec["min"]) + _double(2, rec["max"]) + _double(3, float(rec["num"])) + _double(4, rec["sum"]) +
            _double(5, rec["sum_squares"]) + _bytes(6, struct.pack("<%dd" % len(lim), *lim)) + _bytes(7, struct.pack("<%dd" % len(cnt), *cnt)))


def encode_event(wall_time, step=0, values=None, file_version=None, limits=None):
    """An Event.  ``values``: [(tag, float)] for scalars, [(tag, record dict)] for histograms."""
    out = _double(1, wall_time)
    if step:
        out += _key(2, 0) + _varint(int(step))
    if file_version is not None:
        out += _bytes(3, file_version.encode())
    if values is not None:
        summary = b""
        for tag, value in values:
            body = _bytes(1, tag.encode())
            if isinstance(value, dict):
                body += _bytes(5, encode_histogram(value, limits))
            else:
                body += _float(2, float(value))
            summary += _bytes(1, body)
        out += _bytes(5, summary)
    return out


class EventWriter:
    """tf.summary.FileWriter(logdir): ``<logdir>/events.out.tfevents.<unix time>.<hostname>``, begun with the file_version record."""

    def __init__(self, logdir, limits=None, wall_time=None, hostname=None):
        os.makedirs(logdir, exist_ok=True)
        now = time.time() if wall_time is None else wall_time
        self.path = os.path.join(logdir, "events.out.tfevents.%010d.%s" % (int(now), hostname or socket.gethostname()))
        self.limits = limits
        self._file = open(self.path, "ab")
        self._file.write(record(encode_event(now, file_version="brain.Event:2")))
        self._file.flush()

    def add_summary(self, values, step, wall_time=None):
        """One Event at ``step`` holding every (tag, float | record) of ``values``."""
        now = time.time() if wall_time is None else wall_time
        self._file.write(record(encode_event(now, step=step, values=values, limits=self.limits)))

    def add_scalar(self, tag, value, step, wall_time=None):
        """util.log_scalar_value (helper/utilty.py:446-448): an Event of its own."""
        self.add_summary([(tag, value)], step, wall_time)

    def flush(self):
        self._file.flush()

    def close(self):
        if not self._file.closed:
            self._file.close()


# ---- the reference's tags, as rules ---------------------------------------------------------------------------------------
# util.add_summaries(scope, model, var, header, save_stddev, save_mean) (helper/utilty.py:427-443) writes, inside the name scope it is
# called in, the scalars <scope>/<header>mean/<model> and <scope>/<header>stddev/<model> and the histogram <scope>/<header><model>.
# build_conv / build_depthwise_separable_conv call it for "weight", "output" and "bias" in the layer's variable scope, build_activator for
# "prelu_alpha" (histogram only) in <layer>/prelu, build_graph for the input (scope "X", which TensorFlow makes "X_1" because the
# placeholder "x" holds the name case-insensitively) and for y_ (scope "Y_"), and add_optimizer_op for every gradient with the root scope
# and header = the gradient tensor's name + "/", ":" sanitised to "_" by tf.summary.

def _grad_tensor(var):
    """The name TensorFlow gives the gradient of a variable of the graph (without the ":0"), from the op that consumes the variable."""
    scope, leaf = var.rsplit("/", 1)
    short = scope.rsplit("/", 1)[-1]
    if leaf in ("conv_W", "pointwise_W"):      # tf.nn.conv2d(name=<short>_conv); separable_conv2d(name=<short>_conv) ends in a conv of that name
        return "gradients/%s/%s_conv_grad/Conv2DBackpropFilter" % (scope, short)
    if leaf == "depthwise_W":                  # ... and begins with <short>_conv/depthwise
        return "gradients/%s/%s_conv/depthwise_grad/DepthwiseConv2dNativeBackpropFilter" % (scope, short)
    if leaf == "conv_B":                       # tf.add(output, bias, name=<short>_add): the bias is the second input, its gradient Reshape_1
        return "gradients/%s/%s_add_grad/Reshape_1" % (scope, short)
    if leaf == "Tconv_W":                      # tf.nn.conv2d_transpose(name=<scope>) inside the variable scope
        return "gradients/%s/%s_grad/Conv2DBackpropFilter" % (scope, short)
    if scope.endswith("/prelu"):               # tf.multiply(alphas, ...): the first input of Mul
        return "gradients/%s/Mul_grad/Reshape" % scope
    raise ValueError("no gradient naming rule for variable '%s'" % var)


def summary_plan(layers, variables, model_name, l2_decay=0.0, save_weights=True):
    """What one summary Event holds, in graph order: [(kind, tag, source, field)] with kind "scalar" | "histogram", ``source`` a name of
    Engine.summary (or "loss" / "l2_loss" for the two loss scalars) and ``field`` "mean" | "stddev" | None.

    ``layers``: Engine.layers(); ``variables``: the names of Engine.tensor_specs().  The tags follow the reference's current source;
    DESIGN.md 7.1 lists the tags of the shipped graphs that are left out (the separable layers' unused conv_W, the conv_W gradients under
    l2_decay > 0, whose AddN numbering is TensorFlow's, and the statistics of older versions of the reference)."""
    variables = set(variables)
    plan = []

    def add(scope, source, header="", mean=True, stddev=True):
        if mean:
            plan.append(("scalar", "%s%smean/%s" % (scope, header, model_name), source, "mean"))
        if stddev:
            plan.append(("scalar", "%s%sstddev/%s" % (scope, header, model_name), source, "stddev"))
        plan.append(("histogram", "%s%s%s" % (scope, header, model_name), source, None))

    if save_weights:
        add("X_1/output/", "x")
        for layer in layers:
            scope = layer["name"]
            if scope == "Up-TCNN":             # build_transposed_conv adds no summaries
                continue
            short = scope.rsplit("/", 1)[-1]
            alpha = "%s/prelu/%s_prelu" % (scope, short)
            if alpha in variables:
                add(scope + "/prelu/prelu_alpha/", alpha, mean=False, stddev=False)
            if scope + "/conv_W" in variables:     # (a separable layer summarises its UNUSED conv_W, which the library does not hold)
                add(scope + "/weight/", scope + "/conv_W")
            add(scope + "/output/", scope + "/output")
            if scope + "/conv_B" in variables:
                add(scope + "/bias/", scope + "/conv_B")
        add("Y_/output/", "y_")
    if l2_decay > 0:
        plan.append(("scalar", "L2WeightDecayLoss/" + model_name, "l2_loss", None))
    plan.append(("scalar", "Loss/" + model_name, "loss", None))
    if save_weights:
        for layer in layers:                       # tf.trainable_variables(): creation order, layer by layer
            for var in _layer_variables(layer["name"], variables):
                add("", var + "/grad", header=_grad_tensor(var) + "_0/")
    return plan


def _layer_variables(scope, variables):
    short = scope.rsplit("/", 1)[-1]
    order = ["conv_W", "Tconv_W", "conv_B", "depthwise_W", "pointwise_W", "prelu/%s_prelu" % short]
    return [scope + "/" + leaf for leaf in order if scope + "/" + leaf in variables]


# Tags of the reference's shipped graphs (tests/golden/ref_summary_tags.json) that summary_plan does not produce, with the reason
LEFT_OUT = [
    (r"^gradients/AddN(_\d+)?_0/", "the conv_W gradients of a graph built with l2_decay > 0: the sum of the conv's and the l2 term's, an AddN node "
                                   "numbered by TensorFlow's gradient construction order; written under the conv's Conv2DBackpropFilter_0 name instead"),
    (r"^gradients/L2Loss(_\d+)?_grad/", "gradients of the separable layers' unused conv_W (their l2 term alone); the library does not hold those tensors"),
    (r"/mean_abs/", "a statistic of an older version of the reference; its current add_summaries writes mean"),
    (r"^X/output/", "the input's scope in graphs of an older version of the reference; the current source gives X_1"),
]
LEFT_OUT_SEPARABLE = (r"/weight/", "a separable layer summarises its unused conv_W, which the library does not hold")


def left_out_reason(tag, separable=False):
    """Why a tag of the reference's shipped graphs is not written; None: it is."""
    for pattern, reason in LEFT_OUT + ([LEFT_OUT_SEPARABLE] if separable else []):
        if re.search(pattern, tag):
            return reason
    return None
