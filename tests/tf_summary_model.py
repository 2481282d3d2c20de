"""A numpy restatement of the summary records (include/dcscn.h: "TensorBoard summaries") and an independent reader of TensorBoard event
files, for the tests of csrc/summary.hip and dcscn-super-resolution_amd/events.py.  Nothing here imports the code under test.

The bucket limits, the proto field numbers and the record framing restate TensorFlow's histogram.cc, summary.proto / event.proto and
record_writer.cc from memory; no TensorFlow is at hand to confirm them.  What the tests pin is that the device, the
library's host table, events.py and this file agree exactly, and that a written file is well formed.
"""
import math
import struct
import sys

import numpy as np

DBL_MAX = sys.float_info.max


def bucket_limits():
    pos = []
    v = 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    return np.array([-DBL_MAX] + [-p for p in reversed(pos)] + [0.0] + pos + [DBL_MAX], np.float64)


LIMITS = bucket_limits()


def summarize(values):
    """The record of a float32 array: dict of num, nonfinite, min, max, sum, sum_squares, mean, stddev, buckets (int64 [len(LIMITS)])."""
    v = np.asarray(values, np.float32).ravel()
    finite = np.isfinite(v)
    d = v[finite].astype(np.float64)
    num = int(d.size)
    rec = {"num": num, "nonfinite": int(v.size - num)}
    if num == 0:
        rec.update(min=0.0, max=0.0, sum=0.0, sum_squares=0.0, mean=0.0, stddev=0.0, abs_sum=0.0)
    else:
        s = math.fsum(d)
        mean = s / num
        rec.update(min=float(d.min()), max=float(d.max()), sum=s, sum_squares=math.fsum(d * d), mean=mean,
                   stddev=math.sqrt(math.fsum((d - mean) ** 2) / num), abs_sum=math.fsum(np.abs(d)))
    rec["buckets"] = np.bincount(np.searchsorted(LIMITS, d, side="right"), minlength=LIMITS.size).astype(np.int64)
    assert rec["buckets"].size == LIMITS.size
    return rec


def collapse(buckets, limits=LIMITS):
    """HistogramProto's (bucket_limit, bucket) lists as TensorFlow's Histogram::EncodeToProto writes them: a run of empty buckets becomes
    one entry that carries the run's LAST limit; the last bucket always ends a run."""
    out_limits, out_counts = [], []
    i, n = 0, len(buckets)
    while i < n:
        end = limits[i]
        count = buckets[i]
        i += 1
        if count <= 0:
            while i < n and buckets[i] <= 0:
                end = limits[i]
                count = buckets[i]
                i += 1
        out_limits.append(float(end))
        out_counts.append(float(count))
    return out_limits, out_counts


# ---- crc32c (Castagnoli), bit by bit: independent of events.py's table ----
def crc32c(data):
    crc = 0xFFFFFFFF
    for b in bytes(data):
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ (0x82F63B78 if crc & 1 else 0)
    return crc ^ 0xFFFFFFFF


def masked_crc32c(data):
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


# ---- protobuf wire format ----
def _varint(buf, pos):
    value = shift = 0
    while True:
        b = buf[pos]
        pos += 1
        value |= (b & 0x7F) << shift
        if b < 0x80:
            return value, pos
        shift += 7


def _fields(buf):
    pos = 0
    while pos < len(buf):
        key, pos = _varint(buf, pos)
        wire = key & 7
        if wire == 0:
            val, pos = _varint(buf, pos)
        elif wire == 1:
            val, pos = buf[pos:pos + 8], pos + 8
        elif wire == 5:
            val, pos = buf[pos:pos + 4], pos + 4
        elif wire == 2:
            n, pos = _varint(buf, pos)
            val, pos = buf[pos:pos + n], pos + n
            assert len(val) == n, "truncated field"
        else:
            raise ValueError("wire type %d" % wire)
        yield key >> 3, wire, val


def _doubles(buf):
    return list(struct.unpack("<%dd" % (len(buf) // 8), buf))


def parse_histogram(buf):
    h = {"bucket_limit": [], "bucket": []}
    names = {1: "min", 2: "max", 3: "num", 4: "sum", 5: "sum_squares"}
    for f, wire, val in _fields(buf):
        if f in names:
            assert wire == 1
            h[names[f]] = struct.unpack("<d", val)[0]
        elif f in (6, 7):
            assert wire == 2, "bucket lists are packed"
            h["bucket_limit" if f == 6 else "bucket"] += _doubles(val)
    return h


def parse_event(buf):
    """{"wall_time", "step", "file_version", "values": [{"tag", "simple_value" | "histo"}]}"""
    ev = {"step": 0, "values": []}
    for f, wire, val in _fields(buf):
        if f == 1:
            ev["wall_time"] = struct.unpack("<d", val)[0]
        elif f == 2:
            ev["step"] = val
        elif f == 3:
            ev["file_version"] = val.decode()
        elif f == 5:
            for f2, _, v2 in _fields(val):
                if f2 != 1:
                    continue
                value = {}
                for f3, w3, v3 in _fields(v2):
                    if f3 == 1:
                        value["tag"] = v3.decode()
                    elif f3 == 2:
                        assert w3 == 5
                        value["simple_value"] = struct.unpack("<f", v3)[0]
                    elif f3 == 5:
                        value["histo"] = parse_histogram(v3)
                ev["values"].append(value)
    return ev


def read_events(path):
    """Every record of a TFRecord event file, both CRCs of each verified, parsed as Events."""
    with open(path, "rb") as f:
        buf = f.read()
    events, pos = [], 0
    while pos < len(buf):
        header = buf[pos:pos + 8]
        assert len(header) == 8, "truncated length"
        (length,) = struct.unpack("<Q", header)
        (crc,) = struct.unpack("<I", buf[pos + 8:pos + 12])
        assert crc == masked_crc32c(header), "length crc of the record at %d" % pos
        data = buf[pos + 12:pos + 12 + length]
        assert len(data) == length, "truncated record"
        (crc,) = struct.unpack("<I", buf[pos + 12 + length:pos + 16 + length])
        assert crc == masked_crc32c(data), "data crc of the record at %d" % pos
        events.append(parse_event(data))
        pos += 16 + length
    return events


def check_record(got, want, exact_stddev_zero=False):
    """The bars of the issue: counts, min, max, num, nonfinite exact; sum and sum_squares within 1e-12 of fsum(|v|) resp. fsum(v^2);
    mean and stddev within 1e-10 relative; double against double."""
    assert got["num"] == want["num"] and got["nonfinite"] == want["nonfinite"], (got["num"], got["nonfinite"], want["num"], want["nonfinite"])
    assert got["min"] == want["min"] and got["max"] == want["max"], (got["min"], got["max"], want["min"], want["max"])
    assert np.array_equal(np.asarray(got["buckets"]), want["buckets"]), np.flatnonzero(np.asarray(got["buckets"]) != want["buckets"])[:8]
    assert abs(got["sum"] - want["sum"]) <= 1e-12 * want["abs_sum"], (got["sum"], want["sum"])
    assert abs(got["sum_squares"] - want["sum_squares"]) <= 1e-12 * want["sum_squares"], (got["sum_squares"], want["sum_squares"])
    assert abs(got["mean"] - want["mean"]) <= 1e-10 * abs(want["mean"]), (got["mean"], want["mean"])
    assert abs(got["stddev"] - want["stddev"]) <= 1e-10 * abs(want["stddev"]), (got["stddev"], want["stddev"])
    if exact_stddev_zero:
        assert got["stddev"] == 0.0
