"""Generates tests/golden/ref_summary_tags.json: the TensorBoard tags of the reference's six shipped training graphs.

Every ``models/*.ckpt.meta`` of the reference is the MetaGraphDef tf.train.Saver wrote next to a checkpoint of a model trained with
``--save_weights``: its graph holds one ``ScalarSummary`` node per tf.summary.scalar and one ``HistogramSummary`` node per
tf.summary.histogram (helper/utilty.py add_summaries), and the tag of each is the string constant on the node's first input.  This
script lists those constants per model -- names only, no graph, no weights -- with a protobuf wire-format walker (no TensorFlow):

    MetaGraphDef.graph_def = 2;  GraphDef.node = 1;  NodeDef{name = 1, op = 2, input = 3, attr = 5 (map entry: key = 1, value = 2)}
    AttrValue.tensor = 8;  TensorProto.string_val = 8

tests/test_summary_host.py checks the tag rules of dcscn-super-resolution_amd/events.py against the file.

    python tests/golden/make_ref_summary_tags.py [<reference tree>/models]
"""
import json
import os
import sys


def varint(buf, pos):
    value = shift = 0
    while True:
        byte = buf[pos]
        pos += 1
        value |= (byte & 0x7F) << shift
        if byte < 0x80:
            return value, pos
        shift += 7


def fields(buf):
    """(field number, wire type, payload) of every field of one message."""
    pos = 0
    while pos < len(buf):
        key, pos = varint(buf, pos)
        wire = key & 7
        if wire == 0:
            payload, pos = varint(buf, pos)
        elif wire == 2:
            size, pos = varint(buf, pos)
            payload = buf[pos:pos + size]
            pos += size
        elif wire in (1, 5):
            size = 8 if wire == 1 else 4
            payload = buf[pos:pos + size]
            pos += size
        else:
            raise ValueError("unsupported wire type %d" % wire)
        yield key >> 3, wire, payload


def first(buf, number):
    for f, _, payload in fields(buf):
        if f == number:
            return payload
    return None


def nodes_of(meta_path):
    with open(meta_path, "rb") as f:
        graph = first(f.read(), 2)
    nodes = {}
    for f, _, node in fields(graph):
        if f != 1:
            continue
        name = op = None
        inputs, strings = [], None
        for f2, _, v in fields(node):
            if f2 == 1:
                name = v.decode()
            elif f2 == 2:
                op = v.decode()
            elif f2 == 3:
                inputs.append(v.decode())
            elif f2 == 5 and first(v, 1) == b"value":
                tensor = first(first(v, 2), 8)
                if tensor is not None:
                    strings = [s.decode() for f3, w3, s in fields(tensor) if f3 == 8 and w3 == 2]
        nodes[name] = (op, inputs, strings)
    return nodes


def summary_tags(meta_path):
    nodes = nodes_of(meta_path)
    out = {"scalar": [], "histogram": []}
    for name, (op, inputs, _) in nodes.items():
        kind = {"ScalarSummary": "scalar", "HistogramSummary": "histogram"}.get(op)
        if kind is None:
            continue
        tags = nodes[inputs[0].split(":")[0]][2]
        assert tags and len(tags) == 1, (name, tags)
        out[kind].append(tags[0])
    return {k: sorted(v) for k, v in out.items()}


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    models = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "models")
    doc = {"source": "jiny2001/dcscn-super-resolution models/*.ckpt.meta: tag constants of the ScalarSummary / HistogramSummary nodes "
                     "(tests/golden/make_ref_summary_tags.py, no TensorFlow)", "models": {}}
    for fn in sorted(os.listdir(models)):
        if fn.endswith(".ckpt.meta"):
            doc["models"][fn[:-len(".ckpt.meta")]] = summary_tags(os.path.join(models, fn))
    out = os.path.join(here, "ref_summary_tags.json")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print("wrote", out, "with", len(doc["models"]), "models")


if __name__ == "__main__":
    main()
