"""Option "train_split16", host side (no GPU): the cases of tests/train_split16_cases.py, old and new, reach every branch class of
tconv_gemm_h and of the exponent reduction (csrc/train_h.hip), so that a later edit of the cases cannot silently drop one.

The training plan's layout is restated from dcscn_oracle.build_topology as build_train_plan and carve (csrc/train.hip) lay it out: a
concat is one buffer whose stride is the sum of its sources' channels, every source a slice at its running offset; every other
activation has a buffer of its own; dz is dense with stride cout; every buffer starts on a 256-byte boundary, so a slice is 16-byte
aligned exactly where its offset is a multiple of 4 floats."""
import numpy as np

import train_split16_cases as C


def plan(cfg, n, h, w):
    """One dict per eligible conv and direction: in_stride, in_off (floats), K, N, P (pixels at the layer's resolution), hw (pixels
    of one image), and the element counts of the tensors whose exponent the step reduces (the input slice or dz, and the filter)."""
    import dcscn_oracle as O
    ops = O.build_topology(cfg)
    convs = {op["dst"]: op for op in ops if op["op"] == "conv"}
    where = {}                                                      # tensor name -> (buffer stride, offset)
    for op in ops:
        if op["op"] == "concat":
            stride, off = sum(convs[s]["cout"] for s in op["srcs"]), 0
            where[op["dst"]] = (stride, 0)
            for s in op["srcs"]:
                where[s] = (stride, off)
                off += convs[s]["cout"]
    res, r = {"x": 1}, 1
    out = []
    for op in ops:
        if op["op"] == "depth_to_space":
            r = res[op["src"]] * op["block"]
            res[op["dst"]] = r
            where[op["dst"]] = (convs[op["src"]]["cout"] // op["block"] ** 2, 0)
        elif op["op"] == "concat":
            res[op["dst"]] = res[op["srcs"][0]]
        elif op["op"] == "conv":
            res[op["dst"]] = res[op["src"]]
            where.setdefault(op["dst"], (op["cout"], 0))
            cin, cout = op["cin"], op["cout"]
            if op["src"] == "x" or not C.eligible(cin, cout):
                continue
            stride, off = where[op["src"]]
            hw = h * w * res[op["src"]] ** 2
            common = dict(layer=op["var"], P=n * hw, hw=hw, filter_count=op["k"] ** 2 * cin * cout)
            out.append(dict(common, direction="forward", in_stride=stride, in_off=off, K=cin, N=cout, count=n * hw * cin))
            out.append(dict(common, direction="dgrad", in_stride=cout, in_off=0, K=cout, N=cin, count=n * hw * cout))
    return out


def classes(c):
    """The branch classes of one conv launch and its two reductions."""
    got = set()
    vec = c["in_stride"] % 4 == 0 and c["in_off"] % 4 == 0          # tconv_gemm_h's `vec`
    if not vec:
        got.add("load: by element")
    else:
        got.add("load: 16 bytes at offset 0" if c["in_off"] == 0 else "load: 16 bytes at a non-zero offset")
        if c["K"] % 8:
            got.add("load: aligned with a ragged last group of 8")
    K, N, P = c["K"], c["N"], c["P"]
    got.add("K: below 32" if K < 32 else "K: a multiple of 32" if K % 32 == 0 else "K: ragged over several chunks")
    if N < 64 and N % 16:
        got.add("N: below 64 with a ragged 16-tile")
    if N == 64:
        got.add("N: 64")
    if N > 64 and N % 64:
        got.add("N: above 64 with a ragged last group")
    if P < 128:
        got.add("P: below 128")
    elif P % 128 == 0:
        got.add("P: a multiple of 128")
    else:
        got.add("P: a ragged last block")
    first = np.arange(0, P, 128)
    if np.any(first // c["hw"] != np.minimum(first + 127, P - 1) // c["hw"]):
        got.add("P: a block that spans two images")
    for count in (c["count"], c["filter_count"]):
        blocks, _ = C.texp_partition(count)
        got.add("reduction: 1 block" if blocks == 1 else "reduction: clamped" if count > C.ABS_MAX_BLOCKS * C.ABS_MAX_CHUNK
                else "reduction: several blocks")
    return got


EVERY_CLASS = {
    "load: by element", "load: 16 bytes at offset 0", "load: 16 bytes at a non-zero offset", "load: aligned with a ragged last group of 8",
    "K: below 32", "K: a multiple of 32", "K: ragged over several chunks",
    "N: below 64 with a ragged 16-tile", "N: 64", "N: above 64 with a ragged last group",
    "P: below 128", "P: a multiple of 128", "P: a ragged last block", "P: a block that spans two images",
    "reduction: 1 block", "reduction: several blocks", "reduction: clamped",
}


def _all_cases(oracle):
    shapes = [(name, over, nhw) for name, (over, _, nhw, _, _) in C.CASES.items()]
    shapes += [(name, over, nhw) for name, (over, nhw) in C.EDGE_SHAPES.items()]
    return [(name, oracle.make_config(**over), nhw) for name, over, nhw in shapes]


def test_the_cases_reach_every_branch_class(oracle):
    seen = {}
    for name, cfg, nhw in _all_cases(oracle):
        for c in plan(cfg, *nhw):
            for k in classes(c):
                seen.setdefault(k, "%s %s %s" % (name, c["layer"], c["direction"]))
    for k in sorted(seen):
        print("%-46s %s" % (k, seen[k]))
    assert set(seen) == EVERY_CLASS, sorted(EVERY_CLASS - set(seen))


def test_the_plan_of_the_aligned_net_is_what_the_edge_tests_say(oracle):
    """The branch points the ALIGNED net was chosen for, from the restated layout."""
    convs = {(c["layer"], c["direction"]): c for c in plan(oracle.make_config(**C.ALIGNED), 1, 72, 71)}
    fwd = lambda v: convs[(v, "forward")]
    assert (fwd("CNN3")["in_stride"], fwd("CNN3")["in_off"], fwd("CNN3")["K"]) == (104, 48, 32)
    assert (fwd("A1")["K"], fwd("B1")["K"], fwd("A1")["in_off"]) == (104, 104, 0)
    assert (fwd("Up-PS/Up-PS_CNN")["in_stride"], fwd("Up-PS/Up-PS_CNN")["K"], fwd("Up-PS/Up-PS_CNN")["N"]) == (48, 48, 64)
    count = fwd("A1")["count"]
    blocks, chunk = C.texp_partition(count)
    assert count > C.ABS_MAX_BLOCKS * C.ABS_MAX_CHUNK and blocks == C.ABS_MAX_BLOCKS
    assert chunk > C.ABS_MAX_CHUNK and chunk % 256 and chunk % 104
    one_row = {(c["layer"], c["direction"]): c for c in plan(oracle.make_config(**C.ALIGNED), 1, 1, 5112)}
    assert one_row[("A1", "forward")]["count"] == count


def test_the_reduction_partition_and_exponent_restatements():
    """texp_partition and split16_exponent on the values the kernel's comments name."""
    assert C.texp_partition(1) == (1, 1) and C.texp_partition(2048) == (1, 2048) and C.texp_partition(2049) == (2, 1025)
    assert C.texp_partition(9 * 40 * 26) == (5, 1872) and C.texp_partition(9 * 17 * 17) == (2, 1301)
    assert C.texp_partition(256 * 2048) == (256, 2048) and C.texp_partition(256 * 2048 + 1) == (256, 2049)
    for count in (1, 7, 2047, 2049, 12750, 524287, 531648):          # the blocks cover the tensor and none starts past its end
        blocks, chunk = C.texp_partition(count)
        assert (blocks - 1) * chunk < count <= blocks * chunk
    e = C.split16_exponent
    assert e(0.0) == 0 and e(1.0) == 13 and e(8192.0) == 0 and e(16383.0) == 0 and e(16384.0) == -1 and e(255.0) == 6
    assert e(2.0 ** -130) == 126 and e(2.0 ** -113) == 126 and e(2.0 ** -112) == 125 and e(np.float32(3e38)) == -114
    for top in (1e-30, 3e-5, 0.7, 255.0, 5e4, 1e20):                # the scaled maximum lies in [2^13, 2^14)
        assert 2.0 ** 13 <= float(np.float32(top)) * 2.0 ** e(top) < 2.0 ** 14


def _exponents(cfg, weights, x, x2, y):
    """(e_w, e_in, e_dz) of B1 and B2, {layer: exponent} each, as texp_final computes them, from the float64 activations; and the
    float64 gradients."""
    import train_ref as R
    taps = {k: None for k in ("CNN1", "CNN2", "CNN3", "B1", "B2")}
    _, g64 = R.loss_and_grads(cfg, weights, x, x2, y, keep=C.EDGE_KEEP, key=C.KEY, taps=taps)
    top = lambda a: float(np.max(np.abs(a)))
    e = C.split16_exponent
    concat = max(top(taps[k]["out"]) for k in ("CNN1", "CNN2", "CNN3"))
    e_w = {k: e(top(weights[k + "/conv_W"])) for k in ("B1", "B2")}
    e_in = {"B1": e(concat), "B2": e(top(taps["B1"]["out"]))}
    e_dz = {k: e(top(taps[k]["dz"])) for k in ("B1", "B2")}
    return e_w, e_in, e_dz, g64


def test_the_rebalancing_reaches_the_exponents_it_is_there_for():
    """In float64 on the CPU: the sweep has negative exponents, exponents past 80 and |e_in + e_w| past 126, every gradient stays a
    normal float32, and the float64 gradients follow the symmetry."""
    cfg, weights, x, x2, y = C.edge_inputs("odd-2x7x9")
    _, _, _, g0 = _exponents(cfg, weights, x, x2, y)
    lowest, highest, widest = 0, 0, 0
    for k in C.REBALANCE:
        moved = C.rebalanced(weights, k)
        assert all(np.all(np.isfinite(v)) and np.all((np.abs(v) >= 2.0 ** -126) | (v == 0)) for v in moved.values())
        e_w, e_in, e_dz, g = _exponents(cfg, moved, x, x2, y)
        sums = [e_w[l] + e_in[l] for l in e_w] + [e_w[l] + e_dz[l] for l in e_w]
        print("k %4d: e_w %r e_in %r e_dz %r, e_in + e_w and e_dz + e_w %r" % (k, e_w, e_in, e_dz, sums))
        lowest = min([lowest] + list(e_w.values()) + list(e_in.values()) + list(e_dz.values()))
        highest = max([highest] + list(e_w.values()) + list(e_in.values()) + list(e_dz.values()))
        widest = max([widest] + [abs(s) for s in sums])
        for name, v in g.items():
            top = float(np.max(np.abs(v)))
            assert 1e-30 < top < 1e30, (k, name, top)
        back = C.undo_rebalancing(g, k)
        for name in g:
            np.testing.assert_allclose(back[name], g0[name], rtol=1e-9, atol=1e-12 * float(np.max(np.abs(g0[name]))), err_msg="%d %s" % (k, name))
    assert lowest <= -50 and highest >= 100 and 126 < widest <= 252, (lowest, highest, widest)


def test_the_outliers_sit_where_the_edge_tests_say():
    """The largest magnitude of A1's input slice (outlier in x) and of A1's dz (outlier in y_true) lies in the first, respectively the last,
    block of the reduction, on the one-row shapes the GPU tests run."""
    for name, places in (("odd-1x1x150", ("x-first", "x-last", "y-first", "y-last")), ("aligned-1x1x5112", ("x-last",))):
        cfg, weights, x, x2, y = C.edge_inputs(name)
        for where in places:
            got = C.blocks_of_the_maxima(cfg, weights, *C.pixel_outlier(x, x2, y, where), C.EDGE_KEEP, C.KEY)
            block, blocks = got[0] if where[0] == "x" else got[1]
            print("%s %s: block %d of %d" % (name, where, block, blocks))
            assert blocks > 1 and block == (0 if where.endswith("first") else blocks - 1), (name, where, got)
    for layer, count in (("CNN2", 9 * 40 * 26), ("B2", 9 * 17 * 17)):
        blocks, chunk = C.texp_partition(count)
        pos = C.filter_positions(count)
        assert pos["chunk-end"] // chunk == 0 and pos["chunk-start"] // chunk == 1 and pos["last"] // chunk == blocks - 1
