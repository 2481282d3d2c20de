"""The float64 restatement of separable training (tests/train_ref_separable.py) checked on the CPU: its forward against the oracle's, its
gradients against finite differences, and the margin between torch float32 and the GPU file's bar on every case that file compares."""
import numpy as np
import pytest
import torch

import train_ref_separable as S


@pytest.mark.parametrize("name", sorted(S.NETS))
def test_the_restated_forward_is_the_oracles(oracle, name):
    cfg = S.net(name)
    weights = oracle.synthetic_weights(cfg, seed=0)
    x, x2, _ = S.batch(cfg, 2, 9, 11, 1)
    leaves = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in weights.items()}
    got = S.forward(cfg, leaves, x, x2).permute(0, 2, 3, 1).numpy()
    want = oracle.forward(cfg, weights, x, x2, dtype=np.float64)
    # the same float64 products summed in another order: a few ulps of the largest output
    assert np.max(np.abs(got - want)) <= 1e-11 * np.max(np.abs(want))
    kinds = {k.rsplit("/", 1)[-1] for k in weights}
    assert {"depthwise_W", "pointwise_W", "conv_B"} <= kinds and ("conv_W" in kinds) == (name == "c")


@pytest.mark.parametrize("name", sorted(S.NETS))
def test_gradients_pass_a_finite_difference_probe(oracle, name):
    """Central differences of the float64 loss (dropout on, l2 term on) at three elements of one tensor of every kind.  The step 1e-6 keeps
    the rounding of the difference (about 2.2e-16 * loss / step, loss of a few hundred: 1e-7) and the cubic term far below the bound; what
    is left is a unit that crosses its activator's kink inside the step, which changes the slope of at most that unit's share of the
    gradient.  The bound is 1e-3 of the tensor's largest gradient value plus 1e-6."""
    cfg = S.net(name)
    weights = oracle.synthetic_weights(cfg, seed=0)
    x, x2, y = S.batch(cfg, 2, 7, 9, 1)
    _, grads = S.loss_and_grads(cfg, weights, x, x2, y, keep=0.8, key=S.KEY, l2_decay=S.L2_DECAY)
    rng = np.random.default_rng(0)
    seen = set()
    for tensor in sorted(weights):
        kind = tensor.rsplit("/", 1)[-1]
        kind = "prelu" if kind.endswith("_prelu") else kind
        if kind in seen or tensor.startswith("CNN1/"):           # (one tensor per kind, past the first layer so that data gradients count)
            continue
        seen.add(kind)
        g = grads[tensor]
        for flat in rng.choice(g.size, min(3, g.size), replace=False):
            idx = np.unravel_index(flat, g.shape)
            values = []
            for sign in (1.0, -1.0):
                w = {k: np.asarray(v, np.float64).copy() for k, v in weights.items()}
                w[tensor][idx] += sign * 1e-6
                leaves = {k: torch.tensor(v) for k, v in w.items()}
                values.append(S.loss(cfg, leaves, x, x2, y, keep=0.8, key=S.KEY, l2_decay=S.L2_DECAY)[0].item())
            fd = (values[0] - values[1]) / 2e-6
            assert abs(fd - g[idx]) <= 1e-3 * np.max(np.abs(g)) + 1e-6, (tensor, idx, fd, g[idx])
    assert seen >= {"depthwise_W", "pointwise_W", "conv_B"}


@pytest.mark.parametrize("case", S.MAIN_CASES + S.EDGE_CASES, ids=lambda c: "%s-n%d-%dx%d-s%d-k%g-l1%d" % c)
def test_float32_is_well_inside_the_gpu_bar_and_no_gradient_vanishes(case):
    cfg, weights, x, x2, y = S.case_inputs(case)
    _, g64 = S.reference(case)
    _, g32 = S.loss_and_grads(cfg, {k: v.astype(np.float32) for k, v in weights.items()}, x, x2, y, keep=case[5], key=S.KEY, l1=case[6],
                              l2_decay=S.L2_DECAY, dtype=torch.float32)
    for k, g in g64.items():
        top = float(np.max(np.abs(g)))
        err = float(np.max(np.abs(g32[k] - g)))
        print("%-40s max |g64| %.3g  float32 err / max %.3g" % (k, top, err / top if top else float("nan")))
        assert top > 0.0, k
        assert err <= 2e-5 * top, (k, err, top)


def test_the_edge_batch_divides_no_depthwise_split():
    """23 x 29 pixels of net b: every separable layer's depthwise split has a ragged last part, at LR and at HR."""
    cfg = S.net("b")
    import dcscn_oracle as O
    res, seen = 1, 0
    for op in O.build_topology(cfg):
        if op["op"] == "depth_to_space":
            res *= op["block"]
        if op["op"] == "conv" and op["ds"]:
            pixels = 23 * 29 * res * res
            splits, chunk = S.dw_splits(op["cin"], pixels)
            if splits > 1:
                assert splits * chunk != pixels, (op["name"], splits, chunk)
                seen += 1
    assert seen >= 5
