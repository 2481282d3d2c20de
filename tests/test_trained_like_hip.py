"""The wide inference kernels under weights with the value statistics of the trained checkpoints (tests/trained_like.py), on the
bare branch against ``oracle.forward(..., float64)``.

Every other test that reaches conv3_h, conv3_h8, conv_nin_h, conv5_h, conv_wino2, conv_nin, conv_igemm at k = 5 / 7, conv_cin1 or
conv_cout1 draws PReLU slopes from U(0.05, 0.3), on which a PReLU epilogue written as max(v, a v) or with a clamped slope computes the
same function; tests/test_trained_like_host.py shows that here such an epilogue moves the output by at least 2254 x the bar.

The bar is the rule of tests/bare_branch.py as test_bare_branch_surface_hip._judge applies it: rel <= 5e-6, else within 4 x the
case's own float32 restatement, else a failure that names the worst pixel and the split16 = 0 run of the same case.  Every case
prints a ``TRAINED-LIKE`` line (pytest -s): the device's error, the float32 restatement's, the kernels and the clause that passed;
profiles/r16_trained_like.txt is that output from an MI355X."""
import numpy as np
import pytest

import bare_branch as B
import test_bare_branch_surface_hip as S
import test_hip_parity as P
import train_split16_cases as C
import trained_like as T
from conftest import synthetic_batch

pytestmark = pytest.mark.gpu

_REF = {}           # (net, spread) -> the case with its float64 reference and its float32 restatement's error


def _case(oracle, net, flags, n, hw, spread):
    if (net, spread) not in _REF:
        cfg, weights, x, x2 = T.bare_case(flags, n, hw, spread)
        ref = S._reference(oracle, cfg, weights, x, x2)
        _REF[net, spread] = (cfg, weights, x, x2, ref, B.restatement_error(oracle, cfg, weights, x, x2, ref))
    return _REF[net, spread]


def _judge(oracle, label, y, kernels, ref, r32, cfg, weights, x, x2, options):
    """test_bare_branch_surface_hip._judge, with its tallies left as they were: they speak about that file's cases."""
    cases, reach = len(S._CASES), dict(S._REACH)
    try:
        message = S._judge(oracle, "trained-like", label, y, kernels, ref, cfg, weights, x, x2, options=options)
    finally:
        del S._CASES[cases:]
        S._REACH.update(reach)
    rel = B.rel_error(y, ref) if np.isfinite(y).all() else float("inf")
    clause = "FAILED" if message else "rel <= BAR" if rel <= B.BAR else "rel <= 4 x float32 restatement"
    print("TRAINED-LIKE %s | device %.3g | float32 restatement %.3g | %s | %s" % (label, rel, r32, ",".join(kernels), clause))
    return message


_PLANS = [(net, flags, n, hw, plan) for net, flags, n, hw, plans in T.INFER_CASES for plan in plans]


@pytest.mark.parametrize("spread", T.SPREADS)
@pytest.mark.parametrize("net,flags,n,hw,plan", _PLANS, ids=["%s-%s" % (p[0], p[4][0].replace(" ", "_")) for p in _PLANS])
def test_bare_branch_under_trained_like_weights(oracle, net, flags, n, hw, plan, spread):
    name, options, want = plan
    cfg, weights, x, x2, ref, r32 = _case(oracle, net, flags, n, hw, spread)
    y, kernels = S._forward(cfg, weights, x, x2, options=options)
    for k in want:
        assert k in kernels, (net, name, k, kernels)
    S._finish([_judge(oracle, "%s %dx%dx%d spread %d, plan %s" % (net, n, hw[0], hw[1], spread, name), y, kernels, ref, r32,
                      cfg, weights, x, x2, options)])


def test_the_cases_reach_every_kernel_name(oracle):
    """The launch lists of the cases above (dcscn_op_info_get reports the kernel launch_op obeys) hold every name of
    exec.hip: kernel_name; all of them are within reach of a PReLU net."""
    from dcscn_amd import engine
    reached = {}
    for net, flags, n, hw, (name, options, want) in _PLANS:
        cfg = oracle.make_config(**flags)
        with engine.Engine(cfg, device=0) as eng:
            for key, value in options:
                eng.set_option(key, value)
            eng.load_weights(T.trained_like_weights(cfg, T.BARE_SEED))
            for op in eng.ops():
                reached.setdefault(op["kernel"], "%s, plan %s" % (net, name))
    for k in S.KERNEL_NAMES:
        print("REACH %-16s %s" % (k, reached.get(k)))
    assert set(reached) == set(S.KERNEL_NAMES), sorted(set(S.KERNEL_NAMES) - set(reached))


@pytest.mark.parametrize("spread", T.SPREADS)
@pytest.mark.parametrize("net,flags,n,hw", T.FULL_NETS, ids=[c[0] for c in T.FULL_NETS])
def test_full_output_under_trained_like_weights(oracle, net, flags, n, hw, spread):
    """The whole output, bicubic term included and the last conv attenuated as ``synthetic_weights`` leaves it, on the default plan at
    the 1e-4 of the 0 .. 255 scale of test_hip_parity.py."""
    cfg = oracle.make_config(**flags)
    weights = T.trained_like_weights(cfg, T.BARE_SEED, spread)
    x, x2 = synthetic_batch(n, hw[0], hw[1], cfg["scale"], seed=T.BARE_SEED + 1)
    ref = oracle.forward(cfg, weights, x, x2, dtype=np.float64)
    y, kernels = S._forward(cfg, weights, x, x2)
    err = float(np.max(np.abs(y.astype(np.float64) - ref)))
    print("TRAINED-LIKE full output %s %dx%dx%d spread %d | max-abs %.3g of max|y| %.3g | %s"
          % (net, n, hw[0], hw[1], spread, err, float(np.max(np.abs(ref))), ",".join(kernels)))
    assert y.shape == ref.shape and np.isfinite(y).all() and err <= P.MAX_ABS_TOL, (net, spread, err)


def test_rebalancing_b1_against_b2_by_a_power_of_two(oracle):
    """B1 times 2^k and B2's filter times 2^-k is the same function, exactly (train_split16_cases.rebalanced): the float32 kernels,
    Winograd and direct, give the bits of k = 0, and the split16 kernels, whose f16 pieces move with the magnitudes, meet the bar."""
    net, flags, n, hw = next(c for c in T.FULL_NETS if c[0] == T.REBALANCE_NET)
    cfg, weights, x, x2, ref, r32 = _case(oracle, net, flags, n, hw, 0)
    f32_plans = [(("split16", 0),), (("split16", 0), ("winograd", 0))]
    base = [S._forward(cfg, weights, x, x2, options=o)[0] for o in f32_plans]
    failures = []
    for k in T.REBALANCE_K:
        moved = C.rebalanced(weights, k)
        assert not np.array_equal(moved["B1/conv_W"], weights["B1/conv_W"])
        for o, y0 in zip(f32_plans, base):
            y, kernels = S._forward(cfg, moved, x, x2, options=o)
            assert np.array_equal(y.view(np.uint32), y0.view(np.uint32)), (k, o, kernels, B.rel_error(y, y0.astype(np.float64)))
        y, kernels = S._forward(cfg, moved, x, x2)
        assert "conv3_h" in kernels and "conv_nin_h" in kernels, kernels
        failures.append(_judge(oracle, "%s rebalanced by 2^%d, split16 1" % (net, k), y, kernels, ref, r32, cfg, moved, x, x2, ()))
    S._finish(failures)
