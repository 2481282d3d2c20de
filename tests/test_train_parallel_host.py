"""Data-parallel training, the parts that need no GPU: which patches of a batch a rank trains on and the first_index it passes,
the length of a gradient record, the launch train.py refuses, and the record exchange of a one-process group."""
import pytest
import torch

from dcscn_amd import shard


@pytest.mark.parametrize("batch_num,world,want", [
    (5, 2, [(0, 3), (3, 5)]),
    (5, 3, [(0, 2), (2, 4), (4, 5)]),
    (20, 8, [(0, 3), (3, 6), (6, 9), (9, 12), (12, 14), (14, 16), (16, 18), (18, 20)]),
    (3, 3, [(0, 1), (1, 2), (2, 3)]),
    (7, 1, [(0, 7)]),
])
def test_shard_of_a_batch_and_its_first_index(batch_num, world, want):
    got = [shard.train_shard(batch_num, r, world) for r in range(world)]
    assert got == want
    # contiguous in rank order from patch 0, nobody empty: begin is the first_index the dropout masks are indexed from
    assert got[0][0] == 0 and got[-1][1] == batch_num
    assert all(a[1] == b[0] for a, b in zip(got, got[1:]))
    assert all(end > begin for begin, end in got)


def test_shard_of_a_batch_smaller_than_the_world_is_an_error():
    with pytest.raises(ValueError):
        shard.train_shard(2, 0, 3)
    with pytest.raises(ValueError):
        shard.train_shard(5, 3, 3)


@pytest.mark.parametrize("count,want", [(0, 8), (1, 12), (3, 12), (4, 12), (5, 16), (1000, 1008), (1001, 1012), (2 ** 31 + 1, 2 ** 31 + 12)])
def test_record_length(count, want):
    n = shard.record_floats(count)
    assert n == want
    assert n % 4 == 0 and (n - shard.RECORD_TRAILER_FLOATS) % 4 == 0          # records and their trailers start on 16 bytes
    assert 0 <= n - shard.RECORD_TRAILER_FLOATS - count < 4
    with pytest.raises(ValueError):
        shard.record_floats(-1)


def test_train_py_refuses_a_batch_smaller_than_the_world():
    assert shard.train_batch_refusal(20, 1) is None
    assert shard.train_batch_refusal(8, 8) is None
    assert shard.train_batch_refusal(5, 3) is None
    msg = shard.train_batch_refusal(2, 3)
    assert msg and "--batch_num=2" in msg and "3 ranks" in msg
    assert shard.train_batch_refusal(0, 1)
    assert shard.train_batch_refusal(4, 0)


def test_all_gather_records_of_one_rank_is_the_identity():
    group = shard.Group()
    record = torch.arange(shard.record_floats(10), dtype=torch.float32)
    out = group.all_gather_records(record)
    assert out.shape == (1, record.numel())
    assert out.data_ptr() == record.data_ptr()                                  # the record itself, not a copy
    assert torch.equal(out[0], record)
    assert group.broadcast_object({"a": 1}) == {"a": 1}


# ---- the host restatement of dcscn_train_apply_records (tests/train_ref.py) that tests/test_train_apply_records_hip.py compares
# ---- the device with bit for bit: pinned here against plainer arithmetic, and shown to see what it is there to see

COUNTS = (2604, 27209, 28654, 1823)          # the variable counts of the nets of the device test, one per residue mod 4


def _reduced(count, world, large, order=None):
    import numpy as np
    import train_ref as R
    rec = R.make_records(count, world, R.RECORD_SEEDS[count], large=large)
    grads, tr = R.record_parts(rec, count)
    w = R.rank_weights(tr[:, 2], order)
    return rec, w, R.weighted_sum(grads, w, order).astype(np.float32)


@pytest.mark.parametrize("count", COUNTS)
def test_restated_norm_agrees_with_an_exactly_rounded_sum(count):
    import math
    import numpy as np
    import train_ref as R
    for world, large in ((8, False), (16, True), (1, False)):
        rec, w, g = _reduced(count, world, large)
        exact = math.fsum(float(v) * float(v) for v in g)        # a float32 squared is exact in float64; fsum rounds once
        total = R.tree_sumsq(g)
        assert abs(total - exact) <= 1e-12 * exact, (total, exact)
        got, stats, clip = R.reduce_records(rec, count, 5.0)
        assert np.array_equal(got.view(np.uint32), g.view(np.uint32))
        assert stats[2].dtype == np.float32 and stats[2] == np.float32(math.sqrt(total)) and np.isfinite(stats[2])
        assert clip.dtype == np.float32 and clip == np.float32(5.0) / stats[2] and stats[2] > 5.0
        assert abs(float(np.sum(w)) - 1.0) < 1e-15 and len(set(w)) > 1 or world == 1      # uneven shards


@pytest.mark.parametrize("count", COUNTS)
def test_restated_records_hold_what_they_are_meant_to(count):
    import numpy as np
    import train_ref as R
    rec = R.make_records(count, 16, R.RECORD_SEEDS[count], large=True)
    grads, tr = R.record_parts(rec, count)
    assert rec.shape == (16, shard.record_floats(count)) and rec.dtype == np.float32
    assert np.all(rec[:, count:R.record_pad(count)] == 12345.0)                            # padding that is not zero
    assert np.isfinite(grads).all() and (grads > 0).any() and (grads < 0).any()
    tiny = np.finfo(np.float32).tiny
    assert np.any((grads != 0) & (np.abs(grads) < tiny))                                   # subnormals
    assert np.any(np.signbit(grads) & (grads == 0)) and np.any(~np.signbit(grads) & (grads == 0))      # -0 and +0
    assert np.any((grads[0] == 1.0) & (grads[1] == np.float32(-1.0) + np.float32(2.0 ** -23)))
    assert np.max(np.abs(grads)) == np.float32(2.0e38)
    with np.errstate(over="ignore"):
        assert np.isinf(np.sum(grads, axis=0, dtype=np.float32)).any()                     # a plain float32 sum overflows
    assert np.all(tr[:, 2] == np.round(tr[:, 2])) and np.all(tr[:, 2] >= 1) and len(set(tr[:, 2])) > 1
    assert list(tr[:4, 2]) == [3, 2, 2, 1] and np.all(tr[:, [0, 1, 3]] > 0)


@pytest.mark.parametrize("count", COUNTS)
def test_rank_order_is_visible_in_the_restated_gradient_at_world_8(count):
    """Otherwise a device that reduced in another order would pass the bit-for-bit test.  The float64 sum is rounded to float32
    once, so the order shows only where that sum lies next to a rounding boundary: RECORD_SEEDS holds seeds where it does."""
    import numpy as np
    import train_ref as R
    for large in (False, True):
        rec, w, g = _reduced(count, 8, large)
        _, w_rev, g_rev = _reduced(count, 8, large, order=range(7, -1, -1))
        changed = int(np.count_nonzero(g.view(np.uint32) != g_rev.view(np.uint32)))
        print("count %d large %d: %d float32 values of g change when the ranks are reduced in reversed order" % (count, large, changed))
        assert changed >= 1
        _, tr = R.record_parts(rec, count)
        for k in (0, 1, 3):                                        # and in the stats, which stay float64, directly
            assert R.weighted_sum(tr[:, k], w) != R.weighted_sum(tr[:, k], w, order=range(7, -1, -1)), k


@pytest.mark.parametrize("count", COUNTS)
def test_order_of_the_count_sum_is_visible_with_fractional_counts_only(count):
    """Integer patch counts add up exactly in any order; the records with fractional counts are the ones on which a sum taken from
    the last rank gives other weights, and through them other stats."""
    import numpy as np
    import train_ref as R
    rev = range(7, -1, -1)
    _, tr = R.record_parts(R.make_records(count, 8, R.RECORD_SEEDS[count]), count)
    assert np.array_equal(R.rank_weights(tr[:, 2]), R.rank_weights(tr[:, 2], order=rev))
    rec = R.make_records(count, 8, R.RECORD_SEEDS[count], fractional=True)
    grads, tr = R.record_parts(rec, count)
    assert np.all(tr[:, 2] > 0) and np.any(tr[:, 2] != np.round(tr[:, 2]))
    w, w_rev = R.rank_weights(tr[:, 2]), R.rank_weights(tr[:, 2], order=rev)
    assert not np.array_equal(w, w_rev)
    # a weight that moves by one float64 ulp seldom moves a float32 of g; the float64 stats show it
    changed = [k for k in (0, 1, 3) if R.weighted_sum(tr[:, k], w) != R.weighted_sum(tr[:, k], w_rev)]
    print("count %d: stats %r change when the counts are summed from the last rank" % (count, changed))
    assert changed
