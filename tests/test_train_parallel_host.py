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
