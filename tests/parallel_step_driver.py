"""One training step of SuperResolution under the process group of this launch (a helper of tests/test_train_parallel_hip.py,
not a test): c-DCSCN x2 from the synthetic weights, plain gradient descent without clipping, dropout 0.8, a batch of 5 patches of
24 x 24 drawn from Set14 with a FIXED seed, so that the test can draw the same batch on the host and evaluate the float64
restatement on it.  Every rank writes its variables after the step, the loss the step reported and the patches it drew to
``<out_dir>/rank<r>.npz``.

    python tests/parallel_step_driver.py OUT_DIR                                           one process
    python -m torch.distributed.run --nproc-per-node N tests/parallel_step_driver.py OUT_DIR    N ranks (DCSCN_SHARE_GPU=1: on device 0)
"""
import os
import random
import sys

import numpy as np

from conftest import CONFIGS, GOLDEN          # (conftest puts the repository root and oracle/ on sys.path)

NET = "L7_F32to8_x2"
SEED = 20240607
LR = 1e-3
BATCH_NUM, BATCH_IMAGE_SIZE = 5, 24
FLAGS = dict(optimizer="gd", clipping_norm=0.0, dropout_rate=0.8, batch_num=BATCH_NUM, batch_image_size=BATCH_IMAGE_SIZE,
             initial_lr=LR, self_ensemble=1)


def main(out_dir):
    import dcscn_oracle
    from dcscn_amd import shard
    from dcscn_amd.model import SuperResolution
    from test_host import _flags
    group = shard.init_from_env()
    flags = dict(FLAGS, checkpoint_dir=os.path.join(out_dir, "models"), **CONFIGS[NET])
    if group.world > 1:
        flags["gpu_device_id"] = group.local_rank
    m = SuperResolution(_flags(**flags))
    m.train_group = group
    m.load_dynamic_datasets(os.path.join(GOLDEN, "set14"), BATCH_IMAGE_SIZE)
    if group.world > 1:                                     # one file order on every rank, as train.py does
        m.train.filenames = group.broadcast_object(m.train.filenames)
    m.build_graph()
    m.build_optimizer()
    m.load_weights(dcscn_oracle.synthetic_weights(dcscn_oracle.make_config(**CONFIGS[NET]), seed=0))
    m.init_train_step()
    random.seed(SEED)
    m.init_epoch_index()
    m.build_input_batch()
    patches = list(m._patches)
    key = m.dropout_key()
    m.train_batch()
    tensors = m._training_tensors()
    names = sorted(tensors)
    np.savez(os.path.join(out_dir, "rank%d.npz" % group.rank), names=np.array(names), world=group.world, lr=m.lr, key=key,
             max_value=m.max_value, l2_decay=m.l2_decay, training_loss_sum=m.training_loss_sum, step=m.step,
             files=np.array([os.path.basename(p[0]) for p in patches]), crops=np.array([p[1:] for p in patches], np.int64),
             **{"t%d" % i: tensors[n] for i, n in enumerate(names)})
    m.close()
    group.close()


if __name__ == "__main__":
    main(sys.argv[1])
