"""Train a DCSCN model on the MI355X -- same command line as the reference's train.py:

    python train.py --dataset=bsd200 --test_dataset=set5 [--scale=3] [--layers=7 ...]

Patches are cut from data/<dataset>/ (DynamicDataSets), every step runs on the engine's training plan (forward, backward,
clipping and the optimizer on the device, include/dcscn.h "Training"), every epoch evaluates data/<test_dataset>/ and saves
the checkpoint, and the run ends with the "Model Average" line of evaluate.py.  The checkpoint carries the optimizer slots
under TensorFlow's names and loads in evaluate.py.  --build_batch true (BatchDataSets) is not supported.

One process drives one GPU (``--gpu_device_id``).  Launched under ``torch.distributed.run`` with N ranks on one node the
training is data-parallel: every rank holds a full replica and draws the same patches (one seed per trial, rank 0's), computes
the gradient of its contiguous shard of each batch, the ranks exchange these gradients, and every rank reduces all of them in
rank order and applies the same update -- the replicas stay bit-identical, and the number of steps and the learning-rate
schedule are those of a one-process run (the losses of a given batch agree with it to float32 rounding: the reduction order
differs; include/dcscn.h "Data-parallel training").  Only rank 0 evaluates, logs and writes files.
"""

import logging
import os
import random
import sys

import DCSCN
from dcscn_amd import shard
from helper import args, utilty as util

FLAGS = args.get()


def main(not_parsed_args):
    if len(not_parsed_args) > 1:
        print("Unknown args:%s" % not_parsed_args)
        exit()
    if FLAGS.build_batch:
        print("Error. --build_batch true (BatchDataSets) is not supported; use --build_batch false.")
        sys.exit(-1)
    if not 0 <= FLAGS.train_augment_level <= 8:
        print("Error. --train_augment_level %d is not one of 0 .. 8 (augmentation.py's levels; 0 and 1 train on the images as they are)."
              % FLAGS.train_augment_level)
        sys.exit(-1)

    refusal = shard.train_batch_refusal(FLAGS.batch_num, int(os.environ.get("WORLD_SIZE", "1")))
    if refusal:                                             # before the process group exists: every rank leaves the same way
        print(refusal)
        sys.exit(-1)
    group = shard.init_from_env()
    if group.world > 1:
        FLAGS.gpu_device_id = group.local_rank

    model = DCSCN.SuperResolution(FLAGS, model_name=FLAGS.model_name)
    model.train_group = group
    model.load_dynamic_datasets(FLAGS.data_dir + "/" + FLAGS.dataset, FLAGS.batch_image_size)
    if group.world > 1:                                     # one file order (os.listdir promises none), so one seed draws one batch
        model.train.filenames = group.broadcast_object(model.train.filenames)
    model.build_graph()
    model.build_optimizer()
    model.build_summary_saver()

    root = group.rank == 0
    if root:
        logging.info("\n" + str(sys.argv))
        logging.info("Test Data:" + FLAGS.test_dataset + " Training Data:" + FLAGS.dataset)

    total_psnr = total_ssim = 0
    for i in range(FLAGS.tests):
        psnr, ssim = train(model, FLAGS, i, group)
        total_psnr += psnr
        total_ssim += ssim
        if root:
            logging.info("\nTrial(%d) %s" % (i, util.get_now_date()))
            model.print_steps_completed(output_to_logging=True)
            logging.info("PSNR:%f, SSIM:%f\n" % (psnr, ssim))

    if FLAGS.tests > 1 and root:
        logging.info("\n=== Final Average [%s] PSNR:%f, SSIM:%f ===" % (
            FLAGS.test_dataset, total_psnr / FLAGS.tests, total_ssim / FLAGS.tests))

    if root:
        model.copy_log_to_archive("archive")
    model.close()
    group.close()


def train(model, flags, trial, group):
    """One trial.  With several ranks every rank takes every training step; what surrounds the steps (evaluation between epochs,
    the log, checkpoints, result images) is rank 0's, and the other ranks wait for it at a barrier."""
    root = group.rank == 0
    test_filenames = util.get_files_in_directory(flags.data_dir + "/" + flags.test_dataset)
    if len(test_filenames) <= 0:
        print("Can't load images from [%s]" % (flags.data_dir + "/" + flags.test_dataset))
        exit()

    if group.world > 1:
        # every rank draws the whole batch: one sequence of the loader's `random` calls, seeded by rank 0 once per trial
        random.seed(group.broadcast_object(random.SystemRandom().getrandbits(64) if root else None))

    model.init_all_variables()
    if flags.load_model_name != "":
        model.load_model(flags.load_model_name, output_log=True)

    model.init_train_step()
    model.init_epoch_index()
    model_updated = True

    psnr = ssim = 0
    if root:
        psnr, ssim = model.evaluate(test_filenames)
        model.print_status(psnr, ssim, log=True)
        model.log_to_tensorboard(test_filenames[0], psnr, save_meta_data=True)
    group.barrier()

    while model.lr > flags.end_lr:
        model.build_input_batch()
        model.train_batch()

        if model.training_step * model.batch_num >= model.training_images:
            # one training epoch finished
            model.epochs_completed += 1
            if root:
                psnr, ssim = model.evaluate(test_filenames)
                model.print_status(psnr, ssim, log=model_updated)
                model.log_to_tensorboard(test_filenames[0], psnr, save_meta_data=model_updated)
                model.save_model(trial=trial, output_log=False)
            group.barrier()

            model_updated = model.update_epoch_and_lr()
            model.init_epoch_index()

    model.end_train_step()

    if os.environ.get("DCSCN_TRAIN_DUMP"):                  # tests: every rank's step count and the digest of its replica
        with open(os.environ["DCSCN_TRAIN_DUMP"], "a") as f:
            f.write("%d %d %s\n" % (group.rank, model.step, model.training_digest()))

    if root:
        # save last generation anyway
        model.save_model(trial=trial, output_log=True)

        # outputs result
        evaluate_model(model, flags.test_dataset)
        if flags.do_benchmark:
            for test_data in ["set5", "set14", "bsd100"]:
                if test_data != flags.test_dataset:
                    evaluate_model(model, test_data)
    group.barrier()

    return psnr, ssim


def evaluate_model(model, test_data):
    test_filenames = util.get_files_in_directory(FLAGS.data_dir + "/" + test_data)
    total_psnr = total_ssim = 0
    for filename in test_filenames:
        psnr, ssim = model.do_for_evaluate_with_output(filename, output_directory=FLAGS.output_dir, print_console=False)
        total_psnr += psnr
        total_ssim += ssim
    logging.info("Model Average [%s] PSNR:%f, SSIM:%f" % (
        test_data, total_psnr / len(test_filenames), total_ssim / len(test_filenames)))


if __name__ == "__main__":
    args.run(main)
