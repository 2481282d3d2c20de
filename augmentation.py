"""Write the augmented copy of a training set -- same command line as the reference's augmentation.py:

    python augmentation.py --dataset=bsd200 [--augment_level=4] [--data_dir=data]

For every image of data/<dataset>/ it writes, into data/<dataset>_<level>/, the first <level> of the image's eight flipped and
rotated variants (helper/utilty.py augment, AUGMENT_SUFFIXES): <stem><ext> itself, then <stem>_v, _h, _hv (flips), _r1, _r2
(quarter turns), _r1_v and _r2_v (turns, then flipped), each in the file format of its source.  Train on the copies with
``train.py --dataset=<dataset>_<level>``.

``train.py --dataset=<dataset> --train_augment_level=<level>`` trains on the same set without these files: the variants are cut
on the device from the one uploaded image per file.  The two differ only for a lossy source format (JPEG), whose copies are encoded
a second time here.
"""

import os

from helper import args, utilty as util

args.flags.DEFINE_integer("augment_level", 4, "variants written per image, 1 .. 8: 4 = the image and its three flips, 8 = the rotations too")
FLAGS = args.get()


def main(not_parsed_args):
    if len(not_parsed_args) > 1:
        print("Unknown args:%s" % not_parsed_args)
        exit()
    level = FLAGS.augment_level
    if not 1 <= level <= len(util.AUGMENT_SUFFIXES):
        print("Error. --augment_level %d is not one of 1 .. %d." % (level, len(util.AUGMENT_SUFFIXES)))
        exit(-1)

    print("Building x%d augmented data." % level)
    source_dir = FLAGS.data_dir + "/" + FLAGS.dataset
    target_dir = "%s_%d" % (source_dir, level)
    util.make_dir(target_dir)
    for path in util.get_files_in_directory(source_dir):
        image = util.load_image(path)
        stem, extension = os.path.splitext(os.path.basename(path))
        for code in range(level):
            util.save_image(os.path.join(target_dir, stem + util.AUGMENT_SUFFIXES[code] + extension), util.augment(image, code))


if __name__ == "__main__":
    args.run(main)
