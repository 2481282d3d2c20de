"""Write the Y channel of a training set as grey BMP files -- same command line as the reference's convert_y.py:

    python convert_y.py --dataset=bsd200 [--data_dir=data]

For every image of data/<dataset>/ it writes data/<dataset>_y/<stem>.bmp: the luma of an RGB image (helper/utilty.py
convert_rgb_to_y, cast to uint8 the way save_image casts: truncated), the pixels of a grey one as they are.  Training on
``--dataset=<dataset>_y`` then decodes one channel per image instead of three.
"""

import os

from helper import args, utilty as util

FLAGS = args.get()


def main(not_parsed_args):
    if len(not_parsed_args) > 1:
        print("Unknown args:%s" % not_parsed_args)
        exit()

    print("Building Y channel data...")
    source_dir = FLAGS.data_dir + "/" + FLAGS.dataset
    target_dir = source_dir + "_y"
    util.make_dir(target_dir)
    for path in util.get_files_in_directory(source_dir):
        image = util.load_image(path)
        if image.shape[2] == 3:
            image = util.convert_rgb_to_y(image)
        stem = os.path.splitext(os.path.basename(path))[0]
        util.save_image(os.path.join(target_dir, stem + ".bmp"), image)


if __name__ == "__main__":
    args.run(main)
