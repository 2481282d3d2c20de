"""``helper.loader`` of the reference (loader.py:27-67 and DynamicDataSets, loader.py:278-355).  BatchDataSets
(--build_batch true, pre-cut patch files) is not supported."""

import logging
import random

import numpy as np

import dcscn_amd  # noqa: F401
from dcscn_amd import imaging as util
from dcscn_amd.model import build_input_image          # noqa: F401


def build_image_set(file_path, channels=1, scale=1, convert_ycbcr=True, resampling_method="bicubic",
                    print_console=True):
    """(LR input, bicubic of LR, aligned true image), loader.py:27-38."""
    true_image = util.set_image_alignment(util.load_image(file_path, print_console=print_console), scale)
    if channels == 1 and true_image.shape[2] == 3 and convert_ycbcr:
        true_image = util.convert_rgb_to_y(true_image)
    input_image = util.resize_image_by_pil(true_image, 1.0 / scale, resampling_method=resampling_method)
    interpolated = util.resize_image_by_pil(input_image, scale, resampling_method=resampling_method)
    return input_image, interpolated, true_image


def load_input_image(filename, width=0, height=0, channels=1, scale=1, alignment=0, convert_ycbcr=True,
                     print_console=True):
    image = util.load_image(filename, print_console=print_console)
    return build_input_image(image, width, height, channels, scale, alignment, convert_ycbcr)


class DynamicDataSets:
    """Random patches of the images of a directory (loader.py:278-355), with the reference's sequence of ``random``
    calls: a shuffled image order (random.sample), a crop of batch_image_size * scale (randrange per axis), fliplr with
    probability 1/2 (randrange(2)), then the LR and bicubic images by util.resize_image_by_pil.  Decoded images are
    cached in memory.  next_patch() draws a patch's descriptor only; load_batch_image() cuts it on the host.

    ``augment_level`` N >= 2 trains on the dataset augmentation.py --augment_level N would write of this directory, without the
    copies: the dataset's entries are (filename, code) -- every file of ``filenames`` in order, and within a file the codes
    0 .. N-1 of util.AUGMENT_SUFFIXES -- and an entry's image is util.augment of the one cached decode.  The draws are those of an
    on-disk dataset whose files are listed in that order.  With level 0 or 1 nothing changes."""

    def __init__(self, scale, batch_image_size, channels=1, resampling_method="bicubic", augment_level=0):
        self.scale = scale
        self.batch_image_size = batch_image_size
        self.channels = channels
        self.resampling_method = resampling_method
        self.augment_level = augment_level
        self.filenames = []
        self.entries = None                 # augment_level >= 2: [(filename, code)], derived from filenames by init_batch_index
        self.count = 0
        self.batch_index = None
        self.index = 0
        self._cache = {}

    def set_data_dir(self, data_dir):
        self.filenames = util.get_files_in_directory(data_dir)
        self.count = len(self.filenames)
        if self.count <= 0:
            logging.error("Data Directory is empty.")
            exit(-1)

    def init_batch_index(self):
        if self.augment_level >= 2:         # from the filenames of now: train.py replaces them with rank 0's after set_data_dir
            self.entries = [(f, code) for f in self.filenames for code in range(self.augment_level)]
            self.count = len(self.entries)
        self.batch_index = random.sample(range(0, self.count), self.count)
        self.index = 0

    def get_next_image_no(self):
        if self.index >= self.count:
            self.init_batch_index()
        image_no = self.batch_index[self.index]
        self.index += 1
        return image_no

    def next_patch(self):
        """(filename, top, left, fliplr) of the next patch: the image of the shuffled order (skipping images smaller than a
        patch), a crop of batch_image_size * scale pixels at (top, left), then fliplr with probability 1/2 -- the reference's
        sequence of random calls, which load_batch_image cuts on the host and SuperResolution.train_batch on the device.
        With augment_level >= 2: (filename, top, left, fliplr, code), top and left in util.augment(image, code)."""
        size = self.batch_image_size * self.scale
        while True:
            image_no = self.get_next_image_no()
            filename, code = self.entries[image_no] if self.augment_level >= 2 else (self.filenames[image_no], 0)
            height, width = self.image(filename, code).shape[0:2]
            if height >= size and width >= size:
                break
            print("Error: %s should have more than %d x %d size." % (filename, size, size))
        top = 0 if height == size else random.randrange(height - size)
        left = 0 if width == size else random.randrange(width - size)
        fliplr = int(random.randrange(2) == 0)
        if self.augment_level >= 2:
            return filename, top, left, fliplr, code
        return filename, top, left, fliplr

    def image(self, filename, code=0):
        """The decoded image (uint8 [H, W, 1 | 3]), cached; ``code``: its variant util.augment(image, code), a view of it."""
        image = self._cache.get(filename)
        if image is None:
            image = util.load_image(filename, print_console=False)
            self._cache[filename] = image
        return util.augment(image, code) if code else image

    def load_batch_image(self, max_value):
        filename, top, left, fliplr, code = (self.next_patch() + (0,))[:5]
        size = self.batch_image_size * self.scale
        image = self.image(filename, code)[top:top + size, left:left + size, :]
        image = build_input_image(image, channels=self.channels, convert_ycbcr=True)
        if fliplr:
            image = np.fliplr(image)
        input_image = util.resize_image_by_pil(image, 1 / self.scale, resampling_method=self.resampling_method)
        input_bicubic_image = util.resize_image_by_pil(input_image, self.scale, resampling_method=self.resampling_method)
        if max_value != 255:
            scale = max_value / 255.0
            input_image = np.multiply(input_image, scale)
            input_bicubic_image = np.multiply(input_bicubic_image, scale)
            image = np.multiply(image, scale)
        return input_image, input_bicubic_image, image


class BatchDataSets:
    """--build_batch true (loader.py:86-275): not supported."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("--build_batch true (BatchDataSets) is not supported; use --build_batch false")
