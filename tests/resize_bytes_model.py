"""numpy restatement of the 8-bit bicubic resize (Pillow's ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc,
libImaging/Resample.c) over a given (bounds, coeffs) table, and of save_image's uint8 cast, for the tests of
dcscn_resize_bicubic_bytes / dcscn_sr_rgb_bytes.  No test lives here."""
import numpy as np

PRECISION_BITS = 22       # Resample.c: 32 - 8 - 2

# (in, out) sizes [h, w] -> [oh, ow] of the resize tests, host and device
SHAPES = [
    ((48, 48), (96, 96)), ((17, 33), (51, 99)), ((64, 80), (256, 320)),               # x2, x3, x4
    ((1, 1), (4, 4)), ((1, 7), (4, 28)), ((5, 1), (15, 3)), ((3, 2), (9, 6)),         # degenerate sizes
    ((96, 96), (48, 48)), ((99, 120), (33, 40)), ((128, 64), (32, 16)),               # antialiased shrinking
    ((37, 53), (37, 106)), ((37, 53), (74, 53)),                                      # one pass only
    ((37, 53), (37, 53)),                                                             # identity
    ((50, 70), (61, 23)),                                                             # one axis up, the other down
]


def checkerboard(h, w, c):
    """0 / 255 by pixel parity, the same in every channel."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], c, axis=2)


def pass_accumulators(image, table, axis):
    """int64 accumulators of one pass along `axis` (0: vertical, 1: horizontal) of a uint8 image [h, w, c], started at
    1 << 21 as Pillow starts them: what the int32 `ss` holds in front of the shift."""
    bounds, coeffs = table
    a = np.moveaxis(np.asarray(image).astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + a.shape[1:], np.int64)
    for i, (first, taps) in enumerate(bounds):
        k = coeffs[i, :taps].astype(np.int64).reshape((taps,) + (1,) * (a.ndim - 1))
        out[i] = (1 << (PRECISION_BITS - 1)) + (a[first:first + taps] * k).sum(axis=0)
    return np.moveaxis(out, 0, axis)


def clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(image, out_h, out_w, table_for, accumulators=None):
    """uint8 [h, w, c] -> [out_h, out_w, c]: horizontal pass into a uint8 intermediate, then the vertical pass; a pass that
    keeps its size is skipped.  `table_for(in_size, out_size)` -> (bounds [out, 2], coeffs [out, ksize] int32);
    `accumulators`: a list that receives every pass's accumulators."""
    image = np.asarray(image)
    h, w = image.shape[:2]
    for axis, (size, out_size) in ((1, (w, out_w)), (0, (h, out_h))):
        if size != out_size:
            acc = pass_accumulators(image, table_for(size, out_size), axis)
            if accumulators is not None:
                accumulators.append(acc)
            image = clip8(acc)
    return image


def cast_rule(values):
    """save_image's cast as the device applies it: truncate toward zero to an integer, keep the low 8 bits (defined for
    magnitudes below 2^31; integer operations only, so the result does not depend on the host's float -> uint8 conversion)."""
    return (np.trunc(values).astype(np.int64) & 255).astype(np.uint8)
