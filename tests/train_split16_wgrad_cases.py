"""Shared by tests/test_train_split16_wgrad_hip.py and tests/test_train_split16_wgrad_host.py (test helper, not a test): option
"train_split16_wgrad" of include/dcscn.h.

``wgrad_h_plan`` restates twgrad_h_plan of csrc/train_wgrad_h.hpp: the tiling and the split of one layer's weight gradient, fixed by the
shape alone.  The unit of the partition is a tile of tr rows x tc columns of one image (tiles do not cross images: their halo is the
image's zero padding); split s sums tiles [s * tps, (s + 1) * tps) of the image-major, row-block, column-block order.  On images one
pixel wide a tile is tr consecutive pixels, so that the pixels per split -- the chunk -- are tps * tr, a multiple of 8.

A CPU model of one weight-gradient dot product (tests/test_train_split16_wgrad_host.py) puts the scaled split at or below the f32 chain's
error at K = 2,048 and K = 46,080 for dz of 1e-4 .. 1e-9: the mode has the f32 path's bar, C.TOL * max|g64| per tensor."""
import collections

import numpy as np

from test_train_hip import FLAGS

BLOCK = 64                 # kWgHBlock
PITCH = 288                # kWgHPitch: bytes of one LDS position
LDS_BUDGET = 144 * 1024    # kWgHLdsBudget
LDS_MAX = 160 * 1024       # kWgHLdsMax

Plan = collections.namedtuple("Plan", "tr tc tcp kpad in_cap tiles_y tiles_x tiles tg groups tps splits lds_bytes")


def _ceil(a, b):
    return -(-a // b)


def wgrad_h_plan(ks, cin, cout, n, H, W):
    tc = min(W, 64 if ks <= 3 else 32)
    tcp = tc + ks - 1
    slack = (ks - 1) * (tcp + 1)

    def positions(tr):
        kpad = _ceil(tr * tcp, 32) * 32
        in_cap = _ceil(kpad + slack, 16) * 16
        return kpad, in_cap

    tr = 1
    for cand in range(2, min(8, H) + 1):
        if sum(positions(cand)) * PITCH > LDS_BUDGET:
            break
        tr = cand
    kpad, in_cap = positions(tr)
    tiles_y, tiles_x = _ceil(H, tr), _ceil(W, tc)
    tiles = n * tiles_y * tiles_x
    tg = 9 if ks == 3 else ks
    groups = ks * ks // tg
    blocks = _ceil(cin, BLOCK) * groups * _ceil(cout, BLOCK)
    s = min(max(_ceil(256, blocks), 1), tiles)
    tps = _ceil(tiles, s)
    return Plan(tr, tc, tcp, kpad, in_cap, tiles_y, tiles_x, tiles, tg, groups, tps, _ceil(tiles, tps), (kpad + in_cap) * PITCH)


def engine_for(cfg, weights, split16, wgrad, **flags):
    """A training handle with both options set BEFORE dcscn_train_begin."""
    from dcscn_amd import engine
    eng = engine.Engine(cfg, device=0)
    eng.load_weights(weights)
    eng.set_option("train_split16", 1 if split16 else 0)
    eng.set_option("train_split16_wgrad", 1 if wgrad else 0)
    eng.train_begin(dict(FLAGS, **flags))
    return eng


def split_scaled(v):
    """(hi, lo) f16 pieces, as float64, of v (float32) times the power of two that puts max|v| into [2^13, 2^14), and that exponent."""
    top = float(np.max(np.abs(v)))
    e = 0 if top == 0.0 else 13 - int(np.floor(np.log2(top)))
    s = np.ldexp(v.astype(np.float32), e).astype(np.float32)
    hi = s.astype(np.float16)
    lo = (s - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64), e


def dot_models(a, b):
    """a, b: [dots][K] float32.  (exact, split, chain): the float64 dot products; the scaled split's -- three exact products per element,
    summed exactly over a chunk of 32, added to an f32 accumulator chunk after chunk, unscaled exactly; the f32 fma chain's."""
    exact = np.sum(a.astype(np.float64) * b.astype(np.float64), axis=1)
    ah, al, ea = split_scaled(a)
    bh, bl, eb = split_scaled(b)
    prod = ah * bh + ah * bl + al * bh                     # (each product exact in float64: 11-bit x 11-bit significands)
    acc = np.zeros(a.shape[0], np.float32)
    for k in range(0, a.shape[1], 32):
        acc = (acc.astype(np.float64) + np.sum(prod[:, k:k + 32], axis=1)).astype(np.float32)
    split = np.ldexp(acc.astype(np.float64), -(ea + eb))
    chain = np.zeros(a.shape[0], np.float32)
    p64 = a.astype(np.float64) * b.astype(np.float64)      # (exact: 24-bit x 24-bit), one rounding per fma
    for k in range(a.shape[1]):
        chain = (chain.astype(np.float64) + p64[:, k]).astype(np.float32)
    return exact, split, chain.astype(np.float64)
