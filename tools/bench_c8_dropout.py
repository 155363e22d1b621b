#!/usr/bin/env python
"""Timings of the 16-bit-resident DropOutLayer ops (tn_c8_dropout_fwd / tn_c8_dropout_bwd / tn_c8_scale,
theanet_amd/csrc/drop_c8.hip) against the fp32 route for the same logical tensor (tn_dropout_mask + tn_scale_mask
forward, tn_scale_mask backward; theanet_amd/csrc/pool.hip).

    python tools/bench_c8_dropout.py [--iters N] [--rounds R] [--dtype f16|bf16]

us/launch: HIP events around --iters back-to-back launches after warm-up, one process.  The 16-bit op and its fp32
counterpart are measured alternately, --rounds times each; the table gives the median and the run-to-run spread
((max - min) / median) of each, and the ratio of the medians.  A ratio whose distance from 1 lies inside the two spreads
is no difference.  Bytes are the algorithmic ones over the stored tensors: 16-bit forward / backward 2 * cells * 16 +
cells (tensor in, tensor out, a mask byte per cell); test version 2 * cells * 16; fp32 forward n * (1 + 4 + 1 + 4) (mask
written, x and mask read, y written), backward n * (4 + 1 + 4).  HBM roof: 6.3 TB/s achievable; back-to-back launches on
tensors of this size sit partly in the 256 MB Infinity Cache, so the fractions are upper bounds of what a step sees."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from theanet_amd import _lib  # noqa: E402
from theanet_amd.device import get_context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--dtype", choices=("f16", "bf16"), default="f16")
args = ap.parse_args()
ctx = get_context()
lib = ctx.lib
HBM = 6.3e12


def timeit(fn, iters):
    for _ in range(10):
        fn()
    ctx.sync()
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    lib.tn_event_create(ctx.h, ctypes.byref(a))
    lib.tn_event_create(ctx.h, ctypes.byref(b))
    lib.tn_event_record(ctx.h, a)
    for _ in range(iters):
        fn()
    lib.tn_event_record(ctx.h, b)
    ms = ctypes.c_float()
    ctx.call("tn_event_elapsed_ms", a, b, ctypes.byref(ms))
    return ms.value * 1e3 / iters


def pair(f16, f32):
    """Alternating rounds of both: (median, spread) of each."""
    a, b = [], []
    for _ in range(args.rounds):
        a.append(timeit(f16, args.iters))
        b.append(timeit(f32, args.iters))
    return [(statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for v in (a, b)]


# (N, C, S, pitch): cifar_drop's first two DropOutLayers, wide6's first block, a padded 14 x 14 map
SHAPES = [(2048, 64, 16, 16), (2048, 128, 8, 8), (128, 64, 64, 64), (4096, 32, 14, 16)]
ctx.call("tn_set_matmul_dtype", *((2, 1.0) if args.dtype == "bf16" else (1, 4096.0)))
d_step = ctx.zeros((1,), np.uint32)
print("dtype %s, %d launches per measurement, %d alternating rounds" % (args.dtype, args.iters, args.rounds))
print("%-18s %-5s %9s %7s %6s %9s %7s %6s %7s" % ("N,C,S,pitch", "op", "16-bit us", "spread", "HBM", "fp32 us", "spread",
                                                 "HBM", "ratio"))
for N, C, S, P in SHAPES:
    C8, n = (C + 7) // 8, N * C * S * S
    cells = N * C8 * P * P
    one = np.uint16(0x3f80 if args.dtype == "bf16" else 0x3c00)
    x = ctx.array(np.full((N, C8, P, P, 8), one, np.uint16))
    y = ctx.empty((N, C8, P, P, 8), np.uint16)
    m8 = ctx.zeros((N, C8, P, P), np.uint8)
    x32, y32 = ctx.array(np.ones((N, C, S, S), np.float32)), ctx.empty((N, C, S, S))
    m32 = ctx.empty((N, C, S, S), np.uint8)

    def fwd16():
        ctx.call("tn_c8_dropout_fwd", x.ptr, y.ptr, m8.ptr, N, C, S, P, .25, 1234, 0, d_step.ptr, 0, 1)

    def fwd32():
        ctx.call("tn_dropout_mask", m32.ptr, n, .25, 1234, 0, d_step.ptr, 0)
        ctx.call("tn_scale_mask", x32.ptr, m32.ptr, 1.0, y32.ptr, n, None, _lib.TN_ACT_LINEAR, 0.0)

    def bwd16():
        ctx.call("tn_c8_dropout_bwd", x.ptr, m8.ptr, y.ptr, N, C, S, P)

    def bwd32():
        ctx.call("tn_scale_mask", x32.ptr, m32.ptr, 1.0, y32.ptr, n, None, _lib.TN_ACT_LINEAR, 0.0)

    def test16():
        ctx.call("tn_c8_scale", x.ptr, y.ptr, N, C, S, P, .75)

    def test32():
        ctx.call("tn_scale_mask", x32.ptr, None, .75, y32.ptr, n, None, _lib.TN_ACT_LINEAR, 0.0)

    ops = (("fwd", fwd16, fwd32, 33 * cells, 10 * n), ("bwd", bwd16, bwd32, 33 * cells, 9 * n),
           ("test", test16, test32, 32 * cells, 8 * n))
    for op, f16, f32, b16, b32 in ops:
        (u16, s16), (u32, s32) = pair(f16, f32)
        print("%-18s %-5s %9.2f %6.1f%% %6.2f %9.2f %6.1f%% %6.2f %7.2f" % (
            "%d,%d,%d,%d" % (N, C, S, P), op, u16, 100 * s16, b16 / (u16 * 1e-6) / HBM, u32, 100 * s32,
            b32 / (u32 * 1e-6) / HBM, u16 / u32))
