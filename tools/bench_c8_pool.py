#!/usr/bin/env python
"""Timings of the 16-bit-resident stand-alone PoolLayer ops (tn_c8_pool_fwd / tn_c8_pool_bwd,
theanet_amd/csrc/pool_c8.hip) against the fp32 ops on the same logical tensor (tn_pool_fwd / tn_pool_bwd;
theanet_amd/csrc/pool.hip).

    python tools/bench_c8_pool.py [--iters N] [--rounds R] [--dtype f16|bf16]

us/launch: HIP events around --iters back-to-back launches after warm-up, one process.  The 16-bit op and its fp32
counterpart are measured alternately, --rounds times each; the table gives the median and the run-to-run spread
((max - min) / median) of each, and the ratio of the medians.  A ratio whose distance from 1 lies inside the two spreads
is no difference.  Bytes are the algorithmic ones, every tensor once (the p * p reads of one y / gout cell by the backward
come from cache): 16-bit forward 16 * (cells of x inside the map + cells of y, pad included: they are written), backward
16 * (cells of x inside the map + 2 * cells of y inside the map + cells of gin, pad included); fp32 forward
4 * (n_in + n_out), backward 4 * (2 * n_in + 2 * n_out).  HBM roof: 6.3 TB/s achievable; back-to-back launches on tensors
below the 256 MB Infinity Cache sit in it, so their fractions are upper bounds of what a step sees."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from theanet_amd import _lib  # noqa: E402
from theanet_amd.device import c8_pool_pitch, get_context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--dtype", choices=("f16", "bf16"), default="bf16")
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


# (N, C, S, pitch, p): the two PoolLayers of cifar_pool3.prms at its batch size, and a 2x2 pool on wide6's first maps
SHAPES = [(2048, 32, 32, 32, 3), (2048, 64, 11, 16, 3), (128, 64, 64, 64, 2)]
ctx.call("tn_set_matmul_dtype", *((2, 1.0) if args.dtype == "bf16" else (1, 4096.0)))
rng = np.random.default_rng(0)
print("dtype %s, %d launches per measurement, %d alternating rounds" % (args.dtype, args.iters, args.rounds))
print("%-20s %-4s %9s %7s %6s %9s %7s %6s %7s %9s" % ("N,C,S,pitch,p", "op", "16-bit us", "spread", "HBM", "fp32 us", "spread",
                                                      "HBM", "ratio", "16-bit MB"))
for N, C, S, P, p in SHAPES:
    So = -(-S // p)
    Po, C8 = c8_pool_pitch(So), (C + 7) // 8
    geom = (N, C, S, P, p, So, Po)
    # patterns 0x3000 .. 0x3fff: positive, finite and with many ties in either element type; pad cells zero
    xr = np.zeros((N, C8, P, P, 8), np.uint16)
    xr[:, :, :S, :S] = rng.integers(0x3000, 0x4000, (N, C8, S, S, 8), dtype=np.uint16) & 0xfff0
    x, y = ctx.array(xr), ctx.empty((N, C8, Po, Po, 8), np.uint16)
    g = ctx.array(np.full((N, C8, Po, Po, 8), 0x3c00, np.uint16))
    gin = ctx.empty((N, C8, P, P, 8), np.uint16)
    x32 = ctx.array(rng.integers(0, 16, (N, C, S, S)).astype(np.float32))
    y32, g32, gin32 = ctx.empty((N, C, So, So)), ctx.array(np.ones((N, C, So, So), np.float32)), ctx.empty((N, C, S, S))
    del xr

    def fwd16():
        ctx.call("tn_c8_pool_fwd", x.ptr, y.ptr, *geom)

    def fwd32():
        ctx.call("tn_pool_fwd", x32.ptr, y32.ptr, N * C, S, S, p, So, So)

    def bwd16():
        ctx.call("tn_c8_pool_bwd", x.ptr, y.ptr, g.ptr, gin.ptr, *geom)

    def bwd32():
        ctx.call("tn_pool_bwd", x32.ptr, y32.ptr, g32.ptr, gin32.ptr, N * C, S, S, p, So, So, _lib.TN_ACT_LINEAR, 0.0)

    pl = N * C8
    n_in, n_out = N * C * S * S, N * C * So * So
    ops = (("fwd", fwd16, fwd32, 16 * pl * (S * S + Po * Po), 4 * (n_in + n_out)),
           ("bwd", bwd16, bwd32, 16 * pl * (S * S + 2 * So * So + P * P), 4 * (2 * n_in + 2 * n_out)))
    for op, f16, f32, b16, b32 in ops:
        (u16, s16), (u32, s32) = pair(f16, f32)
        print("%-20s %-4s %9.2f %6.1f%% %6.2f %9.2f %6.1f%% %6.2f %7.2f %9.1f" % (
            "%d,%d,%d,%d,%d" % geom[:5], op, u16, 100 * s16, b16 / (u16 * 1e-6) / HBM, u32, 100 * s32,
            b32 / (u32 * 1e-6) / HBM, u16 / u32, b16 / 1e6))
    del x, y, g, gin, x32, y32, g32, gin32
