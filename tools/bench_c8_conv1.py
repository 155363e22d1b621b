#!/usr/bin/env python
"""Timings of the 16-bit-resident 1x1 conv ops (tn_c8_conv1_fwd / _dgrad / _wgrad, theanet_amd/csrc/conv1_c8.hip) against
the fp32 route for the same logical layer (tn_conv2d_fwd [+ tn_pool_fwd] / tn_conv2d_dgrad / tn_conv2d_wgrad with
filter_sz 1: what a DTYPE 'float32' net runs for such a layer).

    python tools/bench_c8_conv1.py [--iters N] [--rounds R] [--dtype f16|bf16]

us/launch: HIP events around --iters back-to-back launches after warm-up, one process.  The 16-bit op and its fp32
counterpart are measured alternately, --rounds times each (the context's DTYPE is switched outside the timed region);
the table gives the median and the run-to-run spread ((max - min) / median) of each, and the ratio of the medians.  A
ratio whose distance from 1 lies inside the two spreads is no difference.  GB/s: the algorithmic bytes of the 16-bit op
over its stored tensors (2 bytes per element of x and y / dz and dx / x and dz; the pooled forward writes a quarter of y
and a mask byte per pooled element; weights not counted) per second -- with C, K <= 64 the ops move about 2 (C + K) bytes
per pixel against 2 C K flops and are HBM-bound (roof: 6.3 TB/s achievable; back-to-back launches on tensors of this
size sit partly in the 256 MB Infinity Cache, so the figures are upper bounds of what a step sees)."""
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
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--dtype", choices=("f16", "bf16"), default="bf16")
args = ap.parse_args()
ctx = get_context()
lib = ctx.lib
MODE16 = (2, 1.0) if args.dtype == "bf16" else (1, 4096.0)


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
        ctx.call("tn_set_matmul_dtype", *MODE16)
        a.append(timeit(f16, args.iters))
        ctx.call("tn_set_matmul_dtype", 0, 1.0)
        b.append(timeit(f32, args.iters))
    return [(statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for v in (a, b)]


# (N, C, S, K): wide6's first block size, cifar_nin's three blocks, cifar_nin's 10-map head
SHAPES = [(128, 64, 64, 64), (2048, 32, 32, 32), (2048, 64, 16, 64), (2048, 128, 8, 128), (2048, 128, 8, 10)]
LK = _lib.TN_ACT_LEAKY
print("dtype %s, %d launches per measurement, %d alternating rounds" % (args.dtype, args.iters, args.rounds))
print("%-18s %-9s %9s %7s %7s %9s %7s %7s" % ("N,C,S,K", "op", "16-bit us", "spread", "GB/s", "fp32 us", "spread", "ratio"))
rng = np.random.RandomState(0)
for N, C, S, K in SHAPES:
    C8, K8, Sp = (C + 7) // 8, (K + 7) // 8, S // 2
    one = np.uint16(0x3f80 if args.dtype == "bf16" else 0x3c00)
    x = ctx.array(np.full((N, C8, S, S, 8), one, np.uint16))
    dz = ctx.array(np.full((N, K8, S, S, 8), one, np.uint16))
    y, dx = ctx.empty((N, K8, S, S, 8), np.uint16), ctx.empty((N, C8, S, S, 8), np.uint16)
    yp, mk = ctx.empty((N, K8, Sp, Sp, 8), np.uint16), ctx.empty((N, K8, Sp, Sp, 8), np.uint8)
    W = ctx.array((rng.randn(K, C, 1, 1) / np.sqrt(C)).astype(np.float32))
    b = ctx.array(np.zeros((K,), np.float32))
    dW, db = ctx.empty((K, C, 1, 1)), ctx.empty((K,))
    x32, dz32 = ctx.array(np.ones((N, C, S, S), np.float32)), ctx.array(np.ones((N, K, S, S), np.float32))
    y32, dx32, yp32 = ctx.empty((N, K, S, S)), ctx.empty((N, C, S, S)), ctx.empty((N, K, Sp, Sp))
    g32 = (N, C, S, S, K, 1, 1, 0, S, S)

    def fwd16():
        ctx.call("tn_c8_conv1_fwd", x.ptr, W.ptr, b.ptr, y.ptr, None, N, C, S, S, K, LK, .1, 0)

    def fwd32():
        ctx.call("tn_conv2d_fwd", x32.ptr, W.ptr, b.ptr, y32.ptr, *g32, LK, .1)

    def pool16():
        ctx.call("tn_c8_conv1_fwd", x.ptr, W.ptr, b.ptr, yp.ptr, mk.ptr, N, C, S, S, K, LK, .1, 1)

    def pool32():
        ctx.call("tn_conv2d_fwd", x32.ptr, W.ptr, b.ptr, y32.ptr, *g32, LK, .1)
        ctx.call("tn_pool_fwd", y32.ptr, yp32.ptr, N * K, S, S, 2, Sp, Sp)

    def dgrad16():
        ctx.call("tn_c8_conv1_dgrad", dz.ptr, W.ptr, dx.ptr, N, C, S, S, K, x.ptr, LK, .1, 0, None)

    def dgrad32():
        ctx.call("tn_conv2d_dgrad", dz32.ptr, W.ptr, dx32.ptr, *g32, x32.ptr, LK, .1)

    def wgrad16():
        ctx.call("tn_c8_conv1_wgrad", x.ptr, dz.ptr, dW.ptr, db.ptr, N, C, S, S, K, 0, None)

    def wgrad32():
        ctx.call("tn_conv2d_wgrad", x32.ptr, dz32.ptr, dW.ptr, db.ptr, *g32)

    pix = N * S * S
    ops = (("fwd", fwd16, fwd32, 16 * pix * (C8 + K8)), ("fwd+pool", pool16, pool32, 16 * pix * C8 + 6 * pix * K8),
           ("dgrad", dgrad16, dgrad32, 16 * pix * (K8 + 2 * C8)), ("wgrad", wgrad16, wgrad32, 16 * pix * (C8 + K8)))
    for op, f16, f32, nbytes in ops:
        (u16, s16), (u32, s32) = pair(f16, f32)
        print("%-18s %-9s %9.2f %6.1f%% %7.0f %9.2f %6.1f%% %7.2f" % (
            "%d,%d,%d,%d" % (N, C, S, K), op, u16, 100 * s16, nbytes / (u16 * 1e-6) / 1e9, u32, 100 * s32, u16 / u32), flush=True)
    del x, dz, y, dx, yp, mk, x32, dz32, y32, dx32, yp32
