#!/usr/bin/env python
"""Timings of the 16-bit-resident MeanLayer ops (tn_c8_mean_fwd / tn_c8_mean_bwd, theanet_amd/csrc/mean_c8.hip) at the
shapes of the global-average-pooling nets.

    python tools/bench_c8_mean.py [--iters N] [--dtype f16|bf16]

us/launch (HIP events around --iters back-to-back launches, after warm-up) and achieved bytes/s over the algorithmic
bytes: forward N*ceil(C/8)*HW*16 (the c8 tensor) + N*C*4 (the fp32 means); backward twice the tensor (the block's stored
output read for act', the gradient written) + N*C*4 (dy).  HBM roof: 6.3 TB/s achievable."""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from theanet_amd import _lib  # noqa: E402
from theanet_amd.device import bf16_bits, get_context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--dtype", choices=("f16", "bf16"), default="f16")
args = ap.parse_args()
ctx = get_context()
lib = ctx.lib
rng = np.random.default_rng(0)
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


def rnd16(shape):
    v = rng.standard_normal(shape).astype(np.float32)
    return ctx.array(bf16_bits(v) if args.dtype == "bf16" else v.astype(np.float16).view(np.uint16))


SHAPES = [("cifar_gap", 2048, 128, 4, 4), ("wide6-gap 64px", 128, 256, 16, 16)]
ctx.call("tn_set_matmul_dtype", *((2, 1.0) if args.dtype == "bf16" else (1, 4096.0)))
print("dtype %s" % args.dtype)
print("%-16s %-20s %-9s %8s %8s %8s" % ("net", "N,C,H,W", "op", "us", "TB/s", "HBM frac"))
for name, N, C, H, W in SHAPES:
    C8 = (C + 7) // 8
    x = rnd16((N, C8, H, W, 8))
    dx = ctx.empty((N, C8, H, W, 8), np.uint16)
    y = ctx.empty((N, C))
    dy = ctx.array(rng.standard_normal((N, C)).astype(np.float32))
    tensor = N * C8 * H * W * 16
    ops = (("fwd", tensor + N * C * 4, lambda: ctx.call("tn_c8_mean_fwd", x.ptr, y.ptr, N, C, H, W)),
           ("bwd", 2 * tensor + N * C * 4,
            lambda: ctx.call("tn_c8_mean_bwd", dy.ptr, dx.ptr, N, C, H, W, x.ptr, _lib.TN_ACT_LEAKY, 0.1)))
    for op, nbytes, fn in ops:
        us = timeit(fn, args.iters)
        bw = nbytes / (us * 1e-6)
        print("%-16s %-20s %-9s %8.2f %8.2f %8.2f" % (name, "%d,%d,%d,%d" % (N, C, H, W), op, us, bw / 1e12, bw / HBM))
