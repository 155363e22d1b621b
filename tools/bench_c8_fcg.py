#!/usr/bin/env python
"""Timings of the general 16-bit-resident dense products (tn_c8_fcg_*, theanet_amd/csrc/fcg_c8.hip).

    python tools/bench_c8_fcg.py [--iters N] [--rounds R] [--steps K] [--batch B]

1. General against tiled on a shape both families take (2048 x 128 maps x 16 pixels -> 512, bf16): every op of
   tn_c8_fcg_* against tn_c8_fc_*, us/launch from HIP events around --iters back-to-back launches, the arms measured
   alternately --rounds times with the tiled op twice per round (A and A'): median, run-to-run spread ((max - min) /
   median) and the A/A' ratio -- what this harness cannot resolve.
2. The dense products of params/mnist_c8.prms at --batch (32 maps x 49 pixels -> 500): us/launch and the effective
   bytes/s against streaming W (1568 x 500 fp32) once.
3. params/mnist_c8.prms at --batch: ms per training step (two steps in flight, device draws) under DTYPE 'bfloat16' and
   'float32', nets built once and timed alternately --rounds times, --steps steps each, wall clock around enqueue ... sync."""
import argparse
import ast
import copy
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theanet_amd import _lib  # noqa: E402
from theanet_amd.device import get_context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--batch", type=int, default=4096)
args = ap.parse_args()
ctx = get_context()
lib = ctx.lib
LK = _lib.TN_ACT_LEAKY


def timeit(fn, iters):
    for _ in range(5):
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


def med(v):
    return statistics.median(v), (max(v) - min(v)) / statistics.median(v)


def ops(fam, B, C, HW, N, t):
    x, W, b, a, dz, dx, gW, gb, mk = t
    g = (B, C, HW, N)
    return (("fwd", lambda: ctx.call(fam + "_fwd", x.ptr, W.ptr, b.ptr, a.ptr, *g, LK, .1, None)),
            ("fwd_dropout", lambda: ctx.call(fam + "_fwd_dropout", x.ptr, W.ptr, b.ptr, a.ptr, *g, LK, .1, mk.ptr, .5, 99, 5, None, 0)),
            ("dgrad", lambda: ctx.call(fam + "_dgrad", dz.ptr, W.ptr, dx.ptr, *g, x.ptr, LK, .1)),
            ("wgrad", lambda: ctx.call(fam + "_wgrad", x.ptr, dz.ptr, gW.ptr, gb.ptr, *g)))


def tensors(B, C, HW, N):
    rng = np.random.RandomState(0)
    Kc = (C + 7) // 8 * HW * 8
    return (ctx.array(np.full((B, Kc), 0x3f80, np.uint16)), ctx.array((rng.randn(C * HW, N) / np.sqrt(C * HW)).astype(np.float32)),
            ctx.array(np.zeros((N,), np.float32)), ctx.empty((B, N)), ctx.array((rng.randn(B, N) * 1e-3).astype(np.float32)),
            ctx.empty((B, Kc), np.uint16), ctx.empty((C * HW, N)), ctx.empty((N,)), ctx.empty((B * N,), np.uint8))


ctx.call("tn_set_matmul_dtype", 2, 1.0)
B, C, HW, N = 2048, 128, 16, 512
t = tensors(B, C, HW, N)
print("1. %d x %d maps x %d pixels -> %d, bf16, %d launches per measurement, %d alternating rounds" % (B, C, HW, N, args.iters, args.rounds))
print("%-12s %10s %7s %10s %7s %7s %7s" % ("op", "general us", "spread", "tiled us", "spread", "ratio", "A/A'"))
for (name, fg), (_, ft) in zip(ops("tn_c8_fcg", B, C, HW, N, t), ops("tn_c8_fc", B, C, HW, N, t)):
    g, a0, a1 = [], [], []
    for _ in range(args.rounds):
        a0.append(timeit(ft, args.iters)); g.append(timeit(fg, args.iters)); a1.append(timeit(ft, args.iters))
    (ug, sg), (ut, st) = med(g), med(a0)
    print("%-12s %10.2f %6.1f%% %10.2f %6.1f%% %7.2f %7.3f" % (name, ug, 100 * sg, ut, 100 * st, ug / ut, med(a1)[0] / ut), flush=True)
del t

B, C, HW, N = args.batch, 32, 49, 500
t = tensors(B, C, HW, N)
wbytes = C * HW * N * 4
print("2. %d x %d maps x %d pixels -> %d, bf16: W is %.2f MB" % (B, C, HW, N, wbytes / 1e6))
for name, f in ops("tn_c8_fcg", B, C, HW, N, t):
    u, s = med([timeit(f, args.iters) for _ in range(args.rounds)])
    print("%-12s %10.2f us %6.1f%%  %8.1f GB/s of W streamed once" % (name, u, 100 * s, wbytes / (u * 1e-6) / 1e9), flush=True)
del t
ctx.call("tn_set_matmul_dtype", 0, 1.0)

from theanet_amd import NeuralNet  # noqa: E402

with open(os.path.join(ROOT, "params", "mnist_c8.prms")) as fh:
    prms = ast.literal_eval(fh.read())
prms["layers"][0][1]["img_sz"] = 28
rng = np.random.RandomState(1)
nb = 4
x = rng.rand(nb * B, 1, 28, 28).astype(np.float32)
y = rng.randint(0, 10, nb * B).astype(np.int32)
res = {"bfloat16": [], "float32": []}
print("3. params/mnist_c8.prms at batch %d, %d steps per measurement, %d alternating rounds" % (B, args.steps, args.rounds))
for r in range(args.rounds):
    for dt in ("bfloat16", "float32"):
        # (one net at a time: the context's DTYPE is the net's)
        net = NeuralNet(copy.deepcopy(prms["layers"]), dict(prms["training_params"], BATCH_SZ=B, DTYPE=dt))
        fn = net.get_trin_model(x, y)
        for s in range(20):
            fn.enqueue(s % nb)
        fn.fetch()
        ctx.sync()
        t0 = time.perf_counter()
        for s in range(args.steps):
            fn.enqueue(s % nb)
        fn.fetch()
        ctx.sync()
        res[dt].append((time.perf_counter() - t0) * 1e3 / args.steps)
        del fn, net
for dt, v in res.items():
    print("%-9s %8.4f ms/step  spread %.1f%%  (%s)" % (dt, med(v)[0], 100 * med(v)[1], " ".join("%.4f" % u for u in v)))
print("bfloat16 / float32: %.3f" % (med(res["bfloat16"])[0] / med(res["float32"])[0]))
