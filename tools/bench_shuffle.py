#!/usr/bin/env python
"""Timings of shuffled epochs (set_order, theanet_amd/trainfn.py; tn_gather_batch, theanet_amd/csrc/gather.hip).

    python tools/bench_shuffle.py [--iters N] [--steps K] [--reps R] [--only op|steps]

1. The op alone: us/launch (HIP events around --iters back-to-back launches, after warm-up) against the bytes it moves
   -- nrows * (2 * row bytes + 4 (order entry) + 8 (label in and out)) -- at the full batch and at the 512-row shard of
   an 8-GPU run, next to the two tn_gather_rows launches of the take_index_list route.  HBM roof: 6.3 TB/s achievable;
   the datasets here (16 minibatches) sit in the Infinity Cache, as a real epoch's minibatch does not.
2. The step: ms/step of --steps enqueued steps (host clock around a loop that ends in a synchronise) of mnist.prms at
   batch 4096 (float32) and cifar_like.prms at batch 2048 (bfloat16), four arms interleaved --reps times in rotating
   order: in order, in order again (the A/A arm: what this box cannot resolve today), with an order set, and through
   take_index_list.  Every arm is a net of its own from the same seed."""
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
from theanet_amd import NeuralNet  # noqa: E402
from theanet_amd.device import get_context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", choices=("op", "steps"), default="")
ap.add_argument("--batch-div", type=int, default=1, help="divide the steps' batch sizes (a rehearsal without a GPU)")
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


def bench_op():
    print("%-14s %-6s %-20s %8s %8s %8s" % ("rows of", "nrows", "op", "us", "TB/s", "HBM frac"))
    rng = np.random.default_rng(0)
    for name, floats, full in (("mnist", 784, 4096), ("cifar", 3072, 2048)):
        for nrows in (full, 512):
            rows = 16 * nrows
            x = ctx.array(rng.random((rows, floats), dtype=np.float32))
            y = ctx.array(rng.integers(0, 10, rows).astype(np.int32))
            order = ctx.array(rng.permutation(rows).astype(np.int32))
            xs, ys = ctx.empty((nrows, floats)), ctx.empty((nrows,), np.int32)
            nbytes = nrows * (2 * floats * 4 + 12)
            k = [0]

            def batch():
                k[0] = (k[0] + 1) % 16
                ctx.call("tn_gather_batch", order.ptr, k[0] * nrows, nrows, x.ptr, xs.ptr, floats * 4, y.ptr, ys.ptr,
                         None, None, 0)

            def rows2():
                k[0] = (k[0] + 1) % 16
                idx = order.ptr + 4 * k[0] * nrows
                ctx.call("tn_gather_rows", x.ptr, idx, xs.ptr, nrows, floats * 4)
                ctx.call("tn_gather_rows", y.ptr, idx, ys.ptr, nrows, 4)

            for op, fn in (("tn_gather_batch", batch), ("2 x tn_gather_rows", rows2)):
                us = timeit(fn, args.iters)
                bw = nbytes / (us * 1e-6)
                print("%-14s %-6d %-20s %8.2f %8.2f %8.2f" % ("%s %d B" % (name, floats * 4), nrows, op, us, bw / 1e12, bw / HBM))


def bench_steps():
    NB = 12
    for prm, img, ch, B, dtype in (("mnist.prms", 28, 1, 4096, "float32"), ("cifar_like.prms", 32, 3, 2048, "bfloat16")):
        with open(os.path.join(ROOT, "params", prm)) as fh:
            prms = ast.literal_eval(fh.read())
        prms["layers"][0][1]["img_sz"] = img
        B //= args.batch_div
        tr = dict(prms["training_params"], SEED=555555, BATCH_SZ=B, DTYPE=dtype)
        rng = np.random.default_rng(1)
        x = rng.random((NB * B, ch, img, img), dtype=np.float32)
        y = rng.integers(0, 10, NB * B).astype(np.int32)
        perm = rng.permutation(NB * B).astype(np.int32)
        arms = {}
        for arm in ("in order", "in order (A/A)", "set_order", "take_index_list"):
            net = NeuralNet(copy.deepcopy(prms["layers"]), dict(tr))
            fn = net.get_trin_model(x, y, take_index_list=arm == "take_index_list")
            if arm == "set_order":
                fn.set_order(perm)
            batch = (lambda i: perm[i * B:(i + 1) * B]) if arm == "take_index_list" else (lambda i: i)
            arms[arm] = (fn, batch)
            for s in range(60):                       # warm-up: the plan watches, records and starts replaying
                fn.enqueue(batch(s % NB))
            ctx.sync()
        names = list(arms)
        res = {a: [] for a in names}
        for r in range(args.reps):
            for a in names[r % len(names):] + names[:r % len(names)]:
                fn, batch = arms[a]
                ctx.sync()
                t0 = time.perf_counter()
                for s in range(args.steps):
                    fn.enqueue(batch(s % NB))
                ctx.sync()
                res[a].append(1e3 * (time.perf_counter() - t0) / args.steps)
        print("%s batch %d %s: ms/step, median of %d x %d steps (min .. max)" % (prm, B, dtype, args.reps, args.steps))
        base = statistics.median(res["in order"])
        for a in names:
            fn = arms[a][0]
            pl = fn._plan if getattr(fn, "_seq", None) is None else fn._seq._plan
            med = statistics.median(res[a])
            print("  %-18s %8.4f  (%.4f .. %.4f)  %+7.1f us vs in order   %s%s"
                  % (a, med, min(res[a]), max(res[a]), 1e3 * (med - base), type(fn).__name__,
                     ", replayed" if pl is not None and pl.ready else ", interpreted"))


if args.only != "steps":
    bench_op()
if args.only != "op":
    bench_steps()
