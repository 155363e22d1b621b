#!/usr/bin/env python
"""What the reference's MNIST net (params/mnist.prms: 3x3 'valid' convs of 4 and 20 maps, 28 -> 26 -> 13 -> 11 -> 6) costs a
training step at batch 4096 under the settings that can run it:

  float32     DTYPE float32: the fp32 conv kernels, fused conv + pool blocks (bench.py's flagship setting)
  conv-bf16   DTYPE float32 with CONV 'bfloat16': fp32 tensors, bf16 products (conv_bf16.hip), nothing fused
  any-bf16    DTYPE bfloat16 with CONV_SHAPES 'any' (params/mnist_16.prms): 16-bit-resident, the general conv family
  any-f16     DTYPE float16 with CONV_SHAPES 'any'      (tn_c8_convg_*, convg_c8.hip), stand-alone pools

    python tools/bench_c8_convg.py [--steps K] [--reps R] [--rounds N] [--batch B]

ms/step of --steps enqueued steps (host clock around a loop that ends in a synchronise; median of --reps, after a warm-up
in which the step plan watches, records and starts replaying); every arm is built once and the arms are timed in
--rounds alternating rounds, the order rotating, so that clock drift hits all of them.  The table gives each arm's median
over the rounds, its spread ((max - min) / median) and the ratio to float32.  A ratio whose distance from 1 lies inside the
spreads is no difference.

One arm of an interleaved A/B with an A/A control across processes (tools/ab.py --script tools/bench_c8_convg.py --args
--json "BENCH_CONVG_ARM=float32" "BENCH_CONVG_ARM=conv-bf16" ...): --json times the arm named by the environment variable
BENCH_CONVG_ARM alone and prints one JSON line with "ms_per_step"."""
import argparse
import ast
import copy
import json
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
ap.add_argument("--steps", type=int, default=400)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--json", action="store_true")
args = ap.parse_args()
ctx = get_context()
NB = 4

ARMS = {"float32": {"DTYPE": "float32"},
        "conv-bf16": {"DTYPE": "float32", "CONV": "bfloat16"},
        "any-bf16": {"DTYPE": "bfloat16", "CONV_SHAPES": "any"},
        "any-f16": {"DTYPE": "float16", "CONV_SHAPES": "any"}}


def build(arm):
    with open(os.path.join(ROOT, "params", "mnist.prms")) as fh:
        prms = ast.literal_eval(fh.read())
    prms["layers"][0][1]["img_sz"] = 28
    tr = dict(prms["training_params"], SEED=555555, BATCH_SZ=args.batch, **ARMS[arm])
    rng = np.random.default_rng(1)
    x = rng.random((NB * args.batch, 1, 28, 28), dtype=np.float32)
    y = rng.integers(0, 10, NB * args.batch).astype(np.int32)
    net = NeuralNet(copy.deepcopy(prms["layers"]), tr)
    fn = net.get_trin_model(x, y)
    for s in range(60):
        fn.enqueue(s % NB)
    ctx.sync()
    return net, fn


def time_fn(fn):
    for s in range(8):                   # (another arm ran last: the context is taken over outside the timed region)
        fn.enqueue(s % NB)
    ms = []
    for _ in range(args.reps):
        ctx.sync()
        t0 = time.perf_counter()
        for s in range(args.steps):
            fn.enqueue(s % NB)
        ctx.sync()
        ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
    return statistics.median(ms)


def how(fn):
    seq = getattr(fn, "_seq", None)
    pl = (seq or fn)._plan
    return "%s%s" % (type(seq or fn).__name__, ", replayed" if pl is not None and pl.ready else ", interpreted")


if args.json:
    arm = os.environ.get("BENCH_CONVG_ARM", "float32")
    net, fn = build(arm)
    ms = time_fn(fn)
    cost = float(fn.fetch()[0])
    assert np.isfinite(cost), cost
    print(json.dumps({"arm": arm, "batch": args.batch, "ms_per_step": ms, "how": how(fn)}))
    sys.exit(0)

built = {arm: build(arm) for arm in ARMS}
names = list(ARMS)
got = {arm: [] for arm in ARMS}
for r in range(args.rounds):
    for arm in names[r % len(names):] + names[:r % len(names)]:
        got[arm].append(time_fn(built[arm][1]))
base = statistics.median(got["float32"])
print("params/mnist.prms, batch %d, %d steps x %d reps, %d alternating rounds" % (args.batch, args.steps, args.reps, args.rounds))
print("%-10s %10s %8s %8s   %s" % ("arm", "ms/step", "spread", "ratio", "schedule"))
for arm in names:
    med = statistics.median(got[arm])
    cost = float(built[arm][1].fetch()[0])
    assert np.isfinite(cost), (arm, cost)
    print("%-10s %10.4f %7.1f%% %8.2f   %s" % (arm, med, 100 * (max(got[arm]) - min(got[arm])) / med, med / base, how(built[arm][1])))
