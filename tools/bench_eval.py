#!/usr/bin/env python
"""Timings of an evaluation pass (the test functions of theanet_amd/trainfn.py): one call per minibatch against one sweep.

    python tools/bench_eval.py [--batches 16] [--evals N] [--reps R] [--steps K]

mnist.prms at batch 4096 (float32), a corpus of --batches minibatches, behind --steps training steps of the default
schedule (the setting of train.py: the training function is alive, so evaluating first brings the weights up to date).
One evaluation is all --batches minibatches, as

    calls    [fn(i) for i in range(batches)]     one weight sync, one launch of the statistics and one blocking copy back
                                                 per minibatch
    sweep    fn.sweep(range(batches))            one weight sync and one copy back for the run

Three arms -- calls, calls again (the A/A arm: what this box cannot resolve today) and sweep -- are interleaved --reps
times in rotating order, as tools/ab.py does; an arm's figure per repetition is the mean of --evals evaluations, each under
the host clock by itself (both forms end in a blocking copy: nothing is left in flight) behind an untimed epoch of
training steps and a synchronise -- so every evaluation starts from weights the training function has moved, as in
train.py.  Printed: ms per evaluation per arm (median, min .. max), the A/A resolution (the larger of the two medians'
difference and half the min-max range of either), the ratio calls / sweep with a verdict against that resolution, and,
for scale, an epoch of --steps training steps (step_cost loop + drain_costs, as train.py runs it)."""
import argparse
import ast
import copy
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
ap.add_argument("--batches", type=int, default=16)
ap.add_argument("--evals", type=int, default=20)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--steps", type=int, default=15)
ap.add_argument("--batch-div", type=int, default=1, help="divide the batch size (a rehearsal without a GPU)")
args = ap.parse_args()
ctx = get_context()

with open(os.path.join(ROOT, "params", "mnist.prms")) as fh:
    prms = ast.literal_eval(fh.read())
prms["layers"][0][1]["img_sz"] = 28
B, NB = 4096 // args.batch_div, args.batches
tr = dict(prms["training_params"], SEED=555555, BATCH_SZ=B)
rng = np.random.default_rng(1)
x = rng.random((NB * B, 1, 28, 28), dtype=np.float32)
y = rng.integers(0, 10, NB * B).astype(np.int32)
net = NeuralNet(copy.deepcopy(prms["layers"]), dict(tr))
train, fn = net.get_trin_model(x, y), net.get_test_model(x, y)


def epoch():
    for s in range(args.steps):
        train.step_cost(s % NB)
    train.drain_costs()


def calls():
    return [fn(i) for i in range(NB)]


def sweep():
    return fn.sweep(range(NB))


for _ in range(5):                                  # warm-up: the plan watches, records and starts replaying
    epoch()
assert sweep() == calls(), "sweep and calls disagree"
CONTROL = "calls (A/A)"
arms = {"calls": calls, CONTROL: calls, "sweep": sweep}
names = list(arms)
res = {a: [] for a in names}
for r in range(args.reps):
    for a in names[r % len(names):] + names[:r % len(names)]:
        total = 0.
        for _ in range(args.evals):
            epoch()                                 # (untimed: the evaluation finds the weights a step behind, as in train.py)
            ctx.sync()
            t0 = time.perf_counter()
            arms[a]()
            total += time.perf_counter() - t0
        res[a].append(1e3 * total / args.evals)

name, cus, _ = ctx.info()
print("%s (%d CUs), mnist.prms batch %d float32, %s: ms per evaluation of %d minibatches, median of %d x %d (min .. max)"
      % (name, cus, B, type(train).__name__, NB, args.reps, args.evals))
med = {a: statistics.median(res[a]) for a in names}
for a in names:
    print("  %-12s %8.4f  (%.4f .. %.4f)  %7.1f us/minibatch" % (a, med[a], min(res[a]), max(res[a]), 1e3 * med[a] / NB))
base = med["calls"]
floor = max(abs(med[CONTROL] - base) / base, max((max(res[a]) - min(res[a])) / 2 / base for a in ("calls", CONTROL)))
d = (med["sweep"] - base) / base
print("A/A resolution %.2f %%; sweep %+.2f %% vs calls (calls / sweep = %.2f) -> %s"
      % (100 * floor, 100 * d, base / med["sweep"], "FASTER" if d < -floor else ("SLOWER" if d > floor else "WITHIN NOISE")))

ep = []
for _ in range(args.reps):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(args.evals):
        epoch()
    ctx.sync()
    ep.append(1e3 * (time.perf_counter() - t0) / args.evals)
print("an epoch of %d training steps: %.4f ms (%.4f .. %.4f)" % (args.steps, statistics.median(ep), min(ep), max(ep)))
