#!/usr/bin/env python
"""A/B of the MATMUL training param on ONE box, in ONE process: the same net built once per arm ('float32' twice -- the
second build is the A/A control -- and each mode named on the command line), timed in interleaved rounds whose order
rotates, as tools/ab.py does for environments.  (tools/ab.py drives bench.py, which takes MATMUL from the params file;
this is the same protocol for a training param.)

    python tools/ab_matmul.py [--prms mlp3.prms] [--batch 4096] [--steps 100] [--rounds 7] [bfloat16 [bf16x3]]
    python tools/ab_matmul.py --conv --prms mnist_wide.prms --batch 0 [bfloat16]
    python tools/ab_matmul.py --conv --prms cifar_like.prms --batch 0 --img 32 --maps 3 [bfloat16]

--conv: the arms are values of the CONV training param (the conv layers' products) instead of MATMUL's; --batch 0 takes
the spec's own BATCH_SZ; --img / --maps give the input of specs that are not mnist-shaped.

Prints every round, per-arm median / min / max ms per step (wall clock over --steps enqueued steps, the first round
dropped as warm-up), the A/A spread and each arm's difference from 'float32' next to it."""
import argparse
import ast
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--prms", default="mlp3.prms")
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--conv", action="store_true", help="A/B the CONV training param instead of MATMUL")
ap.add_argument("--img", type=int, default=28)
ap.add_argument("--maps", type=int, default=1)
ap.add_argument("modes", nargs="*", default=["bfloat16"])
a = ap.parse_args()
PARAM = "CONV" if a.conv else "MATMUL"

from theanet_amd import NeuralNet  # noqa: E402

with open(os.path.join(ROOT, "params", a.prms)) as fh:
    prms = ast.literal_eval(fh.read())
prms["layers"][0][1]["img_sz"] = a.img
if a.maps != 1:
    prms["layers"][0][1]["num_maps"] = a.maps
if not a.batch:
    a.batch = prms["training_params"]["BATCH_SZ"]
NB = 4
rng = np.random.RandomState(0)
x = rng.rand(NB * a.batch, a.maps, a.img, a.img).astype(np.float32)
y = rng.randint(0, 10, NB * a.batch).astype(np.int32)
CONTROL = "float32 (A/A control)"
arms = {}
for label, mm in [("float32", "float32")] + [(m, m) for m in a.modes] + [(CONTROL, "float32")]:
    tp = dict(prms["training_params"], BATCH_SZ=a.batch, SEED=5)
    tp[PARAM] = mm
    net = NeuralNet([(k, dict(v)) for k, v in prms["layers"]], tp)
    arms[label] = (net, net.get_trin_model(x, y))
res = {k: [] for k in arms}
labels = list(arms)
for r in range(a.rounds):
    for k in labels[r % len(labels):] + labels[:r % len(labels)]:
        net, fn = arms[k]
        for s in range(10):
            fn.enqueue(s % NB)
        fn.fetch()
        net.ctx.sync()
        t0 = time.perf_counter()
        for s in range(a.steps):
            fn.enqueue(s % NB)
        out = fn.fetch()
        net.ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        if r:
            res[k].append(ms)
        print("round %d  [%-22s]  %.4f ms per step   cost %.4f" % (r, k, ms, out[0]), flush=True)
med = {k: statistics.median(v) for k, v in res.items()}
for k in labels:
    print("MEDIAN [%-22s]  %.4f ms per step  (min %.4f max %.4f, n=%d)" % (k, med[k], min(res[k]), max(res[k]), len(res[k])))
spread = abs(med[CONTROL] - med["float32"]) / med["float32"]
print("A/A spread %.2f %%" % (100 * spread))
for m in a.modes:
    d = (med[m] - med["float32"]) / med["float32"]
    print("%s against float32: %+.2f %%  (%s the A/A spread)" % (m, 100 * d, "outside" if abs(d) > spread else "inside"))
