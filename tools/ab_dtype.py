#!/usr/bin/env python
"""Whole training step of DTYPE 'float16' against 'bfloat16' on ONE box: the same net, batch and inputs, each run a
fresh process, interleaved with an A/A control -- arms float16, float16' (identical to the first) and bfloat16, their
order rotating per repetition (as tools/ab.py does for bench.py, which has no bf16 leg).  A run builds the net, takes
--warmup steps, then times --steps steps (enqueued back to back, one sync at the end) with the host clock.

    python tools/ab_dtype.py [--prms cifar_like.prms --img 32 --batch 2048] [--reps 4] [--steps 200] [--warmup 30]

Prints every run and per arm the median / min / max ms per step, the A/A spread and bf16's difference from fp16."""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, ROOT)
    import ast
    import numpy as np
    from theanet_amd import NeuralNet
    with open(os.path.join(ROOT, "params", a.prms)) as fh:
        prms = ast.literal_eval(fh.read())
    prms["layers"][0][1]["img_sz"] = a.img
    tr = dict(prms["training_params"], BATCH_SZ=a.batch, DTYPE=a.child)
    rng = np.random.default_rng(0)
    ch = prms["layers"][0][1].get("num_maps", 3)
    x = rng.random((4 * a.batch, ch, a.img, a.img), dtype=np.float32)
    y = rng.integers(0, 10, 4 * a.batch).astype(np.int32)
    net = NeuralNet(copy.deepcopy(prms["layers"]), tr)
    fn = net.get_trin_model(x, y)
    for s in range(a.warmup):
        fn.enqueue(s % 4)
    fn.fetch()
    t0 = time.perf_counter()
    for s in range(a.steps):
        fn.enqueue(s % 4)
    cost = fn.fetch()[0]
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    print(json.dumps({"dtype": a.child, "ms_per_step": ms, "cost": float(cost)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--prms", default="cifar_like.prms")
    ap.add_argument("--img", type=int, default=32)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per run")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    arms = [("float16", "float16"), ("float16'", "float16"), ("bfloat16", "bfloat16")]
    res = {name: [] for name, _ in arms}
    for r in range(a.reps):
        order = arms[r % 3:] + arms[:r % 3]
        for name, dt in order:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", dt, "--prms", a.prms, "--img", str(a.img),
                   "--batch", str(a.batch), "--steps", str(a.steps), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode:
                sys.exit("run %s failed (exit %d):\n%s" % (name, p.returncode, p.stderr[-3000:]))
            line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            res[name].append(line["ms_per_step"])
            print("rep %d %-9s %.4f ms/step  cost %.5f" % (r, name, line["ms_per_step"], line["cost"]), flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, v in res.items():
        print("%-9s median %.4f  min %.4f  max %.4f ms/step" % (k, med[k], min(v), max(v)))
    aa = 100 * abs(med["float16'"] - med["float16"]) / med["float16"]
    d = 100 * (med["bfloat16"] - med["float16"]) / med["float16"]
    print("A/A spread %.2f %%; bfloat16 vs float16 %+.2f %% (%s)" % (aa, d, "within the A/A spread" if abs(d) <= aa else
                                                                    "outside the A/A spread"))
    print(json.dumps({"prms": a.prms, "img": a.img, "batch": a.batch, "median_ms": med, "aa_spread_pct": aa,
                      "bf16_vs_f16_pct": d}))


if __name__ == "__main__":
    main()
