#!/usr/bin/env python
"""Cycle stamps of one block of the masked conv-block backward (convblock_bwd_mask_mfma, TN_CM_DBG = 16) at the
mnist.prms conv2 shape: what wave 0 of the block spends per phase of each of its images.

    python tools/cm_stamps.py [--block B] [--batch N] [--calls 3]          (TN_HIP_LIB=other.so for another build)

With the stamps on, the kernel writes them into db in place of the bias gradient (thread 0 of block B: setup done;
per image staged / wgrad done / dgrad rows done / copy-out done; slab written).  A build without the stamp between
the dgrad rows and the copy-out has three per image; the count tells which."""
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--block", type=int, default=0)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--calls", type=int, default=3)
a = ap.parse_args()
os.environ["TN_CM_DBG"] = str(16 | (a.block << 8))       # the library reads its knobs once

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tests.gpu_util import act_code, call, ctx, dev, empty  # noqa: E402

N, C, H, K, f, Ho, Hp = a.batch, 4, 13, 20, 3, 11, 6
rng = np.random.RandomState(1)
x = dev(rng.randn(N, C, H, H).astype(np.float32))
W = dev((rng.randn(K, C, f, f) / 6).astype(np.float32))
b = dev(rng.randn(K).astype(np.float32))
g = dev(rng.randn(N, K, Hp, Hp).astype(np.float32))
kind, prm = act_code("relu05")
geom = (N, C, H, H, K, f, 0, Ho, Ho, 2, Hp, Hp, kind, prm)
y, m = empty((N, K, Hp, Hp)), empty((N, K, Hp, Hp), np.uint8)
call("tn_convpool_fwd_mask", x.ptr, W.ptr, b.ptr, y.ptr, m.ptr, *geom)
dx, dW, db = empty((N, C, H, H)), empty((K, C, f, f)), empty((K,))
nblk = min(2 * ctx().info()[1], -(-N // 4))
images = len(range(a.block * 4, N, nblk * 4))
for _ in range(a.calls):
    db.fill_bytes(0)
    call("tn_convblock_bwd_mask", x.ptr, W.ptr, g.ptr, y.ptr, m.ptr, dx.ptr, dW.ptr, db.ptr, *geom)
    t = db.get_value()
    t = t[t > 0]
    d = np.diff(np.concatenate([[0], t])).astype(int)
    per = (len(t) - 2) // max(images, 1)
    names = {3: ["staged", "wgrad", "dgrad+copy"], 4: ["staged", "wgrad", "dgrad", "copy-out"]}.get(per)
    if names is None or len(t) != 2 + per * images:
        print("block %d: %d stamps for %d images: %s" % (a.block, len(t), images, d.tolist()))
        continue
    out = ["setup %d" % d[0]]
    for i in range(images):
        out.append("image %d: " % i + "  ".join("%s %d" % (nm, d[1 + per * i + j]) for j, nm in enumerate(names)))
    out.append("slab %d" % d[-1])
    out.append("total %d" % int(t[-1]))
    print("block %d | " % a.block + " | ".join(out))
