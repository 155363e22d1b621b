#!/usr/bin/env python
"""Bit-level A/B of the fp32 conv family's host dispatch: calls every fp32 conv entry point of the C-ABI on seeded inputs
and prints one line per (entry, case) with a SHA-256 of every output buffer.  Run it once per build of the library and
compare the two outputs; a different route, slab count or summation order changes the bits of a dW.

    TN_HIP_LIB=old/libtheanet_hip.so python tools/conv_ab.py > old.txt
    python tools/conv_ab.py > new.txt && cmp old.txt new.txt

The shapes are the ones tests/test_gpu_kernels.py checks against the oracle (its case lists, imported); nothing is
compared with a reference here.  Entries whose capability query refuses a shape print `unsupported` for it."""
import hashlib
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import theanet_oracle as O                              # noqa: E402
from tests import test_gpu_kernels as G                             # noqa: E402
from tests.gpu_util import act_code, call, ctx, dev, empty          # noqa: E402


def cases(test):
    return next(m.args[1] for m in test.pytestmark if m.name == "parametrize")


def report(entry, case, *outs):
    ctx().sync()
    print("%-34s %-48s %s" % (entry, case, " ".join(hashlib.sha256(o.get_value().tobytes()).hexdigest()[:16] for o in outs)))


def tensors(case_id, N, C, H, K, f, *shapes):
    """x, W, b and one standard-normal tensor per further shape, seeded by the case."""
    rng = np.random.RandomState(zlib.crc32(repr(case_id).encode()))
    x = rng.randn(N, C, H, H).astype(np.float32)
    W = (rng.randn(K, C, f, f) / np.sqrt(C * f * f)).astype(np.float32)
    return [dev(x), dev(W), dev(rng.randn(K).astype(np.float32))] + [dev(rng.randn(*s).astype(np.float32)) for s in shapes]


def conv2d(case):
    N, C, H, K, f, s, mode, act = case
    pad, _, Ho = O.conv_geometry(H, f, s, mode)
    x, W, b, dz, prev = tensors(case, N, C, H, K, f, (N, K, Ho, Ho), (N, C, H, H))
    geom = (N, C, H, H, K, f, s, pad, Ho, Ho)
    a, dW, db, dx = empty((N, K, Ho, Ho)), empty(W.shape), empty((K,)), empty(x.shape)
    call("tn_conv2d_fwd", x.ptr, W.ptr, b.ptr, a.ptr, *geom, *act_code(act))
    report("tn_conv2d_fwd", case, a)
    call("tn_conv2d_wgrad", x.ptr, dz.ptr, dW.ptr, db.ptr, *geom)
    report("tn_conv2d_wgrad", case, dW, db)
    call("tn_conv2d_dgrad", dz.ptr, W.ptr, dx.ptr, *geom, None, 0, 0.0)
    report("tn_conv2d_dgrad", case, dx)
    call("tn_conv2d_dgrad", dz.ptr, W.ptr, dx.ptr, *geom, prev.ptr, *act_code("relu10"))
    report("tn_conv2d_dgrad prev_a", case, dx)


def block(case, N, C, H, K, f, mode, act, ib, entries):
    """One fused block shape through ``entries``: the forward with and without a mask, then every backward named."""
    lib = ctx().lib
    pad, _, Ho = O.conv_geometry(H, f, 1, mode)
    Hp = O.pool_out_sz(Ho, 2, ib)
    x, W, b, g, prev = tensors(case, N, C, H, K, f, (N, K, Hp, Hp), (N, C, H, H))
    geom = (N, C, H, H, K, f, pad, Ho, Ho, 2, Hp, Hp) + act_code(act)
    y, mask = empty((N, K, Hp, Hp)), empty((N, K, Hp, Hp), np.uint8)
    dz, dx, dW, db = empty((N, K, Ho, Ho)), empty(x.shape), empty(W.shape), empty((K,))
    tile = lib.tn_convpool_tile_supported(N, C, H, H, K, f, 1, pad, Ho, Ho, 2, Hp, Hp)
    if not (tile or lib.tn_convpool_supported(C, f, 1, 2)):
        return print("%-34s %-48s unsupported" % ("tn_convpool_fwd_mask", case))
    call("tn_convpool_fwd_mask", x.ptr, W.ptr, b.ptr, y.ptr, None, *geom)
    report("tn_convpool_fwd_mask no mask", case, y)
    if f == 3:
        call("tn_convpool_fwd_mask", x.ptr, W.ptr, b.ptr, y.ptr, mask.ptr, *geom)
        report("tn_convpool_fwd_mask", case, y, mask)
    for entry in entries:
        for out in (dz if entry in ("tn_convpool_bwd", "tn_convpool_bwd_mask") else dx, None):
            tag = entry + ("" if out is not None else " dW only")
            out_ptr = out.ptr if out is not None else None
            for t in (dz, dx, dW, db):
                t.fill_bytes(0)
            if entry == "tn_convpool_bwd":
                call(entry, x.ptr, W.ptr, b.ptr, g.ptr, out_ptr, dW.ptr, db.ptr, *geom)
            elif entry == "tn_convblock_bwd":
                if not lib.tn_convblock_supported(C, K, f, 1, 2, Ho, Ho):
                    print("%-34s %-48s unsupported" % (tag, case))
                    continue
                call(entry, x.ptr, W.ptr, b.ptr, g.ptr, out_ptr, dW.ptr, db.ptr, *geom)
            elif entry == "tn_convpool_bwd_mask":
                call(entry, x.ptr, g.ptr, y.ptr, mask.ptr, out_ptr, dW.ptr, db.ptr, *geom)
            elif entry == "tn_convblock_bwd_mask":
                call(entry, x.ptr, W.ptr, g.ptr, y.ptr, mask.ptr, out_ptr, dW.ptr, db.ptr, *geom)
            else:       # tn_convpool_bwd_mask_dx: the layer below's activation gradient rides on dx
                call(entry, x.ptr, W.ptr, g.ptr, y.ptr, mask.ptr, out_ptr, dW.ptr, db.ptr, *geom, prev.ptr, *act_code("relu10"))
            report(tag, case, *([out] if out is not None else []), dW, db)


def main():
    for case in G.CONV_CASES:
        conv2d(case)
    for case in G.CONVPOOL_CASES:
        block(case, *case, entries=("tn_convpool_bwd",))
    for case in cases(G.test_convblock_lds_backward):
        block(case, *case, entries=("tn_convblock_bwd",))
    for case in cases(G.test_convblock_mask_backward):
        block(case, *case, False, entries=("tn_convblock_bwd_mask",))
    for case in cases(G.test_convpool_tile_block):
        N, C, H, K, act = case
        block(case, N, C, H, K, 3, "same", act, False, entries=("tn_convpool_bwd_mask_dx",))
    for case in cases(G.test_convpool_mask_backward):
        N, C, H, K, mode, act, ib = case
        block(case, N, C, H, K, 3, mode, act, ib, entries=("tn_convpool_bwd_mask",))


if __name__ == "__main__":
    main()
