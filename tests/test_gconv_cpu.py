"""Grouped convolution (ConvLayer groups) without a GPU: the plain-loop tn_gconv_* of the C++ backend behind the same C-ABI
(THEANET_BACKEND=cpu, in a child process) against the float64 grouped convolution ``ref`` -- which tests/test_gpu_gconv.py
holds the HIP kernels to as well -- at the first, fourth and last case of its table; the tn_c8_gconv_* stubs refuse.
Tolerance: assert_close's defaults, dW / db as in the GPU test (the larger of 1e-5 + 1e-4 |want| and n u sum|terms|).

Without the feature the child fails at the first call: the library exports no tn_gconv_fwd."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "theanet_amd", "lib", "libtheanet_cpu.so")

# (N, C, K, g, S, P, f, mode, stride, So, Po)
CASES = [
    (2, 16, 16, 2, 8, 8, 3, "same", 1, 8, 8),          # base: one octet in and out per group, whole plane in one tile
    (3, 32, 16, 2, 7, 8, 3, "same", 1, 7, 8),          # two input octets per group, pitch above side, pad cells as +0
    (2, 16, 48, 2, 10, 16, 5, "valid", 1, 6, 8),       # K/g 24: a full and a ragged 16-row tile, 5x5, ragged reduction tail
    (2, 24, 24, 3, 10, 16, 3, "valid", 2, 4, 8),       # odd group count, stride 2, row / column 9 in no window (dx +0)
    (2, 64, 64, 2, 12, 16, 1, "valid", 1, 12, 16),     # 1x1 grouped, K/g 32, no halo
    (3, 16, 32, 2, 33, 64, 3, "same", 1, 33, 64),      # several pixel tiles with halo between them, ragged last, slabs
    (2, 16, 32, 2, 10, 16, 3, "valid", 2, 4, 8),       # stride 2 with K/g 16: the strided gather on the matrix-core forms
    (2, 6, 9, 3, 9, 9, 3, "valid", 1, 7, 7),           # float32 only: groups of 2 maps and 3 filters
]
SLOPE = .1


def pad_of(f, mode):
    return f - 1 - (f - 1) // 2 if mode == "same" else 0


def ref(x, W, b, dz, g, stride, pad):
    """float64: z, dx (before act'), dW, db of z[n,k] = b[k] + sum over the maps c of k's group and the taps of
    xpad[n,c,i s+u,j s+v] W[k,c,f-1-u,f-1-v]; and the sums of absolute terms of dW and db."""
    N, C, S, _ = x.shape
    K, Cg, f, _ = W.shape
    Kg, So = K // g, dz.shape[-1]
    xp = np.zeros((N, C, S + 2 * f, S + 2 * f))
    xp[:, :, pad:pad + S, pad:pad + S] = x
    z, dxp, dW, aW = np.zeros(dz.shape) + b[None, :, None, None], np.zeros(xp.shape), np.zeros(W.shape), np.zeros(W.shape)
    for grp in range(g):
        cs, ks = slice(grp * Cg, (grp + 1) * Cg), slice(grp * Kg, (grp + 1) * Kg)
        for u in range(f):
            for v in range(f):
                at = (slice(u, u + stride * So, stride), slice(v, v + stride * So, stride))
                win, w = xp[(slice(None), cs) + at], W[ks, :, f - 1 - u, f - 1 - v]
                z[:, ks] += np.einsum("ncij,kc->nkij", win, w)
                dxp[(slice(None), cs) + at] += np.einsum("nkij,kc->ncij", dz[:, ks], w)
                dW[ks, :, f - 1 - u, f - 1 - v] = np.einsum("nkij,ncij->kc", dz[:, ks], win)
                aW[ks, :, f - 1 - u, f - 1 - v] = np.einsum("nkij,ncij->kc", np.abs(dz[:, ks]), np.abs(win))
    return z, dxp[:, :, pad:pad + S, pad:pad + S], dW, dz.sum((0, 2, 3)), aW, np.abs(dz).sum((0, 2, 3))


def check_grads(gW, gb, dW, db, aW, ab, n_terms, c8, gs=1.):
    """dW / db within the larger of the project's bound and n u sum|terms| (u = 2^-24)."""
    n_u = n_terms * 2.0 ** -24
    for what, got, want, absum in (("dW", gW, dW / gs, aW / gs), ("db", gb, db / gs, ab / gs)):
        own = 2e-5 * np.abs(want).max() if c8 else 1e-5 + 1e-4 * np.abs(want)
        err, bound = np.abs(got - want), np.maximum(own, n_u * absum)
        print("%s: max err %.3g, smallest bound %.3g" % (what, err.max(), bound.min()))
        assert (err <= bound).all(), (what, err.max())


def inputs(case, R, gs=1.):
    N, C, K, g, S, P, f, mode, stride, So, Po = case
    rng = np.random.RandomState(0)
    x, dzs = R(rng.randn(N, C, S, S)), R(gs * rng.randn(N, K, So, So) * 1e-3)
    W = (rng.randn(K, C // g, f, f) / f).astype(np.float32)
    b = (rng.randn(K) * .1).astype(np.float32)
    prev = R(rng.randn(N, C, S, S))
    prev[0, 0, 0, :2] = 0                                     # the tie derivative
    return x, dzs, W, b, prev


def child():
    """Runs in the child process, on the CPU backend."""
    from tests.gpu_util import act_code, assert_close, call, ctx, dev
    from theanet_amd import _lib
    R = lambda a: np.asarray(a, np.float32).astype(np.float64)
    for case in (CASES[0], CASES[3], CASES[-1]):
        N, C, K, g, S, P, f, mode, stride, So, Po = case
        pad = pad_of(f, mode)
        x, dzs, W, b, prev = inputs(case, R)
        z, dx, dW, db, aW, ab = ref(x, R(W), b.astype(np.float64), dzs, g, stride, pad)
        geom = (N, C, S, S, K, g, f, stride, pad, So, So)
        assert ctx().lib.tn_gconv_supported(*geom) and not ctx().lib.tn_c8_gconv_supported(N, C, S, P, K, g, f, stride, pad, So, Po)
        xd, dzd, pd, Wd, bd = (dev(a.astype(np.float32)) for a in (x, dzs, prev, W, b))
        act, prm = act_code("relu10")
        y, o = dev(np.full(z.shape, 7., np.float32)), dev(np.full(x.shape, 7., np.float32))
        call("tn_gconv_fwd", xd.ptr, Wd.ptr, bd.ptr, y.ptr, *geom, act, prm)
        assert_close(y.get_value(), np.where(z > 0, z, SLOPE * z), what="fwd")
        call("tn_gconv_dgrad", dzd.ptr, Wd.ptr, o.ptr, *geom, pd.ptr, act, prm)
        assert_close(o.get_value(), dx * np.where(prev > 0, 1., np.where(prev < 0, SLOPE, 1 + SLOPE)), what="dgrad")
        gW, gb = dev(np.full(W.shape, 7., np.float32)), dev(np.full((K,), 7., np.float32))
        call("tn_gconv_wgrad", xd.ptr, dzd.ptr, gW.ptr, gb.ptr, *geom)
        check_grads(gW.get_value(), gb.get_value(), dW, db, aW, ab, N * So * So, False)
    c8_geom = (N, C, S, P, K, g, f, stride, pad, So, Po)
    for name, args in (("tn_c8_gconv_fwd", (xd.ptr, Wd.ptr, bd.ptr, y.ptr) + c8_geom + (act, prm)),
                       ("tn_c8_gconv_dgrad", (dzd.ptr, Wd.ptr, o.ptr) + c8_geom + (None, act, prm)),
                       ("tn_c8_gconv_wgrad", (xd.ptr, dzd.ptr, gW.ptr, gb.ptr) + c8_geom)):
        with pytest.raises(_lib.BackendError, match=name):
            call(name, *args)
    print("GCONV CPU OK")


@pytest.mark.skipif(not os.path.isfile(CPU_LIB), reason="libtheanet_cpu.so not built")
def test_gconv_on_the_cpu_backend():
    env = dict(os.environ, THEANET_BACKEND="cpu", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", "from tests.test_gconv_cpu import child; child()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "GCONV CPU OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
