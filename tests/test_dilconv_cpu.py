"""Dilated convolution (ConvLayer dilation) without a GPU: the case table, the float64 reference ``dil_ref`` -- W zero-stuffed
to the window fe = (f - 1) d + 1 and handed to the dense loops of tests/test_gconv_cpu.ref at g = 1 --, the plain-loop
tn_dilconv_* of the C++ backend behind the same C-ABI (THEANET_BACKEND=cpu, in a child process) against it at the first,
the fourth and the d = 2 narrow case, the tn_c8_dilconv_* stubs, and the constructor's refusals.
Tolerance: assert_close's defaults, dW / db as in the GPU test (the larger of 1e-5 + 1e-4 |want| and n u sum|terms|).

Without the feature the child fails at the first call (the library exports no tn_dilconv_fwd) and ConvLayer takes no
``dilation`` keyword."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gconv_cpu import CPU_LIB, ROOT, SLOPE, check_grads, inputs, ref

# (N, C, K, S, P, f, d, mode, So, Po)
CASES = [
    (2, 16, 16, 9, 16, 3, 2, "same", 9, 16),          # So no multiple of d: ragged phases; padded planes
    (2, 16, 16, 9, 16, 3, 2, "valid", 5, 8),
    (2, 8, 24, 8, 8, 2, 3, "same", 8, 8),             # fe 4: padding 2 / 1, no multiple of d, phases shifted against the pad
    (2, 8, 24, 8, 8, 2, 3, "valid", 5, 8),
    (2, 8, 8, 6, 8, 3, 4, "same", 6, 8),              # fe 9 > S: phases of one or two outputs, taps wholly in the padding
    (1, 40, 32, 20, 32, 3, 2, "same", 20, 32),        # several tiles a phase, the 32-row form, a ragged channel tail
    (1, 256, 256, 12, 16, 3, 4, "same", 12, 16),      # 256 maps on 3x3 phase planes: waves over row tiles
    (1, 256, 16, 20, 32, 5, 2, "same", 20, 32),       # 256 maps under a 5x5 halo tile: the maps go through LDS in chunks
    (3, 4, 6, 7, 8, 5, 1, "same", 7, 8),              # float32 only: the register-tiled form; d = 1 is the dense layer
    (3, 4, 6, 7, 8, 5, 2, "same", 7, 8),              # float32 only
]


def pad_of(f, d, mode):
    fe = (f - 1) * d + 1
    return fe - 1 - (fe - 1) // 2 if mode == "same" else 0


def as_gconv(case):
    """The case as tests/test_gconv_cpu.inputs reads one (one group, stride 1)."""
    N, C, K, S, P, f, d, mode, So, Po = case
    return (N, C, K, 1, S, P, f, mode, 1, So, Po)


def dil_ref(x, W, b, dz, d, pad):
    """test_gconv_cpu.ref of the zero-stuffed dense layer; dW and its sum of absolute terms at the taps W has."""
    K, C, f, _ = W.shape
    Wd = np.zeros((K, C, (f - 1) * d + 1, (f - 1) * d + 1))
    Wd[:, :, ::d, ::d] = W
    z, dx, dW, db, aW, ab = ref(x, Wd, b, dz, 1, 1, pad)
    return z, dx, dW[:, :, ::d, ::d], db, aW[:, :, ::d, ::d], ab


def child():
    """Runs in the child process, on the CPU backend."""
    from tests.gpu_util import act_code, assert_close, call, ctx, dev
    from theanet_amd import _lib
    R = lambda a: np.asarray(a, np.float32).astype(np.float64)
    for case in (CASES[0], CASES[3], CASES[-1]):
        N, C, K, S, P, f, d, mode, So, Po = case
        pad = pad_of(f, d, mode)
        x, dzs, W, b, prev = inputs(as_gconv(case), R)
        z, dx, dW, db, aW, ab = dil_ref(x, R(W), b.astype(np.float64), dzs, d, pad)
        geom = (N, C, S, S, K, d, f, 1, pad, So, So)
        assert ctx().lib.tn_dilconv_supported(*geom) and not ctx().lib.tn_c8_dilconv_supported(N, C, S, P, K, d, f, 1, pad, So, Po)
        xd, dzd, pd, Wd, bd = (dev(a.astype(np.float32)) for a in (x, dzs, prev, W, b))
        act, prm = act_code("relu10")
        y, o = dev(np.full(z.shape, 7., np.float32)), dev(np.full(x.shape, 7., np.float32))
        call("tn_dilconv_fwd", xd.ptr, Wd.ptr, bd.ptr, y.ptr, *geom, act, prm)
        assert_close(y.get_value(), np.where(z > 0, z, SLOPE * z), what="fwd")
        call("tn_dilconv_dgrad", dzd.ptr, Wd.ptr, o.ptr, *geom, pd.ptr, act, prm)
        assert_close(o.get_value(), dx * np.where(prev > 0, 1., np.where(prev < 0, SLOPE, 1 + SLOPE)), what="dgrad")
        gW, gb = dev(np.full(W.shape, 7., np.float32)), dev(np.full((K,), 7., np.float32))
        call("tn_dilconv_wgrad", xd.ptr, dzd.ptr, gW.ptr, gb.ptr, *geom)
        check_grads(gW.get_value(), gb.get_value(), dW, db, aW, ab, N * So * So, False)
    c8_geom = (N, C, S, P, K, d, f, 1, pad, So, Po)
    for name, args in (("tn_c8_dilconv_fwd", (xd.ptr, Wd.ptr, bd.ptr, y.ptr) + c8_geom + (act, prm)),
                       ("tn_c8_dilconv_dgrad", (dzd.ptr, Wd.ptr, o.ptr) + c8_geom + (None, act, prm)),
                       ("tn_c8_dilconv_wgrad", (xd.ptr, dzd.ptr, gW.ptr, gb.ptr) + c8_geom)):
        with pytest.raises(_lib.BackendError, match=name):
            call(name, *args)
    print("DILCONV CPU OK")


@pytest.mark.skipif(not os.path.isfile(CPU_LIB), reason="libtheanet_cpu.so not built")
def test_dilconv_on_the_cpu_backend():
    env = dict(os.environ, THEANET_BACKEND="cpu", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", "from tests.test_dilconv_cpu import child; child()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DILCONV CPU OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("kw, says", [({"dilation": 0}, "dilation must be an integer >= 1"),
                                      ({"dilation": 2, "stride": 2}, "takes stride 1"),
                                      ({"dilation": 2, "depthwise": True, "num_maps": 8}, "dilation > 1 or depthwise"),
                                      ({"dilation": 2, "groups": 2}, "dilation > 1 or groups")],
                         ids=["zero", "stride", "depthwise", "groups"])
def test_dilated_constructor_refuses(kw, says):
    """The refusals come before anything is allocated: no device needed."""
    from theanet_amd.layer import ConvLayer
    args = dict({"num_maps": 16, "filter_sz": 3, "stride": 1}, **kw)
    with pytest.raises(AssertionError, match=says):
        ConvLayer(None, None, np.random.RandomState(0), 16, 8, 12, mode="valid", **args)
