"""Grouped convolution with narrow groups (2 or 4 maps a group in and out) on the 16-bit conv stack: tn_c8_gconv_* through
the C-ABI, float16 (gradient scale 4096) and bfloat16, against the float64 grouped convolution of the operands as stored
(tests/test_gconv_cpu.ref), by the method and with the tolerances of tests/test_gpu_gconv.py: TOL16 for stored tensors,
check_grads' bound for dW / db.  Outputs are pre-filled with garbage, dW / db with 7.

Without the feature every case fails at its first line: tn_c8_gconv_supported is 0 for groups below 8 maps."""
import numpy as np
import pytest

from tests.gpu_util import act_code, call, ctx, dev
from tests.test_gconv_cpu import SLOPE, check_grads, inputs, pad_of, ref
from tests.test_gpu_c8_conv1 import TOL16, _R, _c8, _garbage, _get
from tests.test_gpu_c8_convg import _own_the_context  # noqa: F401  (autouse: dW / db are read right after the call)
from tests.test_gpu_c8_mean import GS
from tests.test_gpu_dwconv import _close16
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

# (N, C, K, g, S, P, f, mode, stride, So, Po)
CASES = [
    (2, 8, 8, 2, 8, 8, 3, "same", 1, 8, 8),            # w 4, one cell, two groups in it
    (2, 8, 8, 4, 8, 8, 3, "same", 1, 8, 8),            # w 2, zeros inside the 4x4 block
    (3, 72, 72, 18, 7, 8, 3, "same", 1, 7, 8),         # nine cells: a full run of eight and a ragged one, pitch above side
    (2, 16, 16, 8, 10, 16, 5, "valid", 1, 6, 8),       # w 2, 5x5 'valid', output pitch differs from input pitch
    (2, 24, 24, 6, 10, 16, 3, "valid", 2, 4, 8),       # stride 2: the gather; row / column 9 in no window (dx +0)
    (2, 16, 16, 4, 12, 16, 1, "valid", 1, 12, 16),     # 1x1, no halo
    (3, 16, 16, 4, 33, 64, 3, "same", 1, 33, 64),      # several pixel tiles with halo between them, ragged last, slabs
]


@pytest.mark.parametrize("case", CASES, ids=["%dx%d-%dg%d-%d@%d-f%d%ss%d" % c[:9] for c in CASES])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_narrow_gconv_ops(dtype, case):
    N, C, K, g, S, P, f, mode, stride, So, Po = case
    pad, gs = pad_of(f, mode), GS[dtype]
    geom = (N, C, S, P, K, g, f, stride, pad, So, Po)
    ctx().set_matmul_dtype(dtype, gs)
    assert ctx().lib.tn_c8_gconv_supported(*geom) == 1
    R = _R(dtype)
    x, dzs, W, b, prev = inputs(case, R, gs)
    z, dx, dW, db, aW, ab = ref(x, R(W), b.astype(np.float64), dzs, g, stride, pad)
    close = lambda got, want, what: _close16(got, R(want), TOL16[dtype], what)
    xd, dzd, pd, Wd, bd = _c8(x, P, dtype), _c8(dzs, Po, dtype), _c8(prev, P, dtype), dev(W), dev(b)
    for name in ("relu10", "linear"):
        act, prm = act_code(name)
        y = _garbage(N, K, Po)
        call("tn_c8_gconv_fwd", xd.ptr, Wd.ptr, bd.ptr, y.ptr, *geom, act, prm)
        close(_get(y, K, So, dtype), np.where(z > 0, z, SLOPE * z) if name == "relu10" else z, "fwd " + name)
    act, prm = act_code("relu10")
    for p_, deriv in ((pd.ptr, np.where(prev > 0, 1., np.where(prev < 0, SLOPE, 1 + SLOPE))), (None, 1.)):
        o = _garbage(N, C, P)
        call("tn_c8_gconv_dgrad", dzd.ptr, Wd.ptr, o.ptr, *geom, p_, act, prm)
        close(_get(o, C, S, dtype), dx * deriv, "dgrad with prev_a" if p_ else "dgrad")
        if stride == 2:                                       # row / column 9 lie in no window: +0, the bits
            raw = np.asarray(o.get_value())
            assert not raw[:, :, 9:].view(np.uint16).any() and not raw[:, :, :, 9:].view(np.uint16).any()
    gW, gb = dev(np.full(W.shape, 7., np.float32)), dev(np.full((K,), 7., np.float32))
    call("tn_c8_gconv_wgrad", xd.ptr, dzd.ptr, gW.ptr, gb.ptr, *geom)
    check_grads(gW.get_value(), gb.get_value(), dW, db, aW, ab, N * So * So, True, gs)


@pytest.mark.parametrize("C, K, g", [(8, 16, 2), (16, 8, 4), (12, 12, 3)], ids=["4on8", "2on4", "12maps"])
def test_narrow_gconv_still_refuses(C, K, g):
    """Unequal narrow widths, and width 4 on maps that are no whole cells: unsupported, BackendError naming the entry point,
    nothing launched (the output keeps its fill)."""
    from theanet_amd import _lib
    ctx().set_matmul_dtype("bfloat16", 1.)
    geom = (2, C, 8, 8, K, g, 3, 1, 1, 8, 8)
    x, y = _c8(np.zeros((2, C, 8, 8)), 8, "bfloat16"), _garbage(2, K, 8)
    W, b = dev(np.zeros((K, C // g, 3, 3), np.float32)), dev(np.zeros((K,), np.float32))
    fill = np.asarray(y.get_value()).copy()
    assert ctx().lib.tn_c8_gconv_supported(*geom) == 0
    with pytest.raises(_lib.BackendError, match="tn_c8_gconv_fwd: bad arguments"):
        call("tn_c8_gconv_fwd", x.ptr, W.ptr, b.ptr, y.ptr, *geom, 0, 0.)
    assert np.array_equal(np.asarray(y.get_value()), fill)
