"""ConvLayers of any filter, mode and stride on the 16-bit-resident conv stack (CONV_SHAPES 'any'): the ops
tn_c8_convg_fwd / tn_c8_convg_dgrad / tn_c8_convg_wgrad through the C-ABI, in both element types, against the oracle's
stored-16-bit statement of a general conv (oracle.theanet_oracle.conv2d_fwd / conv2d_bwd with f16=True; for bf16 the
oracle's rounding is swapped as in tests/test_gpu_c8_conv1.py).  Activation and the store rounding are applied as in that
file's _ops.  Every output is pre-filled with garbage (0x5555): an op must write every cell, pad cells and channels past
the last as exact +0.

Tolerances are the project's own for this arithmetic (operands rounded to the 16-bit type, exact products, fp32
accumulation, one rounding on store): stored 16-bit tensors 1e-3 of the largest entry for fp16 and 1e-2 for bf16, fp32
results (dW, db) 2e-5 of the largest entry (tests/test_gpu_c8_conv1.py).

Fails on a build without the general family: tn_c8_convg_fwd is not exported.  tests/test_c8g_dispatch.py proves on
the CPU that CASES reach every instantiation of the three kernels and every edge."""
import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests.gpu_util import call, ctx, dev, empty
from tests.test_gpu_c8_conv1 import TOL16, _R, _act, _act_grad_from_out, _c8, _code, _garbage, _get, _rel
from tests.test_gpu_c8_conv1 import dtype  # noqa: F401  (fixture: the element type, the oracle's rounding swapped for bf16)
from tests.test_gpu_c8_mean import GS
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _own_the_context():
    """These tests call the C-ABI directly and read dW / db right after the call.  A pipelined training function of an
    earlier test module may have left a step's slab sums parked with its stream (an open tn_defer_reductions window):
    inside it a weight-gradient op only RECORDS its sum.  Take the context over as a net does (NeuralNet._apply_dtype,
    tests/test_gpu_convblock_bwd_loops.py): finish what a living net parked, forget what a dead one did."""
    from theanet_amd.neuralnet import NeuralNet
    ref = NeuralNet._ctx_owner
    prev = ref() if ref is not None else None
    if prev is not None and prev._pipe_fn is not None:
        prev._pipe_fn._flush_parked()
    elif ref is not None:
        call("tn_defer_discard")
    NeuralNet._ctx_owner = None
    yield


# (N, C, S, P, K, f, stride, mode, So, Po)
CASES = [
    (3, 1, 28, 32, 4, 3, 1, "valid", 26, 32),        # 1  mnist conv1, one channel, K < 8
    (3, 4, 13, 16, 20, 3, 1, "valid", 11, 16),       # 2  mnist conv2, padded in and out, K = 2.5 octets
    (2, 3, 12, 16, 10, 5, 1, "valid", 8, 8),         # 3  pitch shrinks
    (2, 8, 8, 8, 16, 5, 1, "same", 8, 8),            # 4  pad 2
    (2, 9, 8, 8, 12, 4, 1, "same", 8, 8),            # 5  even filter, pad 2 low / 1 high, ragged second octet
    (2, 16, 10, 16, 8, 3, 2, "valid", 4, 8),         # 6  stride 2
    (2, 5, 13, 16, 9, 4, 2, "valid", 5, 8),          # 7  stride with an even filter
    (2, 8, 10, 16, 8, 2, 3, "valid", 3, 8),          # 8  stride > f: dx has untouched pixels that must be +0
    (2, 16, 8, 8, 8, 1, 2, "valid", 4, 8),           # 9  1x1 strided
    (2, 8, 16, 16, 20, 3, 1, "same", 16, 16),        # 10 the 3x3 the tiled family refuses for K % 8
    (2, 20, 9, 16, 24, 3, 1, "same", 9, 16),         # 11 three input octets, the last ragged
    (2, 8, 4, 8, 16, 4, 1, "valid", 1, 8),           # 12 filter as large as the map
    (1, 3, 72, 72, 8, 5, 1, "valid", 68, 68),        # 13 dense maps above 64
    (300, 4, 13, 16, 20, 3, 1, "valid", 11, 16),     # 14 many tiles with a partial last one
    (70, 3, 12, 16, 10, 5, 1, "valid", 8, 8),        # 15 several wgrad slabs
    (2, 40, 6, 8, 72, 3, 1, "same", 6, 8),           # 16 several 32-row tiles (forward and input gradient), two filter groups
    (2, 40, 8, 8, 8, 3, 2, "valid", 3, 8),           # 17 ... of the strided input gradient
]
IDS = ["%d-%dx%dx%d@%d-k%d-f%ds%d%s" % ((i + 1,) + c[:8]) for i, c in enumerate(CASES)]
GENERIC = [0, 1, 4, 5, 7]
ACT_NAMES = ("leaky", "tanh", "linear")


def pad_lo(f, mode):
    """ConvLayer's low padding (theanet_amd/layer/convpool.py)."""
    return f - 1 - (f - 1) // 2 if mode == "same" else 0


def geom(case):
    """The geometry arguments of the three entry points."""
    N, C, S, P, K, f, stride, mode, So, Po = case
    return N, C, S, P, K, f, stride, pad_lo(f, mode), So, Po


def convg_launches():
    """Every (op, geometry, activation code) the per-op tests below launch -- what tests/test_c8g_dispatch.py classifies."""
    out = []
    for i, case in enumerate(CASES):
        for name in ACT_NAMES if i in GENERIC else ACT_NAMES[:1]:
            out.append((0, geom(case), name))
            out.append((1, geom(case), name))
        out.append((2, geom(case), "leaky"))
    return out


def _check(figs):
    """Every figure printed, then every bound asserted."""
    for what, e, tol in figs:
        print("%s: %.3g (bound %g)" % (what, e, tol))
    for what, e, tol in figs:
        assert e < tol, (what, e, tol)


def _ops(case, name, dtype, wgrad):
    N, C, S, P, K, f, stride, mode, So, Po = case
    g = geom(case)
    R, tol, gs = _R(dtype), TOL16[dtype], GS[dtype]
    act, prm = _code(name)
    assert ctx().lib.tn_c8_convg_supported(*g)
    rng = np.random.RandomState(0)
    x = R(rng.randn(N, C, S, S))
    W = (rng.randn(K, C, f, f) / np.sqrt(C * f * f)).astype(np.float32)
    b = (rng.randn(K) * .1).astype(np.float32)
    z = O.conv2d_fwd(x, W.astype(np.float64), b.astype(np.float64), stride, mode, f16=True)
    assert z.shape == (N, K, So, So)
    a = _act(name, z)
    xd, Wd, bd = _c8(x, P, dtype), dev(W), dev(b)
    # forward
    out = _garbage(N, K, Po)
    call("tn_c8_convg_fwd", xd.ptr, Wd.ptr, bd.ptr, out.ptr, *g, act, prm)
    figs = [("fwd", _rel(_get(out, K, So, dtype), R(a)), tol)]
    # gradients: dz as stored (it carries the gradient scale); prev_a given (exact zeros planted: the tie derivative)
    dzs = R(gs * rng.randn(N, K, So, So) * 1e-3)
    if name in ("leaky", "linear"):
        prev = R(rng.randn(N, C, S, S))
        prev[0, 0, 0, :2] = 0
    else:
        prev = R(_act(name, 2 * rng.randn(N, C, S, S)))
    dx, dW, db = O.conv2d_bwd(x, W.astype(np.float64), dzs / gs, stride, mode, need_dx=True, f16=True, grad_scale=gs)
    lin = gs * dx
    dzd, pd = _c8(dzs, Po, dtype), _c8(prev, P, dtype)
    dxo = _garbage(N, C, P)
    call("tn_c8_convg_dgrad", dzd.ptr, Wd.ptr, dxo.ptr, *g, pd.ptr, act, prm)
    figs.append(("dgrad", _rel(_get(dxo, C, S, dtype), R(lin * _act_grad_from_out(name, prev))), tol))
    dxo = _garbage(N, C, P)
    call("tn_c8_convg_dgrad", dzd.ptr, Wd.ptr, dxo.ptr, *g, None, act, prm)
    figs.append(("dgrad, no derivative", _rel(_get(dxo, C, S, dtype), R(lin)), tol))
    if stride > f:                         # pixels no window touches: exact +0 (the bits, not just the value)
        untouched = np.ones(P, bool)          # (rows / columns of the stored plane: the pad ones included)
        for i in range(So):
            untouched[i * stride:i * stride + f] = False
        assert untouched[:S].any()
        raw = dxo.get_value()
        assert not raw[:, :, untouched].any() and not raw[:, :, :, untouched].any()
    if not wgrad:
        return _check(figs)
    # weight / bias gradient (fp32, the scale removed); OVERWRITE
    gW, gb = dev(np.full((K, C, f, f), 7., np.float32)), dev(np.full((K,), 7., np.float32))
    call("tn_c8_convg_wgrad", xd.ptr, dzd.ptr, gW.ptr, gb.ptr, *g)
    figs += [("dW", _rel(gW.get_value(), dW), 2e-5), ("db", _rel(gb.get_value(), db), 2e-5)]
    _check(figs)
    # the same input twice: the same bits
    g2, b2 = empty((K, C, f, f)), empty((K,))
    call("tn_c8_convg_wgrad", xd.ptr, dzd.ptr, g2.ptr, b2.ptr, *g)
    np.testing.assert_array_equal(gW.get_value().view(np.uint32), g2.get_value().view(np.uint32))
    np.testing.assert_array_equal(gb.get_value().view(np.uint32), b2.get_value().view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_c8_convg_ops_match_oracle(dtype, case):
    """Forward, input gradient with and without prev_a, weight gradient (and twice: the same bits), leaky-ReLU (relu10)."""
    _ops(case, "leaky", dtype, True)


@pytest.mark.parametrize("name", ACT_NAMES[1:])
@pytest.mark.parametrize("case", [CASES[i] for i in GENERIC], ids=[IDS[i] for i in GENERIC])
def test_c8_convg_ops_generic_activation(dtype, case, name):
    _ops(case, name, dtype, False)


def test_c8_convg_ops_refuse_bad_arguments():
    """NULL tensors, an inconsistent So, a bad pitch and f > S + padding: BackendError naming the entry point, and the
    outputs still hold the garbage (nothing was launched)."""
    from theanet_amd import _lib
    ctx().set_matmul_dtype("float16", 4096.)
    lib = ctx().lib
    x = dev(np.zeros((2, 1, 16, 16, 8), np.uint16))
    y = dev(np.full((2, 1, 16, 16, 8), 0x5555, np.uint16))
    W, b = dev(np.full((8, 8, 7, 7), 7., np.float32)), dev(np.full((8,), 7., np.float32))
    ok = (2, 8, 12, 16, 8, 3, 1, 0, 10, 16)
    assert lib.tn_c8_convg_supported(*ok)
    bad = {"So too large": (2, 8, 12, 16, 8, 3, 1, 0, 11, 16), "So too small": (2, 8, 12, 16, 8, 3, 1, 0, 9, 16),
           "strided So": (2, 8, 12, 16, 8, 3, 2, 0, 4, 8), "pitch below the side": (2, 8, 12, 8, 8, 3, 1, 0, 10, 16),
           "pitch no power of two": (2, 8, 12, 24, 8, 3, 1, 0, 10, 16), "output pitch": (2, 8, 12, 16, 8, 3, 1, 0, 10, 12),
           "f > S + padding": (2, 8, 4, 8, 8, 7, 1, 0, 1, 8), "pad above f / 2": (2, 8, 12, 16, 8, 3, 1, 2, 12, 16),
           "N": (0, 8, 12, 16, 8, 3, 1, 0, 10, 16), "C": (2, 0, 12, 16, 8, 3, 1, 0, 10, 16),
           "K": (2, 8, 12, 16, 0, 3, 1, 0, 10, 16), "f": (2, 8, 12, 16, 8, 0, 1, 0, 13, 16),
           "stride": (2, 8, 12, 16, 8, 3, 0, 0, 10, 16)}
    for why, g in bad.items():
        assert not lib.tn_c8_convg_supported(*g), why
        with pytest.raises(_lib.BackendError, match="tn_c8_convg_fwd: bad arguments"):
            call("tn_c8_convg_fwd", x.ptr, W.ptr, b.ptr, y.ptr, *g, 0, 0.)
        with pytest.raises(_lib.BackendError, match="tn_c8_convg_dgrad: bad arguments"):
            call("tn_c8_convg_dgrad", x.ptr, W.ptr, y.ptr, *g, None, 0, 0.)
        with pytest.raises(_lib.BackendError, match="tn_c8_convg_wgrad: bad arguments"):
            call("tn_c8_convg_wgrad", x.ptr, x.ptr, W.ptr, b.ptr, *g)
    for args in ((None, W.ptr, b.ptr, y.ptr), (x.ptr, None, b.ptr, y.ptr), (x.ptr, W.ptr, None, y.ptr), (x.ptr, W.ptr, b.ptr, None)):
        with pytest.raises(_lib.BackendError, match="tn_c8_convg_fwd: bad arguments"):
            call("tn_c8_convg_fwd", *args, *ok, 0, 0.)
    for args in ((None, W.ptr, y.ptr), (x.ptr, None, y.ptr), (x.ptr, W.ptr, None)):
        with pytest.raises(_lib.BackendError, match="tn_c8_convg_dgrad: bad arguments"):
            call("tn_c8_convg_dgrad", *args, *ok, None, 0, 0.)
    for args in ((None, x.ptr, W.ptr, b.ptr), (x.ptr, None, W.ptr, b.ptr), (x.ptr, x.ptr, None, b.ptr), (x.ptr, x.ptr, W.ptr, None)):
        with pytest.raises(_lib.BackendError, match="tn_c8_convg_wgrad: bad arguments"):
            call("tn_c8_convg_wgrad", *args, *ok)
    assert (y.get_value() == 0x5555).all() and (W.get_value() == 7.).all() and (b.get_value() == 7.).all()
