"""The bf16-RESIDENT kernels of DTYPE 'bfloat16' (tn_set_matmul_dtype mode 2), op by op through the C-ABI: every test of
tests/test_gpu_c8.py over the same case lists, with bf16 cells in place of halfs -- c8 conv forward (+ fused 2x2
max-pool and mask), input gradient (plain and gathered from a pooled gradient + mask), weight gradient (plain and
gathered), the generic activations, 128-pixel rows, the rolling-ring weight-gradient cases, the dense products on a c8
input, pack / unpack, the elastic stage's c8 output, and unsupported shapes as errors.

Specification = the stored-bf16 arithmetic restated in numpy (tests/c8b_util.py): operands rounded to bf16 (nearest
even), products exact, float64 sums standing in for the device's fp32 accumulation, one rounding to bf16 when a tensor
is stored.  Tolerances: a stored bf16 tensor may differ by one rounding where the fp32 and the float64 sums fall on
different sides of a rounding boundary -- one bf16 ulp is at most 2^-7 = 7.8e-3 of the value: 1e-2 of the largest
entry; fp32 results (weight / bias gradients, dense outputs): 2e-5 of the largest entry, as for fp16 (a product of two
bf16 values is exact in fp32, so only the accumulation order differs); pooling masks bit-exact except at provable
near-ties (tests/test_gpu_c8.py's check: its fp32 accumulation bound holds for exact bf16 products as well); pack and the
elastic stage bit-exact against rbf16 of the fp32 values (tests/test_c8_bf16_cpu.py ties rbf16 to torch's bf16
rounding).  The reference itself is float32-only (weights.py:8)."""
import numpy as np
import pytest

from tests import c8_util as U
from tests import c8b_util as B
from tests.gpu_util import ctx, dev, empty, call
from tests.test_gpu_c8 import (ACTS, C8_ACT_NAMES, C8_CASES, C8_FWD_CASES, C8_GENERIC_ACTS, LEAKY, SLOPE,
                               WGRAD_RING_CASES, _act, _act_grad_from_out, _assert_masks_equal_up_to_provable_near_ties,
                               _rel, _rowmap, _wgrad_blas)
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

GS = 1024.0
TOL16 = 1e-2            # stored bf16 tensors: one bf16 ulp of the largest entry
R = B.rbf16


@pytest.fixture
def bf16_mode():
    ctx().set_matmul_dtype("bfloat16", GS)
    assert ctx().lib.tn_get_matmul_dtype(ctx().h) == 2
    yield
    ctx().set_matmul_dtype("float32")


def _c8(a):
    return dev(B.to_c8(a))


def _get(arr, C):
    return B.from_c8(arr.get_value(), C)


def _conv_fwd_dgrad(case, name):
    """tests/test_gpu_c8.py's _conv_fwd_dgrad in bf16: the four conv products of one shape with the epilogue's
    activation `name`.  Returns what the weight gradient of the same layer reads."""
    N, C, H, K = case
    act, prm = ACTS[name]
    rng = np.random.RandomState(0)
    x = R(rng.randn(N, C, H, H))
    W = (rng.randn(K, C, 3, 3) / np.sqrt(9 * C)).astype(np.float32)
    b = (rng.randn(K) * .1).astype(np.float32)
    W16 = R(W)
    a = _act(name, U.conv_same(x, W16) + b[None, :, None, None])
    xd, Wd, bd = _c8(x), dev(W), dev(b)
    K8, C8, Hp = K // 8, (C + 7) // 8, H // 2
    out = empty((N, K8, H, H, 8), np.uint16)
    call("tn_c8_conv_fwd", xd.ptr, Wd.ptr, bd.ptr, out.ptr, None, N, C, H, H, K, act, prm, 0, None)
    assert _rel(_get(out, K), R(a)) < TOL16
    pm, bits = U.pool2(a)
    outp, mk = empty((N, K8, Hp, Hp, 8), np.uint16), empty((N, K8, Hp, Hp, 8), np.uint8)
    call("tn_c8_conv_fwd", xd.ptr, Wd.ptr, bd.ptr, outp.ptr, mk.ptr, N, C, H, H, K, act, prm, 1, None)
    assert _rel(_get(outp, K), R(pm)) < TOL16
    gotm = mk.get_value().transpose(0, 1, 4, 2, 3).reshape(N, K, Hp, Hp)
    _assert_masks_equal_up_to_provable_near_ties(gotm, bits, a, x, W16, b, C, 0. if name == "leaky" else 2.0 ** -21)
    dz = R(GS * rng.randn(N, K, H, H) * 1e-3)
    if name == "leaky":
        prev = R(rng.randn(N, C, H, H))
        prev[0, 0, 0, :2] = 0                          # exact zeros: the tie derivative 1 + slope
    else:
        prev = R(_act(name, 2 * rng.randn(N, C, H, H)))
    dxw = U.conv_same_dgrad(dz, W16) * _act_grad_from_out(name, prev)
    dzd, pd = _c8(dz), _c8(prev)
    dxo = empty((N, C8, H, H, 8), np.uint16)
    call("tn_c8_conv_dgrad", dzd.ptr, Wd.ptr, dxo.ptr, N, C, H, H, K, pd.ptr, act, prm, 0, None, None)
    assert _rel(_get(dxo, C), R(dxw)) < TOL16
    g = R(GS * rng.randn(N, K, Hp, Hp) * 1e-3)
    gd = _c8(g)
    dzp = U.unpool_dz(g, gotm)
    call("tn_c8_conv_dgrad", gd.ptr, Wd.ptr, dxo.ptr, N, C, H, H, K, pd.ptr, act, prm, 1, mk.ptr, None)
    dxw2 = U.conv_same_dgrad(dzp, W16) * _act_grad_from_out(name, prev)
    assert _rel(_get(dxo, C), R(dxw2)) < TOL16
    return x, xd, dz, dzd, gd, dzp, mk


@pytest.mark.parametrize("case", C8_CASES)
def test_c8_bf16_conv_ops(case, bf16_mode):
    """The four conv products with the leaky-ReLU epilogue against the stored-bf16 specification, and the weight
    gradient, plain and gathered from a pooled gradient."""
    N, C, H, K = case
    lib = ctx().lib
    assert lib.tn_c8_conv_supported(N, C, H, H, K, 3, 1, 1) and lib.tn_c8_conv_wgrad_supported(N, C, H, H, K)
    x, xd, dz, dzd, gd, dzp, mk = _conv_fwd_dgrad(case, "leaky")
    gW, gb = empty((K, C, 3, 3)), empty((K,))
    for pooled, src, dzz in ((0, dzd, dz), (1, gd, dzp)):
        call("tn_c8_conv_wgrad", xd.ptr, src.ptr, gW.ptr, gb.ptr, N, C, H, H, K, pooled, mk.ptr if pooled else None)
        assert _rel(gW.get_value(), _wgrad_blas(x, dzz) / GS) < 2e-5
        assert _rel(gb.get_value(), dzz.sum(axis=(0, 2, 3)) / GS) < 2e-5


@pytest.mark.parametrize("name", C8_GENERIC_ACTS)
@pytest.mark.parametrize("case", C8_CASES)
def test_c8_bf16_conv_ops_generic_activation(case, name, bf16_mode):
    N, C, H, K = case
    assert ctx().lib.tn_c8_conv_supported(N, C, H, H, K, 3, 1, 1)
    _conv_fwd_dgrad(case, name)


@pytest.mark.parametrize("name", C8_ACT_NAMES)
@pytest.mark.parametrize("case", C8_FWD_CASES)
def test_c8_bf16_conv_ops_128_pixel_rows(case, name, bf16_mode):
    N, C, H, K = case
    lib = ctx().lib
    assert lib.tn_c8_conv_supported(N, C, H, H, K, 3, 1, 1) and not lib.tn_c8_conv_wgrad_supported(N, C, H, H, K)
    _conv_fwd_dgrad(case, name)


@pytest.mark.parametrize("case", WGRAD_RING_CASES)
def test_c8_bf16_wgrad_rolling_ring_over_many_tiles(case, bf16_mode):
    N, C, H, K = case
    rng = np.random.RandomState(11)
    assert ctx().lib.tn_c8_conv_wgrad_supported(N, C, H, H, K)
    x = R(rng.randn(N, C, H, H))
    dz = R(GS * rng.randn(N, K, H, H) * 1e-3)
    Hp = H // 2
    g = R(GS * rng.randn(N, K, Hp, Hp) * 1e-3)
    bits = rng.randint(1, 16, (N, K, Hp, Hp)).astype(np.uint8)
    mk = dev(np.ascontiguousarray(bits.reshape(N, K // 8, 8, Hp, Hp).transpose(0, 1, 3, 4, 2)))
    dzp = U.unpool_dz(g, bits)
    xd, dzd, gd = _c8(x), _c8(dz), _c8(g)
    gW, gb = empty((K, C, 3, 3)), empty((K,))
    for pooled, src, dzz in ((0, dzd, dz), (1, gd, dzp)):
        call("tn_c8_conv_wgrad", xd.ptr, src.ptr, gW.ptr, gb.ptr, N, C, H, H, K, pooled, mk.ptr if pooled else None)
        assert _rel(gW.get_value(), _wgrad_blas(x, dzz) / GS) < 2e-5
        assert _rel(gb.get_value(), dzz.sum(axis=(0, 2, 3)) / GS) < 2e-5


def test_c8_bf16_generic_activation_and_pack_roundtrip(bf16_mode):
    """tanh through the generic epilogue; pack rounds fp32 to bf16 exactly as rbf16 does, unpack is exact."""
    from theanet_amd.layer.layer import activation_by_name
    N, C, H, K = 3, 16, 16, 24
    rng = np.random.RandomState(3)
    x = R(rng.randn(N, C, H, H))
    W = (rng.randn(K, C, 3, 3) / 12).astype(np.float32)
    b = (rng.randn(K) * .1).astype(np.float32)
    act = activation_by_name("tanh")
    out = empty((N, K // 8, H, H, 8), np.uint16)
    call("tn_c8_conv_fwd", _c8(x).ptr, dev(W).ptr, dev(b).ptr, out.ptr, None, N, C, H, H, K, act.kind, act.prm, 0, None)
    want = np.tanh(U.conv_same(x, R(W)) + b[None, :, None, None])
    assert _rel(_get(out, K), R(want)) < TOL16
    data = rng.randn(N + 2, 3, H, H).astype(np.float32)
    data[0, 0, 0, :4] = [1e30, -3e38, 1.00390625, 1.01171875]      # (beyond fp16's range; exact ties to even)
    data[2, 0, 0, :2] = [1e30, 1.00390625]
    packed = empty((N, 1, H, H, 8), np.uint16)
    call("tn_c8_pack", dev(data).ptr, 2, packed.ptr, N, 3, H * H, 2.0)
    raw = packed.get_value()
    np.testing.assert_array_equal(B.from_c8(raw, 3), R(2.0 * data[2:].astype(np.float64)).astype(np.float32))
    assert not raw[..., 3:].any()
    back = empty((N, 3, H, H))
    call("tn_c8_unpack", packed.ptr, back.ptr, N, 3, H * H, .5)
    np.testing.assert_array_equal(back.get_value(), R(2.0 * data[2:].astype(np.float64)).astype(np.float32) * .5)


@pytest.mark.parametrize("case", [(5, 16, 4, 32), (37, 24, 16, 96), (128, 40, 8, 160), (200, 64, 1, 64), (300, 128, 16, 512),
                                  (2000, 128, 16, 1024)])
def test_c8_bf16_fc_ops(case, bf16_mode):
    """Dense products on a bf16 c8 input, as test_c8_fc_ops."""
    Bn, C, HW, N = case
    rng = np.random.RandomState(1)
    assert ctx().lib.tn_c8_fc_supported(Bn, C, HW, N)
    rm = _rowmap(C, HW)
    Kc, n_in, ok = len(rm), C * HW, rm >= 0
    x = np.zeros((Bn, Kc)); x[:, ok] = R(rng.randn(Bn, n_in))[:, rm[ok]]
    W = (rng.randn(n_in, N) / np.sqrt(n_in)).astype(np.float32)
    b = (rng.randn(N) * .1).astype(np.float32)
    mask = (rng.rand(Bn, N) < .5).astype(np.uint8)
    Wp = np.zeros((Kc, N)); Wp[ok] = R(W)[rm[ok]]
    z = x @ Wp + b
    xd, Wd, bd = dev(B.bf16_bits(x)), dev(W), dev(b)
    a = empty((Bn, N))
    call("tn_c8_fc_fwd", xd.ptr, Wd.ptr, bd.ptr, a.ptr, Bn, C, HW, N, LEAKY, SLOPE, dev(mask).ptr)
    assert _rel(a.get_value(), U.leaky(z, SLOPE) * mask) < 2e-5
    want, got_mask, a2 = empty((Bn * N,), np.uint8), empty((Bn * N,), np.uint8), empty((Bn, N))
    for elem0 in (1000, 1003):
        call("tn_dropout_mask", want.ptr, Bn * N, .3, 99, 5, None, elem0)
        call("tn_c8_fc_fwd_dropout", xd.ptr, Wd.ptr, bd.ptr, a2.ptr, Bn, C, HW, N, LEAKY, SLOPE, got_mask.ptr, .3, 99, 5,
             None, elem0)
        assert np.array_equal(got_mask.get_value(), want.get_value())
        call("tn_c8_fc_fwd", xd.ptr, Wd.ptr, bd.ptr, a.ptr, Bn, C, HW, N, LEAKY, SLOPE, want.ptr)
        assert np.array_equal(a2.get_value(), a.get_value())
    dz = (rng.randn(Bn, N) * 1e-3).astype(np.float32)
    dz16 = R(GS * dz.astype(np.float64))
    y = R(rng.randn(Bn, Kc)); y[0, :3] = 0
    dxw = (dz16 @ Wp.T) * U.leaky_grad_from_out(y, SLOPE)
    dzd = dev(dz)
    dxo = empty((Bn, Kc), np.uint16)
    call("tn_c8_fc_dgrad", dzd.ptr, Wd.ptr, dxo.ptr, Bn, C, HW, N, dev(B.bf16_bits(y)).ptr, LEAKY, SLOPE)
    got = B.bf16_value(dxo.get_value()).astype(np.float64)
    assert _rel(got[:, ok], R(dxw)[:, ok]) < TOL16
    dWw = np.zeros((n_in, N)); dWw[rm[ok]] = (x.T @ dz16)[ok] / GS
    gW, gb = empty((n_in, N)), empty((N,))
    call("tn_c8_fc_wgrad", xd.ptr, dzd.ptr, gW.ptr, gb.ptr, Bn, C, HW, N)
    assert _rel(gW.get_value(), dWw) < 2e-5
    assert _rel(gb.get_value(), dz16.sum(0) / GS) < 2e-5
    # the weight gradient leaves its rounded dz for the input gradient that follows: the same bf16 result
    call("tn_c8_fc_dgrad", dzd.ptr, Wd.ptr, dxo.ptr, Bn, C, HW, N, dev(B.bf16_bits(y)).ptr, LEAKY, SLOPE)
    assert _rel(B.bf16_value(dxo.get_value()).astype(np.float64)[:, ok], R(dxw)[:, ok]) < TOL16


@pytest.mark.parametrize("C,hw,nearest,invert,mode", [
    (3, 32, False, 0, "philox"), (3, 32, True, 1, "mask"), (1, 28, False, 1, "none"), (8, 16, False, 0, "philox"),
    (11, 16, True, 0, "mask"), (4, 64, False, 0, "none"),
])
def test_c8_bf16_elastic_apply_equals_apply_then_round(C, hw, nearest, invert, mode, bf16_mode):
    """tn_c8_elastic_apply in bf16 mode stores exactly bf16(tn_elastic_apply's value), zero beyond C."""
    N, rng = 5, np.random.RandomState(3)
    x = rng.rand(N + 2, C, hw, hw).astype(np.float32)
    idx = dev(rng.randint(0, (hw - 1) * hw - 1, hw * hw).astype(np.int32) // hw * hw + rng.randint(0, hw - 1, hw * hw).astype(np.int32))
    fy, fx = dev(rng.rand(hw * hw).astype(np.float32)), dev(rng.rand(hw * hw).astype(np.float32))
    fm = dev((rng.rand(N, C, hw, hw) < .2).astype(np.uint8)) if mode == "mask" else None
    pflip = .15 if mode == "philox" else 0.0
    d_step = dev(np.array([7], np.uint32))
    args = (int(nearest), idx.ptr, fy.ptr, fx.ptr, pflip, fm.ptr if fm is not None else None, 12345, 3, d_step.ptr, 40)
    xd, row0 = dev(x), dev(np.array([1], np.int64))
    out = empty((N, C, hw, hw))
    call("tn_elastic_apply", xd.ptr, 1, row0.ptr, out.ptr, N, C, hw, hw, invert, *args)
    C8 = (C + 7) // 8
    out16 = empty((N, C8, hw * hw, 8), np.uint16)
    call("tn_c8_elastic_apply", xd.ptr, 1, row0.ptr, out16.ptr, N, C, hw, hw, invert, *args)
    want = np.zeros((N, C8 * 8, hw * hw), np.uint16)
    want[:, :C] = B.bf16_bits(R(out.get_value().astype(np.float64))).reshape(N, C, hw * hw)
    want = want.reshape(N, C8, 8, hw * hw).transpose(0, 1, 3, 2)
    np.testing.assert_array_equal(out16.get_value(), want)


def test_c8_bf16_unsupported_shapes_are_errors_not_fallbacks(bf16_mode):
    from theanet_amd import _lib, NeuralNet
    lib = ctx().lib
    assert not lib.tn_c8_conv_supported(4, 16, 16, 16, 20, 3, 1, 1)
    assert not lib.tn_c8_conv_supported(4, 16, 12, 12, 16, 3, 1, 1)
    assert not lib.tn_c8_conv_supported(4, 16, 16, 16, 16, 5, 1, 2)
    assert not lib.tn_c8_fc_supported(4, 10, 1, 32)
    x, W, b = empty((4, 2, 16, 16, 8), np.uint16), dev(np.zeros((20, 16, 3, 3), np.float32)), dev(np.zeros(20, np.float32))
    with pytest.raises(_lib.BackendError, match="multiple of 8"):
        call("tn_c8_conv_fwd", x.ptr, W.ptr, b.ptr, x.ptr, None, 4, 16, 16, 16, 20, LEAKY, SLOPE, 0, None)
    # the fp32-tensor conv entry points refuse to run in the mode
    xf, yf = empty((4, 16, 16, 16)), empty((4, 16, 16, 16))
    Wf, bf = dev(np.zeros((16, 16, 3, 3), np.float32)), dev(np.zeros(16, np.float32))
    with pytest.raises(_lib.BackendError, match="16-bit DTYPE"):
        call("tn_conv2d_fwd", xf.ptr, Wf.ptr, bf.ptr, yf.ptr, 4, 16, 16, 16, 16, 3, 1, 1, 16, 16, LEAKY, SLOPE)
    tp = {"SEED": 1, "BATCH_SZ": 4, "INIT_LEARNING_RATE": .1, "EPOCHS_TO_HALF_RATE": 1, "DTYPE": "bfloat16"}
    with pytest.raises(AssertionError, match="DTYPE bfloat16"):
        NeuralNet([("InputLayer", {"img_sz": 16, "num_maps": 3}),
                   ("ConvLayer", {"num_maps": 20, "filter_sz": 3, "stride": 1, "mode": "same"}),
                   ("SoftmaxLayer", {"n_out": 10})], dict(tp))
    with pytest.raises(AssertionError, match="DTYPE bfloat16"):
        NeuralNet([("InputLayer", {"img_sz": 16, "num_maps": 3}),
                   ("ConvLayer", {"num_maps": 16, "filter_sz": 3, "stride": 1, "mode": "same"}),
                   ("SoftmaxLayer", {"n_out": 10})], dict(tp))
    ctx().set_matmul_dtype("float32")


def c8_launches():
    """Every tn_c8_conv_{fwd, dgrad, wgrad} call the tests above make, as tests/test_gpu_c8.py's c8_launches lists them
    (tests/test_c8_bf16_cpu.py: the same list, so tests/test_c8_dispatch.py's sweep covers the bf16 kernels too)."""
    out = []
    for N, C, H, K in C8_CASES:
        for name in C8_ACT_NAMES:
            act, prm = ACTS[name]
            out += [(op, N, C, H, K, pool, act, prm) for op in (0, 1) for pool in (0, 1)]
        out += [(2, N, C, H, K, pool, 0, 0.) for pool in (0, 1)]
    for N, C, H, K in C8_FWD_CASES:
        for name in C8_ACT_NAMES:
            act, prm = ACTS[name]
            out += [(op, N, C, H, K, pool, act, prm) for op in (0, 1) for pool in (0, 1)]
    for N, C, H, K in WGRAD_RING_CASES:
        out += [(2, N, C, H, K, pool, 0, 0.) for pool in (0, 1)]
    out.append((0, 3, 16, 16, 24, 0) + ACTS["tanh"])          # test_c8_bf16_generic_activation_and_pack_roundtrip
    return out
