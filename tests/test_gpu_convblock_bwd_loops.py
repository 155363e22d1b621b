"""The loops of the two conv-block backward kernels, at the smallest shapes where they can go wrong.

tn_convpool_bwd_mask walks a thread's pooling windows in groups of MW = 4 / 2 / 1 rounds (every load of a group
first, then the FMAs round by round), with the patch rows as 8-byte loads where the geometry allows; which group
size and which loader a call takes depends on the window count against 2 * num_cus, on the padding, the width and
the alignment of x.  The masked matrix-core backward (tn_convblock_bwd_mask) is run at the mnist.prms conv2 geometry
with and without the remainder product (C = 4 / C = 3), with waves that have no image and odd image counts.

Reference and tolerances are those of tests/test_gpu_kernels.py for the same entry points (the float64 oracle;
tn_convpool_bwd_mask: dz 1e-5, dW / db max(2e-4, 2e-6 max|want|); tn_convblock_bwd_mask: dx 2e-5, dW / db 2e-4).
The oracle runs over slices of the batch (its im2col view of a large batch does not fit), dW / db summed over the
slices in float64."""
import functools

import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests.gpu_util import act_code, assert_close, call, ctx, dev, empty
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _own_the_context():
    """These tests call the C-ABI directly and read dW / db right after the call.  A pipelined training function of an
    earlier test module may have left a step's slab sums parked with its stream (an open tn_defer_reductions window):
    inside it a weight-gradient op only RECORDS its sum, and the records of a collected net point at freed buffers.
    Take the context over as a net does (NeuralNet._apply_dtype): finish what a living net parked, forget what a dead
    one did; and put the dense / conv products back to fp32, which conftest's fixture does for the conv dtype only."""
    from theanet_amd.neuralnet import NeuralNet
    ref = NeuralNet._ctx_owner
    prev = ref() if ref is not None else None
    if prev is not None and prev._pipe_fn is not None:
        prev._pipe_fn._flush_parked()
    elif ref is not None:
        call("tn_defer_discard")
    NeuralNet._ctx_owner = None
    ctx().set_fc_matmul("float32")
    ctx().set_conv_matmul("float32")
    yield


def _cdiv(a, b):
    return -(-a // b)


NEAR_TIE = 1e-4     # two window elements closer than this: which of them is the fp32 forward's maximum is not determined


def _oracle(x, W, b, g, mode, act, ib, need_dx=False, keep_dz=True, chunk=512):
    """(g, y, dz or None, dx or None, dW, db) of the conv + act + 2x2 max-pool block, float64, by the oracle statements of
    tests/test_gpu_kernels.py.  The returned g is the test's pooled gradient: the given one, set to zero in the windows
    whose two largest elements are within NEAR_TIE of each other.  There the float64 oracle and the fp32 forward may
    pick different elements, and the gradient would move from one input patch to another; among a few million windows
    (more so under a saturating activation) some always do.  With g = 0 in them both answers are the same."""
    fa, dfa = O.activation(act)
    W64, b64 = W.astype(np.float64), b.astype(np.float64)
    g = g.copy()
    ys, dzs, dxs = [], [], []
    dW, db = np.zeros(W.shape), np.zeros(b.shape)
    for s in range(0, x.shape[0], chunk):
        x64 = x[s:s + chunk].astype(np.float64)
        z = O.conv2d_fwd(x64, W64, b64, 1, mode)
        a = fa(z)
        win, _ = O._pool_windows(a, 2, ib, -np.inf)                      # N, K, Hp, 2, Wp, 2
        top = np.sort(win.transpose(0, 1, 2, 4, 3, 5).reshape(win.shape[:3] + (win.shape[4], 4)), axis=-1)
        g[s:s + chunk][top[..., 3] - top[..., 2] < NEAR_TIE] = 0.
        ys.append(O.pool_fwd(a, 2, ib))
        dz = O.pool_bwd(a, g[s:s + chunk].astype(np.float64), 2, ib) * dfa(z)
        dx_, dW_, db_ = O.conv2d_bwd(x64, W64, dz, 1, mode, need_dx=need_dx)
        dW += dW_
        db += db_
        if keep_dz:
            dzs.append(dz)
        if need_dx:
            dxs.append(dx_)
    return (g, np.concatenate(ys), np.concatenate(dzs) if keep_dz else None,
            np.concatenate(dxs) if need_dx else None, dW, db)


def _mwin(total):
    """launch_bwd_mask's windows per thread for ``total`` pooling windows on this device."""
    cus = ctx().info()[1]
    mwin = 4
    while mwin > 1 and _cdiv(total, 256 * mwin) < 2 * cus:
        mwin >>= 1
    return mwin


def _batch_for(mwin_want, windows_per_image):
    """The smallest odd N whose window count takes ``mwin_want`` windows per thread (so the last block is partial)."""
    cus = ctx().info()[1]
    n = _cdiv(2 * cus * 256 * mwin_want, windows_per_image)
    while _cdiv(n * windows_per_image, 256 * mwin_want) < 2 * cus or n % 2 == 0:
        n += 1
    assert _mwin(n * windows_per_image) == mwin_want, (n, mwin_want)
    return n


@functools.lru_cache(maxsize=2)
def _mask_case(N, C, H, K, mode, act, ib):
    """Inputs and reference of one block, shared by the cases that differ only in what they ask of the kernel (read only).
    dz is kept for all but the largest batch."""
    _, _, Ho = O.conv_geometry(H, 3, 1, mode)
    Hp = O.pool_out_sz(Ho, 2, ib)
    rng = np.random.RandomState(N * 13 + K)
    x = rng.randn(N, C, H, H).astype(np.float32)
    W = (rng.randn(K, C, 3, 3) / np.sqrt(C * 9)).astype(np.float32)
    b = rng.randn(K).astype(np.float32)
    g = rng.randn(N, K, Hp, Hp).astype(np.float32)
    return (x, W, b) + _oracle(x, W, b, g, mode, act, ib, keep_dz=N < 5000)


def _run_mask_backward(N, C, H, K, mode, act, ib, with_dz, scalar_twin=False):
    f = 3
    pad_lo, _, Ho = O.conv_geometry(H, f, 1, mode)
    Hp = O.pool_out_sz(Ho, 2, ib)
    x, W, b, g, y_w, dz_w, _, dW_w, db_w = _mask_case(N, C, H, K, mode, act, ib)
    assert dz_w is not None or not with_dz
    kind, prm = act_code(act)
    xd, Wd, bd, gd = dev(x), dev(W), dev(b), dev(g)
    y, mask = empty((N, K, Hp, Hp)), empty((N, K, Hp, Hp), np.uint8)
    geom = (N, C, H, H, K, f, pad_lo, Ho, Ho, 2, Hp, Hp, kind, prm)
    call("tn_convpool_fwd_mask", xd.ptr, Wd.ptr, bd.ptr, y.ptr, mask.ptr, *geom)
    assert_close(y.get_value(), y_w, what="convpool fwd (mask)")
    tolW, tolb = max(2e-4, 2e-6 * np.abs(dW_w).max()), max(2e-4, 2e-6 * np.abs(db_w).max())
    dW, db = empty(W.shape), empty((K,))
    if with_dz:
        dz = empty((N, K, Ho, Ho))
        call("tn_convpool_bwd_mask", xd.ptr, gd.ptr, y.ptr, mask.ptr, dz.ptr, dW.ptr, db.ptr, *geom)
        assert_close(dz.get_value(), dz_w, atol=1e-5, what="convpool(mask) dz")
        assert_close(dW.get_value(), dW_w, atol=tolW, what="convpool(mask) dW")
        assert_close(db.get_value(), db_w, atol=tolb, what="convpool(mask) db")
        dW.fill_bytes(0xff)
        db.fill_bytes(0xff)
    call("tn_convpool_bwd_mask", xd.ptr, gd.ptr, y.ptr, mask.ptr, None, dW.ptr, db.ptr, *geom)
    dW_g, db_g = dW.get_value(), db.get_value()
    assert_close(dW_g, dW_w, atol=tolW, what="convpool(mask) dW (no dz)")
    assert_close(db_g, db_w, atol=tolb, what="convpool(mask) db (no dz)")
    if scalar_twin:
        # the same tensor 4 bytes further on: no longer 8-byte aligned, so the 4-byte loader runs -- same values, same
        # order of every sum, hence the same bits
        assert pad_lo == 0 and H % 2 == 0 and 2 * Hp + 2 <= H and xd.ptr % 8 == 0, "not a case of the 8-byte loader"
        buf = empty((x.size + 1,))
        xo = buf.view(1, x.shape)
        xo.set_value(x)
        dW2, db2 = empty(W.shape), empty((K,))
        call("tn_convpool_bwd_mask", xo.ptr, gd.ptr, y.ptr, mask.ptr, None, dW2.ptr, db2.ptr, *geom)
        np.testing.assert_array_equal(dW2.get_value(), dW_g)
        np.testing.assert_array_equal(db2.get_value(), db_g)
        if with_dz:
            dz2 = empty((N, K, Ho, Ho))
            call("tn_convpool_bwd_mask", xo.ptr, gd.ptr, y.ptr, mask.ptr, dz2.ptr, dW2.ptr, db2.ptr, *geom)
            np.testing.assert_array_equal(dz2.get_value(), dz.get_value())


@pytest.mark.parametrize("case", [
    (5, 1, 28, 4, "valid", "relu10", False),        # one round per thread, less than one block, dead lanes
    (3, 1, 15, 5, "valid", "relu05", True),         # odd width: 4-byte loader; ignore_border; K = 5: a ragged filter slice
    (3, 2, 13, 6, "valid", "relu10", False),        # 13 x 13, Hp = 6: the last windows' rows and columns are clamped
    (4, 3, 16, 6, "same", "tanh", False),           # 'same' (pad = 1), C = 3, not leaky
    (3, 3, 14, 5, "valid", "relu10", False),        # C = 3 with dz, 8-byte loader
    (2, 4, 11, 9, "same", "relu", False),           # C = 4 (two filters per thread) with dz
    (3, 4, 12, 3, "valid", "sigmoid", False),       # C = 4, 8-byte loader, not leaky
    (7, 1, 28, 1, "valid", "relu10", False),        # K = 1 < KT: the filters past K repeat filter 0 and are dropped
])
def test_mask_backward_loaders(case):
    N, C, H, K, mode, act, ib = case
    _run_mask_backward(N, C, H, K, mode, act, ib, with_dz=True)


@pytest.mark.parametrize("mwin,act,with_dz", [
    (2, "relu10", True),            # groups of two rounds, with and without dz
    (2, "tanh", False),
    (4, "relu10", False),           # mnist.prms conv1 at full batch: groups of four, 8-byte loader
    (4, "relu10", True),            # with dz the group is capped at two rounds; four windows per thread
    (4, "tanh", False),             # ... not leaky: y is loaded too
])
def test_mask_backward_groups(mwin, act, with_dz):
    """28 x 28, C = 1, K = 4 at the smallest odd batches that take 2 and 4 windows per thread on this device."""
    N = _batch_for(mwin, 13 * 13)
    _run_mask_backward(N, 1, 28, 4, "valid", act, False, with_dz=with_dz, scalar_twin=(act == "relu10"))


def test_mask_backward_over_block_cap():
    """More than 2048 * 1024 windows: the grid stops at 2048 blocks and a thread owns 5 windows -- one group of four
    and one round left over."""
    N = _cdiv(2048 * 1024, 169) + 1
    assert _cdiv(N * 169, 1024) > 2048 and _cdiv(N * 169, 2048 * 256) == 5
    _run_mask_backward(N, 1, 28, 2, "valid", "relu10", False, with_dz=False)     # (K = 2: half the oracle's work)


@pytest.mark.parametrize("C", [3, 4])               # C * 9 + 1 = 28: no remainder product; 37: with it
@pytest.mark.parametrize("K", [8, 20, 32])
@pytest.mark.parametrize("N", [1, 5, 9])            # waves without an image, odd counts
def test_mask_dx_conv2_geometry(N, K, C):
    """The masked matrix-core backward at the mnist.prms conv2 geometry (13 x 13 -> 11 x 11 -> 6 x 6): both gradients and
    dW / db only (the entry point has no dx-only form).  This geometry reaches the kernel through tn_convblock_bwd_mask (tn_convpool_bwd_mask_dx
    takes 'same' blocks of wide layers only); tolerances as in test_gpu_kernels.test_convblock_mask_backward."""
    H, act = 13, "relu05"
    if K == 32:
        # 32 filters (eight filter quads) at 13 x 13 exceed the kernel's LDS bound for two blocks per CU, before and
        # after this change (tn_convblock_mask_supported says no); they run at the 10 x 10 maps that
        # test_gpu_kernels.test_convblock_mask_backward uses for them
        H = 10
    Ho = H - 2
    Hp = (Ho + 1) // 2
    assert ctx().lib.tn_convblock_mask_supported(C, K, 3, 1, 2, H, H, 0, Ho, Ho, Hp, Hp)
    rng = np.random.RandomState(N * 13 + K + C)
    x = rng.randn(N, C, H, H).astype(np.float32)
    W = (rng.randn(K, C, 3, 3) / np.sqrt(C * 9)).astype(np.float32)
    b = rng.randn(K).astype(np.float32)
    g = rng.randn(N, K, Hp, Hp).astype(np.float32)
    g, y_w, _, dx_w, dW_w, db_w = _oracle(x, W, b, g, "valid", act, False, need_dx=True, keep_dz=False)
    kind, prm = act_code(act)
    xd, Wd, bd, gd = dev(x), dev(W), dev(b), dev(g)
    y, mask = empty((N, K, Hp, Hp)), empty((N, K, Hp, Hp), np.uint8)
    geom = (N, C, H, H, K, 3, 0, Ho, Ho, 2, Hp, Hp, kind, prm)
    call("tn_convpool_fwd_mask", xd.ptr, Wd.ptr, bd.ptr, y.ptr, mask.ptr, *geom)
    assert_close(y.get_value(), y_w, what="conv2 block fwd")
    dx, dW, db = empty(x.shape), empty(W.shape), empty((K,))
    call("tn_convblock_bwd_mask", xd.ptr, Wd.ptr, gd.ptr, y.ptr, mask.ptr, dx.ptr, dW.ptr, db.ptr, *geom)
    assert_close(dx.get_value(), dx_w, atol=2e-5, what="conv2 block dx")
    assert_close(dW.get_value(), dW_w, atol=2e-4, what="conv2 block dW")
    assert_close(db.get_value(), db_w, atol=2e-4, what="conv2 block db")
    for buf in (dx, dW, db):
        buf.fill_bytes(0xff)
    call("tn_convblock_bwd_mask", xd.ptr, Wd.ptr, gd.ptr, y.ptr, mask.ptr, None, dW.ptr, db.ptr, *geom)
    assert_close(dW.get_value(), dW_w, atol=2e-4, what="conv2 block dW (no dx)")
    assert_close(db.get_value(), db_w, atol=2e-4, what="conv2 block db (no dx)")
