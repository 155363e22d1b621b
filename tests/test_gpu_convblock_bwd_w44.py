"""The addressing of the masked matrix-core conv-block backward (convblock_bwd_mask_mfma, through tn_convblock_bwd_mask).

Its weight-gradient loop on the 16-block MFMA takes two steps per trip on two operand sets, with every address a lane base
fixed before the image loop plus an immediate, a running offset or a table entry read a step ahead; the dgrad loop takes
two dz rows per trip from one address per trip; the copy-out reads the whole dx tile before the first store.  Each case
below is a geometry at which one of these can go wrong (see the table).  Oracle and tolerances are those of
test_gpu_convblock_bwd_loops.test_mask_dx_conv2_geometry: tn_convpool_fwd_mask, then tn_convblock_bwd_mask against the
float64 oracle, dx at 2e-5, dW / db at 2e-4, both with dx and with dx = None; windows whose two largest elements are within
1e-4 of each other carry no gradient (the oracle helper zeroes it), and at most 1 % of a case's windows may be such."""
import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests.gpu_util import act_code, assert_close, call, ctx, dev, empty
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)
from tests.test_gpu_convblock_bwd_loops import _oracle, _own_the_context  # noqa: F401  (autouse: take the context over)

pytestmark = pytest.mark.gpu

CASES = [
    # N     C  H   K   mode     act
    (1,     4, 13, 20, "valid", "relu05"),      # mnist conv2: waves without an image; remainder product (37 columns)
    (5,     4, 13, 20, "valid", "relu05"),
    (None,  4, 13, 20, "valid", "relu05"),      # N = 8 CUs + 5: a wave's second and third image (operand sets and
                                                # running offsets carried across images)
    (3,     4, 12, 5,  "valid", "relu10"),      # Hp = Wp = 5: window pairs straddle rows, 25 windows (odd), 3 padding
                                                # windows in the last steps; K % 4 != 0
    (3,     3, 4,  8,  "valid", "relu05"),      # PT = 1: two steps, 7 of 8 windows padding; 28 columns, no remainder product
    (2,     1, 7,  7,  "valid", "relu10"),      # C = 1 (10 columns); odd Ho = 5: partial last windows, a last dz row alone
    (3,     2, 10, 30, "same",  "relu05"),      # padded tile (pad_lo = 1), 8 filter quads, 19 columns
    (3,     4, 10, 32, "valid", "relu05"),      # most filters, remainder product with all its registers
    (3,     4, 11, 20, "valid", "tanh"),        # not the 16-block instantiation: the shared staging, dgrad and copy-out
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%s-C%d-H%d-K%d-%s-%s" % c)
def test_mask_backward_addressing(case):
    N, C, H, K, mode, act = case
    if N is None:
        N = 8 * ctx().info()[1] + 5             # 2053 on MI355X: 2 CUs' worth of waves past two images each
    pad_lo, _, Ho = O.conv_geometry(H, 3, 1, mode)
    Hp = O.pool_out_sz(Ho, 2, False)
    assert ctx().lib.tn_convblock_mask_supported(C, K, 3, 1, 2, H, H, pad_lo, Ho, Ho, Hp, Hp)
    rng = np.random.RandomState(N * 13 + K + C)
    x = rng.randn(N, C, H, H).astype(np.float32)
    W = (rng.randn(K, C, 3, 3) / np.sqrt(C * 9)).astype(np.float32)
    b = rng.randn(K).astype(np.float32)
    g0 = rng.randn(N, K, Hp, Hp).astype(np.float32)
    g, y_w, _, dx_w, dW_w, db_w = _oracle(x, W, b, g0, mode, act, False, need_dx=True, keep_dz=False)
    zeroed = np.count_nonzero((g == 0) & (g0 != 0)) / g.size
    print("near-tie windows zeroed: %.2e" % zeroed)
    assert zeroed <= 0.01, zeroed
    kind, prm = act_code(act)
    xd, Wd, bd, gd = dev(x), dev(W), dev(b), dev(g)
    y, mask = empty((N, K, Hp, Hp)), empty((N, K, Hp, Hp), np.uint8)
    geom = (N, C, H, H, K, 3, pad_lo, Ho, Ho, 2, Hp, Hp, kind, prm)
    call("tn_convpool_fwd_mask", xd.ptr, Wd.ptr, bd.ptr, y.ptr, mask.ptr, *geom)
    assert_close(y.get_value(), y_w, what="block fwd")
    dx, dW, db = empty(x.shape), empty(W.shape), empty((K,))
    call("tn_convblock_bwd_mask", xd.ptr, Wd.ptr, gd.ptr, y.ptr, mask.ptr, dx.ptr, dW.ptr, db.ptr, *geom)
    dx_g, dW_g, db_g = dx.get_value(), dW.get_value(), db.get_value()
    print("max |err|: dx %.2e  dW %.2e  db %.2e" % (np.abs(dx_g - dx_w).max(), np.abs(dW_g - dW_w).max(),
                                                    np.abs(db_g - db_w).max()))
    assert_close(dx_g, dx_w, atol=2e-5, what="block dx")
    assert_close(dW_g, dW_w, atol=2e-4, what="block dW")
    assert_close(db_g, db_w, atol=2e-4, what="block db")
    for buf in (dx, dW, db):
        buf.fill_bytes(0xff)
    call("tn_convblock_bwd_mask", xd.ptr, Wd.ptr, gd.ptr, y.ptr, mask.ptr, None, dW.ptr, db.ptr, *geom)
    assert_close(dW.get_value(), dW_w, atol=2e-4, what="block dW (no dx)")
    assert_close(db.get_value(), db_w, atol=2e-4, what="block db (no dx)")
