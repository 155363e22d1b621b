"""The per-geometry lane table of the masked matrix-core conv-block backward (tn_convblock_table, read by
convblock_bwd_mask_mfma through tn_convblock_bwd_mask).

The kernel's set-up -- tile offsets of the staging, the window table, the sources and validity of the dgrad filter
operand -- is loaded from a device table the context builds once per geometry (C, H, Wd, K, pad, Ho, Wo, Hp, Wp) and keeps.
What can go wrong is the cache (a geometry answered with another one's table, filter VALUES kept with it), the table's
contents at the edges of the supported shapes, and waves without an image, which now prefetch one all the same.  Oracle and
tolerances are those of test_gpu_convblock_bwd_w44: tn_convpool_fwd_mask, then tn_convblock_bwd_mask against the float64
oracle, dx at 2e-5, dW / db at 2e-4; near-tie windows carry no gradient and are at most 1 % of a case's windows.  At most
16 images per case."""
import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests.gpu_util import act_code, assert_close, call, ctx, dev, empty
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)
from tests.test_gpu_convblock_bwd_loops import _oracle, _own_the_context  # noqa: F401  (autouse: take the context over)

pytestmark = pytest.mark.gpu

MNIST = (4, 13, 20, "valid")        # mnist.prms conv2: C 4, 13x13 -> 11x11 -> 6x6, K 20


def _geometry(C, H, K, mode):
    pad_lo, _, Ho = O.conv_geometry(H, 3, 1, mode)
    Hp = O.pool_out_sz(Ho, 2, False)
    assert ctx().lib.tn_convblock_mask_supported(C, K, 3, 1, 2, H, H, pad_lo, Ho, Ho, Hp, Hp), (C, H, K, mode)
    return pad_lo, Ho, Hp


class _Case:
    """One problem: host data, the oracle's answer (computed once), and the block's forward on the device."""

    def __init__(self, N, C, H, K, mode, act="relu05", seed=0, W=None):
        self.shape = (N, C, H, K, mode)
        pad_lo, Ho, Hp = _geometry(C, H, K, mode)
        rng = np.random.RandomState(1000 * seed + N * 13 + K + C)
        self.x = rng.randn(N, C, H, H).astype(np.float32)
        self.W = (rng.randn(K, C, 3, 3) / np.sqrt(C * 9)).astype(np.float32) if W is None else W
        b = rng.randn(K).astype(np.float32)
        g0 = rng.randn(N, K, Hp, Hp).astype(np.float32)
        g, y_w, _, self.dx_w, self.dW_w, self.db_w = _oracle(self.x, self.W, b, g0, mode, act, False, need_dx=True,
                                                             keep_dz=False)
        zeroed = np.count_nonzero((g == 0) & (g0 != 0)) / g.size
        assert zeroed <= 0.01, zeroed
        kind, prm = act_code(act)
        self.geom = (N, C, H, H, K, 3, pad_lo, Ho, Ho, 2, Hp, Hp, kind, prm)
        self.table_args = (C, H, H, K, 3, pad_lo, Ho, Ho, 2, Hp, Hp)
        self.xd, self.Wd, self.gd = dev(self.x), dev(self.W), dev(g)
        self.y, self.mask = empty((N, K, Hp, Hp)), empty((N, K, Hp, Hp), np.uint8)
        call("tn_convpool_fwd_mask", self.xd.ptr, self.Wd.ptr, dev(b).ptr, self.y.ptr, self.mask.ptr, *self.geom)
        assert_close(self.y.get_value(), y_w, what="block fwd %s" % (self.shape,))

    def backward(self, with_dx=True, check=True):
        """(dx or None, dW, db) of one tn_convblock_bwd_mask call into poisoned buffers."""
        dx, dW, db = empty(self.x.shape), empty(self.W.shape), empty((self.W.shape[0],))
        for buf in (dx, dW, db):
            buf.fill_bytes(0xff)
        call("tn_convblock_bwd_mask", self.xd.ptr, self.Wd.ptr, self.gd.ptr, self.y.ptr, self.mask.ptr,
             dx.ptr if with_dx else None, dW.ptr, db.ptr, *self.geom)
        out = (dx.get_value() if with_dx else None, dW.get_value(), db.get_value())
        if check:
            self.check(*out)
        return out

    def check(self, dx, dW, db):
        what = " %s" % (self.shape,)
        if dx is not None:
            print("max |err|%s: dx %.2e  dW %.2e  db %.2e" % (what, np.abs(dx - self.dx_w).max(),
                                                               np.abs(dW - self.dW_w).max(), np.abs(db - self.db_w).max()))
            assert_close(dx, self.dx_w, atol=2e-5, what="block dx" + what)
        assert_close(dW, self.dW_w, atol=2e-4, what="block dW" + what)
        assert_close(db, self.db_w, atol=2e-4, what="block db" + what)


def _same_bits(a, b):
    return all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


def test_geometries_alternate_through_one_context():
    """A, B, A: B is right, and the second A is the first A bit for bit (a table is found again by its whole key)."""
    A = _Case(5, *MNIST)
    B = _Case(5, 4, 12, 18, "valid")            # 12x12 -> 10x10 -> 5x5, K 18
    call("tn_convblock_table", *A.table_args)   # the entry point itself; a second build of a known geometry is a lookup
    call("tn_convblock_table", *A.table_args)
    a1 = A.backward()
    B.backward()
    a2 = A.backward()
    assert _same_bits(a1, a2)


def test_same_maps_other_k_c_pad():
    """Neighbours in the key: K 20 / K 18 (one KS2 instantiation, other validity bits and dz rows), C 4 / C 3, pad_lo 0 / 1
    on one image size -- each visited twice, with the others in between."""
    cases = [_Case(4, 4, 13, 20, "valid"), _Case(4, 4, 13, 18, "valid"), _Case(4, 3, 13, 20, "valid"),
             _Case(4, 2, 10, 30, "valid"), _Case(4, 2, 10, 30, "same")]
    assert cases[3].geom[6] == 0 and cases[4].geom[6] == 1
    first = [c.backward() for c in cases]
    for c, f in reversed(list(zip(cases, first))):
        assert _same_bits(f, c.backward())


def test_filter_values_are_not_cached():
    """One geometry, two W in consecutive calls: the second call's dx follows the second W."""
    one = _Case(5, *MNIST, seed=1)
    W2 = (np.random.RandomState(77).randn(*one.W.shape) / 6.).astype(np.float32)
    two = _Case(5, *MNIST, seed=1, W=W2)        # same x, g draw and geometry
    dx1, _, _ = one.backward()
    dx2, _, _ = two.backward()
    assert np.abs(dx2 - dx1).max() > 1e-2       # (the two answers are far apart: the check above told them apart)
    # ... and with the new values in the SAME device buffer the first call read
    one.Wd.set_value(W2)
    dx, dW, db = empty(one.x.shape), empty(one.W.shape), empty((20,))
    call("tn_convblock_bwd_mask", one.xd.ptr, one.Wd.ptr, two.gd.ptr, two.y.ptr, two.mask.ptr, dx.ptr, dW.ptr, db.ptr,
         *one.geom)
    two.check(dx.get_value(), dW.get_value(), db.get_value())


@pytest.mark.parametrize("N", [3, 5, 9])
def test_small_and_uneven_batches(N):
    """N = 3: fewer images than a block's waves; 5 and 9: waves with 0, 1 and 2 images (a wave without an image still
    prefetches one and must write nothing)."""
    c = _Case(N, *MNIST, seed=2)
    c.backward()
    c.backward(with_dx=False)                   # the dW / db only form


CORNERS = [
    (3, 1, 4, 1, "valid"),          # C 1, K 1 on a 4x4 image: one window, one validity bit, 2x2 map (even Ho)
    (3, 2, 16, 15, "valid"),        # Wo = 14, the DPP-row limit; 49 windows (13 tiles, 3 padding windows)
    (3, 4, 13, 20, "valid"),        # odd Ho = 11
    (3, 4, 12, 20, "valid"),        # even Ho = 10
]


@pytest.mark.parametrize("case", CORNERS, ids=lambda c: "N%d-C%d-H%d-K%d-%s" % c)
def test_corners_of_the_supported_shapes(case):
    _Case(*case, seed=3).backward()
