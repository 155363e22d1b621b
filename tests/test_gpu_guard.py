"""Negative controls of the guarded test allocator (tests/guard_util.py): the guard must be able to fail.

Every write here is host-driven -- one tn_h2d or tn_memset of a single byte through a ``view()`` into an allocation this
test owns, bands included; no kernel is made to misbehave.  The autouse fixture is active here as in every GPU module, so
a control that damages a band also consumes the violation (``check_all()`` raises once per damaged band).  The same file
runs against the CPU backend (THEANET_BACKEND=cpu, tests/test_guard_cpu.py)."""
import numpy as np
import pytest

from tests import guard_util as G
from tests.gpu_util import call, ctx, empty
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)
from theanet_amd import _lib, device

pytestmark = pytest.mark.gpu

_PLAIN_INIT, _PLAIN_CALL = device.DeviceArray.__init__, device.Context.call       # (modules are imported unguarded)


def _byte(arr, offset):
    """A one-byte view at ``offset`` bytes from the start of ``arr``'s interior (negative: into the pre band)."""
    return arr.view(0, (1,), np.uint8).view(offset, (1,), np.uint8)


def test_one_byte_past_the_interior_is_a_post_band_violation():
    a = empty((5, 7))                                   # 140 bytes: the post band starts at an address that is 12 mod 128
    _byte(a, a.nbytes).set_value(np.zeros(1, np.uint8))                 # tn_h2d
    with pytest.raises(G.GuardViolation) as e:
        G.check_all()
    msg = str(e.value)
    assert "1 guard violation(s)" in msg and "post band" in msg and "shape (5, 7) dtype float32" in msg, msg
    assert "1 damaged byte(s), bytes +0..+0 past the end" in msg and "first bytes: 00" in msg, msg
    G.check_all()                                       # a damaged band is listed once


def test_one_byte_before_the_interior_is_a_pre_band_violation():
    a = empty((3,), np.int32)
    _byte(a, -1).fill_bytes(0x5a)                       # tn_memset
    ctx().sync()
    with pytest.raises(G.GuardViolation) as e:
        G.check_all()
    msg = str(e.value)
    assert "pre band" in msg and "post band" not in msg and "shape (3,) dtype int32" in msg, msg
    assert "bytes -1..-1 before the start" in msg and "first bytes: 5a" in msg, msg


def test_first_and_last_damaged_offsets_are_reported():
    a = empty((10,), np.float16)
    for off in (a.nbytes + 3, a.nbytes + 4, a.nbytes + G.BAND - 1):
        _byte(a, off).set_value(np.zeros(1, np.uint8))
    with pytest.raises(G.GuardViolation, match=r"3 damaged byte\(s\), bytes \+3\.\.\+%d past the end" % (G.BAND - 1)):
        G.check_all()


def test_damage_is_found_when_the_array_is_freed_and_listed_with_the_rest():
    a, b = empty((4,)), empty((2, 2), np.uint8)
    _byte(a, a.nbytes).set_value(np.zeros(1, np.uint8))
    _byte(b, -G.BAND).set_value(np.zeros(1, np.uint8))                  # the very first byte of the allocation
    del a                                               # recorded inside __del__, not raised
    with pytest.raises(G.GuardViolation) as e:
        G.check_all()
    msg = str(e.value)
    assert "2 guard violation(s)" in msg, msg
    assert "shape (4,) dtype float32" in msg and "found when the array was freed" in msg, msg
    assert "shape (2, 2) dtype uint8" in msg and "bytes -%d..-%d before" % (G.BAND, G.BAND) in msg, msg


def test_writes_inside_the_interior_pass():
    a = empty((3, 5))
    a.set_value(np.arange(15, dtype=np.float32))
    _byte(a, 0).set_value(np.ones(1, np.uint8))
    _byte(a, a.nbytes - 1).set_value(np.ones(1, np.uint8))
    z = ctx().zeros((0,))                               # an empty array has bands and nothing between them
    G.check_all()
    rec = G.record_of(a)
    assert rec.poisoned and a.ptr - rec.raw == G.BAND and a.ptr % 256 == 0 and z.nbytes == 0
    del a, z
    G.check_all()                                       # ... and nothing was found at the frees


def test_fresh_memory_is_poison_and_a_padded_c8_tensor_is_zero():
    assert np.isnan(empty((7, 9)).get_value()).all()
    assert np.isnan(empty((33,), np.float16).get_value()).all()
    assert (empty((6,), np.int32).get_value() == -1).all()
    assert (empty((5,), np.uint8).get_value() == 255).all()
    for elem in device.C8_DTYPES:
        padded = device.C8Array(ctx(), 2, 3, 6, 6, elem, pitch=8)      # allocated zeroed: rows and columns 6, 7 stay zero
        assert (device.DeviceArray.get_value(padded) == 0).all() and (padded.get_value() == 0).all()
        dense = device.C8Array(ctx(), 2, 3, 6, 6, elem)                # no pad cells: nothing promises zeros
        assert (device.DeviceArray.get_value(dense) == 0xFFFF).all() and np.isnan(dense.get_value()).all()
        assert G.record_of(padded).c8 == (3, 6, 6) and G.record_of(padded).nbytes == 2 * 1 * 8 * 8 * 8 * 2
    keep = ctx().zeros((4, 4))                          # zeros / array overwrite the interior as before
    assert (keep.get_value() == 0).all()
    assert (ctx().array(np.arange(6.0), dtype=np.float32).get_value() == np.arange(6)).all()


def test_views_and_reshapes_are_checked_through_their_base():
    a = empty((4, 6))
    live = G.stats()["live"]
    v, r = a.view(6, (2, 6)), a.reshape(6, 4)
    vv = v.reshape(12).view(3, (4,))
    assert G.stats()["live"] == live                    # no allocation, no record of their own
    for t in (v, r, vv):
        assert "_guard" not in vars(t) and G.record_of(t) is G.record_of(a) and t._owns is False
    assert v.ptr == a.ptr + 24 and r.ptr == a.ptr
    _byte(v, v.nbytes).set_value(np.zeros(1, np.uint8))                # past the view, inside the allocation's interior
    G.check_all()
    _byte(v, v.nbytes + 6 * 4).set_value(np.zeros(1, np.uint8))        # past the view AND past its base
    with pytest.raises(G.GuardViolation, match=r"post band of the allocation of shape \(4, 6\) dtype float32.*\+0\.\.\+0"):
        G.check_all()
    live = G.stats()["live"]
    del a, r
    assert G.stats()["live"] == live and G.record_of(vv).raw != 0       # a view keeps its base, bands and all, alive
    assert v.get_value().shape == (2, 6)


def test_a_refused_call_is_no_device_error_and_a_device_error_stops_the_readbacks():
    with pytest.raises(_lib.BackendError, match=r"rc=-2"):
        call("tn_stream_select", 7)                     # TN_E_ARG: an argument refusal
    assert G._S.device_error is None
    a = empty((8,))
    _byte(a, a.nbytes).set_value(np.zeros(1, np.uint8))
    checked = G.stats()["checked"]
    G._S.device_error = "tn_fc_fwd failed (rc=-1): ..."                # what _guarded_call leaves behind on TN_E_HIP
    try:
        G.check_all()                                   # nothing is read back, so nothing is found
        assert G.stats()["checked"] == checked
    finally:
        G._S.device_error = None
    with pytest.raises(G.GuardViolation):
        G.check_all()


def test_an_allocation_inside_a_stream_capture_is_banded_but_not_filled():
    G._S.capturing = True                               # what _guarded_call sets between tn_graph_begin and tn_graph_end
    try:
        a = empty((8,))
        checked = G.stats()["checked"]
        G.check_all()
        assert G.stats()["checked"] == checked
    finally:
        G._S.capturing = False
    rec = G.record_of(a)
    assert not rec.poisoned and a.ptr - rec.raw == G.BAND
    G.check_all()                                       # never filled: never compared


def test_after_uninstall_device_arrays_allocate_as_before():
    assert device.DeviceArray.__init__ is not _PLAIN_INIT and device.Context.call is not _PLAIN_CALL
    guarded = G.stats()["guarded"]
    G.uninstall()
    try:
        assert device.DeviceArray.__init__ is _PLAIN_INIT and device.Context.call is _PLAIN_CALL
        a = empty((5, 7))
        assert a._owns is True and G.record_of(a) is None and "_guard" not in vars(a)
        assert G.stats()["guarded"] == guarded
        a.set_value(np.ones((5, 7), np.float32))
        assert (a.get_value() == 1).all()
    finally:
        G.install()
    G.install()                                         # idempotent: still one layer to take off
    b = empty((2,))
    assert G.record_of(b) is not None and G.stats()["guarded"] == guarded + 1
    G.uninstall()
    assert device.DeviceArray.__init__ is _PLAIN_INIT
    assert np.isnan(b.get_value()).all()                # an array guarded earlier stays guarded (and is freed through its record)
    G.install()
