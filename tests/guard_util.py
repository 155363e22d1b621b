"""A guarded, poisoned device allocator for the tests: every ``DeviceArray`` that allocates while the guard is
installed gets

    [ pre band | interior (nbytes) | post band ]            all of it filled with byte 0xFF

and hands its user the interior.  BAND is a multiple of 256 bytes, so the interior is aligned as tn_alloc's pointers
are; the post band starts at the first byte after ``nbytes``, with no rounding.  0xFF is NaN as fp32 / fp16 / bf16,
255 as a mask byte and -1 as a label -- the poison the suite already used by hand.  When the allocation is freed, and
in ``check_all()``, both bands are copied back (tn_d2h) and compared with 0xFF:

  * a kernel that stores past a ragged tail damages a band                            -> a violation, by name;
  * a kernel that loads past its operand and lets the value matter computes with NaN  -> the test's comparison fails
    (tests/gpu_util.assert_close rejects NaN);
  * an output element that nobody writes, or an output that needed zeroing, reads back NaN -> likewise.

What it cannot see: the C library's own hipMallocs (scratch, tmp), a load further out than BAND bytes, and a load whose
value is discarded (multiplied by nothing, masked off).

The shim sits on the single allocation point, ``DeviceArray.__init__`` (views, reshapes and C8Arrays go through it and
are tracked through the array that owns their memory).  The owning array keeps an ``_Allocation`` that releases the
memory when the array dies -- also after ``uninstall()``, so arrays that outlive a test are freed and checked all the
same.  The guard launches no kernel: it issues tn_memset + one synchronous tn_h2d per allocation and two tn_d2h per
check, and nothing at all while a stream capture (tn_graph_begin .. tn_graph_end) is open or after a call has come
back with a device error.

    from tests.guard_util import device_guard  # noqa: F401      (every tests/test_gpu_*.py: autouse in that module)

    guard_util.install(); ...; guard_util.check_all()             (stand-alone workers)
"""
import ctypes
import gc
import re
import sys
import weakref

import numpy as np

try:
    import pytest
except ImportError:         # a stand-alone worker without pytest: install() / check_all() only
    pytest = None

BAND = 64 * 1024            # bytes on either side; a multiple of 256
POISON = 0xFF
_SYNC_TAIL = 256            # the last bytes of the post band go up with tn_h2d: it waits for the stream, memset included
_SHOWN = 16                 # damaged bytes quoted per violation
_GC_ABOVE = 64              # the fixture collects garbage first when more guarded allocations than this are alive

assert BAND % 256 == 0 and BAND >= 64 * 1024

_TN_E_HIP, _TN_E_COMM = -1, -3


class GuardViolation(AssertionError):
    """Raised by check_all(): one line per damaged band."""


class _State:
    installed = False
    orig_init = None
    orig_call = None
    capturing = False       # between tn_graph_begin and tn_graph_end
    device_error = None     # the message of a call that failed in the HIP runtime / RCCL since install()
    dead = None             # a readback of the guard's own failed: reported once, nothing more is read back
    dead_reported = False
    violations = []         # strings, kept until the next check_all()
    n_guarded = 0           # allocations made under the guard
    n_checked = 0           # allocations whose two bands were read back (each check counts)
    n_unpoisoned = 0        # allocations made inside a stream capture: banded, not filled


_S = _State()
_LIVE = weakref.WeakValueDictionary()       # raw pointer -> _Allocation
_ONES = np.full(BAND, POISON, np.uint8)


def _direct(ctx, name, *args):
    """A call of the guard's own: straight to the library, past Context.call's step recorder and timing hook."""
    from theanet_amd import _lib
    rc = getattr(ctx.lib, name)(ctx.h, *args)
    if rc != 0:
        _lib.check(ctx.h, rc, name)


def _quiet():
    """No GPU work of the guard's own now: a capture is open, or the device has reported an error."""
    return _S.capturing or _S.device_error is not None or _S.dead is not None


class _Allocation:
    """One guarded tn_alloc; owned by the DeviceArray whose memory it is (``array._guard``)."""

    def __init__(self, ctx, nbytes, shape, dtype, c8):
        self.ctx, self.nbytes, self.shape, self.dtype, self.c8 = ctx, int(nbytes), shape, dtype, c8
        self.reported = set()           # bands whose damage has been listed already
        self.poisoned = False
        p = ctypes.c_void_p()
        ctx.call("tn_alloc", BAND + self.nbytes + BAND, ctypes.byref(p))      # (recorded like the unguarded tn_alloc)
        self.raw = p.value
        self.ptr = self.raw + BAND
        _S.n_guarded += 1
        _LIVE[self.raw] = self
        if _quiet():
            _S.n_unpoisoned += 1
            return
        total = BAND + self.nbytes + BAND
        _direct(ctx, "tn_memset", self.raw, POISON, total - _SYNC_TAIL)
        _direct(ctx, "tn_h2d", self.raw + total - _SYNC_TAIL, _ONES.ctypes.data, _SYNC_TAIL)
        self.poisoned = True

    def describe(self):
        what = "shape %s dtype %s" % (self.shape, self.dtype)
        if self.c8 is not None:
            what += " (c8 tensor, C x H x W = %d x %d x %d)" % self.c8
        return what

    def check(self, when):
        """Read both bands back; append a line to the pending violations for each damaged one."""
        if not self.poisoned or _quiet() or len(self.reported) == 2:
            return
        buf = np.empty(BAND, np.uint8)
        for band, start, origin in (("pre", self.raw, -BAND), ("post", self.ptr + self.nbytes, 0)):
            if band in self.reported:
                continue
            try:
                _direct(self.ctx, "tn_d2h", buf.ctypes.data, start, BAND)
            except Exception as e:          # the device is gone: say so once, read nothing more
                _S.dead = "reading back a guard band failed: %s" % e
                return
            hit = np.flatnonzero(buf != POISON)
            if hit.size:
                self.reported.add(band)
                first, last = int(hit[0]) + origin, int(hit[-1]) + origin
                where = ("bytes +%d..+%d past the end of" % (first, last) if band == "post" else
                         "bytes %d..%d before the start of" % (first, last))
                _S.violations.append(
                    "%s band of the allocation of %s: %d damaged byte(s), %s the interior (%d bytes); first bytes: %s [%s]"
                    % (band, self.describe(), hit.size, where, self.nbytes,
                       " ".join("%02x" % b for b in buf[hit[:_SHOWN]]), when))
        _S.n_checked += 1

    def release(self):
        if not self.raw:
            return
        if not sys.is_finalizing():
            self.check("found when the array was freed")
        raw, self.raw = self.raw, 0
        self.ctx.lib.tn_free(self.ctx.h, raw)          # as DeviceArray.__del__ frees: the return code is not looked at

    def __del__(self):
        try:
            self.release()
        except Exception:       # interpreter teardown
            pass


def _guarded_init(self, ctx, shape, dtype=np.float32, ptr=None, base=None):
    if ptr is not None:                                 # a view: its memory belongs to (and is checked with) its base
        return _S.orig_init(self, ctx, shape, dtype, ptr=ptr, base=base)
    _S.orig_init(self, ctx, shape, dtype, ptr=0, base=base)            # shape, dtype, size, nbytes; owns nothing
    self._guard = _Allocation(ctx, self.nbytes, self.shape, self.dtype, getattr(self, "c8", None))
    self.ptr = self._guard.ptr


def _guarded_call(self, name, *args):
    from theanet_amd import _lib
    if name == "tn_graph_begin":
        _S.capturing = True
    try:
        return _S.orig_call(self, name, *args)
    except _lib.BackendError as e:
        if name == "tn_graph_begin":
            _S.capturing = False
        m = re.search(r"\(rc=(-?\d+)\)", str(e))
        if m and int(m.group(1)) in (_TN_E_HIP, _TN_E_COMM):
            _S.device_error = "%s: %s" % (name, e)
        raise
    finally:
        if name == "tn_graph_end":
            _S.capturing = False


def record_of(array):
    """The _Allocation behind ``array`` (through its base, for a view / reshape), or None if it is not guarded."""
    return getattr(array.base if array.base is not None else array, "_guard", None)


def install():
    """Guard every DeviceArray allocated from now on (idempotent).  Forgets a device error seen earlier."""
    from theanet_amd import device
    _S.device_error = None
    _S.capturing = False
    if _S.installed:
        return
    _S.orig_init, _S.orig_call = device.DeviceArray.__init__, device.Context.call
    device.DeviceArray.__init__ = _guarded_init
    device.Context.call = _guarded_call
    _S.installed = True


def uninstall():
    """DeviceArray allocates as before.  Arrays guarded so far stay guarded until they die."""
    from theanet_amd import device
    if not _S.installed:
        return
    device.DeviceArray.__init__, device.Context.call = _S.orig_init, _S.orig_call
    _S.orig_init = _S.orig_call = None
    _S.installed = False


def check_all():
    """Check the bands of every live guarded allocation and raise ONE GuardViolation that lists every damaged band found
    since the last call (those found when arrays were freed included).  After a device error: nothing is read back."""
    for alloc in list(_LIVE.values()):
        alloc.check("found by check_all")
    found, _S.violations = _S.violations, []
    if _S.dead is not None and not _S.dead_reported:
        _S.dead_reported = True
        found.append(_S.dead + " -- no further bands are checked in this process")
    if found:
        raise GuardViolation("%d guard violation(s):\n  " % len(found) + "\n  ".join(found))


def stats():
    return {"guarded": _S.n_guarded, "checked": _S.n_checked, "unpoisoned": _S.n_unpoisoned, "live": len(_LIVE)}


def _device_guard(_release_device_temporaries):
    """Function scope, autouse in every module that imports it.  It depends on conftest's _release_device_temporaries,
    so it is set up after and torn down BEFORE that fixture drops the test's arrays: check_all() sees them alive.
    A net is cyclic garbage once its test returns; left to the collector's own schedule, hundreds of dead allocations
    would be read back again after every later test, so they are collected (and checked as they are freed) here."""
    install()
    try:
        yield
        if len(_LIVE) > _GC_ABOVE:
            gc.collect()
        check_all()
    finally:
        uninstall()


if pytest is not None:
    device_guard = pytest.fixture(autouse=True, name="device_guard")(_device_guard)
