"""tn_gather_batch (theanet_amd/csrc/gather.hip; the CPU backend's twin in csrc_cpu): the minibatch of a shuffled epoch
staged in one launch -- rows order[row0 .. row0 + nrows) of the images, their labels and their aux rows.  A bit copy, so
everything is compared as uint32 against numpy indexing, with NaN payloads and infinities in the data; every output
buffer is one row longer than asked for and that row must come back untouched.  The same file runs against the CPU
backend (THEANET_BACKEND=cpu, tests/test_shuffle_cpu.py)."""
import functools

import numpy as np
import pytest

from tests.gpu_util import call, dev
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

N_ROWS = 300            # dataset rows
AUX_FLOATS = 5
GARBAGE = 0xDEADBEEF


@functools.lru_cache(maxsize=None)
def _dataset(floats):
    """(x, y, aux) as uint32 / int32 bit patterns: random words (many of them NaNs with payloads, denormals) and a few
    planted quiet / signalling NaNs and infinities per row."""
    rng = np.random.RandomState(floats)
    x = rng.randint(0, 2 ** 32, (N_ROWS, floats), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000], np.uint32)
    x[:, 0] = special[np.arange(N_ROWS) % len(special)]
    x[:, -1] = special[(np.arange(N_ROWS) + 3) % len(special)]
    y = rng.randint(-2 ** 31, 2 ** 31, N_ROWS, dtype=np.int64).astype(np.int32)
    aux = rng.randint(0, 2 ** 32, (N_ROWS, AUX_FLOATS), dtype=np.uint64).astype(np.uint32)
    aux[:, 2] = special[np.arange(N_ROWS) % len(special)]
    for a in (x, y, aux):
        a.setflags(write=False)
    return x, y, aux


def _order(nrows, row0):
    """An order with repeats that names dataset row 0 and the last dataset row inside the window read."""
    rng = np.random.RandomState(nrows * 16 + row0)
    order = rng.randint(0, N_ROWS, row0 + nrows + 9).astype(np.int32)
    order[row0] = N_ROWS - 1
    order[row0 + nrows - 1] = 0
    if nrows >= 5:
        order[row0 + 2] = order[row0 + 3] = order[row0 + 1]        # repeats
        order[row0 + nrows // 2] = N_ROWS - 1
    return order


@pytest.mark.parametrize("row0", [0, 7])
@pytest.mark.parametrize("nrows", [1, 5, 257])
@pytest.mark.parametrize("floats", [1, 3, 784, 785, 3072])
def test_gather_batch_is_a_bit_copy_of_the_ordered_rows(floats, nrows, row0):
    x, y, aux = _dataset(floats)
    order = _order(nrows, row0)
    d_x, d_y, d_aux, d_order = dev(x), dev(y), dev(aux), dev(order)
    rows = order[row0:row0 + nrows]
    for with_y in (True, False):
        for with_aux in (True, False):
            x_out = dev(np.full((nrows + 1, floats), GARBAGE, np.uint32))
            y_out = dev(np.full((nrows + 1,), GARBAGE, np.uint32).view(np.int32))
            aux_out = dev(np.full((nrows + 1, AUX_FLOATS), GARBAGE, np.uint32))
            call("tn_gather_batch", d_order.ptr, row0, nrows, d_x.ptr, x_out.ptr, floats * 4,
                 d_y.ptr if with_y else None, y_out.ptr if with_y else None,
                 d_aux.ptr if with_aux else None, aux_out.ptr if with_aux else None, AUX_FLOATS * 4 if with_aux else 0)
            got = x_out.get_value()
            np.testing.assert_array_equal(got[:nrows], x[rows])
            assert (got[nrows] == GARBAGE).all()
            got = y_out.get_value().view(np.uint32)
            np.testing.assert_array_equal(got[:nrows], y[rows].view(np.uint32) if with_y else GARBAGE)
            assert got[nrows] == GARBAGE
            got = aux_out.get_value()
            np.testing.assert_array_equal(got[:nrows], aux[rows] if with_aux else GARBAGE)
            assert (got[nrows] == GARBAGE).all()


def test_gather_batch_of_no_rows_is_a_no_op():
    x, y, aux = _dataset(784)
    d_order = dev(np.zeros(4, np.int32))
    x_out = dev(np.full((1, 784), GARBAGE, np.uint32))
    y_out = dev(np.full((1,), GARBAGE, np.uint32).view(np.int32))
    aux_out = dev(np.full((1, AUX_FLOATS), GARBAGE, np.uint32))
    call("tn_gather_batch", d_order.ptr, 2, 0, dev(x).ptr, x_out.ptr, 784 * 4, dev(y).ptr, y_out.ptr, dev(aux).ptr, aux_out.ptr,
         AUX_FLOATS * 4)
    assert (x_out.get_value() == GARBAGE).all() and (aux_out.get_value() == GARBAGE).all()
    assert (y_out.get_value().view(np.uint32) == GARBAGE).all()


@pytest.mark.parametrize("bad", ["row bytes 6", "NULL order", "negative nrows", "y without y_out"])
def test_gather_batch_refusals(bad):
    from theanet_amd import _lib
    x, y, _ = _dataset(3)
    d_x, d_y, d_order = dev(x), dev(y), dev(np.zeros(8, np.int32))
    x_out = dev(np.full((5, 3), GARBAGE, np.uint32))
    y_out = dev(np.full((5,), GARBAGE, np.uint32).view(np.int32))
    args = {"row bytes 6": (d_order.ptr, 0, 4, d_x.ptr, x_out.ptr, 6, d_y.ptr, y_out.ptr, None, None, 0),
            "NULL order": (None, 0, 4, d_x.ptr, x_out.ptr, 12, d_y.ptr, y_out.ptr, None, None, 0),
            "negative nrows": (d_order.ptr, 0, -1, d_x.ptr, x_out.ptr, 12, d_y.ptr, y_out.ptr, None, None, 0),
            "y without y_out": (d_order.ptr, 0, 4, d_x.ptr, x_out.ptr, 12, d_y.ptr, None, None, None, 0)}[bad]
    with pytest.raises(_lib.BackendError, match="tn_gather_batch"):
        call("tn_gather_batch", *args)
    assert (x_out.get_value() == GARBAGE).all() and (y_out.get_value().view(np.uint32) == GARBAGE).all()
