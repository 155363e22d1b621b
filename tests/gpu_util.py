"""Helpers for the -m gpu parity tests: everything goes through the C-ABI."""
import ast
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ctx():
    from theanet_amd.device import get_context
    return get_context()


_KEEP = []      # device arrays made by dev() stay alive until the test ends (conftest clears)


def dev(a, dtype=None):
    d = ctx().array(np.ascontiguousarray(a), dtype=dtype)
    _KEEP.append(d)
    return d


def empty(shape, dtype=np.float32):
    return ctx().empty(shape, dtype)


def call(name, *args):
    ctx().call(name, *args)


def load_prms(name, img_sz=None, seed=555555, batch=None):
    with open(os.path.join(ROOT, "params", name)) as fh:
        prms = ast.literal_eval(fh.read())
    if img_sz is not None:
        prms["layers"][0][1]["img_sz"] = img_sz
    prms["training_params"]["SEED"] = seed
    if batch:
        prms["training_params"]["BATCH_SZ"] = batch
    return prms


def act_code(name):
    from theanet_amd.layer.layer import activation_by_name
    a = activation_by_name(name)
    return a.kind, a.prm


def assert_close(got, want, rtol=1e-4, atol=1e-5, what=""):
    """|got - want| <= atol + rtol * |want| element by element.  A NaN compares false with every bound, so the test is
    "not within", never "beyond": a NaN or an infinity in ``got`` where ``want`` has a finite number is a mismatch
    and where ``want`` is not finite only the same value matches (equal infinities do; a NaN never does)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.astype(np.float64), want.astype(np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(g - w)
        tol = atol + rtol * np.abs(w)
        bad = ~((np.isfinite(w) & (err <= tol)) | (g == w))
        over = np.where(bad, np.where(np.isnan(err - tol), np.inf, err - tol), -np.inf)
    if bad.any():
        i = tuple(int(k) for k in np.unravel_index(np.argmax(over), err.shape))
        nans = int((np.isnan(g) & bad).sum())
        raise AssertionError("%s: %d/%d mismatches%s, worst at %s: got %r want %r" %
                             (what, bad.sum(), bad.size,
                              ", %d of them NaN (an element never written?)" % nans if nans else "",
                              i, got[i], want[i]))
