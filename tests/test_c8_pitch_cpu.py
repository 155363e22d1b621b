"""Padded pitch on the 16-bit conv stack, the parts that need no GPU: tn_c8_conv_plan_pitch against tn_c8_conv_plan, and
the coverage of every padded instantiation and edge by the GPU cases of tests/test_gpu_c8_pitch.py.

A c8 tensor of S x S maps may be stored at a power-of-two side P > S with zero pad rows and columns (theanet_amd/csrc/
conv_c8.hip, "padded pitch").  The conv kernels then run on the P x P shape and the forward / input gradient clear their
output's pad; tn_c8_conv_plan_pitch reports that sequence: tn_c8_conv_plan's answer at P followed by a 1.  A sweep over
padded shapes collects every (instantiation, edge) pair it reaches -- edges as in tests/test_c8_dispatch.py -- and the
launches of tests/test_gpu_c8_pitch.py must reach all of them."""
import ctypes
import functools

from tests import test_c8_dispatch as D
from tests import test_gpu_c8 as G
from tests import test_gpu_c8_pitch as GP

PITCHES = [8, 16, 32, 64]


@functools.lru_cache(maxsize=None)
def _queries():
    from theanet_amd import _lib
    lib = _lib.get_lib()
    out = (ctypes.c_int * 16)()
    fp, f = lib.tn_c8_conv_plan_pitch, lib.tn_c8_conv_plan

    def plan_pitch(op, N, C, S, P, K, pool, act, prm):
        n = fp(op, N, C, S, P, K, pool, act, prm, out, 16)
        return tuple(out[:n]) if n > 0 else None

    def plan(op, N, C, H, K, pool, act, prm):
        n = f(op, N, C, H, H, K, pool, act, prm, out, 16)
        return tuple(out[:n]) if n > 0 else None
    assert plan_pitch(2, 3, 16, 14, 16, 32, 0, G.LEAKY, G.SLOPE), "tn_c8_conv_plan_pitch answers nothing (CPU backend?)"
    return plan_pitch, plan


def classify(op, N, C, S, P, K, pool, act, prm):
    """(instantiation, set of edges) of one padded call (S < P) -- the kernel at P, marked padded -- or None if refused."""
    plan_pitch, plan = _queries()
    p = plan_pitch(op, N, C, S, P, K, pool, act, prm)
    if p is None:
        return None
    assert p[-1] == 1 and p[:-1] == plan(op, N, C, P, K, pool, act, prm), (op, N, C, S, P, K, pool)
    r = D.classify(op, N, C, P, K, pool, act, prm)
    return ("padded",) + r[0], r[1]


def _reach(calls):
    insts, pairs = set(), set()
    for c in calls:
        r = classify(*c)
        if r is None:
            continue
        insts.add(r[0])
        pairs.update((r[0], e) for e in r[1])
    return insts, pairs


def _sweep_calls():
    # (the plan does not depend on S beyond its validity: one even side per pitch)
    for P in PITCHES:
        S = P - 2
        for N in D.NS_W:
            for C in D.CS:
                for K in D.KS:
                    for pool in (0, 1):
                        yield 2, N, C, S, P, K, pool, 0, 0.
        for N in D.NS_CONV:
            for C in D.CS:
                for K in D.KS:
                    for op in (0, 1):
                        for pool in (0, 1):
                            for act, prm in D.ACTS:
                                yield op, N, C, S, P, K, pool, act, prm


@functools.lru_cache(maxsize=None)
def sweep():
    return _reach(_sweep_calls())


def _fmt(s):
    return "\n  ".join(sorted(map(str, s)))


def test_pitch_query_equals_plan_query_when_unpadded():
    plan_pitch, plan = _queries()
    n = 0
    for H in D.HS_CONV:
        for N in (1, 3, 7, 33):
            for C in (1, 3, 8, 12, 16, 40, 64, 256):
                for K in (8, 16, 24, 40, 64, 128, 256):
                    for op in (0, 1, 2):
                        for pool in (0, 1):
                            for act, prm in D.ACTS:
                                want = plan(op, N, C, H, K, pool, act, prm)
                                assert plan_pitch(op, N, C, H, H, K, pool, act, prm) == want, (op, N, C, H, K, pool)
                                n += want is not None
    assert n > 1000
    # refusals are the same too
    assert plan_pitch(0, 3, 16, 12, 12, 16, 0, G.LEAKY, G.SLOPE) is None
    assert plan_pitch(0, 3, 16, 16, 16, 20, 0, G.LEAKY, G.SLOPE) is None


def test_pitch_query_limits():
    plan_pitch, plan = _queries()
    assert plan_pitch(0, 3, 16, 28, 32, 32, 0, G.LEAKY, G.SLOPE) == plan(0, 3, 16, 32, 32, 0, G.LEAKY, G.SLOPE) + (1,)
    assert plan_pitch(1, 3, 16, 7, 8, 32, 0, G.LEAKY, G.SLOPE) == plan(1, 3, 16, 8, 32, 0, G.LEAKY, G.SLOPE) + (1,)
    assert plan_pitch(2, 3, 16, 5, 8, 32, 1, 0, 0.) is None              # a pool on an odd side
    assert plan_pitch(0, 3, 16, 7, 8, 32, 1, G.LEAKY, G.SLOPE) is None
    assert plan_pitch(0, 3, 16, 3, 4, 32, 0, G.LEAKY, G.SLOPE) is None   # pitch below 8
    assert plan_pitch(0, 3, 16, 80, 128, 32, 0, G.LEAKY, G.SLOPE) is None  # maps above 64
    assert plan_pitch(0, 3, 16, 20, 24, 32, 0, G.LEAKY, G.SLOPE) is None  # pitch not a power of two
    assert plan_pitch(0, 3, 16, 40, 32, 32, 0, G.LEAKY, G.SLOPE) is None  # side above the pitch
    assert plan_pitch(0, 3, 16, 28, 32, 20, 0, G.LEAKY, G.SLOPE) is None  # filters not a multiple of 8


def test_c8_pitch_rule():
    from theanet_amd.device import c8_pitch
    assert [c8_pitch(s) for s in (1, 5, 7, 8, 9, 14, 16, 20, 24, 28, 32, 33, 48, 64)] == \
        [8, 8, 8, 8, 16, 16, 16, 32, 32, 32, 32, 64, 64, 64]


def test_cpu_backend_refuses_the_pitch_ops():
    """The CPU backend keeps refusing the c8 ops, the new ones included (build() makes both libraries)."""
    from theanet_amd import _lib
    lib = _lib.bind(_lib.CPU_LIB_PATH, ctypes.RTLD_LOCAL)
    out = (ctypes.c_int * 16)()
    assert lib.tn_c8_conv_plan_pitch(0, 3, 16, 28, 32, 32, 0, G.LEAKY, G.SLOPE, out, 16) < 0
    assert lib.tn_c8_conv_plan_pitch(0, 3, 16, 32, 32, 32, 0, G.LEAKY, G.SLOPE, out, 16) < 0


def test_gpu_cases_reach_every_padded_instantiation():
    insts, _ = sweep()
    got, _ = _reach(GP.c8_pitch_launches())
    assert insts, "the sweep reaches nothing"
    assert not got - insts, "GPU cases launch padded instantiations the sweep does not reach:\n  " + _fmt(got - insts)
    assert not insts - got, "padded instantiations no GPU case of tests/test_gpu_c8_pitch.py launches:\n  " + _fmt(insts - got)


def test_gpu_cases_reach_every_edge_of_every_padded_instantiation():
    _, pairs = sweep()
    _, got = _reach(GP.c8_pitch_launches())
    missing = pairs - got
    assert not missing, "(padded instantiation, edge) pairs no GPU case of tests/test_gpu_c8_pitch.py reaches:\n  " + \
        _fmt(missing)
