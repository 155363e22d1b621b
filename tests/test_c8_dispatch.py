"""Coverage of the fp16 conv kernels' instantiations by the GPU tests of tests/test_gpu_c8.py, checked on the CPU.

The launchers of theanet_amd/csrc/conv_c8.hip choose a template instantiation from host-only geometry (c8_plan for
c8_conv_kernel<FT, MODE, NS, LK, TK>: forward, forward + pool, input gradient, pooled input gradient; c8w_plan for the
weight gradient: c8_wgrad_tr_kernel<NCT, NGX, POOL, ROLL> or c8_wgrad_kernel<NFT, NCT, POOL, NGX, TM, ROLL>).
tn_c8_conv_plan runs that same selection without a device.  A sweep over the shapes the kernels accept collects every
reachable instantiation, and every (instantiation, edge) pair; the GPU tests' case lists must reach both sets exactly,
so a new variant or a dispatch change fails here until a GPU case covers it.

Edges (where tiling goes wrong):
  K_tail   the last filter tile is partial: filters % (32 FT) (conv ops; the input gradient's filters are the layer's
           C channels) or K % (32 NFT) (weight gradient) != 0
  C_tail   the last reduction group is partial: channels % 16 != 0 (conv ops: chunks of 16 channels per MFMA step; the
           input gradient reduces over the layer's K) or C % (32 NCT) != 0 (weight gradient channel groups; NCT = 0:
           one octet, C % 8 != 0)
  C_odd    the layer's C % 8 != 0: the padded last octet plane (read by the forward and the weight gradient, written
           by the input gradient)
  N_tail   N % NI != 0: several images share a pixel tile and the last tile is partial
  slab     (weight gradient) the last slab is short: tiles % tiles-per-slab != 0
"""
import ctypes
import functools

from tests import test_gpu_c8 as G

NS_W = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 33, 63, 65, 127, 129, 255, 257, 511, 513, 1023, 1025, 2047, 2049, 2100, 2101,
        4096, 4099]
NS_CONV = [1, 2, 3, 4, 5, 7, 9, 33]          # (the conv ops' geometry sees N only through NI = min(N, 256 / (H W)))
CS = list(range(1, 73)) + list(range(73, 257, 3))
KS = list(range(8, 257, 8))
HS_W = [8, 16, 32, 64]                       # the weight gradient takes rows of 8..64 pixels
HS_CONV = [8, 16, 32, 64, 128]
ACTS = [(G.LEAKY, G.SLOPE), G.ACTS["tanh"]]  # LK is a function of the kind alone: leaky-ReLU family or not
EDGES = ("K_tail", "C_tail", "C_odd", "N_tail", "slab")


@functools.lru_cache(maxsize=None)
def _query():
    from theanet_amd import _lib
    lib = _lib.get_lib()
    out = (ctypes.c_int * 16)()
    f = lib.tn_c8_conv_plan

    def plan(op, N, C, H, K, pool, act, prm):
        n = f(op, N, C, H, H, K, pool, act, prm, out, 16)
        return tuple(out[:n]) if n > 0 else None
    assert plan(2, 3, 16, 16, 32, 0, G.LEAKY, G.SLOPE), "tn_c8_conv_plan answers nothing (CPU backend loaded?)"
    return plan


def classify(op, N, C, H, K, pool, act, prm):
    """(instantiation, set of edges) of one tn_c8_conv_{fwd, dgrad, wgrad} call, or None if the call refuses the shape."""
    p = _query()(op, N, C, H, K, pool, act, prm)
    if p is None:
        return None
    if op == 2:
        tr, NFT, NCT, NGX, TM, ROLL, nstage, NI, S, tpb, ntiles, KG, CG = p
        inst = ("wgrad16", NCT, NGX, pool, ROLL) if tr else ("wgrad8", NFT, NCT, pool, NGX, TM, ROLL)
        edges = {"K_tail": K % (32 * NFT) != 0, "C_tail": C % (32 * NCT if NCT else 8) != 0, "C_odd": C % 8 != 0,
                 "N_tail": N % NI != 0, "slab": ntiles % tpb != 0}
    else:
        FT, MODE, NS, LK, TK, NI, RT, KT, MT = p
        inst = ("conv", FT, MODE, NS, LK, TK)
        filters, chans = (C, K) if op == 1 else (K, C)
        edges = {"K_tail": filters % (32 * FT) != 0, "C_tail": chans % 16 != 0, "C_odd": C % 8 != 0,
                 "N_tail": N % NI != 0}
    return inst, {e for e, on in edges.items() if on}


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
    for H in HS_W:
        for N in NS_W:
            for C in CS:
                for K in KS:
                    for pool in (0, 1):
                        yield 2, N, C, H, K, pool, 0, 0.
    for H in HS_CONV:
        for N in NS_CONV:
            for C in CS:
                for K in KS:
                    for op in (0, 1):
                        for pool in (0, 1):
                            for act, prm in ACTS:
                                yield op, N, C, H, K, pool, act, prm


@functools.lru_cache(maxsize=None)
def sweep():
    return _reach(_sweep_calls())


def _fmt(s):
    return "\n  ".join(sorted(map(str, s)))


# Why an (instantiation, edge) pair cannot occur, or None.  test_unreachable_edges_are_the_documented_ones checks that
# these are exactly the pairs missing from the sweep, so each reason holds for the real selection.  Only N_tail is ever
# unreachable: a partial image tile needs NI > 1, i.e. several images per tile -- 8x8 maps only (conv ops: 256-pixel
# tiles; weight gradient: 128-pixel tiles and, for first layers, 256 / 512).
def _why_unreachable(inst, edge):
    if edge != "N_tail":
        return None
    if inst[0] == "conv":
        _, FT, MODE, NS, LK, TK = inst
        if LK and NS == 2 and not TK:
            # NS = 2 without packed taps: 2 NI 10 rows x 8 cells <= 512 staged cells, so NI <= 3 -- and NI = min(4, N),
            # hence NI = N: one tile of all the images
            return "NI = N"
        if LK and NS == 4:
            return "leaky NS = 4 only at 128-pixel rows: NI = 1"
        return None
    if inst[0] == "wgrad16":
        _, NCT, NGX, pool, ROLL = inst
        return "the ring holds bands of one image: NI = 1" if ROLL else None
    _, NFT, NCT, pool, NGX, TM, ROLL = inst
    if ROLL:
        return "the ring holds bands of one image: NI = 1"
    if NCT == 2 and NGX == 3:
        # at 8x8 (NI = 2) the halo tile of two images is 200 cells = 4 KB chunks per octet plane, 8 planes over 8 waves
        return "NGX = 3 only on rows of >= 16 pixels: NI = 1"
    return None


def test_plan_query_runs_the_launchers_selection():
    """Spot checks of the query against the documented selection: FT / NFT from K, NCT from C, LK from the kind."""
    plan = _query()
    assert plan(0, 3, 16, 16, 24, 0, G.LEAKY, G.SLOPE)[:5] == (1, 0, 3, 1, 0)
    assert plan(0, 3, 16, 16, 24, 1, *G.ACTS["tanh"])[:5] == (1, 1, 4, 0, 0)
    assert plan(0, 3, 3, 16, 64, 0, G.LEAKY, G.SLOPE)[:5] == (2, 0, 2, 1, 1)          # C <= 8: taps packed
    assert plan(1, 3, 3, 16, 64, 0, G.LEAKY, G.SLOPE)[:5] == (1, 2, 3, 1, 0)          # dgrad: filters = C, no taps packed
    assert plan(0, 2, 16, 128, 64, 0, G.LEAKY, G.SLOPE)[2] == 4
    assert plan(0, 3, 16, 16, 20, 0, G.LEAKY, G.SLOPE) is None                        # K % 8
    assert plan(0, 3, 16, 12, 16, 0, G.LEAKY, G.SLOPE) is None                        # 12-pixel rows
    assert plan(2, 3, 16, 128, 16, 0, 0, 0.) is None                                  # wgrad: rows of 8..64 pixels
    w = plan(2, 40, 32, 16, 64, 0, 0, 0.)
    assert w[:3] == (1, 2, 1) and w[8] * w[9] >= w[10] > (w[8] - 1) * w[9]          # S slabs of tpb tiles cover them
    assert plan(2, 2100, 8, 16, 32, 0, 0, 0.)[:6] == (0, 1, 0, 2, 4, 0)                # first layer: 512-pixel tiles


def test_supported_shapes_have_a_plan():
    """Every shape both capability queries accept (what a float16 net is built from) has a launch plan, unless its
    tensors exceed the kernels' 32-bit cell offsets (N C8 H W >= 2^28 cells)."""
    from theanet_amd import _lib
    lib = _lib.get_lib()
    plan = _query()
    for H in HS_W:
        for N in (1, 7, 513, 4099):
            for C in (1, 3, 8, 9, 20, 32, 33, 64, 100, 256):
                for K in (8, 16, 32, 40, 64, 72, 128, 256):
                    if not (lib.tn_c8_conv_supported(N, C, H, H, K, 3, 1, 1) and lib.tn_c8_conv_wgrad_supported(N, C, H, H, K)):
                        continue
                    if N * ((max(C, K) + 7) // 8) * H * H >= 1 << 28:
                        continue
                    for op in (0, 1, 2):
                        for pool in (0, 1):
                            assert plan(op, N, C, H, K, pool, G.LEAKY, G.SLOPE), (op, N, C, H, K, pool)


def test_gpu_cases_reach_every_instantiation():
    """The launches of tests/test_gpu_c8.py reach exactly the instantiations the sweep reaches."""
    insts, _ = sweep()
    got, _ = _reach(G.c8_launches())
    assert not got - insts, "GPU cases launch instantiations the sweep does not reach:\n  " + _fmt(got - insts)
    assert not insts - got, "instantiations no GPU case of tests/test_gpu_c8.py launches:\n  " + _fmt(insts - got)


def test_gpu_cases_reach_every_edge_of_every_instantiation():
    _, pairs = sweep()
    _, got = _reach(G.c8_launches())
    missing = pairs - got
    assert not missing, "(instantiation, edge) pairs no GPU case of tests/test_gpu_c8.py reaches:\n  " + _fmt(missing)


def test_unreachable_edges_are_the_documented_ones():
    insts, pairs = sweep()
    edges = {i: EDGES if i[0] != "conv" else EDGES[:4] for i in insts}       # (the conv ops have no slabs)
    absent = {(i, e) for i in insts for e in edges[i] if (i, e) not in pairs}
    documented = {(i, e) for i in insts for e in edges[i] if _why_unreachable(i, e)}
    assert absent == documented, ("undocumented:\n  " + _fmt(absent - documented) +
                                  "\ndocumented but reachable:\n  " + _fmt(documented - absent))
