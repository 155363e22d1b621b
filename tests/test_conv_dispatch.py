"""Coverage of the fp32 conv kernels' instantiations by the GPU tests of tests/test_gpu_kernels.py, checked on the CPU.

tn_conv2d_fwd, tn_conv2d_wgrad and tn_conv2d_dgrad choose among the kernels of theanet_amd/csrc/conv.hip, conv_mfma.hip and
conv_tile.hip (its POOL = false instantiations) from the shape, stride, padding, the operands' alignment, the CU count and
the knobs.  tn_conv_plan runs that same selection (conv_route and the plan functions the launchers themselves call)
without a device.  A sweep at 256 CUs collects every reachable instantiation and every (instantiation, edge) pair; the
launches the GPU tests make (test_gpu_kernels.conv_launches) must reach both sets exactly, so a new variant or a dispatch
change fails here until a GPU case covers it.  The fused blocks (convpool.hip, convblock*.hip, the POOL = true
instantiations) and CONV 'bfloat16' are not part of this.

Instantiations: (kernel, template arguments...) as tn_conv_plan reports them:
  (fwd_direct, F, KT)  (wgrad_direct, F, KT, CT)  (dgrad_direct, F, CT)  (dgrad_lds,)  (wgrad_generic,)
  (mfma, PADDED, DGRAD)  (mfma_wgrad, PADDED)  (tile, FT, DGRAD, NCP)  (tile_wgrad, NFT)  (tile_smallc,)

Edges (where tiling goes wrong).  A layer is (N, C, H, H) -> K maps (Ho, Ho), window f, the modes 'valid' (any stride) and
'same' (stride 1), so pad_lo is 0 or f - 1 - (f - 1) // 2.
Direct forward / input gradient (a thread per output pixel, blocks of 256; KT filters / CT channels per thread):
  pix_tail    the last 256-pixel block is partial          pix_blocks  more than one pixel block
  k_tail / c_tail   a partial last KT / CT group           stride      stride > 1
  pad         zero padding (pad_lo > 0)                    pad_asym    pad_lo != pad_hi ('same' with an even window)
  prev / bare input gradient with / without the act' of the layer below
Direct weight gradient (nblk blocks stride over the pixels, one slab each; tn_conv_wgrad_finish sums and flips them):
  slabs       nblk > 1                                     short_slab  the blocks' last round of 256 pixels is partial
  k_tail, c_tail, stride, pad, pad_asym as above
conv_dgrad_lds (G images of dz in LDS, 4 channels per block):
  G1 .. G4    the group size                               n_tail      N % G != 0
  c_tail      C % 4 != 0                                   pad1, pad2  the halo the kernel reads (2 - pad_lo)
  prev / bare
Generic weight gradient: stride, pad, pad_asym
MFMA forward / input gradient (64 x 64 tiles over rows x pixels, 16-deep reduction tiles; rows = K, or C for dgrad):
  m_tail      pixels % 64 != 0                             rows_tail   rows % 64 != 0
  row_tiles   more than one row tile                       kd_tail     reduction depth % 16 != 0
  ntile_odd / ntile_even   the parity of the number of reduction tiles (the pipeline's tail)
  a_scalar    the A rows are not loaded 16 bytes at a time: depth % 4 != 0
  a_unal      ... because W is not 16-byte aligned (forward; the input gradient's transposed weights are scratch)
  grid_pad    pixel tiles % 8 != 0: blocks beyond the last tile return
  prev / bare
MFMA weight gradient (S pixel slabs of mchunk pixels):
  S8 S16 S32 S64   the slab count                          short_slab  the last slab that has pixels is short
  empty_slabs  slabs beyond the pixels                     kd_tail     C*f*f % 64 != 0
  k_tail      K % 64 != 0                                  kd_tiles    more than one tile over C*f*f
LDS-tile forward / input gradient (a block = NI whole images or TH rows of one, 32 FT filters, chunks of 8 channels;
for the input gradient the filters are the C input maps and the channels the K maps):
  NI          several images per tile                      n_tail      N % NI != 0
  RT          several row tiles per image
  row_tail_v / row_tail_s   the last row tile is partial, under the 16-byte / the scalar epilogue (whose guards cut it)
  k_tail      filters % (32 FT) != 0                       c_tail      channels % 8 != 0
  chunks      more than one channel chunk                  pad0 pad1 pad2   the kernel's padding
  scalar_out  the epilogue does not store 16 bytes: row length % 4 != 0
  out_unal    ... because out or prev_a is not 16-byte aligned
  grid_pad    pixel tiles % 8 != 0                         prev / bare
LDS-tile weight gradient (32 NFT filters x 32 channels x a slab of images per block):
  NI, RT as above                                          slabs       S > 1
  slab_tail   N % (images per slab) != 0                   img_tail    N % NI != 0
  k_tail      K % (32 NFT) != 0                            c_tail      C % 32 != 0
  grid_pad    S % 8 != 0
Small-C weight gradient: C1 C2 C3 (the channel count), k_tail (K % 32), slabs, NI, RT, slab_tail, img_tail
Routes the alignment flags open (an edge of the kernel that runs instead):
  unal_from_tile     an MFMA product that the LDS-tile kernels would run with aligned operands
  unal_from_smallc   a direct weight gradient that the small-C kernel would run
"""
import ctypes
import functools

import pytest

from tests import test_gpu_kernels as G
from tests.test_abi import KNOB_DEFAULTS

CUS = 256
F_UNAL, F_BARE, F_UNAL_OUT, F_UNAL_W = 1, 2, 4, 8
FWD, WGRAD, DGRAD = range(3)
NINTS = 16
R_TILE, R_SMALLC, R_MFMA = 1, 2, 3
KERNELS = ("fwd_direct", "wgrad_direct", "dgrad_direct", "dgrad_lds", "wgrad_generic", "mfma", "mfma_wgrad", "tile",
           "tile_wgrad", "tile_smallc")
NARGS = (2, 3, 2, 0, 0, 2, 1, 3, 1, 0)         # template arguments that tell instantiations apart (dgrad_lds has one F)

# dense around the thresholds of the selection: C*f*f = 32 and C*9 = 32 (C = 3, 4; 8, 9; 32 at f = 1), K = 16 and 32 (and the
# 64-row tiles), C = 2, 4, 8, 16, row lengths % 4, the power-of-two maps of the tile weight gradient, the 60 KiB of
# conv_dgrad_lds, M = 4096 pixels per direct slab, the MFMA slab rule (blocks against 2 x 256, M / 2S against 128)
NS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 64, 70, 200]
CS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 32, 33, 64]
KS = [1, 3, 4, 8, 15, 16, 17, 31, 32, 33, 40, 64, 65, 96]
HS = [4, 5, 7, 8, 9, 12, 13, 14, 16, 17, 18, 28, 32, 33, 40, 63, 64]
FS = [1, 2, 3, 4, 5, 7]
MODES = [(1, "valid"), (1, "same"), (2, "valid"), (3, "valid")]
PROD_FLAGS = {FWD: [a | b | c for a in (0, F_UNAL) for b in (0, F_UNAL_OUT) for c in (0, F_UNAL_W)],
              WGRAD: [0, F_UNAL],
              DGRAD: [a | b | c for a in (0, F_UNAL) for b in (0, F_BARE) for c in (0, F_UNAL_OUT)]}
N_ALL_FLAGS = (1, 3, 8, 70)                    # the alignment flags change nothing that depends on N beyond these


def geometry(H, f, s, mode):
    """(pad_lo, Ho) of the layer, None where the reference refuses it (oracle.conv_geometry)."""
    if mode == "same":
        return (f - 1 - (f - 1) // 2, H) if s == 1 else None
    out = (H - f + 1) // s
    return (0, out) if out > 0 and out == (H - f) // s + 1 else None


@functools.lru_cache(maxsize=None)
def _query():
    from theanet_amd import _lib
    lib = _lib.get_lib()
    buf = ctypes.create_string_buffer(4096)
    assert lib.tn_knobs(buf, len(buf)) == 0
    knobs = dict(kv.split("=") for kv in buf.value.decode().split())
    off = sorted(k for k, v in KNOB_DEFAULTS.items() if int(knobs[k]) != v)
    if off:
        pytest.skip("the dispatch coverage holds for the default selection only; unset " + ", ".join(off))
    out = (ctypes.c_int * NINTS)()
    f = lib.tn_conv_plan

    def plan(prod, N, C, H, K, f_, s, pad, Ho, flags=0, cus=CUS):
        n = f(prod, N, C, H, H, K, f_, s, pad, Ho, Ho, cus, flags, out, NINTS)
        return tuple(out) if n == NINTS else None
    assert plan(FWD, 2, 16, 16, 32, 3, 1, 1, 16), "tn_conv_plan answers nothing (CPU backend loaded?)"
    return plan


def classify(prod, N, C, H, K, f, s, mode, flags=0):
    """(instantiation, set of edges) of the kernel one tn_conv2d_* call launches; None where the call refuses."""
    geo = geometry(H, f, s, mode)
    if geo is None:
        return None
    pad, Ho = geo
    plan = _query()
    rec = plan(prod, N, C, H, K, f, s, pad, Ho, flags)
    if rec is None:
        return None
    route, ker = rec[:2]
    t, v = rec[2:6], rec[6:]
    name = KERNELS[ker]
    inst = (name,) + tuple(t[:NARGS[ker]])
    assert not any(t[NARGS[ker] + (name == "dgrad_lds"):])
    prev = "bare" if flags & F_BARE else "prev"
    geo_e = {"stride": s > 1, "pad": pad > 0, "pad_asym": mode == "same" and f % 2 == 0}
    if name in ("fwd_direct", "dgrad_direct"):
        M = N * (Ho * Ho if prod == FWD else H * H)
        assert v[0] == -(-M // 256)
        e = dict(geo_e, pix_tail=M % 256 != 0, pix_blocks=v[0] > 1)
        e["k_tail" if prod == FWD else "c_tail"] = (K if prod == FWD else C) % t[1] != 0
    elif name == "wgrad_direct":
        M, nblk = N * Ho * Ho, v[0]
        e = dict(geo_e, slabs=nblk > 1, short_slab=nblk > 1 and M % (256 * nblk) != 0, k_tail=K % t[1] != 0,
                 c_tail=C % t[2] != 0)
    elif name == "dgrad_lds":
        e = {"G%d" % v[0]: True, "n_tail": N % v[0] != 0, "c_tail": C % 4 != 0, "pad%d" % (2 - pad): True}
    elif name == "wgrad_generic":
        e = geo_e
    elif name == "mfma":
        KT, MT, Kd, M, a_vec = v[:5]
        rows = C if prod == DGRAD else K
        ntile = -(-Kd // 16)
        e = {"m_tail": M % 64 != 0, "rows_tail": rows % 64 != 0, "row_tiles": KT > 1, "kd_tail": Kd % 16 != 0,
             "ntile_odd": ntile % 2 == 1, "ntile_even": ntile % 2 == 0, "grid_pad": MT % 8 != 0,
             "a_unal" if Kd % 4 == 0 else "a_scalar": not a_vec}
        assert a_vec or Kd % 4 or flags & F_UNAL_W
    elif name == "mfma_wgrad":
        KT, MT, Kd, M, S, mchunk = v[:6]
        assert S in (8, 16, 32, 64) and mchunk % 16 == 0 and S * mchunk >= M
        e = {"S%d" % S: True, "short_slab": M % mchunk != 0, "empty_slabs": (S - 1) * mchunk >= M, "kd_tail": Kd % 64 != 0,
             "k_tail": K % 64 != 0, "kd_tiles": MT > 1}
    elif name == "tile":
        KT, MT, RT, NI, TH, nchunk, vec_out, kpad = v[:8]
        filt, chan, Hout = (C, K, H) if prod == DGRAD else (K, C, Ho)
        assert MT == -(-N // NI) * RT and (RT == 1 or NI == 1)
        e = {"NI": NI > 1, "n_tail": N % NI != 0, "RT": RT > 1,
             "row_tail_v" if vec_out else "row_tail_s": RT > 1 and Hout % TH != 0, "k_tail": filt % (32 * t[0]) != 0, "c_tail": chan % 8 != 0, "chunks": nchunk > 1, "pad%d" % kpad: True,
             "out_unal" if Hout % 4 == 0 else "scalar_out": not vec_out, "grid_pad": MT % 8 != 0}
        assert vec_out or Hout % 4 or flags & F_UNAL_OUT
    elif name == "tile_wgrad":
        KG, CG, S, ipb, NI, RT, NT = v[:7]
        e = {"NI": NI > 1, "RT": RT > 1, "slabs": S > 1, "slab_tail": N % ipb != 0, "img_tail": N % NI != 0,
             "k_tail": K % (32 * t[0]) != 0, "c_tail": C % 32 != 0, "grid_pad": S % 8 != 0}
    else:
        KG, S, ipb, NI, RT, NT = v[:6]
        e = {"C%d" % C: True, "k_tail": K % 32 != 0, "slabs": S > 1, "NI": NI > 1, "RT": RT > 1, "slab_tail": N % ipb != 0,
             "img_tail": N % NI != 0}
    if prod == DGRAD:
        e[prev] = True
        assert v[{"dgrad_direct": 2, "dgrad_lds": 4, "mfma": 5, "tile": 8}[name]] == (prev == "prev")
    if flags & F_UNAL:
        was = plan(prod, N, C, H, K, f, s, pad, Ho, flags & ~F_UNAL)[0]
        if was != route:
            assert (was, route) in ((R_TILE, R_MFMA), (R_SMALLC, 5)) or (was == R_TILE and prod == FWD and route == 5), (was, route)
            e["unal_from_tile" if was == R_TILE else "unal_from_smallc"] = True
    return inst, {k for k, on in e.items() if on}


def _reach(calls):
    insts, pairs = set(), set()
    for c in calls:
        got = classify(*c)
        assert got is not None, "the call refuses: %s" % (c,)
        insts.add(got[0])
        pairs.update((got[0], e) for e in got[1])
    return insts, pairs


def sweep_calls():
    for f in FS:
        for s, mode in MODES:
            for H in HS:
                if geometry(H, f, s, mode) is None:
                    continue
                for C in CS:
                    for K in KS:
                        for N in NS:
                            for prod, flagset in PROD_FLAGS.items():
                                for fl in flagset if N in N_ALL_FLAGS else (x for x in flagset if not x & ~F_BARE):
                                    yield prod, N, C, H, K, f, s, mode, fl


@functools.lru_cache(maxsize=None)
def sweep():
    return _reach(sweep_calls())


@functools.lru_cache(maxsize=None)
def gpu_reach():
    return _reach(G.conv_launches())


def _fmt(s):
    return "\n  ".join(sorted(map(str, s)))


def test_plan_query_runs_the_launchers_selection():
    """Spot checks of the query against the documented selection."""
    plan = _query()

    def k(prod, N, C, H, K, f, s, mode, flags=0):
        pad, Ho = geometry(H, f, s, mode)
        r = plan(prod, N, C, H, K, f, s, pad, Ho, flags)
        return (KERNELS[r[1]],) + r[2:6]
    assert k(FWD, 3, 1, 28, 4, 3, 1, "valid") == ("fwd_direct", 3, 4, 0, 0)           # mnist.prms conv1
    assert k(FWD, 2, 4, 9, 8, 2, 2, "valid") == ("fwd_direct", 0, 8, 0, 0)
    assert k(WGRAD, 2, 4, 13, 6, 3, 1, "valid") == ("wgrad_direct", 3, 4, 4, 0)
    assert k(WGRAD, 2, 2, 8, 3, 4, 1, "same") == ("wgrad_generic", 0, 0, 0, 0)
    assert k(DGRAD, 2, 8, 18, 32, 3, 1, "valid") == ("dgrad_lds", 3, 0, 0, 0)        # C = 8 < 16 rows: no matrix core
    assert k(DGRAD, 2, 16, 14, 16, 3, 1, "valid") == ("tile", 1, 1, 4, 0)
    assert k(DGRAD, 2, 16, 14, 16, 3, 1, "valid", F_UNAL) == ("mfma", 1, 1, 0, 0)
    assert k(FWD, 3, 3, 32, 32, 3, 1, "same") == ("tile", 1, 0, 2, 0)                 # cifar_like conv1: two channel pairs
    assert k(FWD, 3, 3, 32, 32, 3, 1, "same", F_UNAL) == ("fwd_direct", 3, 8, 0, 0)
    assert k(FWD, 2, 16, 32, 64, 3, 1, "same") == ("tile", 2, 0, 4, 0)
    assert k(FWD, 2, 24, 7, 40, 2, 1, "valid") == ("mfma", 0, 0, 0, 0)
    assert k(WGRAD, 3, 3, 32, 32, 3, 1, "same") == ("tile_smallc", 0, 0, 0, 0)
    assert k(WGRAD, 3, 3, 32, 32, 3, 1, "same", F_UNAL) == ("wgrad_direct", 3, 4, 2, 0)
    assert k(WGRAD, 3, 20, 32, 64, 3, 1, "same") == ("tile_wgrad", 2, 0, 0, 0)
    assert k(WGRAD, 3, 20, 32, 64, 3, 1, "same", F_UNAL) == ("mfma_wgrad", 1, 0, 0, 0)
    pad, Ho = geometry(13, 3, 1, "valid")
    big = plan(WGRAD, 64, 4, 13, 20, 3, 1, pad, Ho)                                   # C*9 = 36: the MFMA kernel, 32 slabs
    assert KERNELS[big[1]] == "mfma_wgrad" and big[10] == 32
    assert plan(FWD, 0, 4, 13, 20, 3, 1, pad, Ho) is None and plan(3, 2, 4, 13, 20, 3, 1, pad, Ho) is None
    assert plan(FWD, 2, 4, 13, 20, 3, 0, pad, Ho) is None


def test_cpu_backend_has_no_plan():
    from theanet_amd import _lib
    import os
    if not os.path.isfile(_lib.CPU_LIB_PATH):
        pytest.skip("libtheanet_cpu.so not built")
    lib = _lib.bind(_lib.CPU_LIB_PATH, ctypes.RTLD_LOCAL)
    out = (ctypes.c_int * NINTS)()
    assert lib.tn_conv_plan(0, 2, 16, 16, 16, 32, 3, 1, 1, 16, 16, 256, 0, out, NINTS) < 0


def test_gpu_cases_reach_every_instantiation():
    """The launches of tests/test_gpu_kernels.py reach exactly the instantiations the sweep reaches."""
    insts, _ = sweep()
    got, _ = gpu_reach()
    assert not got - insts, "GPU cases launch instantiations the sweep does not reach:\n  " + _fmt(got - insts)
    assert not insts - got, "instantiations no GPU case of tests/test_gpu_kernels.py launches:\n  " + _fmt(insts - got)


def test_gpu_cases_reach_every_edge_of_every_instantiation():
    _, pairs = sweep()
    _, got = gpu_reach()
    assert not got - pairs, "GPU cases reach pairs the sweep does not:\n  " + _fmt(got - pairs)
    missing = pairs - got
    assert not missing, "(instantiation, edge) pairs no GPU case of tests/test_gpu_kernels.py reaches:\n  " + _fmt(missing)


def test_every_new_case_adds_a_pair():
    """A case of CONV_CASES_NEW / CONV_UNAL_CASES that reaches nothing the other cases do not is left out."""
    calls = list(G.conv_launches(tagged=True))
    _, every = gpu_reach()
    idle = []
    for tag in sorted({t for t, _ in calls if t is not None}, key=str):
        _, rest = _reach(c for t, c in calls if t != tag)
        if rest == every:
            idle.append(tag)
    assert not idle, "cases that add no (instantiation, edge) pair: %s" % idle


# The compiled instantiations (the switch tables of conv.hip, ct_run, cw_run and the MFMA launchers; POOL = false).
COMPILED = ({("fwd_direct", F, KT) for F in (3, 5, 0) for KT in (8, 4)} |
            {("wgrad_direct",) + a for a in ((3, 4, 4), (3, 4, 2), (3, 4, 1), (5, 2, 2), (5, 4, 1), (2, 4, 4), (2, 4, 1), (1, 8, 4),
                                             (1, 8, 1))} |
            {("dgrad_direct", F, CT) for F in (3, 0) for CT in (8, 4)} | {("dgrad_lds",), ("wgrad_generic",), ("tile_smallc",)} |
            {("mfma", 1, 0), ("mfma", 0, 0), ("mfma", 1, 1), ("mfma_wgrad", 1), ("mfma_wgrad", 0)} |
            {("tile", FT, 0, NCP) for FT in (1, 2) for NCP in (2, 4)} | {("tile", FT, 1, 4) for FT in (1, 2)} |
            {("tile_wgrad", 1), ("tile_wgrad", 2)})


def test_every_compiled_instantiation_is_reachable():
    insts, _ = sweep()
    assert not insts - COMPILED, "the sweep reaches instantiations this list does not know:\n  " + _fmt(insts - COMPILED)
    assert not COMPILED - insts, "compiled but reached by no shape of the sweep:\n  " + _fmt(COMPILED - insts)
