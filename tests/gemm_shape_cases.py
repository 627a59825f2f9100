"""Case table of the GEMM shape-boundary matrix (tests/test_gpu_gemm_shapes.py, tests/test_host_gemm_shapes.py): every
kernel family either side of its tile, vector, split and dispatch edges.

A family is one kernel (or the default dispatch) pinned by the env switches of the epilogue matrix.  Its shapes are one
ragged base shape swept ONE AXIS AT A TIME through {edge - step, edge, edge + step} for every edge of that axis, the 27
corner shapes around one (M, N, K) tile corner, the fp32 families' alignment cases, and a few extra sizes.  `step` is the
granule the contract sets for the axis (1 for fp32 tensors; 8 along the contiguous extent of a bf16 operand; 4 where the
float4 epilogue is what the family needs).  Every shape is run through the few probes whose code depends on raggedness
(PROBES), names the kernel the dispatcher must pick for it (`expected_kernel`: a mirror of the dispatch conditions, each
cited next to the code that restates it) or is listed as refused.  The comparison is `check_case` of
tests/gemm_epilogue_cases.py against tests/gemm_epilogue_ref.py, bars unchanged.

Inputs: A and B are +-U[0.75, 1.25] K^(-1/4) (rounded to bf16 where the matrix cores read bf16).  Every product term
|A_ik B_jk| is then at least 0.5625 / sqrt(K) while an element of the product stays O(1), so ONE missing, doubled or
misplaced k-term in ONE element is larger than that element's bar (`term_margin`; the host test holds every case to
>= 1.5).  With N(0, 1) operands a dropped term is often far below the bar."""
import functools
from collections import namedtuple

import torch

from tests import gemm_epilogue_cases as T
from tests import gemm_epilogue_ref as R
from tests.parity import ATOL_RMS, RTOL

Case = T.Case
CASE_BUDGET = 100                          # shapes per family (the issue asks for roughly 60 - 90)

# ------------------------------------------------------------------------------------------------ probes
_BARE = Case("bare", False, False, False, False, False, False, False, False, T.ACT_NONE, False, False, False)
_LOADED = Case("loaded", rb=False, pre=True, dact=False, res=True, acc=False, cwin=False, split=False, bias=True,
               act=T.ACT_GELU_TANH, drop=True, c16=False, p16=False)
PROBES = {
    "bare": _BARE,                                   # alpha only
    "loaded": _LOADED,                               # bias, tanh-GELU with a stored pre-activation, residual, dropout
    "split": _BARE._replace(split=True),             # split_k asked for SPLIT_ASKED
    "cwin": _BARE._replace(cwin=True),               # window scatter of C (N even)
    "c16": _BARE._replace(c16=True),                 # bf16 C (tecm_gemm_bf16, float4-friendly epilogue only)
    "loaded_split": _LOADED._replace(split=True),    # the reducer meets the full epilogue
}
SPLIT_ASKED = 3
C_OFF = 4                                            # default element offset of C: non-zero, 16-byte friendly


# ------------------------------------------------------------------------------------------------ shapes
# lda / ldb / ldc None: the default leading dimension (default_ld, Inputs.ldc); inst / epi: for the alignment cases the
# loader instance "(avec,bvec)" and the epilogue width the case was WRITTEN to select -- the host test checks that
# pick_vec / the vec4 rule agree, the GPU test asserts the instance by name
Shape = namedtuple("Shape", "M N K lda ldb a_off b_off ldc c_off inst epi")


def shape(M, N, K, lda=None, ldb=None, a_off=0, b_off=0, ldc=None, c_off=C_OFF, inst=None, epi=None):
    return Shape(M, N, K, lda, ldb, a_off, b_off, ldc, c_off, inst, epi)


ShapeFamily = namedtuple("ShapeFamily", "name prec a16 b16 km kn env base edges step corner cstep extra align refused probes")


def _up(x, q):
    return (x + q - 1) // q * q


def default_ld(fam, s, which):
    """Leading dimension of operand `which` ('a' / 'b') when the shape does not state one: K where k is contiguous
    (natural: K % 4 then decides the loader), else the contiguous extent rounded up to the operand's vector (4 floats,
    8 bf16) plus one vector -- wider than the rows, and friendly, so that the family's own kernel runs."""
    if which == "a":
        if not fam.km:
            return s.K
        return _up(s.M, 8) + 8 if fam.a16 else _up(s.M, 4) + 4
    if not fam.kn:
        return s.K
    return _up(s.N, 8) + 8 if fam.b16 else _up(s.N, 4) + 4


def lds(fam, s):
    return (s.lda if s.lda is not None else default_ld(fam, s, "a"), s.ldb if s.ldb is not None else default_ld(fam, s, "b"))


def _fam(name, base, edges, prec=0, a16=False, b16=False, km=False, kn=False, env=None, step=(1, 1, 1), corner=None,
         cstep=None, extra=(), align=(), refused=(), probes=("bare", "loaded", "split", "cwin", "c16")):
    edges = {k: tuple(v) for k, v in edges.items()}
    return ShapeFamily(name, prec, a16, b16, km, kn, dict(env or {}), tuple(base), edges, tuple(step), corner,
                       tuple(cstep or step), tuple(extra), tuple(align), tuple(refused), tuple(probes))


# ---- fp32 (gemm_impl.h: BM = 128, BK = 32; gemm_mk_nk.hip / gemm_mk_kn.hip / gemm_km_kn.hip: BN = 32 for N <= 32, 64 for
# N <= 64, else 128; gemm_km_kn.hip: the 64-row tile dispatch_m64 for M <= 64 with the (4,4) loaders and N > 32).
# M edges: the 64-row tile, BM, 2 BM.  N edges: the three BN (a tile edge and a dispatch threshold at once) and 4, the
# float4 epilogue's width.  K edges: 4 (the loaders' vector: pick_vec, gemm.hip), BK, 2 BK.
_F32_EDGES = {"M": (64, 128, 256), "N": (4, 32, 64, 128), "K": (4, 32, 64)}
_F32_BASE = (130, 132, 36)
_F32_EXTRA = ((1, 132, 36), (2, 132, 36), (130, 1, 36), (130, 36, 36), (130, 68, 36), (130, 260, 36), (130, 132, 1),
              (130, 132, 2), (130, 132, 34), (130, 132, 96), (130, 132, 100), (1, 1, 1), (1, 1, 3), (2, 3, 2))

# the alignment axis.  pick_vec (gemm.hip): the widest v in 4, 2, 1 with a (4 v)-byte aligned pointer, ld % v == 0 and --
# where k is the operand's contiguous index -- K % v == 0; dispatch (gemm_impl.h): (4,4) both 4; A_MK: (2,1) from
# avec >= 2, else (1,1); A_KM: (4,2) for avec == 4 and bvec >= 2, else (1,1).  vec4 rule (gemm_entry): N % 4 == 0, C
# 16-byte aligned, ldc % 4 == 0 (and the same of every epilogue operand: they are whole tensors with ld = N + 4 here).
# Offsets 0, 1, 2 elements and leading dimensions K, K+1, K+2, K+4, each instance on ragged M, N, K.
_ALIGN_MK = (
    shape(130, 132, 36, inst="(4,4)", epi="vec4"),
    shape(130, 132, 36, lda=40, ldb=40, inst="(4,4)", epi="vec4"),                       # ld = K + 4
    shape(130, 132, 36, ldc=137, inst="(4,4)", epi="scalar"),                             # ldc % 4 != 0
    shape(130, 132, 36, c_off=1, inst="(4,4)", epi="scalar"),
    shape(130, 132, 36, c_off=2, inst="(4,4)", epi="scalar"),
    shape(130, 130, 36, inst="(4,4)", epi="scalar"),                                      # N % 4 != 0
    shape(130, 132, 36, lda=38, inst="(2,1)", epi="vec4"),                                # lda = K + 2
    shape(130, 132, 36, a_off=2, ldb=38, inst="(2,1)", epi="vec4"),
    shape(130, 132, 38, ldb=39, b_off=1, c_off=2, inst="(2,1)", epi="scalar"),            # K % 4 = 2
    shape(129, 131, 34, lda=36, ldb=38, inst="(2,1)", epi="scalar"),
    shape(130, 132, 36, lda=37, inst="(1,1)", epi="vec4"),                                # lda = K + 1
    shape(130, 132, 36, a_off=1, inst="(1,1)", epi="vec4"),
    shape(130, 132, 36, a_off=1, b_off=1, lda=37, ldb=37, c_off=1, inst="(1,1)", epi="scalar"),
    shape(129, 131, 35, inst="(1,1)", epi="scalar"),                                      # K odd
    shape(127, 33, 33, lda=34, ldb=35, a_off=2, b_off=1, inst="(1,1)", epi="scalar"),
    shape(1, 1, 3, a_off=1, c_off=1, inst="(1,1)", epi="scalar"),
)
# B stored [k][n]: its vector runs along n, so ldb (default 136 for N = 132) and b_off decide, not K
_ALIGN_MK_KN = (
    shape(130, 132, 36, inst="(4,4)", epi="vec4"),
    shape(130, 132, 36, c_off=1, inst="(4,4)", epi="scalar"),
    shape(130, 132, 36, ldb=134, inst="(2,1)", epi="vec4"),                               # bvec = 2: not both 4
    shape(130, 132, 38, inst="(2,1)", epi="vec4"),                                        # avec = 2 (K % 4 = 2)
    shape(129, 131, 34, lda=36, b_off=2, c_off=2, inst="(2,1)", epi="scalar"),
    shape(130, 132, 36, lda=37, inst="(1,1)", epi="vec4"),
    shape(129, 131, 35, ldb=133, b_off=1, c_off=1, inst="(1,1)", epi="scalar"),
    shape(127, 33, 33, a_off=1, ldb=35, inst="(1,1)", epi="scalar"),
)
# A stored [k][m] and B stored [k][n]: lda (default 136 for M = 130) / ldb and the offsets decide; K is the row index
_ALIGN_KM_KN = (
    shape(130, 132, 36, inst="(4,4)", epi="vec4"),
    shape(130, 132, 35, c_off=2, inst="(4,4)", epi="scalar"),
    shape(130, 132, 36, ldb=134, inst="(4,2)", epi="vec4"),
    shape(130, 132, 33, b_off=2, inst="(4,2)", epi="vec4"),
    shape(129, 131, 35, ldb=134, b_off=2, c_off=1, inst="(4,2)", epi="scalar"),
    shape(61, 131, 35, ldb=134, inst="(4,2)", epi="scalar"),                              # M <= 64 but not (4,4): 128-row tile
    shape(130, 132, 36, lda=134, inst="(1,1)", epi="vec4"),                               # avec = 2: A_KM has no (2,x)
    shape(130, 132, 36, ldb=133, inst="(1,1)", epi="vec4"),                               # bvec = 1
    shape(129, 131, 35, lda=131, ldb=133, a_off=1, b_off=1, c_off=1, inst="(1,1)", epi="scalar"),
    shape(127, 33, 33, a_off=2, inst="(1,1)", epi="scalar"),
)

# ---- bf16 matrix cores.  Register-staged kernel (gemm_bf16_impl.h): BM = 256, BN = 128, BK = 64; bf16x3 / bf16x6
# (gemm_x3_impl.h, gemm_x3.hip): 256 x 128 x 32 / x 16.  LDS-DMA geometries (gemm_bf16_dma.hip): DBM x DBN x DBK = 256 x 256 x 64,
# D2M x D2N x D2K = 256 x 128 x 32, the 256- and 288-row rings at 32 deep; eight-phase kernel (gemm_bf16_p8.hip,
# gemm_bf16_p8_loop.h): 2 * TECM_P8_ROWS x 256 x 64.  M = 256 is the least the DMA kernels take, N = 32 / 33..127 / >= 128 and
# N % 256 in 1..128 route (tecm_gemm16_dma_try), K % 32 and K % 64 meet the 32- and 64-deep K-tiles, K = 32 (k32) and K < 128
# (tecm_gemm16_p8_try) route again.  A bf16 operand moves in vectors of 8 along its contiguous extent and a bf16-mode call
# needs K % 4 == 0: the neighbours of an edge are one such granule away.
_B16_EDGES = {"M": (256, 288, 512), "N": (64, 128, 256, 384), "K": (32, 64, 128, 192)}
_B16_BASE = (300, 264, 160)
_B16_EXTRA = ((1, 264, 160), (300, 264, 8), (300, 264, 96), (300, 32, 160), (300, 36, 160), (256, 128, 32), (256, 32, 32),
              (256, 128, 64))
_B16_REFUSED = (shape(300, 264, 100), shape(300, 264, 63))           # bf16 A / B: K % 8 != 0 (include/tecmollm.h)
_B16_PROBES = ("bare", "loaded", "split", "cwin", "c16")


def _b16(name, env, extra=(), edges=None, corner=(512, 256, 64)):
    # the corner sits at the end of the SECOND m-tile (M = 255 is below what the DMA kernels take: the M sweep asserts that
    # fallback) with K one whole 32-deep granule either side, so that all 27 shapes run the family's own kernel
    return _fam(name, _B16_BASE, edges or _B16_EDGES, prec=1, a16=True, b16=True, env=env, step=(1, 4, 8),
                corner=corner, cstep=(1, 4, 32), extra=_B16_EXTRA + tuple(extra), refused=_B16_REFUSED,
                probes=_B16_PROBES)


def _p8(rows):
    # two tiles of 2 * rows: the seam between the first and the second m-tile, and the end of the second; K >= 128
    e = dict(_B16_EDGES)
    e["M"] = tuple(sorted(set(_B16_EDGES["M"]) | {2 * rows, 4 * rows}))
    return _b16(f"bf16_p8_{rows}", {"TECM_BF16_P8": "1", "TECM_P8_ROWS": str(rows)}, edges=e, corner=(4 * rows, 256, 192))


# fp32 tensors on the bf16 cores: ops.uses_bf16 / uses_x3 send N < BF16_MIN_N = 64, K % 4 != 0 and unfriendly leading
# dimensions to the exact fp32 kernel instead -- the neighbours below 64 and off the granule assert that fallback by name
_F32OPS_EDGES = {"M": (256, 512), "N": (64, 128, 256), "K": (4, 64, 128, 192)}
_F32OPS_EXTRA = ((1, 260, 100), (300, 260, 63), (300, 260, 65), (300, 260, 31), (300, 132, 100), (300, 260, 8))
_X3_EDGES = {"M": (256, 512), "N": (64, 128, 256), "K": (4, 32, 64)}
_X6_EDGES = {"M": (256, 512), "N": (64, 128, 256), "K": (4, 16, 32)}

# operand-resident kernels (gemm_bf16_res_mk.hip, gemm_bf16_res_km.hip: the register-staged tile with ONE operand bf16 in
# HBM).  The bf16 operand's contiguous extent moves in granules of 8, the fp32 one's leading dimension in 4.
_RES_K = (64, 128)
_TN_GEO = ((192, 256), (128, 192), (64, 192), (256, 32), (32, 256))       # tn_geometry / tn_tile (gemm_bf16_tn.hip)

SHAPE_FAMILIES = [
    _fam("f32_mk_nk", _F32_BASE, _F32_EDGES, corner=(128, 128, 32), extra=_F32_EXTRA, align=_ALIGN_MK,
         probes=("bare", "loaded", "split", "cwin")),
    _fam("f32_mk_kn", _F32_BASE, _F32_EDGES, kn=True, corner=(128, 128, 32), extra=_F32_EXTRA, align=_ALIGN_MK_KN,
         probes=("bare", "loaded", "split", "cwin")),
    _fam("f32_km_kn", _F32_BASE, _F32_EDGES, km=True, kn=True, corner=(128, 128, 32), extra=_F32_EXTRA, align=_ALIGN_KM_KN,
         probes=("bare", "loaded", "split", "cwin")),
    # the 64-row tile (M <= 64): N and K swept below it, the corner at its own M edge and the BN = 64 edge
    _fam("f32_km_kn_m64", (62, 132, 36), {"M": (64,), "N": (32, 64, 128), "K": (32, 64)}, km=True, kn=True,
         corner=(64, 64, 32), extra=((1, 132, 36), (62, 260, 36), (62, 132, 1), (62, 132, 100), (33, 36, 3)),
         probes=("bare", "loaded", "split", "cwin")),
    _fam("bf16_reg_f32ops", (300, 260, 100), _F32OPS_EDGES, prec=1, step=(1, 1, 4), corner=(256, 128, 64),
         extra=_F32OPS_EXTRA),
    _fam("bf16_reg_op16", _B16_BASE, _B16_EDGES, prec=1, a16=True, b16=True, env={"TECM_BF16_DMA": "0"}, step=(1, 4, 8),
         corner=(256, 128, 64), extra=_B16_EXTRA, refused=_B16_REFUSED, probes=_B16_PROBES),
    _fam("bf16_res_a_mk_kn", (300, 260, 104), {"M": (256, 512), "N": (64, 128, 256), "K": _RES_K}, prec=1, a16=True, kn=True,
         step=(1, 1, 8), corner=(256, 128, 64), extra=((1, 260, 104), (300, 1, 104), (300, 260, 8)),
         refused=(shape(300, 260, 100), shape(300, 260, 104, ldb=262))),      # K % 8 != 0; fp32 B with ldb % 4 != 0
    _fam("bf16_res_a_km_kn", (296, 260, 100), {"M": (256, 512), "N": (64, 128, 256), "K": _RES_K}, prec=1, a16=True, km=True,
         kn=True, step=(8, 1, 1), corner=(256, 128, 64), extra=((8, 260, 100), (296, 1, 100), (296, 260, 1), (296, 260, 3)),
         refused=(shape(300, 260, 100), shape(296, 260, 100, lda=300))),      # M % 8 != 0; lda % 8 != 0
    _fam("bf16_res_b_km_kn", (300, 264, 100), {"M": (256, 512), "N": (64, 128, 256), "K": _RES_K}, prec=1, b16=True, km=True,
         kn=True, step=(1, 8, 1), corner=(256, 128, 64), extra=((1, 264, 100), (300, 8, 100), (300, 264, 1), (300, 264, 3)),
         refused=(shape(300, 260, 100), shape(300, 264, 100, lda=302))),      # N % 8 != 0; fp32 A with lda % 4 != 0
    _b16("bf16_dma1", {"TECM_BF16_DMA": "1"}),
    _b16("bf16_dma2", {"TECM_BF16_DMA": "2"}),
    _b16("bf16_dma5", {"TECM_BF16_DMA": "5"}),
    _b16("bf16_dma8", {"TECM_BF16_DMA": "8"}, corner=(576, 256, 64)),                                   # 2 x 288 rows
    _p8(128), _p8(112), _p8(96),
    # natural-orientation kernel: its five output shapes at K = 4096 (the bound), 4104, 4127; K = 4095 and an M no geometry
    # divides fall back to the register-transposing kernel.  It is a split-K kernel: no unsplit probe reaches it.
    _fam("bf16_tn", (192, 256, 4104), {}, prec=1, a16=True, b16=True, km=True, kn=True,
         extra=tuple((m, n, k) for m, n in _TN_GEO for k in (4096, 4104, 4127)) + ((192, 256, 4095), (64, 192, 4095),
                                                                                  (200, 256, 4104), (96, 192, 4104)),
         probes=("bare", "split", "loaded_split")),
    _fam("bf16x3", (300, 260, 100), _X3_EDGES, prec=2, step=(1, 1, 4), corner=(256, 128, 32), extra=_F32OPS_EXTRA,
         probes=("bare", "loaded", "split", "cwin")),
    _fam("bf16x6", (300, 260, 100), _X6_EDGES, prec=3, step=(1, 1, 4), corner=(256, 128, 16), extra=_F32OPS_EXTRA,
         probes=("bare", "loaded", "split", "cwin")),
    # no switch set: what tecm_gemm16_dma_try / tecm_gemm16_p8_try choose by themselves at every threshold -- M = 256, N = 32 |
    # 33..127 | >= 128, N % 256 in 1..128 (below and from N = 768), K = 32 | 64..127 | >= 128.  (The fp32 thresholds -- N <= 32,
    # <= 64, > 64, M <= 64 -- and the natural-orientation kernel's run without a switch in their own families above.)
    _fam("default_dispatch", _B16_BASE, {"M": (256,), "N": (128, 256, 384, 768), "K": (32, 64, 128)}, prec=1, a16=True,
         b16=True, step=(1, 4, 32), corner=(256, 384, 128), cstep=(1, 4, 32),
         extra=((300, 32, 160), (300, 36, 160), (300, 64, 160), (300, 32, 32), (300, 388, 160), (300, 640, 160),
                (300, 644, 160), (300, 264, 8), (300, 264, 40),
                (300, 256, 64), (300, 256, 96), (300, 512, 32)),         # wide n-tile below K = 128: the rings, DBM x DBN under c_win
         probes=_B16_PROBES),
]
SHAPE_FAMILY = {f.name: f for f in SHAPE_FAMILIES}


def shapes(fam):
    """The family's accepted-or-fallback shapes: sweeps, corner, alignment cases, extras (refused ones: fam.refused)."""
    out = []

    def add(s):
        if s not in out and min(s.M, s.N, s.K) > 0:
            out.append(s)

    bM, bN, bK = fam.base
    add(shape(bM, bN, bK))
    for axis, i in (("M", 0), ("N", 1), ("K", 2)):
        for e in fam.edges.get(axis, ()):
            for v in (e - fam.step[i], e, e + fam.step[i]):
                mnk = [bM, bN, bK]
                mnk[i] = v
                add(shape(*mnk))
    if fam.corner:
        cm, cn, ck = fam.corner
        for dm in (-1, 0, 1):
            for dn in (-1, 0, 1):
                for dk in (-1, 0, 1):
                    add(shape(cm + dm * fam.cstep[0], cn + dn * fam.cstep[1], ck + dk * fam.cstep[2]))
    for e in fam.extra:
        add(shape(*e))
    for s in fam.align:
        add(s)
    return out


# ------------------------------------------------------------------------------------------------ dispatch mirror
def pick_vec(off, ld, inner_is_k, K, cw=None):
    """pick_vec of gemm.hip for a tensor whose base is 16-byte aligned and `off` fp32 elements in."""
    v = 4
    while v > 1:
        if (4 * off) % (4 * v) == 0 and ld % v == 0 and (cw is None or cw % v == 0) and (not inner_is_k or K % v == 0):
            break
        v //= 2
    return v


def loader_instance(fam, s, a_cw=None):
    lda, ldb = lds(fam, s)
    avec = pick_vec(s.a_off, lda, not fam.km, s.K, a_cw)
    bvec = pick_vec(s.b_off, ldb, not fam.kn, s.K)
    if avec == 4 and bvec == 4:                              # dispatch (gemm_impl.h)
        return (4, 4)
    if not fam.km:
        return (2, 1) if avec >= 2 else (1, 1)
    return (4, 2) if avec == 4 and bvec >= 2 else (1, 1)


def f32_kernel(fam, s, a_cw=None):
    """gemm_{mk_nk,mk_kn,km_kn}.hip + dispatch / dispatch_m64 / launch of gemm_impl.h."""
    inst = loader_instance(fam, s, a_cw)
    bn = 32 if s.N <= 32 else 64 if s.N <= 64 else 128
    bmt = 64 if (fam.km and s.N > 32 and s.M <= 64 and inst == (4, 4)) else 128
    flags = ("true" if a_cw else "false") + ",false" if inst == (4, 4) else "true,true"
    return f"gemm_kernel<{int(fam.km)},{int(fam.kn)},{inst[0]},{inst[1]},{bn},{flags},{bmt}>"


def epilogue_vec4(fam, s, probe, ldc):
    """The vec4 rule of gemm_entry (gemm.hip) for this table's buffers: every epilogue operand but C is a whole tensor
    with ld = N + 4; C sits c_off elements (fp32 or bf16: 8-byte alignment serves a bf16 C) into its buffer."""
    c = PROBES[probe]
    return s.N % 4 == 0 and s.c_off % 4 == 0 and ldc % 4 == 0 and (not c.cwin or (s.N // T.TAPS) % 4 == 0)


def _p8_kernel(env, M, N, K):
    """tecm_gemm16_p8_try / tecm_p8_rows (gemm_bf16_p8.hip), on a 256-CU device; None: declined."""
    sel = env.get("TECM_BF16_P8")
    if sel == "0" or K < 128 or K % 32 or M < 256 or N < 128:
        return None
    nrem = N % 256
    if sel != "1" and 1 <= nrem <= 128 and N < 768:
        return None
    rows = env.get("TECM_P8_ROWS")
    if rows not in ("128", "112", "96"):
        tn = (N + 255) // 256

        def cost(wr):
            return ((((M + 2 * wr - 1) // (2 * wr)) * tn + 255) // 256) * wr
        rows = "112" if (tn <= 3 or M <= 32768) and cost(112) < cost(128) else "128"
    return f"gemm_bf16_p8_kernel<{rows}>"


def _op16_mk_nk_kernel(env, M, N, K, probe, vec4):
    """tecm_gemm16_dispatch_mk_nk (gemm_bf16_mk_nk.hip) -> tecm_gemm16_dma_try (gemm_bf16_dma.hip) for plain views."""
    c = PROBES[probe]
    reg = "gemm_bf16_kernel<0,0,false,false>"
    sel = env.get("TECM_BF16_DMA")
    k32, n_small = K < 64, N < 128
    if sel == "0" or not vec4 or c.split or K % 32 or K < 32 or M < 256 or N < 32 or (n_small and N > 32):
        return reg
    streams = int(c.res) + int(c.dact) + int(c.acc)
    fast = (streams == 0 and not c.rb and not c.pre and not c.c16) if c.cwin else (streams == 0 if c.rb else streams <= 1)
    if sel is None and fast:
        p8 = _p8_kernel(env, M, N, K)
        if p8:
            return p8
    nrem = N % 256
    if n_small or ((sel == "2") if (sel and not k32) else 1 <= nrem <= 128):
        return "gemm_bf16_dma2_kernel"
    can16 = not c.cwin and not c.rb and streams <= 1
    if k32 and not can16:
        return reg
    want16 = sel in ("5", "8") if (sel and not k32) else True
    if can16 and want16:
        tiles_n = (N + 255) // 256

        def cost(bm):
            return ((((M + bm - 1) // bm) * tiles_n + 255) // 256) * bm
        tall = True if sel == "8" else False if (sel == "5" or env.get("TECM_BF16_TALL") == "0") else cost(288) * 100 < cost(256) * 95
        return "gemm_bf16_dma5w_kernel" if tall else "gemm_bf16_dma5_kernel"
    return "gemm_bf16_dma_kernel"


def tn_geometry(M, N):
    """tn_geometry of gemm_bf16_tn.hip."""
    if M % 192 == 0 and N % 256 == 0:
        return 0
    if M % 128 == 0 and N % 192 == 0:
        return 1
    if M % 64 == 0 and N % 192 == 0:
        return 2
    if M % 256 == 0 and N % 32 == 0 and N < 64:
        return 3
    if M % 32 == 0 and M < 64 and N % 256 == 0:
        return 4
    return -1


def refusal(fam, s, probe="bare", a_cw=None):
    """Why tecm_gemm_bf16 refuses the shape (gemm_entry's io_bf16 checks; include/tecmollm.h), or None.  Calls with fp32
    tensors are never refused for their shape: ops.gemm runs the exact fp32 kernel where the bf16 ones do not serve."""
    lda, ldb = lds(fam, s)
    if fam.a16 and (s.a_off % 8 or lda % 8 or (s.M if fam.km else s.K) % 8 or (a_cw or 8) % 8):
        return "bf16 A needs a 16-byte friendly base, lda and contiguous extent"
    if fam.b16 and (s.b_off % 8 or ldb % 8 or (s.N if fam.kn else s.K) % 8):
        return "bf16 B needs a 16-byte friendly base, ldb and contiguous extent"
    if (fam.a16 or fam.b16) and not (fam.a16 and fam.b16):
        if (fam.a16 and pick_vec(s.b_off, ldb, not fam.kn, s.K) != 4) or (fam.b16 and pick_vec(s.a_off, lda, not fam.km, s.K) != 4):
            return "the fp32 operand of tecm_gemm_bf16 needs the float4 loader"
    return None


def fp32_fallback(fam, s, a_cw=None):
    """ops.gemm (uses_bf16 / uses_x3): fp32 tensors the bf16 kernels do not serve run on the exact fp32 kernel."""
    if fam.prec == 0 or fam.a16 or fam.b16:
        return fam.prec == 0
    lda, ldb = lds(fam, s)
    ok = s.N >= 64 and lda % 4 == 0 and ldb % 4 == 0 and (a_cw or 4) % 4 == 0 and (fam.km or s.K % 4 == 0)
    if fam.prec >= 2:
        ok = ok and s.K % 4 == 0 and not fam.km and not fam.kn and not a_cw
    return not (ok and s.a_off % 4 == 0 and s.b_off % 4 == 0)


def expected_kernel(fam, s, probe, ldc):
    """Name tecm_gemm_last_kernel must report for an accepted shape."""
    if fp32_fallback(fam, s):
        return f32_kernel(fam, s)
    if fam.prec == 2:
        return "gemm_x3_kernel<2,32>"
    if fam.prec == 3:
        return "gemm_x3_kernel<3,16>"
    lay = f"{int(fam.km)},{int(fam.kn)}"
    if not (fam.a16 or fam.b16):
        return f"gemm_bf16_kernel<{lay},false,false>"                # tecm_gemm16::dispatch (gemm_bf16_impl.h)
    if fam.km:                                                      # tecm_gemm16_dispatch_km_kn
        if fam.a16 and fam.b16 and PROBES[probe].split and s.K >= 4096 and tn_geometry(s.M, s.N) >= 0 \
                and fam.env.get("TECM_BF16_TN") != "0":
            return "gemm_bf16_tn_kernel"
        return "gemm_bf16_kernel<1,1,true,false>"                   # gemm_bf16_res_km.hip
    if fam.kn:
        return "gemm_bf16_kernel<0,1,true,false>"                   # gemm_bf16_res_mk.hip
    assert fam.a16 and fam.b16
    return _op16_mk_nk_kernel(fam.env, s.M, s.N, s.K, probe, epilogue_vec4(fam, s, probe, ldc))


def kernel_bk(name):
    """K-tile the launch's k_chunk is rounded to."""
    if name.startswith("gemm_kernel<") or name in ("gemm_x3_kernel<2,32>", "gemm_bf16_tn_kernel"):
        return 32
    return 16 if name == "gemm_x3_kernel<3,16>" else 64


def real_splits(K, asked, bk):
    """launch() of gemm_impl.h / gemm_bf16_impl.h / gemm_x3_impl.h, tn_launch: k_chunk is K / asked rounded up to whole
    K-tiles, and the grid gets only as many splits as still start inside K."""
    asked = max(asked, 1)
    k_chunk = _up((K + asked - 1) // asked, bk)
    return (K + k_chunk - 1) // k_chunk


def reducer(splits):
    """gemm_entry: which splitk_reduce_kernel instantiation finishes the call."""
    return None if splits <= 1 else 4 if splits <= 16 else 8 if splits <= 32 else 16


def probes_of(fam, s):
    """The probes a shape runs: the window scatter where N is even, a bf16 C where the contract allows one."""
    out = []
    for p in fam.probes:
        if p == "cwin" and s.N % T.TAPS:
            continue
        if p == "c16" and not (fam.prec == 1 and s.N % 4 == 0 and s.c_off % 4 == 0 and not fp32_fallback(fam, s)):
            continue
        out.append(p)
    return out


# ------------------------------------------------------------------------------------------------ inputs
class ShapeInputs(T.Inputs):
    """Inputs of one shape: the epilogue matrix's, with bounded-magnitude operands and C buffers of exactly the size the
    contract asks for (c_off + (rows - 1) ldc + width elements, NaN everywhere)."""

    def __init__(self, M, N, K, rounded, ldc=None):
        super().__init__(T._fam(f"{M}x{N}x{K}", M, N, K, prec=1 if rounded else 0))
        if ldc is not None:
            self.ldc = ldc
            self.drop_ld = ldc + 3
        del self.prev, self.prev_win, self.dact, self.dact16                 # no probe accumulates or takes a GELU' source

    @staticmethod
    def draw_operand(g, rows, K):
        mag = 0.75 + 0.5 * torch.rand(rows, K, generator=g)
        return torch.where(torch.rand(rows, K, generator=g) < 0.5, -mag, mag)

    def c_len(self, c):
        rows, width = (self.win_rows, self.Cw) if c.cwin else (self.fam.M, self.fam.N)
        return (rows - 1) * self.ldc_of(c) + width

    def prefill(self, c, c_off=0):
        buf = torch.full((c_off + self.c_len(c),), float("nan"))
        return buf.bfloat16() if c.c16 else buf


@functools.lru_cache(maxsize=None)
def inputs_of(M, N, K, rounded, ldc=None):
    """Drawn once per (shape, operand rounding) and shared by every family and test that uses the shape: read only."""
    return ShapeInputs(M, N, K, rounded, ldc)


def inputs_for(fam, s):
    return inputs_of(s.M, s.N, s.K, fam.prec == 1, s.ldc)


def check_shape(inp, c, got_c, got_pre, prefill, c_off):
    """check_case of the epilogue matrix on the buffer behind c_off, plus the c_off elements in front of it bit for bit."""
    fails, err = T.check_case(inp, c, got_c.detach().cpu()[c_off:], got_pre, prefill[c_off:])
    head = got_c.detach().cpu()[:c_off]
    bits = torch.int16 if head.dtype == torch.bfloat16 else torch.int32
    if not torch.equal(head.view(bits), prefill[:c_off].view(bits)):
        fails.append("wrote in front of c_off")
    return fails, err


def term_margin(inp, alpha=T.ALPHA):
    """Lower bound over all (i, j) of  min_k |alpha A_ik B_jk| / bar(i, j)  for the bare probe, bar(i, j) = RTOL |C_ij| +
    ATOL_RMS rms(C) as parity.elem_err sets it: how many element bars ONE k-term of ONE element is worth at least.  (The
    zeros a window view reads where a time step does not exist are no terms.)"""
    Cm = alpha * inp.P
    bar = RTOL * Cm.abs() + ATOL_RMS * float(Cm.pow(2).mean().sqrt())
    Aabs = inp.A.double().abs()
    Aabs = torch.where(Aabs == 0, torch.full_like(Aabs, float("inf")), Aabs)
    low = alpha * Aabs.min(dim=1).values[:, None] * inp.B.double().abs().min(dim=1).values[None, :]
    return float((low / bar).min())


# ------------------------------------------------------------------------------------------------ split-K sweep
# launch(): real splits = ceil(K / k_chunk), k_chunk = ceil(ceil(K / asked) / BK) BK.  K = splits * BK makes the count real;
# K - d leaves the last split one short K-tile; K + d (and an asked count of 2 splits + 1 at K = splits * BK) ask for more
# splits than get launched.  d: the family's K granule.  Counts 2..16 end in splitk_reduce_kernel<4>, 17..32 in <8>, 33.. in <16>.
SPLIT_COUNTS = (2, 3, 4, 5, 16, 17, 32, 33, 64)
SPLIT_MN = (130, 68)
SPLIT_FAMILIES = {"f32_mk_nk": (1, 32), "bf16_reg_f32ops": (4, 64), "bf16_reg_op16": (8, 64)}      # family -> (d, BK)
SPLIT_PROBES = ("split", "loaded_split")
SplitCase = namedtuple("SplitCase", "K asked real")


def split_cases(name):
    d, bk = SPLIT_FAMILIES[name]
    out = []
    for n in SPLIT_COUNTS:
        for asked, K in ((n, n * bk - d), (n, n * bk), (n, n * bk + d), (2 * n + 1, n * bk)):
            out.append(SplitCase(K, asked, real_splits(K, asked, bk)))
    return out


def split_shape(sc):
    return shape(SPLIT_MN[0], SPLIT_MN[1], sc.K)


# ------------------------------------------------------------------------------------------------ window view of A
# Conv1d-shaped views (include/tecmollm.h: TecmWin): x is (B, Lin, nodes, Cw) time-major, row m = (b Lout + t_out) nodes + node
# of the view holds x[b, t_out stride + tap - pad, node, :] for every tap, zeros where that time step does not exist.
WinCase = namedtuple("WinCase", "B Lout nodes taps stride Cw")
WIN_N = 68
WIN_FAMILIES = ("f32_mk_nk", "bf16_reg_f32ops", "bf16_res_a_mk_nk")
_WIN_M = ((1, 127, 1), (2, 16, 4), (1, 43, 3), (3, 17, 5), (2, 32, 4), (1, 257, 1))      # M = 127, 128, 129, 255, 256, 257
WIN_CASES = [WinCase(1, 43, 3, taps, stride, cw) for taps in (3, 7) for stride in (1, 2) for cw in (4, 6, 7, 24)] + \
            [WinCase(b, l, n, taps, stride, cw) for (b, l, n) in _WIN_M if (b, l, n) != (1, 43, 3)
             for taps, stride, cw in ((3, 2, 24), (7, 1, 4))]
# the resident-A kernel of gemm_bf16_res_mk.hip behind a window: bf16 A, fp32 B [n][k]
WIN_RES_A = _fam("bf16_res_a_mk_nk", (129, WIN_N, 72), {}, prec=1, a16=True)


def win_geometry(w):
    pad = (w.taps - 1) // 2
    Lin = w.Lout if w.stride == 1 else 2 * w.Lout                # Conv1d: Lout = (Lin + 2 pad - taps) // stride + 1
    assert (Lin + 2 * pad - w.taps) // w.stride + 1 == w.Lout
    return (w.nodes, Lin, w.Lout, w.stride, w.taps, w.Cw, pad)    # the arguments of ops.win


class WinInputs(ShapeInputs):
    """A window case: x and the Conv1d weight drawn bounded like A and B, A = the view of x written out row by row, B = the
    weight as [n][tap Cw + c], P = torch's conv1d in fp64."""

    def __init__(self, w, rounded):
        M, K = w.B * w.Lout * w.nodes, w.taps * w.Cw
        super().__init__(M, WIN_N, K, rounded)
        nodes, Lin, Lout, stride, taps, Cw, pad = win_geometry(w)
        g = torch.Generator().manual_seed(977 + 31 * M + K + (1000 if rounded else 0))
        s = float(K) ** -0.25
        x = self.draw_operand(g, w.B * Lin * nodes, Cw) * s
        wt = self.draw_operand(g, WIN_N * Cw, taps).view(WIN_N, Cw, taps) * s
        if rounded:
            x, wt = R.round_bf16(x), R.round_bf16(wt)
        self.x = x                                                 # the source tensor, rows (b, t_in, node)
        self.B = wt.permute(0, 2, 1).reshape(WIN_N, K).contiguous()
        x4 = x.view(w.B, Lin, nodes, Cw)
        A = torch.zeros(w.B, Lout, nodes, taps, Cw)
        for t in range(Lout):
            for tap in range(taps):
                t_in = t * stride + tap - pad
                if 0 <= t_in < Lin:
                    A[:, t, :, tap] = x4[:, t_in]
        self.A = A.view(M, K)
        conv = torch.nn.functional.conv1d(x4.permute(0, 2, 3, 1).reshape(w.B * nodes, Cw, Lin).double(), wt.double(),
                                          stride=stride, padding=pad)
        self.P = conv.view(w.B, nodes, WIN_N, Lout).permute(0, 3, 1, 2).reshape(M, WIN_N).contiguous()


@functools.lru_cache(maxsize=None)
def win_inputs(w, rounded):
    return WinInputs(w, rounded)


def win_family(name):
    return WIN_RES_A if name == "bf16_res_a_mk_nk" else SHAPE_FAMILY[name]


def win_expected(name, w):
    """Kernel name of a window case, or None where tecm_gemm_bf16 refuses it (a bf16 A needs Cw % 8 == 0)."""
    fam = win_family(name)
    s = shape(w.B * w.Lout * w.nodes, WIN_N, w.taps * w.Cw, lda=w.Cw)
    if refusal(fam, s, a_cw=w.Cw):
        return None
    if fp32_fallback(fam, s, a_cw=w.Cw):
        return f32_kernel(fam, s, a_cw=w.Cw)
    return "gemm_bf16_kernel<0,0,true,false>"         # tecm_gemm16::dispatch with win / tecm_gemm16_res_a_mk_nk
