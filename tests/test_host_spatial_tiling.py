"""CPU tests of tests/spatial_tiling_cases.py: every case gets the tiling and the entry points the table names, asked of
graph.build and of the library's own predicates; the table covers every rung of graph.TILE_SIZES, both formulations and the
boundaries its comments claim; the per-tile lists graph.build hands to the kernels equal a plain-Python brute force; and the
oracle the GPU tests compare with agrees with itself in float64 to a tenth of their bar on every tensor of every case."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import spatial_tiling_cases as sc
from tests.input_grad_cases import brute_by_source
from tests.parity import ATOL_RMS, RTOL, elem_err, rel_err

ALL = [(c, cin) for case in sc.CASES for c, cin in sc.variants(case)]
IDS = [f"{c.name}_cin{cin}" for c, cin in ALL]


def _tiling(m):
    return (m.tile_nodes, m.num_tiles, m.win_max, m.tile_edges_max)


def _lds(m, cin):
    from tecmollm import graph as G
    return (G.lds_bytes_fwd(m.win_max, m.tile_nodes, m.tile_edges_max),
            G.lds_bytes_bwd(m.win_max, m.tile_nodes, 22 - cin, m.tile_edges_max))


@pytest.mark.parametrize("c,cin", ALL, ids=IDS)
def test_every_case_gets_the_tiling_and_the_route_the_table_names(c, cin):
    m = sc.meta_of(c, cin)
    assert _tiling(m) == c.tiling and m.num_nodes == c.N
    assert sc.routes(c, m, cin) == (c.fwd, c.bwd)
    fwd, bwd = _lds(m, cin)
    assert 0 < fwd <= sc.LDS_BUDGET and 0 < bwd <= sc.LDS_BUDGET
    # the predicates' own terms: the second formulation serves windows of at most 256 rows, its backward a map within 80 KiB
    assert (c.fwd == sc.FWD2) == (m.win_max <= 256)
    assert c.bwd != sc.BWD2 or c.fwd == sc.FWD2
    d = sc.descriptor(c, m, cin)
    total = c.B * c.L * m.num_tiles
    want = min(total, 256) if total <= 256 * sc.MAXI else (total + sc.MAXI - 1) // sc.MAXI
    assert sc._h().tecm_spatial_bwd_blocks(C.byref(d)) == want


def test_the_table_covers_every_tile_size_the_builder_can_return():
    """Every rung of graph.TILE_SIZES is some case's tile size: none is unreachable, so none needs a justification."""
    from tecmollm import graph as G
    assert G.TILE_SIZES == (128, 120, 112, 110, 104, 96, 80, 64, 48, 32, 16, 8, 4, 2, 1)
    assert {c.tiling[0] for c in sc.CASES} == set(G.TILE_SIZES)
    assert len({c.name for c in sc.CASES}) == len(sc.CASES)
    assert {c.cin for c in sc.CASES} == {6, 10} and abs(sum(c.cin == 6 for c in sc.CASES) * 2 - len(sc.CASES)) <= 2


def test_the_table_covers_the_regimes_it_states():
    """The table against its own comments, judged by the library: a change to the ladder, an LDS map or a predicate that moves
    a case out of its regime fails here, not silently in the coverage of the GPU tests."""
    from tecmollm import graph as G
    metas = {c.name: sc.meta_of(c) for c in sc.CASES}
    wins = {c.name: metas[c.name].win_max for c in sc.CASES}
    # both sides of the 256-row line for the sizes both formulations serve
    for tn in (128, 120, 112, 104, 96):
        sides = {wins[c.name] <= 256 for c in sc.CASES if c.tiling[0] == tn and c.gen == "band"}
        assert sides == {True, False}, tn
    assert 256 in wins.values() and 257 in wins.values()
    c257 = sc.BY_NAME["t128_w257"]
    assert c257.tiling[0] == 128 and (c257.fwd, c257.bwd) == (sc.FWD1, sc.BWD1)
    hi_lo = (metas["t128_w257"].tile_hi - metas["t128_w257"].tile_lo).tolist()
    assert hi_lo == [192, 256, 256, 256, 257]                # one tile needs the second by-source round, for one row
    # the forward's LDS equal to the budget, to the byte
    b = sc.BY_NAME["t112_w323_budget"]
    assert G.lds_bytes_fwd(*[b.tiling[i] for i in (2, 0, 3)]) == sc.LDS_BUDGET
    # the widest window the builder admits (the next graph is refused: test below), at Cin = 10 and at Cin = 6: 3880 of the
    # 4096 floats the forward's x prefetch (8 float2 x 256 threads per slot) holds
    widest = max(wins.values())
    assert widest == 388 and all(c.cin == 10 for c in sc.CASES if wins[c.name] == widest and c.B * c.L == 1)
    assert any(wins[c.name] == widest and c.cin == 10 for c in sc.CASES) and widest * 10 <= 8 * 2 * 256
    assert any(wins[c.name] == widest and c.cin == 6 for c in sc.CASES)
    # the dense cases: either side of the second backward's 80 KiB line while the second forward serves, and the first
    # backward within 5 % of its 160 KiB
    under, over, full = (sc.BY_NAME[n] for n in ("dense_under_bwd2", "dense_over_bwd2", "dense_bwd_lds"))
    assert (under.fwd, under.bwd) == (sc.FWD2, sc.BWD2) and (over.fwd, over.bwd) == (sc.FWD2, sc.BWD1)
    assert under.tiling[0] == over.tiling[0] and 0 < over.tiling[3] - under.tiling[3] < 0.08 * under.tiling[3]
    assert (full.fwd, full.bwd) == (sc.FWD2, sc.BWD1)
    assert 0.95 * sc.LDS_BUDGET < _lds(metas[full.name], full.cin)[1] <= sc.LDS_BUDGET
    # the small tiles: more items than blocks, so a block of the first backward owns several and switches tile inside
    for tn in (1, 2, 4, 8):
        assert any(c.tiling[0] == tn and c.B * c.L * c.tiling[1] > 256 for c in sc.CASES), tn
    # an odd graph count on a multi-tile case of each formulation; both launchers at MAXI items per block
    for fwd in (sc.FWD2, sc.FWD1):
        assert any(c.fwd == fwd and (c.B, c.L) == (1, 3) and c.tiling[1] > 1 for c in sc.CASES)
    assert any(c.B * c.L * c.tiling[1] > 256 * sc.MAXI for c in sc.CASES)
    # a last tile shorter than the others under both formulations, and a last tile of one node
    last = {c.name: c.N - (c.tiling[1] - 1) * c.tiling[0] for c in sc.CASES}
    for fwd in (sc.FWD2, sc.FWD1):
        assert any(c.fwd == fwd and 1 < last[c.name] < c.tiling[0] for c in sc.CASES)
    assert any(last[c.name] == 1 and c.tiling[0] > 1 for c in sc.CASES)
    # the full cross of Cin x mode x train on one case per pair of kernels
    assert {(c.fwd, c.bwd) for c in sc.CASES if c.cross} == {(sc.FWD2, sc.BWD2), (sc.FWD1, sc.BWD1)}
    # kernels by name: all five serve some case
    served = {k for c in sc.CASES for v2 in (True, False) for k in sc.kernels(c, v2)}
    assert served == {"spatial_fwd", "spatial_fwd2", "spatial_bwd<1>", "spatial_bwd<2>", "spatial_bwd2"}


def test_the_first_graph_past_the_limit_is_refused():
    """Band (194, 194): even one-node tiles need 389 rows, more than the forward's two slots hold; build raises, it does not
    hand out a tiling no launcher takes."""
    from tecmollm import graph as G
    gen, lo, hi, N = sc.REFUSED
    assert gen == "band"
    assert G.lds_bytes_fwd(388, 1, 6) <= sc.LDS_BUDGET < G.lds_bytes_fwd(389, 1, 6)
    with pytest.raises(ValueError, match="bandwidth too large"):
        G.build(sc.banded(N, lo, hi), N, torch.device("cpu"))


@pytest.mark.parametrize("c", sc.CASES, ids=[c.name for c in sc.CASES])
def test_graph_lists_equal_a_brute_force(c):
    """tile_lo / tile_hi, the per-tile by-source lists (src_ptr, src_col, src_ptr_off) and the whole-graph by-source CSR
    (out_ptr, out_target, out_slot) against plain Python working from the edge list alone."""
    m = sc.meta_of(c)
    ei = sc.edges(c).numpy()
    tiles = sc.brute_tiles(ei, c.N, m.tile_nodes)
    assert len(tiles) == m.num_tiles
    assert m.tile_lo.tolist() == [t[0] for t in tiles] and m.tile_hi.tolist() == [t[1] for t in tiles]
    assert max(t[1] - t[0] for t in tiles) == m.win_max and max(len(t[2]) for t in tiles) == m.tile_edges_max
    rowptr, colidx = m.rowptr.numpy(), m.colidx.numpy()
    src_ptr, src_col, off = m.src_ptr.numpy(), m.src_col.numpy(), m.src_ptr_off.tolist()
    pos = 0
    for k, (lo, hi, seg) in enumerate(tiles):
        n0 = k * m.tile_nodes
        e0 = int(rowptr[n0])
        assert colidx[e0:e0 + len(seg)].tolist() == [j for _, j in seg]
        ptr, codes = sc.brute_by_source_tile(lo, hi, n0, seg)
        assert off[k] == pos
        assert src_ptr[pos:pos + hi - lo + 1].tolist() == ptr
        assert src_col[e0:e0 + len(seg)].tolist() == codes
        pos += hi - lo + 1
    assert pos == src_ptr.size
    ptr, tgt, slot = brute_by_source(ei, c.N)
    assert np.array_equal(m.out_ptr.numpy(), ptr) and np.array_equal(m.out_target.numpy(), tgt)
    assert np.array_equal(m.out_slot.numpy(), slot)


@pytest.mark.parametrize("c,cin", ALL, ids=IDS)
def test_the_oracle_in_float32_and_in_float64_agree_to_a_tenth_of_the_bar(c, cin):
    """No case sits on a LeakyReLU kink or a cancellation that the float32 oracle itself resolves badly: forward, d x and all
    eleven parameter gradients of the float32 oracle are within RTOL / 10 (max norm) and a tenth of the element-wise bar of
    the same oracle run on float64 copies of inputs and parameters -- both graph modes, eval and the mirrored dropout."""
    for mode in sc.MODES:
        for train in (False, True):
            r32 = sc.oracle(c, cin, mode, train)
            r64 = sc.oracle(c, cin, mode, train, torch.float64)
            assert r32["out"].dtype == torch.float32 and r64["out"].dtype == torch.float64
            for k, want in r64.items():
                r, e = rel_err(r32[k], want), elem_err(r32[k], want, RTOL, ATOL_RMS)
                assert r < RTOL / 10 and e < 0.1, (mode, train, k, r, e)
            sc._oracle_cache.pop((c.name, cin, mode, train, torch.float64))
