"""Host side of TecmGemm's two hints (include/tecmollm.h): the scalar row test the fp32 GEMM applies per block tile
(csrc/gemm_tile_map.h, compiled for the host as tecm_gemm_rows_in_rect) and the tile count built on it, against brute force
over every row; the binding's view of the descriptor; the attention query.  No GPU."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


@pytest.fixture(scope="module")
def lib():
    from tecmollm import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


# (M, nodes, T): rows are (b T + t) nodes + n, the rectangle is the token-0 run of every sequence.  M % 128 != 0 in most, T = 1
# makes every row a token-0 row, nodes = 128 / 256 put every run on tile edges, nodes < tile leaves no tile inside.
SHAPES = [(1800, 300, 3), (1800, 300, 6), (69864, 2911, 3), (2 * 3 * 128, 128, 3), (4 * 256, 256, 1), (777, 37, 3),
          (1000, 1000, 1), (5 * 2 * 129, 129, 2), (640, 64, 5), (513, 171, 3)]
TILES = (128, 64, 32)
ROWS_OF = (lambda n: n, lambda n: n - 1, lambda n: 100)


@pytest.mark.parametrize("M,nodes,T", SHAPES)
def test_row_test_and_tile_count_against_brute_force(lib, M, nodes, T):
    period = T * nodes
    r = np.arange(M)
    for bm, rows_of in itertools.product(TILES, ROWS_OF):
        rows = rows_of(nodes)
        inside = (r % period) < rows
        want = [bool(inside[m0:m0 + bm].all()) for m0 in range(0, M, bm)]
        got = [bool(lib.tecm_gemm_rows_in_rect(m0, min(m0 + bm, M), period, rows)) for m0 in range(0, M, bm)]
        assert got == want, (bm, rows)
        for N, bn, cols in ((768, 128, 256), (768, 128, 200), (800, 128, 800), (32, 32, 32), (100, 64, 100)):
            col_tiles = sum(min(n0 + bn, N) <= cols for n0 in range(0, N, bn))
            assert lib.tecm_gemm_rect_tiles(M, N, bm, bn, period, rows, cols) == sum(want) * col_tiles, (bm, rows, N, bn, cols)


def test_the_benchmark_shape_skips_a_tenth_of_c_attn(lib):
    """B = 8, T = 3, N = 2911: 8 runs of 2911 rows hold 21 or 22 whole 128-row tiles each; six of the 18 column tiles are q."""
    M, nodes, T = 8 * 3 * 2911, 2911, 3
    dead = lib.tecm_gemm_rect_tiles(M, 2304, 128, 128, T * nodes, nodes, 768)
    total = -(-M // 128) * 18
    assert dead % 6 == 0 and 8 * 21 <= dead // 6 <= 8 * 22
    assert 0.10 < dead / total < 0.11


def test_degenerate_arguments_count_nothing(lib):
    assert lib.tecm_gemm_rect_tiles(1800, 768, 128, 128, 0, 300, 256) == 0
    assert lib.tecm_gemm_rect_tiles(1800, 768, 128, 128, 900, 0, 256) == 0
    assert lib.tecm_gemm_rect_tiles(1800, 768, 128, 128, 900, 300, 0) == 0
    assert lib.tecm_gemm_rows_in_rect(0, 128, 0, 300) == 0 and lib.tecm_gemm_rows_in_rect(128, 128, 900, 300) == 0
    assert lib.tecm_gemm_rows_in_rect(0, 128, 900, 900) == 1 and lib.tecm_gemm_rows_in_rect(0, 5000, 900, 1000) == 1


def test_binding_carries_the_hints_at_the_end_of_the_descriptor(lib):
    from tecmollm import _lib
    header = open(os.path.join(ROOT, "include", "tecmollm.h")).read()
    body = re.search(r"typedef struct TecmGemm \{(.*?)\} TecmGemm;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    tail = [f[0] for f in _lib.TecmGemm._fields_][-6:]
    assert tail == ["dead_period", "dead_rows", "dead_cols", "zero_period", "zero_rows", "zero_k"]
    assert re.findall(r"\b(dead_\w+|zero_\w+)\b", body) == tail
    assert body.rstrip().endswith("int32_t zero_period, zero_rows, zero_k;")
    assert ctypes.sizeof(_lib.TecmGemm) % 8 == 0
    assert _lib.TecmGemm.zero_k.offset + 4 == ctypes.sizeof(_lib.TecmGemm)
    g = _lib.TecmGemm()
    assert (g.dead_period, g.dead_rows, g.dead_cols, g.zero_period, g.zero_rows, g.zero_k) == (0,) * 6    # default: no hint


def test_attention_query_names_the_compile_time_instances(lib):
    assert [t for t in range(1, 33) if not lib.tecm_attention_reads_q0(t)] == [1, 2, 3, 4, 6, 8, 12]
    assert lib.tecm_attention_reads_q0(33) == 1 and lib.tecm_attention_reads_q0(1024) == 1


def test_switch_and_precision_gate_the_call_sites(lib, monkeypatch):
    from tecmollm import functions as F_, ops
    monkeypatch.delenv("TECM_CAUSAL_Q0", raising=False)
    assert F_._causal_q0(3, ops.PREC_FP32) and F_._causal_q0(6, False)
    assert not F_._causal_q0(21, ops.PREC_FP32) and not F_._causal_q0(3, ops.PREC_BF16) and not F_._causal_q0(3, ops.PREC_BF16X3)
    monkeypatch.setenv("TECM_CAUSAL_Q0", "0")
    assert not F_._causal_q0(3, ops.PREC_FP32)
