"""CPU tests of the host side of the temporal attention maps: the float64 restatement of the trunk
(tests/temporal_attention_ref.py) against the frozen oracle, `derive` on a two-token case worked out by hand, the uniform
constants, empty groups, the C ABI entries and what the host refuses, and the files `write_temporal_attention` writes.  No GPU."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests import temporal_attention_ref as TA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_reproduces_the_oracle_trunk():
    """`gpt2_lora_attentions` returns oracle.ref_cpu.gpt2_lora's last_hidden_state (float64 on both sides) to rounding, and its
    attentions are causal distributions."""
    cfg = R.default_config(L_in=96, L_out=12, num_nodes=5, llm_layers=2)
    p = {k: v.double() for k, v in R.init_params(cfg, seed=3).items()}
    for name in p:                                        # LoRA-B starts at zero: give the branch something to do
        if "lora_B" in name:
            p[name] = 0.05 * torch.randn(p[name].shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    S, T = 4, 6
    h = torch.randn(S, T, 768, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    want = R.gpt2_lora(h, p, 2)
    got, atts = TA.gpt2_lora_attentions(h, p, 2)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-12, atol=1e-12)
    assert len(atts) == 2
    for w in atts:
        w = w.numpy()
        assert w.shape == (S, 12, T, T) and (np.triu(w, 1) == 0).all() and (w[:, :, 0, 0] == 1).all()
        np.testing.assert_allclose(w.sum(-1), 1.0, rtol=0, atol=1e-14)


def test_causal_probs_ignores_q0_and_matches_torch_softmax():
    B, T, N = 2, 5, 3
    qkv = np.random.default_rng(0).standard_normal((B * T * N, 3 * 768))
    a = TA.causal_probs(qkv, B, T, N)
    poisoned = qkv.reshape(B, T, N, 3 * 768).copy()
    poisoned[:, 0, :, :768] = np.nan
    assert np.array_equal(TA.causal_probs(poisoned.reshape(B * T * N, -1), B, T, N), a)
    t = torch.from_numpy(qkv).view(B, T, N, 3, 12, 64)
    q, k = t[:, :, :, 0].permute(0, 2, 3, 1, 4), t[:, :, :, 1].permute(0, 2, 3, 1, 4)
    s = (q @ k.transpose(-1, -2) / 8).masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool)), float("-inf"))
    np.testing.assert_allclose(a, s.softmax(-1).numpy(), rtol=1e-13, atol=1e-16)


def _two_token_case(a=0.25, windows=2):
    """T = 2, N = 1, 12 heads, `windows` identical windows: p = [[1, 0], [a, 1 - a]]."""
    p = np.zeros((windows, 1, 12, 2, 2), np.float32)
    p[..., 0, 0] = 1.0
    p[..., 1, 0] = a
    p[..., 1, 1] = 1.0 - a
    return p


def test_derive_on_the_two_token_case_by_hand():
    from tecmollm.temporal_attention import derive, uniform_constants
    a = 0.25
    node, lag, mat, counts = TA.accumulate_ref(_two_token_case(a), None, 1)
    got = derive(node[:, None], lag[:, None], counts, mat[:, None])
    assert got["count"].tolist() == [2.0]
    ent = 0.5 * (-a * math.log(a) - (1 - a) * math.log(1 - a))
    np.testing.assert_allclose(got["entropy"], np.full((1, 1, 1, 12), ent), rtol=1e-15)
    np.testing.assert_allclose(got["lookback"], 0.5 * a, rtol=1e-15)
    np.testing.assert_allclose(got["sink_weight"], 0.5 * (1 + a), rtol=1e-15)
    np.testing.assert_allclose(got["self_weight"], 0.5 * (1 + 1 - a), rtol=1e-15)
    np.testing.assert_allclose(got["effective_tokens"], math.exp(ent), rtol=1e-15)
    #   lag 0 has two rows (1 and 1 - a), lag 1 one row (a): the profile is their mean
    np.testing.assert_allclose(got["lag_profile"][0, 0, :, 0], 0.5 * (2 - a), rtol=1e-15)
    np.testing.assert_allclose(got["lag_profile"][0, 0, :, 1], a, rtol=1e-15)
    np.testing.assert_allclose(got["mean"][0, 0, 3], [[1.0, 0.0], [a, 1 - a]], rtol=1e-15)
    #   uniform causal attention at T = 2: rows [1], [1/2, 1/2]
    assert got["entropy_uniform"] == 0.5 * math.log(2.0) and got["lookback_uniform"] == 0.25
    np.testing.assert_allclose(got["lookback_gap"], 0.5 * a - 0.25, rtol=1e-15)
    u = uniform_constants(4)
    assert u["entropy_uniform"] == (math.log(1.0) + math.log(2.0) + math.log(3.0) + math.log(4.0)) / 4
    assert u["lookback_uniform"] == (0 + 0.5 + 1.0 + 1.5) / 4
    # uniform rows reproduce the constants through the loops
    T = 4
    pu = np.tril(np.ones((T, T))) / np.arange(1, T + 1).reshape(T, 1)
    s = TA.sequence_stats(pu)
    np.testing.assert_allclose(s[:2], [u["entropy_uniform"], u["lookback_uniform"]], rtol=1e-15)


def test_fast_accumulation_is_the_loops():
    rng = np.random.default_rng(2)
    p = np.tril(rng.random((3, 2, 12, 5, 5))).astype(np.float32)
    want = TA.accumulate_ref(p, [1, 3, 1], 3)
    got = TA.accumulate_fast(p, [1, 3, 1], 3)
    for w, g in zip(want[:3], got[:3]):
        np.testing.assert_allclose(g, w, rtol=1e-14, atol=0)
    assert got[3].tolist() == want[3].tolist() == [0, 2, 0]


def test_a_group_without_windows_reads_nan():
    from tecmollm.temporal_attention import derive
    node, lag, mat, counts = TA.accumulate_ref(_two_token_case(windows=1), [2], 3)
    got = derive(node[:, None], lag[:, None], counts, mat[:, None])
    assert got["count"].tolist() == [0.0, 0.0, 1.0]
    for k in ("entropy", "lookback", "sink_weight", "self_weight", "effective_tokens", "lag_profile", "mean", "lookback_gap"):
        assert np.isnan(got[k][:2]).all() and np.isfinite(got[k][2]).all(), k


def _desc(**kw):
    from tecmollm import _lib
    d = _lib.TecmTemporalAttn(B=2, T=6, N=5, heads=12, D=768, num_groups=1, num_layers=1)
    for f in ("qkv", "probs"):
        setattr(d, f, 64)                                 # never dereferenced on the host
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_abi_declares_binds_and_exports_the_two_entries():
    from tecmollm import _lib, ops
    import tecmollm
    header = open(os.path.join(ROOT, "include", "tecmollm.h")).read()
    assert "int64_t tecm_temporal_attention_ws_floats(const TecmTemporalAttn* a);" in header
    assert "int tecm_temporal_attention(const TecmTemporalAttn* a, void* stream);" in header
    assert "#define TECM_TATT_COUNT 8" in header and _lib.TECM_TATT_COUNT == 8
    assert "modeling_gpt2.py:144-226" in header and "modules.py:205-209" in header
    assert int(re.search(r"#define\s+TECM_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION == 21
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tecm_temporal_attention_ws_floats", "tecm_temporal_attention"):
        assert name in _lib.EXPORTS and hasattr(handle, name)
    body = re.search(r"typedef struct TecmTemporalAttn \{(.*?)\} TecmTemporalAttn;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.TecmTemporalAttn._fields_]
    assert ctypes.sizeof(_lib.TecmTemporalAttn) == 11 * 8 + 10 * 4
    assert _lib.lib().tecm_abi_version() == 21
    for name in ("temporal_attention", "TemporalAttentionStats", "evaluate_temporal_attention", "write_temporal_attention"):
        assert callable(getattr(tecmollm, name)) and name in tecmollm.__all__
    # pure host arithmetic: per window 4 doubles per (node, head) and, per block of 16 (T <= 32) or 4 nodes and head, T (+ T*T)
    N, H = 2911, 12
    for T, ipb in ((3, 16), (6, 16), (21, 16), (32, 16), (33, 4), (90, 4), (1024, 4)):
        nb = (N + ipb - 1) // ipb
        for B in (1, 2, 16):
            for matrix in (False, True) if T <= 32 else (False,):
                per = 2 * (4 * N * H + nb * H * T * (T + 1 if matrix else 1))
                chunk = max(1, min(B, (64 << 20) // (4 * per)))
                got = ops.temporal_attention_ws_floats(B, T, N, H, 768, True, matrix)
                assert got == chunk * per > 0, (T, B, matrix)
                assert got * 4 <= (64 << 20) or chunk == 1
        assert ops.temporal_attention_ws_floats(2, T, N, H, 768, False) == 4          # the export alone needs no workspace


def test_the_host_refuses_what_it_does_not_serve():
    from tecmollm import _lib
    L = _lib.lib()
    ok = _desc()
    assert L.tecm_temporal_attention_ws_floats(ctypes.byref(ok)) > 0
    bad = {"T = 0": _desc(T=0), "T = 1025": _desc(T=1025), "head dim 32": _desc(D=384), "head dim 128": _desc(heads=6),
           "matrix_stats at T = 33": _desc(T=33, node_stats=64, lag_stats=64, counts=64, err_flag=64, matrix_stats=64),
           "both outputs NULL": _desc(probs=None), "no nodes": _desc(N=0), "empty node list": _desc(nodes=64, Ns=0)}
    for what, d in bad.items():
        assert L.tecm_temporal_attention_ws_floats(ctypes.byref(d)) == 0, what
        assert L.tecm_temporal_attention(ctypes.byref(d), None) == -1, what           # TECM_E_ARG before any launch
        assert L.tecm_last_error(), what
    assert L.tecm_temporal_attention(None, None) == -1
    # the statistics need all their parts, a layer slot inside its range, and a workspace that holds one window
    for d in (_desc(node_stats=64), _desc(node_stats=64, lag_stats=64, counts=64, err_flag=64, layer=1),
              _desc(node_stats=64, lag_stats=64, counts=64, err_flag=64, ws=64, ws_floats=16),
              _desc(flags=16)):
        assert L.tecm_temporal_attention(ctypes.byref(d), None) == -1
    assert L.tecm_temporal_attention_ws_floats(ctypes.byref(_desc(matrix_stats=64, node_stats=64, T=32))) > 0


def test_an_export_over_max_bytes_is_refused_before_anything_runs():
    from tecmollm import temporal_attention
    model = types.SimpleNamespace(num_patches=21, num_nodes=2911, llm_backbone=types.SimpleNamespace(num_layers=3))
    x, tf = torch.zeros(2, 4, 2911, 6), torch.zeros(2, 4, 2911, 4)
    ei = torch.zeros(2, 0, dtype=torch.int64)
    need = 3 * 2 * 2911 * 12 * 21 * 21 * 4                                     # 0.37 GB: inside the default cap of 1 GiB
    with pytest.raises(ValueError, match=r"nodes=.*layers="):
        temporal_attention(model, x, tf, ei, max_bytes=need - 1)
    with pytest.raises(ValueError, match=str(need)):
        temporal_attention(model, x, tf, ei, max_bytes=1 << 20)
    big = types.SimpleNamespace(num_patches=90, num_nodes=2911, llm_backbone=types.SimpleNamespace(num_layers=3))
    with pytest.raises(ValueError, match=r"nodes=.*layers="):                  # 5.7 GB > the default 1 GiB
        temporal_attention(big, x, tf, ei)
    with pytest.raises(ValueError, match="layers"):
        temporal_attention(model, x, tf, ei, layers=[3])
    from tecmollm import TecmError
    with pytest.raises(TecmError):                                             # fits: goes on and refuses the CPU tensor
        temporal_attention(model, x, tf, ei, layers=[1], nodes=[0, 5], max_bytes=need)


def test_write_temporal_attention_writes_the_stated_files(tmp_path):
    from tecmollm.temporal_attention import derive, write_temporal_attention
    rows, cols, G, Ly, T = 2, 3, 2, 2, 4
    N = rows * cols
    rng = np.random.default_rng(0)
    p = np.tril(rng.random((5, N, 12, T, T)))
    p = (p / p.sum(-1, keepdims=True)).astype(np.float32)
    parts = [TA.accumulate_fast(p * s, [0, 1, 1, 0, 1], G) for s in (1.0, 0.5)]        # two "layers"
    node = np.stack([q[0] for q in parts], 1)
    lag = np.stack([q[1] for q in parts], 1)
    mat = np.stack([q[2] for q in parts], 1)
    att = derive(node, lag, parts[0][3], mat)
    paths = write_temporal_attention(att, str(tmp_path), grid=(rows, cols))
    assert sorted(os.path.basename(q) for q in paths.values()) == ["temporal_attention_by_layer.csv",
                                                                   "temporal_attention_maps.npz"]
    z = np.load(paths["npz"])
    assert set(z.files) == {"count", "entropy", "lookback", "sink_weight", "self_weight", "effective_tokens", "lookback_gap",
                            "lag_profile", "mean", "entropy_uniform", "lookback_uniform"}
    for k in ("entropy", "lookback", "sink_weight", "self_weight", "effective_tokens", "lookback_gap"):
        assert z[k].shape == (G, Ly, 12, rows, cols)
        np.testing.assert_array_equal(z[k][1, 0, 7].reshape(-1), att[k][1, 0, :, 7])
    assert z["lag_profile"].shape == (G, Ly, 12, T) and z["mean"].shape == (G, Ly, 12, T, T)
    assert z["count"].tolist() == [2.0, 3.0]
    np.testing.assert_allclose(z["mean"][:, 0].sum(-1), 1.0, rtol=1e-6)     # a mean of distributions is a distribution
    lines = open(paths["csv"]).read().strip().splitlines()
    assert lines[0] == ("group,layer,head,count,entropy_mean,lookback_mean,lookback_gap_mean,sink_weight_mean,"
                        "self_weight_mean")
    assert len(lines) == 1 + G * Ly * 12 and lines[1 + 12 * Ly].startswith("1,0,0,3,")
    assert float(lines[1 + 12 * Ly].split(",")[4]) == float(np.mean(att["entropy"][1, 0, :, 0]))
    without = dict(att)
    del without["mean"]
    assert "mean" not in np.load(write_temporal_attention(without, str(tmp_path / "b"), grid=(rows, cols))["npz"]).files
