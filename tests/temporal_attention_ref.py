"""float64 reference of the temporal attention export and its statistics (tecmollm/temporal_attention.py,
csrc/attention_probs.hip): the causal softmax from a qkv array, the row statistics / lag sums / matrix sums of a probability
array as ordered float64 loops, and a restatement of the GPT-2 trunk (oracle.ref_cpu.gpt2_lora) that also returns every
block's attention probabilities.  numpy / torch on the CPU only."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as R

HEADS = 12
HD = 64


def causal_probs(qkv: np.ndarray, B: int, T: int, N: int, D: int = HEADS * HD) -> np.ndarray:
    """qkv (B*T*N, 3*D) as the kernels read it (time-major rows (b*T + p)*N + n, columns [q | k | v]) -> float64 causal softmax
    (B, N, H, T, T), exact zeros beyond the diagonal.  Row 0 is [1, 0, ...] whatever q_0 holds (its q columns are not read:
    they may be NaN)."""
    a = np.asarray(qkv, np.float64).reshape(B, T, N, 3, D // HD, HD)
    q = a[:, :, :, 0].transpose(0, 2, 3, 1, 4)                  # (B, N, H, T, hd)
    k = a[:, :, :, 1].transpose(0, 2, 3, 1, 4)
    q = q.copy()
    q[:, :, :, 0] = 0.0
    s = q @ k.transpose(0, 1, 2, 4, 3) / 8.0
    mask = np.tril(np.ones((T, T), bool))
    s = np.where(mask, s, -np.inf)
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def values_of(qkv: np.ndarray, B: int, T: int, N: int, D: int = HEADS * HD) -> np.ndarray:
    """The v columns as float64 (B, N, H, T, hd)."""
    a = np.asarray(qkv, np.float64).reshape(B, T, N, 3, D // HD, HD)
    return a[:, :, :, 2].transpose(0, 2, 3, 1, 4)


def sequence_stats(p: np.ndarray) -> np.ndarray:
    """p (T, T) -> [entropy, look-back, sink, self] of one sequence: ordered float64 loops over i, then j, divided by T."""
    T = p.shape[0]
    ent = lb = sink = self_ = 0.0
    for i in range(T):
        for j in range(i + 1):
            v = float(p[i, j])
            if v > 0.0:
                ent -= v * math.log(v)
            lb += v * (i - j)
        sink += float(p[i, 0])
        self_ += float(p[i, i])
    return np.array([ent / T, lb / T, sink / T, self_ / T])


def accumulate_ref(probs: np.ndarray, groups, G: int):
    """probs (B, N, H, T, T) (the exported fp32 values) -> (node (G, 4, N, H), lag (G, H, T), matrix (G, H, T, T), counts (G))
    float64, windows in ascending b; an id outside [0, G) skips the window."""
    p = np.asarray(probs, np.float64)
    B, N, H, T, _ = p.shape
    node, lag, mat = np.zeros((G, 4, N, H)), np.zeros((G, H, T)), np.zeros((G, H, T, T))
    counts = np.zeros(G, np.int64)
    for b in range(B):
        g = 0 if groups is None else int(groups[b])
        if not 0 <= g < G:
            continue
        counts[g] += 1
        for n in range(N):
            for h in range(H):
                node[g, :, n, h] += sequence_stats(p[b, n, h])
                for d in range(T):
                    for i in range(d, T):
                        lag[g, h, d] += p[b, n, h, i, i - d]
                mat[g, h] += p[b, n, h]
    return node, lag, mat, counts


def accumulate_fast(probs: np.ndarray, groups, G: int):
    """The same sums with vectorised float64 numpy (for the full grid, where the loops take minutes): the order of the
    additions differs, which the tests' bar n * 2^-52 covers (every term is non-negative)."""
    p = np.asarray(probs, np.float64)
    B, N, H, T, _ = p.shape
    node, lag, mat = np.zeros((G, 4, N, H)), np.zeros((G, H, T)), np.zeros((G, H, T, T))
    counts = np.zeros(G, np.int64)
    i, j = np.arange(T).reshape(T, 1), np.arange(T).reshape(1, T)
    with np.errstate(divide="ignore", invalid="ignore"):
        plogp = np.where(p > 0, -p * np.log(np.where(p > 0, p, 1.0)), 0.0)
    per = np.stack([plogp.sum((-1, -2)) / T, (p * np.maximum(i - j, 0)).sum((-1, -2)) / T, p[..., :, 0].sum(-1) / T,
                    np.diagonal(p, axis1=-2, axis2=-1).sum(-1) / T], 1)            # (B, 4, N, H)
    lags = np.stack([np.diagonal(p, offset=-d, axis1=-2, axis2=-1).sum(-1) for d in range(T)], -1).sum(1)   # (B, H, T)
    for b in range(B):
        g = 0 if groups is None else int(groups[b])
        if not 0 <= g < G:
            continue
        counts[g] += 1
        node[g] += per[b]
        lag[g] += lags[b]
        mat[g] += p[b].sum(0)
    return node, lag, mat, counts


def terms(B_in_group: int, N: int, T: int):
    """Number of fp32 probabilities added into one cell of (node_stats, lag_stats[d = 0], matrix_stats), plus one per window
    for the division by T of the node cells: the n of the bar n * 2^-52."""
    return B_in_group * (T * (T + 1) // 2 + 1), B_in_group * N * T, B_in_group * N


def gpt2_lora_attentions(h: torch.Tensor, p, n_layers: int):
    """oracle.ref_cpu.gpt2_lora in eval mode (masks None, FP32 rounding), restated so that it also returns every block's
    attention probabilities: (last_hidden_state (S, T, 768), [w_0 .. w_{L-1}] each (S, 12, T, T)), in h's dtype."""
    S, T, D = h.shape
    hd = D // R.GPT2_HEADS
    h = h + p[R.P_GPT + "wpe.weight"][:T]
    causal = torch.tril(torch.ones(T, T, dtype=torch.bool))
    atts = []
    for i in range(n_layers):
        pre = f"{R.P_GPT}h.{i}."
        u = F.layer_norm(h, (D,), p[pre + "ln_1.weight"], p[pre + "ln_1.bias"], R.LN_EPS)
        A = p[pre + "attn.c_attn.lora_A.default.weight"]
        Bm = p[pre + "attn.c_attn.lora_B.default.weight"]
        z = u @ A.t()
        wcat = torch.cat([p[pre + "attn.c_attn.base_layer.weight"], R.LORA_SCALE * Bm.t()], 0)
        qkv = torch.cat([u, z], -1) @ wcat + p[pre + "attn.c_attn.base_layer.bias"]
        qq, k, v = qkv.split(D, dim=-1)
        qq = qq.view(S, T, R.GPT2_HEADS, hd).transpose(1, 2)
        k = k.view(S, T, R.GPT2_HEADS, hd).transpose(1, 2)
        v = v.view(S, T, R.GPT2_HEADS, hd).transpose(1, 2)
        w = ((qq @ k.transpose(-1, -2)) / math.sqrt(hd)).masked_fill(~causal, float("-inf")).softmax(-1)
        atts.append(w)
        ctx = (w @ v).transpose(1, 2).reshape(S, T, D)
        h = h + ctx @ p[pre + "attn.c_proj.weight"] + p[pre + "attn.c_proj.bias"]
        u = F.layer_norm(h, (D,), p[pre + "ln_2.weight"], p[pre + "ln_2.bias"], R.LN_EPS)
        f = R.gelu_new(u @ p[pre + "mlp.c_fc.weight"] + p[pre + "mlp.c_fc.bias"])
        h = h + f @ p[pre + "mlp.c_proj.weight"] + p[pre + "mlp.c_proj.bias"]
    return F.layer_norm(h, (D,), p[R.P_GPT + "ln_f.weight"], p[R.P_GPT + "ln_f.bias"], R.LN_EPS), atts


def model_attentions(x: torch.Tensor, tf: torch.Tensor, edge_index: torch.Tensor, p, cfg: dict, graphs_with_edges=1):
    """oracle.ref_cpu.forward up to the trunk, then `gpt2_lora_attentions`: [w_l (B, N, 12, T, T)] in the dtype of x / p."""
    B, L, N, _ = x.shape
    hh = R.embed(x, tf, p)
    xs = R.spatial(hh, edge_index, p, cfg["spatial_heads"], graphs_with_edges)
    C = xs.shape[-1]
    xt = xs.view(L, B, N, C).permute(1, 2, 0, 3).reshape(B * N, L, C)
    tok = R.temporal_encoder(xt, p, cfg["temporal_strides"], cfg["patch_len"])
    _, atts = gpt2_lora_attentions(tok, p, cfg["llm_layers"])
    return [w.reshape(B, N, *w.shape[1:]) for w in atts]
