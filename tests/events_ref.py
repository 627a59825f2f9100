"""numpy restatement of the event-verification kernels (tecm_event_hist, tecm_event_fss), shared by
tests/test_host_events.py and tests/test_gpu_events.py: the value pipeline of tests/error_maps_ref.py, events by plain
comparison in float32, histograms by np.bincount, and the box sums of the fractions skill score by brute force over the
window offsets -- no summed-area table, so the restatement and the kernel share no trick.  Everything is an integer count:
the comparisons with the device are exact."""
import numpy as np

from tests.error_maps_ref import pipeline

F32 = np.float32


def threshold_field(values, strides, Q, slots, S, H, I):
    """(Q, S, H, I) float32: values.flat[q*sq + slot[s, h]*sk + i*si]; slots (S, H) ints or None (slot 0).  A slot the caller
    marks invalid must be masked by the caller: here it is read as slot 0."""
    flat = np.asarray(values, dtype=F32).reshape(-1)
    sq, sk, si = strides
    sl = np.zeros((S, H), dtype=np.int64) if slots is None else np.asarray(slots, dtype=np.int64)
    q = np.arange(Q)[:, None, None, None]
    i = np.arange(I)[None, None, None, :]
    return flat[q * sq + sl[None, :, :, None] * sk + i * si]


def events(v, thr, dirs):
    """(Q, ...) bool: v > thr[q] where dirs[q] > 0, v < thr[q] where dirs[q] < 0, in float32, strictly."""
    v = np.asarray(v, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.stack([(v > thr[q]) if dirs[q] > 0 else (v < thr[q]) for q in range(len(dirs))])


def valid_samples(S, H, G, groups=None, slots=None, num_slots=1):
    """(S,) group of every sample (-1: skipped) and (S, H) bool: the (sample, horizon) pairs that count."""
    g = np.zeros(S, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64).copy()
    g[(g < 0) | (g >= G)] = -1
    ok = np.ones((S, H), dtype=bool)
    if slots is not None:
        sl = np.asarray(slots, dtype=np.int64)
        ok &= (sl >= 0) & (sl < num_slots)
    ok &= (g >= 0)[:, None]
    return g, ok


def accumulate_hist(hist, members, true, values, strides, dirs, groups=None, scaler=None, slots=None, num_slots=1):
    """One update into hist (G, Q, H, K+1, 2, I) int64 from members (K, S, H, I) and true (S, H, I), scaled float32.
    Returns the number of ties met: values (of any member or of the truth) equal to their threshold."""
    K, S, H, I = members.shape
    G, Q = hist.shape[0], len(dirs)
    g, ok = valid_samples(S, H, G, groups, slots, num_slots)
    safe = None if slots is None else np.where((np.asarray(slots) >= 0) & (np.asarray(slots) < num_slots), slots, 0)
    thr = threshold_field(values, strides, Q, safe, S, H, I)
    j = np.zeros((Q, S, H, I), dtype=np.int64)
    ties = 0
    t = None
    for k in range(K):
        t, p = pipeline(members[k], true, scaler)
        j += events(p, thr, dirs)
        ties += int((p[None] == thr).sum())
    o = events(t, thr, dirs)
    ties += int((t[None] == thr).sum())
    hh, ii = np.meshgrid(np.arange(H), np.arange(I), indexing="ij")
    for s in range(S):
        if g[s] < 0:
            continue
        m = np.broadcast_to(ok[s][:, None], (H, I))
        for q in range(Q):
            flat = ((hh * (K + 1) + j[q, s]) * 2) * I + ii
            n = np.bincount(flat[m], minlength=H * (K + 1) * 2 * I)
            n += np.bincount((flat + I)[m & o[q, s]], minlength=H * (K + 1) * 2 * I)
            hist[g[s], q] += n.reshape(H, K + 1, 2, I)
    return ties


def box_sums(field, n):
    """(rows, cols) int64: the sum of the binary `field` over the n x n window centred on every cell, cells outside the grid
    counting 0 -- one shifted addition per window offset that can reach the grid."""
    rows, cols = field.shape
    half = n // 2
    b = field.astype(np.int64)
    out = np.zeros((rows, cols), dtype=np.int64)
    for dr in range(-min(half, rows - 1), min(half, rows - 1) + 1):
        for dc in range(-min(half, cols - 1), min(half, cols - 1) + 1):
            r0, r1 = max(0, -dr), min(rows, rows - dr)                     # out[r, c] += b[r + dr, c + dc]
            c0, c1 = max(0, -dc), min(cols, cols - dc)
            out[r0:r1, c0:c1] += b[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return out


def box_sums_sat(field, n):
    """The same by a summed-area table (np.cumsum): a second implementation, to check `box_sums` against."""
    rows, cols = field.shape
    half = n // 2
    P = np.zeros((rows + 1, cols + 1), dtype=np.int64)
    P[1:, 1:] = np.cumsum(np.cumsum(field.astype(np.int64), axis=0), axis=1)
    r = np.arange(rows)[:, None]
    c = np.arange(cols)[None, :]
    r0, r1 = np.maximum(r - half, 0), np.minimum(r + half, rows - 1) + 1
    c0, c1 = np.maximum(c - half, 0), np.minimum(c + half, cols - 1) + 1
    return P[r1, c1] - P[r0, c1] - P[r1, c0] + P[r0, c0]


def fss_terms(bf, bo, n):
    """[sum (cf - co)^2, sum cf^2, sum co^2] as Python ints."""
    cf, co = box_sums(bf, n), box_sums(bo, n)
    return [int(((cf - co) ** 2).sum()), int((cf ** 2).sum()), int((co ** 2).sum())]


def accumulate_fss(sums, pred, true, values, strides, dirs, widths, grid, groups=None, scaler=None, slots=None, num_slots=1):
    """One update into sums (G, Q, H, W, 3) int64 from pred and true (S, H, I), scaled float32, on the (rows, cols) grid."""
    S, H, I = pred.shape
    rows, cols = grid
    G, Q = sums.shape[0], len(dirs)
    g, ok = valid_samples(S, H, G, groups, slots, num_slots)
    safe = None if slots is None else np.where((np.asarray(slots) >= 0) & (np.asarray(slots) < num_slots), slots, 0)
    thr = threshold_field(values, strides, Q, safe, S, H, I)
    t, p = pipeline(pred, true, scaler)
    ef, eo = events(p, thr, dirs), events(t, thr, dirs)
    for s in range(S):
        for h in range(H):
            if not ok[s, h]:
                continue
            for q in range(Q):
                bf, bo = ef[q, s, h].reshape(rows, cols), eo[q, s, h].reshape(rows, cols)
                for w, n in enumerate(widths):
                    sums[g[s], q, h, w] += np.array(fss_terms(bf, bo, n), dtype=np.int64)


def fss(sums):
    s = np.asarray(sums, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 1.0 - s[..., 0] / (s[..., 1] + s[..., 2])


def contingency(hist):
    """K = 1 hist (..., 2, 2, I) -> hits, false alarms, misses, correct negatives."""
    n0, o0, n1, o1 = hist[..., 0, 0, :], hist[..., 0, 1, :], hist[..., 1, 0, :], hist[..., 1, 1, :]
    return o1, n1 - o1, o0, n0 - o0
