"""numpy restatement of the member reordering (tecm_member_reorder, include/tecmollm.h (3n)) and of what surrounds it in
tecmollm/coherence.py, shared by tests/test_host_coherence.py and tests/test_gpu_coherence.py.

The total order of the contract -- numbers by <, equal numbers (-0.0 == +0.0) by member index, NaN after every number and
NaNs among themselves by member index -- is the order of `np.argsort(kind="stable")`: it compares with <, leaves equal keys
in their order of appearance and puts NaNs last in their order of appearance.  The values are sorted by that argsort and a
take, not by np.sort, so that the place of a -0.0 among zeros and of every NaN payload is defined; everything moves as
uint32 bit patterns."""
import numpy as np

F32, F64 = np.float32, np.float64


def ranks(template):
    """(K, ...) float32 -> int64 (K, ...): the position of every member among the K members of its cell."""
    order = np.argsort(template, axis=0, kind="stable")
    return np.argsort(order, axis=0, kind="stable")            # the inverse permutation of every cell


def reorder(values, template, want_ranks=False):
    """values, template (K, S, H, I) float32 -> out (K, S, H, I) float32: out[k] = the value of the cell whose position among
    the cell's values is the position of template[k] among the cell's template members; the bits of the values move."""
    values = np.ascontiguousarray(values, dtype=F32)
    assert values.shape == template.shape
    r = ranks(np.asarray(template, dtype=F32))
    order = np.argsort(values, axis=0, kind="stable")
    bits = np.take_along_axis(values.view(np.uint32), order, axis=0)           # the cell's values in the contract's order
    out = np.take_along_axis(bits, r, axis=0).view(F32)
    return (out, r.astype(np.uint8)) if want_ranks else out


def dated_template(series, rows, H):
    """series (T, I), rows (S, K) -> (template (K, S, H, I), bad (S,)): template[k, s, h] = series[rows[s, k] + h]; a sample with a
    row < 0 or a row + H > T is `bad` and its template is left at zero (nothing of the series is read for it)."""
    series, rows = np.asarray(series, dtype=F32), np.asarray(rows, dtype=np.int64)
    T, I = series.shape
    S, K = rows.shape
    bad = ((rows < 0) | (rows + H > T)).any(axis=1)
    out = np.zeros((K, S, H, I), dtype=F32)
    for s in np.flatnonzero(~bad):
        for k in range(K):
            out[k, s] = series[rows[s, k]:rows[s, k] + H]
    return out, bad


def reorder_dated(values, series, rows, want_ranks=False):
    """`reorder` with the dated template; the outputs of a bad sample are NaN and its ranks 255."""
    K, S, H, I = values.shape
    t, bad = dated_template(series, rows, H)
    out, r = reorder(values, t, want_ranks=True)
    out[:, bad] = np.nan
    r[:, bad] = 255
    return (out, r) if want_ranks else out


def quantile_members(levels, taus, K):
    """(B, Q, H, N) float32 levels at the probabilities taus -> (K, B, H, N) float32: the levels sorted per cell, member k the
    piecewise-linear quantile function at p_k = (k + 0.5) / K, float64 `lo + (hi - lo) * ((p_k - tau_j) / (tau_{j+1} - tau_j))`
    rounded to float32 once, clamped to the outermost level outside [tau_0, tau_{Q-1}]."""
    taus = [float(t) for t in taus]
    z = np.sort(np.asarray(levels, dtype=F32).astype(F64), axis=1)
    B, Q, H, N = z.shape
    out = np.empty((K, B, H, N), dtype=F32)
    for k in range(K):
        p = (k + 0.5) / K
        if p <= taus[0]:
            m = z[:, 0]
        elif p >= taus[-1]:
            m = z[:, Q - 1]
        else:
            j = max(n for n in range(Q - 1) if taus[n] <= p)
            w = (p - taus[j]) / (taus[j + 1] - taus[j])
            lo, hi = z[:, j], z[:, j + 1]
            m = lo + (hi - lo) * F64(w)
        out[k] = m.astype(F32)
    return out


def schaake_dates(num_rows, first_row, L_out, slots, slot, same_slot, k, min_gap, seed, window):
    """The date rule of `SchaakeTemplate`: candidates are the rows r >= first_row with r + L_out <= num_rows and, with
    same_slot, r < len(slots) and slots[r] == slot; they are visited in the order of
    `default_rng([seed, window]).permutation(candidates)` and one is taken unless it lies nearer than min_gap rows to a date
    already taken, until k are taken.  None when fewer than k can be had."""
    cand = [r for r in range(first_row, num_rows - L_out + 1)
            if not same_slot or (r < len(slots) and int(slots[r]) == slot)]
    perm = np.random.default_rng([seed, window]).permutation(np.asarray(cand, dtype=np.int64))
    taken = []
    for r in perm.tolist():
        if all(abs(r - c) >= min_gap for c in taken):
            taken.append(r)
            if len(taken) == k:
                return np.asarray(taken, dtype=np.int32)
    return None
