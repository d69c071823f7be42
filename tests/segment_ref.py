"""numpy float64 restatement of the long-file segment plan, split and cross-fade merge (remfx_amd/segment.py, csrc/segment.hip)
for tests/test_segment_cpu.py and tests/test_gpu_segment.py.  Test infrastructure only; written from the formulas, not from the
implementation:

  hop = L - overlap;  s_i = min(i * hop, max(T - L, 0)) for i = 0 .. S-1, S the smallest count whose last segment reaches T
  split:  clip (r, i) = x[r, s_i : s_i + L], zeros beyond T
  merge:  a network returns L' = L - lead - trail samples per clip, sample j belonging to input sample s_i + lead + j;
          w[j] = min(j + 1, L' - j);  out[r, t] = sum_i w[t - s_i] y[r, i, t - s_i] / sum_i w[t - s_i] for t in [0, T - lead - trail),
          over the clips with 0 <= t - s_i < L' (t counts from input sample `lead`).
"""
import numpy as np


def starts(T, L, overlap):
    if not 0 <= overlap < L:
        raise ValueError("overlap")
    hop = L - overlap
    last = max(T - L, 0)
    out = [0]
    while out[-1] + L < T:                       # the last segment does not reach T yet: one more
        out.append(min(len(out) * hop, last))
    return np.asarray(out, dtype=np.int64)


def weights(Lp):
    j = np.arange(Lp)
    return np.minimum(j + 1, Lp - j).astype(np.float64)


def cover(T, L, overlap, lead=0, trail=0):
    """Number of clips covering every output index, and the summed weights."""
    Lp, To = L - lead - trail, T - lead - trail
    cnt, wsum = np.zeros(To, dtype=np.int64), np.zeros(To)
    w = weights(Lp)
    for s in starts(T, L, overlap):
        n = min(Lp, To - s)
        if n > 0:
            cnt[s:s + n] += 1
            wsum[s:s + n] += w[:n]
    return cnt, wsum


def split(x, L, overlap):
    """(rows, T) -> (rows * S, L)"""
    x = np.asarray(x)
    rows, T = x.shape
    st = starts(T, L, overlap)
    out = np.zeros((rows, len(st), L), dtype=x.dtype)
    for i, s in enumerate(st):
        n = min(L, T - s)
        out[:, i, :n] = x[:, s:s + n]
    return out.reshape(rows * len(st), L)


def merge(y, T, L, overlap, lead=0, trail=0):
    """(rows * S, L') -> (rows, T - lead - trail), float64"""
    Lp, To = L - lead - trail, T - lead - trail
    st = starts(T, L, overlap)
    y = np.asarray(y, dtype=np.float64).reshape(-1, len(st), Lp)
    w = weights(Lp)
    acc, wsum = np.zeros((y.shape[0], To)), np.zeros(To)
    for i, s in enumerate(st):                    # increasing i
        n = min(Lp, To - s)
        if n > 0:
            acc[:, s:s + n] += w[:n] * y[:, i, :n]
            wsum[s:s + n] += w[:n]
    return acc / wsum
