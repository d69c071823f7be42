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


# ---- the kernels' side: layouts, forms, the per-element merge bound and the case table of tests/test_gpu_segment_kernel.py ---------------
#   The kernels' unit of work is a 256-sample chunk of one row; a lane moves 16 bytes (VEC) when every length the index
# arithmetic uses and both bases are multiples of four samples, one dword otherwise.
CHUNK = 256
HALF = 2.0 ** -24
SCALES = (1.0, 1e3, 1e-3)                         # clip i of every row is scaled by SCALES[i % 3]

# (B, C, T, L, overlap, lead, trail); C > 1 runs the _c entries (clips ordered [b][segment][channel])
CASES = (
    (2, 1, 1280, 512, 128, 0, 0),                 # VEC, the tail clip on the hop grid (768 = 2 x 384)
    (1, 1, 1284, 512, 128, 0, 0),                 # VEC, the tail clip off the grid (772)
    (1, 1, 1280, 512, 0, 0, 0),                   # overlap 0: cover 1 except under the tail clip
    (2, 1, 1000, 252, 60, 0, 0),                  # chunk edges: L = 252, 256, 260 at a hop of 192
    (2, 1, 1000, 256, 64, 0, 0),
    (2, 1, 1000, 260, 68, 0, 0),
    (2, 1, 100, 256, 64, 0, 0),                   # T < L: one zero-padded clip
    (1, 2, 101, 256, 0, 0, 0),
    (1, 1, 256, 256, 64, 0, 0),                   # T = L
    (1, 1, 257, 256, 64, 0, 0),                   # T = L + 1: the second clip starts at 1
    (3, 1, 1001, 100, 25, 0, 0),                  # an odd hop
    (1, 1, 1000, 256, 62, 0, 0),                  # T and L multiples of 4, the hop (194) not
    (1, 1, 1024, 256, 192, 0, 0),                 # overlap 0.75 L: cover 4
    (1, 1, 1280, 512, 128, 128, 0),               # lead = overlap
    (1, 1, 1280, 512, 128, 20, 0),                # L' = 492: still VEC
    (1, 1, 1280, 512, 128, 21, 0),                # L' = 491: dword
    (1, 1, 1280, 512, 128, 8, 12),
    (1, 1, 100, 256, 64, 20, 0),                  # a short file with a lead
    (2, 2, 1284, 512, 128, 0, 0),                 # channel-grouped clips, C = 2 and 3
    (2, 3, 1001, 100, 25, 0, 0),
    (2, 3, 1280, 512, 128, 8, 12),
    (2, 2, 100, 256, 64, 0, 0),
)


def plan(T, L, overlap, lead=0, trail=0):
    """(hop, S, last, L', To) of the ABI's arguments"""
    st = starts(T, L, overlap)
    return L - overlap, len(st), max(T - L, 0), L - lead - trail, T - lead - trail


def forms(kind, T, L, overlap, lead=0, trail=0, in_off=0, out_off=0):
    """"vec" / "dword" of segment_split / segment_merge, from their launch conditions; in_off / out_off: samples the input / output base
    sits past a 16-byte boundary.  None: the geometry is refused"""
    if not (T > 0 and L > 0 and 0 <= overlap < L and lead >= 0 and trail >= 0 and lead + trail <= overlap and T - lead - trail >= 1):
        return None
    hop, S, last, Lp, To = plan(T, L, overlap, lead, trail)
    aligned = in_off % 4 == 0 and out_off % 4 == 0
    lengths = (T, L, hop) if kind == "split" else (To, Lp, hop, last)
    return "vec" if aligned and all(v % 4 == 0 for v in lengths) else "dword"


def steering(kind, T, L, overlap, lead=0, trail=0):
    """what of the chunk decode a case exercises"""
    hop, S, last, Lp, To = plan(T, L, overlap, lead, trail)
    n = L if kind == "split" else To
    out = {"chunks>1"} if n > CHUNK else {"chunks=1"}
    out.add("ragged_chunk" if n % CHUNK else "exact_chunk")
    if kind == "split" and T < L:
        out.add("zero_fill")
    if S > 1 and last % hop:
        out.add("tail_off_grid")
    if S > 1 and last % hop == 0:
        out.add("tail_on_grid")
    return out


def group(clips, B, S, C):
    """(B * C * S, n) ordered [row = b C + c][segment] -> (B * S * C, n) ordered [b][segment][channel], the layout of the _c entries"""
    n = clips.shape[-1]
    return np.ascontiguousarray(clips.reshape(B, C, S, n).transpose(0, 2, 1, 3)).reshape(B * S * C, n)


def ungroup(clips, B, S, C):
    n = clips.shape[-1]
    return np.ascontiguousarray(clips.reshape(B, S, C, n).transpose(0, 2, 1, 3)).reshape(B * C * S, n)


def split_input(B, C, T, seed=0):
    """(B * C, T) fp32, nowhere zero (a zero-filled tail is told from data)"""
    x = np.random.default_rng(1000 + seed + 7 * B + 3 * C + T).standard_normal((B * C, T)).astype(np.float32)
    return np.where(x == 0, np.float32(1.0), x)


def merge_input(B, C, T, L, overlap, lead=0, trail=0, seed=0):
    """(B * C * S, L') fp32 ordered [row][segment]: clip i of every row scaled by SCALES[i % 3], so that a neighbouring clip's sample, a
    weight off by one or a clip counted twice is outside the per-element bound at the quiet positions"""
    _, S, _, Lp, _ = plan(T, L, overlap, lead, trail)
    y = np.random.default_rng(2000 + seed + 7 * B + 3 * C + T + L).standard_normal((B * C, S, Lp))
    y *= np.asarray([SCALES[i % 3] for i in range(S)])[None, :, None]
    return y.astype(np.float32).reshape(B * C * S, Lp)


def merge_bound(y, T, L, overlap, lead=0, trail=0):
    """per element: (cover(t) + 2) x 2^-24 x sum_i w_i |y_i| / sum_i w_i -- the products round once each (together at most one such unit:
    the weights are exact, each product is within half an ulp of itself), cover - 1 rounded adds (the first lands on 0), the divide, and
    one unit for second order.  Holds with and without FMA contraction (an FMA drops a product's rounding)."""
    cnt, _ = cover(T, L, overlap, lead, trail)
    return (cnt + 2)[None, :] * HALF * merge(np.abs(np.asarray(y, np.float64)), T, L, overlap, lead, trail)


def merge_restate32(y, T, L, overlap, lead=0, trail=0, mutate=None):
    """float32 numpy, the sum in the kernel's order: acc = 0; acc += fl(w y) in increasing i (the tail clip last); acc / fl(sum w).
    mutate: "weights_min_j" (w = min(j, L' - j)), "tail_after_last" (the tail clip taken at t > last), "tail_twice" (a tail clip on the
    grid counted in the range too)"""
    hop, S, last, Lp, To = plan(T, L, overlap, lead, trail)
    y = np.asarray(y, np.float32).reshape(-1, S, Lp)
    j = np.arange(Lp)
    w = (np.minimum(j, Lp - j) if mutate == "weights_min_j" else np.minimum(j + 1, Lp - j)).astype(np.float32)
    acc, wsum = np.zeros((y.shape[0], To), np.float32), np.zeros(To, np.int64)
    st = starts(T, L, overlap)
    order = list(range(S))
    if mutate == "tail_twice" and S > 1 and last % hop == 0:
        order.insert(S - 1, S - 1)
    for i in order:
        s = int(st[i])
        n = min(Lp, To - s)
        lo = 1 if (mutate == "tail_after_last" and i == S - 1) else 0
        if n > lo:
            acc[:, s + lo:s + n] = acc[:, s + lo:s + n] + (w[lo:n] * y[:, i, lo:n]).astype(np.float32)
            wsum[s + lo:s + n] += w[lo:n].astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (acc / wsum.astype(np.float32)).astype(np.float32)
