"""Segmented long-file inference: cut a file into overlapping training-length clips on the device, run a network on batches
of clips, cross-fade the results back into one signal (csrc/segment.hip).  split / merge make every channel a
mono clip of its own; split_c / merge_c keep a clip's channels together for networks that take (clips, C, L) and return
(clips, Co, L') -- multi-source Hybrid Demucs (HDemucs.separate).

The reference's single-file path (scripts/remfx_detect.py:44-55) hands the whole file to the chain as one clip of arbitrary
length; the demucs family cuts it instead (`apply_model(split=True, overlap=...)`).  Here:

  hop = segment - overlap;   s_i = min(i * hop, max(T - segment, 0)),  i = 0 .. S-1
  S   = 1 for T <= segment, else ceil((T - segment) / hop) + 1: the smallest count whose last segment reaches T.

The LAST segment is tail-aligned (it ends at T) whenever T >= segment, never zero-padded: a mostly silent clip would make
Hybrid Demucs divide by a near-zero standard deviation and would hand the detector silence.  Only a file shorter than one
segment is padded.  A network that returns L' = segment - lead - trail samples per clip (output sample j belonging to input
sample j + lead: a causal TCN has lead = segment - L', trail = 0) owns the window [s_i + lead, s_i + segment - trail) of clip
i; lead + trail <= overlap makes those windows abut, and the merged signal covers [lead, T - trail) -- exactly what the same
network returns for the whole file.  Inside the overlaps the clips are cross-faded with the triangular weights
w[j] = min(j + 1, L' - j) over the valid window.
"""
import numpy as np
import torch

from . import ops


class SegmentPlan:
    """The geometry above for T samples.  `starts` (int64 array, input coordinates), `n_segments`, `hop`, `clip_len` (L'),
    `out_len` (T - lead - trail) and `max_cover` (the largest number of clips any output sample is blended from)."""

    def __init__(self, T, segment, overlap, lead=0, trail=0):
        T, segment, overlap, lead, trail = int(T), int(segment), int(overlap), int(lead), int(trail)
        if segment <= 0 or T <= 0:
            raise ValueError(f"SegmentPlan: need T > 0 and segment > 0 (got T={T}, segment={segment})")
        if not 0 <= overlap < segment:
            raise ValueError(f"SegmentPlan: need 0 <= overlap < segment (got overlap={overlap}, segment={segment})")
        if lead < 0 or trail < 0 or lead + trail > overlap:
            raise ValueError(f"SegmentPlan: lead + trail = {lead} + {trail} must lie in [0, overlap = {overlap}], otherwise the "
                             "clips' valid windows leave gaps")
        if T - lead - trail < 1:
            raise ValueError(f"SegmentPlan: {T} samples are too few for a network that drops {lead} + {trail} of them")
        if max(T, segment) >= 1 << 30:
            raise ValueError("SegmentPlan: lengths are limited to 2^30 samples")
        self.T, self.segment, self.overlap, self.lead, self.trail = T, segment, overlap, lead, trail
        self.hop = segment - overlap
        self.last = max(T - segment, 0)
        self.n_segments = 1 if T <= segment else -(-(T - segment) // self.hop) + 1
        self.starts = np.minimum(np.arange(self.n_segments, dtype=np.int64) * self.hop, self.last)
        self.clip_len = segment - lead - trail
        self.out_len = T - lead - trail
        # the cover count only rises at a window's first sample: evaluate it there
        first = np.minimum(self.starts, self.out_len - 1)
        self.max_cover = int((np.searchsorted(self.starts, first, side="right")
                              - np.searchsorted(self.starts + self.clip_len, first, side="right")).max())

    def weights(self):
        j = np.arange(self.clip_len, dtype=np.int64)
        return np.minimum(j + 1, self.clip_len - j)

    def __repr__(self):
        return (f"SegmentPlan(T={self.T}, segment={self.segment}, overlap={self.overlap}, lead={self.lead}, trail={self.trail}: "
                f"{self.n_segments} segments, hop {self.hop})")


def overlap_samples(segment, overlap):
    """`overlap` as samples: a float below 1 is a fraction of the segment, an integer is a sample count."""
    if isinstance(overlap, float):
        if not 0.0 <= overlap < 1.0:
            raise ValueError(f"overlap fraction must lie in [0, 1) (got {overlap})")
        return int(segment * overlap)
    return int(overlap)


def split(x, plan):
    """(B, C, T) -> (B * C * S, 1, L): every channel is a row of its own, clip i of row r at index r * S + i."""
    ops._req(x, "segment.split")
    if x.dim() != 3 or x.shape[-1] != plan.T:
        raise ValueError(f"segment.split: expected (B, C, {plan.T}), got {tuple(x.shape)}")
    x = x.contiguous()
    rows = x.shape[0] * x.shape[1]
    out = torch.empty(rows * plan.n_segments, 1, plan.segment, device=x.device, dtype=torch.float32)
    ops.launch("rfx_segment_split", x, out, rows, plan.T, plan.segment, plan.hop, plan.n_segments)
    return out


def merge(y, plan, channels=1, out=None):
    """(rows * S, 1, L') or (rows * S, L') -> (rows / channels, channels, T - lead - trail), the inverse layout of split()."""
    ops._req(y, "segment.merge")
    S = plan.n_segments
    if y.shape[-1] != plan.clip_len or y.numel() % (S * plan.clip_len) or y.numel() == 0:
        raise ValueError(f"segment.merge: expected (rows * {S}, {plan.clip_len}) clips, got {tuple(y.shape)}")
    rows = y.numel() // (S * plan.clip_len)
    if rows % channels:
        raise ValueError(f"segment.merge: {rows} rows do not split into {channels} channels")
    y = y.contiguous()
    if out is None:
        out = torch.empty(rows // channels, channels, plan.out_len, device=y.device, dtype=torch.float32)
    else:
        ops._req(out, "segment.merge out")
        if out.numel() != rows * plan.out_len or not out.is_contiguous():
            raise ValueError(f"segment.merge: out must be contiguous with {rows} x {plan.out_len} samples")
    ops.launch("rfx_segment_merge", y, out, rows, plan.T, plan.segment, plan.hop, plan.lead, plan.trail, S)
    return out


def split_c(x, plan):
    """(B, C, T) -> (B * S, C, L): the channels of a clip stay together, clip i of signal b at index b * S + i."""
    ops._req(x, "segment.split_c")
    if x.dim() != 3 or x.shape[-1] != plan.T:
        raise ValueError(f"segment.split_c: expected (B, C, {plan.T}), got {tuple(x.shape)}")
    x = x.contiguous()
    B, Cn = x.shape[0], x.shape[1]
    out = torch.empty(B * plan.n_segments, Cn, plan.segment, device=x.device, dtype=torch.float32)
    ops.launch("rfx_segment_split_c", x, out, B, Cn, plan.T, plan.segment, plan.hop, plan.n_segments)
    return out


def merge_c(y, plan):
    """(B * S, Co, L') -> (B, Co, T - lead - trail), the inverse layout of split_c(); Co is whatever the network returned."""
    ops._req(y, "segment.merge_c")
    S = plan.n_segments
    if y.dim() != 3 or y.shape[-1] != plan.clip_len or y.shape[0] % S or y.numel() == 0:
        raise ValueError(f"segment.merge_c: expected (B * {S}, Co, {plan.clip_len}) clips, got {tuple(y.shape)}")
    y = y.contiguous()
    B, Co = y.shape[0] // S, y.shape[1]
    out = torch.empty(B, Co, plan.out_len, device=y.device, dtype=torch.float32)
    ops.launch("rfx_segment_merge_c", y, out, B, Co, plan.T, plan.segment, plan.hop, plan.lead, plan.trail, S)
    return out


def _crop(segment, clip_len, align):
    drop = segment - clip_len
    if drop < 0:
        raise ValueError(f"segment.apply: the network returned {clip_len} samples for a {segment}-sample clip")
    if align == "same":
        if drop:
            raise ValueError(f"segment.apply: align='same' but the network returned {clip_len} of {segment} samples; "
                             "use align='end' (causal) or 'center'")
        return 0, 0
    if align == "end":
        return drop, 0
    if align == "center":
        return drop // 2, drop - drop // 2            # utils.center_crop
    raise ValueError(f"segment.apply: align must be 'same', 'end' or 'center' (got {align!r})")


def apply(fn, x, segment=262144, overlap=0.25, batch=64, align="same", group_channels=False):
    """fn on a long (B, C, T) signal through clips of `segment` samples: split, fn on sub-batches of at most `batch` clips (each
    (n, 1, segment) -> (n, 1, L')), cross-fade merge.  L' is read off the first result; `align` says where those samples sit in
    the clip: "same" (L' = segment), "end" (a causal network: the last L'), "center".

    group_channels=True keeps the channels of a clip together for a network that mixes them: fn sees (n, C, segment) and returns
    (n, Co, L') or (n, S, Cc, L') (flattened to Co = S * Cc); the result is (B, Co, T - lead - trail)."""
    ops._req(x, "segment.apply")
    B, Cn, T = x.shape
    ov = overlap_samples(segment, overlap)
    if group_channels:
        clips = split_c(x, SegmentPlan(T, segment, ov))
        n = clips.shape[0]
        res, plan = None, None
        for k in range(0, n, max(1, int(batch))):
            y = fn(clips[k:k + batch])
            if res is None:
                if y.dim() not in (3, 4):
                    raise ValueError(f"segment.apply: with group_channels the network returns (n, Co, L') or (n, S, Cc, L'), got {tuple(y.shape)}")
                lead, trail = _crop(segment, y.shape[-1], align)
                plan = SegmentPlan(T, segment, ov, lead, trail)
                res = torch.empty(n, y.numel() // (y.shape[0] * plan.clip_len), plan.clip_len, device=x.device, dtype=torch.float32)
            res[k:k + batch].copy_(y.reshape(-1, res.shape[1], plan.clip_len))
        return merge_c(res, plan)
    clips = split(x, SegmentPlan(T, segment, ov))
    n = clips.shape[0]
    res, plan = None, None
    for k in range(0, n, max(1, int(batch))):
        y = fn(clips[k:k + batch])
        if res is None:
            lead, trail = _crop(segment, y.shape[-1], align)
            plan = SegmentPlan(T, segment, ov, lead, trail)
            res = torch.empty(n, 1, plan.clip_len, device=x.device, dtype=torch.float32)
        res[k:k + batch].copy_(y.reshape(-1, 1, plan.clip_len))
    return merge(res, plan, channels=Cn)
