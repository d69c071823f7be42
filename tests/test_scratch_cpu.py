"""Every scratch-size query of include/remfx_hip.h, called without a device (the library loads on a machine with no GPU): each `_ws`
query the package sizes a buffer with is swept through zero and negative geometry, through the first values at which its launcher's
grid cap binds (the uncapped workgroup count at cap - 1, cap, cap + 1) and one large value, and has to equal BOTH

  * the independent restatement of the kernel's rule in tests/*_ref.py, and
  * the expression the Python call site spelled before the library owned the size (written out below, OLD): no allocation of the
    package changed its length when the queries took over.

The older total-size queries with plain arguments are swept in test_older_total_size_queries (rfx_stft_scaled_loss_ws, rfx_wiener_ws_floats,
the rfx_fx_*_ws_* family; rfx_time_sums_ws, rfx_logcosh_ws and rfx_norm_bwd_work_floats beside their new neighbours).  Those that take a
descriptor or a tensor are swept where their geometry tables live: rfx_fft_synthesis_ws in tests/test_fft_any_cpu.py and, per case against
fft_ref, in tests/test_gpu_fft_kernel.py with rfx_stft_pair_loss_ws; rfx_channel_sum_ws against elem_ref.channel_geometry in
tests/test_gpu_elem_kernel.py; rfx_cl_wgrad_ws_floats against clast_ref in tests/test_gpu_clast_kernel.py.

test_header_declares_a_query_for_every_scratch_parameter keeps the rule of the header's conventions block true: a prototype with a
parameter named ws / work / partial / hop_ws / env_ws has a `_ws` query."""
import ctypes as C
import itertools
import os
import re

import pytest

from remfx_amd import _lib
from tests import cldconv_ref as CLD
from tests import cplx_ref as CX
from tests import dconv_ref as D
from tests import elem_ref as E
from tests import fft_ref as F
from tests import loss_ref as X
from tests import norm_ref as NR
from tests import optim_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 64 * 262144                                               # a 64-clip batch of 262144 samples as one flat length
MAX_ROWS = 65535


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def around(cap, per):
    """lengths whose uncapped workgroup count ceil(n / per) is cap - 1, cap, cap + 1, and the edges of each"""
    return (per * (cap - 1), per * (cap - 1) + 1, per * cap, per * cap + 1, per * (cap + 1))


def ceil_div(a, b):
    return -(-a // b)


# ---- flat reductions: the size is the cap itself, for every n ---------------------------------------------------------------------------
def test_sumsq(L):
    for n in (-5, -1):
        assert L.rfx_sumsq_ws(n) == -1
    for n in (0, 1, 1023, 1025, BIG) + around(O.SLOTS, 1024):
        got = L.rfx_sumsq_ws(n)
        assert got == O.SLOTS, n                                 # tests/optim_ref.py
        assert got == 4096, n                                    # OLD optim.py: torch.empty(4096)
        assert O.forms(n)["slots"] <= got, n                     # what the launcher writes fits
    assert O.forms(O.SLOTS * 1024 + 1)["slots"] == O.SLOTS


def test_l1_sum(L):
    for n in (-5, -1):
        assert L.rfx_l1_sum_ws(n) == -1
    for n in (0, 1, 1025, BIG) + around(E.L1_SLOTS, 1024) + around(2048, 1024):
        got = L.rfx_l1_sum_ws(n)
        assert got == E.L1_SLOTS, n                              # tests/elem_ref.py
        assert got == 512, n                                     # OLD losses.py: torch.empty(512)
        assert E.l1_slots(n) <= got and (n <= 0 or E.l1_slots(n) == min(E.grid_for(n), got)), n
    first_past = next(n for n in range(1024 * 511, 1024 * 513) if E.grid_for(n) > E.L1_SLOTS)
    assert first_past == 1024 * 512 + 1 and first_past in E.L1_N  # the GPU case one workgroup past the cap


ROWS_SWEEP = (-1, 0, 1, 3, 64, MAX_ROWS, MAX_ROWS + 1)


def test_stft_loss_reduce(L):
    for R, n in itertools.product(ROWS_SWEEP, (-1, 0, 1, 40001, BIG) + around(F.REDUCE_SLOTS, 16384)):
        got = L.rfx_stft_loss_reduce_ws(R, n)
        if R <= 0 or R > MAX_ROWS or n <= 0:
            assert got == -1, (R, n)
            continue
        assert got == 3 * R * F.REDUCE_SLOTS, (R, n)             # tests/fft_ref.py
        assert got == 3 * R * 64, (R, n)                         # OLD losses.py: torch.empty(3 * R * 64)
        assert 3 * R * min(max(ceil_div(n, 16384), 1), F.REDUCE_SLOTS) <= got


def test_sisdr_sums_and_the_exact_time_queries(L):
    for R, Ln in itertools.product(ROWS_SWEEP, (-1, 0, 1, 2049, 70001, BIG) + around(X.SLOTS, 2048) + around(512, 2048)):
        got = L.rfx_sisdr_sums_ws(R, Ln)
        if R <= 0 or R > MAX_ROWS or Ln <= 0:
            assert got == -1, (R, Ln)
            if R <= 0 or Ln <= 0:
                assert L.rfx_time_sums_ws(R, Ln) == 0 and L.rfx_logcosh_ws(R, Ln) == 0, (R, Ln)
            continue
        assert got == 5 * R * X.SLOTS, (R, Ln)                   # tests/loss_ref.py
        assert got == 5 * R * 128, (R, Ln)                       # OLD losses.py: torch.empty(5 * R * 128)
        g = min(X.grid_x(Ln), X.SLOTS)
        assert g == X.time_sums_grid(Ln)
        assert L.rfx_time_sums_ws(R, Ln) == 5 * R * g <= got and L.rfx_logcosh_ws(R, Ln) == R * g, (R, Ln)
    assert X.grid_x(X.SLOTS * 2048 + 1) == X.SLOTS + 1           # the GPU case one workgroup past the cap


# ---- one slot per (row, chunk) ----------------------------------------------------------------------------------------------------------
def test_prelu_bwd(L):
    for N, Cc, Ln in itertools.product((-1, 0, 1, 3, 64), (-1, 0, 1, 2, 256), (-1, 0, 1, BIG)):
        got = L.rfx_prelu_bwd_ws(N, Cc, Ln)
        if N <= 0 or Cc <= 0 or Ln <= 0:
            assert got == -1, (N, Cc, Ln)
        else:
            assert got == N * Cc, (N, Cc, Ln)                    # OLD dptnet.py: torch.empty(N * C); elem_ref.prelu_bwd: a slot per (n, c)
    assert L.rfx_prelu_bwd_ws(2 ** 16, 2 ** 15, 4) == -1 and L.rfx_prelu_bwd_ws(2 ** 16, 2 ** 15 - 1, 4) == 2 ** 16 * (2 ** 15 - 1)


def test_row_moments(L):
    for R, Ln in itertools.product((-1, 0, 1, 3, 64), (-1, 0, 1, 2, 16385, 40001, BIG) + around(256, 16384)):
        got = L.rfx_row_moments_ws(R, Ln)
        if R <= 0 or Ln <= 1:
            assert got == -1, (R, Ln)
            continue
        assert got == 2 * R * E.moments_slots(Ln), (R, Ln)       # tests/elem_ref.py
        slots_old = min(max(ceil_div(Ln, 16384), 1), 256)        # what rfx_row_moments_slots(L) answered
        assert got == 2 * R * slots_old, (R, Ln)                 # OLD nnops.py: 2 * R * query("rfx_row_moments_slots", L)


CHUNK_S = (-1, 0, 1, 4095, 4096, 4097, 8193, 262144)


def test_cplx(L):
    for N, Cc, S in itertools.product((-1, 0, 1, 3, 64), (-1, 0, 1, 45), CHUNK_S + (BIG,)):
        m, a = L.rfx_cplx_moments_ws(N, Cc, S), L.rfx_cplx_affine_act_bwd_ws(N, Cc, S)
        if N <= 0 or Cc <= 0 or S <= 0:
            assert (m, a) == (-1, -1), (N, Cc, S)
            continue
        assert (m, a) == (CX.moments_ws(N, Cc, S), CX.affine_bwd_ws(N, Cc, S)), (N, Cc, S)      # tests/cplx_ref.py
        slots_old = N * ceil_div(S, 4096)                        # what rfx_cplx_slots(N, S) answered
        assert slots_old == CX.slots(N, S)
        assert (m, a) == (5 * Cc * slots_old, 6 * Cc * slots_old), (N, Cc, S)                   # OLD dcunet.py: 5 * Cc * slots, 6 * Cc * slots
    # the launchers refuse more than 2^31 - 1 slots per channel
    assert L.rfx_cplx_moments_ws(2 ** 20, 1, 4096 * 2 ** 11) == -1 and L.rfx_cplx_moments_ws(2 ** 20, 1, 4096 * (2 ** 11 - 1)) > 0


def test_batchnorm_and_groupnorm_statistics(L):
    for N, Cc, S in itertools.product((-1, 0, 1, 3, 70), (-1, 0, 1, 8, 48), CHUNK_S):
        got = L.rfx_batchnorm_fwd_ws(N, Cc, S)
        if N <= 0 or Cc <= 0 or S <= 0:
            assert got == -1, (N, Cc, S)
        else:
            assert got == 2 * Cc * NR.bn_stat_slots(N, S), (N, Cc, S)                            # tests/norm_ref.py
            assert got == Cc * 2 * (N * ceil_div(S, 4096)), (N, Cc, S)      # OLD nnops.py: Cc * 2 * query("rfx_batchnorm_stat_slots", N, S)
        for G in (-1, 0, 1, 2, 8, 5):
            got, chunks = L.rfx_groupnorm_fwd_ws(N, Cc, S, G), L.rfx_groupnorm_stat_chunks(Cc, S, G)
            if N <= 0 or Cc <= 0 or S <= 0 or G <= 0 or Cc % G:
                assert got == -1, (N, Cc, S, G)
                continue
            assert chunks == NR.stat_chunks(Cc, S, G) and got == 2 * N * G * NR.stat_chunks(Cc, S, G), (N, Cc, S, G)
            assert got == N * G * 2 * max(chunks, 1), (N, Cc, S, G)         # OLD nnops.py: N * groups * 2 * max(chunks, 1)
    assert L.rfx_groupnorm_fwd_ws(64, 48, 262144, 1) == 2 * 64 * ceil_div(48 * 262144, 4096)
    # the older total-size query of the family keeps its restatement
    for N, Cc, S, G in ((3, 8, 4097, 2), (70, 48, 231, 0), (1, 2, 1, 1)):
        assert L.rfx_norm_bwd_work_floats(N, Cc, S, G) == NR.work_floats(N, Cc, S, G)
    assert L.rfx_norm_bwd_work_floats(0, 8, 8, 1) == -1 and L.rfx_norm_bwd_work_floats(3, 8, -1, 1) == -1


def test_dconv_layer_bwd(L):
    for N in (1, 2, 3, 100000) + around(256, 2):
        for dil in (1, 2):
            got = L.rfx_dconv_layer_bwd_ws(N, D.C, D.T, dil)
            assert got == D.bwd_rows(N) * D.ROWS, N              # tests/dconv_ref.py
            rows_old = min((N + 1) // 2, 256)                    # what rfx_dconv_layer_bwd_rows(N) answered
            assert got == rows_old * (5 * D.C + 2 * (D.C // 4)), N          # OLD nnops.py: (rows, 5 * Cc + 2 * H)
    for bad in ((0, 48, 256, 1), (-3, 48, 256, 1), (4, 96, 256, 1), (4, 48, 512, 1), (4, 48, 256, 0), (4, 48, 256, 3)):
        assert L.rfx_dconv_layer_bwd_ws(*bad) == -1, bad


# ---- channels-last family ---------------------------------------------------------------------------------------------------------------
def test_cl_rowsum(L):
    for N, A, B, Cc, G in itertools.product((-1, 0, 1, 2100), (-1, 0, 1, 5), (0, 64), (-8, 0, 8, 12, 256, 264), (-1, 0, 1, 410, 2048)):
        got = L.rfx_cl_rowsum_ws(N, A, B, Cc, G)
        if N <= 0 or A <= 0 or B <= 0 or Cc <= 0 or Cc % 8 or Cc > 256 or G < 1:
            assert got == -1, (N, A, B, Cc, G)
        else:
            assert got == G * A * Cc, (N, A, B, Cc, G)           # OLD clchain.py: torch.empty((G, A, Cc)); clast_ref.restate_rowsum: G partials


def _cld(S, Cc, H, grid, TPS):
    d = _lib.ClDconvDesc()
    d.S, d.C, d.H, d.grid, d.TPS, d.dil = S, Cc, H, grid, TPS, 1
    return C.byref(d)


def test_cl_dconv(L):
    for Cc, TPS, nsamp, grid in itertools.product((48, 96), (1, 2, 3), (1, 2, 3, 255, 256, 257, 16384), (1, 3, 256, 304)):
        S, H = nsamp * TPS, Cc // 4
        d = _cld(S, Cc, H, grid, TPS)
        G = CLD.forms(Cc, TPS, nsamp, grid, True)[1]["G"]        # tests/cldconv_ref.py: workgroups = rows of `partial`
        passes = "means" in CLD.forms(Cc, TPS, nsamp, grid, True)[0]
        assert G == min(grid, S) and passes == (TPS > 1 or Cc != 48)
        npg = 5 * Cc + 2 * H
        # OLD cldconv.py: part (S, 2) if TPS > 1; partial (min(GRID, S), npg); tsum (S, 2), sums (Bn * A, 4) if passes
        assert L.rfx_cl_dconv_fwd_ws_partial(d) == (S * 2 if TPS > 1 else 0), (Cc, TPS, nsamp, grid)
        assert L.rfx_cl_dconv_bwd_ws_partial(d) == G * npg == min(grid, S) * npg, (Cc, TPS, nsamp, grid)
        assert L.rfx_cl_dconv_bwd_ws_tsum(d) == (S * 2 if passes else 0), (Cc, TPS, nsamp, grid)
        assert L.rfx_cl_dconv_bwd_ws_sums(d) == (nsamp * 4 if passes else 0), (Cc, TPS, nsamp, grid)
    queries = (L.rfx_cl_dconv_fwd_ws_partial, L.rfx_cl_dconv_bwd_ws_partial, L.rfx_cl_dconv_bwd_ws_tsum, L.rfx_cl_dconv_bwd_ws_sums)
    for bad in ((0, 48, 12, 256, 1), (-4, 48, 12, 256, 1), (4, 48, 12, 0, 1), (4, 48, 12, -1, 1), (4, 48, 12, 256, 0), (4, 48, 12, 256, 3),
                (4, 64, 16, 256, 1), (4, 48, 24, 256, 1)):
        for q in queries:
            assert q(_cld(*bad)) == -1, bad
    for q in queries:
        assert q(None) == -1


# ---- effects ----------------------------------------------------------------------------------------------------------------------------
def test_fx(L):
    for B, T in itertools.product((-1, 0, 1, 3, 65535, 65536), (-1, 0, 1, 262144)):
        c, lim = L.rfx_fx_compressor_ws(B, T), L.rfx_fx_limiter_ws(B, T)
        if B <= 0 or B > 65535 or T <= 0:
            assert (c, lim) == (-1, -1), (B, T)
        else:
            assert c == B * T, (B, T)                            # OLD effects.py: torch.empty_like(clips), clips (B, T)
            assert lim == 2 * B * T, (B, T)                      # OLD effects.py: torch.empty((2, N, T))
    T, chunk, hop, nblk = 262144, 4096, 4410, 56
    nhop = nblk + 3
    for B, Cc in itertools.product((-1, 0, 1, 64, 65535, 65536), (-1, 0, 1, 2)):
        j = L.rfx_fx_loudness_joint_ws(B, Cc, T, chunk, hop, nhop, nblk)
        ok = B > 0 and Cc > 0 and B * Cc <= 65535
        assert j == (B * Cc * nhop if ok else -1), (B, Cc)       # OLD effects.py: torch.empty((B * Ch, nhop))
        if Cc == 1:
            assert L.rfx_fx_loudness_ws(B, T, chunk, hop, nhop, nblk) == (B * nhop if ok else -1), B      # OLD: torch.empty((N, nhop))
    for bad in ((0, chunk, hop, nhop, nblk), (T, 0, hop, nhop, nblk), (T, chunk, 0, nhop, nblk), (T, chunk, hop, 3, 1), (T, chunk, hop, nhop, 0),
                (T, chunk, hop, nblk + 2, nblk), (T, T // 64 - 1, hop, nhop, nblk)):
        assert L.rfx_fx_loudness_ws(4, *bad) == -1 and L.rfx_fx_loudness_joint_ws(4, 2, *bad) == -1, bad
    assert L.rfx_fx_loudness_ws(4, T, T // 64, hop, nhop, nblk) == 4 * nhop


def test_older_total_size_queries(L):
    """the total-size queries from before the rule, against tests/loss_ref.py, tests/fx_ref.py and the layouts their headers state"""
    from tests import fx_ref as FX
    for R, frames in itertools.product((-1, 0, 1, 3, 64), (-1, 0, 1, 2, 255, 513, 4040, 2 ** 20)):
        got = L.rfx_stft_scaled_loss_ws(R, frames)
        assert got == (4 * R * X.scaled_grid(frames) if R > 0 and frames > 0 else 0), (R, frames)
    for B, T in itertools.product((1, 3, 64, 65535), (1, 3, 4, 5, 31, 32, 33, 262144)):
        assert L.rfx_fx_phaser_ws_floats(B, T) == FX.phaser_ws_floats(B, T), (B, T)
        for Cin in (1, 2):
            assert L.rfx_fx_sox_reverb_ws_floats(B, Cin, T) == B * Cin * 2 * T, (B, Cin, T)      # one row of T per bank
    for n, nhop in itertools.product((1, 3, 64), (4, 59)):
        assert L.rfx_fx_normalize_ws_bytes(n, nhop) == n * nhop * 8 + 2 * n * 4, (n, nhop)         # hop sums, then lufs and gain
    for B, T in ((0, 5), (5, 0)):                                # no rows or no samples: nothing to hold
        assert L.rfx_fx_phaser_ws_floats(B, T) == 0 and L.rfx_fx_sox_reverb_ws_floats(B, 2, T) == 0
    wmax = L.rfx_wiener_max_window()
    for B, Cc, bins, frames, W in itertools.product((-1, 0, 1, 3), (0, 1, 2, 3), (0, 1, 16, 17, 2049), (0, 1, 299, 300, 301), (0, 1, 300, wmax, wmax + 1)):
        got = L.rfx_wiener_ws_floats(B, Cc, bins, frames, W)
        if B <= 0 or Cc not in (1, 2) or bins <= 0 or frames <= 0 or W <= 0 or W > wmax:
            assert got == -1, (B, Cc, bins, frames, W)
        else:                                                    # one float per (sample, window, 16 rows of (channel, bin))
            assert got == B * ceil_div(frames, W) * ceil_div(Cc * bins, 16), (B, Cc, bins, frames, W)


# ---- the header's rule ------------------------------------------------------------------------------------------------------------------
SCRATCH_PARAMS = ("ws", "work", "partial", "hop_ws", "env_ws")
# entry points whose scratch is sized otherwise, and how
SIZED_BY = {
    "rfx_gemm_wgrad": None,                                      # takes its capacity (ws_floats) and checks it
    "rfx_lstm_fwd": "rfx_lstm_ws_bytes", "rfx_lstm_bwd": "rfx_lstm_ws_bytes",
    # one query per geometry, shared by the entry points of a family
    "rfx_fft_synthesis_lossgrad": "rfx_fft_synthesis_ws",
    "rfx_groupnorm_bwd": "rfx_norm_bwd_work_floats", "rfx_groupnorm_bwd_x16": "rfx_norm_bwd_work_floats",
    "rfx_batchnorm_bwd": "rfx_norm_bwd_work_floats",
    "rfx_logcosh_rows": "rfx_logcosh_ws",
    "rfx_fx_normalize_rows": "rfx_fx_normalize_ws_bytes",
}


def _prototypes():
    text = open(os.path.join(ROOT, "include", "remfx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return text, {m.group(1): m.group(2) for m in re.finditer(r"\b(?:int|int64_t)\s+(rfx_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}


def test_header_declares_a_query_for_every_scratch_parameter():
    text, protos = _prototypes()
    assert set(protos) == set(_lib.SIGNATURES), set(protos) ^ set(_lib.SIGNATURES)
    found = 0
    for entry, params in protos.items():
        names = [re.split(r"[\s*]+", p.strip())[-1] for p in params.split(",")]
        mine = [(p, n) for p, n in zip(params.split(","), names) if n in SCRATCH_PARAMS and "const" not in p]
        if not mine:
            continue
        found += 1
        if entry in SIZED_BY:
            assert SIZED_BY[entry] is None or SIZED_BY[entry] in protos, entry
            continue
        queries = [q for q in protos if q == entry + "_ws" or q.startswith(entry + "_ws_")]
        assert queries, (entry, "takes", [n for _, n in mine], "and the header declares no", entry + "_ws")
        for q in queries:
            assert q in _lib._RET64, (q, "returns int64_t")
    assert found >= 25
    assert set(SIZED_BY) <= set(protos)
    for gone in ("RFX_SUMSQ_SLOTS", "RFX_L1_SLOTS", "RFX_STFT_REDUCE_SLOTS", "RFX_SISDR_SLOTS"):
        assert gone not in text, gone
    # a slot-count query stays only where a caller passes the count on (rfx_groupnorm_stat_chunks -> rfx_epilogue.stat_slots)
    assert not [q for q in protos if q.endswith("_slots")] and "rfx_dconv_layer_bwd_rows" not in protos


def test_every_query_returning_int64_is_declared_so():
    text, _ = _prototypes()
    for q in _lib._RET64:
        assert re.search(r"\bint64_t\s+" + q + r"\s*\(", text), q
    for m in re.finditer(r"\bint64_t\s+(rfx_\w+)\s*\(", text):
        assert m.group(1) in _lib._RET64, m.group(1)
