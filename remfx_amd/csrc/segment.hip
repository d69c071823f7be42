// Segmented long-file inference: cut (rows, T) into overlapping training-length clips and cross-fade the networks' outputs back
// into one signal (remfx_amd/segment.py).  The call site is the single-file path of the reference,
// scripts/remfx_detect.py:44-55, which hands the whole file to the chain as one clip.
//
// Plan (mirrored on the host, SegmentPlan): hop = L - overlap; S segments start at s_i = min(i * hop, max(T - L, 0)), i.e. segments
// 0 .. S-2 sit on the hop grid and the LAST one is tail-aligned (it ends at T) instead of zero-padded; only a file shorter than one
// segment is padded (S = 1).  A network returns Lp = L - lead - trail samples per clip, output sample j belonging to input sample
// j + lead, so in OUTPUT coordinates (t = input position - lead) clip i owns the window [s_i, s_i + Lp).
//
// Both kernels are copies at HBM rate: one wave per 256-sample chunk of one row, the (row, segment, chunk) decode is wave-uniform
// 32-bit arithmetic, lanes move 16 bytes when every base and length is a multiple of four samples and one dword otherwise.
#include "common.h"

struct SegArgs {
  const float* in; float* out;
  int32_t T;         // input samples per row
  int32_t L;         // split: segment length; merge: Lp, samples per clip the network returned
  int32_t hop, S;
  int32_t last;      // start of the tail-aligned last segment, max(T - L, 0)
  int32_t To;        // merge: output samples per row, T - lead - trail
  int32_t C;         // channels kept together in one clip (rfx_segment_split_c / _merge_c); 1: every row is a clip of its own
  uint32_t nitems, ipr;
};

// out[(r * S + i)][j] = x[r][s_i + j], zeros beyond T; with C channels per clip, row r = b * C + c: out[(b * S + i) * C + c][j]
template <bool VEC>
__global__ __launch_bounds__(256) void segment_split_kernel(const SegArgs a) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t w = blockIdx.x * 4u + wave;
  if (w >= a.nitems) return;
  const uint32_t rs = w / a.ipr, ck = w - rs * a.ipr;
  const uint32_t bi = rs / (uint32_t)a.C, c = rs - bi * (uint32_t)a.C;
  const uint32_t b = bi / (uint32_t)a.S, i = bi - b * (uint32_t)a.S;
  const int32_t hs = (int32_t)i * a.hop, s = hs < a.last ? hs : a.last;
  const float* xr = a.in + ((int64_t)b * a.C + c) * a.T + s;
  float* orow = a.out + (int64_t)rs * a.L;
  const int32_t left = a.T - s;                      // samples of the row from s on
  const int lane = threadIdx.x & 63;
  if (VEC) {
    const int32_t j = (int32_t)ck * 256 + lane * 4;
    if (j >= a.L) return;
    rfx_st4(orow + j, j < left ? rfx_ld4(xr + j) : f32x4{0.f, 0.f, 0.f, 0.f});     // T, s, j multiples of 4: all four in or out
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int32_t j = (int32_t)ck * 256 + q * 64 + lane;
      if (j < a.L) orow[j] = j < left ? xr[j] : 0.f;
    }
  }
}

// The clips covering output position t, from integer arithmetic on t: hop-grid clips i with i * hop <= t < i * hop + Lp, clipped to
// 0 .. S-2, and the tail-aligned clip S-1 when t >= last (it is the one clip off the grid; when it happens to sit on the grid it is
// still taken here and not in the range, so nothing is counted twice).  Terms are added in increasing i, the integer weights
// w[j] = min(j + 1, Lp - j) are exact in fp32, their sum is kept as an integer: one rounding per product, per add and for the divide.
__device__ __forceinline__ float segment_merge_one(const SegArgs& a, const float* __restrict__ yr, int64_t cs, int32_t t, int32_t ilo,
                                                   int32_t ihi) {
  float acc = 0.f;
  int32_t wsum = 0;
  for (int32_t i = ilo; i <= ihi; ++i) {
    const int32_t j = t - i * a.hop, wj = min(j + 1, a.L - j);
    acc += (float)wj * yr[i * cs + j];
    wsum += wj;
  }
  if (t >= a.last) {
    const int32_t j = t - a.last, wj = min(j + 1, a.L - j);
    acc += (float)wj * yr[(a.S - 1) * cs + j];
    wsum += wj;
  }
  return acc / (float)wsum;
}

// out[r][t] = sum_i w[t - s_i] y[r * S + i][t - s_i] / sum_i w[t - s_i]: every output sample is computed by one thread and stored
// exactly once (no atomics, no zero-filled target: DESIGN.md 4.11).  With C channels per clip, row r = b * C + c reads clip i at
// y[(b * S + i) * C + c]: the same sum with a clip pitch of C * Lp.
template <bool VEC>
__global__ __launch_bounds__(256) void segment_merge_kernel(const SegArgs a) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t w = blockIdx.x * 4u + wave;
  if (w >= a.nitems) return;
  const uint32_t r = w / a.ipr, ck = w - r * a.ipr;
  const uint32_t b = r / (uint32_t)a.C, c = r - b * (uint32_t)a.C;
  const int64_t cs = (int64_t)a.C * a.L;                         // pitch between two clips of one row
  const float* yr = a.in + ((int64_t)b * a.S * a.C + c) * a.L;
  float* orow = a.out + (int64_t)r * a.To;
  const int lane = threadIdx.x & 63;
  if (VEC) {
    const int32_t t = (int32_t)ck * 256 + lane * 4;
    if (t >= a.To) return;
    // hop, Lp, last and t are multiples of 4: the four samples share their covering clips
    const int32_t ihi = min((int32_t)((uint32_t)t / (uint32_t)a.hop), a.S - 2);
    const int32_t ilo = t < a.L ? 0 : (int32_t)((uint32_t)(t - a.L) / (uint32_t)a.hop) + 1;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int32_t ws[4] = {0, 0, 0, 0};
    for (int32_t i = ilo; i <= ihi; ++i) {
      const int32_t j = t - i * a.hop;
      const f32x4 v = rfx_ld4(yr + i * cs + j);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int32_t wj = min(j + c + 1, a.L - j - c);
        acc[c] += (float)wj * v[c];
        ws[c] += wj;
      }
    }
    if (t >= a.last) {
      const int32_t j = t - a.last;
      const f32x4 v = rfx_ld4(yr + (a.S - 1) * cs + j);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int32_t wj = min(j + c + 1, a.L - j - c);
        acc[c] += (float)wj * v[c];
        ws[c] += wj;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = acc[c] / (float)ws[c];
    rfx_st4(orow + t, acc);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int32_t t = (int32_t)ck * 256 + q * 64 + lane;
      if (t < a.To) {
        const int32_t ihi = min((int32_t)((uint32_t)t / (uint32_t)a.hop), a.S - 2);
        const int32_t ilo = t < a.L ? 0 : (int32_t)((uint32_t)(t - a.L) / (uint32_t)a.hop) + 1;
        orow[t] = segment_merge_one(a, yr, cs, t, ilo, ihi);
      }
    }
  }
}

// number of segments of the plan, 0 when the geometry is refused.  Lengths stay below 2^30 so that every index above fits 32 bits.
static int32_t segment_count(int64_t T, int32_t L, int32_t hop) {
  if (T <= 0 || T >= (1LL << 30) || L <= 0 || L >= (1 << 30) || hop <= 0 || hop > L) return 0;
  if (T <= L) return 1;
  return (int32_t)((T - L + hop - 1) / hop) + 1;
}

static int segment_split(const float* x, float* out, int32_t rows, int32_t C, int64_t T, int32_t L, int32_t hop, int32_t S, void* stream) {
  if (!x || !out || rows <= 0 || C <= 0 || rows % C) return -1;
  if (segment_count(T, L, hop) != S || S <= 0) return -1;          // the caller sized `out` by its own S: they must agree
  const int64_t per = ((int64_t)L + 255) / 256, items = (int64_t)rows * S * per;
  if (items > 0x7fffffffLL) return -1;
  SegArgs a;
  a.in = x; a.out = out; a.T = (int32_t)T; a.L = L; a.hop = hop; a.S = S;
  a.last = T > L ? (int32_t)(T - L) : 0; a.To = 0; a.C = C;
  a.nitems = (uint32_t)items; a.ipr = (uint32_t)per;
  const bool vec = !((T | L | hop) & 3) && !((uintptr_t)x & 15) && !((uintptr_t)out & 15);     // last = T - L follows
  const dim3 grid((a.nitems + 3) / 4);
  if (vec) hipLaunchKernelGGL((segment_split_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((segment_split_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, a);
  RFX_CHECK_LAUNCH();
  return 0;
}

extern "C" int rfx_segment_split(const float* x, float* out, int32_t rows, int64_t T, int32_t L, int32_t hop, int32_t S, void* stream) {
  return segment_split(x, out, rows, 1, T, L, hop, S, stream);
}
// (B, C, T) -> clips (B * S, C, L), ordered [b][segment][channel]: the clips of a network that takes multi-channel input
extern "C" int rfx_segment_split_c(const float* x, float* out, int32_t B, int32_t C, int64_t T, int32_t L, int32_t hop, int32_t S,
                                   void* stream) {
  if (B <= 0 || C <= 0 || (int64_t)B * C > 0x7fffffffLL) return -1;
  return segment_split(x, out, B * C, C, T, L, hop, S, stream);
}

static int segment_merge(const float* y, float* out, int32_t rows, int32_t C, int64_t T, int32_t L, int32_t hop, int32_t lead,
                         int32_t trail, int32_t S, void* stream) {
  if (!y || !out || rows <= 0 || C <= 0 || rows % C || lead < 0 || trail < 0) return -1;
  if (segment_count(T, L, hop) != S || S <= 0) return -1;
  if ((int64_t)lead + trail > (int64_t)L - hop) return -1;          // valid windows must abut: lead + trail <= overlap
  const int64_t To = T - lead - trail;
  if (To < 1) return -1;
  const int32_t Lp = L - lead - trail;                              // >= hop >= 1
  const int64_t per = (To + 255) / 256, items = (int64_t)rows * per;
  if (items > 0x7fffffffLL) return -1;
  SegArgs a;
  a.in = y; a.out = out; a.T = (int32_t)T; a.L = Lp; a.hop = hop; a.S = S;
  a.last = T > L ? (int32_t)(T - L) : 0; a.To = (int32_t)To; a.C = C;
  a.nitems = (uint32_t)items; a.ipr = (uint32_t)per;
  const bool vec = !((To | Lp | hop | a.last) & 3) && !((uintptr_t)y & 15) && !((uintptr_t)out & 15);
  const dim3 grid((a.nitems + 3) / 4);
  if (vec) hipLaunchKernelGGL((segment_merge_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((segment_merge_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, a);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_segment_merge(const float* y, float* out, int32_t rows, int64_t T, int32_t L, int32_t hop, int32_t lead,
                                 int32_t trail, int32_t S, void* stream) {
  return segment_merge(y, out, rows, 1, T, L, hop, lead, trail, S, stream);
}
// clips (B * S, Co, Lp), ordered [b][segment][channel] -> (B, Co, T - lead - trail); Co is the network's output channel count
extern "C" int rfx_segment_merge_c(const float* y, float* out, int32_t B, int32_t Co, int64_t T, int32_t L, int32_t hop, int32_t lead,
                                   int32_t trail, int32_t S, void* stream) {
  if (B <= 0 || Co <= 0 || (int64_t)B * Co > 0x7fffffffLL) return -1;
  return segment_merge(y, out, B * Co, Co, T, L, hop, lead, trail, S, stream);
}
