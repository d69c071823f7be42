// Generic framed real FFT: STFT / iSTFT forward and backward for n_fft = 2^k, k = 4 .. 15, except the four lengths csrc/fft.hip
// owns (512 / 1024 / 2048 / 4096: register passes built on NC = RA * 16 * 16, which no other length fits).  Same descriptor, same
// semantics: every rfx_stft_desc field the kernels of fft.hip honour is honoured here (mode, bins, frame0, frames_out, extra pads,
// in_mode / in_offset / mul, herm, scale, accum, a `win`-sample window centred in n_fft).
//
// Structure:
//   * a real n_fft-point transform is the NC = n_fft / 2 point complex FFT of z[n] = x[2n] + i x[2n+1] plus the split / merge step;
//   * one workgroup = 256 threads = FB frames, FB = max(1, 2048 / n_fft):
//         n_fft   16   32   64  128  256 | 8192 16384 32768
//         FB     128   64   32   16    8 |    1     1     1
//     The frames live in dynamic LDS for the whole transform (FB * NC complex values: 8 KiB up to n_fft 256, then 32 / 64 / 128 KiB;
//     the 128 KiB of n_fft = 32768 leave room for one workgroup per CU);
//   * the FFT is decimation in frequency, in place: one radix-2 stage first when log2 NC is odd, then radix-4 stages of span
//     L = 4^j down to 4.  A stage of span L reads x[base + m L/4], m = 0..3, and writes the butterfly's outputs times W_L^(q m)
//     back to the same four places, so no second buffer is needed (there is none to have at 128 KiB).  Output bin k ends at the
//     digit-reversed position pos_of(k);
//   * twiddles come from a table the host computes in double precision, one per (n_fft, device): [NC] W_NC^t | [NC] e^{-i pi k / NC};
//   * LDS layout.  ds_read_b64 banks are (byte address / 4) % 64 per 32-lane half, i.e. 32 eight-byte slots.  With lane = butterfly
//     index, a stage of quarter span s = L/4 >= 32 reads 32 consecutive values (conflict-free as stored); the last three stages
//     (s = 16, 4, 1) read at strides of 64, 16 and 4 values and would put a half-wave on 16, 4 or 8 ... 1 slot(s).  So value i of a
//     frame is stored at i ^ swz(i), where swz folds address bits 5 and 6 into the slot bits:
//         slot0 ^= a5, slot1 ^= a6, slot2 ^= a5, slot3 ^= a6, slot4 ^= a6        (xor with 5 * a5 ^ 26 * a6)
//     The lanes of a half-wave differ in address bits {0..4} (s >= 32), {0..3, 6} (s = 16), {0, 1, 4, 5, 6} (s = 4) and {2..6} (s = 1,
//     and the radix-2 stage is first, where s = NC / 2); on each of these sets the map to the five slot bits is one-to-one, so every
//     stage read is conflict-free (writes, banked % 32 dwords, are at most 2-way).  The split step reads bin k at the digit-reversed
//     pos_of(k), whose low bits come from the HIGH bits of k: for NC >= 512 the top digit of the position (= the low two bits of k) is
//     folded into slot bits 3..4 as well, and the lanes of the epilogue take k in runs of four (32-byte stores) whose other lane bits
//     are the top two digits of k (= position bits 0..3): one-to-one again for even log2 NC, 2-way for odd (n_fft = 16384).
//     Frames of the small sizes are NC + 1 values apart, so lanes that run along frames fall on different slots;
//   * the inverse transform is the same forward code on conjugated data (the merge step writes conj Z, the store reads conj z);
//   * synthesis is two launches BY OWNERSHIP: (1) per frame merge -> inverse FFT -> window -> scratch [R][frames_out][n_fft];
//     (2) one thread per output sample adds, in a fixed order, every frame that covers every padded position that maps to the sample
//     (the position itself; in_mode 0: its mirror images under the reflect padding; in_mode 1: the offset position times `mul`),
//     applies `scale` and stores once (accum: adds once).  No atomics, no zero fill, no waits on other workgroups: bit-reproducible.
#include "fft_any.h"
#include "common.h"
#include <climits>
#include <math.h>
#include <mutex>

typedef float v2f __attribute__((ext_vector_type(2)));

struct AnyArgs {
  rfx_stft_desc d;
  const float* x;        // analysis: signal [R][T];  synthesis: spectrum
  const float* window;   // [win]
  const float* mul;      // optional multiplier per padded sample (iSTFT 1 / envelope)
  float* out;            // analysis: spectrum;  synthesis: signal [R][T]
  const v2f* tables;     // [NC] W_NC^t | [NC] e^{-i pi k / NC}
  float* ws;             // synthesis: windowed frames [R][frames_out][n_fft]
  int batches;           // frame batches (FB frames each) per row
};

template <int LOGNC>
struct AnyCfg {
  static constexpr int NC = 1 << LOGNC, N = 2 * NC;
  static constexpr int FB = N >= 2048 ? 1 : 2048 / N;
  static constexpr int FS = FB > 1 ? NC + 1 : NC;              // frame stride in values
  static constexpr int LDS = FB * FS * (int)sizeof(v2f);
};

__device__ __forceinline__ v2f any_cmul(v2f a, v2f b) { return a.xx * b + a.yy * v2f{-b.y, b.x}; }
__device__ __forceinline__ v2f any_conj(v2f a) { return v2f{a.x, -a.y}; }
__device__ __forceinline__ v2f any_negi(v2f a) { return v2f{a.y, -a.x}; }

// LDS place of value i of a frame (file header)
template <int LOGNC> __device__ __forceinline__ int any_swz(int i) {
  if (LOGNC >= 7) i ^= (((i >> 5) & 1) * 5) ^ (((i >> 6) & 1) * 26);
  if (LOGNC >= 9) i ^= ((i >> (LOGNC - 2)) & 3) << 3;
  return i;
}
// where output k of the in-place decimation-in-frequency FFT ends: the digits of k (radix 2 first when LOGNC is odd, then radix 4) reversed
template <int LOGNC> __device__ __forceinline__ int any_pos_of(int k) {
  int pos = 0, rem = LOGNC;
  if (LOGNC & 1) { pos |= (k & 1) << (rem - 1); k >>= 1; rem -= 1; }
#pragma unroll
  for (; rem > 0; rem -= 2) { pos |= (k & 3) << (rem - 2); k >>= 2; }
  return pos;
}
// epilogue item r -> bin (or time pair) index: runs of four, then the top two digits (position bits 0..3), then the rest
template <int LOGNC> __device__ __forceinline__ int any_item_k(int r) {
  if (LOGNC < 9) return r;
  return (r & 3) | (((r >> 2) & 3) << (LOGNC - 2)) | (((r >> 4) & 3) << (LOGNC - 4)) | ((r >> 6) << 2);
}

// padded-signal coordinate p -> sample index of the row (or -1): centre + reflect on top of an optional extra reflect pad, or an offset
__device__ __forceinline__ int64_t any_map(const rfx_stft_desc& d, int64_t p) {
  if (d.in_mode == 0) {
    const int64_t Tp = (int64_t)d.T + d.extra_pad_l + d.extra_pad_r;
    int64_t s = p - d.n_fft / 2;
    if (s < 0) s = -s;
    if (s >= Tp) s = 2 * (Tp - 1) - s;
    s -= d.extra_pad_l;
    if (s < 0) s = -s;
    if (s >= d.T) s = 2 * ((int64_t)d.T - 1) - s;
    return (s >= 0 && s < d.T) ? s : -1;
  }
  const int64_t s = p - d.in_offset;
  return (s >= 0 && s < d.T) ? s : -1;
}
// the padded signal of a row at position p (zero where nothing maps), times the optional multiplier
__device__ __forceinline__ float any_sample(const AnyArgs& a, const float* xr, int64_t p) {
  const int64_t s = any_map(a.d, p);
  if (s < 0) return 0.f;
  float v = xr[s];
  if (a.mul) v *= a.mul[p];
  return v;
}

// forward FFT of the FB frames in LDS, in place; ends with a barrier
template <int LOGNC>
__device__ __forceinline__ void any_fft(v2f* lds, const v2f* __restrict__ tw) {
  typedef AnyCfg<LOGNC> K;
  constexpr int NC = K::NC;
  const int tid = threadIdx.x;
  if (LOGNC & 1) {
    constexpr int H = NC / 2;
    for (int idx = tid; idx < K::FB * H; idx += 256) {
      const int fl = idx >> (LOGNC - 1), q = idx & (H - 1);
      v2f* fr = lds + fl * K::FS;
      const int i0 = any_swz<LOGNC>(q), i1 = any_swz<LOGNC>(q + H);
      const v2f x0 = fr[i0], x1 = fr[i1];
      fr[i0] = x0 + x1;
      fr[i1] = any_cmul(x0 - x1, tw[q]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int lg = LOGNC & ~1; lg >= 2; lg -= 2) {                 // span L = 2^lg, quarter span s, twiddle step NC / L
    const int s = 1 << (lg - 2), ts = LOGNC - lg;
    for (int idx = tid; idx < K::FB * (NC / 4); idx += 256) {
      const int fl = idx >> (LOGNC - 2), j = idx & (NC / 4 - 1);
      const int q = j & (s - 1), base = ((j >> (lg - 2)) << lg) + q;
      v2f* fr = lds + fl * K::FS;
      const int i0 = any_swz<LOGNC>(base), i1 = any_swz<LOGNC>(base + s), i2 = any_swz<LOGNC>(base + 2 * s),
                i3 = any_swz<LOGNC>(base + 3 * s);
      const v2f x0 = fr[i0], x1 = fr[i1], x2 = fr[i2], x3 = fr[i3];
      const v2f t0 = x0 + x2, t1 = x0 - x2, t2 = x1 + x3, t3 = any_negi(x1 - x3);
      v2f y0 = t0 + t2, y1 = t1 + t3, y2 = t0 - t2, y3 = t1 - t3;
      if (lg > 2) {
        const int t = q << ts;                                    // 3 t < NC
        y1 = any_cmul(y1, tw[t]);
        y2 = any_cmul(y2, tw[2 * t]);
        y3 = any_cmul(y3, tw[3 * t]);
      }
      fr[i0] = y0; fr[i1] = y1; fr[i2] = y2; fr[i3] = y3;
    }
    __syncthreads();
  }
}

// one spectrum value of the analysis: every output mode
__device__ __forceinline__ void any_store_bin(const AnyArgs& a, int row, int fo, int k, v2f X) {
  const rfx_stft_desc& d = a.d;
  if (k >= d.bins) return;
  if (d.herm) {                                                   // gradient of irfft: middle bins doubled, DC / Nyquist imaginary part dropped
    if (k == 0 || k == d.n_fft / 2) X.y = 0.f;
    else X = X * 2.f;
  }
  const int64_t FO = d.frames_out;
  const int64_t rb = (int64_t)row * d.bins + k;
  switch (d.mode) {
    case RFX_STFT_COMPLEX_FM:
      reinterpret_cast<v2f*>(a.out)[((int64_t)row * FO + fo) * d.bins + k] = X;
      break;
    case RFX_STFT_COMPLEX:
      reinterpret_cast<v2f*>(a.out)[rb * FO + fo] = X;
      break;
    case RFX_STFT_CAC:
      a.out[((int64_t)row * 2 * d.bins + k) * FO + fo] = X.x;
      a.out[((int64_t)row * 2 * d.bins + d.bins + k) * FO + fo] = X.y;
      break;
    case RFX_STFT_MAG:
      a.out[rb * FO + fo] = sqrtf(fmaxf(X.x * X.x + X.y * X.y, d.eps));
      break;
    case RFX_STFT_POW:
      a.out[rb * FO + fo] = X.x * X.x + X.y * X.y;
      break;
    default:  // RFX_STFT_MAGPOW
      a.out[rb * FO + fo] = powf(sqrtf(X.x * X.x + X.y * X.y) + d.eps, d.alpha);
      break;
  }
}
// one spectrum value of the synthesis, as the merge step wants it: missing bins are zero, DC / Nyquist are real, and the adjoint of
// the one-sided transform (herm 0) halves the middle bins
__device__ __forceinline__ v2f any_load_bin(const AnyArgs& a, int row, int fo, int k) {
  const rfx_stft_desc& d = a.d;
  if (k >= d.bins) return v2f{0.f, 0.f};
  const int64_t FO = d.frames_out;
  v2f v;
  if (d.mode == RFX_STFT_COMPLEX_FM) v = reinterpret_cast<const v2f*>(a.x)[((int64_t)row * FO + fo) * d.bins + k];
  else if (d.mode == RFX_STFT_COMPLEX) v = reinterpret_cast<const v2f*>(a.x)[((int64_t)row * d.bins + k) * FO + fo];
  else {
    v.x = a.x[((int64_t)row * 2 * d.bins + k) * FO + fo];
    v.y = a.x[((int64_t)row * 2 * d.bins + d.bins + k) * FO + fo];
  }
  if (k == 0 || k == d.n_fft / 2) v.y = 0.f;
  else if (!d.herm) v = v * 0.5f;
  return v;
}

template <int LOGNC>
__global__ __launch_bounds__(256) void fft_any_analysis_kernel(const AnyArgs a) {
  typedef AnyCfg<LOGNC> K;
  constexpr int NC = K::NC, N = K::N, FB = K::FB;
  extern __shared__ v2f any_lds[];
  const rfx_stft_desc& d = a.d;
  const int tid = threadIdx.x;
  const int row = blockIdx.x / a.batches, fb0 = d.frame0 + (blockIdx.x - row * a.batches) * FB;
  const int f_end = d.frame0 + d.frames_out;
  const float* xr = a.x + (int64_t)row * d.T;
  const v2f* twH = a.tables + NC;
  const int woff = (N - d.win) / 2;
  for (int idx = tid; idx < FB * NC; idx += 256) {
    const int fl = idx >> LOGNC, i = idx & (NC - 1), f = fb0 + fl;
    v2f z = v2f{0.f, 0.f};
    if (f < f_end) {
      const int64_t p = (int64_t)f * d.hop + 2 * i;
      const int w0 = 2 * i - woff, w1 = w0 + 1;
      if (w0 >= 0 && w0 < d.win) z.x = any_sample(a, xr, p) * (a.window[w0] * d.scale);
      if (w1 >= 0 && w1 < d.win) z.y = any_sample(a, xr, p + 1) * (a.window[w1] * d.scale);
    }
    any_lds[fl * K::FS + any_swz<LOGNC>(i)] = z;
  }
  __syncthreads();
  any_fft<LOGNC>(any_lds, a.tables);
  // split step, one bin per item (bin NC rides with bin 0):  E = (A + conj B) / 2, P = (A - conj B) / 2 * e^{-i pi k / NC},
  //   X[k] = E - i P,  X[NC] = conj E - i conj P at k = 0.   A = Z[k], B = Z[NC - k]
  const bool along_frames = FB > 1 && d.mode != RFX_STFT_COMPLEX_FM;     // [bin][frame] outputs: lanes along frames
  for (int idx = tid; idx < FB * NC; idx += 256) {
    int fl, k;
    if (along_frames) { fl = idx & (FB - 1); k = idx / FB; }
    else { fl = idx >> LOGNC; k = any_item_k<LOGNC>(idx & (NC - 1)); }
    const int f = fb0 + fl;
    if (f >= f_end) continue;
    const v2f* fr = any_lds + fl * K::FS;
    const v2f A = fr[any_swz<LOGNC>(any_pos_of<LOGNC>(k))];
    const v2f B = any_conj(fr[any_swz<LOGNC>(any_pos_of<LOGNC>((NC - k) & (NC - 1)))]);
    const v2f E = (A + B) * 0.5f, D = (A - B) * 0.5f;
    const v2f P = any_cmul(D, twH[k]);
    any_store_bin(a, row, f - d.frame0, k, v2f{E.x + P.y, E.y - P.x});
    if (k == 0) any_store_bin(a, row, f - d.frame0, NC, v2f{E.x - P.y, -E.y - P.x});
  }
}

// synthesis, launch 1: merge -> inverse FFT -> window -> frame scratch
template <int LOGNC>
__global__ __launch_bounds__(256) void fft_any_frames_kernel(const AnyArgs a) {
  typedef AnyCfg<LOGNC> K;
  constexpr int NC = K::NC, N = K::N, FB = K::FB;
  extern __shared__ v2f any_lds[];
  const rfx_stft_desc& d = a.d;
  const int tid = threadIdx.x;
  const int row = blockIdx.x / a.batches, fb0 = d.frame0 + (blockIdx.x - row * a.batches) * FB;
  const int f_end = d.frame0 + d.frames_out;
  const v2f* twH = a.tables + NC;
  const int woff = (N - d.win) / 2;
  // merge step: S = Y[k] + conj Y[NC-k], W = (Y[k] - conj Y[NC-k]) e^{+i pi k / NC}, Z[k] = S + i W; conj Z is stored in natural order
  for (int idx = tid; idx < FB * NC; idx += 256) {
    const int fl = idx >> LOGNC, k = idx & (NC - 1), f = fb0 + fl;
    v2f Z = v2f{0.f, 0.f};
    if (f < f_end) {
      const v2f yk = any_load_bin(a, row, f - d.frame0, k), ym = any_conj(any_load_bin(a, row, f - d.frame0, NC - k));
      const v2f S = yk + ym, D = yk - ym;
      const v2f W = any_cmul(D, any_conj(twH[k]));
      Z = v2f{S.x - W.y, -(S.y + W.x)};
    }
    any_lds[fl * K::FS + any_swz<LOGNC>(k)] = Z;
  }
  __syncthreads();
  any_fft<LOGNC>(any_lds, a.tables);
  for (int idx = tid; idx < FB * NC; idx += 256) {
    const int fl = idx >> LOGNC, n = any_item_k<LOGNC>(idx & (NC - 1)), f = fb0 + fl;
    if (f >= f_end) continue;
    const v2f z = any_lds[fl * K::FS + any_swz<LOGNC>(any_pos_of<LOGNC>(n))];
    const int w0 = 2 * n - woff, w1 = w0 + 1;
    const float g0 = (w0 >= 0 && w0 < d.win) ? a.window[w0] : 0.f, g1 = (w1 >= 0 && w1 < d.win) ? a.window[w1] : 0.f;
    reinterpret_cast<v2f*>(a.ws + ((int64_t)row * d.frames_out + (f - d.frame0)) * N)[n] = v2f{z.x * g0, -z.y * g1};
  }
}

// synthesis, launch 2: one thread per output sample
__global__ __launch_bounds__(256) void fft_any_gather_kernel(const AnyArgs a) {
  const rfx_stft_desc& d = a.d;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)d.R * d.T) return;
  const int row = (int)(idx / d.T);
  const int64_t s = idx - (int64_t)row * d.T;
  const int N = d.n_fft, woff = (N - d.win) / 2, f_end = d.frame0 + d.frames_out;
  const float* wr = a.ws + (int64_t)row * d.frames_out * N;
  // the overlap-added value of padded position p: its covering frames in ascending order, then scale, then the multiplier
  auto at = [&](int64_t p) -> float {
    const int64_t qw = p - woff;
    if (qw < 0) return 0.f;
    const int64_t lo_num = qw - d.win + 1;
    int64_t f_hi = qw / d.hop, f_lo = lo_num > 0 ? (lo_num + d.hop - 1) / d.hop : 0;
    if (f_hi > f_end - 1) f_hi = f_end - 1;
    if (f_lo < d.frame0) f_lo = d.frame0;
    if (f_lo > f_hi) return 0.f;
    float v = 0.f;
    for (int64_t f = f_lo; f <= f_hi; ++f) v += wr[(f - d.frame0) * N + (p - f * d.hop)];
    v *= d.scale;
    if (a.mul) v *= a.mul[p];
    return v;
  };
  float acc = 0.f;
  if (d.in_mode == 1) {
    const int64_t p = s + d.in_offset;
    if (p >= 0) acc = at(p);
  } else {
    // adjoint of the padding: every padded position any_map sends to s.  Each of the two reflections x -> (x, -x, 2 (len - 1) - x,
    // x - 2 (len - 1)) lists all its preimages, so the 16 combinations hold every candidate; any_map decides, duplicates count once.
    const int64_t Tp = (int64_t)d.T + d.extra_pad_l + d.extra_pad_r, m2 = 2 * ((int64_t)d.T - 1), m1 = 2 * (Tp - 1);
    auto cand = [&](int c) -> int64_t {
      const int c2 = c >> 2, c1 = c & 3;
      const int64_t s2 = c2 == 0 ? s : c2 == 1 ? -s : c2 == 2 ? m2 - s : s - m2;
      const int64_t r1 = s2 + d.extra_pad_l;
      const int64_t s1 = c1 == 0 ? r1 : c1 == 1 ? -r1 : c1 == 2 ? m1 - r1 : r1 - m1;
      return s1 + N / 2;
    };
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int64_t p = cand(c);
      bool ok = p >= 0 && any_map(d, p) == s;
#pragma unroll
      for (int j = 0; j < c; ++j) ok = ok && cand(j) != p;
      if (ok) acc += at(p);
    }
  }
  float* o = a.out + idx;
  *o = d.accum ? *o + acc : acc;
}

static int any_lognc(int n_fft) {
  for (int k = 4; k <= 15; ++k)
    if (n_fft == (1 << k)) return k - 1;
  return -1;
}
bool fft_any_covers(const rfx_stft_desc* d) {
  if (!d) return false;
  const int n = d->n_fft;
  return any_lognc(n) >= 0 && n != 512 && n != 1024 && n != 2048 && n != 4096;
}
static bool any_desc_ok(const rfx_stft_desc* d) {
  if (!fft_any_covers(d)) return false;
  const int n = d->n_fft;
  return d->R > 0 && d->T > 0 && d->hop > 0 && d->win > 0 && d->win <= n && d->frames_out > 0 && d->bins > 0 && d->bins <= n / 2 + 1 &&
         d->frame0 >= 0;
}
int64_t fft_any_synthesis_ws(const rfx_stft_desc* d) {
  if (!any_desc_ok(d)) return -1;
  return (int64_t)d->R * d->frames_out * d->n_fft;
}

// twiddle tables of one n_fft on the current device: [NC] W_NC^t | [NC] e^{-i pi k / NC}
static const v2f* any_tables(int lognc) {
  static std::mutex mu;
  static v2f* tab[16][16] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16 || lognc < 0 || lognc >= 16) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  if (tab[dev][lognc]) return tab[dev][lognc];
  const int nc = 1 << lognc;
  float* h = new float[4 * nc];
  const double pi = 3.14159265358979323846;
  for (int t = 0; t < nc; ++t) {
    h[2 * t] = (float)cos(-2.0 * pi * t / (double)nc);
    h[2 * t + 1] = (float)sin(-2.0 * pi * t / (double)nc);
    h[2 * (nc + t)] = (float)cos(-pi * t / (double)nc);
    h[2 * (nc + t) + 1] = (float)sin(-pi * t / (double)nc);
  }
  v2f* p = nullptr;
  if (hipMalloc(&p, sizeof(float) * 4 * nc) == hipSuccess && hipMemcpy(p, h, sizeof(float) * 4 * nc, hipMemcpyHostToDevice) == hipSuccess)
    tab[dev][lognc] = p;
  else if (p) { (void)hipFree(p); p = nullptr; }
  delete[] h;
  return tab[dev][lognc];
}

template <int LOGNC, bool SYN>
static int any_launch1(const AnyArgs& a, unsigned grid, hipStream_t s) {
  constexpr int lds = AnyCfg<LOGNC>::LDS;
  static_assert(lds <= 160 * 1024, "");
  static bool attr = false;
  const void* k = SYN ? reinterpret_cast<const void*>(&fft_any_frames_kernel<LOGNC>) : reinterpret_cast<const void*>(&fft_any_analysis_kernel<LOGNC>);
  if (!attr) {
    if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return -3;
    attr = true;
  }
  if (SYN) hipLaunchKernelGGL(fft_any_frames_kernel<LOGNC>, dim3(grid), dim3(256), lds, s, a);
  else hipLaunchKernelGGL(fft_any_analysis_kernel<LOGNC>, dim3(grid), dim3(256), lds, s, a);
  RFX_CHECK_LAUNCH();
  return 0;
}

template <bool SYN>
static int any_launch(const rfx_stft_desc* d, const float* x, const float* window, const float* mul, float* ws, float* out, void* stream) {
  if (!any_desc_ok(d) || !x || !window || !out || (SYN && !ws)) return -1;
  const int lognc = any_lognc(d->n_fft);
  AnyArgs a;
  a.d = *d; a.x = x; a.window = window; a.mul = mul; a.out = out; a.ws = ws;
  a.tables = any_tables(lognc);
  if (!a.tables) return -3;
  const int fb = d->n_fft >= 2048 ? 1 : 2048 / d->n_fft;
  a.batches = (d->frames_out + fb - 1) / fb;
  const int64_t grid = (int64_t)a.batches * d->R;
  if (grid > INT_MAX) return -1;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  switch (lognc) {
    case 3: rc = any_launch1<3, SYN>(a, (unsigned)grid, s); break;
    case 4: rc = any_launch1<4, SYN>(a, (unsigned)grid, s); break;
    case 5: rc = any_launch1<5, SYN>(a, (unsigned)grid, s); break;
    case 6: rc = any_launch1<6, SYN>(a, (unsigned)grid, s); break;
    case 7: rc = any_launch1<7, SYN>(a, (unsigned)grid, s); break;
    case 12: rc = any_launch1<12, SYN>(a, (unsigned)grid, s); break;
    case 13: rc = any_launch1<13, SYN>(a, (unsigned)grid, s); break;
    case 14: rc = any_launch1<14, SYN>(a, (unsigned)grid, s); break;
    default: return -1;
  }
  if (rc != 0 || !SYN) return rc;
  const int64_t blocks = ((int64_t)d->R * d->T + 255) / 256;
  if (blocks > INT_MAX) return -1;
  hipLaunchKernelGGL(fft_any_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
  RFX_CHECK_LAUNCH();
  return 0;
}

int fft_any_analysis(const rfx_stft_desc* d, const float* x, const float* window, const float* mul, float* out, void* stream) {
  return any_launch<false>(d, x, window, mul, nullptr, out, stream);
}
int fft_any_synthesis(const rfx_stft_desc* d, const float* spec, const float* window, const float* mul, float* ws, float* out,
                      void* stream) {
  if (d && d->mode != RFX_STFT_COMPLEX && d->mode != RFX_STFT_CAC && d->mode != RFX_STFT_COMPLEX_FM) return -1;
  return any_launch<true>(d, spec, window, mul, ws, out, stream);
}
