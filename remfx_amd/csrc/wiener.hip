// Open-Unmix's multichannel Wiener filter refined by expectation-maximisation (open-unmix-pytorch `filtering.wiener` +
// `expectation_maximization`, called from `Separator.forward` once per sample and per window of `wiener_win_len` frames): DESIGN.md 4.27.
//
// Upstream runs a Python loop of dozens of small torch ops per window, sample and iteration over the (frames, bins, channels, 2,
// sources) estimate.  Everything but one scalar per window -- the scale m -- is independent per frequency bin, and a window of one bin
// fits on chip, so here ONE workgroup owns one (sample, window, bin): as many whole waves as the longest window has frames, four at
// the most (the kernel is bound by instruction issue, VALU and LDS together, not by latency: with a fifth wave for the 257th frame of
// a 262144-sample clip it ran 1.37 times as long as with four waves of which the first makes a second trip -- DESIGN.md 4.27):
//   * lanes run along the frames (contiguous for a fixed bin: coalesced 8-byte loads and stores); thread t owns frames t, t + 256, ...;
//   * x and every y_j of the window live in LDS from the initial estimate to the final store -- HBM sees S and X read once (X once more by the
//     small scale launch below) and Y written once, whatever niter is;
//   * the frame sums of R_j and its weight are wave butterflies, the waves' partials added in wave order;
//   * a thread only ever touches its own frames in LDS, so the only exchanges are the R_j partials (two barriers per iteration).
// The scale m = max(1, max |X| / 10) over a window's channels, bins and frames is an exact maximum: a first small launch stores
// max |X|^2 of 16 (channel, bin) rows into its own slot of the workspace, and every workgroup of the main launch takes the maximum of
// its window's slots -- no zero fill, no atomics, and a maximum does not depend on the order anyway.
#include "common.h"

constexpr int WN_THREADS = 256;                    // the scale launch
constexpr int WN_MAXT = 256, WN_MAXWAVES = 4;      // the main launch: whole waves, one thread per frame up to 256
constexpr int WN_MAXJ = 8;
constexpr int WN_MAXW = 448;                       // (8 * 2 + 2) rows * 448 frames * 8 B = 64512 B of LDS + 784 B of partials <= 64 KiB
constexpr int WN_ROWS = 16;                        // (channel, bin) rows per slot of the scale launch
constexpr float WN_EPS = 1e-10f;
constexpr float WN_SQRT_EPS = 1e-5f;

__device__ __forceinline__ float wn_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

static int wn_windows(int frames, int W) { return (frames + W - 1) / W; }
static int wn_slots(int C, int bins) { return (C * bins + WN_ROWS - 1) / WN_ROWS; }

// ws[(b * nwin + w) * nslots + s] = max |X|^2 over rows [16 s, 16 s + 16) of sample b's (channel, bin) rows and the frames of window w
__global__ __launch_bounds__(WN_THREADS) void wiener_scale_kernel(const float* __restrict__ X, int rows, int frames, int W, int nwin,
                                                                  int nslots, float* __restrict__ ws) {
  __shared__ float part[4];
  const int s = blockIdx.x % nslots, bw = blockIdx.x / nslots;
  const int w = bw % nwin, b = bw / nwin;
  const int t0 = w * W, n = min(W, frames - t0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float h = 0.f;
  for (int q = wave; q < WN_ROWS; q += 4) {
    const int r = s * WN_ROWS + q;
    if (r >= rows) break;
    const float* p = X + (((int64_t)b * rows + r) * frames + t0) * 2;
    for (int t = lane; t < n; t += 64) h = fmaxf(h, rfx_pow2(p[2 * t], p[2 * t + 1]));
  }
  h = wn_wave_max(h);
  if (lane == 0) part[wave] = h;
  __syncthreads();
  if (threadIdx.x == 0) ws[(int64_t)bw * nslots + s] = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

// cos / sin of atan2(im, re): x / |x| formed on the operand scaled by its larger component (no overflow or underflow of the square);
// x = 0 takes (1, 0) as atan2(0, 0) = 0 does
__device__ __forceinline__ void wn_phase(float re, float im, float& c, float& s) {
  const float e = fmaxf(fabsf(re), fabsf(im));
  if (!(e > 0.f)) { c = 1.f; s = 0.f; return; }
  const float a = re / e, b = im / e;
  const float r = sqrtf(fmaf(b, b, a * a));
  c = a / r; s = b / r;
}

template <int C, bool VEC>                            // VEC: X and Y are 8-byte aligned, one access per complex value
__global__ __launch_bounds__(WN_MAXT) void wiener_kernel(const float* __restrict__ X, const float* __restrict__ S, float* __restrict__ Y,
                                                            int B, int J0, int residual, int bins, int frames, int W, int nwin,
                                                            int niter, int softmask, int nslots, const float* __restrict__ ws) {
  extern __shared__ float2 wn_lds[];                  // x: [C][np], then y: [J][C][np]
  __shared__ float part[WN_MAXJ][WN_MAXWAVES][5];               // per source and wave: sum v, sum |y0|^2, sum |y1|^2, sum y0 conj(y1) (re, im)
  __shared__ float Rf[WN_MAXJ][4];                    // R_j: R00, R11, R01 (re, im)
  __shared__ float mpart[WN_MAXWAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nthreads = blockDim.x, nwaves = nthreads >> 6;
  const int k = blockIdx.x % bins, bw = blockIdx.x / bins;
  const int w = bw % nwin, b = bw / nwin;
  const int t0 = w * W, n = min(W, frames - t0), np = min(W, frames);
  const int J = J0 + residual;
  float2* xl = wn_lds;
  float2* yl = wn_lds + C * np;

  float m = 1.f;                                      // B. the window's scale
  if (niter > 0) {
    float h = 0.f;
    for (int i = tid; i < nslots; i += nthreads) h = fmaxf(h, ws[(int64_t)bw * nslots + i]);
    h = wn_wave_max(h);
    if (lane == 0) mpart[wave] = h;
    __syncthreads();
    h = mpart[0];
    for (int q = 1; q < nwaves; ++q) h = fmaxf(h, mpart[q]);
    m = fmaxf(1.f, sqrtf(h) / 10.f);
  }

  // A. initial estimates (then / m).  The loads of a frame -- X and up to eight S of every channel -- are issued together: the loop over the
  // targets is unrolled to WN_MAXJ with the index clamped to the last target (a load past J0 repeats that one and is dropped), where a
  // loop of J0 trips waited for each load before the next.
  const float rm = 1.f / m;
  for (int t = tid; t < n; t += nthreads) {
    float xr[C], xi[C], sv[C][WN_MAXJ];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int64_t i = (((int64_t)b * C + c) * bins + k) * frames + t0 + t;
      if constexpr (VEC) {
        const float2 v = reinterpret_cast<const float2*>(X)[i];
        xr[c] = v.x; xi[c] = v.y;
      } else {
        xr[c] = X[2 * i]; xi[c] = X[2 * i + 1];
      }
#pragma unroll
      for (int j = 0; j < WN_MAXJ; ++j) {
        const int jj = j < J0 ? j : J0 - 1;
        sv[c][j] = S[((((int64_t)jj * B + b) * C + c) * bins + k) * frames + t0 + t];
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float re = xr[c], im = xi[c];
      float den = WN_EPS;
#pragma unroll
      for (int j = 0; j < WN_MAXJ; ++j) den += j < J0 ? sv[c][j] : 0.f;
      float pc, ps;
      wn_phase(re, im, pc, ps);
      float rr = re, ri = im;                         // the residual: X - sum of the target estimates
#pragma unroll
      for (int j = 0; j < WN_MAXJ; ++j) {
        if (j < J0) {
          float yr, yi;
          if (softmask) {
            const float g = sv[c][j] / den;
            yr = re * g; yi = im * g;
          } else {
            yr = sv[c][j] * pc; yi = sv[c][j] * ps;
          }
          rr -= yr; ri -= yi;
          yl[(j * C + c) * np + t] = make_float2(yr * rm, yi * rm);
        }
      }
      if (residual) yl[(J0 * C + c) * np + t] = make_float2(rr * rm, ri * rm);
      xl[c * np + t] = make_float2(re * rm, im * rm);
    }
  }

  // C. expectation-maximisation
  for (int it = 0; it < niter; ++it) {
    for (int j = 0; j < J; ++j) {
      float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
      for (int t = tid; t < n; t += nthreads) {
        const float2 y0 = yl[(j * C) * np + t];
        const float p0 = y0.x * y0.x + y0.y * y0.y;
        if constexpr (C == 1) {
          a[0] += p0;
        } else {
          const float2 y1 = yl[(j * C + 1) * np + t];
          const float p1 = y1.x * y1.x + y1.y * y1.y;
          a[0] += 0.5f * (p0 + p1);
          a[1] += p0;
          a[2] += p1;
          a[3] += y0.x * y1.x + y0.y * y1.y;          // y0 conj(y1)
          a[4] += y0.y * y1.x - y0.x * y1.y;
        }
      }
#pragma unroll
      for (int q = 0; q < (C == 1 ? 1 : 5); ++q) {
        const float v = rfx_wave_sum(a[q]);
        if (lane == 0) part[j][wave][q] = v;
      }
    }
    __syncthreads();
    if (tid < J) {
      float s[5];
#pragma unroll
      for (int q = 0; q < (C == 1 ? 1 : 5); ++q) {
        s[q] = part[tid][0][q];
        for (int wv = 1; wv < nwaves; ++wv) s[q] += part[tid][wv][q];
      }
      const float den = WN_EPS + s[0];
      if constexpr (C == 1) {
        Rf[tid][0] = s[0] / den;
      } else {
        Rf[tid][0] = s[1] / den; Rf[tid][1] = s[2] / den; Rf[tid][2] = s[3] / den; Rf[tid][3] = s[4] / den;
      }
    }
    __syncthreads();
    for (int t = tid; t < n; t += nthreads) {
      if constexpr (C == 1) {
        const float2 x0 = xl[t];
        float cx = WN_SQRT_EPS;
        for (int j = 0; j < J; ++j) {
          const float2 y0 = yl[j * np + t];
          cx += (y0.x * y0.x + y0.y * y0.y) * Rf[j][0];
        }
        const float zr = x0.x / cx, zi = x0.y / cx;
        for (int j = 0; j < J; ++j) {
          const float2 y0 = yl[j * np + t];
          const float g = (y0.x * y0.x + y0.y * y0.y) * Rf[j][0];
          yl[j * np + t] = make_float2(g * zr, g * zi);
        }
      } else {
        const float2 x0 = xl[t], x1 = xl[np + t];
        float ca = WN_SQRT_EPS, cd = WN_SQRT_EPS, cbr = 0.f, cbi = 0.f;          // Cxx = [[ca, cb], [conj(cb), cd]]
        for (int j = 0; j < J; ++j) {
          const float2 y0 = yl[(j * 2) * np + t], y1 = yl[(j * 2 + 1) * np + t];
          const float v = 0.5f * ((y0.x * y0.x + y0.y * y0.y) + (y1.x * y1.x + y1.y * y1.y));
          ca += v * Rf[j][0]; cd += v * Rf[j][1]; cbr += v * Rf[j][2]; cbi += v * Rf[j][3];
        }
        // z = Cxx^{-1} x, the inverse as adjugate / determinant: [[cd, -cb], [-conj(cb), ca]] / det
        const float det = fmaf(ca, cd, -(cbr * cbr + cbi * cbi));
        const float z0r = (cd * x0.x - (cbr * x1.x - cbi * x1.y)) / det;
        const float z0i = (cd * x0.y - (cbr * x1.y + cbi * x1.x)) / det;
        const float z1r = (ca * x1.x - (cbr * x0.x + cbi * x0.y)) / det;
        const float z1i = (ca * x1.y - (cbr * x0.y - cbi * x0.x)) / det;
        for (int j = 0; j < J; ++j) {
          const float2 y0 = yl[(j * 2) * np + t], y1 = yl[(j * 2 + 1) * np + t];
          const float v = 0.5f * ((y0.x * y0.x + y0.y * y0.y) + (y1.x * y1.x + y1.y * y1.y));
          const float r00 = Rf[j][0], r11 = Rf[j][1], br = Rf[j][2], bi = Rf[j][3];
          // y_j = v_j R_j z, R_j = [[r00, b], [conj(b), r11]]
          const float u0r = r00 * z0r + (br * z1r - bi * z1i), u0i = r00 * z0i + (br * z1i + bi * z1r);
          const float u1r = (br * z0r + bi * z0i) + r11 * z1r, u1i = (br * z0i - bi * z0r) + r11 * z1i;
          yl[(j * 2) * np + t] = make_float2(v * u0r, v * u0i);
          yl[(j * 2 + 1) * np + t] = make_float2(v * u1r, v * u1i);
        }
      }
    }
  }

  // D. store m y
  for (int t = tid; t < n; t += nthreads) {
    for (int j = 0; j < J; ++j) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float2 y = yl[(j * C + c) * np + t];
        const int64_t i = (((((int64_t)b * J + j) * C + c) * bins + k) * frames) + t0 + t;
        if constexpr (VEC) {
          reinterpret_cast<float2*>(Y)[i] = make_float2(m * y.x, m * y.y);
        } else {
          Y[2 * i] = m * y.x; Y[2 * i + 1] = m * y.y;
        }
      }
    }
  }
}

extern "C" int rfx_wiener_max_window(void) { return WN_MAXW; }

static bool wn_ok(int B, int C, int J0, int residual, int bins, int frames, int W, int niter) {
  if (B <= 0 || bins <= 0 || frames <= 0 || W <= 0 || W > WN_MAXW || niter < 0 || J0 < 1) return false;
  if (C != 1 && C != 2) return false;
  if (residual != 0 && residual != 1) return false;
  const int J = J0 + residual;
  if (J > WN_MAXJ) return false;
  if (niter > 0 && J == 1) return false;
  const int64_t nwin = wn_windows(frames, W);
  if ((int64_t)B * nwin * bins > 0x7fffffffLL || (int64_t)B * nwin * wn_slots(C, bins) > 0x7fffffffLL) return false;
  return true;
}

extern "C" int64_t rfx_wiener_ws_floats(int32_t B, int32_t C, int32_t bins, int32_t frames, int32_t W) {
  if (!wn_ok(B, C, 1, 0, bins, frames, W, 0)) return -1;
  return (int64_t)B * wn_windows(frames, W) * wn_slots(C, bins);
}

extern "C" int rfx_wiener(const float* X, const float* S, float* Y, int32_t B, int32_t C, int32_t J0, int32_t residual, int32_t bins,
                          int32_t frames, int32_t W, int32_t niter, int32_t softmask, float* ws, void* stream) {
  if (!X || !S || !Y || !wn_ok(B, C, J0, residual, bins, frames, W, niter) || (niter > 0 && !ws)) return -1;
  const int nwin = wn_windows(frames, W), nslots = wn_slots(C, bins), np = W < frames ? W : frames;
  const int J = J0 + residual;
  if (niter > 0) {
    hipLaunchKernelGGL(wiener_scale_kernel, dim3(B * nwin * nslots), dim3(WN_THREADS), 0, (hipStream_t)stream, X, C * bins, frames, W,
                       nwin, nslots, ws);
    RFX_CHECK_LAUNCH();
  }
  const size_t lds = (size_t)(J + 1) * C * np * sizeof(float2);
  const dim3 grid(B * nwin * bins), block(np >= WN_MAXT ? WN_MAXT : (np + 63) / 64 * 64);
  const bool vec = (((uintptr_t)X | (uintptr_t)Y) & 7) == 0;
#define WN_LAUNCH(CC, VV)                                                                                                     \
  hipLaunchKernelGGL((wiener_kernel<CC, VV>), grid, block, lds, (hipStream_t)stream, X, S, Y, B, J0, residual, bins, frames, W, nwin, \
                     niter, softmask != 0, nslots, ws)
  if (C == 1) { if (vec) WN_LAUNCH(1, true); else WN_LAUNCH(1, false); }
  else { if (vec) WN_LAUNCH(2, true); else WN_LAUNCH(2, false); }
#undef WN_LAUNCH
  RFX_CHECK_LAUNCH();
  return 0;
}
