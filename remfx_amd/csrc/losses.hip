// Loss reductions of the hot path: auraloss STFTLoss terms (spectral convergence +
// log-magnitude L1), waveform L1, SI-SDR sums.  All HBM-bound streaming reductions.
// Replaces: models.py:107,299,320,362,385 (mrstft + 100*L1), models.py:227-255 (metrics).
#include "common.h"

// xc, yc: [R][n] complex (float2); sums[r] = { sum (ym-xm)^2, sum ym^2, sum |log xm - log ym| }
__global__ __launch_bounds__(256) void stft_loss_reduce_kernel(const float2* __restrict__ xc,
                                                               const float2* __restrict__ yc, int64_t n,
                                                               float eps, double* __restrict__ slots) {
  const int r = blockIdx.y;
  const float2* xr = xc + (int64_t)r * n;
  const float2* yr = yc + (int64_t)r * n;
  // |log xm - log ym| = |log px - log py| / 2 on the clamped powers; hardware sqrt / log (1 ulp) -- the kernel is
  // otherwise bound by the transcendental fix-up sequences, not by HBM.  Eight terms are summed in fp32, then in fp64.
  double a = 0, b = 0, c = 0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < n; i0 += 8 * stride) {
    float fa = 0.f, fb = 0.f, fc = 0.f;
    float2 xv[8], yv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {            // all loads first, unconditional (clamped index; masked below)
      const int64_t i = i0 + u * stride;
      xv[u] = xr[i < n ? i : n - 1];
      yv[u] = yr[i < n ? i : n - 1];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float m = (i0 + u * stride) < n ? 1.f : 0.f;
      const float2 x = xv[u], y = yv[u];
      const float px = fmaxf(x.x * x.x + x.y * x.y, eps), py = fmaxf(y.x * y.x + y.y * y.y, eps);
      const float dd = __builtin_amdgcn_sqrtf(py) - __builtin_amdgcn_sqrtf(px);
      fa += m * dd * dd;
      fb += m * py;
      fc += m * fabsf(__builtin_amdgcn_logf(px) - __builtin_amdgcn_logf(py));
    }
    a += (double)fa; b += (double)fb; c += (double)(fc * 0.34657359027997264f);   // log2 -> ln, halved
  }
  const double v[3] = {a, b, c};
  rfx_block_store_slot<3>(v, slots, r, gridDim.x, blockIdx.x);
}

// gxc = d/dxc [ w_sc * sqrt(A_r)/sqrt(B_r) + w_lm * sum |log xm - log ym| ]
//   w_sc, w_lm already contain the upstream gradient and the 1/R, 1/(R*n), 1/3 factors.
// ymag != NULL: the clamped target magnitudes sqrt(max(|Y|^2, eps)) as stored by rfx_stft_pair_loss (yc unused)
__global__ __launch_bounds__(256) void stft_loss_grad_kernel(const float2* __restrict__ xc,
                                                             const float2* __restrict__ yc, const float* __restrict__ ymag, int64_t n,
                                                             float eps, const float* __restrict__ sums,
                                                             float w_sc, float w_lm, const float* __restrict__ gup, float2* __restrict__ gxc) {
  const int r = blockIdx.y;
  if (gup) { const float u = gup[0]; w_sc *= u; w_lm *= u; }      // upstream scalar gradient read on the device (no host sync)
  const float A = sums[3 * r], B = sums[3 * r + 1];
  const float ksc = (A > 0.f && B > 0.f) ? w_sc / (sqrtf(A) * sqrtf(B)) : 0.f;   // d sqrt(A)/sqrt(B) / dA * 2
  const float2* xr = xc + (int64_t)r * n;
  const float2* yr = yc ? yc + (int64_t)r * n : nullptr;
  const float* mr = ymag ? ymag + (int64_t)r * n : nullptr;
  float2* gr = gxc + (int64_t)r * n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float2 x = xr[i];
    float2 g = make_float2(0.f, 0.f);
    if (mr) {
      // paired forward (rfx_stft_pair_loss): the same rounding sequence as its epilogue -- rfx_pow2, hardware sqrt -- and the sign of
      // log xm - log ym taken from xm - ym, so identical signals (|X| == |Y| bit for bit) get an exactly zero gradient
      const float px = rfx_pow2(x.x, x.y);
      if (px > eps) {
        const float xm = __builtin_amdgcn_sqrtf(px), ym = mr[i];
        const float dm = ksc * (xm - ym) + w_lm * (xm > ym ? 1.f : (xm < ym ? -1.f : 0.f)) / xm;
        g.x = dm * x.x / xm;
        g.y = dm * x.y / xm;
      }
    } else {
      const float px = x.x * x.x + x.y * x.y;
      if (px > eps) {   // clamp(min=eps) passes no gradient below eps
        const float xm = sqrtf(px);
        const float2 y = yr[i];
        const float ym = sqrtf(fmaxf(y.x * y.x + y.y * y.y, eps));
        const float lg = logf(xm) - logf(ym);
        const float dm = ksc * (xm - ym) + w_lm * (lg > 0.f ? 1.f : (lg < 0.f ? -1.f : 0.f)) / xm;
        g.x = dm * x.x / xm;
        g.y = dm * x.y / xm;
      }
    }
    gr[i] = g;
  }
}

// g[i] = w * sign(a[i]-b[i])
__global__ void l1_grad_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n, float w,
                               const float* __restrict__ gup, float* __restrict__ g) {
  if (gup) w *= gup[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float d = a[i] - b[i];
    g[i] = d > 0.f ? w : (d < 0.f ? -w : 0.f);
  }
}

// per row r of [R][L]: sums[r] = { sum x, sum t, sum x*t, sum x*x, sum t*t }  (double accumulate)
__global__ __launch_bounds__(256) void sisdr_sums_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                         int64_t L, int64_t xs, int64_t ts, double* __restrict__ sums /* slots */) {
  const int r = blockIdx.y;
  const float* xr = x + (int64_t)r * xs;
  const float* tr = t + (int64_t)r * ts;
  double s[5] = {0, 0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += (int64_t)gridDim.x * 256) {
    const double a = xr[i], b = tr[i];
    s[0] += a; s[1] += b; s[2] += a * b; s[3] += a * a; s[4] += b * b;
  }
  rfx_block_store_slot<5>(s, sums, r, gridDim.x, blockIdx.x);
}

// The scalar tail of auraloss MultiResolutionSTFTLoss over the row sums of all resolutions in ONE launch (it was ~24 one-element torch
// launches per evaluation, three evaluations per training step): per resolution k, sums_k [R][3] = { sum (ym - xm)^2, sum ym^2,
// sum |log xm - log ym| } per row, n_k spectrum cells per row:
//   sc_k = per_example ? mean_r sqrt(A_r) / sqrt(B_r) : sqrt(sum_r A_r) / sqrt(sum_r B_r);   lm_k = sum_r C_r / (R n_k)
//   out[0] = (1 / nres) sum_k (sc_k + lm_k)
// One wave; rows are taken in order by lane l = r mod 64 and reduced with the fixed butterfly (bit-reproducible).
struct MrCombineArgs {
  const float* sums[8];
  double n[8];
  int nres, R, per_example;
  float* out;
};
__global__ __launch_bounds__(64) void mrstft_combine_kernel(const MrCombineArgs a) {
  const int lane = threadIdx.x;
  double total = 0.0;
  for (int k = 0; k < a.nres; ++k) {
    const float* s = a.sums[k];
    double sc = 0.0, sa = 0.0, sb = 0.0, sl = 0.0;
    for (int r = lane; r < a.R; r += 64) {
      const float A = s[3 * r], B = s[3 * r + 1], C = s[3 * r + 2];
      sc += (double)(sqrtf(A) / sqrtf(B));
      sa += (double)A; sb += (double)B; sl += (double)C;
    }
    sc = rfx_wave_sum_d(sc); sa = rfx_wave_sum_d(sa); sb = rfx_wave_sum_d(sb); sl = rfx_wave_sum_d(sl);
    const double scv = a.per_example ? sc / (double)a.R : (double)(sqrtf((float)sa) / sqrtf((float)sb));
    total += scv + sl / ((double)a.R * a.n[k]);
  }
  if (lane == 0) a.out[0] = (float)(total / (double)a.nres);
}

// ---- auraloss STFTLoss with a frequency scale (scale="mel") and the three magnitude term weights -------------------------------
// A triangular filter bank is banded: filter f covers bins [first_f, first_f + len_f) and every bin feeds at most two filters, so the
// (n_out x bins) matmul auraloss runs on the magnitudes (torch.matmul(self.fb, x_mag)) is ~2 * bins multiply-adds per frame and
// belongs in the pass that already walks the spectra.  Band tables: idx[n][3] = { first, len, offset into w }, w = the weights of
// row 0, row 1, ... packed.  The forward takes the band of fb (one row per filter), the backward the band of fb^T (one row per bin).
//
// Forward, one workgroup per (row, frame group), one frame at a time:
//   1. 256 threads read the frame's line of X and Y and store { |X|, |Y| } (sqrt of the clamped power) as one float2 per bin in LDS;
//   2. eight lanes per filter walk its band (lane j takes elements j, j + 8, ...), so a ds_read_b64 fetches both magnitudes of a bin
//      and the eight lanes of a filter read 64 contiguous bytes; the partial dot products meet in a fixed xor butterfly (4, 2, 1);
//   3. lane 0 of the eight adds the filter's four terms to its fp64 partials and stores Mx, My for the backward.
// The magnitudes of a frame are ONE line (no row pitch to pad): two lanes of a 32-lane half collide only when their bins differ by a
// non-zero multiple of 32 (64 banks / 2 dwords), which the band starts of neighbouring filters decide, not a pitch.  The weights sit
// behind the magnitudes in LDS, staged once per workgroup.
// Identity (idx == NULL, the linear scale with non-default weights): Mx = |X| per bin, no LDS.
__global__ __launch_bounds__(256) void stft_scaled_loss_kernel(const float2* __restrict__ xc, const float2* __restrict__ yc, int frames,
                                                               int bins, const int32_t* __restrict__ idx, const float* __restrict__ fbw,
                                                               int n_out, int n_w, float eps, double* __restrict__ slots,
                                                               float* __restrict__ mx, float* __restrict__ my) {
  extern __shared__ float2 rfx_scaled_lds_[];
  float2* mag = rfx_scaled_lds_;                                  // [bins]
  float* wl = (float*)(rfx_scaled_lds_ + bins);                   // [n_w]
  const int r = blockIdx.y, tid = threadIdx.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (idx) {
    for (int i = tid; i < n_w; i += 256) wl[i] = fbw[i];
  }
  for (int fr = blockIdx.x; fr < frames; fr += gridDim.x) {
    const int64_t line = (int64_t)r * frames + fr;
    const float2* xr = xc + line * bins;
    const float2* yr = yc + line * bins;
    if (!idx) {
      for (int b = tid; b < bins; b += 256) {
        const float2 x = xr[b], y = yr[b];
        const float a = sqrtf(fmaxf(rfx_pow2(x.x, x.y), eps)), c = sqrtf(fmaxf(rfx_pow2(y.x, y.y), eps));
        const float d = c - a;
        acc[0] += (double)d * (double)d; acc[1] += (double)c * (double)c;
        acc[2] += (double)fabsf(logf(a) - logf(c)); acc[3] += (double)fabsf(a - c);
        if (mx) { mx[line * n_out + b] = a; my[line * n_out + b] = c; }
      }
      continue;
    }
    __syncthreads();                                              // the previous frame's band walks are done (and wl is staged)
    for (int b = tid; b < bins; b += 256) {
      const float2 x = xr[b], y = yr[b];
      mag[b] = make_float2(sqrtf(fmaxf(rfx_pow2(x.x, x.y), eps)), sqrtf(fmaxf(rfx_pow2(y.x, y.y), eps)));
    }
    __syncthreads();
    const int j = tid & 7;
    for (int f0 = 0; f0 < n_out; f0 += 32) {                      // wave-uniform trip count: the shuffles below run in every lane
      const int f = f0 + (tid >> 3);
      int first = 0, len = 0, off = 0;
      if (f < n_out) { first = idx[3 * f]; len = idx[3 * f + 1]; off = idx[3 * f + 2]; }
      float a = 0.f, c = 0.f;
      for (int i = j; i < len; i += 8) {
        const float w = wl[off + i];
        const float2 m = mag[first + i];
        a = fmaf(w, m.x, a); c = fmaf(w, m.y, c);
      }
#pragma unroll
      for (int o = 4; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); c += __shfl_xor(c, o, 64); }
      if (j == 0 && f < n_out) {
        const float d = c - a;
        acc[0] += (double)d * (double)d; acc[1] += (double)c * (double)c;
        acc[2] += (double)fabsf(logf(a) - logf(c)); acc[3] += (double)fabsf(a - c);
        if (mx) { mx[line * n_out + f] = a; my[line * n_out + f] = c; }
      }
    }
  }
  rfx_block_store_slot<4>(acc, slots, r, gridDim.x, blockIdx.x);
}

// G = d|X| * X / |X| with d|X| = fb^T dM and, per filter,
//   dM = ksc (Mx - My) + (w_lm / Mx + w_lin) sign(Mx - My),   ksc = w_sc / (sqrt(A) sqrt(B))
// (A, B of the row, or of the whole batch when !per_example; the sign of log Mx - log My is the sign of Mx - My, so identical signals
// get an exactly zero gradient).  One workgroup per (row, frame group): the frame's dM in LDS, then every bin GATHERS from the filters
// of its row of the transposed band -- no scatter, no atomics.  tidx == NULL: identity.
__global__ __launch_bounds__(256) void stft_scaled_loss_grad_kernel(const float2* __restrict__ xc, const float* __restrict__ mx,
                                                                    const float* __restrict__ my, int R, int frames, int bins, int n_out,
                                                                    const int32_t* __restrict__ tidx, const float* __restrict__ tw,
                                                                    float eps, const double* __restrict__ sums, int per_example,
                                                                    float w_sc, float w_lm, float w_lin, const float* __restrict__ gup,
                                                                    float2* __restrict__ gxc) {
  extern __shared__ float2 rfx_scaled_lds_[];
  float* dm = (float*)rfx_scaled_lds_;                            // [n_out]
  __shared__ float ksc_s;
  const int r = blockIdx.y, tid = threadIdx.x;
  if (gup) { const float u = gup[0]; w_sc *= u; w_lm *= u; w_lin *= u; }
  if (tid < 64) {
    double A = 0.0, B = 0.0;
    if (per_example) { A = sums[4 * r]; B = sums[4 * r + 1]; }
    else {
      for (int q = tid; q < R; q += 64) { A += sums[4 * q]; B += sums[4 * q + 1]; }     // rows in lane order, fixed butterfly
      A = rfx_wave_sum_d(A); B = rfx_wave_sum_d(B);
    }
    if (tid == 0) ksc_s = (A > 0.0 && B > 0.0) ? (float)((double)w_sc / (sqrt(A) * sqrt(B))) : 0.f;
  }
  __syncthreads();
  const float ksc = ksc_s;
  for (int fr = blockIdx.x; fr < frames; fr += gridDim.x) {
    const int64_t line = (int64_t)r * frames + fr;
    __syncthreads();                                              // the previous frame's gathers are done
    for (int f = tid; f < n_out; f += 256) {
      const float a = mx[line * n_out + f], c = my[line * n_out + f];
      const float sg = a > c ? 1.f : (a < c ? -1.f : 0.f);
      dm[f] = ksc * (a - c) + (w_lm / a + w_lin) * sg;
    }
    __syncthreads();
    const float2* xr = xc + line * bins;
    float2* gr = gxc + line * bins;
    for (int b = tid; b < bins; b += 256) {
      const float2 x = xr[b];
      const float px = rfx_pow2(x.x, x.y);
      float2 g = make_float2(0.f, 0.f);
      if (px > eps) {                                             // clamp(min=eps) passes no gradient below eps
        float d;
        if (tidx) {
          const int first = tidx[3 * b], len = tidx[3 * b + 1], off = tidx[3 * b + 2];
          d = 0.f;
          for (int i = 0; i < len; ++i) d = fmaf(tw[off + i], dm[first + i], d);
        } else {
          d = dm[b];
        }
        const float s = d / sqrtf(px);
        g.x = s * x.x; g.y = s * x.y;
      }
      gr[b] = g;
    }
  }
}

// rfx_mrstft_combine with the three term weights of auraloss STFTLoss (w_sc, w_log_mag, w_lin_mag) on the fp64 [R][4] row sums of
// rfx_stft_scaled_loss: out[0] = (1 / nres) sum_k (w_sc sc_k + w_lm lm_k + w_lin lin_k), lin_k = sum_r D_r / (R n_k).  A term whose
// weight is zero is left out, as auraloss does not evaluate it.  One wave, rows in lane order, fixed butterfly.
struct MrCombineWArgs {
  const double* sums[8];
  double n[8];
  int nres, R, per_example;
  float w_sc, w_lm, w_lin;
  float* out;
};
__global__ __launch_bounds__(64) void mrstft_combine_w_kernel(const MrCombineWArgs a) {
  const int lane = threadIdx.x;
  double total = 0.0;
  for (int k = 0; k < a.nres; ++k) {
    const double* s = a.sums[k];
    double sc = 0.0, sa = 0.0, sb = 0.0, sl = 0.0, sd = 0.0;
    for (int r = lane; r < a.R; r += 64) {
      const double A = s[4 * r], B = s[4 * r + 1];
      sc += sqrt(A) / sqrt(B);
      sa += A; sb += B; sl += s[4 * r + 2]; sd += s[4 * r + 3];
    }
    sc = rfx_wave_sum_d(sc); sa = rfx_wave_sum_d(sa); sb = rfx_wave_sum_d(sb); sl = rfx_wave_sum_d(sl); sd = rfx_wave_sum_d(sd);
    const double scv = a.per_example ? sc / (double)a.R : sqrt(sa) / sqrt(sb);
    const double cells = (double)a.R * a.n[k];
    if (a.w_sc != 0.f) total += (double)a.w_sc * scv;
    if (a.w_lm != 0.f) total += (double)a.w_lm * (sl / cells);
    if (a.w_lin != 0.f) total += (double)a.w_lin * (sd / cells);
  }
  if (lane == 0) a.out[0] = (float)(total / (double)a.nres);
}

// The scalar tail of auraloss SISDRLoss over the fp64 row sums of rfx_sisdr_sums: out[0] = -mean_r 10 log10(|alpha t|^2 / (|x - alpha t|^2 + eps) + eps),
// alpha = <x, t> / (|t|^2 + eps), after removing the row means when zero_mean (the ~22 one-element torch launches it replaces ran
// twice per training step).  One wave, rows in lane order, fixed butterfly.
__global__ __launch_bounds__(64) void sisdr_finish_kernel(const double* __restrict__ sums, int R, double L, int zero_mean, double eps,
                                                          float* __restrict__ out) {
  const int lane = threadIdx.x;
  double acc = 0.0;
  for (int r = lane; r < R; r += 64) {
    const double sx = sums[5 * r], st = sums[5 * r + 1];
    double sxt = sums[5 * r + 2], sxx = sums[5 * r + 3], stt = sums[5 * r + 4];
    if (zero_mean) { sxt -= sx * st / L; sxx -= sx * sx / L; stt -= st * st / L; }
    const double alpha = sxt / (stt + eps);
    const double tt = alpha * alpha * stt;
    const double res = sxx - 2.0 * alpha * sxt + tt;
    acc += 10.0 * log10(tt / (res + eps) + eps);
  }
  acc = rfx_wave_sum_d(acc);
  if (lane == 0) out[0] = (float)(-acc / (double)R);
}

static int grid_x(int64_t n) {
  const int64_t b = (n + 2047) / 2048;
  return (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
}
// reductions: fewer, longer workgroups per row (each ends in one slot store)
constexpr int STFT_REDUCE_MAX_SLOTS = 64;
static int grid_red(int64_t n) {
  const int64_t b = (n + 16383) / 16384;
  return (int)(b < 1 ? 1 : (b > STFT_REDUCE_MAX_SLOTS ? STFT_REDUCE_MAX_SLOTS : b));   // <= the cap rfx_stft_loss_reduce_ws answers, by this clamp
}
// workgroups per row of the five-sum kernels (rfx_sisdr_sums, rfx_time_sums, rfx_logcosh_rows), one slot each
constexpr int TIME_SUMS_MAX_SLOTS = 128;
static int time_sums_grid(int64_t L) {
  const int g = grid_x(L);
  return g > TIME_SUMS_MAX_SLOTS ? TIME_SUMS_MAX_SLOTS : g;              // <= the cap rfx_sisdr_sums_ws answers, by this clamp
}
static bool loss_rows_ok(int32_t R, int64_t n) { return R > 0 && R <= RFX_LOSS_MAX_ROWS && n > 0; }

// the bound of grid_red per row and sum, not grid_red(n): enough for every n
extern "C" int64_t rfx_stft_loss_reduce_ws(int32_t R, int64_t n) {
  return loss_rows_ok(R, n) ? (int64_t)3 * R * STFT_REDUCE_MAX_SLOTS : -1;
}
extern "C" int rfx_stft_loss_reduce(const float* xc, const float* yc, int32_t R, int64_t n, float eps, double* ws,
                                    float* sums, void* stream) {
  if (!xc || !yc || !sums || !ws || !loss_rows_ok(R, n)) return -1;
  const int g = grid_red(n);
  hipLaunchKernelGGL(stft_loss_reduce_kernel, dim3(g, R), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)xc, (const float2*)yc, n, eps, ws);
  RFX_CHECK_LAUNCH();
  hipLaunchKernelGGL(rfx_slot_sum_kernel<float>, RFX_SLOT_SUM_GRID(3 * R), 0, (hipStream_t)stream, ws, R, g, 3, sums);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_stft_loss_grad(const float* xc, const float* yc, int32_t R, int64_t n, float eps,
                                  const float* sums, float w_sc, float w_lm, const float* gup, float* gxc, void* stream) {
  if (!xc || !yc || !sums || !gxc || R <= 0 || R > RFX_LOSS_MAX_ROWS || n <= 0) return -1;
  hipLaunchKernelGGL(stft_loss_grad_kernel, dim3(grid_x(n), R), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)xc, (const float2*)yc, (const float*)nullptr, n, eps, sums, w_sc, w_lm, gup, (float2*)gxc);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_stft_loss_grad_m(const float* xc, const float* ymag, int32_t R, int64_t n, float eps,
                                    const float* sums, float w_sc, float w_lm, const float* gup, float* gxc, void* stream) {
  if (!xc || !ymag || !sums || !gxc || R <= 0 || R > RFX_LOSS_MAX_ROWS || n <= 0) return -1;
  hipLaunchKernelGGL(stft_loss_grad_kernel, dim3(grid_x(n), R), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)xc, (const float2*)nullptr, ymag, n, eps, sums, w_sc, w_lm, gup, (float2*)gxc);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_l1_grad(const float* a, const float* b, int64_t n, float w, const float* gup, float* g, void* stream) {
  if (!a || !b || !g || n <= 0) return -1;
  hipLaunchKernelGGL(l1_grad_kernel, dim3(grid_x(n) * 4), dim3(256), 0, (hipStream_t)stream, a, b, n, w, gup, g);
  RFX_CHECK_LAUNCH();
  return 0;
}
// the bound of time_sums_grid per row and sum, not time_sums_grid(L) (that is rfx_time_sums_ws): enough for every L
extern "C" int64_t rfx_sisdr_sums_ws(int32_t R, int64_t L) {
  return loss_rows_ok(R, L) ? (int64_t)5 * R * TIME_SUMS_MAX_SLOTS : -1;
}
extern "C" int rfx_sisdr_sums(const float* x, const float* t, int32_t R, int64_t L, int64_t x_rs,
                              int64_t t_rs, double* ws, double* sums, void* stream) {
  if (!x || !t || !sums || !ws || !loss_rows_ok(R, L)) return -1;
  const int g = time_sums_grid(L);
  hipLaunchKernelGGL(sisdr_sums_kernel, dim3(g, R), dim3(256), 0, (hipStream_t)stream, x, t, L, x_rs, t_rs, ws);
  RFX_CHECK_LAUNCH();
  hipLaunchKernelGGL(rfx_slot_sum_kernel<double>, RFX_SLOT_SUM_GRID(5 * R), 0, (hipStream_t)stream, ws, R, g, 5, sums);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_mrstft_combine(const float* const* sums, const int64_t* n, int32_t nres, int32_t R, int32_t per_example_sc,
                                  float* out, void* stream) {
  if (!sums || !n || !out || nres <= 0 || nres > 8 || R <= 0) return -1;
  MrCombineArgs a;
  for (int k = 0; k < 8; ++k) { a.sums[k] = nullptr; a.n[k] = 1.0; }
  for (int k = 0; k < nres; ++k) {
    if (!sums[k] || n[k] <= 0) return -1;
    a.sums[k] = sums[k];
    a.n[k] = (double)n[k];
  }
  a.nres = nres; a.R = R; a.per_example = per_example_sc; a.out = out;
  hipLaunchKernelGGL(mrstft_combine_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  RFX_CHECK_LAUNCH();
  return 0;
}
// one slot per workgroup: frame groups per row
static int scaled_grid(int frames) { return frames < 1 ? 1 : (frames > 64 ? 64 : frames); }
static size_t scaled_lds(int bins, int n_w) { return (size_t)bins * sizeof(float2) + (size_t)n_w * sizeof(float); }
#define RFX_SCALED_LDS_MAX (64 * 1024)
extern "C" int64_t rfx_stft_scaled_loss_ws(int32_t R, int32_t frames) {
  if (R <= 0 || frames <= 0) return 0;
  return (int64_t)4 * R * scaled_grid(frames);
}
extern "C" int rfx_stft_scaled_loss(const float* xc, const float* yc, int32_t R, int32_t frames, int32_t bins, const int32_t* fb_idx,
                                    const float* fb_w, int32_t n_out, int32_t n_w, float eps, double* ws, double* sums, float* mx,
                                    float* my, void* stream) {
  if (!xc || !yc || !sums || !ws || R <= 0 || R > RFX_LOSS_MAX_ROWS || frames <= 0 || bins <= 0 || (!mx) != (!my)) return -1;
  if (fb_idx ? (!fb_w || n_out <= 0 || n_w <= 0) : (n_out != bins)) return -1;
  const size_t lds = fb_idx ? scaled_lds(bins, n_w) : 0;
  if (lds > RFX_SCALED_LDS_MAX) return -1;
  const int g = scaled_grid(frames);
  hipLaunchKernelGGL(stft_scaled_loss_kernel, dim3(g, R), dim3(256), lds, (hipStream_t)stream, (const float2*)xc, (const float2*)yc,
                     frames, bins, fb_idx, fb_w, n_out, fb_idx ? n_w : 0, eps, ws, mx, my);
  RFX_CHECK_LAUNCH();
  hipLaunchKernelGGL(rfx_slot_sum_kernel<double>, RFX_SLOT_SUM_GRID(4 * R), 0, (hipStream_t)stream, ws, R, g, 4, sums);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_stft_scaled_loss_grad(const float* xc, const float* mx, const float* my, int32_t R, int32_t frames, int32_t bins,
                                         const int32_t* fbt_idx, const float* fbt_w, int32_t n_out, float eps, const double* sums,
                                         int32_t per_example_sc, float w_sc, float w_lm, float w_lin, const float* gup, float* gxc,
                                         void* stream) {
  if (!xc || !mx || !my || !sums || !gxc || R <= 0 || R > RFX_LOSS_MAX_ROWS || frames <= 0 || bins <= 0 || n_out <= 0) return -1;
  if (fbt_idx ? !fbt_w : (n_out != bins)) return -1;
  const size_t lds = (size_t)n_out * sizeof(float);
  if (lds > RFX_SCALED_LDS_MAX) {
    // the linear scale at n_fft = 32768: a frame's 16385 dM values are four bytes more than the default dynamic LDS limit
    if (lds > 160 * 1024) return -1;
    static size_t attr_lds = 0;
    if (lds > attr_lds) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(stft_scaled_loss_grad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds) != hipSuccess) return -3;
      attr_lds = lds;
    }
  }
  const int g = frames > 512 ? 512 : frames;
  hipLaunchKernelGGL(stft_scaled_loss_grad_kernel, dim3(g, R), dim3(256), lds, (hipStream_t)stream, (const float2*)xc, mx, my, R,
                     frames, bins, n_out, fbt_idx, fbt_w, eps, sums, per_example_sc, w_sc, w_lm, w_lin, gup, (float2*)gxc);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_mrstft_combine_w(const double* const* sums, const int64_t* n, int32_t nres, int32_t R, int32_t per_example_sc,
                                    float w_sc, float w_lm, float w_lin, float* out, void* stream) {
  if (!sums || !n || !out || nres <= 0 || nres > 8 || R <= 0) return -1;
  MrCombineWArgs a;
  for (int k = 0; k < 8; ++k) { a.sums[k] = nullptr; a.n[k] = 1.0; }
  for (int k = 0; k < nres; ++k) {
    if (!sums[k] || n[k] <= 0) return -1;
    a.sums[k] = sums[k];
    a.n[k] = (double)n[k];
  }
  a.nres = nres; a.R = R; a.per_example = per_example_sc; a.w_sc = w_sc; a.w_lm = w_lm; a.w_lin = w_lin; a.out = out;
  hipLaunchKernelGGL(mrstft_combine_w_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_sisdr_finish(const double* sums, int32_t R, int64_t L, int32_t zero_mean, double eps, float* out, void* stream) {
  if (!sums || !out || R <= 0 || L <= 0) return -1;
  hipLaunchKernelGGL(sisdr_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, R, (double)L, zero_mean, eps, out);
  RFX_CHECK_LAUNCH();
  return 0;
}

// ---- time-domain training losses (auraloss.time: SISDRLoss, SDSDRLoss, SNRLoss, ESRLoss, DCLoss, LogCoshLoss) ---------------------
// The five ratio losses are functions of the row sums { Sx, St, Sxt, Sxx, Stt } of the (optionally FIR-filtered) rows, so
//   d loss_r / d x~[n] = 2 dl/dSxx x~[n] + dl/dSxt t~[n] + dl/dSx = a_r x~[n] + b_r t~[n] + c_r
// with three per-row coefficients: one sums pass, one per-row kernel (fp64), one streaming gradient pass.
// The optional prefilter is x~[n] = h_prev x[n-1] + h_cur x[n] + h_next x[n+1] with zeros outside the row.

// Row sums of the filtered rows.  One element per lane; the two neighbours come from the adjacent lanes (the loop bound is uniform in
// the workgroup, lanes past L hold 0, which IS the halo value), only lanes 0 / 63 of a wave load theirs -- from inside the row, or 0 at
// the row's ends, never the neighbouring row's memory.
__global__ __launch_bounds__(256) void time_sums_kernel(const float* __restrict__ x, const float* __restrict__ t, int64_t L, int64_t xs,
                                                        int64_t ts, double hp, double hc, double hn, double* __restrict__ slots) {
  const int r = blockIdx.y, lane = threadIdx.x & 63;
  const float* xr = x + (int64_t)r * xs;
  const float* tr = t + (int64_t)r * ts;
  double s[5] = {0, 0, 0, 0, 0};
  for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < L; i0 += (int64_t)gridDim.x * 256) {
    const int64_t i = i0 + threadIdx.x;
    const bool in = i < L;
    const float xc = in ? xr[i] : 0.f, tc = in ? tr[i] : 0.f;
    float xm = __shfl_up(xc, 1, 64), xp = __shfl_down(xc, 1, 64);
    float tm = __shfl_up(tc, 1, 64), tp = __shfl_down(tc, 1, 64);
    if (lane == 0) { const bool ok = in && i >= 1; xm = ok ? xr[i - 1] : 0.f; tm = ok ? tr[i - 1] : 0.f; }
    if (lane == 63) { const bool ok = i + 1 < L; xp = ok ? xr[i + 1] : 0.f; tp = ok ? tr[i + 1] : 0.f; }
    if (in) {
      const double a = hp * (double)xm + hc * (double)xc + hn * (double)xp;
      const double b = hp * (double)tm + hc * (double)tc + hn * (double)tp;
      s[0] += a; s[1] += b; s[2] += a * b; s[3] += a * a; s[4] += b * b;
    }
  }
  rfx_block_store_slot<5>(s, slots, r, gridDim.x, blockIdx.x);
}

// Per-row losses, gradient coefficients and the reduced scalar from the fp64 row sums.  One wave, rows in lane order, fixed butterfly.
// With f(Sxx', Sxt', Stt') on the (centred) sums, fa = df/dSxx', fb = df/dSxt':  a = 2 fa, b = fb and, through the centring
// Sxx' = Sxx - Sx^2 / n, Sxt' = Sxt - Sx St / n,  c = -(2 fa Sx + fb St) / n  (0 without it).
// The SI-SDR value is written exactly as in sisdr_finish_kernel: reduction "mean" returns the same bits.
__global__ __launch_bounds__(64) void time_loss_rows_kernel(const double* __restrict__ sums, int R, double L, int kind, int zero_mean,
                                                            double eps, int reduction, float* __restrict__ rows,
                                                            double* __restrict__ coef, float* __restrict__ out) {
  const int lane = threadIdx.x;
  const bool logk = kind <= RFX_TIME_SNR;
  const double K10 = -4.3429448190325182765;            // -10 / ln 10
  double acc = 0.0;
  for (int r = lane; r < R; r += 64) {
    double ca = 0.0, cb = 0.0, cc = 0.0, val;
    if (kind == RFX_TIME_LOGCOSH) {                      // sums [R][1] = sum_n log(cosh(a z) + eps) / a
      val = sums[r] / L;
      acc += val;
    } else {
      const double sx = sums[5 * r], st = sums[5 * r + 1];
      double sxt = sums[5 * r + 2], sxx = sums[5 * r + 3], stt = sums[5 * r + 4];
      if (kind == RFX_TIME_ESR) {
        const double inv = 1.0 / (stt + eps);
        val = (stt - 2.0 * sxt + sxx) * inv;
        ca = 2.0 * inv; cb = -2.0 * inv;
        acc += val;
      } else if (kind == RFX_TIME_DC) {
        const double d = (st - sx) / L, inv = 1.0 / (stt / L + eps);
        val = d * d * inv;
        cc = -2.0 * d / L * inv;
        acc += val;
      } else {
        const bool zm = zero_mean != 0;
        if (zm) { sxt -= sx * st / L; sxx -= sx * sx / L; stt -= st * st / L; }
        double fa, fb, lg;
        if (kind == RFX_TIME_SNR) {
          const double den = sxx - 2.0 * sxt + stt + eps;
          const double q = stt / den + eps;
          lg = log10(q);
          fa = K10 / q * (-stt / (den * den));
          fb = -2.0 * fa;
        } else {
          const double ia = 1.0 / (stt + eps);
          const double alpha = sxt / (stt + eps);
          const double tt = alpha * alpha * stt;
          double res, dres;                              // the residual energy and d res / d Sxt'
          if (kind == RFX_TIME_SISDR) {
            res = sxx - 2.0 * alpha * sxt + tt;
            dres = -2.0 * alpha - 2.0 * sxt * ia + 2.0 * alpha * stt * ia;
          } else {
            res = sxx - 2.0 * sxt + stt;
            dres = -2.0;
          }
          lg = log10(tt / (res + eps) + eps);
          const double den = res + eps, q = tt / den + eps;
          const double dtt = 2.0 * alpha * stt * ia;     // d tt / d Sxt'
          fa = K10 / q * (-tt / (den * den));
          fb = K10 / q * ((dtt * den - tt * dres) / (den * den));
        }
        acc += 10.0 * lg;
        val = -(10.0 * lg);
        ca = 2.0 * fa; cb = fb;
        if (zm) cc = -(2.0 * fa * sx + fb * st) / L;
      }
    }
    rows[r] = (float)val;
    if (coef) { coef[3 * r] = ca; coef[3 * r + 1] = cb; coef[3 * r + 2] = cc; }
  }
  acc = rfx_wave_sum_d(acc);
  if (lane == 0 && out && reduction != RFX_REDUCE_NONE) {   // "none": out stays untouched, as the header promises
    const double tot = logk ? -acc : acc;
    out[0] = (float)(reduction == RFX_REDUCE_MEAN ? tot / (double)R : tot);
  }
}

// upstream gradient of row r, read on the device: one value (/ R for "mean") or one per row ("none")
__device__ __forceinline__ double rfx_row_gup(const float* __restrict__ gup, int reduction, int r, int R) {
  if (reduction == RFX_REDUCE_NONE) return (double)gup[r];
  return reduction == RFX_REDUCE_MEAN ? (double)gup[0] / (double)R : (double)gup[0];
}

struct TimeGradArgs {
  const float* x; const float* t; float* gx;
  const double* coef; const float* gup;
  int64_t L, xs, ts;
  double hp, hc, hn;
  int R, reduction;
};

// gx[n] for one element from the five-sample windows of x and t (row ends are zeros): the scalar head / tail of a row
template <bool TAPS>
__device__ __forceinline__ float time_grad_one(const float* __restrict__ xr, const float* __restrict__ tr, int64_t n, int64_t L, double a,
                                               double b, double c, double hp, double hc, double hn) {
  if (!TAPS) return (float)(a * (double)xr[n] + b * (double)tr[n] + c);
  double xw[5], tw[5], u[3];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int64_t m = n + k - 2;
    const bool ok = m >= 0 && m < L;
    xw[k] = ok ? (double)xr[m] : 0.0; tw[k] = ok ? (double)tr[m] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {                          // u[n - 1 + k], zero outside the row
    const int64_t m = n + k - 1;
    const double xf = hp * xw[k] + hc * xw[k + 1] + hn * xw[k + 2], tf = hp * tw[k] + hc * tw[k + 1] + hn * tw[k + 2];
    u[k] = (m >= 0 && m < L) ? a * xf + b * tf + c : 0.0;
  }
  return (float)(hn * u[0] + hc * u[1] + hp * u[2]);
}

// four consecutive samples of a row, as one 16-byte access when the row's phase allows it
__device__ __forceinline__ f32x4 time_ld4(const float* __restrict__ p, bool vec) {
  if (vec) return rfx_ld4(p);
  return f32x4{p[0], p[1], p[2], p[3]};
}

// The gradient pass: gx[r][n] = g_r (h_prev u[n+1] + h_cur u[n] + h_next u[n-1]), u[m] = a x~[m] + b t~[m] + c inside the row and 0
// outside (the adjoint of the zero-padded filter), every element formed in fp64 and rounded once.  A lane owns the four samples
// n0 .. n0+3 of a 16-byte-aligned group of gx; the two samples on either side come from the neighbouring lanes' groups, and from memory
// (inside the row, else 0) at the ends of a wave and of the vector body.  x / t rows whose 16-byte phase differs from gx's are read as
// four dwords.  The <= 3 samples in front of the first aligned group and behind the last full one go through time_grad_one.
template <bool TAPS>
__global__ __launch_bounds__(256) void time_loss_grad_kernel(const TimeGradArgs p) {
  const int r = blockIdx.y, lane = threadIdx.x & 63;
  const float* xr = p.x + (int64_t)r * p.xs;
  const float* tr = p.t + (int64_t)r * p.ts;
  float* gr = p.gx + (int64_t)r * p.L;
  const double g = rfx_row_gup(p.gup, p.reduction, r, p.R);
  const double a = g * p.coef[3 * r], b = g * p.coef[3 * r + 1], c = g * p.coef[3 * r + 2];
  const double hp = p.hp, hc = p.hc, hn = p.hn;
  const int64_t L = p.L;
  const int phg = (int)(((uintptr_t)gr >> 2) & 3);
  int64_t head = (4 - phg) & 3;
  head = head < L ? head : L;
  const int64_t nvec = (L - head) >> 2, tail0 = head + 4 * nvec;
  const bool xvec = (int)((((uintptr_t)(xr + head)) >> 2) & 3) == 0, tvec = (int)((((uintptr_t)(tr + head)) >> 2) & 3) == 0;
  if (blockIdx.x == 0 && threadIdx.x < 6) {              // scalar head (lanes 0..2) and tail (lanes 3..5)
    const int64_t n = threadIdx.x < 3 ? (int64_t)threadIdx.x : tail0 + threadIdx.x - 3;
    if (threadIdx.x < 3 ? n < head : n < L) gr[n] = time_grad_one<TAPS>(xr, tr, n, L, a, b, c, hp, hc, hn);
  }
  for (int64_t k0 = (int64_t)blockIdx.x * 256; k0 < nvec; k0 += (int64_t)gridDim.x * 256) {
    const int64_t k = k0 + threadIdx.x;
    const bool in = k < nvec;
    const int64_t n0 = head + 4 * k;
    f32x4 xv = {0.f, 0.f, 0.f, 0.f}, tv = {0.f, 0.f, 0.f, 0.f};
    if (in) { xv = time_ld4(xr + n0, xvec); tv = time_ld4(tr + n0, tvec); }
    if (!TAPS) {
      if (in) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (float)(a * (double)xv[j] + b * (double)tv[j] + c);
        rfx_st4(gr + n0, o);
      }
      continue;
    }
    // window w[0..7] = samples n0-2 .. n0+5
    double xw[8], tw[8];
    {
      float xl0 = __shfl_up(xv[2], 1, 64), xl1 = __shfl_up(xv[3], 1, 64), xh0 = __shfl_down(xv[0], 1, 64), xh1 = __shfl_down(xv[1], 1, 64);
      float tl0 = __shfl_up(tv[2], 1, 64), tl1 = __shfl_up(tv[3], 1, 64), th0 = __shfl_down(tv[0], 1, 64), th1 = __shfl_down(tv[1], 1, 64);
      if (in && (lane == 0 || k == 0)) {
        const bool o1 = n0 >= 1, o2 = n0 >= 2;
        xl0 = o2 ? xr[n0 - 2] : 0.f; xl1 = o1 ? xr[n0 - 1] : 0.f;
        tl0 = o2 ? tr[n0 - 2] : 0.f; tl1 = o1 ? tr[n0 - 1] : 0.f;
      }
      if (in && (lane == 63 || k + 1 >= nvec)) {
        const bool o4 = n0 + 4 < L, o5 = n0 + 5 < L;
        xh0 = o4 ? xr[n0 + 4] : 0.f; xh1 = o5 ? xr[n0 + 5] : 0.f;
        th0 = o4 ? tr[n0 + 4] : 0.f; th1 = o5 ? tr[n0 + 5] : 0.f;
      }
      xw[0] = xl0; xw[1] = xl1; xw[6] = xh0; xw[7] = xh1;
      tw[0] = tl0; tw[1] = tl1; tw[6] = th0; tw[7] = th1;
#pragma unroll
      for (int j = 0; j < 4; ++j) { xw[2 + j] = xv[j]; tw[2 + j] = tv[j]; }
    }
    if (in) {
      double u[6];                                       // u[n0-1 .. n0+4]
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const int64_t m = n0 - 1 + j;
        const double xf = hp * xw[j] + hc * xw[j + 1] + hn * xw[j + 2], tf = hp * tw[j] + hc * tw[j + 1] + hn * tw[j + 2];
        u[j] = (m >= 0 && m < L) ? a * xf + b * tf + c : 0.0;
      }
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (float)(hn * u[j] + hc * u[j + 1] + hp * u[j + 2]);
      rfx_st4(gr + n0, o);
    }
  }
}

// log(cosh(y) + eps) = |y| + log((1 + e^-2|y|) / 2 + eps e^-|y|): no overflow for any y.  fp64: with x close to t the value is ~y^2 / 2
// next to cosh ~ 1, which fp32 resolves to 1e-7 ABSOLUTE only.
__global__ __launch_bounds__(256) void logcosh_rows_kernel(const float* __restrict__ x, const float* __restrict__ t, int64_t L, int64_t xs,
                                                           int64_t ts, double a, double eps, double* __restrict__ slots) {
  const int r = blockIdx.y;
  const float* xr = x + (int64_t)r * xs;
  const float* tr = t + (int64_t)r * ts;
  double s[1] = {0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += (int64_t)gridDim.x * 256) {
    const double y = fabs(a * ((double)xr[i] - (double)tr[i]));
    const double e1 = exp(-y);
    s[0] += y + log(0.5 * (1.0 + e1 * e1) + eps * e1);
  }
  s[0] /= a;
  rfx_block_store_slot<1>(s, slots, r, gridDim.x, blockIdx.x);
}

// gx[r][n] = g_r sinh(a z) / (cosh(a z) + eps) / L = g_r sign(z) (1 - e2) / (1 + e2 + 2 eps e1) / L,  e1 = e^-|a z|, e2 = e1^2
__global__ __launch_bounds__(256) void logcosh_grad_kernel(const float* __restrict__ x, const float* __restrict__ t, int R, int64_t L,
                                                           int64_t xs, int64_t ts, double a, double eps, const float* __restrict__ gup,
                                                           int reduction, float* __restrict__ gx) {
  const int r = blockIdx.y;
  const float* xr = x + (int64_t)r * xs;
  const float* tr = t + (int64_t)r * ts;
  float* gr = gx + (int64_t)r * L;
  const double w = rfx_row_gup(gup, reduction, r, R) / (double)L;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += (int64_t)gridDim.x * 256) {
    const double z = a * ((double)xr[i] - (double)tr[i]);
    const double e1 = exp(-fabs(z)), e2 = e1 * e1;
    const double v = w * (1.0 - e2) / (1.0 + e2 + 2.0 * eps * e1);
    gr[i] = (float)(z < 0.0 ? -v : v);
  }
}

// streaming passes over [R][n units]: ~4096 workgroups in all, at least 1024 units each before another workgroup is worth its launch
static int time_stream_grid(int64_t units, int R) {
  int64_t want = (units + 1023) / 1024, cap = 4096 / R;
  cap = cap < 1 ? 1 : cap;
  want = want > cap ? cap : want;
  return (int)(want < 1 ? 1 : want);
}
static bool time_kind_ok(int kind) { return kind >= RFX_TIME_SISDR && kind <= RFX_TIME_LOGCOSH; }
static bool time_red_ok(int red) { return red >= RFX_REDUCE_MEAN && red <= RFX_REDUCE_NONE; }

extern "C" int64_t rfx_time_sums_ws(int32_t R, int64_t L) {
  if (R <= 0 || L <= 0) return 0;
  return (int64_t)5 * R * time_sums_grid(L);
}
extern "C" int rfx_time_sums(const float* x, const float* t, int32_t R, int64_t L, int64_t x_rs, int64_t t_rs, int32_t has_taps,
                             double h_prev, double h_cur, double h_next, double* ws, double* sums, void* stream) {
  if (!x || !t || !sums || !ws || R <= 0 || R > RFX_LOSS_MAX_ROWS || L <= 0) return -1;
  const int g = time_sums_grid(L);                       // the grid of rfx_sisdr_sums: without taps, its kernel and its bits
  if (has_taps)
    hipLaunchKernelGGL(time_sums_kernel, dim3(g, R), dim3(256), 0, (hipStream_t)stream, x, t, L, x_rs, t_rs, h_prev, h_cur, h_next, ws);
  else
    hipLaunchKernelGGL(sisdr_sums_kernel, dim3(g, R), dim3(256), 0, (hipStream_t)stream, x, t, L, x_rs, t_rs, ws);
  RFX_CHECK_LAUNCH();
  hipLaunchKernelGGL(rfx_slot_sum_kernel<double>, RFX_SLOT_SUM_GRID(5 * R), 0, (hipStream_t)stream, ws, R, g, 5, sums);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_time_loss_rows(const double* sums, int32_t R, int64_t L, int32_t kind, int32_t zero_mean, double eps,
                                  int32_t reduction, float* rows, double* coef, float* out, void* stream) {
  if (!sums || !rows || R <= 0 || L <= 0 || !time_kind_ok(kind) || !time_red_ok(reduction)) return -1;
  if (reduction != RFX_REDUCE_NONE && !out) return -1;
  hipLaunchKernelGGL(time_loss_rows_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, R, (double)L, kind, zero_mean, eps,
                     reduction, rows, coef, out);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_time_loss_grad(const float* x, const float* t, int32_t R, int64_t L, int64_t x_rs, int64_t t_rs, const double* coef,
                                  int32_t has_taps, double h_prev, double h_cur, double h_next, const float* gup, int32_t reduction,
                                  float* gx, void* stream) {
  if (!x || !t || !coef || !gup || !gx || R <= 0 || R > RFX_LOSS_MAX_ROWS || L <= 0 || !time_red_ok(reduction)) return -1;
  if ((((uintptr_t)x | (uintptr_t)t | (uintptr_t)gx) & 3) != 0) return -1;
  TimeGradArgs p;
  p.x = x; p.t = t; p.gx = gx; p.coef = coef; p.gup = gup; p.L = L; p.xs = x_rs; p.ts = t_rs;
  p.hp = h_prev; p.hc = h_cur; p.hn = h_next; p.R = R; p.reduction = reduction;
  const dim3 grid(time_stream_grid((L + 3) / 4, R), R);
  if (has_taps) hipLaunchKernelGGL(time_loss_grad_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(time_loss_grad_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int64_t rfx_logcosh_ws(int32_t R, int64_t L) {
  if (R <= 0 || L <= 0) return 0;
  return (int64_t)R * time_sums_grid(L);
}
extern "C" int rfx_logcosh_rows(const float* x, const float* t, int32_t R, int64_t L, int64_t x_rs, int64_t t_rs, double a, double eps,
                                double* ws, double* sums, void* stream) {
  if (!x || !t || !sums || !ws || R <= 0 || R > RFX_LOSS_MAX_ROWS || L <= 0 || !(a > 0.0)) return -1;
  const int g = time_sums_grid(L);
  hipLaunchKernelGGL(logcosh_rows_kernel, dim3(g, R), dim3(256), 0, (hipStream_t)stream, x, t, L, x_rs, t_rs, a, eps, ws);
  RFX_CHECK_LAUNCH();
  hipLaunchKernelGGL(rfx_slot_sum_kernel<double>, RFX_SLOT_SUM_GRID(R), 0, (hipStream_t)stream, ws, R, g, 1, sums);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_logcosh_grad(const float* x, const float* t, int32_t R, int64_t L, int64_t x_rs, int64_t t_rs, double a, double eps,
                                const float* gup, int32_t reduction, float* gx, void* stream) {
  if (!x || !t || !gup || !gx || R <= 0 || R > RFX_LOSS_MAX_ROWS || L <= 0 || !(a > 0.0) || !time_red_ok(reduction)) return -1;
  hipLaunchKernelGGL(logcosh_grad_kernel, dim3(time_stream_grid(L, R), R), dim3(256), 0, (hipStream_t)stream, x, t, R, L, x_rs, t_rs, a,
                     eps, gup, reduction, gx);
  RFX_CHECK_LAUNCH();
  return 0;
}
