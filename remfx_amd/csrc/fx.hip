// Audio-effect rendering on the device: the five effects of remfx/effects.py:297-616 that the
// reference renders on the CPU with pedalboard (JUCE DSP) while it builds / augments the dataset, and the BS.1770
// loudness normalisation it applies after every effect (effects.py:619-629, pyloudnorm).  All kernels take a batch of
// mono clips x: (B, T) fp32 contiguous and PER-CLIP parameter vectors (every clip draws its own random parameters,
// datasets.py:109-202 / 205-330), so one launch renders a whole training batch.
//
// These are HBM-bound byte-streaming or latency-bound recurrence kernels, not GEMMs: coalesced reads along T, recurrences
// blocked by their own lag (a delay line of D samples makes D consecutive outputs independent), wave-level scans where
// the lag is one sample.  Algorithms restated from the published JUCE / pedalboard / pyloudnorm sources (absent from
// the image: parity unpinned, oracle/ref_effects.py is the same restatement in numpy float64).
#include "common.h"

// Row table of the round normalisation (rfx_fx_normalize_rows): output row i goes to row rows[i] of a larger state buffer;
// rows == nullptr is the dense case (row i).
__device__ __forceinline__ int64_t fx_row(const int32_t* __restrict__ rows, int b) { return rows ? (int64_t)rows[b] : (int64_t)b; }

// ---- distortion: pedalboard.Distortion = JUCE Gain(drive_db) -> WaveShaper(tanh) ------------------------------------
__global__ __launch_bounds__(256) void fx_distortion_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t T,
                                                            const float* __restrict__ gain) {
  const int b = blockIdx.y;
  const float g = gain[b];
  const float* xr = x + (int64_t)b * T;
  float* yr = y + (int64_t)b * T;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < T; i += (int64_t)gridDim.x * 1024) {
    if (i + 3 < T) {
      f32x4 v = rfx_ld4(xr + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = tanhf(g * v[j]);
      rfx_st4(yr + i, v);
    } else {
      for (int64_t k = i; k < T; ++k) yr[k] = tanhf(g * xr[k]);
    }
  }
}

// ---- delay: pedalboard.Delay = JUCE DelayLine (integer delay D = int(seconds * sr)), feedback, dry/wet mix ------------
//   delayed[n] = w[n - D];  w[n] = x[n] + fb * delayed[n];  y[n] = (1 - mix) x[n] + mix * delayed[n]
// Unrolled in closed form (the line starts empty): delayed[n] = sum_{k >= 1} fb^(k-1) x[n - k D]: every output sample is
// independent, no workspace, <= T / D taps (D >= 0.1 s in the reference's ranges).
__global__ __launch_bounds__(256) void fx_delay_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t T,
                                                       const int32_t* __restrict__ delay, const float* __restrict__ fb,
                                                       const float* __restrict__ mix) {
  const int b = blockIdx.y;
  const int64_t D = delay[b];
  const float f = fb[b], m = mix[b];
  const float* xr = x + (int64_t)b * T;
  float* yr = y + (int64_t)b * T;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < T; n += (int64_t)gridDim.x * 256) {
    float acc = 0.f, w = 1.f;
    if (D > 0)
      for (int64_t k = n - D; k >= 0; k -= D) { acc = fmaf(w, xr[k], acc); w *= f; }
    else acc = 0.f;
    yr[n] = (1.0f - m) * xr[n] + m * acc;
  }
}

// ---- chorus: JUCE dsp::Chorus (pedalboard.Chorus) -----------------------------------------------------------------------
//   lfo[n] = sin(2 pi rate n / sr - pi) * depth / 2;   d[n] = max(1 ms, 20 ms * lfo[n] + centre) * sr / 1000  (samples)
//   pushed[n] = x[n] - fb * popped[n - 1];  popped[n] = linear interpolation of `pushed` at n - d[n];  y = (1 - mix) x + mix * popped
// The feedback lags ONE sample but reaches back at least 1 ms (48 samples at 48 kHz): blocks of BLK = 32 consecutive
// samples are independent given the history.  One wave per clip, the `pushed` history in an LDS ring.
#define FX_CH_RING 4096
__global__ __launch_bounds__(64) void fx_chorus_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t T, float sr,
                                                       const float* __restrict__ rate, const float* __restrict__ depth,
                                                       const float* __restrict__ centre_ms, const float* __restrict__ fb,
                                                       const float* __restrict__ mix, int blk) {
  __shared__ float ring[FX_CH_RING];
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* xr = x + (int64_t)b * T;
  float* yr = y + (int64_t)b * T;
  const float f = fb[b], m = mix[b], dep = 0.5f * depth[b], cen = centre_ms[b];
  const double winc = 2.0 * 3.14159265358979323846 * (double)rate[b] / (double)sr;
  for (int i = lane; i < FX_CH_RING; i += 64) ring[i] = 0.f;
  __syncthreads();
  float prev_pop = 0.f;                       // popped[n0 - 1]
  for (int64_t n0 = 0; n0 < T; n0 += blk) {
    const int64_t n = n0 + lane;
    const bool act = lane < blk && n < T;
    float pop = 0.f, xv = 0.f;
    if (act) {
      xv = xr[n];
      double ph = winc * (double)n;                     // sin(ph - pi) = -sin(ph); reduce in fp64, evaluate in fp32
      ph -= floor(ph * 0.15915494309189535) * 6.283185307179586;
      const float lfo = -sinf((float)ph) * dep;
      const float dms = fmaxf(1.0f, 20.0f * lfo + cen);
      const float d = dms * sr / 1000.0f;
      const int di = (int)d;
      const float fr = d - (float)di;
      const int64_t i1 = n - di, i2 = i1 - 1;
      const float v1 = i1 >= 0 ? ring[i1 & (FX_CH_RING - 1)] : 0.f;
      const float v2 = i2 >= 0 ? ring[i2 & (FX_CH_RING - 1)] : 0.f;
      pop = v1 + fr * (v2 - v1);
    }
    // pushed[n] = x[n] - fb * popped[n - 1]: previous lane's pop (lane 0: carried from the last block)
    float pm1 = __shfl_up(pop, 1, 64);
    if (lane == 0) pm1 = prev_pop;
    prev_pop = __shfl(pop, blk - 1, 64);
    __syncthreads();                          // all ring reads of this block are done
    if (act) {
      ring[n & (FX_CH_RING - 1)] = xv - f * pm1;
      yr[n] = (1.0f - m) * xv + m * pop;
    }
    __syncthreads();
  }
}

// ---- compressor: JUCE dsp::Compressor (pedalboard.Compressor): peak ballistics envelope + static gain computer ---------
//   env[n] = a + c (env[n-1] - a),  a = |x[n]|, c = (a > env[n-1]) ? c_attack : c_release,   c_* = exp(-2 pi 1000 / (sr ms))
//   gain = env < thr ? 1 : (env / thr)^(1 / ratio - 1);   y = gain * x
// A nonlinear one-sample recurrence: one LANE per clip walks its clip sequentially (the envelope only), then the gain is
// applied by all lanes.  64 clips = one wave; the envelope is written to a workspace so the second pass is coalesced.
__global__ __launch_bounds__(64) void fx_comp_env_kernel(const float* __restrict__ x, float* __restrict__ env, int B, int64_t T,
                                                         const float* __restrict__ c_at, const float* __restrict__ c_rl) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const float ca = c_at[b], cr = c_rl[b];
  const float* xr = x + (int64_t)b * T;
  float* er = env + (int64_t)b * T;
  float yv = 0.f;
  // the recurrence is a ~20-cycle dependent chain per sample; the loads do not depend on it: 8 x 16 bytes in flight per lane
  int64_t n = 0;
  for (; n + 32 <= T; n += 32) {
    f32x4 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = rfx_ld4(xr + n + 4 * q);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float a = fabsf(v[q][j]);
        const float c = a > yv ? ca : cr;
        yv = a + c * (yv - a);
        o[j] = yv;
      }
      rfx_st4(er + n + 4 * q, o);
    }
  }
  for (; n < T; ++n) {
    const float a = fabsf(xr[n]);
    const float c = a > yv ? ca : cr;
    yv = a + c * (yv - a);
    er[n] = yv;
  }
}
// the static gain computer, shared by the compressor and the limiter's output pass
__device__ __forceinline__ float fx_comp_gain(float e, float th, float ti, float ex) { return e < th ? 1.0f : powf(e * ti, ex); }
__global__ __launch_bounds__(256) void fx_comp_gain_kernel(const float* __restrict__ x, const float* __restrict__ env,
                                                           float* __restrict__ y, int64_t T, const float* __restrict__ thr,
                                                           const float* __restrict__ ratio) {
  const int b = blockIdx.y;
  const float th = thr[b], ti = 1.0f / th, ex = 1.0f / ratio[b] - 1.0f;
  const float* xr = x + (int64_t)b * T;
  const float* er = env + (int64_t)b * T;
  float* yr = y + (int64_t)b * T;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < T; n += (int64_t)gridDim.x * 256) {
    const float g = fx_comp_gain(er[n], th, ti, ex);
    yr[n] = g * xr[n];
  }
}

// ---- limiter: JUCE dsp::Limiter (pedalboard.Limiter) = two Compressors in series, make-up gain, hard clip to [-1, 1] --------
//   stage 1: -10 dB, ratio 4, attack 2 ms, release 200 ms;  stage 2: threshold_db, ratio 1000, attack 0.001 ms, release_ms
//   make-up = min(10^(10 (1 - 1/4) / 40), 10^(-threshold_db / 20))
// Stage 1 is the compressor's two kernels as they are; stage 2's envelope walks stage 1's output with the same lane kernel, and one
// coalesced pass applies stage 2's gain, the make-up gain and the clip.  Two lane walks of ~5 instructions per sample each: the
// gain computer's powf stays off the serial lanes.
__global__ __launch_bounds__(256) void fx_limit_out_kernel(const float* __restrict__ x, const float* __restrict__ env,
                                                           float* __restrict__ y, int64_t T, const float* __restrict__ thr,
                                                           const float* __restrict__ ratio, const float* __restrict__ makeup) {
  const int b = blockIdx.y;
  const float th = thr[b], ti = 1.0f / th, ex = 1.0f / ratio[b] - 1.0f, mk = makeup[b];
  const float* xr = x + (int64_t)b * T;
  const float* er = env + (int64_t)b * T;
  float* yr = y + (int64_t)b * T;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < T; n += (int64_t)gridDim.x * 256) {
    const float v = (fx_comp_gain(er[n], th, ti, ex) * xr[n]) * mk;
    yr[n] = fminf(fmaxf(v, -1.0f), 1.0f);
  }
}

// ---- reverb: JUCE Reverb (Freeverb; pedalboard.Reverb), mono path ----------------------------------------------------
//   in = 0.015 x;  out = sum_j comb_j(in);  out = allpass_3(allpass_2(allpass_1(allpass_0(out))));  y = wet1 * out + dry * x
//   comb:    o = buf[i]; last = o (1 - damp) + last damp; buf[i] = in + last * feedback; return o          (lag = comb length)
//   allpass: o = buf[i]; buf[i] = in + 0.5 o; return o - in                                                (lag = length)
// Every filter's lag (>= 225 * sr / 44100 samples, at least 64 from 12544 Hz: lower rates are refused) covers a 64-sample block, so one wave per clip renders 64 samples per
// iteration; the one-pole damping filter inside a comb is a one-sample linear recurrence = a 6-step wave scan.
// All 12 delay buffers of a clip live in LDS.
#define FX_RV_NC 8
#define FX_RV_NA 4
struct FxReverbArgs {
  const float* x;
  float* y;
  int64_t T;
  const float *damp, *feedback, *wet1, *dry;     // per clip
  int comb_len[FX_RV_NC], ap_len[FX_RV_NA];
  int comb_off[FX_RV_NC], ap_off[FX_RV_NA];      // offsets in the LDS arena
  int arena;
};
__global__ __launch_bounds__(64) void fx_reverb_kernel(const FxReverbArgs a) {
  extern __shared__ float arena[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* xr = a.x + (int64_t)b * a.T;
  float* yr = a.y + (int64_t)b * a.T;
  const float damp = a.damp[b], fbk = a.feedback[b], wet1 = a.wet1[b], dry = a.dry[b];
  for (int i = lane; i < a.arena; i += 64) arena[i] = 0.f;
  float last[FX_RV_NC];
  int cpos[FX_RV_NC], apos[FX_RV_NA];
#pragma unroll
  for (int j = 0; j < FX_RV_NC; ++j) { last[j] = 0.f; cpos[j] = 0; }
#pragma unroll
  for (int j = 0; j < FX_RV_NA; ++j) apos[j] = 0;
  // damp^(2^s) for the scan, damp^(lane + 1) for the carried state
  float dpw[6];
  dpw[0] = damp;
#pragma unroll
  for (int s = 1; s < 6; ++s) dpw[s] = dpw[s - 1] * dpw[s - 1];
  const float dl1 = powf(damp, (float)(lane + 1));
  __syncthreads();
  for (int64_t n0 = 0; n0 < a.T; n0 += 64) {
    const int64_t n = n0 + lane;
    const bool act = n < a.T;
    const float xv = act ? xr[n] : 0.f;
    const float in = xv * 0.015f;
    float out = 0.f;
#pragma unroll
    for (int j = 0; j < FX_RV_NC; ++j) {
      float* buf = arena + a.comb_off[j];
      int idx = cpos[j] + lane;
      idx -= idx >= a.comb_len[j] ? a.comb_len[j] : 0;
      const float o = buf[idx];
      // last[i] = (1 - damp) o[i] + damp last[i - 1]: inclusive weighted scan over the 64 lanes
      float v = (1.0f - damp) * o;
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        const float u = __shfl_up(v, 1 << s, 64);
        if (lane >= (1 << s)) v = fmaf(dpw[s], u, v);
      }
      v = fmaf(dl1, last[j], v);
      buf[idx] = in + v * fbk;               // lanes beyond T write garbage-free values (in = 0) that are never read back in range
      last[j] = __shfl(v, 63, 64);
      cpos[j] += 64;
      cpos[j] -= cpos[j] >= a.comb_len[j] ? a.comb_len[j] : 0;
      out += o;
    }
#pragma unroll
    for (int j = 0; j < FX_RV_NA; ++j) {
      float* buf = arena + a.ap_off[j];
      int idx = apos[j] + lane;
      idx -= idx >= a.ap_len[j] ? a.ap_len[j] : 0;
      const float o = buf[idx];
      buf[idx] = out + 0.5f * o;
      out = o - out;
      apos[j] += 64;
      apos[j] -= apos[j] >= a.ap_len[j] ? a.ap_len[j] : 0;
    }
    if (act) yr[n] = out * wet1 + xv * dry;
  }
}

// ---- SoX `reverb` (RandomSoxReverb, effects.py:516-572): Freeverb banks with PER-BANK geometry, wet only, mono or stereo in, stereo out
//   bank(in) = gain * allpass_0(allpass_1(allpass_2(allpass_3( sum_{j = 7..0} comb_j(in) ))));   in[n] = clip(x[n - delay], -1, 1)
//   comb:    o = buf[p]; store = o + (store - o) damp; buf[p] = in + store * feedback; return o
//   allpass: o = buf[p]; buf[p] = in + 0.5 o; return o - in
//   wet[w] = clip(mean over the input channels of bank_w(channel));   y[w] = x[min(w, Cin - 1)] (1 - wet_dry) + wet[w] wet_dry
// Room scale, stereo depth and pre-delay are drawn per clip, so the twelve lengths, the pre-delay and the input row of a bank come
// from device memory (geom), as do feedback, damp, gain and wet_dry (coef).  One workgroup of one wave owns ONE bank (<= 55 KB of LDS
// at 48 kHz): the 2 Cin banks of a clip run side by side and leave their wet signal in a workspace; fx_sox_mix_kernel then averages
// the channels, clips, mixes with the dry signal and stores every output sample once.  The scheme inside a bank is fx_reverb_kernel's;
// the block is narrowed to the bank's shortest lag where that is below 64 samples.  The pre-delay reads x[n - delay] from global memory.
#define FX_SOX_GEOM 16       // int32 per bank: pre-delay, 8 comb lengths, 4 all-pass lengths, input row of x, 2 spare
#define FX_SOX_COEF 4        // float per bank: feedback, damp, gain, wet_dry
__global__ __launch_bounds__(64) void fx_sox_bank_kernel(const float* __restrict__ x, float* __restrict__ ws, int64_t T,
                                                         const int32_t* __restrict__ geom, const float* __restrict__ coef,
                                                         int lds_floats, int64_t x_rows) {
  extern __shared__ float sox_arena[];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int32_t* g = geom + (int64_t)r * FX_SOX_GEOM;
  const float* cf = coef + (int64_t)r * FX_SOX_COEF;
  float* wr = ws + (int64_t)r * T;
  const int64_t delay = g[0], row = g[1 + FX_RV_NC + FX_RV_NA];
  int clen[FX_RV_NC], alen[FX_RV_NA], coff[FX_RV_NC], aoff[FX_RV_NA];
  int off = 0, blk = 64;
  bool ok = delay >= 0 && row >= 0 && row < x_rows;
#pragma unroll
  for (int j = 0; j < FX_RV_NC; ++j) {
    clen[j] = g[1 + j]; coff[j] = off;
    ok = ok && clen[j] >= 1 && clen[j] <= lds_floats;        // bounded before it is summed: `off` cannot overflow
    off += ok ? clen[j] : 0;
    blk = clen[j] < blk ? clen[j] : blk;
  }
#pragma unroll
  for (int j = 0; j < FX_RV_NA; ++j) {
    alen[j] = g[1 + FX_RV_NC + j]; aoff[j] = off;
    ok = ok && alen[j] >= 1 && alen[j] <= lds_floats;
    off += ok ? alen[j] : 0;
    blk = alen[j] < blk ? alen[j] : blk;
  }
  if (!ok || off > lds_floats) {                 // a plan the launch cannot hold: a loud result, never an access outside the arena
    for (int64_t n = lane; n < T; n += 64) wr[n] = __builtin_nanf("");
    return;
  }
  const float* xr = x + row * T;
  const float fbk = cf[0], damp = cf[1], gain = cf[2];
  for (int i = lane; i < off; i += 64) sox_arena[i] = 0.f;
  float last[FX_RV_NC];
  int cpos[FX_RV_NC], apos[FX_RV_NA];
#pragma unroll
  for (int j = 0; j < FX_RV_NC; ++j) { last[j] = 0.f; cpos[j] = 0; }
#pragma unroll
  for (int j = 0; j < FX_RV_NA; ++j) apos[j] = 0;
  float dpw[6];
  dpw[0] = damp;
#pragma unroll
  for (int s = 1; s < 6; ++s) dpw[s] = dpw[s - 1] * dpw[s - 1];
  const float dl1 = powf(damp, (float)(lane + 1));
  const bool in_blk = lane < blk;
  __syncthreads();
  for (int64_t n0 = 0; n0 < T; n0 += blk) {
    const int64_t n = n0 + lane;
    const bool act = in_blk && n < T;
    const float in = act && n >= delay ? fminf(fmaxf(xr[n - delay], -1.0f), 1.0f) : 0.f;
    float out = 0.f;
#pragma unroll
    for (int j = FX_RV_NC - 1; j >= 0; --j) {
      float* buf = sox_arena + coff[j];
      int idx = cpos[j] + lane;
      idx -= idx >= clen[j] ? clen[j] : 0;
      const float o = in_blk ? buf[idx] : 0.f;
      // store[i] = (1 - damp) o[i] + damp store[i - 1]: inclusive weighted scan; lanes beyond the block hold zeros and feed no lane below
      float v = (1.0f - damp) * o;
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        const float u = __shfl_up(v, 1 << s, 64);
        if (lane >= (1 << s)) v = fmaf(dpw[s], u, v);
      }
      v = fmaf(dl1, last[j], v);
      if (in_blk) buf[idx] = in + v * fbk;     // lanes beyond T store values (in = 0) that no sample below T reads back
      last[j] = __shfl(v, blk - 1, 64);
      cpos[j] += blk;
      cpos[j] -= cpos[j] >= clen[j] ? clen[j] : 0;
      out += o;
    }
#pragma unroll
    for (int j = FX_RV_NA - 1; j >= 0; --j) {
      float* buf = sox_arena + aoff[j];
      int idx = apos[j] + lane;
      idx -= idx >= alen[j] ? alen[j] : 0;
      const float o = in_blk ? buf[idx] : 0.f;
      if (in_blk) buf[idx] = out + 0.5f * o;
      out = o - out;
      apos[j] += blk;
      apos[j] -= apos[j] >= alen[j] ? alen[j] : 0;
    }
    if (act) wr[n] = out * gain;
  }
}
// y: (B, 2, T).  The banks of clip b are workspace rows ((b Cin + c) 2 + w); wet_dry is read from the clip's first bank.
__global__ __launch_bounds__(256) void fx_sox_mix_kernel(const float* __restrict__ x, const float* __restrict__ ws, float* __restrict__ y,
                                                         int Cin, int64_t T, const float* __restrict__ coef) {
  const int b = blockIdx.y >> 1, w = blockIdx.y & 1;
  const float wd = coef[(int64_t)b * Cin * 2 * FX_SOX_COEF + 3], dry = 1.0f - wd;
  const float* xr = x + ((int64_t)b * Cin + (w < Cin ? w : Cin - 1)) * T;
  const float* w0 = ws + ((int64_t)b * Cin * 2 + w) * T;
  const float* w1 = w0 + 2 * T;
  float* yr = y + ((int64_t)b * 2 + w) * T;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < T; n += (int64_t)gridDim.x * 256) {
    float wet = w0[n];
    if (Cin == 2) wet = 0.5f * (wet + w1[n]);
    wet = wet > 1.0f ? 1.0f : (wet < -1.0f ? -1.0f : wet);            // a NaN (refused plan) stays a NaN
    yr[n] = xr[n] * dry + wet * wd;
  }
}

// ---- BS.1770 integrated loudness (pyloudnorm.Meter.integrated_loudness) + gain --------------------------------------
// K-weighting = two biquads in series evaluated in fp64 (scipy.signal.lfilter on float64).  A 4th-order LINEAR recurrence:
// the clip is cut into 64 chunks, one lane each.  Pass 1: every lane filters its chunk from a ZERO state and keeps the
// final state; the true initial states follow from s_k = M s_(k-1) + z_k with M = (state transition)^chunk (4 x 4, from the
// host); pass 2 re-filters with the right initial state and accumulates the squared output into 100 ms hop sums.
// The gating (400 ms blocks, 75 % overlap, -70 LUFS absolute and -10 LU relative gates) runs on the ~55 hop sums.
struct FxLoudArgs {
  const float* x;
  double* hop;            // (B, nhop) sums of squares of the K-weighted signal per hop (zeroed by the caller)
  int64_t T;
  int chunk, nhop;
  const int32_t* hop_of;  // not used: hops are uniform (hop_len) except that block bounds come from blk_lo / blk_hi
  int hop_len;
  double b1[3], a1[3], b2[3], a2[3];     // normalised (a[0] = 1)
  double M[16];                          // state transition of `chunk` samples, row-major 4 x 4 (states: s1a, s1b, s2a, s2b)
};
// transposed direct form II (scipy lfilter): y = b0 x + s0; s0 = b1 x - a1 y + s1; s1 = b2 x - a2 y
__device__ __forceinline__ double fx_biquad(const double* b, const double* a, double x, double& s0, double& s1) {
  const double y = b[0] * x + s0;
  s0 = b[1] * x - a[1] * y + s1;
  s1 = b[2] * x - a[2] * y;
  return y;
}
__global__ __launch_bounds__(64) void fx_kweight_kernel(const FxLoudArgs a) {
  __shared__ double st[64][4];
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* xr = a.x + (int64_t)b * a.T;
  const int64_t lo = (int64_t)lane * a.chunk, hi = lo + a.chunk < a.T ? lo + a.chunk : a.T;
  double s[4] = {0, 0, 0, 0};
  for (int64_t n = lo; n < hi; ++n) {
    const double v = fx_biquad(a.b1, a.a1, (double)xr[n], s[0], s[1]);
    fx_biquad(a.b2, a.a2, v, s[2], s[3]);
  }
  // chunks shorter than `chunk` (the tail) would need their own transition; only the LAST non-empty chunk can be short and
  // its end state is never used
#pragma unroll
  for (int i = 0; i < 4; ++i) st[lane][i] = s[i];
  __syncthreads();
  if (lane == 0) {                       // 64 tiny 4x4 steps: true state at the START of every chunk
    double cur[4] = {0, 0, 0, 0};
    for (int k = 0; k < 64; ++k) {
      double z[4], nxt[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { z[i] = st[k][i]; st[k][i] = cur[i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double acc = z[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += a.M[i * 4 + j] * cur[j];
        nxt[i] = acc;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = st[lane][i];
  double acc = 0.0;
  int64_t h = lo / a.hop_len;
  int64_t hend = (h + 1) * a.hop_len;
  double* hp = a.hop + (int64_t)b * a.nhop;
  for (int64_t n = lo; n < hi; ++n) {
    if (n == hend) {
      if (h < a.nhop) atomicAdd(hp + h, acc);
      acc = 0.0; ++h; hend += a.hop_len;
    }
    const double v = fx_biquad(a.b1, a.a1, (double)xr[n], s[0], s[1]);
    const double w = fx_biquad(a.b2, a.a2, v, s[2], s[3]);
    acc += w * w;
  }
  if (hi > lo && h < a.nhop) atomicAdd(hp + h, acc);
}
// gating on the hop sums; gain[b] = 10^(clamp(target - L, -120, 40) / 20).  One thread per clip.  A clip of C channels owns C
// consecutive rows of hop sums: pyloudnorm's multichannel block power is the sum of the channels' mean squares (weight 1 for L, R).
__device__ __forceinline__ double fx_hop_sum(const double* hp, int nhop, int C, int j) {
  double h = hp[j];
  for (int c = 1; c < C; ++c) h += hp[(int64_t)c * nhop + j];
  return h;
}
__global__ void fx_loud_gate_kernel(const double* __restrict__ hop, int B, int C, int nhop, int nblk, double inv_block, float target,
                                    float* __restrict__ lufs, float* __restrict__ gain) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* hp = hop + (int64_t)b * C * nhop;
  // block j = hops j .. j + 3 (400 ms at 75 % overlap)
  double s1 = 0.0; int n1 = 0;
  for (int j = 0; j < nblk; ++j) {
    const double z = (fx_hop_sum(hp, nhop, C, j) + fx_hop_sum(hp, nhop, C, j + 1) + fx_hop_sum(hp, nhop, C, j + 2) +
                      fx_hop_sum(hp, nhop, C, j + 3)) * inv_block;
    const double l = -0.691 + 10.0 * log10(z);
    if (l >= -70.0) { s1 += z; ++n1; }
  }
  double L;
  if (n1 == 0) L = -INFINITY;
  else {
    const double gamma_r = -0.691 + 10.0 * log10(s1 / n1) - 10.0;
    double s2 = 0.0; int n2 = 0;
    for (int j = 0; j < nblk; ++j) {
      const double z = (fx_hop_sum(hp, nhop, C, j) + fx_hop_sum(hp, nhop, C, j + 1) + fx_hop_sum(hp, nhop, C, j + 2) +
                        fx_hop_sum(hp, nhop, C, j + 3)) * inv_block;
      const double l = -0.691 + 10.0 * log10(z);
      if (l > gamma_r && l > -70.0) { s2 += z; ++n2; }
    }
    L = n2 ? -0.691 + 10.0 * log10(s2 / n2) : -INFINITY;
  }
  lufs[b] = (float)L;
  float d = target - (float)L;
  d = fminf(fmaxf(d, -120.0f), 40.0f);
  gain[b] = powf(10.0f, d / 20.0f);
}
__global__ __launch_bounds__(256) void fx_scale_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t T,
                                                       const float* __restrict__ gain, const int32_t* __restrict__ rows) {
  const int b = blockIdx.y;
  const float g = gain[b];
  const float* xr = x + (int64_t)b * T;
  float* yr = y + fx_row(rows, b) * T;          // gain[i] * x[i] -> y[rows[i]]
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < T; n += (int64_t)gridDim.x * 256) yr[n] = g * xr[n];
}

// ---- parametric EQ (reference parametric_eq: low shelf -> N peaking bands -> high shelf, RBJ biquads, lfilter in fp64) ------
// A cascade of NS = N + 2 biquads in transposed direct form II, fp64, rounded to fp32 at the end: an order-2 NS linear recurrence,
// blocked like fx_kweight_kernel.  64 chunks per row, one lane each: pass 1 filters every chunk from a zero state; the true start
// state of every chunk follows from s_k = M s_(k-1) + z_k with the row's own M = A^chunk (2 NS x 2 NS, from the host), one lane per
// state component; pass 2 re-filters from the right state and stores.  Only the last non-empty chunk can be short, and its end
// state is never used.  coef per row: NS x {b0, b1, b2, a1, a2} (a0 = 1), then M row-major.
#define FX_EQ_MAX_NS 8
__device__ __forceinline__ double fx_biquad5(const double* c, double x, double& s0, double& s1) {
  const double y = c[0] * x + s0;
  s0 = c[1] * x - c[3] * y + s1;
  s1 = c[2] * x - c[4] * y;
  return y;
}
template <int NS>
__global__ __launch_bounds__(64) void fx_eq_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t T, int chunk,
                                                   const double* __restrict__ coef) {
  constexpr int D = 2 * NS, CS = 5 * NS + D * D;
  __shared__ double st[64][D];
  const int row = blockIdx.x, lane = threadIdx.x;
  const double* cr = coef + (int64_t)row * CS;
  double c[5 * NS];
#pragma unroll
  for (int i = 0; i < 5 * NS; ++i) c[i] = cr[i];
  const float* xr = x + (int64_t)row * T;
  float* yr = y + (int64_t)row * T;
  const int64_t lo = (int64_t)lane * chunk, hi = lo + chunk < T ? lo + chunk : T;
  double s[D];
#pragma unroll
  for (int i = 0; i < D; ++i) s[i] = 0.0;
  for (int64_t n = lo; n < hi; ++n) {
    double v = (double)xr[n];
#pragma unroll
    for (int k = 0; k < NS; ++k) v = fx_biquad5(c + 5 * k, v, s[2 * k], s[2 * k + 1]);
  }
#pragma unroll
  for (int i = 0; i < D; ++i) st[lane][i] = s[i];
  __syncthreads();
  {
    // lane i < D carries component i of the running state; lanes >= D shadow lane 0 and store nothing
    const int i = lane < D ? lane : 0;
    double m[D];
#pragma unroll
    for (int j = 0; j < D; ++j) m[j] = cr[5 * NS + i * D + j];
    double cur = 0.0;
    for (int k = 0; k < 64; ++k) {
      double acc = st[k][i];
      if (lane < D) st[k][i] = cur;
#pragma unroll
      for (int j = 0; j < D; ++j) acc += m[j] * __shfl(cur, j, 64);
      cur = acc;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < D; ++i) s[i] = st[lane][i];
  for (int64_t n = lo; n < hi; ++n) {
    double v = (double)xr[n];
#pragma unroll
    for (int k = 0; k < NS; ++k) v = fx_biquad5(c + 5 * k, v, s[2 * k], s[2 * k + 1]);
    yr[n] = (float)v;
  }
}

// ---- stereo widener (reference stereo_widener, fp32 torch) on (2, T) clips ---------------------------------------------------
//   mid = (l + r) / sqrt2;  side = (l - r) / sqrt2;  mid *= 2 (1 - w);  side *= 2 w;  l' = (mid + side) / sqrt2;  r' = (mid - side) / sqrt2
// The reference's operation order and roundings: correctly rounded divisions by fp32(sqrt2), every product rounded before the
// following add.  -ffp-contract=fast fuses across a `fp contract(off)` pragma and the _rn intrinsics alike (mid * gm + side
// became one fma: 1-ulp differences that the cancellation in mid - side grew to thousands of ulps), so the products pass through
// fx_rounded, an empty asm the combiner cannot look through.  16-byte vectors.
__device__ __forceinline__ float fx_rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ void fx_widen(float l, float r, float gm, float gs, float& ol, float& orr) {
  const float r2 = 1.41421356237309515f;
  const float mid = fx_rounded(((l + r) / r2) * gm), side = fx_rounded(((l - r) / r2) * gs);
  ol = (mid + side) / r2;
  orr = (mid - side) / r2;
}
__global__ __launch_bounds__(256) void fx_widener_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t T,
                                                         const float* __restrict__ g_mid, const float* __restrict__ g_side) {
  const int b = blockIdx.y;
  const float gm = g_mid[b], gs = g_side[b];
  const float* xl = x + (int64_t)b * 2 * T;
  const float* xr = xl + T;
  float* yl = y + (int64_t)b * 2 * T;
  float* yr = yl + T;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < T; i += (int64_t)gridDim.x * 1024) {
    if (i + 3 < T) {
      const f32x4 l = rfx_ld4(xl + i), r = rfx_ld4(xr + i);
      f32x4 ol, orr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float a, c;
        fx_widen(l[j], r[j], gm, gs, a, c);
        ol[j] = a;
        orr[j] = c;
      }
      rfx_st4(yl + i, ol);
      rfx_st4(yr + i, orr);
    } else {
      for (int64_t k = i; k < T; ++k) fx_widen(xl[k], xr[k], gm, gs, yl[k], yr[k]);
    }
  }
}

// ---- volume automation (reference RandomVolumeAutomation): piecewise-linear dB ramps, applied IN PLACE -------------------------
// Per row a table of S segments (end sample, start dB, end dB), contiguous from sample 0; samples past the last end keep 0 dB
// (gain 1: left untouched).  The dB value of a sample follows torch.linspace's fp32 formula, step = (end - start) / (steps - 1),
// start + step i in the first half and end - step (steps - 1 - i) in the second; then x *= 10^(dB / 20).
#define FX_VOL_MAXSEG 64
__global__ __launch_bounds__(256) void fx_volume_kernel(float* __restrict__ x, int64_t T, int S, const int32_t* __restrict__ seg_end,
                                                        const float* __restrict__ db_start, const float* __restrict__ db_end) {
  __shared__ int64_t se[FX_VOL_MAXSEG];
  __shared__ float sa[FX_VOL_MAXSEG], sb[FX_VOL_MAXSEG];
  const int b = blockIdx.y;
  if (threadIdx.x < S) {
    se[threadIdx.x] = seg_end[b * S + threadIdx.x];
    sa[threadIdx.x] = db_start[b * S + threadIdx.x];
    sb[threadIdx.x] = db_end[b * S + threadIdx.x];
  }
  __syncthreads();
  const int64_t filled = se[S - 1] < T ? se[S - 1] : T;
  float* xr = x + (int64_t)b * T;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < filled; n += (int64_t)gridDim.x * 256) {
    int s = 0;
    while (n >= se[s]) ++s;                 // n < se[S - 1]: ends at s <= S - 1; zero-length segments are skipped
    const int64_t lo = s ? se[s - 1] : 0, steps = se[s] - lo, i = n - lo;
    const float st = sa[s], en = sb[s];
    float v = st;
    if (steps > 1) {
      const float step = (en - st) / (float)(steps - 1);
      v = i < steps / 2 ? st + step * (float)i : en - step * (float)(steps - i - 1);     // fused: within an ulp of torch's dB
    }
    xr[n] = xr[n] * powf(10.0f, v / 20.0f);
  }
}

// ---- phaser: JUCE dsp::Phaser (pedalboard.Phaser) ------------------------------------------------------------------------------
//   every 4th sample (m = n / 4): lfo = sin(2 pi rate m / (sr / 4) - pi) depth / 2;  f = mapToLog10(clamp(lfo + normCentre, 0, 1),
//   20, fmax), fmax = min(20000, 0.49 sr);  G = g / (1 + g), g = tan(pi f / sr)
//   u = x[n] - fb out[n - 1];  6 first-order TPT all-passes: v = G (u - s), y = v + s, s = y + v, u = 2 y - u;  out = u
//   y[n] = (1 - mix) x[n] + mix out
// Pass 1 (coalesced): the coefficient stream G[m] of every row, evaluated in fp64 and rounded to fp32.  Pass 2: one LANE per row
// walks the one-sample feedback loop (a linear but time-varying recurrence); like the compressor envelope, the loads of 32
// samples and their 8 coefficients are issued ahead of the chain.  Rows are padded to a multiple of 8 coefficients.
__global__ __launch_bounds__(256) void fx_phaser_coef_kernel(float* __restrict__ G, int64_t M, int64_t Mpad, float sr,
                                                             const float* __restrict__ rate, const float* __restrict__ depth,
                                                             const float* __restrict__ centre) {
  const int b = blockIdx.y;
  const double pi = 3.14159265358979323846;
  const double fhi = fmin(20000.0, 0.49 * (double)sr), lmin = log10(20.0), lmax = log10(fhi);
  const double nc = (log10((double)centre[b]) - lmin) / (lmax - lmin);
  const double winc = 2.0 * pi * (double)rate[b] / ((double)sr / 4.0), dep = 0.5 * (double)depth[b];
  float* gr = G + (int64_t)b * Mpad;
  for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    double ph = winc * (double)m;
    ph -= floor(ph * (0.5 / pi)) * (2.0 * pi);
    const double v = fmin(fmax(sin(ph - pi) * dep + nc, 0.0), 1.0);
    const double g = tan(pi * (20.0 * pow(fhi / 20.0, v)) / (double)sr);
    gr[m] = (float)(g / (1.0 + g));
  }
}
__device__ __forceinline__ float fx_phaser_step(float xv, float g, float (&s)[6], float& last, float fb, float mix, float dry) {
  float u = xv - last;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float v = g * (u - s[k]);
    const float yk = v + s[k];
    s[k] = yk + v;
    u = 2.0f * yk - u;
  }
  last = u * fb;
  return u * mix + xv * dry;
}
__global__ __launch_bounds__(64) void fx_phaser_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ G,
                                                       int B, int64_t T, int64_t Mpad, const float* __restrict__ fb,
                                                       const float* __restrict__ mix) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const float f = fb[b], m = mix[b], dry = 1.0f - m;
  const float* xr = x + (int64_t)b * T;
  const float* gr = G + (int64_t)b * Mpad;
  float* yr = y + (int64_t)b * T;
  float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float last = 0.f;
  int64_t n = 0;
  for (; n + 32 <= T; n += 32) {
    f32x4 v[8], g[2];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = rfx_ld4(xr + n + 4 * q);
    g[0] = rfx_ld4(gr + n / 4);
    g[1] = rfx_ld4(gr + n / 4 + 4);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = fx_phaser_step(v[q][j], g[q >> 2][q & 3], s, last, f, m, dry);
      rfx_st4(yr + n + 4 * q, o);
    }
  }
  for (; n < T; ++n) yr[n] = fx_phaser_step(xr[n], gr[n / 4], s, last, f, m, dry);
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------
static dim3 fx_grid(int64_t T, int B, int per_block) {
  int64_t gx = (T + per_block - 1) / per_block;
  if (gx > 2048) gx = 2048;
  if (gx < 1) gx = 1;
  return dim3((unsigned)gx, (unsigned)B);
}
static bool fx_geometry_ok(int B, int64_t T) { return B > 0 && B <= 65535 && T > 0; }
static bool fx_ok(const void* x, const void* y, int B, int64_t T) { return x && y && fx_geometry_ok(B, T); }
// floats of one (B, T) envelope image: env_ws of the compressor; the limiter's ws holds two (stage 2's envelope, stage 1's output)
static int64_t fx_env_floats(int B, int64_t T) { return (int64_t)B * T; }

extern "C" int rfx_fx_distortion(const float* x, float* y, int32_t B, int64_t T, const float* gain, void* stream) {
  if (!fx_ok(x, y, B, T) || !gain) return -1;
  hipLaunchKernelGGL(fx_distortion_kernel, fx_grid(T, B, 1024), dim3(256), 0, (hipStream_t)stream, x, y, T, gain);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_fx_delay(const float* x, float* y, int32_t B, int64_t T, const int32_t* delay_samples, const float* feedback,
                            const float* mix, void* stream) {
  if (!fx_ok(x, y, B, T) || !delay_samples || !feedback || !mix || x == y) return -1;
  hipLaunchKernelGGL(fx_delay_kernel, fx_grid(T, B, 256), dim3(256), 0, (hipStream_t)stream, x, y, T, delay_samples, feedback, mix);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_fx_chorus(const float* x, float* y, int32_t B, int64_t T, float sample_rate, const float* rate_hz,
                             const float* depth, const float* centre_delay_ms, const float* feedback, const float* mix,
                             void* stream) {
  if (!fx_ok(x, y, B, T) || !rate_hz || !depth || !centre_delay_ms || !feedback || !mix || sample_rate < 4000.f) return -1;
  // blocks no longer than the 1 ms floor of the modulated delay minus the interpolation tap; the ring must hold the longest
  // delay the reference's ranges allow (centre + 20 ms * depth / 2, plus a block)
  int blk = (int)(sample_rate / 1000.0f) - 2;
  blk = blk > 64 ? 64 : blk;
  if (blk < 1 || (int)(sample_rate * 0.05f) + 66 > FX_CH_RING) return -1;
  hipLaunchKernelGGL(fx_chorus_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, x, y, T, sample_rate, rate_hz, depth,
                     centre_delay_ms, feedback, mix, blk);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int64_t rfx_fx_compressor_ws(int32_t B, int64_t T) { return fx_geometry_ok(B, T) ? fx_env_floats(B, T) : -1; }
extern "C" int rfx_fx_compressor(const float* x, float* y, float* env_ws, int32_t B, int64_t T, const float* threshold_lin,
                                 const float* ratio, const float* c_attack, const float* c_release, void* stream) {
  if (!fx_ok(x, y, B, T) || !env_ws || !threshold_lin || !ratio || !c_attack || !c_release) return -1;
  hipLaunchKernelGGL(fx_comp_env_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, x, env_ws, B, T, c_attack, c_release);
  hipLaunchKernelGGL(fx_comp_gain_kernel, fx_grid(T, B, 256), dim3(256), 0, (hipStream_t)stream, x, env_ws, y, T, threshold_lin, ratio);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_fx_reverb(const float* x, float* y, int32_t B, int64_t T, int32_t sample_rate, const float* damp,
                             const float* feedback, const float* wet1, const float* dry, void* stream) {
  // 12544 ... 143526 Hz: below, the shortest ring (225 * sr / 44100) is under one 64-sample block; above, the twelve rings
  // (12587 * sr / 44100 floats) exceed 160 KB of LDS.  The per-ring and arena checks below are what decides.
  if (!fx_ok(x, y, B, T) || !damp || !feedback || !wet1 || !dry || sample_rate < 12544 || sample_rate > 143526) return -1;
  static const int comb_t[FX_RV_NC] = {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617};
  static const int ap_t[FX_RV_NA] = {556, 441, 341, 225};
  FxReverbArgs a{};
  a.x = x; a.y = y; a.T = T; a.damp = damp; a.feedback = feedback; a.wet1 = wet1; a.dry = dry;
  int off = 0;
  for (int j = 0; j < FX_RV_NC; ++j) {
    a.comb_len[j] = (int)(((int64_t)sample_rate * comb_t[j]) / 44100);
    if (a.comb_len[j] < 64) return -1;
    a.comb_off[j] = off; off += a.comb_len[j];
  }
  for (int j = 0; j < FX_RV_NA; ++j) {
    a.ap_len[j] = (int)(((int64_t)sample_rate * ap_t[j]) / 44100);
    if (a.ap_len[j] < 64) return -1;
    a.ap_off[j] = off; off += a.ap_len[j];
  }
  a.arena = off;
  const size_t lds = sizeof(float) * (size_t)off;
  if (lds > 160 * 1024) return -1;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(fx_reverb_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess) return -3;
  hipLaunchKernelGGL(fx_reverb_kernel, dim3(B), dim3(64), lds, (hipStream_t)stream, a);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int64_t rfx_fx_sox_reverb_ws_floats(int32_t B, int32_t Cin, int64_t T) { return (int64_t)B * Cin * 2 * T; }
extern "C" int rfx_fx_sox_reverb(const float* x, float* y, float* ws, int32_t B, int32_t Cin, int64_t T, const int32_t* geom,
                                 const float* coef, int32_t lds_floats, void* stream) {
  if (!fx_ok(x, y, B, T) || !ws || !geom || !coef || x == y || (Cin != 1 && Cin != 2) || B > 32767 || lds_floats < FX_RV_NC + FX_RV_NA)
    return -1;
  const size_t lds = sizeof(float) * (size_t)lds_floats;
  if (lds > 160 * 1024) return -1;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(fx_sox_bank_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess) return -3;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fx_sox_bank_kernel, dim3(B * Cin * 2), dim3(64), lds, s, x, ws, T, geom, coef, lds_floats, (int64_t)B * Cin);
  hipLaunchKernelGGL(fx_sox_mix_kernel, fx_grid(T, 2 * B, 256), dim3(256), 0, s, x, ws, y, Cin, T, coef);
  RFX_CHECK_LAUNCH();
  return 0;
}
// doubles of hop_ws: nhop hop sums per row of the K-weighting pass; -1: geometry the launcher refuses
static int64_t fx_hop_doubles(int32_t B, int32_t C, int64_t T, int32_t chunk, int32_t hop_len, int32_t nhop, int32_t nblk) {
  if (B <= 0 || C <= 0 || (int64_t)B * C > 65535 || T <= 0 || chunk <= 0 || hop_len <= 0 || nhop < 4 || nblk < 1 || nblk + 3 > nhop ||
      (int64_t)chunk * 64 < T) return -1;
  return (int64_t)B * C * nhop;
}
extern "C" int64_t rfx_fx_loudness_ws(int32_t B, int64_t T, int32_t chunk, int32_t hop_len, int32_t nhop, int32_t nblk) {
  return fx_hop_doubles(B, 1, T, chunk, hop_len, nhop, nblk);
}
extern "C" int64_t rfx_fx_loudness_joint_ws(int32_t B, int32_t C, int64_t T, int32_t chunk, int32_t hop_len, int32_t nhop, int32_t nblk) {
  return fx_hop_doubles(B, C, T, chunk, hop_len, nhop, nblk);
}
// B clips of C channels: the K-weighting runs over all B * C rows, the gate sums each clip's C rows of hop sums
static int fx_loudness(const float* x, int32_t B, int32_t C, int64_t T, int32_t chunk, int32_t hop_len, int32_t nhop, int32_t nblk,
                       double inv_block, const double* coef, float target_lufs, double* hop_ws, float* lufs, float* gain,
                       void* stream) {
  const int64_t hop_doubles = fx_hop_doubles(B, C, T, chunk, hop_len, nhop, nblk);
  if (!x || !coef || !hop_ws || !lufs || !gain || hop_doubles < 0) return -1;
  FxLoudArgs a{};
  a.x = x; a.hop = hop_ws; a.T = T; a.chunk = chunk; a.nhop = nhop; a.hop_len = hop_len; a.hop_of = nullptr;
  for (int i = 0; i < 3; ++i) { a.b1[i] = coef[i]; a.a1[i] = coef[3 + i]; a.b2[i] = coef[6 + i]; a.a2[i] = coef[9 + i]; }
  for (int i = 0; i < 16; ++i) a.M[i] = coef[12 + i];
  const int rows = B * C;
  if (hipMemsetAsync(hop_ws, 0, sizeof(double) * (size_t)hop_doubles, (hipStream_t)stream) != hipSuccess) return -3;
  hipLaunchKernelGGL(fx_kweight_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(fx_loud_gate_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, hop_ws, B, C, nhop, nblk, inv_block,
                     target_lufs, lufs, gain);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_fx_loudness(const float* x, int32_t B, int64_t T, int32_t chunk, int32_t hop_len, int32_t nhop, int32_t nblk,
                               double inv_block, const double* coef /* b1[3] a1[3] b2[3] a2[3] M[16] on the HOST */,
                               float target_lufs, double* hop_ws, float* lufs, float* gain, void* stream) {
  return fx_loudness(x, B, 1, T, chunk, hop_len, nhop, nblk, inv_block, coef, target_lufs, hop_ws, lufs, gain, stream);
}
extern "C" int rfx_fx_loudness_joint(const float* x, int32_t B, int32_t C, int64_t T, int32_t chunk, int32_t hop_len, int32_t nhop,
                                     int32_t nblk, double inv_block, const double* coef, float target_lufs, double* hop_ws, float* lufs,
                                     float* gain, void* stream) {
  return fx_loudness(x, B, C, T, chunk, hop_len, nhop, nblk, inv_block, coef, target_lufs, hop_ws, lufs, gain, stream);
}
extern "C" int64_t rfx_fx_limiter_ws(int32_t B, int64_t T) { return fx_geometry_ok(B, T) ? 2 * fx_env_floats(B, T) : -1; }
extern "C" int rfx_fx_limiter(const float* x, float* y, float* ws, int32_t B, int64_t T, const float* params, void* stream) {
  if (!fx_ok(x, y, B, T) || !ws || !params) return -1;
  const float* p[9];
  for (int i = 0; i < 9; ++i) p[i] = params + (size_t)i * B;   // thr1 ratio1 ca1 cr1 thr2 ratio2 ca2 cr2 makeup
  float* env = ws;
  float* y1 = ws + fx_env_floats(B, T);
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fx_comp_env_kernel, dim3((B + 63) / 64), dim3(64), 0, s, x, env, B, T, p[2], p[3]);
  hipLaunchKernelGGL(fx_comp_gain_kernel, fx_grid(T, B, 256), dim3(256), 0, s, x, env, y1, T, p[0], p[1]);
  hipLaunchKernelGGL(fx_comp_env_kernel, dim3((B + 63) / 64), dim3(64), 0, s, y1, env, B, T, p[6], p[7]);
  hipLaunchKernelGGL(fx_limit_out_kernel, fx_grid(T, B, 256), dim3(256), 0, s, y1, env, y, T, p[4], p[5], p[8]);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_fx_eq(const float* x, float* y, int32_t B, int64_t T, int32_t nsec, int32_t chunk, const double* coef, void* stream) {
  if (!fx_ok(x, y, B, T) || !coef || chunk <= 0 || (int64_t)chunk * 64 < T) return -1;
  const hipStream_t s = (hipStream_t)stream;
  switch (nsec) {
    case 2: hipLaunchKernelGGL(fx_eq_kernel<2>, dim3(B), dim3(64), 0, s, x, y, T, chunk, coef); break;
    case 3: hipLaunchKernelGGL(fx_eq_kernel<3>, dim3(B), dim3(64), 0, s, x, y, T, chunk, coef); break;
    case 4: hipLaunchKernelGGL(fx_eq_kernel<4>, dim3(B), dim3(64), 0, s, x, y, T, chunk, coef); break;
    case 5: hipLaunchKernelGGL(fx_eq_kernel<5>, dim3(B), dim3(64), 0, s, x, y, T, chunk, coef); break;
    case 6: hipLaunchKernelGGL(fx_eq_kernel<6>, dim3(B), dim3(64), 0, s, x, y, T, chunk, coef); break;
    case 7: hipLaunchKernelGGL(fx_eq_kernel<7>, dim3(B), dim3(64), 0, s, x, y, T, chunk, coef); break;
    case FX_EQ_MAX_NS: hipLaunchKernelGGL(fx_eq_kernel<FX_EQ_MAX_NS>, dim3(B), dim3(64), 0, s, x, y, T, chunk, coef); break;
    default: return -1;
  }
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_fx_widener(const float* x, float* y, int32_t B, int64_t T, const float* g_mid, const float* g_side, void* stream) {
  if (!fx_ok(x, y, B, T) || !g_mid || !g_side) return -1;
  hipLaunchKernelGGL(fx_widener_kernel, fx_grid(T, B, 1024), dim3(256), 0, (hipStream_t)stream, x, y, T, g_mid, g_side);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_fx_volume(float* x, int32_t B, int64_t T, int32_t S, const int32_t* seg_end, const float* db_start,
                             const float* db_end, void* stream) {
  if (!fx_ok(x, x, B, T) || !seg_end || !db_start || !db_end || S < 1 || S > FX_VOL_MAXSEG) return -1;
  hipLaunchKernelGGL(fx_volume_kernel, fx_grid(T, B, 256), dim3(256), 0, (hipStream_t)stream, x, T, S, seg_end, db_start, db_end);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int64_t rfx_fx_phaser_ws_floats(int32_t B, int64_t T) { return (int64_t)B * ((((T + 3) / 4) + 7) / 8 * 8); }
extern "C" int rfx_fx_phaser(const float* x, float* y, float* ws, int32_t B, int64_t T, float sample_rate, const float* rate_hz,
                             const float* depth, const float* centre_hz, const float* feedback, const float* mix, void* stream) {
  if (!fx_ok(x, y, B, T) || !ws || !rate_hz || !depth || !centre_hz || !feedback || !mix || sample_rate <= 0.f) return -1;
  const int64_t M = (T + 3) / 4, Mpad = (M + 7) / 8 * 8;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fx_phaser_coef_kernel, fx_grid(M, B, 256), dim3(256), 0, s, ws, M, Mpad, sample_rate, rate_hz, depth, centre_hz);
  hipLaunchKernelGGL(fx_phaser_kernel, dim3((B + 63) / 64), dim3(64), 0, s, x, y, ws, B, T, Mpad, feedback, mix);
  RFX_CHECK_LAUNCH();
  return 0;
}
extern "C" int rfx_fx_scale(const float* x, float* y, int32_t B, int64_t T, const float* gain, void* stream) {
  if (!fx_ok(x, y, B, T) || !gain) return -1;
  hipLaunchKernelGGL(fx_scale_kernel, fx_grid(T, B, 256), dim3(256), 0, (hipStream_t)stream, x, y, T, gain, nullptr);
  RFX_CHECK_LAUNCH();
  return 0;
}
// The normalisation of a round of batched dataset rendering: measure the n compact rows of x (the K-weighting and gate kernels
// above, unchanged), then store gain[i] * x[i] into row rows[i] of the (N, T) buffer y (device int32 table; the CALLER guarantees
// 0 <= rows[i] < N and that no row occurs twice; rows == nullptr: row i).  Every addressed row of y is written exactly once, the
// others are not touched.  ws: rfx_fx_normalize_ws_bytes(n, nhop) bytes = n * nhop hop sums (double), then lufs[n] and gain[n] (float), which
// stay readable there after the call.
extern "C" int64_t rfx_fx_normalize_ws_bytes(int32_t n, int32_t nhop) {
  return (int64_t)n * nhop * (int64_t)sizeof(double) + 2 * (int64_t)n * (int64_t)sizeof(float);
}
extern "C" int rfx_fx_normalize_rows(const float* x, float* y, const int32_t* rows, int32_t n, int64_t T, int32_t chunk,
                                     int32_t hop_len, int32_t nhop, int32_t nblk, double inv_block, const double* coef,
                                     float target_lufs, void* ws, void* stream) {
  if (!fx_ok(x, y, n, T) || !ws || (rows && x == y)) return -1;
  double* hop_ws = (double*)ws;
  float* lufs = (float*)(hop_ws + (size_t)n * (nhop > 0 ? nhop : 0));
  float* gain = lufs + n;
  const int rc = fx_loudness(x, n, 1, T, chunk, hop_len, nhop, nblk, inv_block, coef, target_lufs, hop_ws, lufs, gain, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(fx_scale_kernel, fx_grid(T, n, 256), dim3(256), 0, (hipStream_t)stream, x, y, T, gain, rows);
  RFX_CHECK_LAUNCH();
  return 0;
}
