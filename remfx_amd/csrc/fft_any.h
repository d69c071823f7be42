// Generic framed real FFT (csrc/fft_any.hip): every power-of-two n_fft from 16 to 32768 that csrc/fft.hip has no kernel for.
// Internal to the library: rfx_fft_analysis / rfx_fft_synthesis / rfx_fft_synthesis_ws (csrc/fft.hip) forward here.
#pragma once
#include "remfx_hip.h"

bool fft_any_covers(const rfx_stft_desc* d);                  // n_fft = 2^k, 16 <= n_fft <= 32768, not 512 / 1024 / 2048 / 4096
int64_t fft_any_synthesis_ws(const rfx_stft_desc* d);         // floats of frame scratch: R * frames_out * n_fft
int fft_any_analysis(const rfx_stft_desc* d, const float* x, const float* window, const float* mul, float* out, void* stream);
int fft_any_synthesis(const rfx_stft_desc* d, const float* spec, const float* window, const float* mul, float* ws, float* out,
                      void* stream);
