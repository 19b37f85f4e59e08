// The decoders' non-GEMM kernels: the NSF source, noise conv, conv_post and z_p sampling (nsf_source.hip), the
// per-sample harmonic source (source_harm.hip) and RefineGAN's resampling and AdaIN (refinegan.hip)
#pragma once
#include "kernel_base.h"

namespace rvcx {

// y[b][t][c] += nb[c] + sum_{q < taps*stride} wf[(q / stride) * C + c][q % stride] * har[b*har_bs + t*stride + q]
// (the NSF noise conv, hifigan_nsf.py:196-199, in its framed form); C % 4 == 0, taps*stride <= 16
// (store: y = the noise conv itself, not accumulated)
hipError_t noise_conv_add(const float* har, long long har_bs, int stride, int taps, const float* wf, const float* nb,
                          float* y, int B, int T, int C, hipStream_t s, bool store = false);
hipError_t sine_source(const float* f0, int B, int L, int upp, float sr, const float* eps, uint64_t seed,
                       float lin_w, float lin_b, double* cum_ws, float* har, long long har_ld, hipStream_t s);
// (y_bs: floats between the output rows of two batch entries, 0 = T)
hipError_t conv_post_tanh(const float* x, int B, int T, int C, const float* w, int K, float slope, float* y,
                          hipStream_t s, float bias = 0.f, long long y_bs = 0);
hipError_t zp_sample(const float* stats, int B, int T, int I, const float* eps, uint64_t seed, const float* mask,
                     float* zp, hipStream_t s);

// per-sample harmonic source of the MRF HiFi-GAN / RefineGAN decoders (source_harm.hip): f0 [B][L] -> har row b
// at har + b*har_ld, N = L*upp samples; eps [B][N][H] and ini [B][H] injected or drawn (Philox(seed))
size_t harm_source_ws_doubles(int B, int L, int upp, int H);
hipError_t harm_source(const float* f0, int B, int L, int upp, float sr, int H, int linear_up, const float* eps,
                       const float* ini, uint64_t seed, const float* lin_w, float lin_b, double* ws, float* har,
                       long long har_ld, hipStream_t st);

// RefineGAN (refinegan.hip): depthwise kaiser-sinc downsampling by `orig` (new_freq 1), linear x rate upsampling of
// lrelu(x) concatenated with a skip, AdaIN (mode 0 store, 1 add, 2 add then / div)
hipError_t resample_dw(const float* x, int B, int T_in, int C, const float* ker, int K, int orig, int width, float* y,
                       int T_out, hipStream_t s);
hipError_t lerp_up_cat(const float* x, int B, int T, int C, int ldx, int rate, float slope, const float* skip, int Cd,
                       float* y, int ldy, hipStream_t s);
hipError_t adain(const float* x, int B, int T, int C, const float* w, const float* eps, uint64_t seed, float slope,
                 float* y, int mode, float div, hipStream_t s);

}  // namespace rvcx
