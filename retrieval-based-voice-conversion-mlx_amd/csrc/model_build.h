// What every model's runtime file builds with (model_build.cpp): the checked weight lookup and repacks of finalize_*,
// the ConvArgs builders of the forward passes, the mel front end RMVPE and FCPE share, and torchaudio's sinc resampling
// table. Host code only.
#pragma once
#include <initializer_list>

#include "runtime.h"

namespace rvcx {

// the uploaded tensor `n` of model slot `model`; throws RVCX_E_STATE when missing, RVCX_E_SHAPE when not `shape`
const HostTensor& host_weight(Ctx& c, int model, const std::string& n, const std::vector<int64_t>& shape);
// torch Conv1d weight [O][I][K] -> [K][O][I]
std::vector<float> pack_conv1d(const HostTensor& t);
std::vector<float> cat(std::initializer_list<const std::vector<float>*> parts);

// y [rows][N] = x [rows][K] W^T + bias, W [N][K]
inline ConvArgs lin(const float* x, int ldx, int rows, int K, const float* w, int N, const float* bias, float* y,
                    int ldy) {
  ConvArgs a;
  a.x = x;
  a.ldx = ldx;
  a.T_in = rows;
  a.C_in = K;
  a.w = w;
  a.ldw = K;
  a.y = y;
  a.ldy = ldy;
  a.T_out = rows;
  a.N = N;
  a.bias = bias;
  return a;
}

// 1-D conv over B independent sequences of Tin rows ([B][Tin][ldx] -> [B][Tout][ldy]); weights packed [taps][N][Cin]
inline ConvArgs conv1d(const float* x, int ldx, int Tin, int Cin, const float* w, int N, int taps, int dil, int pad,
                       const float* bias, float* y, int ldy, int Tout, int B) {
  ConvArgs a = lin(x, ldx, Tin, Cin, w, N, bias, y, ldy);
  a.x_bs = (long long)Tin * ldx;
  a.w_ts = (long long)N * Cin;
  a.taps = taps;
  a.dil = dil;
  a.pad = pad;
  a.y_bs = (long long)Tout * ldy;
  a.T_out = Tout;
  a.batch = B;
  return a;
}

inline void run1(Ctx& c, const ConvArgs& a, hipStream_t s, double flops = -1.0) { launch_conv(c, a, false, s, flops); }
inline void run2(Ctx& c, const ConvArgs& a, hipStream_t s, double flops = -1.0) { launch_conv(c, a, true, s, flops); }

// ---- log-mel front end: reflect (or zero) pad -> STFT as a conv over 32-sample rows -> magnitude -> mel GEMM with
// log(clamp(1e-5)). win = n_fft, a multiple of 32 like hop.
struct MelSpec {
  int sr, win, hop, n_mels;
  double fmin, fmax;
  bool htk;       // librosa's htk=True mel scale (RMVPE), else Slaney's (FCPE)
  float mag_eps;  // sqrt(re^2 + im^2 + mag_eps)
  constexpr int nbin() const { return win / 2 + 1; }
  // magnitude / mel-basis row: the bins padded to whole 32-bin chunks
  constexpr int ld() const { return (nbin() + 31) / 32 * 32; }
};
// librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax, htk, norm='slaney'): [n_mels][ld()], bins past nbin() zero
std::vector<float> mel_basis(const MelSpec& m);
// the STFT (periodic Hann window of `win`) as conv weights W[tap][n][c], sample 32 tap + c; n < nbin real, else
// imaginary
std::vector<float> stft_weights(int win);
// how the caller frames a stream of n samples: pl / pr samples of padding (zeros instead of the reflection when
// zero_pad), Fm frames out of the STFT written to the first Fm of the stream's F rows of mel. per_stream: the mel GEMM
// takes the stream as its batch index; otherwise it runs once over the B Fm rows (Fm == F).
struct MelFrames {
  int64_t pl, pr;
  bool zero_pad;
  int Fm, F;
  bool per_stream;
};
// B streams of n samples (row b at audio + b ld) -> mel [B][F][n_mels]. Weights `pfx`stft / `pfx`mel, work buffers
// `pfx`xp / spec / mag. nv (device, optional; reflect pad only): stream b has nv[b] <= n samples and is padded at its
// own end; its frames past its own count are computed on the zeros after it (finite, for the caller to ignore).
void mel_forward(Ctx& c, const MelSpec& m, const std::string& pfx, const float* audio, int64_t n, int64_t ld, int B,
                 const MelFrames& g, float* mel, hipStream_t s, const int* nv = nullptr);

// ---- torchaudio.functional._get_sinc_resample_kernel, evaluated in float32 as a float32 waveform requests
struct SincKernel {
  int orig = 1, nw = 1, width = 0, K = 0;  // the rates over their gcd; K = 2 width + orig taps per phase
  std::vector<float> k;                    // [nw][K]
};
enum SincWindow { SINC_HANN, SINC_KAISER };  // "sinc_interp_hann" / "sinc_interp_kaiser" (beta)
SincKernel sinc_resample_kernel(int orig_freq, int new_freq, double lowpass_width, double rolloff, SincWindow window,
                                double beta);

}  // namespace rvcx
