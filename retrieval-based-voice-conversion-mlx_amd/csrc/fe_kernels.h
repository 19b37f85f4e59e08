// The feature extractors' non-GEMM kernels: HuBERT's fused conv0 (hubert_front.hip), RMVPE's pads, STFT magnitude,
// pooling and salience decode (rmvpe_aux.hip) and its bidirectional GRU (gru.hip)
#pragma once
#include "kernel_base.h"

namespace rvcx {

// ws: groupnorm_ws_doubles(C, B) doubles; x = B sequences of T rows back to back
constexpr int GN_CHUNKS = 256;
inline size_t groupnorm_ws_doubles(int C, int B = 1) { return (size_t)B * (GN_CHUNKS * C * 2 + C); }
// HuBERT conv_layers.0 fused: y[b][t][c] = GELU(GroupNorm_c(sum_k w10[c][k] x[b ldx + 5t + k])), C % 64 == 0,
// C <= 1024, y 16-byte aligned; ws as above (hubert_front.hip). Sequence b has T[b] rows (1 <= T[b] <= T_max) and its
// statistics are over those rows alone; y is [B][T_max][C], rows from T[b] on written as zero
hipError_t hubert_conv0_gn_gelu(const float* x, long long ldx, const float* w10, Len T, int T_max, int C,
                                const float* gamma, const float* beta, float eps, double* ws, float* y, hipStream_t s,
                                int B = 1);

// nv (device, optional): row b has nv[b] <= n samples (each longer than the pads: the caller's check) and is reflected
// about its own ends into its ldy >= n + pad_l + pad_r floats of y, zeros after
hipError_t reflect_pad_1d(const float* x, int n, int pad_l, int pad_r, float* y, hipStream_t s, int B = 1,
                          long long ldx = 0, long long ldy = 0, const int* nv = nullptr);
hipError_t reflect_pad_rows(const float* x, int rows, int C, int pad_r, float* y, hipStream_t s, int B = 1);
// images of different heights: x [B][ld_in][C] -> y [B][ld_out][C], image b's rows[b] rows reflected about its own last
// row up to out[b] rows (rows, out: device; out[b] - rows[b] < rows[b]), zeros from there to ld_out
hipError_t reflect_pad_rows_v(const float* x, const int* rows, const int* out, int ld_in, int ld_out, int C, float* y,
                              hipStream_t s, int B);
// sqrt(re^2 + im^2 + eps) of spec [F][2 nbins] into rows of ldm floats (zeros past nbins); eps 0 or 1e-9f
hipError_t stft_magnitude(const float* spec, int F, int nbins, float eps, float* mag, int ldm, hipStream_t s);
hipError_t avgpool2(const float* x, int H, int W, int C, int ldx, float* y, hipStream_t s);
hipError_t nhwc_to_hcw(const float* x, int H, int W, int C, float* y, hipStream_t s);
// ConvTranspose2d 3x3 / stride 2 / pad 1 / output pad 1 weights w [C][co][3][3] -> the 2x2-tap phase conv's
// [4][4 co][C] (virtual column (ph 2 + pw) co + o; ConvArgs::out_map OUT_UPSAMPLE2D scatters the phases)
hipError_t upconv_phase_pack(const float* w, int C, int co, float* out, hipStream_t s);
// B sequences: sal rows of sequence b start at b*Fs (Fs = F when 0), f0 [B][ldf] (ldf = F when 0); Fv (device,
// optional): sequence b has Fv[b] <= F frames, and f0 past them is not written
hipError_t rmvpe_decode(const float* sal, int F, int ncls, float thred, double* f0, hipStream_t s, int B = 1,
                        int Fs = 0, const int* Fv = nullptr, long long ldf = 0);

// B independent sequences (gi [B][T][1536], out [B][T][512], xchg gru_xchg_words(B) words); next_tag: the
// hand-off tag counter of this xchg buffer, owned by the caller (0 = buffer state unknown: zeroed first). Tv (device,
// optional): sequence b runs Tv[b] steps, 1 <= Tv[b] <= T, in rows of stride T; its rows from Tv[b] on are not written
hipError_t gru_bidir(const float* gi, const float* whh_f, const float* bhh_f, const float* whh_b,
                     const float* bhh_b, int T, float* out, unsigned long long* xchg, unsigned* status,
                     unsigned* next_tag, hipStream_t s, int B = 1, const int* Tv = nullptr);
inline size_t gru_xchg_words(int B) { return (size_t)B * 4 * 2 * 128; }

}  // namespace rvcx
