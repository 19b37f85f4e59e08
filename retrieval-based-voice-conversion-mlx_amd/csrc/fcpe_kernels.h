// FCPE pitch network: the Performer attention (performer_attn.hip) and the non-GEMM kernels (fcpe.hip)
#pragma once
#include "kernel_base.h"

namespace rvcx {

// Performer (FAVOR+) linear attention (performer_attn.hip; FCPE.py:179-212, :354-363): element (h, t, d) of q / k / v
// at p + h hs + t ld + d (d < 64), P [M][64] the random-feature matrix, out element (h, t, d) at out + h out_hs +
// t out_ld + d; ws: performer_ws_floats(H, T, M, B) floats (ctx, ksum and, for T > PERFORMER_SLAB, one partial image
// of both per time slab, added in slab order). Every pointer 16-byte aligned, strides multiples of 4. B streams of
// T rows per launch: stream b's operands at p + b bs, its output at out + b out_bs; ctx, ksum, the row maximum and
// the denominator are per (stream, head). Tv (device, optional): stream b has Tv[b] <= T rows in its T-row slot; its
// keys end there, rows past it are neither read nor written, and its rows are the B = 1 call's bit for bit.
constexpr int PERFORMER_SLAB = 128, PERFORMER_MAX_FEATURES = 512;
int performer_slabs(int T);
long long performer_ws_floats(int H, int T, int M, int B = 1);
hipError_t performer_attention(const float* q, const float* k, const float* v, long long hs, int ld, int H, int T,
                               const float* P, int M, float* ws, float* out, long long out_hs, int out_ld,
                               hipStream_t s, int B = 1, long long bs = 0, long long out_bs = 0,
                               const int* Tv = nullptr);

// FCPE (fcpe.hip): GroupNorm(G, C) + LeakyReLU over x [B][T][C] in place, the statistics per (stream, group) (ws: B *
// G * FCPE_GN_CHUNKS * 2 doubles, the time chunks' sums). Tv (device, optional): stream b's statistics cover its own
// Tv[b] <= T rows, in the chunks a call on those rows alone forms, and its rows Tv[b] .. T - 1 are set to zero (the zero
// padding of the k = 3 conv that follows)
constexpr int FCPE_GN_CHUNKS = 64;
hipError_t groupnorm_lrelu(float* x, int T, int C, int G, const float* gamma, const float* beta, float eps, float slope,
                           double* ws, hipStream_t s, int B = 1, const int* Tv = nullptr);
// y [B][T][C2] = swish(b + depthwise_K(GLU(x [B][T][2 C2]))) with zero padding `pad` at each stream's own ends
// (w [K][C2], C2 % 64 == 0, K <= 64). Tv (device, optional): stream b ends at its own row Tv[b] <= T: taps from there
// on read zero and rows from there on are not written
hipError_t glu_dwconv_swish(const float* x, int T, int C2, const float* w, const float* b, int K, int pad, float* y,
                            hipStream_t s, int B = 1, const int* Tv = nullptr);
// fcpe_zero_pad: y [B][ldy] = pad_l zeros | x row b (n of ldx) | zeros
hipError_t fcpe_zero_pad(const float* x, int n, int pad_l, long long ldx, float* y, long long ldy, int B,
                         hipStream_t s);
// fcpe_dup_last_frame: row F - 1 of every stream of mel [B][F][C] = its row F - 2
hipError_t fcpe_dup_last_frame(float* mel, int B, int F, int C, hipStream_t s);
// the same per stream of Fv[b] <= F frames (device): row Fv[b] - 1 of stream b = its row Fv[b] - 2, and its rows
// Fv[b] .. F - 1 zero (what stack.0's tap past the stream's end reads); F_min = the shortest stream's frames (>= 2)
hipError_t fcpe_mel_tail_v(float* mel, int B, const int* Fv, int F, int F_min, int C, hipStream_t s);
// the cents decoders (mode 0 local_argmax, 1 argmax) on salience [F][nb] with the checkpoint's cent table -> f0 [F]
// (fp64 holding the fp32 value)
hipError_t fcpe_decode(const float* sal, int F, int nb, const float* cent, float thr, int mode, double* f0,
                       hipStream_t s);
// the same on B streams of Fv[b] <= F frames (device) in salience [B][F][nb]: stream b's f0 [Fv[b]] at f0 + b ldf,
// nothing written past it
hipError_t fcpe_decode_v(const float* sal, int B, const int* Fv, int F, int nb, const float* cent, float thr, int mode,
                         double* f0, long long ldf, hipStream_t s);
// FCPEF0Predictor.post_process: nearest expansion of f0 [F] to n frames and linear interpolation through the unvoiced
// ones (links: 2 n ints)
hipError_t fcpe_post_process(const double* f0, int F, int n, int hop, int sr, int* links, double* out, hipStream_t s);

}  // namespace rvcx
