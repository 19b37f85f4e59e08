// Realtime conversion: the per-hop stream kernels (stream.hip) and the noise gate (spectral_gate.hip)
#pragma once
#include "kernel_base.h"

namespace rvcx {

// streaming (stream.hip): B slots of one geometry per launch. slot2row [B] (-1 = idle this hop) / row2slot [B_act]
// map a group's slots to the compact rows the networks run on; null = identity (stream.hip's header)
hipError_t rt_resample(const float* x, long long ldx, int n_in, const float* ker, int K, int width, int orig, int nw,
                       float* y, long long ldy, int n_out, const float* pre, const int* slot2row, int B,
                       hipStream_t s);
hipError_t rt_ingest(const float* in16, int n16, const float* abuf_old, float* abuf_new, int na, const float* cbuf_old,
                     float* cbuf_new, int nc, double sensitivity, float* vol, float* volsq, int* gate,
                     const int* slot2row, float* cbuf_rows, int B, hipStream_t s);
hipError_t rt_pitch(const double* f0, int F, const double* factor, const int* pold, int* pnew, const float* fold,
                    float* fnew, int nbuf, const int* slot2row, int B, hipStream_t s);
hipError_t rt_up2(const float* feats, const float* feats0, int L, int D, float* phone, int T, const float* pitchf_buf,
                  int nbuf, float pscale, const float* protect, const int* use_protect, int* pitch_out,
                  const int* pitch_buf, float* pitchf_out, const int* row2slot, int B, hipStream_t s);
hipError_t rt_clip(float* x, long long ld, int n, int B, hipStream_t s);
hipError_t rt_sola(const float* audio, long long lda, const float* volsq, const int* gate, float* sola_buf, int cf,
                   int search, const float* fade_in, float* out, int block, int* offs, const int* slot2row, int B,
                   hipStream_t s);

// The realtime noise gate (spectral_gate.hip: TorchGate's stationary mode, core.py:86-94 / pipeline.py:326-327) over
// x [B][n] (rows ldx apart) -> y [B][n] (rows ldy apart): samples [0, sg_n_out(n)) gated, the rest zeros. strength
// [B] on the device: prop_decrease per row, negative = the row is copied through. nf / nt: the smoothing filter's half
// widths in bins / frames (1..SG_MAX_HALF). tab: sg_tables' floats on the device. Scratch per call: X [B][F][513][2],
// db [B][F][513] floats, mask [B][F][513] bytes, frames [B][F][1024] floats, F = sg_frames(n). mask_out (optional)
// [B][513][F]. Four launches whatever B is; needs n >= 2 * SG_NFFT.
constexpr int SG_NFFT = 1024, SG_HOP = 256, SG_BINS = SG_NFFT / 2 + 1, SG_MAX_HALF = 64;
constexpr int SG_TAB_FLOATS = 3 * SG_NFFT;
inline long long sg_frames(long long n) { return 1 + n / SG_HOP; }
inline long long sg_n_out(long long n) { return SG_HOP * (n / SG_HOP); }
// twiddles exp(-2 pi i m / 1024) as [1024][2], then the periodic Hann window [1024]; computed in double (host)
void sg_tables(float* tab);
hipError_t spectral_gate(const float* x, long long ldx, long long n, const float* strength, int nf, int nt,
                         const float* tab, float* X, float* db, unsigned char* mask, float* frames, float* y,
                         long long ldy, unsigned char* mask_out, int B, hipStream_t s);

}  // namespace rvcx
