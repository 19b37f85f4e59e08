// The whole-utterance pipeline's DSP on device: the f0 post-processing (f0_post.hip), the (b, a) high-pass, peak
// normalisation, split points and the RMS envelope (pipeline_dsp.hip) and the second-order-section high-pass
// (iir_scan.hip)
#pragma once
#include "kernel_base.h"

namespace rvcx {

// Pipeline.get_f0 / Pipeline.pipeline host DSP moved on device (f0_post.hip)
hipError_t f0_post(const double* f0, int F, double shift, int32_t* coarse, float* pitchf, double* f0_out,
                   hipStream_t s);
hipError_t f0_autotune(double* f0, int F, double strength, int skip_unvoiced, hipStream_t s);
// every frame of the rows of f0 [B][F] with on[b] != 0, each at its own strength[b]; the other rows are not written
hipError_t f0_autotune_rows(double* f0, int F, const double* strength, const int* on, int B, hipStream_t s);

// pipeline DSP
constexpr int IIR_MAXO = 8;
hipError_t filtfilt_pad(const double* x, long long n, const double* b, const double* a, const double* zi, int order,
                        long long t_pad, double* ws, double* pad64, float* pad32, hipStream_t s);
size_t filtfilt_ws_doubles(long long n, int order);
// dst row b = src row b / (max|src row b| / 0.99) when that exceeds 1, else a copy (src == dst: in place), over the
// row's first n[b] samples (n_max >= every n[b]); ws peak_normalize_ws_floats(B)
hipError_t peak_normalize(const float* src, long long lds, float* dst, long long ldd, Len n, long long n_max, float* ws,
                          hipStream_t s, int B = 1);
size_t peak_normalize_ws_floats(int B);
hipError_t split_points(const double* x, long long n, int window, long long t_center, long long t_query,
                        double* sum_ws, long long* ts, int nts, hipStream_t s);
int rms_frame_count(long long n, int sr);
// fp64 frame RMS (librosa.feature.rms, center=True, constant pad): nframes = 1 + (n + 2*(frame/2) - frame)/hop
hipError_t rms_frames_f64(const double* x, long long n, int frame, int hop, double* rms, int nframes, hipStream_t s);
// AudioProcessor.change_rms of B rows in one launch set: source row b (fp64 or fp32, stride ld_src) of n_src[b]
// samples, target row b (stride ld_y) of n_y[b]; rate_v (optional, device) is a rate per row in place of rate, and a
// row whose entry is exactly 1 is left untouched. ws [B][rms_frame_count(n_src_max, sr_src) +
// rms_frame_count(n_y_max, sr_y)] floats: a row's source frames, then its target frames
template <class S>
hipError_t change_rms(const S* src, long long ld_src, Len n_src, long long n_src_max, int sr_src, float* y,
                      long long ld_y, Len n_y, long long n_y_max, int sr_y, float rate, const float* rate_v, float* ws,
                      hipStream_t s, int B = 1);

// second-order-section filtfilt (iir_scan.hip): the cascade's tables in one device buffer
struct SosPlan {
  int nsec = 0;
  const double* casc = nullptr;  // the cascade as one system (iir_scan.hip casc_filtfilt_pad), chunks of casc_L
  int casc_L = 128;
};
// filtfilt over the odd-extended input ext [ne] as two passes of the whole cascade (p.casc), trimmed and reflect-padded
hipError_t casc_filtfilt_pad(const SosPlan& p, const double* ext, long long ne, int padlen, long long n,
                             long long t_pad, double* ws, double* pad64, float* pad32, hipStream_t s);
size_t casc_ws_doubles(long long ne, int L);
// filtfilt (odd padding 3*(order+1)) through the SOS plan + reflect pad t_pad (pipeline.py:439, :459)
hipError_t filtfilt_sos_pad(const SosPlan& p, int order, const double* x, long long n, long long t_pad, double* ws,
                            double* pad64, float* pad32, hipStream_t s);
size_t filtfilt_sos_ws_doubles(long long n, int order);

}  // namespace rvcx
