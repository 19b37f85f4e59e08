// The shared host side of the model runtime files: weight lookup and repacks, the mel front end's tables and runner,
// the sinc resampling table (declarations and the ConvArgs builders in model_build.h).
#include "model_build.h"

#include <algorithm>
#include <cmath>

namespace rvcx {

const HostTensor& host_weight(Ctx& c, int model, const std::string& n, const std::vector<int64_t>& shape) {
  auto it = c.host[model].find(n);
  if (it == c.host[model].end()) throw Error(RVCX_E_STATE, "missing weight: " + n);
  if (it->second.shape != shape) {
    std::string got, want;
    for (auto s : it->second.shape) got += std::to_string(s) + ",";
    for (auto s : shape) want += std::to_string(s) + ",";
    throw Error(RVCX_E_SHAPE, "weight " + n + " has shape (" + got + ") expected (" + want + ")");
  }
  return it->second;
}

std::vector<float> pack_conv1d(const HostTensor& t) {
  const int64_t O = t.shape[0], I = t.shape[1], K = t.shape[2];
  std::vector<float> out(t.v.size());
  for (int64_t o = 0; o < O; ++o)
    for (int64_t i = 0; i < I; ++i)
      for (int64_t k = 0; k < K; ++k) out[(k * O + o) * I + i] = t.v[(o * I + i) * K + k];
  return out;
}

std::vector<float> cat(std::initializer_list<const std::vector<float>*> parts) {
  std::vector<float> out;
  for (auto* p : parts) out.insert(out.end(), p->begin(), p->end());
  return out;
}

std::vector<float> mel_basis(const MelSpec& m) {
  // Slaney's scale: linear below 1 kHz, logarithmic above
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
  auto hz2mel = [&](double f) {
    if (m.htk) return 2595.0 * std::log10(1.0 + f / 700.0);
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
  };
  auto mel2hz = [&](double v) {
    if (m.htk) return 700.0 * (std::pow(10.0, v / 2595.0) - 1.0);
    return v >= min_log_mel ? min_log_hz * std::exp(logstep * (v - min_log_mel)) : f_sp * v;
  };
  const int n = m.n_mels + 2, nbin = m.nbin(), ld = m.ld();
  const double lo = hz2mel(m.fmin), hi = hz2mel(m.fmax), step = (hi - lo) / (n - 1);
  std::vector<double> mel_f(n);
  for (int i = 0; i < n; ++i) mel_f[i] = mel2hz(i == n - 1 ? hi : lo + i * step);
  std::vector<float> w((size_t)m.n_mels * ld, 0.f);
  for (int i = 0; i < m.n_mels; ++i) {
    const double fd0 = mel_f[i + 1] - mel_f[i], fd1 = mel_f[i + 2] - mel_f[i + 1];
    const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
    for (int k = 0; k < nbin; ++k) {
      const double f = k * ((double)m.sr / m.win);
      const float tri = (float)std::max(0.0, std::min(-(mel_f[i] - f) / fd0, (mel_f[i + 2] - f) / fd1));
      w[(size_t)i * ld + k] = (float)((double)tri * enorm);
    }
  }
  return w;
}

std::vector<float> stft_weights(int win) {
  const int nbin = win / 2 + 1, taps = win / 32;
  std::vector<float> w((size_t)taps * 2 * nbin * 32);
  const double pi = 3.14159265358979323846;
  for (int t = 0; t < taps; ++t)
    for (int nn = 0; nn < 2 * nbin; ++nn)
      for (int cc = 0; cc < 32; ++cc) {
        const int k = 32 * t + cc;
        const double wn = 0.5 - 0.5 * std::cos(2.0 * pi * k / win);
        const int f = nn < nbin ? nn : nn - nbin;
        const double ang = 2.0 * pi * (double)((long long)k * f % win) / win;
        w[((size_t)t * 2 * nbin + nn) * 32 + cc] = (float)(wn * (nn < nbin ? std::cos(ang) : -std::sin(ang)));
      }
  return w;
}

void mel_forward(Ctx& c, const MelSpec& m, const std::string& pfx, const float* audio, int64_t n, int64_t ld, int B,
                 const MelFrames& g, float* mel, hipStream_t s, const int* nv) {
  const int nbin = m.nbin(), ldm = m.ld();
  const int64_t rows = (n + g.pl + g.pr + 31) / 32;
  float* xp = c.buf<float>(pfx + "xp", (size_t)B * rows * 32, s);
  if (nv && g.zero_pad) throw Error(RVCX_E_INVALID, "mel: a length per stream takes the reflect pad");
  if (g.zero_pad) {
    check(fcpe_zero_pad(audio, (int)n, (int)g.pl, ld, xp, rows * 32, B, s), "mel_pad");
  } else {
    check(reflect_pad_1d(audio, (int)n, (int)g.pl, (int)g.pr, xp, s, B, ld, rows * 32, nv), "mel_pad");
  }
  float* spec = c.buf<float>(pfx + "spec", (size_t)B * g.Fm * 2 * nbin, s);
  {
    ConvArgs a = lin(xp, 32, (int)rows, 32, c.W(pfx + "stft"), 2 * nbin, nullptr, spec, 2 * nbin);
    a.taps = m.win / 32;
    a.stride = m.hop / 32;
    a.w_ts = (long long)2 * nbin * 32;
    a.T_out = g.Fm;
    a.batch = B;
    a.x_bs = rows * 32;
    a.y_bs = (long long)g.Fm * 2 * nbin;
    run1(c, a, s, 0.0);
  }
  float* mag = c.buf<float>(pfx + "mag", (size_t)B * g.Fm * ldm, s);
  check(stft_magnitude(spec, B * g.Fm, nbin, m.mag_eps, mag, ldm, s), "stft_magnitude");
  ConvArgs a = lin(mag, ldm, g.per_stream ? g.Fm : B * g.Fm, ldm, c.W(pfx + "mel"), m.n_mels, nullptr, mel, m.n_mels);
  a.act = ACT_LOGCLAMP;
  a.slope = 1e-5f;
  if (g.per_stream) {  // Fm rows of each stream into its F rows of mel
    a.batch = B;
    a.x_bs = (long long)g.Fm * ldm;
    a.y_bs = (long long)g.F * m.n_mels;
  }
  run1(c, a, s);
}

// modified Bessel function of the first kind, order 0 (series)
static double bessel_i0(double x) {
  double sum = 1.0, term = 1.0;
  const double q = 0.25 * x * x;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * k);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

SincKernel sinc_resample_kernel(int orig_freq, int new_freq, double lowpass_width, double rolloff, SincWindow window,
                                double beta) {
  int g = orig_freq;
  for (int b = new_freq; b;) {
    const int t = g % b;
    g = b;
    b = t;
  }
  SincKernel r;
  r.orig = orig_freq / g;
  r.nw = new_freq / g;
  const double base_d = (double)std::min(r.orig, r.nw) * rolloff;
  r.width = (int)std::ceil(lowpass_width * r.orig / base_d);
  r.K = 2 * r.width + r.orig;
  r.k.resize((size_t)r.nw * r.K);
  const float lpw = (float)lowpass_width, base = (float)base_d, pi = (float)M_PI, fbeta = (float)beta;
  const float i0b = (float)bessel_i0((double)fbeta), scale = (float)(base_d / r.orig);
  for (int p = 0; p < r.nw; ++p) {
    for (int i = 0; i < r.K; ++i) {
      const float idx = (float)(i - r.width) / (float)r.orig;
      float t = (-(float)p) / (float)r.nw + idx;
      t = t * base;
      t = std::min(std::max(t, -lpw), lpw);
      float win;
      if (window == SINC_KAISER) {
        const float q = t / lpw;
        win = (float)bessel_i0((double)(fbeta * std::sqrt(1.f - q * q))) / i0b;
      } else {
        const float cs = std::cos(t * pi / lpw / 2.0f);
        win = cs * cs;
      }
      t = t * pi;
      const float kv = t == 0.0f ? 1.0f : std::sin(t) / t;
      r.k[(size_t)p * r.K + i] = kv * (win * scale);
    }
  }
  return r;
}

}  // namespace rvcx
