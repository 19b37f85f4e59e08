// extern "C" boundary of the kernel-level test entries (include/rvcx_test.h): single kernels, the planner query and the
// comparison switches, for the numerics tests and A/B timing. The product ABI (include/rvcx.h) is capi.cpp.
#include <cstdint>
#include <string>

#include "../../include/rvcx_test.h"
#include "capi_common.h"

using namespace rvcx;

namespace {
// the dispatcher's record of a 1-D test descriptor (rvcx_conv1d_ex, rvcx_conv_plan)
ConvArgs conv_args_of(const rvcx_conv_test_desc* d) {
  ConvArgs a;
  a.x = d->x; a.x_bs = d->x_bs; a.x_bs2 = d->x_bs2; a.ldx = d->ldx; a.T_in = d->T_in; a.C_in = d->C_in;
  a.pre_act = d->pre_act; a.pre_slope = d->pre_slope; a.pre_mask = d->pre_mask; a.pre_mask_bs = d->pre_mask_bs;
  a.w = d->w; a.ldw = d->C_in; a.w_ts = (long long)d->N * d->C_in; a.w_bs2 = d->w_bs2;
  a.taps = d->taps; a.stride = d->stride; a.dil = d->dil; a.pad = d->pad;
  a.y = d->y; a.y_bs = d->y_bs; a.y_bs2 = d->y_bs2; a.ldy = d->ldy; a.T_out = d->T_out; a.N = d->N;
  a.bias = d->bias; a.bias_bs2 = d->bias_bs2; a.alpha = d->alpha; a.act = d->act; a.slope = d->slope;
  a.res = d->res; a.res_bs = d->res_bs; a.res_bs2 = d->res_bs2; a.ldr = d->ldr; a.res_mode = d->res_mode;
  a.mask = d->mask; a.mask_bs = d->mask_bs; a.acc_mode = d->acc_mode; a.acc_div = d->acc_div;
  a.gate_h = d->gate_h; a.gate_g = d->gate_g; a.gate_g_bs = d->gate_g_bs;
  a.ln_g = d->ln_g; a.ln_b = d->ln_b; a.ln_eps = d->ln_eps;
  a.batch = d->batch; a.batch_inner = d->batch_inner;
  a.nz_har = d->nz_har; a.nz_bs = d->nz_bs; a.nz_stride = d->nz_stride; a.nz_kk = d->nz_kk; a.nz_u = d->nz_u;
  a.nz_C = d->nz_C; a.nz_w = d->nz_w; a.nz_b = d->nz_b;
  a.no_splitk = d->no_splitk ? 1 : 0;
  return a;
}
}  // namespace

extern "C" {

int rvcx_set_conv_math(rvcx_ctx* ctx, int mode) {
  return guard(ctx, [&] {
    if (mode < 0 || mode > 3) throw Error(RVCX_E_INVALID, "conv math mode must be 0, 1, 2 or 3");
    ctx->conv_math = mode;
  });
}

int rvcx_set_dec_window(rvcx_ctx* ctx, int on) {
  return guard(ctx, [&] { ctx->dec_window = on != 0; });
}

int rvcx_dec_margin_frames(const rvcx_synth_desc* d, int* frames) {
  try {
    if (!frames) return RVCX_E_INVALID;
    *frames = dec_margin_frames(synth_cfg_of(d));
    return RVCX_OK;
  } catch (const Error& e) {
    return e.code;
  } catch (...) {
    return RVCX_E_INVALID;
  }
}

int rvcx_conv_plan(const rvcx_conv_test_desc* d, const rvcx_conv_plan_form* f, int two_d, int static_weight, int math,
                   int plan_T, int force_kind, int force_tile, int* kind, int* tile, int* ksplit, int* wsplit_fmt) {
  if (!d || !kind || !tile || !ksplit || !wsplit_fmt || math < 0 || math > 3 || (two_d && !f)) return RVCX_E_INVALID;
  ConvArgs a = conv_args_of(d);
  a.math = math;
  a.plan_T = plan_T;
  if (f) {
    a.W_in = f->W_in; a.W_out = f->W_out; a.KH = f->KH; a.KW = f->KW; a.padh = f->padh; a.padw = f->padw;
    a.out_map = f->out_map; a.out_cv = f->out_cv; a.lowp = f->lowp;
    if (f->ldw > 0) a.ldw = f->ldw;
    if (f->w_ts > 0) a.w_ts = f->w_ts;
    a.w_bs = f->w_bs; a.bias_bs = f->bias_bs;
  }
  const ConvPlan p = conv_plan(a, two_d != 0, static_weight != 0, ConvForce{force_kind, force_tile});
  *kind = p.kind, *tile = p.tile, *ksplit = p.ksplit, *wsplit_fmt = p.wsplit_fmt;
  return RVCX_OK;
}

int rvcx_conv1d(rvcx_ctx* ctx, const float* d_x, int64_t T, int C_in, const float* d_w, const float* d_bias, int N,
                int taps, int dilation, int pad, int stride, int math, float* d_y, int64_t T_out, void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    if (!d_x || !d_w || !d_y || T <= 0 || C_in <= 0 || N <= 0 || taps <= 0 || dilation <= 0 || stride <= 0 ||
        pad < 0 || T_out <= 0 || math < 0 || math > 7)
      throw Error(RVCX_E_INVALID, "rvcx_conv1d: bad argument");
    if ((T_out - 1) * stride + (int64_t)(taps - 1) * dilation + 1 > T + 2 * (int64_t)pad)
      throw Error(RVCX_E_SHAPE, "rvcx_conv1d: T_out exceeds the padded input");
    if (T > INT32_MAX || T_out > INT32_MAX || (int64_t)taps * N * C_in > INT32_MAX)
      throw Error(RVCX_E_SHAPE, "rvcx_conv1d: size out of range");
    ConvArgs a;
    a.x = d_x; a.ldx = C_in; a.T_in = (int)T; a.C_in = C_in;
    a.w = d_w; a.ldw = C_in; a.w_ts = (long long)N * C_in; a.taps = taps; a.dil = dilation; a.pad = pad;
    a.stride = stride;
    a.y = d_y; a.ldy = N; a.T_out = (int)T_out; a.N = N; a.bias = d_bias;
    // math -> the arithmetic, the forced family, the reduced-precision mode. 3 / 5 / 6: the weight-streamed kernel on
    // the tile the size policy picks, unsplit (5: the two-plane fp16 arithmetic, 6: its hi plane alone); 4 / 7: the
    // gather-streamed kernel, split-K by the size policy (7: fp16)
    static const struct { int math, kind, lowp; } route[8] = {{0, -1, 0}, {1, -1, 0}, {2, -1, 0}, {2, CK_WSB16, 0},
                                                              {2, CK_GS, 0}, {3, CK_WSB16, 0}, {3, CK_WSB16, 1}, {3, CK_GS, 0}};
    a.math = route[math].math;
    a.lowp = route[math].lowp;
    a.no_splitk = route[math].kind == CK_WSB16;
    const ConvForce force{route[math].kind};
    launch_conv_test(*ctx, a, false, force.kind >= 0, force, -1, "rvcx_conv1d", static_cast<hipStream_t>(stream));
  });
}

int rvcx_conv1d_gen(rvcx_ctx* ctx, const float* d_x, int64_t T, int C_in, const float* d_w, const float* d_bias,
                    int N, int taps, int dilation, int pad, int pre_act, float pre_slope, int act, float slope,
                    const float* d_res, int acc_mode, float acc_div, int kernel, float* d_y, void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    if (!d_x || !d_w || !d_y || T <= 0 || C_in <= 0 || N <= 0 || taps <= 0 || dilation <= 0 || pad < 0 || act < 0 ||
        act > 1 || pre_act < 0 || pre_act > 1 || acc_mode < 0 || acc_mode > 2 || kernel < 0 || kernel > 2 || (d_res && d_res == d_x))
      throw Error(RVCX_E_INVALID, "rvcx_conv1d_gen: bad argument");
    const int64_t T_out = T + 2 * (int64_t)pad - (int64_t)(taps - 1) * dilation;
    if (T_out <= 0 || T > INT32_MAX || (int64_t)taps * N * C_in > INT32_MAX)
      throw Error(RVCX_E_SHAPE, "rvcx_conv1d_gen: size out of range");
    ConvArgs a;
    a.x = d_x; a.ldx = C_in; a.T_in = (int)T; a.C_in = C_in;
    a.w = d_w; a.ldw = C_in; a.w_ts = (long long)N * C_in; a.taps = taps; a.dil = dilation; a.pad = pad;
    a.y = d_y; a.ldy = N; a.T_out = (int)T_out; a.N = N; a.bias = d_bias;
    a.pre_act = pre_act ? ACT_LRELU : ACT_NONE;
    a.pre_slope = pre_slope;
    a.act = act ? ACT_LRELU : ACT_NONE;
    a.slope = slope;
    if (d_res) {
      a.res = d_res;
      a.ldr = N;
      a.res_mode = RES_ADD_POST;
    }
    a.acc_mode = acc_mode == 0 ? ACC_STORE : (acc_mode == 1 ? ACC_ADD : ACC_ADD_DIV);
    a.acc_div = acc_div;
    a.math = 3;
    a.no_splitk = 1;
    if (!conv_wsb_eligible(a)) throw Error(RVCX_E_SHAPE, "rvcx_conv1d_gen: shape not eligible for the weight-streamed kernel");
    // 0: the size policy's route, 1: the weight-streamed tile the policy would pick, 2: the weight-stationary kernel
    const ConvForce force{kernel == 1 ? CK_WSB16 : (kernel == 2 ? CK_WST : -1)};
    launch_conv_test(*ctx, a, false, true, force, -1, "rvcx_conv1d_gen", static_cast<hipStream_t>(stream));
  });
}

int rvcx_conv1d_ex(rvcx_ctx* ctx, const rvcx_conv_test_desc* d, int* kind_out, int* ksplit_out, void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!d || !d->x || !d->w || !d->y || d->T_in <= 0 || d->C_in <= 0 || d->N <= 0 || d->taps <= 0 || d->dil <= 0 ||
        d->stride <= 0 || d->pad < 0 || d->T_out <= 0 || d->batch <= 0 || d->batch_inner <= 0 || d->ldx < d->C_in ||
        d->ldy < (d->gate_h > 0 ? d->gate_h : d->N) || d->pre_act < 0 || d->pre_act > ACT_LOGCLAMP || d->act < 0 ||
        d->act > ACT_LOGCLAMP || d->res_mode < RES_NONE || d->res_mode > RES_RSUB_POST || d->acc_mode < ACC_STORE ||
        d->acc_mode > ACC_ADD_DIV || (d->res_mode != RES_NONE && !d->res) || (d->res && d->ldr != 0 && d->ldr < d->N) ||
        d->route < 0 || d->route > 5 || d->gate_h < 0 || (d->gate_h > 0 && !d->gate_g) ||
        (d->ln_g && (!d->ln_b || !d->res)) ||
        (d->nz_har && (!d->nz_w || !d->nz_b || d->nz_C <= 0 || d->nz_u <= 0 || d->nz_stride <= 0)) ||
        ctx->is_weight(d->w))
      throw Error(RVCX_E_INVALID, "rvcx_conv1d_ex: bad argument");
    if ((int64_t)(d->T_out - 1) * d->stride + (int64_t)(d->taps - 1) * d->dil + 1 > d->T_in + 2 * (int64_t)d->pad)
      throw Error(RVCX_E_SHAPE, "rvcx_conv1d_ex: T_out exceeds the padded input");
    if ((int64_t)d->taps * d->N * d->C_in > INT32_MAX) throw Error(RVCX_E_SHAPE, "rvcx_conv1d_ex: size out of range");
    ConvArgs a = conv_args_of(d);
    // the combine-time epilogues as their kernels take them (launch_splitk_reduce's conditions)
    if (a.ln_g && (a.N > 1024 || a.batch_inner != 1 || a.res_mode != RES_NONE || a.acc_mode != ACC_STORE || a.gate_h > 0))
      throw Error(RVCX_E_SHAPE, "rvcx_conv1d_ex: the combine's LayerNorm takes N <= 1024, one group, no other residual");
    if (a.gate_h > 0 && (a.N != 2 * a.gate_h || a.batch_inner != 1 || a.act != ACT_NONE || a.alpha != 1.f || a.res ||
                         a.mask || a.acc_mode != ACC_STORE))
      throw Error(RVCX_E_SHAPE, "rvcx_conv1d_ex: the combine's gate takes N = 2 gate_h and no other epilogue field");
    if (a.nz_har && (a.nz_kk != 1 || a.N != a.nz_u * a.nz_C || a.gate_h > 0 || a.ln_g))
      throw Error(RVCX_E_SHAPE, "rvcx_conv1d_ex: the fused noise conv takes one tap and N = nz_u nz_C");
    // route -> the arithmetic, a static weight, the forced family and the family the launch has to get
    static const struct { int math, stat, force, expect; } route[6] = {{0, 1, -1, -1},       {1, 0, -1, CK_GEMM},
                                                                       {2, 0, -1, CK_EMU},   {3, 1, CK_WSB16, -1},
                                                                       {3, 1, CK_GS, -1},    {3, 1, CK_WST, -1}};
    const auto& r = route[d->route];
    a.math = r.math;
    const ConvPlan p = launch_conv_test(*ctx, a, false, r.stat != 0, ConvForce{r.force}, r.expect, "rvcx_conv1d_ex", s);
    if (ksplit_out) *ksplit_out = p.ksplit;
    if (kind_out) *kind_out = p.kind;
  });
}

namespace {
// the per-image heights of a *_v entry on device (host array H[B], each in [1, H_max]); nullptr without one
const int* test_heights(Ctx& c, const int* H, int B, int H_max, const char* who, hipStream_t s) {
  if (!H) return nullptr;
  for (int b = 0; b < B; ++b)
    if (H[b] < 1 || H[b] > H_max) throw Error(RVCX_E_INVALID, std::string(who) + ": a height outside [1, H_max]");
  int* d = c.buf<int>("conv.test.h", (size_t)B, s);
  RVCX_HIP(hipMemcpyAsync(d, H, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, s));
  return d;
}

// rvcx_conv2d3x3 on B images of H rows back to back, image b's own height Hv[b] (host, optional)
void conv2d3x3_run(rvcx_ctx* ctx, const float* d_x, int B, const int* Hv, int H, int W, int C_in, const float* d_w,
                   const float* d_bias, int N, int act, int math, float* d_y, void* stream, const char* who) {
  set_device(ctx);
  if (!d_x || !d_w || !d_y || B <= 0 || H <= 0 || W <= 0 || C_in <= 0 || N <= 0 || act < 0 || act > 1 || math < 0 ||
      math > 2)
    throw Error(RVCX_E_INVALID, std::string(who) + ": bad argument");
  if ((int64_t)B * H * W * (C_in > N ? C_in : N) > INT32_MAX) throw Error(RVCX_E_SHAPE, std::string(who) + ": size out of range");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ConvArgs a;
  a.x = d_x; a.ldx = C_in; a.T_in = H; a.W_in = W; a.C_in = C_in;
  a.w = d_w; a.ldw = C_in; a.w_ts = (long long)N * C_in; a.taps = 9; a.KH = 3; a.KW = 3; a.padh = 1; a.padw = 1;
  a.y = d_y; a.ldy = N; a.T_out = H; a.W_out = W; a.N = N; a.bias = d_bias;
  a.act = act ? ACT_RELU : ACT_NONE;
  if (B > 1) {
    a.batch = B;
    a.x_bs = (long long)H * W * C_in;
    a.y_bs = (long long)H * W * N;
  }
  a.h_in = test_heights(*ctx, Hv, B, H, who, s);
  // math 2: the windowed gather-streamed kernel of the U-Net's deep levels in the two-plane fp16 split (64 x 64 tiles,
  // K split over workgroups by the size policy); else the policy for a weight that is not static (the 3x3
  // small-channel form reads a fresh fp16 image under the fp16-split arithmetic)
  static const struct { int math, kind; } route[3] = {{0, -1}, {1, -1}, {3, CK_GSW}};
  a.math = route[math].math;
  const ConvForce force{route[math].kind};
  if (math == 2 && !conv_gsw_eligible(a)) throw Error(RVCX_E_SHAPE, std::string(who) + ": shape not eligible for the windowed kernel");
  launch_conv_test(*ctx, a, true, math == 2, force, -1, who, s);
}

// rvcx_convtranspose2d_s2 likewise
void convtranspose2d_s2_run(rvcx_ctx* ctx, const float* d_x, int B, const int* Hv, int H, int W, int C_in,
                            const float* d_w, const float* d_bias, int N, int act, int math, float* d_y, void* stream,
                            const char* who) {
  set_device(ctx);
  if (!d_x || !d_w || !d_y || B <= 0 || H <= 0 || W <= 0 || C_in <= 0 || N <= 0 || act < 0 || act > 1 || math < 0 ||
      math > 1)
    throw Error(RVCX_E_INVALID, std::string(who) + ": bad argument");
  if ((int64_t)4 * B * H * W * (C_in > 4 * N ? C_in : 4 * N) > INT32_MAX)
    throw Error(RVCX_E_SHAPE, std::string(who) + ": size out of range");
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the phase-conv weights (and its bias per virtual column) in test buffers, rebuilt every call
  float* wp = ctx->buf<float>("conv.test.upw", (size_t)16 * N * C_in, s);
  check(upconv_phase_pack(d_w, C_in, N, wp, s), "upconv_phase_pack");
  float* bp = nullptr;
  if (d_bias) {
    bp = ctx->buf<float>("conv.test.upb", (size_t)4 * N, s);
    for (int p = 0; p < 4; ++p)
      RVCX_HIP(hipMemcpyAsync(bp + (size_t)p * N, d_bias, sizeof(float) * N, hipMemcpyDeviceToDevice, s));
  }
  ConvArgs a;  // runtime_fe.cpp's decoder up-conv
  a.x = d_x; a.ldx = C_in; a.T_in = H; a.W_in = W; a.C_in = C_in;
  a.w = wp; a.ldw = C_in; a.w_ts = (long long)4 * N * C_in; a.taps = 4; a.KH = 2; a.KW = 2;
  a.y = d_y; a.ldy = N; a.T_out = H; a.W_out = W; a.N = 4 * N;
  a.out_map = OUT_UPSAMPLE2D;
  a.out_cv = N;
  a.bias = bp;
  a.act = act ? ACT_RELU : ACT_NONE;
  if (B > 1) {
    a.batch = B;
    a.x_bs = (long long)H * W * C_in;
    a.y_bs = (long long)4 * H * W * N;
  }
  a.h_in = test_heights(*ctx, Hv, B, H, who, s);
  // math 0: the gather-streamed kernel the pipeline's policy routes the up-convs to (under a split arithmetic); 1: the
  // native fp32 kernel
  a.math = math == 1 ? 1 : 0;
  const ConvForce force{math == 0 && conv_math(ctx->conv_math) >= 2 ? CK_GS : -1};
  launch_conv_test(*ctx, a, true, force.kind >= 0, force, -1, who, s);
}
}  // namespace

int rvcx_conv2d3x3(rvcx_ctx* ctx, const float* d_x, int H, int W, int C_in, const float* d_w, const float* d_bias,
                   int N, int act, int math, float* d_y, void* stream) {
  return guard(ctx, [&] {
    conv2d3x3_run(ctx, d_x, 1, nullptr, H, W, C_in, d_w, d_bias, N, act, math, d_y, stream, "rvcx_conv2d3x3");
  });
}

int rvcx_conv2d3x3_v(rvcx_ctx* ctx, const float* d_x, int B, const int* H, int H_max, int W, int C_in,
                     const float* d_w, const float* d_bias, int N, int act, int math, float* d_y, void* stream) {
  return guard(ctx, [&] {
    if (!H) throw Error(RVCX_E_INVALID, "rvcx_conv2d3x3_v: bad argument");
    conv2d3x3_run(ctx, d_x, B, H, H_max, W, C_in, d_w, d_bias, N, act, math, d_y, stream, "rvcx_conv2d3x3_v");
  });
}

int rvcx_convtranspose2d_s2(rvcx_ctx* ctx, const float* d_x, int H, int W, int C_in, const float* d_w,
                            const float* d_bias, int N, int act, int math, float* d_y, void* stream) {
  return guard(ctx, [&] {
    convtranspose2d_s2_run(ctx, d_x, 1, nullptr, H, W, C_in, d_w, d_bias, N, act, math, d_y, stream,
                           "rvcx_convtranspose2d_s2");
  });
}

int rvcx_convtranspose2d_s2_v(rvcx_ctx* ctx, const float* d_x, int B, const int* H, int H_max, int W, int C_in,
                              const float* d_w, const float* d_bias, int N, int act, int math, float* d_y,
                              void* stream) {
  return guard(ctx, [&] {
    if (!H) throw Error(RVCX_E_INVALID, "rvcx_convtranspose2d_s2_v: bad argument");
    convtranspose2d_s2_run(ctx, d_x, B, H, H_max, W, C_in, d_w, d_bias, N, act, math, d_y, stream,
                           "rvcx_convtranspose2d_s2_v");
  });
}

int rvcx_flash_attention(rvcx_ctx* ctx, const float* d_qkv, int B, int T, int n_heads, int dk, float qscale,
                         const float* d_rel_k, const float* d_rel_v, int window, const float* d_mask, float* d_out,
                         void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    if (!d_qkv || !d_out || B <= 0 || T <= 0 || n_heads <= 0 || (dk != 64 && dk != 96) || window < 0 ||
        (d_rel_k != nullptr) != (d_rel_v != nullptr))
      throw Error(RVCX_E_INVALID, "rvcx_flash_attention: bad argument");
    if ((long long)B * T * 3 * n_heads * dk > INT32_MAX) throw Error(RVCX_E_SHAPE, "rvcx_flash_attention: too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nsplit = flash_attn_splits(B, n_heads, T);
    float* po = ctx->buf<float>("att.test.o", (size_t)flash_attn_ws_floats(B, n_heads, T, dk, nsplit), s);
    float* pml = ctx->buf<float>("att.test.ml", (size_t)nsplit * B * n_heads * T * 2, s);
    check(flash_attn(d_qkv, 3 * n_heads * dk, B, T, n_heads, dk, qscale, d_rel_k, d_rel_v, window, d_mask, po, pml,
                     nsplit, d_out, n_heads * dk, s),
          "flash_attn");
  });
}

int rvcx_resblock_pair(rvcx_ctx* ctx, const float* d_x, int B, int64_t T, int C, const float* d_w1, const float* d_b1,
                       const float* d_w2, const float* d_b2, int k, int dilation, int acc_mode, float acc_div, int cfg,
                       float* d_y, void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    if (!d_x || !d_y || !d_w1 || !d_w2 || !d_b1 || !d_b2 || B <= 0 || T <= 0 || acc_mode < 0 || acc_mode > 2 ||
        d_x == d_y || cfg < 0)
      throw Error(RVCX_E_INVALID, "rvcx_resblock_pair: bad argument");
    if (!rb_pair_fits(C, k, dilation) || T > INT32_MAX / C)
      throw Error(RVCX_E_SHAPE, "rvcx_resblock_pair: shape not supported by the fused kernel");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int fmt = (cfg >> 4) & 3;
    if (fmt > 2) throw Error(RVCX_E_INVALID, "rvcx_resblock_pair: arithmetic (cfg bits 4-5) must be 0, 1 or 2");
    cfg &= 15;
    const int wfmt = fmt ? RB_WF16 : RB_WBF16;
    // fresh split images every call (test entry: the weight pointers may be reused by the caller)
    void* w1s = ctx->buf<char>("rb.test.w1s", (size_t)rb_wsplit_bytes(C, k, wfmt), s);
    void* w2s = ctx->buf<char>("rb.test.w2s", (size_t)rb_wsplit_bytes(C, k, wfmt), s);
    check(rb_wsplit_build(d_w1, C, k, w1s, s, wfmt), "rb_wsplit_build");
    check(rb_wsplit_build(d_w2, C, k, w2s, s, wfmt), "rb_wsplit_build");
    RbPairArgs a;
    a.wfmt = wfmt;
    a.lowp = fmt == 2;
    a.x = d_x;
    a.x_bs = T * C;
    a.w1s = w1s;
    a.b1 = d_b1;
    a.w2s = w2s;
    a.b2 = d_b2;
    a.C = C;
    a.k = k;
    a.d = dilation;
    a.T = (int)T;
    a.B = B;
    a.y = d_y;
    a.y_bs = T * C;
    a.acc_mode = acc_mode;
    a.acc_div = acc_div;
    check(rb_pair(a, cfg, s), "rb_pair");
  });
}

int rvcx_fcpe_mel(rvcx_ctx* ctx, const float* d_audio, int64_t n, float* d_mel, int64_t cap_frames, int64_t* frames_out,
                  void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_FCPE]) throw Error(RVCX_E_STATE, "fcpe weights not finalized");
    if (!d_audio || !d_mel || n <= 0) throw Error(RVCX_E_INVALID, "rvcx_fcpe_mel: bad arguments");
    if (cap_frames < fcpe_frames(*ctx, n)) throw Error(RVCX_E_CAPACITY, "rvcx_fcpe_mel: output capacity too small");
    set_device(ctx);
    const int F = fcpe_mel(*ctx, d_audio, n, n, 1, d_mel, static_cast<hipStream_t>(stream));
    if (frames_out) *frames_out = F;
  });
}

int rvcx_performer_attention(rvcx_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, int H, int T,
                             const float* d_P, int M, float* d_out, void* stream) {
  return guard(ctx, [&] {
    if (!d_q || !d_k || !d_v || !d_P || !d_out || H <= 0 || T <= 0 || M <= 0)
      throw Error(RVCX_E_INVALID, "rvcx_performer_attention: bad argument");
    if (M > PERFORMER_MAX_FEATURES || (long long)H * T * 64 > INT32_MAX)
      throw Error(RVCX_E_SHAPE, "rvcx_performer_attention: at most 512 features and 2^31 elements per operand");
    set_device(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ws = ctx->buf<float>("perf.test.ws", (size_t)performer_ws_floats(H, T, M), s);
    check(performer_attention(d_q, d_k, d_v, (long long)T * 64, 64, H, T, d_P, M, ws, d_out, (long long)T * 64, 64, s),
          "performer_attention");
  });
}

int rvcx_performer_attention_b(rvcx_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, int B, int H, int T,
                               const float* d_P, int M, float* d_out, void* stream) {
  return guard(ctx, [&] {
    if (!d_q || !d_k || !d_v || !d_P || !d_out || B <= 0 || H <= 0 || T <= 0 || M <= 0)
      throw Error(RVCX_E_INVALID, "rvcx_performer_attention_b: bad argument");
    if (M > PERFORMER_MAX_FEATURES || B > 4096 || (long long)B * H * T * 64 > INT32_MAX)
      throw Error(RVCX_E_SHAPE, "rvcx_performer_attention_b: at most 512 features and 2^31 elements per operand");
    set_device(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ws = ctx->buf<float>("perf.test.ws", (size_t)performer_ws_floats(H, T, M, B), s);
    const long long bs = (long long)H * T * 64;
    check(performer_attention(d_q, d_k, d_v, (long long)T * 64, 64, H, T, d_P, M, ws, d_out, (long long)T * 64, 64, s, B,
                              bs, bs),
          "performer_attention");
  });
}

int rvcx_performer_attention_v(rvcx_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, int B, int H,
                               const int32_t* T, int T_max, const float* d_P, int M, float* d_out, void* stream) {
  return guard(ctx, [&] {
    if (!d_q || !d_k || !d_v || !d_P || !d_out || !T || B <= 0 || H <= 0 || T_max <= 0 || M <= 0)
      throw Error(RVCX_E_INVALID, "rvcx_performer_attention_v: bad argument");
    for (int b = 0; b < B; ++b)
      if (T[b] < 1 || T[b] > T_max) throw Error(RVCX_E_INVALID, "rvcx_performer_attention_v: bad row count");
    if (M > PERFORMER_MAX_FEATURES || B > 4096 || (long long)B * H * T_max * 64 > INT32_MAX)
      throw Error(RVCX_E_SHAPE, "rvcx_performer_attention_v: at most 512 features and 2^31 elements per operand");
    set_device(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t* dT = ctx->buf<int32_t>("perf.test.T", (size_t)B, s);
    RVCX_HIP(hipMemcpyAsync(dT, T, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, s));
    float* ws = ctx->buf<float>("perf.test.ws", (size_t)performer_ws_floats(H, T_max, M, B), s);
    const long long bs = (long long)H * T_max * 64;
    check(performer_attention(d_q, d_k, d_v, (long long)T_max * 64, 64, H, T_max, d_P, M, ws, d_out,
                              (long long)T_max * 64, 64, s, B, bs, bs, dT),
          "performer_attention");
    RVCX_HIP(hipStreamSynchronize(s));  // T is the caller's
  });
}

int rvcx_kmeans_assign(rvcx_ctx* ctx, const float* d_x, int64_t n, int d, const float* d_cent, int64_t nlist,
                       int32_t* d_assign, float* d_dist, void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    kmeans_assign_run(*ctx, d_x, n, d, d_cent, nlist, d_assign, d_dist, static_cast<hipStream_t>(stream));
  });
}

int rvcx_kmeans_update(rvcx_ctx* ctx, const float* d_x, int64_t n, int d, const int32_t* d_assign, int64_t nlist,
                       float* d_cent, int64_t* d_sizes, void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    kmeans_update_run(*ctx, d_x, n, d, d_assign, nlist, d_cent, d_sizes, static_cast<hipStream_t>(stream));
  });
}

namespace {
// rvcx_gru_bidir with each sequence's own step count Tv[b] <= T (host, optional)
void gru_bidir_test(rvcx_ctx* ctx, const float* d_gi, int B, int T, const int* Tv, const float* d_whh_f,
                    const float* d_bhh_f, const float* d_whh_b, const float* d_bhh_b, float* d_out, int64_t tag_start,
                    void* stream, const char* who) {
  // T: the kernel's 32-bit row offsets (t * 1536); the weights are read as float4
  if (!d_gi || !d_whh_f || !d_bhh_f || !d_whh_b || !d_bhh_b || !d_out || B < 1 || B > 65535 || T < 1 ||
      T > (1 << 20) || tag_start > (int64_t)UINT32_MAX || (reinterpret_cast<uintptr_t>(d_whh_f) & 15) ||
      (reinterpret_cast<uintptr_t>(d_whh_b) & 15))
    throw Error(RVCX_E_INVALID, std::string(who) + ": bad arguments");
  set_device(ctx);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int* d_T = nullptr;
  if (Tv) {
    int* d = ctx->buf<int>("gru.test.T", (size_t)B, s);
    RVCX_HIP(hipMemcpyAsync(d, Tv, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, s));
    d_T = d;
  }
  gru_bidir_run(*ctx, d_gi, B, T, d_whh_f, d_bhh_f, d_whh_b, d_bhh_b, d_out, tag_start < 0 ? -1 : (long long)tag_start,
                s, d_T);
}
}  // namespace

int rvcx_gru_bidir(rvcx_ctx* ctx, const float* d_gi, int B, int T, const float* d_whh_f, const float* d_bhh_f,
                   const float* d_whh_b, const float* d_bhh_b, float* d_out, int64_t tag_start, void* stream) {
  return guard(ctx, [&] {
    gru_bidir_test(ctx, d_gi, B, T, nullptr, d_whh_f, d_bhh_f, d_whh_b, d_bhh_b, d_out, tag_start, stream,
                   "rvcx_gru_bidir");
  });
}

int rvcx_gru_bidir_v(rvcx_ctx* ctx, const float* d_gi, int B, const int* T, const float* d_whh_f, const float* d_bhh_f,
                     const float* d_whh_b, const float* d_bhh_b, float* d_out, int64_t tag_start, void* stream) {
  return guard(ctx, [&] {
    if (!T || B < 1) throw Error(RVCX_E_INVALID, "rvcx_gru_bidir_v: bad arguments");
    int T_max = 0;
    for (int b = 0; b < B; ++b) {
      if (T[b] < 1) throw Error(RVCX_E_INVALID, "rvcx_gru_bidir_v: a sequence of no steps");
      T_max = T[b] > T_max ? T[b] : T_max;
    }
    gru_bidir_test(ctx, d_gi, B, T_max, T, d_whh_f, d_bhh_f, d_whh_b, d_bhh_b, d_out, tag_start, stream,
                   "rvcx_gru_bidir_v");
  });
}

int rvcx_dec_source(rvcx_ctx* ctx, int B, int T, const float* d_f0, const float* d_eps_src, uint64_t seed, float* d_har,
                    void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_SYNTH] || !ctx->scfg.f0 || ctx->scfg.vocoder == 2)
      throw Error(RVCX_E_STATE, "rvcx_dec_source: needs a finalized pitch-guided HiFi-GAN (NSF) or MRF synthesizer");
    if (B < 1 || T < 1 || !d_f0 || !d_har) throw Error(RVCX_E_INVALID, "rvcx_dec_source: bad arguments");
    set_device(ctx);
    dec_source_rows(*ctx, B, T, d_f0, d_eps_src, seed, d_har, static_cast<hipStream_t>(stream));
  });
}

int rvcx_rg_resample_dw(rvcx_ctx* ctx, const float* d_x, int B, int T_in, int C, const float* d_ker, int orig, int width,
                        float* d_y, int T_out, void* stream) {
  return guard(ctx, [&] {
    if (!d_x || !d_ker || !d_y || B < 1 || T_in < 1 || C < 1 || orig < 1 || width < 0 || T_out < 1)
      throw Error(RVCX_E_INVALID, "rvcx_rg_resample_dw: bad argument");
    const int64_t K = 2 * (int64_t)width + orig;
    if (K > 8192 || T_out > ((int64_t)T_in + orig - 1) / orig || (int64_t)B * T_in * C > INT32_MAX)
      throw Error(RVCX_E_SHAPE, "rvcx_rg_resample_dw: at most 8192 taps, T_out <= ceil(T_in / orig), 2^31 elements");
    set_device(ctx);
    check(resample_dw(d_x, B, T_in, C, d_ker, (int)K, orig, width, d_y, T_out, static_cast<hipStream_t>(stream)),
          "resample_dw");
  });
}

int rvcx_rg_lerp_up_cat(rvcx_ctx* ctx, const float* d_x, int B, int T, int C, int ldx, int rate, float slope,
                        const float* d_skip, int Cd, float* d_y, int ldy, void* stream) {
  return guard(ctx, [&] {
    if (!d_x || !d_skip || !d_y || B < 1 || T < 1 || C < 1 || Cd < 1 || rate < 1)
      throw Error(RVCX_E_INVALID, "rvcx_rg_lerp_up_cat: bad argument");
    if (ldx < C || ldy < (int64_t)C + Cd || (int64_t)B * T * rate * ldy > INT32_MAX || (int64_t)B * T * ldx > INT32_MAX)
      throw Error(RVCX_E_SHAPE, "rvcx_rg_lerp_up_cat: ldx >= C, ldy >= C + Cd, 2^31 elements");
    set_device(ctx);
    check(lerp_up_cat(d_x, B, T, C, ldx, rate, slope, d_skip, Cd, d_y, ldy, static_cast<hipStream_t>(stream)),
          "lerp_up_cat");
  });
}

int rvcx_rg_adain(rvcx_ctx* ctx, const float* d_x, int B, int T, int C, const float* d_w, const float* d_eps,
                  uint64_t seed, float slope, float* d_y, int mode, float div, void* stream) {
  return guard(ctx, [&] {
    if (!d_x || !d_w || !d_y || B < 1 || T < 1 || C < 1 || mode < 0 || mode > 2 || (mode == 2 && div == 0.f))
      throw Error(RVCX_E_INVALID, "rvcx_rg_adain: bad argument");
    if ((int64_t)B * T * C > INT32_MAX) throw Error(RVCX_E_SHAPE, "rvcx_rg_adain: at most 2^31 elements");
    set_device(ctx);
    check(adain(d_x, B, T, C, d_w, d_eps, seed, slope, d_y, mode, div, static_cast<hipStream_t>(stream)), "adain");
  });
}

int rvcx_rt_model_rows(rvcx_ctx* ctx, rvcx_rt* rt, int gated, float* d_dst, int64_t ld, void* stream) {
  return guard(ctx, [&] {
    if (!rt || !rt->s) throw Error(RVCX_E_INVALID, "rt_model_rows: null stream group");
    RVCX_HIP(hipSetDevice(ctx->device));  // not a compute call: the pool the rows lie in is left as the hop left it
    rt_model_rows(*rt->s, gated, d_dst, ld, static_cast<hipStream_t>(stream));
  });
}

}  // extern "C"
