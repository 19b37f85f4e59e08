// Elementwise maps, layout transforms and LayerNorm over [rows][C] matrices (rowops.hip)
#pragma once
#include "kernel_base.h"

namespace rvcx {

hipError_t fill(float* p, float v, long long n, hipStream_t s);
hipError_t randn(float* y, long long n, uint64_t seed, uint64_t offset, hipStream_t s);
hipError_t act_inplace(float* x, long long n, int act, float slope, hipStream_t s);
hipError_t affine_inplace(float* x, long long n, float a, float b, hipStream_t s);
hipError_t transpose_bct_btc(const float* x, float* y, int B, int C, int T, hipStream_t s); // [B][C][T] -> [B][T][C]
hipError_t channel_flip(const float* x, float* y, int rows, int C, hipStream_t s);
hipError_t gather_rows(const float* table, int ld_table, const int32_t* idx, float* y, int rows, int C,
                       hipStream_t s);
hipError_t seq_mask(const int32_t* lengths, float* mask, int B, int T, hipStream_t s);
hipError_t layernorm_rows(const float* x, const float* r, float* y, const float* gamma, const float* beta,
                          int rows, int D, float eps, const float* mask, hipStream_t s);
// x2 upsample + protect blend of B rows in one launch: feats / feats0 [B][L_max][D], L[b] valid -> out [B][T_max][D],
// T[b] valid, the rest zero; pitchf (optional) rows of stride ldp
hipError_t upsample2_protect(const float* feats, const float* feats0, Len L, int L_max, int D, float* out, Len T,
                             int T_max, const float* pitchf, long long ldp, float protect, hipStream_t s, int B = 1);
// pitch / pitchf rows of stride ldp -> pc / pf [B][T_max], zero from Tv[b] on
hipError_t pack_pitch(const int32_t* pitch, const float* pitchf, long long ldp, const int* Tv, int T_max, int32_t* pc,
                      float* pf, int B, hipStream_t s);

}  // namespace rvcx
