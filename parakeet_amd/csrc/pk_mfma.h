// pk_mfma.h -- the vector types and the few device helpers every MFMA kernel of the library is written with: the
// accumulator layout of a 32x32 tile, the in-register (hi, lo) split of the split-fp16 scheme (pk_split.h: its block
// scaling) and the small pieces around it.  Each exists once, here.
// (pwg.hip keeps private copies of mfma_row, dpp_max_step and wave_max64: its text is what profiles/pwg_layer_traffic.json is keyed to.)
#pragma once
#include "pk_split.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __fp16 pkh2 __attribute__((ext_vector_type(2)));

// row of a 32x32 accumulator tile that register r of a lane in half wave hi holds (the column is lane & 31); also the
// order host code packs MFMA fragments in
__host__ __device__ __forceinline__ int mfma_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

__device__ __forceinline__ f32x16 mfma16(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// In-register split of 8 values, x = hi + lo: hi = v_cvt_pkrtz (round toward zero, saturating at +-65504); x - hi exactly
// by v_fma_mix_f32 on the packed high part; lo = fp16_rne(x - hi): |x - hi - lo| <= 2^-21 |x|
__device__ __forceinline__ void split8(const float (&v)[8], f16x8& hi, f16x8& lo) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const pkh2 h = __builtin_amdgcn_cvt_pkrtz(v[2 * p], v[2 * p + 1]);
        const unsigned hu = __builtin_bit_cast(unsigned, h);
        float l0, l1;
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(hu), "v"(v[2 * p]));
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(hu), "v"(v[2 * p + 1]));
        hi[2 * p] = (_Float16)h[0];
        hi[2 * p + 1] = (_Float16)h[1];
        lo[2 * p] = (_Float16)l0;
        lo[2 * p + 1] = (_Float16)l1;
    }
}
// split of 2^k * x (block scaling, pk_split.h: x scaled exactly, then as split8)
__device__ __forceinline__ void split8s(const float (&v)[8], float s, f16x8& hi, f16x8& lo) {
    float t[8];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        f32x2 u = {v[2 * p], v[2 * p + 1]};
        u *= s;
        t[2 * p] = u[0];
        t[2 * p + 1] = u[1];
    }
    split8(t, hi, lo);
}
// The stored pair of a layer input (producer side, once per value): hi = fp16_rne(s x), lo = fp16_rne(s x - hi).  Round to
// nearest, not toward zero as in the in-register splits above: |lo| is at most half an ulp of hi (one more bit for the pair),
// and hi alone IS the correctly rounded fp16 of the value -- the fp16-operand mode reads only the hi plane.  (The block scale
// keeps |s x| below 2^14, so the conversion cannot overflow.)
__device__ __forceinline__ void store_pair8(const float (&v)[8], float s, f16x8& hi, f16x8& lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float t = v[e] * s;
        const _Float16 h = (_Float16)t;
        hi[e] = h;
        lo[e] = (_Float16)(t - (float)h);
    }
}
// biased exponent of a block maximum, clamped as blk_scale_exp clamps it (pk_split.h)
__device__ __forceinline__ int amax_exp(unsigned bits) {
    const int e = (int)(bits >> 23);
    return e < PK_EXP_MIN ? PK_EXP_MIN : (e > PK_EXP_MAX ? PK_EXP_MAX : e);
}
__device__ __forceinline__ f16x8 ld_h8(const char* p) { return *reinterpret_cast<const f16x8*>(p); }
__device__ __forceinline__ void st_h8(char* p, f16x8 v) { *reinterpret_cast<f16x8*>(p) = v; }

// wave-uniform maximum: five steps inside the rows of 16 lanes and across them on the data-parallel path, the result read
// from lane 63
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_max_step(float v) {
    const int t = __builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xf, false);
    return fmaxf(v, __int_as_float(t));
}
__device__ __forceinline__ float wave_max64(float v) {
    v = dpp_max_step<0xB1, 0xf>(v);
    v = dpp_max_step<0x4E, 0xf>(v);
    v = dpp_max_step<0x124, 0xf>(v);
    v = dpp_max_step<0x128, 0xf>(v);
    v = dpp_max_step<0x142, 0xa>(v);
    v = dpp_max_step<0x143, 0xc>(v);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// the gate of the LSTM cells (taco2.hip, spk.hip)
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }
