// The next-input-embedding store shared by the encoder and every decoder head (encoder_decoder.hip, decoder_sample.hip):
// emb + wpe of 4 consecutive columns, written in the element type of the destination row.
#pragma once

#include "gemm_common.hpp"

namespace mli {

__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    auto cvt = [](float f) -> uint32_t {  // round to nearest even, NaN preserved
        uint32_t u = __float_as_uint(f);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x0040u;
        return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    };
    return cvt(lo) | (cvt(hi) << 16);
}

// emb + wpe of 4 consecutive columns -> fp32 row, bf16 row or fp8 (OCP e4m3) row; ELEM = MLI_ELEM_* (false / true = f32 / bf16)
template <int ELEM>
__device__ __forceinline__ void store_sum4(float* dst_row, int i4, const float4& a, const float4& c) {
    const float4 r = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
    if (ELEM == MLI_ELEM_FP8) reinterpret_cast<uint32_t*>(dst_row)[i4] = f32x4_to_fp8x4(r.x, r.y, r.z, r.w);
    else if (ELEM == MLI_ELEM_BF16) reinterpret_cast<uint2*>(dst_row)[i4] = make_uint2(pack_bf16x2(r.x, r.y), pack_bf16x2(r.z, r.w));
    else reinterpret_cast<float4*>(dst_row)[i4] = r;
}

// the row of position s in segment `seg` of a page whose elements are ELEM
template <int ELEM>
__device__ __forceinline__ float* page_row_ptr(float* page, int s, int D, int seg) {
    const int64_t off = page_row_offset(s, D, seg);
    if (ELEM == MLI_ELEM_FP8) return reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(page) + off);
    if (ELEM == MLI_ELEM_BF16) return reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(page) + off);
    return page + off;
}

}  // namespace mli
