// sg_h16.hpp -- a lane's pair of 16-bit elements <-> fp32, for the stream kernels on 16-bit storage (sg_stream_dma_h16.hip, sg_stream.hip).  The storage
// type is a wave-uniform argument, as in sg_k1d_h16.hpp, whose converts these are: widening is exact (fp16 subnormals included: the hardware convert
// with the kernels' default denormal mode), narrowing rounds once to nearest even (NaN stays NaN, overflow into fp16 gives +-Inf).
#pragma once

#include <hip/hip_runtime.h>

#include "sg_pk.hpp"

namespace sg {

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16   bf16x2 __attribute__((ext_vector_type(2)));

// one dword as loaded (element 0 in the low half) -> two fp32
__device__ __forceinline__ f32x2 widen2(const unsigned raw, const bool bf)
{
    if (bf) return f32x2{__uint_as_float(raw << 16), __uint_as_float(raw & 0xffff0000u)};
    const f16x2 h = __builtin_bit_cast(f16x2, raw);
    return f32x2{(float)h.x, (float)h.y};
}
__device__ __forceinline__ float widen1(const unsigned short raw, const bool bf)
{
    if (bf) return __uint_as_float((unsigned)raw << 16);
    return (float)__builtin_bit_cast(_Float16, raw);
}
__device__ __forceinline__ unsigned narrow2(const f32x2 v, const bool bf)
{
    if (bf) return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
}
__device__ __forceinline__ unsigned short narrow1(const float v, const bool bf)
{
    if (bf) return __builtin_bit_cast(unsigned short, (__bf16)v);
    return __builtin_bit_cast(unsigned short, (_Float16)v);
}

}  // namespace sg
