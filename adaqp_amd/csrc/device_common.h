// Device helpers shared by every translation unit of adaqp_amd._C:
// the stateless counter-hash RNG and the bf16 <-> fp32 bit conversions.
// Single-sourced on purpose: quant_pack's stochastic rounding and
// norm_act's dropout mask must both match ops/quant.py::uniform_noise
// bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#define WAVE 64

// ---------------------------------------------------------------------------
// RNG: triple32 hash -> U[0,1). Must match ops/quant.py::_hash_u32 exactly.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t hash_u32(uint32_t h) {
    h ^= h >> 16; h *= 0x7FEB352Du;
    h ^= h >> 15; h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h;
}

__device__ __forceinline__ float uniform01(uint32_t seed, uint32_t tag, uint32_t feat) {
    uint32_t h = seed ^ (tag * 0x9E3779B9u) ^ (feat * 0x85EBCA6Bu);
    return (float)((double)hash_u32(h) * 2.3283064365386963e-10);
}

// round-to-nearest-even f32 -> bf16 bits (parity with torch .to(bfloat16))
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    uint32_t b = __float_as_uint(f);
    uint32_t r = (b + 0x7FFFu + ((b >> 16) & 1u)) >> 16;
    return (uint16_t)r;
}
__device__ __forceinline__ float bf16_to_f32(uint16_t h) {
    return __uint_as_float(((uint32_t)h) << 16);
}

// T = float (V=4 feats/lane) or ushort bf16 bits (V=8 feats/lane); fp32 accumulate.
template <typename T>
__device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<ushort>(ushort v) {
    return bf16_to_f32(v);
}

// ---------------------------------------------------------------------------
// SpMM helpers shared by kernels.hip and spmm_packed.hip
// ---------------------------------------------------------------------------
// Value stored to y for the fp32 SpMM result o. With an epilogue addend
// (ad != nullptr) o is first rounded to T — the value spmm alone stores —
// and the addend is added with a rounding of its own, never contracted
// into the dst-scale multiply that produced o, so y equals torch's
// ``spmm(...) + addend`` bit for bit (bf16: round, widen, add, round).
template <typename T>
__device__ __forceinline__ T round_add(float o, const T* ad) {
#pragma clang fp contract(off)
    if constexpr (sizeof(T) == 2) {
        uint16_t h = f32_to_bf16(o);
        if (ad) h = f32_to_bf16(bf16_to_f32(h) + bf16_to_f32(*ad));
        return h;
    } else {
        return ad ? o + *ad : o;
    }
}


// raw load/store type of NB bytes
template <int NB> struct RawVec;
template <> struct RawVec<16> { using type = uint4; };
template <> struct RawVec<8>  { using type = uint2; };
template <> struct RawVec<4>  { using type = unsigned; };
template <> struct RawVec<2>  { using type = ushort; };
