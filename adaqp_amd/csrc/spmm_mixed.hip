// Mixed-precision SpMM for the fp32 backward aggregation (gfx950 / MI355X):
// the gathered rows are bf16, everything else stays fp32.
//
// The dense fp32 SpMM pulls 4F bytes per edge; at F = 256 that is eight
// 128-byte lines per row and the gather is bound by bytes. The backward
// operand (g @ W^T) is a dense GEMM output, so there is nothing to pack. What
// can be done is to gather half-width rows: the operand is cast once per
// propagation to bf16 with UNBIASED stochastic rounding (the treatment remote
// rows already get at 2/4/8 bits) and the SpMM gathers those, accumulating,
// scaling, adding the epilogue addend and storing in fp32.
//
// Two kernels:
//
// round_rows_bf16_kernel   one pass, contiguous fp32 [N, F] -> bf16 [N, F].
//   Element (row, f) draws h = hash_u32(seed ^ (t * 0x9E3779B9) ^
//   (f * 0x85EBCA6B)) with t = tag_base + row (the integer behind uniform01)
//   and stores (b + (h >> 16)) >> 16 of its bit pattern b: the low 16 bits
//   are rounded up with probability low16 / 2^16, so E[out] = x, and a carry
//   into the exponent is the rounding to the next binade (or to inf from the
//   last one). Inf/NaN keep their top half, NaN with the quiet bit set so a
//   payload in the low half does not turn into inf. -0.0 stays -0.0.
//   The tensor is walked as a flat array, lanes along the rows: a thread
//   reads one aligned 16-byte group of four consecutive elements and writes
//   their 8 bytes. With F % 4 != 0 a group can straddle a row end, so each
//   element carries its own (row, f), found with ONE division per thread and
//   a carry afterwards; the last N * F % 4 elements are the scalar tail.
//   No atomics: the same input and seed give the same bits.
//
// spmm_bf16in_kernel<SW, VE, SS>   spmm_csr_kernel's work split and
//   arithmetic (segments, partial slots, the XCD swizzle, four edges in
//   flight, edge j of a segment into accumulator j & 1 in increasing j, one
//   fmaf(to_f32(v), s, acc) per feature, epilogue (acc0 + acc1) * ds and
//   round_add<float>). Widening bf16 is exact, so the result equals the fp32
//   dense kernel fed the widened operands bit for bit.
//   Data movement: a lane owns VE in {8, 4, 2} consecutive features and
//   fetches them with one 16/8/4-byte load per edge; the sub-wavefront width
//   SW in {16, 32, 64} is the smallest covering F with VE per lane, so
//   F = 256 runs on 32 lanes (two segments per wavefront, against one for
//   the fp32 kernel) and a row is four 128-byte lines instead of eight. The
//   lane's VE fp32 results leave as 4 * VE bytes: two 16-byte stores for
//   VE = 8, one for VE = 4, one 8-byte store for VE = 2; the addend is read
//   the same way. Partial slots are fp32 and combine_parts_kernel<float>
//   (kernels.hip) sums them, as for the fp32 kernel. SS (a src_scale vector
//   is given) is a template flag: the no-scale variant carries no scale
//   loads and no per-edge branch.
//
// Built without packed fp32 instructions (v_pk_fma_f32 and kin), as
// spmm_quant.hip: a lane's fmafs are scalar v_fma_f32.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>

#include "device_common.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// ---------------------------------------------------------------------------
// stochastic-rounding cast
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint16_t sr_bf16(float x, uint32_t seed,
                                            uint32_t tag, uint32_t f) {
    const uint32_t b = __float_as_uint(x);
    if ((b & 0x7F800000u) == 0x7F800000u)
        return (uint16_t)((b >> 16) | ((b & 0x007FFFFFu) ? 0x0040u : 0u));
    const uint32_t h = hash_u32(seed ^ (tag * 0x9E3779B9u) ^ (f * 0x85EBCA6Bu));
    return (uint16_t)((b + (h >> 16)) >> 16);
}

#define RR_THREADS 256

__global__ void __launch_bounds__(RR_THREADS) round_rows_bf16_kernel(
    const float* __restrict__ x, uint16_t* __restrict__ out,
    int64_t total, uint32_t F, uint32_t seed, uint32_t tag_base) {
    const int64_t i0 = ((int64_t)blockIdx.x * RR_THREADS + threadIdx.x) * 4;
    if (i0 >= total) return;
    // (row, f) of element i0: 32-bit division whenever the tensor allows it
    // (uniform branch); the tag is u32 arithmetic, so only row's low half counts
    uint32_t row, f;
    if (total <= 0xFFFFFFFFll) {
        row = (uint32_t)i0 / F;
        f = (uint32_t)i0 - row * F;
    } else {
        const int64_t r = i0 / F;
        row = (uint32_t)r;
        f = (uint32_t)(i0 - r * F);
    }
    if (i0 + 4 <= total) {
        const float4 v = *reinterpret_cast<const float4*>(x + i0);
        const float vv[4] = {v.x, v.y, v.z, v.w};
        uint16_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k] = sr_bf16(vv[k], seed, tag_base + row, f);
            if (++f == F) { f = 0; ++row; }
        }
        uint2 w;
        w.x = (uint32_t)o[0] | ((uint32_t)o[1] << 16);
        w.y = (uint32_t)o[2] | ((uint32_t)o[3] << 16);
        *reinterpret_cast<uint2*>(out + i0) = w;
    } else {
        for (int64_t i = i0; i < total; ++i) {      // scalar tail
            out[i] = sr_bf16(x[i], seed, tag_base + row, f);
            if (++f == F) { f = 0; ++row; }
        }
    }
}

// ---------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------
// fp32 vector of N floats stored/loaded as 16-byte (or one 8-byte) pieces
template <int N>
__device__ __forceinline__ void store_f32(float* __restrict__ p,
                                          const float (&v)[N]) {
    if constexpr (N == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
    } else {
#pragma unroll
        for (int k = 0; k < N; k += 4)
            *reinterpret_cast<float4*>(p + k) =
                make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
    }
}

template <int N>
__device__ __forceinline__ void load_f32(const float* __restrict__ p,
                                         float (&v)[N]) {
    if constexpr (N == 2) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        v[0] = t.x; v[1] = t.y;
    } else {
#pragma unroll
        for (int k = 0; k < N; k += 4) {
            const float4 t = *reinterpret_cast<const float4*>(p + k);
            v[k] = t.x; v[k + 1] = t.y; v[k + 2] = t.z; v[k + 3] = t.w;
        }
    }
}

template <int SW, int VE, bool SS>
__global__ void __launch_bounds__(256) spmm_bf16in_kernel(
    const int32_t* __restrict__ indices,
    const ushort* __restrict__ xl, const ushort* __restrict__ xr,
    float* __restrict__ y,
    const float* __restrict__ src_scale, const float* __restrict__ dst_scale,
    const int32_t* __restrict__ seg_row, const int32_t* __restrict__ seg_e0,
    const int32_t* __restrict__ seg_e1, const int32_t* __restrict__ seg_part,
    float* __restrict__ part, const float* __restrict__ addend,
    int64_t n_seg, int64_t F, int64_t n_local) {
    using Raw = typename RawVec<VE * 2>::type;
    const int rows_per_block = blockDim.x / SW;
    // bijective XCD swizzle, as spmm_csr_kernel
    const int64_t nwg = gridDim.x;
    const int64_t q = nwg / 8, rem = nwg % 8;
    const int64_t xcd = blockIdx.x % 8, idx = blockIdx.x / 8;
    const int64_t swz = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + idx;
    const int64_t sub0 = swz * rows_per_block + threadIdx.x / SW;
    const int64_t stride = nwg * rows_per_block;
    const int sl = threadIdx.x & (SW - 1);

    for (int64_t it = sub0; it < n_seg; it += stride) {
        const int64_t r = seg_row[it];
        const int64_t e0 = seg_e0[it], e1 = seg_e1[it];
        const int64_t slot = seg_part[it];
        const float ds = dst_scale ? dst_scale[r] : 1.f;
        for (int64_t f0 = (int64_t)sl * VE; f0 < F; f0 += (int64_t)SW * VE) {
            float acc0[VE], acc1[VE];
#pragma unroll
            for (int k = 0; k < VE; ++k) { acc0[k] = 0.f; acc1[k] = 0.f; }

            // every batch starts at an even distance from e0, so edge
            // e + u goes to accumulator u & 1. All NB half-width row loads
            // are issued before the first fmaf (VE divides F: in bounds)
            auto batch = [&](int64_t e, auto nb_tag) {
                constexpr int NB = decltype(nb_tag)::value;
                float s[NB];
                Raw rv[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int64_t c = indices[e + u];
                    s[u] = SS ? src_scale[c] : 1.f;
                    const ushort* p = (c < n_local ? xl + c * F
                                                   : xr + (c - n_local) * F) + f0;
                    rv[u] = *reinterpret_cast<const Raw*>(p);
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const ushort* v = reinterpret_cast<const ushort*>(&rv[u]);
#pragma unroll
                    for (int k = 0; k < VE; ++k) {
                        if (u & 1) acc1[k] = fmaf(bf16_to_f32(v[k]), s[u], acc1[k]);
                        else acc0[k] = fmaf(bf16_to_f32(v[k]), s[u], acc0[k]);
                    }
                }
            };
            int64_t e = e0;
            for (; e + 3 < e1; e += 4) batch(e, std::integral_constant<int, 4>{});
            for (; e + 1 < e1; e += 2) batch(e, std::integral_constant<int, 2>{});
            if (e < e1) batch(e, std::integral_constant<int, 1>{});

            float outv[VE];
            if (slot < 0) {
                float ad[VE];
                if (addend) load_f32<VE>(addend + r * F + f0, ad);
#pragma unroll
                for (int k = 0; k < VE; ++k)
                    outv[k] = round_add<float>((acc0[k] + acc1[k]) * ds,
                                               addend ? ad + k : nullptr);
                store_f32<VE>(y + r * F + f0, outv);
            } else {
                // long row split across segments: fp32 partial into this
                // segment's own slot, summed by combine_parts_kernel<float>
#pragma unroll
                for (int k = 0; k < VE; ++k)
                    outv[k] = (acc0[k] + acc1[k]) * ds;
                store_f32<VE>(part + slot * F + f0, outv);
            }
        }
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
torch::Tensor round_rows_bf16(torch::Tensor x, int64_t seed, int64_t tag_base) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2 &&
                x.scalar_type() == torch::kFloat32,
                "round_rows_bf16 expects a contiguous fp32 [N, F] GPU tensor");
    const int64_t F = x.size(1), total = x.numel();
    TORCH_CHECK(F < (1ll << 32), "round_rows_bf16: F must fit 32 bits");
    torch::Tensor out = torch::empty({x.size(0), F},
                                     x.options().dtype(torch::kBFloat16));
    if (total == 0) return out;
    // the 16-byte loads and 8-byte stores start at the tensors' bases
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                reinterpret_cast<uintptr_t>(out.data_ptr()) % 8 == 0,
                "round_rows_bf16: x must start 16-byte aligned");
    const int64_t groups = (total + 3) / 4;
    const int64_t blocks = (groups + RR_THREADS - 1) / RR_THREADS;
    TORCH_CHECK(blocks < (1ll << 31), "round_rows_bf16: tensor too large");
    round_rows_bf16_kernel<<<dim3((unsigned)blocks), dim3(RR_THREADS), 0,
                             at::cuda::getCurrentHIPStream().stream()>>>(
        x.data_ptr<float>(),
        reinterpret_cast<uint16_t*>(out.data_ptr<at::BFloat16>()), total,
        (uint32_t)F, (uint32_t)seed, (uint32_t)tag_base);
    return out;
}

// vector width (bf16 elements per lane) and sub-wavefront width for F
void spmm_bf16in_shape(int64_t F, int* ve, int* sw) {
    int v = 8;
    while (v > 2 && F % v) v >>= 1;
    int s = 16;
    while (s < 64 && (int64_t)s * v < F) s *= 2;
    *ve = v;
    *sw = s;
}

// called by spmm_csr_bf16in (kernels.hip), which checked the operands and
// allocated the partial slots
void launch_spmm_bf16in(
    hipStream_t s, const int32_t* indices, const ushort* xl, const ushort* xr,
    float* y, const float* src_scale, const float* dst_scale,
    const int32_t* seg_row, const int32_t* seg_e0, const int32_t* seg_e1,
    const int32_t* seg_part, float* part, const float* addend,
    int64_t n_seg, int64_t F, int64_t n_local) {
    int ve, sw;
    spmm_bf16in_shape(F, &ve, &sw);
    TORCH_CHECK(F > 0 && F % ve == 0, "mixed spmm needs an even feature dim");
    const int block_threads = 256;
    const int rows_per_block = block_threads / sw;
    int64_t blocks = (n_seg + rows_per_block - 1) / rows_per_block;
    blocks = std::max<int64_t>(std::min<int64_t>(blocks, 16384), 1);
    const dim3 grid(blocks), block(block_threads);
#define LAUNCH(SWC, VEC, SSC) spmm_bf16in_kernel<SWC, VEC, SSC><<<grid, block, 0, s>>>( \
        indices, xl, xr, y, src_scale, dst_scale, seg_row, seg_e0, seg_e1, \
        seg_part, part, addend, n_seg, F, n_local)
#define BY_SS(SWC, VEC) do { \
        if (src_scale) LAUNCH(SWC, VEC, true); else LAUNCH(SWC, VEC, false); \
    } while (0)
#define BY_VE(SWC) do { \
        switch (ve) { \
            case 8: BY_SS(SWC, 8); break; \
            case 4: BY_SS(SWC, 4); break; \
            default: BY_SS(SWC, 2); break; \
        } \
    } while (0)
    switch (sw) {
        case 64: BY_VE(64); break;
        case 32: BY_VE(32); break;
        default: BY_VE(16); break;
    }
#undef BY_VE
#undef BY_SS
#undef LAUNCH
}
