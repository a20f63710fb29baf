// CDNA4 (gfx950 / MI355X) HIP kernels for adaqp_amd.
//
// Reference parity: quant_cuda pack/unpack
// (/root/reference/AdaQP/util/quantization/src/quantization_cuda_kernel.cu:34-156)
// and DGL's update_all CSR SpMM (delegated by the reference at
// AdaQP/model/ops.py:30). MI355X-first redesign:
//
//  * quant_pack fuses per-node min/max + scale + stochastic round + bit-pack
//    + the per-(peer,bit-group) wire scatter into ONE kernel and ONE read
//    of x (lane-register staging for F<=1024; the reference computes
//    rmin/rmax with two torch reductions in Python first, then re-reads
//    x in the pack kernel).
//  * packing is along the FEATURE axis so each node is a contiguous byte
//    run: lane l owns (8/bits) consecutive features and emits whole bytes —
//    coalesced float4/float2/float loads and byte stores across the
//    64-wide wavefront (the reference packs along the node axis).
//  * RNG is a stateless counter hash (triple32) of (seed, node, feature) —
//    no curand state; bit-compatible with the CPU oracle in ops/quant.py.
//  * spmm_csr: one SUB-wavefront per destination-row segment (hub rows are
//    split; partial sums combined in fixed order), dtype-templated (fp32 / bf16 with fp32
//    accumulate), vector width chosen so row-base loads stay aligned, fused
//    src/dst degree scaling, XCD-aware block swizzle, int32 column indices
//    + segment bounds (half the index bytes), four gather loads in flight.
//
// Built for gfx950 only. No CUDA compatibility path.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>

#define CHECK_DEV(x) TORCH_CHECK(x.is_cuda(), #x " must be on the GPU")
#define CHECK_CONTIG(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

// hash_u32 / uniform01 / f32_to_bf16 / bf16_to_f32 / to_f32 and WAVE
#include "device_common.h"

// ---------------------------------------------------------------------------
// quant_pack: one wave per node.
//   rows[i]   : row of x to quantize
//   pos[i]    : wire node position (params slot + RNG tag)
//   off[i]    : wire byte offset of this node's payload
// Lane l owns features [l*vpb + k*WAVE*vpb, ...): it loads vpb consecutive
// floats, reduces min/max across the wave, then emits one byte per k.
// ---------------------------------------------------------------------------
template <int BITS, typename T>
__global__ void quant_pack_kernel(
    const T* __restrict__ x, const int64_t* __restrict__ rows,
    const int64_t* __restrict__ pos, const int64_t* __restrict__ off,
    int64_t n, int64_t F, int64_t ld, uint32_t seed,
    uint8_t* __restrict__ payload, uint16_t* __restrict__ params) {
    constexpr int VPB = 8 / BITS;          // values per byte
    constexpr int MAXV = 16;               // staged floats per lane
    constexpr int MAXCH = MAXV / VPB;      // register path covers F <= WAVE*MAXV
    const int64_t wid = (int64_t)blockIdx.x * (blockDim.x / WAVE)
                      + threadIdx.x / WAVE;
    if (wid >= n) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t row = rows[wid];
    const T* xr = x + row * ld;
    const int64_t bpn = (F * BITS + 7) / 8;

    // single pass over x: stage this lane's values in registers while
    // reducing min/max (the round-1 kernel read x twice). F beyond the
    // register budget falls back to the two-pass read below.
    const bool staged = F <= (int64_t)WAVE * MAXV;
    float vals[MAXV];
    float mn = 1e38f, mx = -1e38f;
    if (staged) {
#pragma unroll
        for (int c = 0; c < MAXCH; ++c) {
            const int64_t f0 = ((int64_t)lane + (int64_t)c * WAVE) * VPB;
            if (f0 >= F) break;
#pragma unroll
            for (int k = 0; k < VPB; ++k) {
                float v = 0.f;
                if (f0 + k < F) {
                    v = to_f32<T>(xr[f0 + k]);
                    mn = fminf(mn, v);
                    mx = fmaxf(mx, v);
                }
                vals[c * VPB + k] = v;
            }
        }
    } else {
        for (int64_t f0 = (int64_t)lane * VPB; f0 < F; f0 += (int64_t)WAVE * VPB) {
#pragma unroll
            for (int k = 0; k < VPB; ++k) {
                if (f0 + k < F) {
                    float v = to_f32<T>(xr[f0 + k]);
                    mn = fminf(mn, v);
                    mx = fmaxf(mx, v);
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    const float rng = mx - mn;
    float scale_f = rng > 0.f ? ((float)((1 << BITS) - 1)) / fmaxf(rng, 1e-30f) : 0.f;
    const uint16_t scale_h = f32_to_bf16(scale_f);
    const uint16_t rmin_h = f32_to_bf16(mn);
    const float scale = bf16_to_f32(scale_h);     // quantize with the wire scale
    const float rmin = bf16_to_f32(rmin_h);
    const int64_t p = pos[wid];
    if (lane == 0) {
        params[2 * p] = scale_h;
        params[2 * p + 1] = rmin_h;
    }
    const uint32_t tag = (uint32_t)p;

    // quantize + pack one byte per lane-step. The staged path is fully
    // unrolled so vals[] indices are compile-time constants (registers,
    // no scratch).
    uint8_t* out = payload + off[wid];
    if (staged) {
#pragma unroll
        for (int c = 0; c < MAXCH; ++c) {
            const int64_t b0 = (int64_t)lane + (int64_t)c * WAVE;
            if (b0 * VPB >= F) break;
            uint32_t byte = 0;
#pragma unroll
            for (int k = 0; k < VPB; ++k) {
                const int64_t f = b0 * VPB + k;
                if (f < F && scale > 0.f) {
                    float v = (vals[c * VPB + k] - rmin) * scale;
                    float u = uniform01(seed, tag, (uint32_t)f);
                    int q = (int)floorf(v + u);
                    q = max(0, min(q, (1 << BITS) - 1));
                    byte |= ((uint32_t)q) << (k * BITS);
                }
            }
            out[b0] = (uint8_t)byte;
        }
    } else {
        for (int64_t b0 = lane; b0 * VPB < F; b0 += WAVE) {
            uint32_t byte = 0;
#pragma unroll
            for (int k = 0; k < VPB; ++k) {
                const int64_t f = b0 * VPB + k;
                if (f < F && scale > 0.f) {
                    float v = (to_f32<T>(xr[f]) - rmin) * scale;
                    float u = uniform01(seed, tag, (uint32_t)f);
                    int q = (int)floorf(v + u);
                    q = max(0, min(q, (1 << BITS) - 1));
                    byte |= ((uint32_t)q) << (k * BITS);
                }
            }
            out[b0] = (uint8_t)byte;
        }
    }
}

// ---------------------------------------------------------------------------
// quant_unpack: one wave per node, fused scatter into out[rows[i]].
// ---------------------------------------------------------------------------
template <int BITS, typename T>
__global__ void quant_unpack_kernel(
    const uint8_t* __restrict__ payload, const uint16_t* __restrict__ params,
    const int64_t* __restrict__ rows, const int64_t* __restrict__ pos,
    const int64_t* __restrict__ off, int64_t n, int64_t F, int64_t ld,
    T* __restrict__ out) {
    constexpr bool BF = sizeof(T) == 2;
    constexpr int VPB = 8 / BITS;
    const int64_t wid = (int64_t)blockIdx.x * (blockDim.x / WAVE)
                      + threadIdx.x / WAVE;
    if (wid >= n) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t p = pos[wid];
    const float scale = bf16_to_f32(params[2 * p]);
    const float rmin = bf16_to_f32(params[2 * p + 1]);
    const float inv = scale > 0.f ? 1.f / scale : 0.f;
    const uint8_t* in = payload + off[wid];
    T* o = out + rows[wid] * ld;
    for (int64_t b0 = lane; b0 * VPB < F; b0 += WAVE) {
        const uint32_t byte = in[b0];
#pragma unroll
        for (int k = 0; k < VPB; ++k) {
            const int64_t f = b0 * VPB + k;
            if (f < F) {
                const int q = (byte >> (k * BITS)) & ((1 << BITS) - 1);
                const float v = (float)q * inv + rmin;
                if constexpr (BF) o[f] = f32_to_bf16(v);
                else o[f] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// spmm_csr: y[r] = dst_scale[r] * sum_{e in row r} src_scale[c_e] * x[c_e]
//
// One SUB-wavefront (SW in {16,32,64}, chosen to cover F) per destination-row
// SEGMENT (seg_* arrays; hub rows are split to <=SEG_EDGES edges; each such
// segment stores its fp32 partial into its own slot of a scratch buffer and
// combine_parts_kernel sums a row's slots in segment order, so the result
// is bit-identical from run to run). Lane sl owns features
// [VE*sl, VE*sl+VE) per chunk of VE*SW, VE picked host-side so the
// VE*sizeof(T)-byte row-base loads stay aligned (VE | F). Two edges are
// accumulated in flight (dual accumulators) to cover gather latency.
// Dual-tensor input: columns >= n_local read the REMOTE block directly
// (no [N,F] concat per layer). XCD-aware bijective block swizzle gives
// each XCD a contiguous chunk of work items so clustered neighbor rows
// hit the same L2 (guide §5.5 T1).
// ---------------------------------------------------------------------------
// round_add (the value stored to y, with the optional epilogue addend) and
// RawVec live in device_common.h, shared with spmm_packed.hip
// One wavefront per split row: y[rows[j]] = sum of its partial slots
// [part_ptr[j], part_ptr[j+1]) in slot order (an empty range writes zeros),
// plus the row's addend when one is given.
template <typename T>
__global__ void combine_parts_kernel(T* __restrict__ y,
                                     const float* __restrict__ part,
                                     const int32_t* __restrict__ rows,
                                     const int32_t* __restrict__ part_ptr,
                                     const T* __restrict__ addend,
                                     int64_t n, int64_t F) {
    const int64_t wid = (int64_t)blockIdx.x * (blockDim.x / WAVE)
                      + threadIdx.x / WAVE;
    if (wid >= n) return;
    T* p = y + (int64_t)rows[wid] * F;
    const T* a = addend ? addend + (int64_t)rows[wid] * F : nullptr;
    const int64_t p0 = part_ptr[wid], p1 = part_ptr[wid + 1];
    for (int64_t f = threadIdx.x & (WAVE - 1); f < F; f += WAVE) {
        float acc = 0.f;
        for (int64_t q = p0; q < p1; ++q) acc += part[q * F + f];
        p[f] = round_add<T>(acc, a ? a + f : nullptr);
    }
}

// VE = elements per lane per load; chosen host-side as the largest of
// {8,4,2}(bf16) / {4,2,1}(f32) dividing F, so every row-base load of
// width VE*sizeof(T) is aligned (rows are x + c*F*sizeof(T)).
template <int SW, typename T, int VE>
__global__ void spmm_csr_kernel(
    const int32_t* __restrict__ indices,   // int32: halves index bytes
    const T* __restrict__ xl, const T* __restrict__ xr,
    T* __restrict__ y,
    const float* __restrict__ src_scale, const float* __restrict__ dst_scale,
    const int32_t* __restrict__ seg_row, const int32_t* __restrict__ seg_e0,
    const int32_t* __restrict__ seg_e1, const int32_t* __restrict__ seg_part,
    float* __restrict__ part, const T* __restrict__ addend,
    int64_t n_seg, int64_t F, int64_t n_local) {
    constexpr int NB = VE * sizeof(T);
    using Raw = typename RawVec<NB>::type;
    const int rows_per_block = blockDim.x / SW;
    // bijective XCD swizzle: blocks [0,nwg) -> xcd-contiguous chunks
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
        const int64_t slot = seg_part[it];     // >= 0: row split across segments
        const float ds = dst_scale ? dst_scale[r] : 1.f;
        for (int64_t f0 = (int64_t)sl * VE; f0 < F; f0 += (int64_t)SW * VE) {
            float acc0[VE], acc1[VE];
#pragma unroll
            for (int k = 0; k < VE; ++k) { acc0[k] = 0.f; acc1[k] = 0.f; }
            int64_t e = e0;
            // FOUR edges in flight: the gather is latency-bound on L2
            // misses; independent loads + accumulator pairs keep more
            // of them outstanding (round-1 version had two)
            for (; e + 3 < e1; e += 4) {
                const int64_t c0 = indices[e],     c1 = indices[e + 1];
                const int64_t c2 = indices[e + 2], c3 = indices[e + 3];
                const float s0 = src_scale ? src_scale[c0] : 1.f;
                const float s1 = src_scale ? src_scale[c1] : 1.f;
                const float s2 = src_scale ? src_scale[c2] : 1.f;
                const float s3 = src_scale ? src_scale[c3] : 1.f;
                const T* p0 = (c0 < n_local ? xl + c0 * F : xr + (c0 - n_local) * F) + f0;
                const T* p1 = (c1 < n_local ? xl + c1 * F : xr + (c1 - n_local) * F) + f0;
                const T* p2 = (c2 < n_local ? xl + c2 * F : xr + (c2 - n_local) * F) + f0;
                const T* p3 = (c3 < n_local ? xl + c3 * F : xr + (c3 - n_local) * F) + f0;
                const Raw r0 = *reinterpret_cast<const Raw*>(p0);
                const Raw r1 = *reinterpret_cast<const Raw*>(p1);
                const Raw r2 = *reinterpret_cast<const Raw*>(p2);
                const Raw r3 = *reinterpret_cast<const Raw*>(p3);
                const T* v0 = reinterpret_cast<const T*>(&r0);
                const T* v1 = reinterpret_cast<const T*>(&r1);
                const T* v2 = reinterpret_cast<const T*>(&r2);
                const T* v3 = reinterpret_cast<const T*>(&r3);
#pragma unroll
                for (int k = 0; k < VE; ++k) {
                    acc0[k] = fmaf(to_f32<T>(v0[k]), s0, acc0[k]);
                    acc1[k] = fmaf(to_f32<T>(v1[k]), s1, acc1[k]);
                    acc0[k] = fmaf(to_f32<T>(v2[k]), s2, acc0[k]);
                    acc1[k] = fmaf(to_f32<T>(v3[k]), s3, acc1[k]);
                }
            }
            for (; e + 1 < e1; e += 2) {   // VE divides F: loads always in-bounds
                const int64_t c0 = indices[e];
                const int64_t c1 = indices[e + 1];
                const float s0 = src_scale ? src_scale[c0] : 1.f;
                const float s1 = src_scale ? src_scale[c1] : 1.f;
                const T* p0 = (c0 < n_local ? xl + c0 * F : xr + (c0 - n_local) * F) + f0;
                const T* p1 = (c1 < n_local ? xl + c1 * F : xr + (c1 - n_local) * F) + f0;
                const Raw r0 = *reinterpret_cast<const Raw*>(p0);
                const Raw r1 = *reinterpret_cast<const Raw*>(p1);
                const T* v0 = reinterpret_cast<const T*>(&r0);
                const T* v1 = reinterpret_cast<const T*>(&r1);
#pragma unroll
                for (int k = 0; k < VE; ++k) {
                    acc0[k] = fmaf(to_f32<T>(v0[k]), s0, acc0[k]);
                    acc1[k] = fmaf(to_f32<T>(v1[k]), s1, acc1[k]);
                }
            }
            for (; e < e1; ++e) {
                const int64_t c = indices[e];
                const float s = src_scale ? src_scale[c] : 1.f;
                const T* xc = (c < n_local ? xl + c * F : xr + (c - n_local) * F) + f0;
                const Raw rv = *reinterpret_cast<const Raw*>(xc);
                const T* v = reinterpret_cast<const T*>(&rv);
#pragma unroll
                for (int k = 0; k < VE; ++k)
                    acc0[k] = fmaf(to_f32<T>(v[k]), s, acc0[k]);
            }
            T* yr = y + r * F + f0;
            if (slot < 0) {
                Raw av = {};
                if (addend)
                    av = *reinterpret_cast<const Raw*>(addend + r * F + f0);
                const T* ad = reinterpret_cast<const T*>(&av);
                T outv[VE];
#pragma unroll
                for (int k = 0; k < VE; ++k)
                    outv[k] = round_add<T>((acc0[k] + acc1[k]) * ds,
                                           addend ? ad + k : nullptr);
                *reinterpret_cast<Raw*>(yr) = *reinterpret_cast<const Raw*>(outv);
            } else {
                // long row split across segments: fp32 partial into this
                // segment's own slot, summed by combine_parts_kernel
                float* pp = part + slot * F + f0;
#pragma unroll
                for (int k = 0; k < VE; ++k)
                    pp[k] = (acc0[k] + acc1[k]) * ds;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// spmm_csr, wave-uniform index path (the SW == 64 case: one whole wavefront
// per segment). Same result as spmm_csr_kernel<64, T, VE> bit for bit — edge
// j of a segment goes into accumulator j & 1 in increasing j, one fmaf each,
// epilogue (acc0 + acc1) * ds — but the per-edge integer work is done once
// per wave instead of once per lane: the segment record is read through
// scalar registers, each chunk of 64 column indices (and their src_scale
// values) is fetched with ONE coalesced load, lane l holding edge eb + l,
// and every edge's column/scale is broadcast with readlane, so the
// local/remote select and the row base address are scalar arithmetic. Only
// the 16-byte row loads and the FMAs remain per lane.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float readlane_f32(float v, int l) {
    return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), l));
}

// accumulate edges [0, n) of one index chunk held one-per-lane in myc/mys:
// batches of 4, then 2, then 1 row loads in flight, as spmm_csr_kernel.
// Every batch starts at an even j (chunks before a segment's last hold 64
// edges), so edge j + u goes to accumulator u & 1. (Eight loads in flight
// measured the same as four on the products-like microbench: the gather
// runs at the memory system's rate either way.)
template <typename T, int VE, bool SS>
__device__ __forceinline__ void spmm_chunk(
    int myc, float mys, int n, const T* __restrict__ xl,
    const T* __restrict__ xr, int64_t F, int64_t n_local, int64_t f0,
    float (&acc0)[VE], float (&acc1)[VE]) {
    using Raw = typename RawVec<VE * sizeof(T)>::type;
    // columns, n_local and F all fit 32 bits (host-checked): the select
    // and the 32x32->64 row offset stay short scalar sequences
    const uint32_t nl = (uint32_t)n_local, Fu = (uint32_t)F;
    auto row = [&](int j) -> const T* {
        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane(myc, j);
        const bool loc = c < nl;
        const T* base = loc ? xl : xr;
        return base + (uint64_t)(loc ? c : c - nl) * Fu + f0;
    };
    auto batch = [&](int j, auto nb_tag) {
        constexpr int NB = decltype(nb_tag)::value;
        float s[NB];
        Raw r[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            s[u] = SS ? readlane_f32(mys, j + u) : 1.f;
            r[u] = *reinterpret_cast<const Raw*>(row(j + u));
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const T* v = reinterpret_cast<const T*>(&r[u]);
#pragma unroll
            for (int k = 0; k < VE; ++k) {
                if (u & 1) acc1[k] = fmaf(to_f32<T>(v[k]), s[u], acc1[k]);
                else acc0[k] = fmaf(to_f32<T>(v[k]), s[u], acc0[k]);
            }
        }
    };
    int j = 0;
    for (; j + 3 < n; j += 4) batch(j, std::integral_constant<int, 4>{});
    for (; j + 1 < n; j += 2) batch(j, std::integral_constant<int, 2>{});
    if (j < n) batch(j, std::integral_constant<int, 1>{});
}

template <typename T, int VE>
__global__ void spmm_csr_wave_kernel(
    const int32_t* __restrict__ indices,
    const T* __restrict__ xl, const T* __restrict__ xr,
    T* __restrict__ y,
    const float* __restrict__ src_scale, const float* __restrict__ dst_scale,
    const int32_t* __restrict__ seg_row, const int32_t* __restrict__ seg_e0,
    const int32_t* __restrict__ seg_e1, const int32_t* __restrict__ seg_part,
    float* __restrict__ part, const T* __restrict__ addend,
    int64_t n_seg, int64_t F, int64_t n_local) {
    using Raw = typename RawVec<VE * sizeof(T)>::type;
    const int waves_per_block = blockDim.x / WAVE;
    // same bijective XCD swizzle as spmm_csr_kernel
    const int64_t nwg = gridDim.x;
    const int64_t q = nwg / 8, rem = nwg % 8;
    const int64_t xcd = blockIdx.x % 8, idx = blockIdx.x / 8;
    const int64_t swz = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + idx;
    // the wave id is uniform but not provably so: readfirstlane it, and
    // everything read through it lands in scalar registers
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t stride = nwg * waves_per_block;

    for (int64_t it = swz * waves_per_block + wave; it < n_seg; it += stride) {
        const int64_t r = __builtin_amdgcn_readfirstlane(seg_row[it]);
        const int e0 = __builtin_amdgcn_readfirstlane(seg_e0[it]);
        const int e1 = __builtin_amdgcn_readfirstlane(seg_e1[it]);
        const int slot = __builtin_amdgcn_readfirstlane(seg_part[it]);
        const float ds = dst_scale
            ? __uint_as_float(__builtin_amdgcn_readfirstlane(
                  __float_as_uint(dst_scale[r])))
            : 1.f;
        for (int64_t fc = 0; fc < F; fc += (int64_t)WAVE * VE) {
            // lanes past F (F < 64*VE, or the last chunk of a wider row)
            // still take part in the index loads; they gather from
            // feature 0 (in bounds, VE | F) and store nothing
            const int64_t fl = fc + (int64_t)lane * VE;
            const bool active = fl < F;
            const int64_t f0 = active ? fl : 0;
            float acc0[VE], acc1[VE];
#pragma unroll
            for (int k = 0; k < VE; ++k) { acc0[k] = 0.f; acc1[k] = 0.f; }
            for (int eb = e0; eb < e1; eb += WAVE) {
                const int n = min(e1 - eb, WAVE);
                int myc = 0;
                float mys = 1.f;
                if (lane < n) {
                    myc = indices[eb + lane];
                    if (src_scale) mys = src_scale[myc];
                }
                if (src_scale)
                    spmm_chunk<T, VE, true>(myc, mys, n, xl, xr, F, n_local,
                                            f0, acc0, acc1);
                else
                    spmm_chunk<T, VE, false>(myc, mys, n, xl, xr, F, n_local,
                                             f0, acc0, acc1);
            }
            if (!active) continue;
            if (slot < 0) {
                Raw av = {};
                if (addend)
                    av = *reinterpret_cast<const Raw*>(addend + r * F + f0);
                const T* ad = reinterpret_cast<const T*>(&av);
                T outv[VE];
#pragma unroll
                for (int k = 0; k < VE; ++k)
                    outv[k] = round_add<T>((acc0[k] + acc1[k]) * ds,
                                           addend ? ad + k : nullptr);
                *reinterpret_cast<Raw*>(y + r * F + f0) =
                    *reinterpret_cast<const Raw*>(outv);
            } else {
                float* pp = part + (int64_t)slot * F + f0;
#pragma unroll
                for (int k = 0; k < VE; ++k)
                    pp[k] = (acc0[k] + acc1[k]) * ds;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// fused dual GEMM (bf16, MFMA): out[M,N] = A1@W1 + A2@W2 + bias
//
// The SAGE 'mean' layer computes fc_self(x) + fc_neigh(h) + biases — two
// rocBLAS GEMMs plus an elementwise add, writing/reading the [M,N] output
// three times. This kernel produces it in ONE pass: per 64-row block, the
// TRANSPOSED weights (Wt = W.T, [N,K]) are staged through LDS (shared by
// the block's 4 waves; W1 first, then W2), and each wave accumulates its
// 16xN rows with v_mfma_f32_16x16x32_bf16. fp32 accumulate, bf16 I/O.
// Fragment layouts per guide §3: A row = lane&15, k = (lane>>4)*8+j;
// B col = lane&15, same k; C/D col = lane&15, row = (lane>>4)*4+reg.
// ---------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define FDG_MAXNT 16      // N <= 256

__device__ __forceinline__ bf16x8 load_bf16x8(const ushort* p) {
    uint4 raw = *reinterpret_cast<const uint4*>(p);
    return *reinterpret_cast<const bf16x8*>(&raw);
}

__global__ void __launch_bounds__(256)
fused_dual_gemm_bf16_kernel(
    const ushort* __restrict__ a1, const ushort* __restrict__ a2,
    const ushort* __restrict__ w1t, const ushort* __restrict__ w2t,
    const ushort* __restrict__ bias,     // [N] bf16 (b1+b2), may be null
    ushort* __restrict__ out,
    int64_t M, int64_t N, int64_t K1, int64_t K2) {
    // Wt fragments are read straight from global: the whole weight set
    // (<=256KB) is L2-resident and re-read by every block; LDS staging
    // was measured SLOWER (135KB/block -> 1 block/CU, no latency hiding).
    const int wid = threadIdx.x / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t row0 = (int64_t)blockIdx.x * 64 + wid * 16;
    const int arow = lane & 15;          // A row / B col within a 16-tile
    const int kgrp = lane >> 4;          // k sub-block (8 elems each)
    const int NT = (int)(N / 16);

    f32x4 acc[FDG_MAXNT];
#pragma unroll
    for (int nt = 0; nt < FDG_MAXNT; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};

    for (int pass = 0; pass < 2; ++pass) {
        const ushort* A = pass ? a2 : a1;
        const ushort* Wt = pass ? w2t : w1t;
        const int64_t K = pass ? K2 : K1;
        const int64_t arow_g = row0 + arow;
        const ushort* arow_p = A + arow_g * K;
        const ushort* wt_p = Wt + arow * K;   // row (=out col) within 16-tile
        // double-buffered K pipeline: while the MFMAs of chunk i issue,
        // the loads of chunk i+1 are already in flight (round-1 version
        // had no K-pipelining — every chunk stalled on L2/HBM latency)
        bf16x8 af0 = {}, af1 = {};
        bf16x8 b0[FDG_MAXNT], b1[FDG_MAXNT];
        auto load_chunk = [&](int64_t k, bf16x8& af, bf16x8* bfr) {
            af = (arow_g < M && k < K) ? load_bf16x8(arow_p + k) : bf16x8{};
#pragma unroll
            for (int nt = 0; nt < FDG_MAXNT; ++nt) {
                if (nt >= NT) break;
                bfr[nt] = (k < K) ? load_bf16x8(wt_p + (int64_t)nt * 16 * K + k)
                                  : bf16x8{};
            }
        };
        auto mfma_chunk = [&](const bf16x8& af, const bf16x8* bfr) {
#pragma unroll
            for (int nt = 0; nt < FDG_MAXNT; ++nt) {
                if (nt >= NT) break;
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    af, bfr[nt], acc[nt], 0, 0, 0);
            }
        };
        load_chunk(kgrp * 8, af0, b0);
        for (int64_t k0 = 0; k0 < K; k0 += 64) {
            if (k0 + 32 < K) load_chunk(k0 + 32 + kgrp * 8, af1, b1);
            mfma_chunk(af0, b0);
            if (k0 + 64 < K) load_chunk(k0 + 64 + kgrp * 8, af0, b0);
            if (k0 + 32 < K) mfma_chunk(af1, b1);
        }
    }

    // epilogue: bias + bf16 store. C/D: col = lane&15, row = kgrp*4 + q
#pragma unroll
    for (int nt = 0; nt < FDG_MAXNT; ++nt) {
        if (nt >= NT) break;
        const int col = nt * 16 + arow;
        const float bv = bias ? bf16_to_f32(bias[col]) : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t r = row0 + kgrp * 4 + q;
            if (r < M)
                out[r * N + col] = f32_to_bf16(acc[nt][q] + bv);
        }
    }
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
// spmm_packed.hip
bool spmm_packable(int64_t F);
int64_t packed_meta_bytes(int64_t F);
int64_t packed_row_stride(int64_t F);
int64_t packed_buffer_bytes(int64_t n, int64_t F);
torch::Tensor pack_rows(torch::Tensor x);
void launch_spmm_packed(
    dim3 grid, dim3 block, hipStream_t s, int depth,
    const int32_t* indices, const float* xl, const float* xr,
    const uint8_t* pk, float* y, const float* src_scale,
    const float* dst_scale, const int32_t* seg_row, const int32_t* seg_e0,
    const int32_t* seg_e1, const int32_t* seg_part, float* part,
    const float* addend, int64_t n_seg, int64_t F, int64_t n_local);

static inline hipStream_t cur_stream() {
    return at::cuda::getCurrentHIPStream().stream();
}

void quant_pack(torch::Tensor x, torch::Tensor rows, torch::Tensor pos,
                torch::Tensor off, int64_t bits, int64_t seed,
                torch::Tensor payload, torch::Tensor params) {
    CHECK_DEV(x); CHECK_CONTIG(x); CHECK_DEV(rows); CHECK_DEV(payload); CHECK_DEV(params);
    const bool bf16 = x.scalar_type() == torch::kBFloat16;
    TORCH_CHECK(bf16 || x.scalar_type() == torch::kFloat32,
                "quant_pack expects fp32 or bf16");
    const int64_t n = rows.numel();
    if (n == 0) return;
    const int64_t F = x.size(1), ld = x.stride(0);
    const int waves_per_block = 4;
    const dim3 block(WAVE * waves_per_block);
    const dim3 grid((n + waves_per_block - 1) / waves_per_block);
    auto s = cur_stream();
#define LAUNCH(B, T) quant_pack_kernel<B, T><<<grid, block, 0, s>>>( \
        reinterpret_cast<const T*>(x.data_ptr()), rows.data_ptr<int64_t>(), \
        pos.data_ptr<int64_t>(), \
        off.data_ptr<int64_t>(), n, F, ld, (uint32_t)seed, \
        payload.data_ptr<uint8_t>(), reinterpret_cast<uint16_t*>(params.data_ptr<at::BFloat16>()))
    switch (bits) {
        case 2: if (bf16) LAUNCH(2, ushort); else LAUNCH(2, float); break;
        case 4: if (bf16) LAUNCH(4, ushort); else LAUNCH(4, float); break;
        case 8: if (bf16) LAUNCH(8, ushort); else LAUNCH(8, float); break;
        default: TORCH_CHECK(false, "bits must be 2/4/8");
    }
#undef LAUNCH
}

void quant_unpack(torch::Tensor payload, torch::Tensor params, torch::Tensor rows,
                  torch::Tensor pos, torch::Tensor off, int64_t bits, int64_t F,
                  torch::Tensor out) {
    CHECK_DEV(payload); CHECK_DEV(out); CHECK_CONTIG(out);
    const bool bf16 = out.scalar_type() == torch::kBFloat16;
    TORCH_CHECK(bf16 || out.scalar_type() == torch::kFloat32,
                "quant_unpack expects fp32 or bf16 out");
    const int64_t n = rows.numel();
    if (n == 0) return;
    const int waves_per_block = 4;
    const dim3 block(WAVE * waves_per_block);
    const dim3 grid((n + waves_per_block - 1) / waves_per_block);
    auto s = cur_stream();
#define LAUNCH(B, T) quant_unpack_kernel<B, T><<<grid, block, 0, s>>>( \
        payload.data_ptr<uint8_t>(), \
        reinterpret_cast<uint16_t*>(params.data_ptr<at::BFloat16>()), \
        rows.data_ptr<int64_t>(), pos.data_ptr<int64_t>(), off.data_ptr<int64_t>(), \
        n, F, out.stride(0), reinterpret_cast<T*>(out.data_ptr()))
    switch (bits) {
        case 2: if (bf16) LAUNCH(2, ushort); else LAUNCH(2, float); break;
        case 4: if (bf16) LAUNCH(4, ushort); else LAUNCH(4, float); break;
        case 8: if (bf16) LAUNCH(8, ushort); else LAUNCH(8, float); break;
        default: TORCH_CHECK(false, "bits must be 2/4/8");
    }
#undef LAUNCH
}

void spmm_csr(torch::Tensor indices, torch::Tensor xl,
              torch::Tensor xr, torch::Tensor y, torch::Tensor src_scale,
              torch::Tensor dst_scale, torch::Tensor seg_row,
              torch::Tensor seg_e0, torch::Tensor seg_e1,
              torch::Tensor seg_part, torch::Tensor zero_rows,
              torch::Tensor part_ptr, int64_t n_part,
              torch::Tensor addend, bool wave_index,
              torch::Tensor packed, int64_t packed_depth) {
    CHECK_DEV(xl); CHECK_CONTIG(xl); CHECK_DEV(y); CHECK_CONTIG(y);
    const bool bf16 = xl.scalar_type() == torch::kBFloat16;
    TORCH_CHECK(bf16 || xl.scalar_type() == torch::kFloat32,
                "spmm_csr expects fp32 or bf16");
    TORCH_CHECK(y.scalar_type() == xl.scalar_type(), "x/y dtype mismatch");
    const int64_t F = xl.size(1);
    const int64_t n_local = xl.size(0);
    const int64_t n_seg = seg_row.numel();
    const void* xr_ptr = nullptr;
    if (xr.numel()) {
        CHECK_DEV(xr); CHECK_CONTIG(xr);
        TORCH_CHECK(xr.size(1) == F, "remote feature dim mismatch");
        TORCH_CHECK(xr.scalar_type() == xl.scalar_type(), "x dtype mismatch");
        xr_ptr = xr.data_ptr();
    }
    // optional epilogue addend: y = spmm + addend ([nrows, F], y's dtype)
    const void* ad_ptr = nullptr;
    if (addend.dim() == 2) {        // a 1-D empty tensor means "none"
        CHECK_DEV(addend); CHECK_CONTIG(addend);
        TORCH_CHECK(addend.size(0) == y.size(0) && addend.size(1) == F,
                    "addend must be [nrows, F]");
        TORCH_CHECK(addend.scalar_type() == y.scalar_type(),
                    "addend/y dtype mismatch");
        ad_ptr = addend.numel() ? addend.data_ptr() : nullptr;
    }
    auto s = cur_stream();
    TORCH_CHECK(seg_part.scalar_type() == torch::kInt32 &&
                seg_part.numel() == n_seg &&
                zero_rows.scalar_type() == torch::kInt32 &&
                part_ptr.scalar_type() == torch::kInt32 &&
                part_ptr.numel() == zero_rows.numel() + 1,
                "seg_part/zero_rows/part_ptr must be the int32 arrays "
                "SpmmView builds");
    // one fp32 [F] slot per segment of a split row (SpmmView.n_part of them)
    TORCH_CHECK(n_part >= 0 && n_part <= n_seg, "bad partial slot count");
    torch::Tensor part = torch::empty(
        {n_part, F}, xl.options().dtype(torch::kFloat32));
    auto combine = [&]() {
        if (!zero_rows.numel()) return;
        const dim3 zb(256), zg((zero_rows.numel() + 3) / 4);
        if (bf16)
            combine_parts_kernel<ushort><<<zg, zb, 0, s>>>(
                reinterpret_cast<ushort*>(y.data_ptr()),
                part.data_ptr<float>(), zero_rows.data_ptr<int32_t>(),
                part_ptr.data_ptr<int32_t>(),
                reinterpret_cast<const ushort*>(ad_ptr), zero_rows.numel(), F);
        else
            combine_parts_kernel<float><<<zg, zb, 0, s>>>(
                y.data_ptr<float>(), part.data_ptr<float>(),
                zero_rows.data_ptr<int32_t>(), part_ptr.data_ptr<int32_t>(),
                reinterpret_cast<const float*>(ad_ptr), zero_rows.numel(), F);
    };
    if (n_seg == 0) { combine(); return; }
    // largest vector width dividing F (keeps every row-base load aligned)
    int ve = bf16 ? 8 : 4;
    while (ve > 1 && F % ve) ve >>= 1;
    if (bf16 && ve == 1) ve = 2;              // bf16 loads are >= one dword
    TORCH_CHECK(!bf16 || F % 2 == 0, "bf16 spmm needs even feature dim");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(ad_ptr) % (ve * (bf16 ? 2 : 4)) == 0,
                "addend rows must be aligned to the vector load width");
    // sub-wavefront width: smallest of {16,32,64} covering F with ve/lane
    int sw = 16;
    while (sw < 64 && (int64_t)sw * ve < F) sw *= 2;
    const int block_threads = WAVE * 4;
    const int rows_per_block = block_threads / sw;
    int64_t blocks = (n_seg + rows_per_block - 1) / rows_per_block;
    blocks = std::max<int64_t>(std::min<int64_t>(blocks, 16384), 1);
    const dim3 grid(blocks), block(block_threads);
    TORCH_CHECK(indices.scalar_type() == torch::kInt32,
                "spmm_csr expects int32 indices (SpmmView builds them)");
    const int32_t* ind_p = indices.data_ptr<int32_t>();
    const float* ss_p = src_scale.numel() ? src_scale.data_ptr<float>() : nullptr;
    const float* ds_p = dst_scale.numel() ? dst_scale.data_ptr<float>() : nullptr;
    const int32_t* sr_p = seg_row.data_ptr<int32_t>();
    TORCH_CHECK(seg_e0.scalar_type() == torch::kInt32 &&
                seg_e1.scalar_type() == torch::kInt32,
                "seg_e0/e1 must be int32 (SpmmView builds them)");
    const int32_t* e0_p = seg_e0.data_ptr<int32_t>();
    const int32_t* e1_p = seg_e1.data_ptr<int32_t>();
    const int32_t* sp_p = seg_part.data_ptr<int32_t>();
    // packed operand (pack_rows(xl); a 0-element tensor means "none"):
    // local columns are gathered from it, the result is the same bits
    if (packed.numel()) {
        CHECK_DEV(packed); CHECK_CONTIG(packed);
        TORCH_CHECK(!bf16 && spmm_packable(F) && n_local > 0,
                    "packed spmm expects fp32, F % 4 == 0, F <= 256 and "
                    "at least one local row");
        TORCH_CHECK(packed.scalar_type() == torch::kUInt8 &&
                    packed.numel() == packed_buffer_bytes(n_local, F),
                    "packed operand does not match xl (pack_rows(xl))");
        launch_spmm_packed(
            grid, block, s, (int)packed_depth, ind_p, xl.data_ptr<float>(),
            reinterpret_cast<const float*>(xr_ptr),
            packed.data_ptr<uint8_t>(), y.data_ptr<float>(), ss_p, ds_p,
            sr_p, e0_p, e1_p, sp_p, part.data_ptr<float>(),
            reinterpret_cast<const float*>(ad_ptr), n_seg, F, n_local);
        combine();
        return;
    }
    auto run = [&](auto sw_tag, auto t_tag, auto ve_tag) {
        constexpr int SWC = decltype(sw_tag)::value;
        using TC = typename decltype(t_tag)::type;
        constexpr int VEC = decltype(ve_tag)::value;
        // SW == 64: the whole wavefront owns one segment, so the index
        // work can be wave-uniform; wave_index selects that kernel, the
        // per-lane one stays the default (A/B runs, the equality test)
        if constexpr (SWC == 64) {
            if (wave_index) {
                TORCH_CHECK(F < (1ll << 31) && n_local < (1ll << 31),
                            "spmm_csr: F and n_local must fit 31 bits");
                spmm_csr_wave_kernel<TC, VEC><<<grid, block, 0, s>>>(
                    ind_p, reinterpret_cast<const TC*>(xl.data_ptr()),
                    reinterpret_cast<const TC*>(xr_ptr),
                    reinterpret_cast<TC*>(y.data_ptr()), ss_p, ds_p,
                    sr_p, e0_p, e1_p, sp_p, part.data_ptr<float>(),
                    reinterpret_cast<const TC*>(ad_ptr), n_seg, F, n_local);
                return;
            }
        }
        spmm_csr_kernel<SWC, TC, VEC><<<grid, block, 0, s>>>(
            ind_p, reinterpret_cast<const TC*>(xl.data_ptr()),
            reinterpret_cast<const TC*>(xr_ptr),
            reinterpret_cast<TC*>(y.data_ptr()), ss_p, ds_p,
            sr_p, e0_p, e1_p, sp_p, part.data_ptr<float>(),
            reinterpret_cast<const TC*>(ad_ptr), n_seg, F, n_local);
    };
    struct FT { using type = float; };
    struct BT { using type = ushort; };
    auto by_ve = [&](auto sw_tag) {
        if (bf16) {
            switch (ve) {
                case 8: run(sw_tag, BT{}, std::integral_constant<int,8>{}); break;
                case 4: run(sw_tag, BT{}, std::integral_constant<int,4>{}); break;
                default: run(sw_tag, BT{}, std::integral_constant<int,2>{}); break;
            }
        } else {
            switch (ve) {
                case 4: run(sw_tag, FT{}, std::integral_constant<int,4>{}); break;
                case 2: run(sw_tag, FT{}, std::integral_constant<int,2>{}); break;
                default: run(sw_tag, FT{}, std::integral_constant<int,1>{}); break;
            }
        }
    };
    switch (sw) {
        case 64: by_ve(std::integral_constant<int,64>{}); break;
        case 32: by_ve(std::integral_constant<int,32>{}); break;
        default: by_ve(std::integral_constant<int,16>{}); break;
    }
    combine();
}


// norm_act.hip
void norm_act_fwd(torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
                  double eps, double p, int64_t seed, bool training,
                  torch::Tensor y, torch::Tensor mean, torch::Tensor rstd);
torch::Tensor norm_act_bwd(torch::Tensor dy, torch::Tensor x,
                           torch::Tensor mean, torch::Tensor rstd,
                           torch::Tensor weight, torch::Tensor bias,
                           double p, int64_t seed, bool training,
                           torch::Tensor dx);
int64_t norm_act_bwd_max_blocks();
int64_t norm_act_waves_per_block();
int64_t norm_act_max_feats();

// colsum.hip
torch::Tensor colsum(torch::Tensor g);

// masked_loss.hip
std::vector<torch::Tensor> masked_loss_fwd(torch::Tensor logits,
                                           torch::Tensor labels,
                                           torch::Tensor mask,
                                           bool multilabel);
torch::Tensor masked_loss_bwd(torch::Tensor logits, torch::Tensor labels,
                              torch::Tensor mask, torch::Tensor stats,
                              torch::Tensor g, bool multilabel);
int64_t masked_loss_max_blocks();
int64_t masked_loss_max_classes();
int64_t masked_loss_rows_per_block(int64_t C);

void fused_dual_gemm_bf16(torch::Tensor a1, torch::Tensor a2,
                          torch::Tensor w1t, torch::Tensor w2t,
                          torch::Tensor bias, torch::Tensor out) {
    CHECK_DEV(a1); CHECK_CONTIG(a1); CHECK_DEV(a2); CHECK_CONTIG(a2);
    CHECK_DEV(w1t); CHECK_CONTIG(w1t); CHECK_DEV(w2t); CHECK_CONTIG(w2t);
    CHECK_DEV(out); CHECK_CONTIG(out);
    TORCH_CHECK(a1.scalar_type() == torch::kBFloat16, "bf16 only");
    const int64_t M = a1.size(0), K1 = a1.size(1), K2 = a2.size(1);
    const int64_t N = out.size(1);
    TORCH_CHECK(a2.size(0) == M && out.size(0) == M, "M mismatch");
    TORCH_CHECK(w1t.size(0) == N && w1t.size(1) == K1, "w1t must be [N,K1]");
    TORCH_CHECK(w2t.size(0) == N && w2t.size(1) == K2, "w2t must be [N,K2]");
    TORCH_CHECK(N % 16 == 0 && N <= 256, "N must be mult of 16, <=256");
    TORCH_CHECK(K1 % 8 == 0 && K2 % 8 == 0, "K must be mult of 8");
    const dim3 block(256), grid((M + 63) / 64);
    fused_dual_gemm_bf16_kernel<<<grid, block, 0, cur_stream()>>>(
        reinterpret_cast<const ushort*>(a1.data_ptr()),
        reinterpret_cast<const ushort*>(a2.data_ptr()),
        reinterpret_cast<const ushort*>(w1t.data_ptr()),
        reinterpret_cast<const ushort*>(w2t.data_ptr()),
        bias.numel() ? reinterpret_cast<const ushort*>(bias.data_ptr()) : nullptr,
        reinterpret_cast<ushort*>(out.data_ptr()), M, N, K1, K2);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("quant_pack", &quant_pack,
          "fused minmax+stochastic-quantize+bitpack (CDNA4)");
    m.def("quant_unpack", &quant_unpack,
          "fused dequantize+scatter (CDNA4)");
    m.def("spmm_csr", &spmm_csr,
          "CSR SpMM with fused degree normalization and an optional "
          "epilogue addend (CDNA4)",
          pybind11::arg("indices"), pybind11::arg("xl"), pybind11::arg("xr"),
          pybind11::arg("y"), pybind11::arg("src_scale"),
          pybind11::arg("dst_scale"), pybind11::arg("seg_row"),
          pybind11::arg("seg_e0"), pybind11::arg("seg_e1"),
          pybind11::arg("seg_part"), pybind11::arg("zero_rows"),
          pybind11::arg("part_ptr"), pybind11::arg("n_part"),
          pybind11::arg("addend"), pybind11::arg("wave_index") = false,
          pybind11::arg("packed") = torch::Tensor(),
          pybind11::arg("packed_depth") = 4);
    m.def("pack_rows", &pack_rows,
          "fixed-stride packed copy of a sparse fp32 [N,F] tensor for the "
          "packed-gather SpMM (CDNA4)");
    m.def("spmm_packable", &spmm_packable);
    m.def("packed_meta_bytes", &packed_meta_bytes);
    m.def("packed_row_stride", &packed_row_stride);
    m.def("packed_buffer_bytes", &packed_buffer_bytes);
    m.def("colsum", &colsum,
          "deterministic column sum of a [N,F] fp32/bf16 matrix, fp32 "
          "accumulate (CDNA4)");
    m.def("fused_dual_gemm_bf16", &fused_dual_gemm_bf16,
          "out = A1@W1 + A2@W2 + bias, one-pass MFMA (CDNA4)");
    m.def("norm_act_fwd", &norm_act_fwd,
          "fused LayerNorm+ReLU+dropout forward (CDNA4)");
    m.def("norm_act_bwd", &norm_act_bwd,
          "fused LayerNorm+ReLU+dropout backward; returns [2,F] "
          "(dweight, dbias) (CDNA4)");
    m.attr("NORM_ACT_BWD_MAX_BLOCKS") = norm_act_bwd_max_blocks();
    m.attr("NORM_ACT_WAVES_PER_BLOCK") = norm_act_waves_per_block();
    m.attr("NORM_ACT_MAX_FEATS") = norm_act_max_feats();
    m.def("masked_loss_fwd", &masked_loss_fwd,
          "masked softmax-CE / BCE-with-logits sum; returns {loss, stats} "
          "(CDNA4)");
    m.def("masked_loss_bwd", &masked_loss_bwd,
          "gradient of masked_loss_fwd with respect to the logits (CDNA4)");
    m.def("masked_loss_rows_per_block", &masked_loss_rows_per_block,
          "rows a block handles per trip of its row loop, for C classes");
    m.attr("MASKED_LOSS_MAX_BLOCKS") = masked_loss_max_blocks();
    m.attr("MASKED_LOSS_MAX_CLASSES") = masked_loss_max_classes();
}
