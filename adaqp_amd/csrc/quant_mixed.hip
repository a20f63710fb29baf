// One-launch mixed-bit quantizer with an in-kernel variance trace
// (gfx950 / MI355X, fp32 and bf16 rows).
//
// quant_pack_kernel<BITS, T> (kernels.hip) is launched once per bit width in
// use, gives every node a whole 64-lane wavefront whatever F is, reads the row
// with 4-byte loads strided by 8 / bits, stores one byte per lane and takes
// three int64 loads per node from three arrays. quant_pack_mixed_kernel packs
// a whole send set, every bit width, in ONE launch and writes the same bytes.
//
// quant_pack_mixed_kernel<SW, T, TRACE>   T = float or ushort (bf16 bits).
//
//   work split   A lane owns 4 consecutive features: one 16-byte load (fp32)
//     or one 8-byte load (bf16). SW is the smallest of 16/32/64 lanes covering
//     F / 4, and a sub-wavefront of SW lanes serves one send slot: four slots
//     per wavefront for F <= 64, two for F <= 128, one above. For F > 256
//     (SW == 64) a lane stages up to 4 chunks of 4 features, 256 features
//     apart, in registers, so a row of up to 1024 features is read once; the
//     chunk loops are fully unrolled, every register index is a constant and
//     nothing goes to scratch.
//   descriptor   One 16-byte load of send_tab[s] = {source row, wire byte
//     offset (u32 bits), params slot = RNG tag, bits}, same address in every
//     lane of the sub-wavefront.
//   reduction    min/max by width-SW xor shuffles (v_min_f32/v_max_f32 order
//     -0 below +0, so the reduction order does not show in the result), then
//     scale, rmin and their bf16 roundings by quant_pack_kernel's own
//     expressions: quantize with the wire scale, scale = 0 for a constant
//     row. Lane 0 writes the two params.
//   bit width    bits is uniform over a sub-wavefront. One branch per row
//     enters a body specialised for 2, 4 or 8 bits: a lane's 4 levels are then
//     W = 1, 2 or 4 bytes of the row.
//   store rule   A chunk's bytes (all of the row for F <= 256) form a segment
//     that starts at wire address B, any byte (26-byte rows at F = 104 and 2
//     bits). Every lane fetches the words of its next 1 (8 bits), 2 (4 bits)
//     or 3 (2 bits) neighbours by shuffle and so holds the 4..8 segment bytes
//     from its own first byte on. The lane that owns the segment byte at a
//     4-byte-aligned ADDRESS stores the naturally aligned dword starting
//     there, if all 4 bytes lie inside the segment. The up to 3 bytes before
//     the first such dword and the up to 3 after the last one are stored as
//     single bytes by the lanes that own them. So every byte of the row's
//     F * bits / 8 is written exactly once, by one lane, and no store crosses
//     the row's end. (The segments of a multi-chunk row start 64 * W bytes
//     apart, at the same alignment; each has its own head and tail bytes.)
//   same bits    The level of feature f is
//         clamp((int)floorf(fmaf(v - rmin, scale, uniform01(seed, tag, f))))
//     under the same `scale > 0` guard. quant_pack_kernel writes
//     `(v - rmin) * scale` and `+ u`; in its gfx950 ISA that is v_sub_f32
//     followed by ONE v_fmac_f32 (the multiply and the add are contracted, in
//     all six instantiations, staged path), so the FMA FORM is written out
//     here: a subtraction with its own rounding, then fmaf.
//   TRACE        trace[s] += c * (rng * rng), c = (float)(F / 6.0), rng =
//     rmax - rmin, rounded to bf16 first when T is bf16: GraphEngine.trace's
//     value bit for bit (it subtracts in the send dtype, squares and scales in
//     fp32 with a rounding each). One slot has one writer, so lane 0 does a
//     plain load, add, store: no atomics, the same result on every run.
//
// No LDS and no matrix instructions: a row is read once, by one
// sub-wavefront, and quantizing is elementwise after the min/max, so there is
// no reuse for either to exploit. Data goes global memory -> registers ->
// global memory; the only cross-lane traffic is the shuffles of the reduction
// and of the store rule.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>

#include "device_common.h"

#define QM_THREADS 256
#define QM_MAX_FEATS 1024

// 4 consecutive features of a row as fp32
template <typename T>
__device__ __forceinline__ void load4(const T* p, float (&v)[4]);
template <>
__device__ __forceinline__ void load4<float>(const float* p, float (&v)[4]) {
    const float4 r = *reinterpret_cast<const float4*>(p);
    v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
}
template <>
__device__ __forceinline__ void load4<ushort>(const ushort* p, float (&v)[4]) {
    const uint2 r = *reinterpret_cast<const uint2*>(p);
    v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xFFFF0000u);
    v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xFFFF0000u);
}

// the 4 levels of features [f0, f0 + 4), level k at bit k * BITS
template <int BITS>
__device__ __forceinline__ uint32_t quant4(const float (&v)[4], float rmin,
                                           float scale, uint32_t seed,
                                           uint32_t tag, uint32_t f0) {
    uint32_t word = 0;
    if (scale > 0.f) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = v[k] - rmin;
            const float w = fmaf(d, scale, uniform01(seed, tag, f0 + k));
            int q = (int)floorf(w);
            q = max(0, min(q, (1 << BITS) - 1));
            word |= ((uint32_t)q) << (k * BITS);
        }
    }
    return word;
}

// acc + c * (rng * rng) with a rounding after each of the three operations,
// as the three torch kernels of GraphEngine.trace leave them: nothing is
// contracted into an fma.
__device__ __forceinline__ float trace_add(float acc, float c, float rng) {
#pragma clang fp contract(off)
    const float sq = rng * rng;
    const float v = c * sq;
    return acc + v;
}

// Store one segment: lane sl holds segment bytes [sl * W, sl * W + W) in the
// low W bytes of `word` (0 in a lane past the segment's nbs bytes). Every lane
// of the sub-wavefront calls it.
template <int BITS, int SW>
__device__ __forceinline__ void store_segment(uint8_t* __restrict__ seg,
                                              uint32_t word, int sl, int nbs) {
    constexpr int W = BITS / 2;
    // the 4..8 segment bytes from this lane's first byte on
    uint64_t win = word;
    if constexpr (W == 4) {
        win |= (uint64_t)(uint32_t)__shfl_down((int)word, 1, SW) << 32;
    } else if constexpr (W == 2) {
        win |= (uint64_t)(uint32_t)__shfl_down((int)word, 1, SW) << 16;
        win |= (uint64_t)(uint32_t)__shfl_down((int)word, 2, SW) << 32;
    } else {
        win |= (uint64_t)(uint32_t)__shfl_down((int)word, 1, SW) << 8;
        win |= (uint64_t)(uint32_t)__shfl_down((int)word, 2, SW) << 16;
        win |= (uint64_t)(uint32_t)__shfl_down((int)word, 3, SW) << 24;
    }
    const uint32_t a = (uint32_t)reinterpret_cast<uintptr_t>(seg) & 3u;
    const int jb = sl * W;                          // my first segment byte
    // r: distance from jb to the next byte at a 4-byte-aligned address
    const int r = (int)((0u - ((uint32_t)jb + a)) & 3u);
    if (r < W && jb + r + 4 <= nbs)
        *reinterpret_cast<uint32_t*>(seg + jb + r) = (uint32_t)(win >> (8 * r));
    // head [0, h) and tail [t, nbs): the bytes no aligned dword covers
    const int h = min((int)((4u - a) & 3u), nbs);
    const int t = h + ((nbs - h) & ~3);
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const int j = jb + i;
        if (j < nbs && (j < h || j >= t)) seg[j] = (uint8_t)(word >> (8 * i));
    }
}

template <int BITS, int SW, int NCH>
__device__ __forceinline__ void pack_row(const float (&v)[NCH][4], float rmin,
                                         float scale, uint32_t seed,
                                         uint32_t tag, int F, int sl,
                                         uint8_t* __restrict__ out) {
    constexpr int W = BITS / 2;
    const int groups = F / 4;                       // lanes' worth of features
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c * SW >= groups) break;                // uniform over the row
        const int g = c * SW + sl;
        const uint32_t word = g < groups
            ? quant4<BITS>(v[c], rmin, scale, seed, tag, (uint32_t)g * 4u) : 0u;
        store_segment<BITS, SW>(out + c * SW * W, word, sl,
                                min(SW, groups - c * SW) * W);
    }
}

template <int SW, typename T, bool TRACE>
__global__ void __launch_bounds__(QM_THREADS) quant_pack_mixed_kernel(
    const T* __restrict__ x, const int4* __restrict__ tab, int64_t S, int F,
    uint32_t seed, uint8_t* __restrict__ payload,
    uint16_t* __restrict__ params, float* __restrict__ trace, float c_trace) {
    constexpr int NCH = SW == 64 ? QM_MAX_FEATS / (4 * 64) : 1;
    const int64_t s = (int64_t)blockIdx.x * (QM_THREADS / SW) + threadIdx.x / SW;
    if (s >= S) return;                             // whole sub-wavefronts
    const int sl = threadIdx.x & (SW - 1);
    const int4 d = tab[s];              // {row, wire offset, slot, bits}
    const T* xr = x + (int64_t)d.x * F;

    float v[NCH][4];
    float mn = 1e38f, mx = -1e38f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int f0 = (c * SW + sl) * 4;
        if (f0 < F) {                               // F % 4 == 0: all 4 inside
            load4<T>(xr + f0, v[c]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                mn = fminf(mn, v[c][k]);
                mx = fmaxf(mx, v[c][k]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[c][k] = 0.f;
        }
    }
#pragma unroll
    for (int o = SW / 2; o; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, SW));
        mx = fmaxf(mx, __shfl_xor(mx, o, SW));
    }
    const int bits = d.w;
    const float rng = mx - mn;
    const float scale_f = rng > 0.f
        ? ((float)((1 << bits) - 1)) / fmaxf(rng, 1e-30f) : 0.f;
    const uint16_t scale_h = f32_to_bf16(scale_f);
    const uint16_t rmin_h = f32_to_bf16(mn);
    const float scale = bf16_to_f32(scale_h);       // quantize with the wire scale
    const float rmin = bf16_to_f32(rmin_h);
    if (sl == 0) {
        params[2 * (int64_t)d.z] = scale_h;
        params[2 * (int64_t)d.z + 1] = rmin_h;
        if constexpr (TRACE) {
            const float rt = sizeof(T) == 2 ? bf16_to_f32(f32_to_bf16(rng)) : rng;
            trace[s] = trace_add(trace[s], c_trace, rt);
        }
    }
    const uint32_t tag = (uint32_t)d.z;
    uint8_t* out = payload + (uint64_t)(uint32_t)d.y;
    if (bits == 2)
        pack_row<2, SW, NCH>(v, rmin, scale, seed, tag, F, sl, out);
    else if (bits == 4)
        pack_row<4, SW, NCH>(v, rmin, scale, seed, tag, F, sl, out);
    else if (bits == 8)
        pack_row<8, SW, NCH>(v, rmin, scale, seed, tag, F, sl, out);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
bool quant_mixed_ok(int64_t F) {
    return F > 0 && F % 4 == 0 && F <= QM_MAX_FEATS;
}

template <int SW, typename T>
static void launch_qm(hipStream_t st, const torch::Tensor& x,
                      const torch::Tensor& tab, int64_t seed,
                      torch::Tensor& payload, torch::Tensor& params,
                      float* trace) {
    const int64_t S = tab.size(0);
    const int F = (int)x.size(1);
    const dim3 block(QM_THREADS);
    const dim3 grid((unsigned)((S + QM_THREADS / SW - 1) / (QM_THREADS / SW)));
    const T* xp = reinterpret_cast<const T*>(x.data_ptr());
    const int4* tp = reinterpret_cast<const int4*>(tab.data_ptr<int32_t>());
    uint8_t* pp = payload.data_ptr<uint8_t>();
    uint16_t* qp = reinterpret_cast<uint16_t*>(params.data_ptr<at::BFloat16>());
    const float c = (float)((double)F / 6.0);
    if (trace)
        quant_pack_mixed_kernel<SW, T, true><<<grid, block, 0, st>>>(
            xp, tp, S, F, (uint32_t)seed, pp, qp, trace, c);
    else
        quant_pack_mixed_kernel<SW, T, false><<<grid, block, 0, st>>>(
            xp, tp, S, F, (uint32_t)seed, pp, qp, nullptr, c);
}

// x [N, F] contiguous fp32/bf16; send_tab int32 [S, 4] (SidePlan.send_tab);
// payload uint8 and params bf16 as mixed_quantize allocates them; trace fp32
// [S], or a 0-element tensor for none. The table's contents are the caller's
// (ops/kernels.py checks the plan against x, payload and params).
void quant_pack_mixed(torch::Tensor x, torch::Tensor send_tab, int64_t seed,
                      torch::Tensor payload, torch::Tensor params,
                      torch::Tensor trace) {
    TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous(),
                "x must be a contiguous [N, F] GPU tensor");
    const bool bf16 = x.scalar_type() == torch::kBFloat16;
    TORCH_CHECK(bf16 || x.scalar_type() == torch::kFloat32,
                "quant_pack_mixed expects fp32 or bf16");
    const int64_t F = x.size(1);
    TORCH_CHECK(quant_mixed_ok(F), "quant_pack_mixed needs F % 4 == 0 and "
                "F <= 1024");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % (bf16 ? 8 : 16) == 0,
                "x must be aligned to the 4-feature load");
    TORCH_CHECK(send_tab.is_cuda() && send_tab.is_contiguous() &&
                send_tab.scalar_type() == torch::kInt32 &&
                send_tab.dim() == 2 && send_tab.size(1) == 4,
                "send_tab must be a contiguous int32 [S, 4] GPU tensor");
    TORCH_CHECK(payload.is_cuda() && payload.is_contiguous() &&
                payload.scalar_type() == torch::kUInt8,
                "payload must be a contiguous uint8 GPU tensor");
    TORCH_CHECK(params.is_cuda() && params.is_contiguous() &&
                params.scalar_type() == torch::kBFloat16 &&
                params.numel() == 2 * send_tab.size(0),
                "params must be bf16 [2 S] on the GPU");
    float* tr = nullptr;
    if (trace.numel()) {
        TORCH_CHECK(trace.is_cuda() && trace.is_contiguous() &&
                    trace.scalar_type() == torch::kFloat32 &&
                    trace.numel() == send_tab.size(0),
                    "trace must be fp32 [S] on the GPU");
        tr = trace.data_ptr<float>();
    }
    if (send_tab.size(0) == 0) return;
    auto st = at::cuda::getCurrentHIPStream().stream();
    const int sw = F <= 64 ? 16 : (F <= 128 ? 32 : 64);
#define QM_LAUNCH(SWV)                                                        \
    do {                                                                      \
        if (bf16) launch_qm<SWV, ushort>(st, x, send_tab, seed, payload,      \
                                         params, tr);                         \
        else launch_qm<SWV, float>(st, x, send_tab, seed, payload, params,    \
                                   tr);                                       \
    } while (0)
    if (sw == 16) QM_LAUNCH(16);
    else if (sw == 32) QM_LAUNCH(32);
    else QM_LAUNCH(64);
#undef QM_LAUNCH
}
