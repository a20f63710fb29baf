// SpMM that gathers remote columns straight from the quantized wire buffer
// where the gathered rows are bf16 (gfx950 / MI355X): the bf16 engine's
// forward and backward SpMMs (bf16 rows in, bf16 out) and the fp32 engine's
// mixed backward (bf16 rows in, fp32 out and addend).
//
// spmm_quant.hip does this for fp32 rows. Under bf16 the unfused path unpacks
// the wire into a [R, F] bf16 block (one quant_unpack launch per bit width)
// and the SpMM gathers it at 2F bytes per remote edge; here a remote edge
// pulls the F * bits / 8 wire bytes and the block does not exist. The row
// descriptors are the 16-byte {byte offset, bits, inv, rmin} records that
// quant_row_desc_kernel (spmm_quant.hip) writes; nothing else is prepared.
//
// spmm_quant_bf16_kernel<SW, VE, OutT, SS>
//   Work split and arithmetic are spmm_csr_kernel<SW, ushort, VE>'s and
//   spmm_bf16in_kernel's: a lane owns VE in {8, 4, 2} consecutive features
//   (one 16/8/4-byte load of a local row), SW in {16, 32, 64} is the smallest
//   sub-wavefront covering F / VE lanes (F = 256: 32 lanes, two segments per
//   wavefront), segments, fp32 partial slots, the XCD swizzle, the static
//   order, four edges in flight, edge j of a segment into accumulator j & 1 in
//   increasing j with one fmaf(to_f32(v), s, acc) per feature, epilogue
//   (acc0 + acc1) * ds and round_add<OutT>. OutT is ushort (bf16 bits) or
//   float; SS says a src_scale vector is given.
//
//   Window fetch. A lane needs the VE * bits <= 64 bits that start at bit
//   8 * off + f0 * bits of the payload (the fp32 kernel's lanes need 32).
//   Rows start at any byte, and with VE = 2 at 2 bits a lane starts in the
//   middle of a byte, so the lane takes naturally aligned dwords from the
//   4-byte-aligned address at or below the byte that holds its first bit:
//   the first bit then sits at shift = 8 * (byte & 3) + (bit & 7) <= 31 of
//   the window. VE = 8 loads three dwords (shift + 64 <= 95 bits are always
//   inside) and two v_alignbit_b32 give the low and the high 32 bits; level
//   k is a shift and a mask of the low word while k * bits < 32 and of the
//   high word from there on (bits divides 32: no level straddles the two).
//   VE <= 4 needs at most 32 bits: two dwords and one v_alignbit_b32, as in
//   the fp32 kernel. No load is narrower than a dword or misaligned; the
//   dwords are adjacent and the compiler may fetch them with one load. The
//   last dword of the last row's last lane can end up to 11 bytes past the
//   wire length (first byte <= L - 1, aligned down, 12 bytes read): the
//   payload carries QUANT_PAD = 12 spare bytes, checked on the host against
//   the tensor's storage.
//
//   Dequantization. quant_unpack_kernel<BITS, ushort> stores
//   f32_to_bf16((float)q * inv + rmin) with the multiply-add contracted to
//   one fma; the SpMM then widens that bf16. The gather computes
//   fmaf((float)q, inv, rmin), rounds it with the same f32_to_bf16 and widens
//   it, so the fmaf(v, s, acc) chain sees the same operands in the same order
//   and the result equals the dense (OutT = ushort) or mixed (OutT = float)
//   kernel fed the unpacked bf16 block bit for bit. The rounding is VALU work
//   the fp32 kernel does not have; it is what keeps the bits equal.
//
//   Local/remote mix, as in spmm_quant_kernel: one wave-wide ballot per batch
//   of 4/2/1 edges. No remote edge in any lane: the dense batch, row loads
//   only. Otherwise one branch-free block: every edge issues its descriptor
//   load, its dense row load and its window dwords; the loads an edge does
//   not need point at always-valid hot addresses (descriptor 0, row 0 of xl,
//   the payload's first dwords) and a select drops their values. Which batch
//   runs changes neither the order nor the operands of any fmaf.
//
// No LDS and no matrix instructions: a gathered row is used once. Built
// without packed fp32 instructions, as spmm_quant.hip.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>

#include "device_common.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// N elements of T moved as 16-byte pieces, or as one piece when they are fewer
template <typename T, int N>
__device__ __forceinline__ void load_vec(const T* __restrict__ p, T (&v)[N]) {
    constexpr int B = N * sizeof(T) < 16 ? N * sizeof(T) : 16;
    using Raw = typename RawVec<B>::type;
    constexpr int PER = B / sizeof(T);
#pragma unroll
    for (int k = 0; k < N; k += PER)
        *reinterpret_cast<Raw*>(&v[k]) = *reinterpret_cast<const Raw*>(p + k);
}

template <typename T, int N>
__device__ __forceinline__ void store_vec(T* __restrict__ p, const T (&v)[N]) {
    constexpr int B = N * sizeof(T) < 16 ? N * sizeof(T) : 16;
    using Raw = typename RawVec<B>::type;
    constexpr int PER = B / sizeof(T);
#pragma unroll
    for (int k = 0; k < N; k += PER)
        *reinterpret_cast<Raw*>(p + k) = *reinterpret_cast<const Raw*>(&v[k]);
}

template <int SW, int VE, typename OutT, bool SS>
__global__ void __launch_bounds__(256) spmm_quant_bf16_kernel(
    const int32_t* __restrict__ indices,
    const ushort* __restrict__ xl, const uint8_t* __restrict__ payload,
    const uint4* __restrict__ desc, OutT* __restrict__ y,
    const float* __restrict__ src_scale, const float* __restrict__ dst_scale,
    const int32_t* __restrict__ seg_row, const int32_t* __restrict__ seg_e0,
    const int32_t* __restrict__ seg_e1, const int32_t* __restrict__ seg_part,
    float* __restrict__ part, const OutT* __restrict__ addend,
    int64_t n_seg, int64_t F, int64_t n_local) {
    using Raw = typename RawVec<VE * 2>::type;
    // dwords of a lane's window: its VE * bits <= VE * 8 bits at a shift <= 31
    constexpr int NW = VE * 8 > 32 ? 3 : 2;
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
            const uint32_t fb = (uint32_t)f0;      // F * 8 fits 32 bits (host)

            // every batch starts at an even distance from e0, so edge
            // e + u goes to accumulator u & 1
            auto batch = [&](int64_t e, auto nb_tag) {
                constexpr int NB = decltype(nb_tag)::value;
                int64_t c[NB];
                float s[NB];
                Raw dv[NB];
                bool any_remote = false;
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    c[u] = indices[e + u];
                    any_remote |= c[u] >= n_local;
                }
                if (__builtin_amdgcn_ballot_w64(any_remote) == 0) {
                    // the dense bf16 kernel's batch
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        s[u] = SS ? src_scale[c[u]] : 1.f;
                        dv[u] = *reinterpret_cast<const Raw*>(xl + c[u] * F + f0);
                    }
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        const ushort* v = reinterpret_cast<const ushort*>(&dv[u]);
#pragma unroll
                        for (int k = 0; k < VE; ++k) {
                            if (u & 1) acc1[k] = fmaf(bf16_to_f32(v[k]), s[u], acc1[k]);
                            else acc0[k] = fmaf(bf16_to_f32(v[k]), s[u], acc0[k]);
                        }
                    }
                    return;
                }
                uint4 d[NB];
                uint32_t w[NB][NW], sh[NB];
                // a local column reads descriptor 0 and drops it
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    s[u] = SS ? src_scale[c[u]] : 1.f;
                    d[u] = desc[c[u] < n_local ? 0 : c[u] - n_local];
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const bool loc = c[u] < n_local;
                    // a remote column reads row 0 of xl and drops it
                    dv[u] = *reinterpret_cast<const Raw*>(
                        xl + (loc ? c[u] : 0) * F + f0);
                    // a local column reads the payload's first dwords
                    const uint32_t bits = loc ? 0u : d[u].y;
                    const uint32_t sb = fb * bits;
                    const uint64_t byte = (uint64_t)(loc ? 0u : d[u].x) + (sb >> 3);
                    sh[u] = ((uint32_t)(byte & 3u) << 3) | (sb & 7u);
                    const uint32_t* wp = reinterpret_cast<const uint32_t*>(
                        payload + (byte & ~(uint64_t)3));
#pragma unroll
                    for (int i = 0; i < NW; ++i) w[u][i] = wp[i];
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const bool loc = c[u] < n_local;
                    const uint32_t bits = d[u].y;
                    const uint32_t mask = (1u << bits) - 1u;
                    // (a bit cast, not __uint_as_float: the header's helper
                    // lacks this file's target attribute and is not inlined)
                    const float inv = __builtin_bit_cast(float, d[u].z);
                    const float rmin = __builtin_bit_cast(float, d[u].w);
                    // bits [sh, sh + 32) and, for VE = 8, [sh + 32, sh + 64)
                    // of the window
                    const uint32_t lo = __builtin_amdgcn_alignbit(w[u][1], w[u][0], sh[u]);
                    uint32_t hi = 0;
                    if constexpr (NW == 3)
                        hi = __builtin_amdgcn_alignbit(w[u][2], w[u][1], sh[u]);
                    const ushort* dense = reinterpret_cast<const ushort*>(&dv[u]);
#pragma unroll
                    for (int k = 0; k < VE; ++k) {
                        const uint32_t p = k * bits;
                        uint32_t word = lo;
                        // k < 4: k * bits <= 24 whatever the width
                        if constexpr (NW == 3) { if (k >= 4 && p >= 32u) word = hi; }
                        const uint32_t lv = (word >> (p & 31u)) & mask;
                        const ushort dq = f32_to_bf16(fmaf((float)lv, inv, rmin));
                        const float v = bf16_to_f32(loc ? dense[k] : dq);
                        if (u & 1) acc1[k] = fmaf(v, s[u], acc1[k]);
                        else acc0[k] = fmaf(v, s[u], acc0[k]);
                    }
                }
            };
            int64_t e = e0;
            for (; e + 3 < e1; e += 4) batch(e, std::integral_constant<int, 4>{});
            for (; e + 1 < e1; e += 2) batch(e, std::integral_constant<int, 2>{});
            if (e < e1) batch(e, std::integral_constant<int, 1>{});

            if (slot < 0) {
                alignas(16) OutT ad[VE], outv[VE];
                if (addend) load_vec<OutT, VE>(addend + r * F + f0, ad);
#pragma unroll
                for (int k = 0; k < VE; ++k)
                    outv[k] = round_add<OutT>((acc0[k] + acc1[k]) * ds,
                                              addend ? ad + k : nullptr);
                store_vec<OutT, VE>(y + r * F + f0, outv);
            } else {
                // long row split across segments: fp32 partial into this
                // segment's own slot, summed by combine_parts_kernel<OutT>
                alignas(16) float pv[VE];
#pragma unroll
                for (int k = 0; k < VE; ++k)
                    pv[k] = (acc0[k] + acc1[k]) * ds;
                store_vec<float, VE>(part + slot * F + f0, pv);
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
// bytes a three-dword window can reach past the wire length; QUANT_PAD
// (spmm_quant.hip), which QuantRemote.wire_buffer allocates, is no smaller
#define WINDOW_SPARE 12
void spmm_bf16in_shape(int64_t F, int* ve, int* sw);        // spmm_mixed.hip

// called by spmm_csr_quant_bf16 (kernels.hip), which checked the dense
// operands and the view's arrays and allocated the partial slots. y and
// addend are bf16 bits (out_f32 false) or fp32 (true). The wire operands are
// checked here: every window load has to stay inside the payload's storage.
void launch_spmm_quant_bf16(
    hipStream_t s, bool out_f32, const int32_t* indices, const ushort* xl,
    torch::Tensor payload, torch::Tensor desc, void* y, const float* src_scale,
    const float* dst_scale, const int32_t* seg_row, const int32_t* seg_e0,
    const int32_t* seg_e1, const int32_t* seg_part, float* part,
    const void* addend, int64_t n_seg, int64_t F, int64_t n_local) {
    TORCH_CHECK(payload.is_cuda() && payload.is_contiguous() &&
                payload.scalar_type() == torch::kUInt8,
                "quantized bf16 spmm expects a contiguous uint8 GPU payload");
    const int64_t spare = (int64_t)payload.storage().nbytes()
                          - (payload.storage_offset() + payload.numel());
    TORCH_CHECK(reinterpret_cast<uintptr_t>(payload.data_ptr()) % 4 == 0 &&
                spare >= WINDOW_SPARE,
                "quantized bf16 spmm: the payload must start 4-byte aligned "
                "and have 12 spare bytes behind it in its storage");
    TORCH_CHECK(desc.is_cuda() && desc.is_contiguous() && desc.dim() == 2 &&
                desc.size(1) == 4 && desc.size(0) > 0 &&
                desc.scalar_type() == torch::kInt32,
                "quantized bf16 spmm expects quant_row_desc's int32 [R, 4] block");
    int ve, sw;
    spmm_bf16in_shape(F, &ve, &sw);
    TORCH_CHECK(n_local > 0 && F > 0 && F % ve == 0 && F < (1ll << 28),
                "quantized bf16 spmm needs at least one local row and an "
                "even F < 2^28");
    const int block_threads = 256;
    const int rows_per_block = block_threads / sw;
    int64_t blocks = (n_seg + rows_per_block - 1) / rows_per_block;
    blocks = std::max<int64_t>(std::min<int64_t>(blocks, 16384), 1);
    const dim3 grid(blocks), block(block_threads);
    const uint8_t* pl = payload.data_ptr<uint8_t>();
    const uint4* dp = reinterpret_cast<const uint4*>(desc.data_ptr<int32_t>());
#define LAUNCH(SWC, VEC, T, SSC) spmm_quant_bf16_kernel<SWC, VEC, T, SSC><<<grid, block, 0, s>>>( \
        indices, xl, pl, dp, reinterpret_cast<T*>(y), src_scale, dst_scale, \
        seg_row, seg_e0, seg_e1, seg_part, part, \
        reinterpret_cast<const T*>(addend), n_seg, F, n_local)
#define BY_SS(SWC, VEC, T) do { \
        if (src_scale) LAUNCH(SWC, VEC, T, true); else LAUNCH(SWC, VEC, T, false); \
    } while (0)
#define BY_OUT(SWC, VEC) do { \
        if (out_f32) BY_SS(SWC, VEC, float); else BY_SS(SWC, VEC, ushort); \
    } while (0)
#define BY_VE(SWC) do { \
        switch (ve) { \
            case 8: BY_OUT(SWC, 8); break; \
            case 4: BY_OUT(SWC, 4); break; \
            default: BY_OUT(SWC, 2); break; \
        } \
    } while (0)
    switch (sw) {
        case 64: BY_VE(64); break;
        case 32: BY_VE(32); break;
        default: BY_VE(16); break;
    }
#undef BY_VE
#undef BY_OUT
#undef BY_SS
#undef LAUNCH
}
