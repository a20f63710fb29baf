// SpMM that gathers remote columns straight from the quantized wire buffer
// (gfx950 / MI355X, fp32).
//
// After the boundary all-to-all the remote block exists as the wire payload:
// per remote row ceil(F * bits / 8) bytes of bits-wide levels (bits in
// {2, 4, 8}, feature k at bit k * bits of the row, little endian) plus a bf16
// (scale, rmin) pair. quant_unpack expands that into a [R, F] fp32 block which
// the SpMM then gathers at 4F bytes per edge. Here the expansion is done in
// the gather instead: a remote edge pulls F * bits / 8 bytes, and the
// [R, F] block and the unpack launches do not exist.
//
// Two kernels:
//
// quant_row_desc_kernel   one thread per remote-block row. From the plan's
//   static table {wire byte offset, params slot, bits, 0} and this
//   exchange's params it writes the 16-byte descriptor
//       {u32 byte offset into the payload, u32 bits, f32 inv, f32 rmin}
//   with inv = scale > 0 ? 1 / scale : 0 and rmin = bf16_to_f32(...), the
//   same fp32 expressions as quant_unpack_kernel. A row the plan does not
//   cover has bits = 0 in the table and gets the all-zero descriptor: it
//   gathers as +0.0f.
//
// spmm_quant_kernel   spmm_csr_kernel<SW, float, VE> with the fetch of a
//   remote column changed; segments, partial slots, the XCD swizzle, the
//   accumulation rule (edge j of a segment into accumulator j & 1 in
//   increasing j, one fmaf(v, s, acc) per feature), the epilogue
//   (acc0 + acc1) * ds and round_add are the same, so the result equals the
//   dense kernel fed the unpacked block bit for bit.
//
//   Fetch of a remote column: the sub-wavefront reads the row's descriptor
//   (one 16-byte load, same address in every lane). The lane that owns
//   features [f0, f0 + VE) needs the VE * bits <= 32 bits that start at bit
//   8 * off + f0 * bits of the payload. Rows start at any byte, so it takes
//   the two naturally aligned dwords at the 4-byte-aligned address at or
//   below the byte that holds its first bit: the first bit then sits at
//   shift = 8 * (byte & 3) + (bit & 7) <= 31 of that 64-bit window, and
//   shift + 32 <= 63 bits are always inside it. (The two dwords are adjacent,
//   and the compiler fetches them with one global_load_dwordx2 at that
//   dword-aligned address, the alignment the instruction asks for.) One
//   v_alignbit_b32 moves the lane's bits to bit 0; level k is a shift and a
//   mask. The second dword of
//   the last row's last lane can lie up to 8 bytes past the wire length: the
//   payload is allocated with QUANT_PAD spare bytes (checked on the host
//   against the tensor's storage) and the collective is handed a view of the
//   exact wire length.
//   Level q dequantizes to fmaf((float)q, inv, rmin): quant_unpack_kernel's
//   `(float)q * inv + rmin` is contracted to v_fma_f32 / v_pk_fma_f32 in its
//   compiled ISA, so the fma is written out here.
//
//   Local/remote mix: CSR rows are not sorted local-first, so a batch of four
//   edges can hold both kinds. Each batch first asks, with one wave-wide
//   ballot, whether any of its edges in any lane of the wavefront is remote.
//   If none is (every batch of a local-only stretch), it runs the dense
//   kernel's batch: four row loads, nothing else. Otherwise it runs the mixed
//   batch, which has no branch: every edge issues its descriptor load, its
//   dense row load and its two window dwords, and the loads an edge does not
//   need are pointed at addresses that are always valid and hot (descriptor
//   0, row 0 of xl, the first 8 payload bytes) and their values dropped by a
//   select. So a mixed batch is one basic block with all four edges'
//   descriptor loads in flight together, then all four edges' row and window
//   loads, as the packed kernel does for its word/window pair. The branch is
//   wave-uniform (the ballot is a scalar), so it costs no divergence; which
//   batch runs changes neither the order nor the operands of any fmaf.
//
// The kernels in this file are built without packed fp32 instructions
// (v_pk_fma_f32 and kin): the four fmafs of a lane are scalar v_fma_f32.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>

#include "device_common.h"

// spare bytes behind the wire payload: this kernel's second dword reaches up
// to 8 bytes past the wire length, spmm_quant_bf16.hip's third one up to 12
#define QUANT_PAD 12

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// ---------------------------------------------------------------------------
// descriptors
// ---------------------------------------------------------------------------
__global__ void quant_row_desc_kernel(const int4* __restrict__ tab,
                                      const uint16_t* __restrict__ params,
                                      uint4* __restrict__ desc, int64_t R) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int4 t = tab[r];                  // {offset, params slot, bits, 0}
    float inv = 0.f, rmin = 0.f;
    if (t.z) {
        const float scale = bf16_to_f32(params[2 * (int64_t)t.y]);
        rmin = bf16_to_f32(params[2 * (int64_t)t.y + 1]);
        inv = scale > 0.f ? 1.f / scale : 0.f;
    }
    desc[r] = make_uint4((uint32_t)t.x, (uint32_t)t.z, __float_as_uint(inv),
                         __float_as_uint(rmin));
}

// ---------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------
template <int SW, int VE, bool SS>
__global__ void __launch_bounds__(WAVE * 4) spmm_quant_kernel(
    const int32_t* __restrict__ indices,
    const float* __restrict__ xl, const uint8_t* __restrict__ payload,
    const uint4* __restrict__ desc, float* __restrict__ y,
    const float* __restrict__ src_scale, const float* __restrict__ dst_scale,
    const int32_t* __restrict__ seg_row, const int32_t* __restrict__ seg_e0,
    const int32_t* __restrict__ seg_e1, const int32_t* __restrict__ seg_part,
    float* __restrict__ part, const float* __restrict__ addend,
    int64_t n_seg, int64_t F, int64_t n_local) {
    using Raw = typename RawVec<VE * 4>::type;
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
                    // the dense kernel's batch
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        s[u] = SS ? src_scale[c[u]] : 1.f;
                        dv[u] = *reinterpret_cast<const Raw*>(xl + c[u] * F + f0);
                    }
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        const float* v = reinterpret_cast<const float*>(&dv[u]);
#pragma unroll
                        for (int k = 0; k < VE; ++k) {
                            if (u & 1) acc1[k] = fmaf(v[k], s[u], acc1[k]);
                            else acc0[k] = fmaf(v[k], s[u], acc0[k]);
                        }
                    }
                    return;
                }
                uint4 d[NB];
                uint32_t w0[NB], w1[NB], sh[NB];
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
                    // a local column reads the payload's first two dwords
                    const uint32_t bits = loc ? 0u : d[u].y;
                    const uint32_t sb = fb * bits;
                    const uint64_t byte = (uint64_t)(loc ? 0u : d[u].x) + (sb >> 3);
                    sh[u] = ((uint32_t)(byte & 3u) << 3) | (sb & 7u);
                    const uint32_t* wp = reinterpret_cast<const uint32_t*>(
                        payload + (byte & ~(uint64_t)3));
                    w0[u] = wp[0];
                    w1[u] = wp[1];
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const bool loc = c[u] < n_local;
                    const uint32_t bits = d[u].y;
                    const uint32_t mask = (1u << bits) - 1u;
                    const float inv = __uint_as_float(d[u].z);
                    const float rmin = __uint_as_float(d[u].w);
                    // bits [sh, sh + 32) of the 64-bit window w1:w0
                    const uint32_t win = __builtin_amdgcn_alignbit(w1[u], w0[u], sh[u]);
                    const float* dense = reinterpret_cast<const float*>(&dv[u]);
#pragma unroll
                    for (int k = 0; k < VE; ++k) {
                        const uint32_t lv = (win >> (k * bits)) & mask;
                        const float dq = fmaf((float)lv, inv, rmin);
                        const float v = loc ? dense[k] : dq;
                        if (u & 1) acc1[k] = fmaf(v, s[u], acc1[k]);
                        else acc0[k] = fmaf(v, s[u], acc0[k]);
                    }
                }
            };
            int64_t e = e0;
            for (; e + 3 < e1; e += 4) batch(e, std::integral_constant<int, 4>{});
            for (; e + 1 < e1; e += 2) batch(e, std::integral_constant<int, 2>{});
            if (e < e1) batch(e, std::integral_constant<int, 1>{});

            float* yr = y + r * F + f0;
            if (slot < 0) {
                Raw av = {};
                if (addend)
                    av = *reinterpret_cast<const Raw*>(addend + r * F + f0);
                const float* ad = reinterpret_cast<const float*>(&av);
                float outv[VE];
#pragma unroll
                for (int k = 0; k < VE; ++k)
                    outv[k] = round_add<float>((acc0[k] + acc1[k]) * ds,
                                               addend ? ad + k : nullptr);
                *reinterpret_cast<Raw*>(yr) = *reinterpret_cast<const Raw*>(outv);
            } else {
                float* pp = part + slot * F + f0;
#pragma unroll
                for (int k = 0; k < VE; ++k)
                    pp[k] = (acc0[k] + acc1[k]) * ds;
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
int64_t quant_pad_bytes() { return QUANT_PAD; }

// bytes of the tensor's storage behind its last element
static inline int64_t spare_bytes(const torch::Tensor& t) {
    return (int64_t)t.storage().nbytes()
           - (t.storage_offset() + t.numel()) * (int64_t)t.element_size();
}

// tab: int32 [R, 4] rows {wire byte offset (u32 bits), params slot, bits, 0}
// (SidePlan.row_tab); params: this exchange's bf16 [2 * nodes]. Returns the
// int32 [R, 4] descriptor block the gather reads.
torch::Tensor quant_row_desc(torch::Tensor tab, torch::Tensor params) {
    TORCH_CHECK(tab.is_cuda() && tab.is_contiguous() && tab.dim() == 2 &&
                tab.size(1) == 4 && tab.scalar_type() == torch::kInt32,
                "quant_row_desc expects the plan's int32 [R, 4] GPU table");
    TORCH_CHECK(params.is_cuda() && params.is_contiguous() &&
                params.scalar_type() == torch::kBFloat16,
                "quant_row_desc expects contiguous bf16 GPU params");
    const int64_t R = tab.size(0);
    torch::Tensor desc = torch::empty({R, 4}, tab.options());
    if (R == 0) return desc;
    const dim3 block(256), grid((R + 255) / 256);
    quant_row_desc_kernel<<<grid, block, 0,
                            at::cuda::getCurrentHIPStream().stream()>>>(
        reinterpret_cast<const int4*>(tab.data_ptr<int32_t>()),
        reinterpret_cast<const uint16_t*>(params.data_ptr<at::BFloat16>()),
        reinterpret_cast<uint4*>(desc.data_ptr<int32_t>()), R);
    return desc;
}

// called by spmm_csr (kernels.hip) with the grid, vector width and
// sub-wavefront width it computed for the dense kernel
void launch_spmm_quant(
    dim3 grid, dim3 block, hipStream_t s, int sw, int ve,
    const int32_t* indices, const float* xl, torch::Tensor payload,
    torch::Tensor desc, float* y, const float* src_scale,
    const float* dst_scale, const int32_t* seg_row, const int32_t* seg_e0,
    const int32_t* seg_e1, const int32_t* seg_part, float* part,
    const float* addend, int64_t n_seg, int64_t F, int64_t n_local) {
    TORCH_CHECK(payload.is_cuda() && payload.is_contiguous() &&
                payload.scalar_type() == torch::kUInt8,
                "quantized spmm expects a contiguous uint8 GPU payload");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(payload.data_ptr()) % 4 == 0 &&
                spare_bytes(payload) >= QUANT_PAD,
                "quantized spmm: the payload must start 4-byte aligned and "
                "have QUANT_PAD spare bytes behind it in its storage");
    TORCH_CHECK(desc.is_cuda() && desc.is_contiguous() && desc.dim() == 2 &&
                desc.size(1) == 4 && desc.size(0) > 0 &&
                desc.scalar_type() == torch::kInt32,
                "quantized spmm expects quant_row_desc's int32 [R, 4] block");
    TORCH_CHECK(n_local > 0 && F < (1ll << 28),
                "quantized spmm needs at least one local row and F < 2^28");
    const uint8_t* pl = payload.data_ptr<uint8_t>();
    const uint4* dp = reinterpret_cast<const uint4*>(desc.data_ptr<int32_t>());
#define LAUNCH(SWC, VEC, SSC) spmm_quant_kernel<SWC, VEC, SSC><<<grid, block, 0, s>>>( \
        indices, xl, pl, dp, y, src_scale, dst_scale, seg_row, seg_e0, \
        seg_e1, seg_part, part, addend, n_seg, F, n_local)
#define BY_SS(SWC, VEC) do { \
        if (src_scale) LAUNCH(SWC, VEC, true); else LAUNCH(SWC, VEC, false); \
    } while (0)
#define BY_VE(SWC) do { \
        switch (ve) { \
            case 4: BY_SS(SWC, 4); break; \
            case 2: BY_SS(SWC, 2); break; \
            default: BY_SS(SWC, 1); break; \
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
