// Row-skipping fp32 SpMM (gfx950 / MI355X): the dense gather of
// spmm_csr_kernel, minus the rows that are known to be all zero.
//
// The backward SpMM of the OUTPUT layer gathers gh = g @ W_neigh^T, where g
// is the gradient of a masked loss: every row of a node outside the train
// mask is exactly zero, in g and therefore in gh. The dense kernel still
// pulls 4F bytes for every edge that names such a row and multiplies zeros.
// Here one pass marks the rows that hold anything (row_live) and the SpMM
// consults that mark before it fetches a local row.
//
// Two kernels:
//
// row_live_kernel<SW, VE>   contiguous fp32 [N, F] -> uint8 [N]; 1 iff some
//   element has a non-zero magnitude, tested on the bit pattern
//   ((bits & 0x7fffffff) != 0): denormals, NaN and Inf are live whatever the
//   denormal mode, -0.0 is zero. A sub-wavefront of SW lanes owns RL_ROWS
//   consecutive rows; a lane reads VE consecutive words per row with one
//   16/8/4-byte load (VE | F keeps them aligned), all RL_ROWS loads are
//   issued before the first use, and one ballot per row folds the lanes.
//   Rows past the end are clamped to the last row (loaded, not stored), so
//   there is no branch around the loads. One byte per row: the SpMM reads a
//   flag with a plain byte load and no shift.
//
// spmm_rowskip_kernel<SW, VE, SS>   spmm_csr_kernel<SW, float, VE>'s work
//   split and arithmetic: segments, partial slots, the XCD swizzle, four
//   edges in flight, edge j of a segment into accumulator j & 1 in
//   increasing j, one fmaf per edge and feature, accumulators from +0.f,
//   epilogue (acc0 + acc1) * ds and round_add<float>. The only difference:
//   for an edge whose column is local and not live, neither the row nor its
//   src_scale entry is loaded; the fmaf runs on (+0.f, 1.f), which leaves the
//   accumulator as it is. Remote columns are always fetched. The dense kernel
//   would have computed fmaf(+-0, s, acc) with a finite s, which returns acc
//   as well (acc starts at +0 and a sum only becomes -0 from two -0 terms),
//   so the result equals spmm_csr's bit for bit. The one exception is an
//   accumulator that an underflowing product already turned into -0.f
//   meeting a dead row of -0.0 values: dense keeps -0.f, this kernel stores
//   +0.f.
//   A flag is read as live[min(c, n_local - 1)] so the lookup itself needs no
//   branch; the four flags of a batch are loaded together, then the four
//   predicated row loads are issued back to back before the first fmaf.
//   SS (a src_scale vector is given) is a template flag, as in
//   spmm_bf16in_kernel.
//
// Built without packed fp32 instructions (v_pk_fma_f32 and kin), as
// spmm_quant.hip and spmm_mixed.hip: a lane's fmafs are scalar v_fma_f32.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>

#include "device_common.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// ---------------------------------------------------------------------------
// liveness pass
// ---------------------------------------------------------------------------
#define RL_THREADS 256
#define RL_ROWS 4          // rows per sub-wavefront, loads in flight per lane

template <int SW, int VE>
__global__ void __launch_bounds__(RL_THREADS) row_live_kernel(
    const uint32_t* __restrict__ x, uint8_t* __restrict__ live,
    int64_t rows, int64_t F) {
    using Raw = typename RawVec<VE * 4>::type;
    constexpr int groups = RL_THREADS / SW;
    const int64_t grp = (int64_t)blockIdx.x * groups + threadIdx.x / SW;
    const int sl = threadIdx.x & (SW - 1);
    const int64_t r0 = grp * RL_ROWS;
    uint32_t any[RL_ROWS];
    const uint32_t* base[RL_ROWS];
#pragma unroll
    for (int u = 0; u < RL_ROWS; ++u) {
        any[u] = 0u;
        const int64_t r = r0 + u < rows ? r0 + u : rows - 1;   // rows > 0
        base[u] = x + r * F;
    }
    for (int64_t f0 = (int64_t)sl * VE; f0 < F; f0 += (int64_t)SW * VE) {
        Raw v[RL_ROWS];
#pragma unroll
        for (int u = 0; u < RL_ROWS; ++u)
            v[u] = *reinterpret_cast<const Raw*>(base[u] + f0);
#pragma unroll
        for (int u = 0; u < RL_ROWS; ++u) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(&v[u]);
#pragma unroll
            for (int k = 0; k < VE; ++k) any[u] |= w[k] & 0x7FFFFFFFu;
        }
    }
    // every lane of the wavefront gets here: fold each row's lanes
    const int shift = ((threadIdx.x & (WAVE - 1)) / SW) * SW;
    constexpr uint64_t mask = SW == 64 ? ~0ull : ((1ull << (SW & 63)) - 1ull);
#pragma unroll
    for (int u = 0; u < RL_ROWS; ++u) {
        const uint64_t b = __ballot(any[u] != 0u);
        if (sl == 0 && r0 + u < rows)
            live[r0 + u] = ((b >> shift) & mask) != 0ull ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------
template <int SW, int VE, bool SS, bool ORD>
__global__ void __launch_bounds__(256) spmm_rowskip_kernel(
    const int32_t* __restrict__ indices,
    const float* __restrict__ xl, const float* __restrict__ xr,
    const uint8_t* __restrict__ live,
    float* __restrict__ y,
    const float* __restrict__ src_scale, const float* __restrict__ dst_scale,
    const int32_t* __restrict__ seg_row, const int32_t* __restrict__ seg_e0,
    const int32_t* __restrict__ seg_e1, const int32_t* __restrict__ seg_part,
    float* __restrict__ part, const float* __restrict__ addend,
    int64_t n_seg, int64_t F, int64_t n_local,
    int chunk, int32_t* __restrict__ ticket) {
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
    const int64_t last_local = n_local - 1;              // n_local > 0
    // !ORD: one pass of the static grid-stride loop; ORD: the ordered
    // sweep, as spmm_csr_kernel (next_chunk in device_common.h)
    const int wsub = (threadIdx.x & (WAVE - 1)) / SW;
    for (int64_t c0 = ORD ? next_chunk(ticket, chunk) : 0; c0 < n_seg;
         c0 = ORD ? next_chunk(ticket, chunk) : n_seg) {
    const int64_t c1 = ORD ? min(c0 + chunk, n_seg) : n_seg;
    for (int64_t it = ORD ? c0 + wsub : sub0; it < c1;
         it += ORD ? WAVE / SW : stride) {
        const int64_t r = seg_row[it];
        const int64_t e0 = seg_e0[it], e1 = seg_e1[it];
        const int64_t slot = seg_part[it];     // >= 0: row split across segments
        const float ds = dst_scale ? dst_scale[r] : 1.f;
        for (int64_t f0 = (int64_t)sl * VE; f0 < F; f0 += (int64_t)SW * VE) {
            float acc0[VE], acc1[VE];
#pragma unroll
            for (int k = 0; k < VE; ++k) { acc0[k] = 0.f; acc1[k] = 0.f; }

            // every batch starts at an even distance from e0, so edge e + u
            // goes to accumulator u & 1. The NB flags are loaded together,
            // then the NB predicated row loads (VE divides F: in bounds)
            auto batch = [&](int64_t e, auto nb_tag) {
                constexpr int NB = decltype(nb_tag)::value;
                int64_t c[NB];
                uint8_t lv[NB];
                float s[NB];
                Raw rv[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) c[u] = indices[e + u];
#pragma unroll
                for (int u = 0; u < NB; ++u)
                    lv[u] = live[c[u] < n_local ? c[u] : last_local];
                // one fetch bit per edge, made opaque to the compiler: all NB
                // flags are waited for HERE, once. Left to itself it waits
                // for flag u just before branch u, and since it cannot know
                // how many loads the earlier branches issued, that wait also
                // drains the row loads already in flight
                unsigned fetch = 0;
#pragma unroll
                for (int u = 0; u < NB; ++u)
                    fetch |= (unsigned)(c[u] >= n_local || lv[u]) << u;
                asm volatile("" : "+v"(fetch));
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const bool loc = c[u] < n_local;
                    const float* p = (loc ? xl + c[u] * F
                                          : xr + (c[u] - n_local) * F) + f0;
                    s[u] = 1.f;
                    rv[u] = Raw{};
                    if (fetch >> u & 1u) {
                        if (SS) s[u] = src_scale[c[u]];
                        rv[u] = *reinterpret_cast<const Raw*>(p);
                    }
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const float* v = reinterpret_cast<const float*>(&rv[u]);
#pragma unroll
                    for (int k = 0; k < VE; ++k) {
                        if (u & 1) acc1[k] = fmaf(v[k], s[u], acc1[k]);
                        else acc0[k] = fmaf(v[k], s[u], acc0[k]);
                    }
                }
            };
            int64_t e = e0;
            for (; e + 3 < e1; e += 4) batch(e, std::integral_constant<int, 4>{});
            for (; e + 1 < e1; e += 2) batch(e, std::integral_constant<int, 2>{});
            if (e < e1) batch(e, std::integral_constant<int, 1>{});

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
                *reinterpret_cast<Raw*>(y + r * F + f0) =
                    *reinterpret_cast<const Raw*>(outv);
            } else {
                // long row split across segments: fp32 partial into this
                // segment's own slot, summed by combine_parts_kernel<float>
                float* pp = part + slot * F + f0;
#pragma unroll
                for (int k = 0; k < VE; ++k)
                    pp[k] = (acc0[k] + acc1[k]) * ds;
            }
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
// vector width (fp32 elements per lane) and sub-wavefront width for F: the
// dense fp32 kernel's choice (spmm_csr, kernels.hip)
void spmm_rowskip_shape(int64_t F, int* ve, int* sw) {
    int v = 4;
    while (v > 1 && F % v) v >>= 1;
    int s = 16;
    while (s < 64 && (int64_t)s * v < F) s *= 2;
    *ve = v;
    *sw = s;
}

#define BY_SHAPE(RUN) do { \
        switch (sw) { \
            case 64: BY_VE(RUN, 64); break; \
            case 32: BY_VE(RUN, 32); break; \
            default: BY_VE(RUN, 16); break; \
        } \
    } while (0)
#define BY_VE(RUN, SWC) do { \
        switch (ve) { \
            case 4: RUN(SWC, 4); break; \
            case 2: RUN(SWC, 2); break; \
            default: RUN(SWC, 1); break; \
        } \
    } while (0)

torch::Tensor row_live(torch::Tensor x) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2 &&
                x.scalar_type() == torch::kFloat32,
                "row_live expects a contiguous fp32 [N, F] GPU tensor");
    const int64_t rows = x.size(0), F = x.size(1);
    torch::Tensor out = torch::empty({rows}, x.options().dtype(torch::kUInt8));
    if (rows == 0) return out;
    if (F == 0) return out.zero_();
    int ve, sw;
    spmm_rowskip_shape(F, &ve, &sw);
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % (4 * ve) == 0,
                "row_live: x must be aligned to the vector load width");
    const int64_t groups = (rows + RL_ROWS - 1) / RL_ROWS;
    const int64_t per_block = RL_THREADS / sw;
    const int64_t blocks = (groups + per_block - 1) / per_block;
    TORCH_CHECK(blocks < (1ll << 31), "row_live: tensor too large");
    const dim3 grid((unsigned)blocks), block(RL_THREADS);
    hipStream_t s = at::cuda::getCurrentHIPStream().stream();
#define RUN_LIVE(SWC, VEC) row_live_kernel<SWC, VEC><<<grid, block, 0, s>>>( \
        reinterpret_cast<const uint32_t*>(x.data_ptr<float>()), \
        out.data_ptr<uint8_t>(), rows, F)
    BY_SHAPE(RUN_LIVE);
#undef RUN_LIVE
    return out;
}

// called by spmm_csr_rowskip (kernels.hip), which checked the operands and
// allocated the partial slots
void launch_spmm_rowskip(
    hipStream_t s, const int32_t* indices, const float* xl, const float* xr,
    const uint8_t* live, float* y, const float* src_scale,
    const float* dst_scale, const int32_t* seg_row, const int32_t* seg_e0,
    const int32_t* seg_e1, const int32_t* seg_part, float* part,
    const float* addend, int64_t n_seg, int64_t F, int64_t n_local,
    int order, int chunk, int32_t* ticket) {
    int ve, sw;
    spmm_rowskip_shape(F, &ve, &sw);
    const int block_threads = 256;
    const int rows_per_block = block_threads / sw;
    const int64_t needed = (n_seg + rows_per_block - 1) / rows_per_block;
    const int64_t blocks = std::max<int64_t>(std::min<int64_t>(needed, 16384), 1);
    const dim3 block(block_threads);
    // order 1: the resident blocks of the instantiation, see ordered_grid
#define LAUNCH_O(SWC, VEC, SSC, ORDC) do { \
        dim3 grid(blocks); \
        if (ORDC) { \
            grid = dim3(ordered_grid(spmm_rowskip_kernel<SWC, VEC, SSC, ORDC>, \
                                     block_threads, needed)); \
            TORCH_CHECK(grid.x > 0, "row-skipping spmm: occupancy query failed"); \
        } \
        spmm_rowskip_kernel<SWC, VEC, SSC, ORDC><<<grid, block, 0, s>>>( \
            indices, xl, xr, live, y, src_scale, dst_scale, seg_row, seg_e0, \
            seg_e1, seg_part, part, addend, n_seg, F, n_local, chunk, ticket); \
    } while (0)
#define LAUNCH(SWC, VEC, SSC) do { \
        if (order) LAUNCH_O(SWC, VEC, SSC, true); \
        else LAUNCH_O(SWC, VEC, SSC, false); \
    } while (0)
#define RUN_SPMM(SWC, VEC) do { \
        if (src_scale) LAUNCH(SWC, VEC, true); else LAUNCH(SWC, VEC, false); \
    } while (0)
    BY_SHAPE(RUN_SPMM);
#undef RUN_SPMM
#undef LAUNCH
#undef LAUNCH_O
}
#undef BY_VE
#undef BY_SHAPE
