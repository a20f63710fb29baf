// Edge-compacting row-skipping SpMM (gfx950 / MI355X), fp32 and bf16: the
// gather of spmm_csr_kernel<SW, T, VE>, spending row fetches only on the
// edges whose row holds something.
//
// spmm_rowskip.hip skips the all-zero rows of the output layer's gradient,
// but it is fp32 only and it still walks every edge: each lane repeats the
// same index load and the same flag load, four edges per batch, and a batch
// with one live edge costs what a batch with four costs. With 92 % dead rows
// (the ogbn-products split) that walk is what the kernel spends its time on.
// Here a sub-wavefront finds the live edges of a segment cooperatively and
// its batches hold live edges only.
//
// Two kernels:
//
// row_live_bf16_kernel<SW, VE>   row_live_kernel for contiguous bf16 [N, F]
//   with even F -> uint8 [N]; 1 iff some halfword has bits & 0x7fff != 0:
//   denormals, NaN and Inf are live, -0.0 is not. A sub-wavefront of SW lanes
//   owns RLB_ROWS consecutive rows, a lane reads VE in {8, 4, 2} halfwords per
//   row with one 16/8/4-byte load (VE | F keeps them aligned), all RLB_ROWS
//   loads are issued before the first use and one ballot per row folds the
//   lanes. Rows past the end are clamped to the last row (loaded, not stored).
//
// spmm_compact_kernel<SW, T, VE, SS, ORD>   T = float (VE in {4, 2, 1}) or
//   ushort bf16 bits (VE in {8, 4, 2}); SW the smallest of 16/32/64 lanes
//   covering F. Segments, partial slots, the XCD swizzle, the ORD ordered
//   sweep and the epilogue are spmm_csr_kernel<SW, T, VE>'s. The edge loop:
//
//   chunk   the sub-wavefront takes the segment's edges SW at a time. Lane l
//           loads indices[eb + l] (one coalesced load per chunk), its own
//           flag live[min(c, n_local - 1)], and fetch = (c >= n_local) | flag;
//           with SS its src_scale[c], only where fetch is set.
//   ballot  one wave ballot gives the fetch mask; a sub-wavefront takes
//           its SW bits by shift and mask.
//   pop     the set bits are popped lowest first, up to four per batch (a tail
//           of 2 or 1 takes a batch of that size). Column and scale of
//           position j are broadcast from lane j (readlane for SW == 64, where
//           j is wave-uniform, else a width-SW shuffle), and the batch's row
//           loads are issued back to back before the first fmaf. A dead edge
//           costs its share of the coalesced index and flag loads and nothing
//           else.
//
//   Every lane of a sub-wavefront stays in the edge loop, because any lane may
//   hold the column of a live edge: lanes past F (F < SW * VE, or the last
//   pass of a wider row) gather from feature 0, which is in bounds, and store
//   nothing, as in spmm_csr_wave_kernel. The chunk masks are recomputed in
//   every pass of the outer feature loop.
//
//   Bit equality with the dense kernel. The dense kernel puts edge j of a
//   segment into accumulator j & 1, in increasing j, one fmaf each, both
//   accumulators starting at +0.f. Chunk bases lie a multiple of SW, so an
//   even distance, from e0: the parity of a chunk position is the parity of
//   the edge. A live edge at position j is accumulated into accumulator j & 1
//   with one fmaf(to_f32(v), s, acc); the parity is a run-time value, and the
//   accumulator is picked by selecting on the RESULT (v_cndmask), never by a
//   multiplication by zero, so an Inf or NaN row reaches its own accumulator
//   only. Each accumulator thus receives exactly its live edges in increasing
//   edge order. For a dead edge the dense kernel computes fmaf(+-0, s, acc)
//   with a finite s, which returns acc (acc starts at +0 and a sum only
//   becomes -0 from two -0 terms), so leaving it out changes nothing. The one
//   exception is the one spmm_rowskip.hip documents: an accumulator that an
//   underflowing product already turned into -0.f meeting a dead row of -0.0
//   values. Remote columns are always fetched.
//
// No LDS and no matrix instructions: a gathered row is used once, by one
// sub-wavefront, so there is no reuse for either to exploit. Data goes from
// global memory to registers; the only cross-lane traffic is the ballot and
// the broadcasts.
//
// Built without packed fp32 instructions (v_pk_fma_f32 and kin), as
// spmm_rowskip.hip: a lane's fmafs are scalar v_fma_f32.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>
#include <type_traits>

#include "device_common.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// ---------------------------------------------------------------------------
// liveness pass, bf16
// ---------------------------------------------------------------------------
#define RLB_THREADS 256
#define RLB_ROWS 4         // rows per sub-wavefront, loads in flight per lane

template <int SW, int VE>
__global__ void __launch_bounds__(RLB_THREADS) row_live_bf16_kernel(
    const ushort* __restrict__ x, uint8_t* __restrict__ live,
    int64_t rows, int64_t F) {
    using Raw = typename RawVec<VE * 2>::type;
    constexpr int groups = RLB_THREADS / SW;
    const int64_t grp = (int64_t)blockIdx.x * groups + threadIdx.x / SW;
    const int sl = threadIdx.x & (SW - 1);
    const int64_t r0 = grp * RLB_ROWS;
    uint32_t any[RLB_ROWS];
    const ushort* base[RLB_ROWS];
#pragma unroll
    for (int u = 0; u < RLB_ROWS; ++u) {
        any[u] = 0u;
        const int64_t r = r0 + u < rows ? r0 + u : rows - 1;   // rows > 0
        base[u] = x + r * F;
    }
    for (int64_t f0 = (int64_t)sl * VE; f0 < F; f0 += (int64_t)SW * VE) {
        Raw v[RLB_ROWS];
#pragma unroll
        for (int u = 0; u < RLB_ROWS; ++u)
            v[u] = *reinterpret_cast<const Raw*>(base[u] + f0);
#pragma unroll
        for (int u = 0; u < RLB_ROWS; ++u) {
            // two halfwords per word, the sign bit of each masked off
            const uint32_t* w = reinterpret_cast<const uint32_t*>(&v[u]);
#pragma unroll
            for (int k = 0; k < VE / 2; ++k) any[u] |= w[k] & 0x7FFF7FFFu;
        }
    }
    // every lane of the wavefront gets here: fold each row's lanes
    const int shift = ((threadIdx.x & (WAVE - 1)) / SW) * SW;
    constexpr uint64_t mask = SW == 64 ? ~0ull : ((1ull << (SW & 63)) - 1ull);
#pragma unroll
    for (int u = 0; u < RLB_ROWS; ++u) {
        const uint64_t b = __builtin_amdgcn_ballot_w64(any[u] != 0u);
        if (sl == 0 && r0 + u < rows)
            live[r0 + u] = ((b >> shift) & mask) != 0ull ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------
// The cross-lane and bit helpers below are compiler builtins on purpose. The
// HIP header's __ballot, __shfl, __popc and __float_as_int are compiled with
// the default target features, the functions of this file without packed
// fp32, and the compiler does not inline across that difference: each use
// would be a call (s_swappc_b64) in the edge loop.
//
// value of lane j of the calling sub-wavefront, whose first lane is `base`.
// SW == 64: the sub-wavefront is the wavefront and j is the same in every
// lane, so it is a readlane; below that a width-SW shuffle (ds_bpermute)
template <int SW>
__device__ __forceinline__ int bcast_i32(int v, int j, int base) {
    if constexpr (SW == 64)
        return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(j));
    else
        return __builtin_amdgcn_ds_bpermute((base + j) << 2, v);
}
template <int SW>
__device__ __forceinline__ float bcast_f32(float v, int j, int base) {
    return __builtin_bit_cast(
        float, bcast_i32<SW>(__builtin_bit_cast(int, v), j, base));
}

__device__ __forceinline__ int low_bit(uint64_t m) { return __builtin_ctzll(m); }
__device__ __forceinline__ int low_bit(uint32_t m) { return __builtin_ctz(m); }
__device__ __forceinline__ int bit_count(uint64_t m) { return __builtin_popcountll(m); }
__device__ __forceinline__ int bit_count(uint32_t m) { return __builtin_popcount(m); }

template <int SW, typename T, int VE, bool SS, bool ORD>
__global__ void __launch_bounds__(256) spmm_compact_kernel(
    const int32_t* __restrict__ indices,
    const T* __restrict__ xl, const T* __restrict__ xr,
    const uint8_t* __restrict__ live,
    T* __restrict__ y,
    const float* __restrict__ src_scale, const float* __restrict__ dst_scale,
    const int32_t* __restrict__ seg_row, const int32_t* __restrict__ seg_e0,
    const int32_t* __restrict__ seg_e1, const int32_t* __restrict__ seg_part,
    float* __restrict__ part, const T* __restrict__ addend,
    int64_t n_seg, int64_t F, int64_t n_local,
    int chunk, int32_t* __restrict__ ticket) {
    using Raw = typename RawVec<VE * sizeof(T)>::type;
    // a sub-wavefront's share of the ballot: one word is enough below 64 lanes
    using Mask = typename std::conditional<SW == 64, uint64_t, uint32_t>::type;
    constexpr Mask sub_mask = SW == 64 ? ~(Mask)0 : (Mask)((1ull << (SW & 63)) - 1ull);
    const int rows_per_block = blockDim.x / SW;
    // bijective XCD swizzle, as spmm_csr_kernel
    const int64_t nwg = gridDim.x;
    const int64_t q = nwg / 8, rem = nwg % 8;
    const int64_t xcd = blockIdx.x % 8, idx = blockIdx.x / 8;
    const int64_t swz = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + idx;
    const int64_t sub0 = swz * rows_per_block + threadIdx.x / SW;
    const int64_t stride = nwg * rows_per_block;
    const int sl = threadIdx.x & (SW - 1);
    // columns, n_local and F all fit 31 bits (host-checked)
    const uint32_t nl = (uint32_t)n_local, Fu = (uint32_t)F;
    const uint32_t last_local = nl - 1u;                 // n_local > 0
    // !ORD: one pass of the static grid-stride loop; ORD: the ordered
    // sweep, as spmm_csr_kernel (next_chunk in device_common.h)
    const int wsub = (threadIdx.x & (WAVE - 1)) / SW;
    const int shift = wsub * SW;
    for (int64_t c0 = ORD ? next_chunk(ticket, chunk) : 0; c0 < n_seg;
         c0 = ORD ? next_chunk(ticket, chunk) : n_seg) {
    const int64_t c1 = ORD ? min(c0 + chunk, n_seg) : n_seg;
    for (int64_t it = ORD ? c0 + wsub : sub0; it < c1;
         it += ORD ? WAVE / SW : stride) {
        const int64_t r = seg_row[it];
        const int e0 = seg_e0[it], e1 = seg_e1[it];
        const int64_t slot = seg_part[it];     // >= 0: row split across segments
        const float ds = dst_scale ? dst_scale[r] : 1.f;
        for (int64_t fc = 0; fc < F; fc += (int64_t)SW * VE) {
            // all SW lanes stay in the edge loop (any of them may hold a live
            // edge's column); those past F gather from feature 0 (in bounds,
            // VE | F) and store nothing
            const int64_t fl = fc + (int64_t)sl * VE;
            const bool active = fl < F;
            const int64_t f0 = active ? fl : 0;
            float acc0[VE], acc1[VE];
#pragma unroll
            for (int k = 0; k < VE; ++k) { acc0[k] = 0.f; acc1[k] = 0.f; }

            for (int eb = e0; eb < e1; eb += SW) {
                // chunk: lane sl holds edge eb + sl
                int myc = 0;
                float mys = 1.f;
                bool fetch = false;
                if (sl < e1 - eb) {
                    myc = indices[eb + sl];
                    const uint32_t c = (uint32_t)myc;
                    const uint8_t flag = live[c < nl ? c : last_local];
                    fetch = c >= nl || flag;
                    if (SS && fetch) mys = src_scale[c];
                }
                // ballot: this sub-wavefront's live positions
                Mask m = (Mask)(__builtin_amdgcn_ballot_w64(fetch) >> shift)
                         & sub_mask;

                // pop: NB live positions lowest first, their rows loaded back
                // to back (VE divides F: in bounds), then accumulated, the
                // edge at position j into accumulator j & 1
                auto batch = [&](auto nb_tag) {
                    constexpr int NB = decltype(nb_tag)::value;
                    int j[NB];
                    float s[NB];
                    Raw rv[NB];
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        j[u] = low_bit(m);
                        m &= m - 1;
                    }
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        const uint32_t c =
                            (uint32_t)bcast_i32<SW>(myc, j[u], shift);
                        s[u] = SS ? bcast_f32<SW>(mys, j[u], shift) : 1.f;
                        const bool loc = c < nl;
                        const T* p = (loc ? xl : xr)
                            + (uint64_t)(loc ? c : c - nl) * Fu + f0;
                        rv[u] = *reinterpret_cast<const Raw*>(p);
                    }
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        const T* v = reinterpret_cast<const T*>(&rv[u]);
                        const bool odd = j[u] & 1;
#pragma unroll
                        for (int k = 0; k < VE; ++k) {
                            const float a = fmaf(to_f32<T>(v[k]), s[u],
                                                 odd ? acc1[k] : acc0[k]);
                            acc0[k] = odd ? acc0[k] : a;
                            acc1[k] = odd ? a : acc1[k];
                        }
                    }
                };
                while (m) {
                    const int n = bit_count(m);
                    if (n >= 4) batch(std::integral_constant<int, 4>{});
                    else if (n >= 2) batch(std::integral_constant<int, 2>{});
                    else batch(std::integral_constant<int, 1>{});
                }
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
                // long row split across segments: fp32 partial into this
                // segment's own slot, summed by combine_parts_kernel<T>
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
// vector width (elements per lane) and sub-wavefront width for F: the dense
// kernel's choice for the dtype (spmm_csr, kernels.hip)
void spmm_compact_shape(bool bf16, int64_t F, int* ve, int* sw) {
    int v = bf16 ? 8 : 4;
    while (v > 1 && F % v) v >>= 1;
    if (bf16 && v == 1) v = 2;                // bf16 loads are >= one dword
    int s = 16;
    while (s < 64 && (int64_t)s * v < F) s *= 2;
    *ve = v;
    *sw = s;
}

#define BY_SW(RUN, ...) do { \
        switch (sw) { \
            case 64: RUN(64, __VA_ARGS__); break; \
            case 32: RUN(32, __VA_ARGS__); break; \
            default: RUN(16, __VA_ARGS__); break; \
        } \
    } while (0)

torch::Tensor row_live_bf16(torch::Tensor x) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2 &&
                x.scalar_type() == torch::kBFloat16 && x.size(1) % 2 == 0,
                "row_live_bf16 expects a contiguous bf16 [N, F] GPU tensor "
                "with even F");
    const int64_t rows = x.size(0), F = x.size(1);
    torch::Tensor out = torch::empty({rows}, x.options().dtype(torch::kUInt8));
    if (rows == 0) return out;
    if (F == 0) return out.zero_();
    int ve, sw;
    spmm_compact_shape(true, F, &ve, &sw);
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % (2 * ve) == 0,
                "row_live_bf16: x must be aligned to the vector load width");
    const int64_t groups = (rows + RLB_ROWS - 1) / RLB_ROWS;
    const int64_t per_block = RLB_THREADS / sw;
    const int64_t blocks = (groups + per_block - 1) / per_block;
    TORCH_CHECK(blocks < (1ll << 31), "row_live_bf16: tensor too large");
    const dim3 grid((unsigned)blocks), block(RLB_THREADS);
    hipStream_t s = at::cuda::getCurrentHIPStream().stream();
#define RUN_LIVE(SWC, VEC) row_live_bf16_kernel<SWC, VEC><<<grid, block, 0, s>>>( \
        reinterpret_cast<const ushort*>(x.data_ptr()), \
        out.data_ptr<uint8_t>(), rows, F)
    switch (ve) {
        case 8: BY_SW(RUN_LIVE, 8); break;
        case 4: BY_SW(RUN_LIVE, 4); break;
        default: BY_SW(RUN_LIVE, 2); break;
    }
#undef RUN_LIVE
    return out;
}

// called by spmm_csr_compact (kernels.hip), which checked the operands and
// allocated the partial slots. xl, xr, y and addend are float or bf16 bits.
template <typename T>
static void launch_compact_t(
    hipStream_t s, int ve, int sw, const int32_t* indices, const T* xl,
    const T* xr, const uint8_t* live, T* y, const float* src_scale,
    const float* dst_scale, const int32_t* seg_row, const int32_t* seg_e0,
    const int32_t* seg_e1, const int32_t* seg_part, float* part,
    const T* addend, int64_t n_seg, int64_t F, int64_t n_local,
    int order, int chunk, int32_t* ticket) {
    const int block_threads = 256;
    const int rows_per_block = block_threads / sw;
    const int64_t needed = (n_seg + rows_per_block - 1) / rows_per_block;
    const int64_t blocks = std::max<int64_t>(std::min<int64_t>(needed, 16384), 1);
    const dim3 block(block_threads);
    // order 1: the resident blocks of the instantiation, see ordered_grid
#define LAUNCH_O(SWC, VEC, SSC, ORDC) do { \
        dim3 grid(blocks); \
        if (ORDC) { \
            grid = dim3(ordered_grid(spmm_compact_kernel<SWC, T, VEC, SSC, ORDC>, \
                                     block_threads, needed)); \
            TORCH_CHECK(grid.x > 0, "compacting spmm: occupancy query failed"); \
        } \
        spmm_compact_kernel<SWC, T, VEC, SSC, ORDC><<<grid, block, 0, s>>>( \
            indices, xl, xr, live, y, src_scale, dst_scale, seg_row, seg_e0, \
            seg_e1, seg_part, part, addend, n_seg, F, n_local, chunk, ticket); \
    } while (0)
#define LAUNCH(SWC, VEC) do { \
        if (src_scale) { \
            if (order) LAUNCH_O(SWC, VEC, true, true); \
            else LAUNCH_O(SWC, VEC, true, false); \
        } else { \
            if (order) LAUNCH_O(SWC, VEC, false, true); \
            else LAUNCH_O(SWC, VEC, false, false); \
        } \
    } while (0)
    // VE: {8, 4, 2} bf16 elements or {4, 2, 1} fp32 ones, 16/8/4 bytes
    constexpr int V0 = 16 / sizeof(T);
    if (ve == V0) BY_SW(LAUNCH, V0);
    else if (ve == V0 / 2) BY_SW(LAUNCH, V0 / 2);
    else BY_SW(LAUNCH, V0 / 4);
#undef LAUNCH
#undef LAUNCH_O
}
#undef BY_SW

void launch_spmm_compact(
    hipStream_t s, bool bf16, const int32_t* indices, const void* xl,
    const void* xr, const uint8_t* live, void* y, const float* src_scale,
    const float* dst_scale, const int32_t* seg_row, const int32_t* seg_e0,
    const int32_t* seg_e1, const int32_t* seg_part, float* part,
    const void* addend, int64_t n_seg, int64_t F, int64_t n_local,
    int order, int chunk, int32_t* ticket) {
    int ve, sw;
    spmm_compact_shape(bf16, F, &ve, &sw);
    if (bf16)
        launch_compact_t<ushort>(
            s, ve, sw, indices, static_cast<const ushort*>(xl),
            static_cast<const ushort*>(xr), live, static_cast<ushort*>(y),
            src_scale, dst_scale, seg_row, seg_e0, seg_e1, seg_part, part,
            static_cast<const ushort*>(addend), n_seg, F, n_local, order,
            chunk, ticket);
    else
        launch_compact_t<float>(
            s, ve, sw, indices, static_cast<const float*>(xl),
            static_cast<const float*>(xr), live, static_cast<float*>(y),
            src_scale, dst_scale, seg_row, seg_e0, seg_e1, seg_part, part,
            static_cast<const float*>(addend), n_seg, F, n_local, order,
            chunk, ticket);
}
