// Packed sparse rows and the packed-gather SpMM (gfx950 / MI355X).
//
// The forward aggregation of layers > 0 gathers dropout(relu(norm(h))):
// three quarters of every gathered row are zeros, and the dense SpMM still
// pulls all of its 128-byte lines for every edge. pack_rows makes one pass
// over a contiguous fp32 [N, F] tensor (F % 4 == 0, F <= 256) and writes a
// fixed-stride packed copy; spmm_packed_kernel is spmm_csr_kernel with
// only the fetch of a gathered value changed, so its result is the same
// bit for bit.
//
// Packed row layout (G = F / 4 lane groups, group g = features 4g..4g+3):
//
//   byte 0            G 16-bit words, word g =
//                       bits 0-7   offset of the group's first kept value in
//                                  the row's value run (kept values before it)
//                       bits 8-11  presence mask, bit k = feature 4g + k kept
//                       bit  15    row overflow (same in every word of a row)
//   byte META         the row's kept values as fp32, in feature order,
//                     capacity F / 2
//   META   = 2 G rounded up to 16 bytes
//   stride = META + 2 F rounded up to 128 bytes (F = 256: 128 + 512 = 640)
//
// "Kept" is any element whose bit pattern is not all-zero: -0.0, denormals,
// NaN and inf are values. A row with more than F / 2 kept elements is an
// overflow row: its words carry bit 15, no values are stored, and the SpMM
// reads that row from the dense tensor. Bytes the layout does not name
// (word padding, unused value capacity) are never written.
//
// The SpMM lane of group g reads word g, then ONE 16-byte window at the
// 4-byte-aligned address of its first kept value and expands it with the
// mask (+0.0f for absent features). The window of a row's last group can
// reach 16 bytes past the value capacity (offset <= F / 2), which for the
// last row is past its stride: the buffer is allocated with PACK_TAIL
// extra bytes so that no load leaves the allocation.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>

#include "device_common.h"

#define PACK_TAIL 16

static inline int64_t pack_meta_bytes(int64_t F) {
    return ((F / 4) * 2 + 15) / 16 * 16;
}
static inline int64_t pack_stride(int64_t F) {
    return (pack_meta_bytes(F) + 2 * F + 127) / 128 * 128;
}

// ---------------------------------------------------------------------------
// pack: one sub-wavefront of SW lanes per row, lane g < G owns group g.
// ---------------------------------------------------------------------------
template <int SW>
__global__ void pack_rows_kernel(const float* __restrict__ x,
                                 uint8_t* __restrict__ pk, int64_t n, int F,
                                 int meta, int64_t stride) {
    const int rows_per_block = blockDim.x / SW;
    const int64_t row = (int64_t)blockIdx.x * rows_per_block + threadIdx.x / SW;
    const int sl = threadIdx.x & (SW - 1);
    // every lane takes part in the scan; lanes without a group count zero
    const bool active = row < n && sl < (F >> 2);
    uint4 b = {0u, 0u, 0u, 0u};
    if (active)
        b = *reinterpret_cast<const uint4*>(x + row * F + 4 * sl);
    const uint32_t mask = (b.x != 0u) | ((b.y != 0u) << 1) |
                          ((b.z != 0u) << 2) | ((b.w != 0u) << 3);
    const int cnt = __popc(mask);
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < SW; o <<= 1) {
        const int t = __shfl_up(inc, o, SW);
        if (sl >= o) inc += t;
    }
    const int total = __shfl(inc, SW - 1, SW);
    if (!active) return;
    const bool ovf = total > (F >> 1);
    const int off = inc - cnt;
    uint8_t* base = pk + row * stride;
    reinterpret_cast<uint16_t*>(base)[sl] =
        (uint16_t)((off & 0xFF) | (mask << 8) | (ovf ? 0x8000u : 0u));
    if (ovf) return;
    uint32_t* v = reinterpret_cast<uint32_t*>(base + meta) + off;
    int i = 0;
    if (mask & 1u) v[i++] = b.x;
    if (mask & 2u) v[i++] = b.y;
    if (mask & 4u) v[i++] = b.z;
    if (mask & 8u) v[i] = b.w;
}

// ---------------------------------------------------------------------------
// packed-gather SpMM, sub-wavefronts of SW = 16 or 32 lanes per segment
// (F <= 128): spmm_csr_kernel<SW, float, 4> with the fetch changed.
// Same segments, slots, scales, addend and accumulation order: edge j of a
// segment goes into accumulator j & 1 in increasing j, one fmaf per feature
// (also for absent features: v = +0.0f, the fmaf is kept), epilogue
// (acc0 + acc1) * ds. NE row fetches are in flight per lane; every batch
// starts at an even j.
// ---------------------------------------------------------------------------
// 16 bytes at a 4-byte-aligned address (one global_load_dwordx4)
struct __attribute__((packed, aligned(4))) Win4 { uint32_t w[4]; };

// SS: a src_scale vector is given (a template flag, so that the batch
// below stays one basic block and its loads are issued together)
template <int SW, int NE, bool SS>
__global__ void __launch_bounds__(WAVE * 4) spmm_packed_kernel(
    const int32_t* __restrict__ indices,
    const float* __restrict__ xl, const float* __restrict__ xr,
    const uint8_t* __restrict__ pk,
    float* __restrict__ y,
    const float* __restrict__ src_scale, const float* __restrict__ dst_scale,
    const int32_t* __restrict__ seg_row, const int32_t* __restrict__ seg_e0,
    const int32_t* __restrict__ seg_e1, const int32_t* __restrict__ seg_part,
    float* __restrict__ part, const float* __restrict__ addend,
    int64_t n_seg, int64_t F, int64_t n_local, int64_t meta, int64_t stride) {
    constexpr int VE = 4;
    const int rows_per_block = blockDim.x / SW;
    // bijective XCD swizzle, as spmm_csr_kernel
    const int64_t nwg = gridDim.x;
    const int64_t q = nwg / 8, rem = nwg % 8;
    const int64_t xcd = blockIdx.x % 8, idx = blockIdx.x / 8;
    const int64_t swz = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + idx;
    const int64_t sub0 = swz * rows_per_block + threadIdx.x / SW;
    const int64_t step = nwg * rows_per_block;
    const int sl = threadIdx.x & (SW - 1);
    const int64_t f0 = (int64_t)sl * VE;     // SW * VE >= F (host-checked)
    if (f0 >= F) return;
    const uint8_t* pkw = pk + 2 * sl;        // this lane's word in row 0
    const uint8_t* pkv = pk + meta;          // value run of row 0

    for (int64_t it = sub0; it < n_seg; it += step) {
        const int64_t r = seg_row[it];
        const int64_t e0 = seg_e0[it], e1 = seg_e1[it];
        const int64_t slot = seg_part[it];
        const float ds = dst_scale ? dst_scale[r] : 1.f;
        float acc0[VE], acc1[VE];
#pragma unroll
        for (int k = 0; k < VE; ++k) { acc0[k] = 0.f; acc1[k] = 0.f; }

        auto batch = [&](int64_t e, auto nb_tag) {
            constexpr int NB = decltype(nb_tag)::value;
            int64_t c[NB], cm[NB];
            float s[NB];
            uint32_t w[NB];
            Win4 win[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) c[u] = indices[e + u];
            // a remote column reads row 0's word (n_local > 0, host-checked)
            // and ignores it: no branch between the loads
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                s[u] = SS ? src_scale[c[u]] : 1.f;
                cm[u] = c[u] < n_local ? c[u] : 0;
                w[u] = *reinterpret_cast<const uint16_t*>(pkw + cm[u] * stride);
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const bool loc = c[u] < n_local;
                const bool dense = !loc || (w[u] & 0x8000u);
                const float* dp = (loc ? xl + c[u] * F : xr + (c[u] - n_local) * F) + f0;
                const float* pp = reinterpret_cast<const float*>(pkv + cm[u] * stride)
                                  + (w[u] & 0xFFu);
                win[u] = *reinterpret_cast<const Win4*>(dense ? dp : pp);
                w[u] = dense ? 0xFu : (w[u] >> 8) & 0xFu;
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                // expand: feature k takes the next window word if present
                uint32_t t0 = win[u].w[0], t1 = win[u].w[1];
                uint32_t t2 = win[u].w[2], t3 = win[u].w[3];
                float v[VE];
                const bool b0 = w[u] & 1u, b1 = w[u] & 2u;
                const bool b2 = w[u] & 4u, b3 = w[u] & 8u;
                v[0] = __uint_as_float(b0 ? t0 : 0u);
                t0 = b0 ? t1 : t0; t1 = b0 ? t2 : t1; t2 = b0 ? t3 : t2;
                v[1] = __uint_as_float(b1 ? t0 : 0u);
                t0 = b1 ? t1 : t0; t1 = b1 ? t2 : t1;
                v[2] = __uint_as_float(b2 ? t0 : 0u);
                t0 = b2 ? t1 : t0;
                v[3] = __uint_as_float(b3 ? t0 : 0u);
#pragma unroll
                for (int k = 0; k < VE; ++k) {
                    if (u & 1) acc1[k] = fmaf(v[k], s[u], acc1[k]);
                    else acc0[k] = fmaf(v[k], s[u], acc0[k]);
                }
            }
        };
        int64_t e = e0;
        if constexpr (NE >= 8)
            for (; e + 7 < e1; e += 8) batch(e, std::integral_constant<int, 8>{});
        for (; e + 3 < e1; e += 4) batch(e, std::integral_constant<int, 4>{});
        for (; e + 1 < e1; e += 2) batch(e, std::integral_constant<int, 2>{});
        if (e < e1) batch(e, std::integral_constant<int, 1>{});

        using Raw = typename RawVec<16>::type;
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
            float* pp = part + slot * F + f0;
#pragma unroll
            for (int k = 0; k < VE; ++k)
                pp[k] = (acc0[k] + acc1[k]) * ds;
        }
    }
}

// ---------------------------------------------------------------------------
// packed-gather SpMM, one whole wavefront per segment (SW == 64: F > 128).
// Same result bit for bit. The per-lane kernel above spends most of its
// instructions on per-edge integer work that is the same in all 64 lanes
// (column, local/remote select, two 64-bit row offsets), and with fewer
// bytes per edge that work, not the memory system, sets its time. Here, as
// in spmm_csr_wave_kernel, a chunk of 64 column indices (and src scales) is
// fetched with one coalesced load, each edge's column is broadcast with
// readlane, and the row bases are scalar arithmetic; per lane remain the
// word load, the window address, the window load, the expand and the FMAs.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float readlane_f32(float v, int l) {
    return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), l));
}

template <int NE, bool SS>
__global__ void __launch_bounds__(WAVE * 4) spmm_packed_wave_kernel(
    const int32_t* __restrict__ indices,
    const float* __restrict__ xl, const float* __restrict__ xr,
    const uint8_t* __restrict__ pk,
    float* __restrict__ y,
    const float* __restrict__ src_scale, const float* __restrict__ dst_scale,
    const int32_t* __restrict__ seg_row, const int32_t* __restrict__ seg_e0,
    const int32_t* __restrict__ seg_e1, const int32_t* __restrict__ seg_part,
    float* __restrict__ part, const float* __restrict__ addend,
    int64_t n_seg, int64_t F, int64_t n_local, int64_t meta, int64_t stride) {
    constexpr int VE = 4;
    const int waves_per_block = blockDim.x / WAVE;
    const int64_t nwg = gridDim.x;
    const int64_t q = nwg / 8, rem = nwg % 8;
    const int64_t xcd = blockIdx.x % 8, idx = blockIdx.x / 8;
    const int64_t swz = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + idx;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t step = nwg * waves_per_block;
    // lanes past F take part in the index loads and broadcasts; they fetch
    // as group 0 (in bounds) and store nothing
    const bool active = (int64_t)lane * VE < F;
    const uint32_t g = active ? lane : 0;
    const uint32_t f0 = g * VE;
    // columns, n_local, F and the stride fit 32 bits (host-checked)
    const uint32_t nl = (uint32_t)n_local, Fu = (uint32_t)F;
    const uint32_t st = (uint32_t)stride, mt = (uint32_t)meta;

    for (int64_t it = swz * waves_per_block + wave; it < n_seg; it += step) {
        const int64_t r = __builtin_amdgcn_readfirstlane(seg_row[it]);
        const int e0 = __builtin_amdgcn_readfirstlane(seg_e0[it]);
        const int e1 = __builtin_amdgcn_readfirstlane(seg_e1[it]);
        const int slot = __builtin_amdgcn_readfirstlane(seg_part[it]);
        const float ds = dst_scale
            ? __uint_as_float(__builtin_amdgcn_readfirstlane(
                  __float_as_uint(dst_scale[r])))
            : 1.f;
        float acc0[VE], acc1[VE];
#pragma unroll
        for (int k = 0; k < VE; ++k) { acc0[k] = 0.f; acc1[k] = 0.f; }
        for (int eb = e0; eb < e1; eb += WAVE) {
            const int n = min(e1 - eb, WAVE);
            int myc = 0;
            float mys = 1.f;
            if (lane < n) {
                myc = indices[eb + lane];
                if (SS) mys = src_scale[myc];
            }
            // edges [0, n) of this chunk, lane l holding edge eb + l; every
            // batch starts at an even j, so edge j + u goes to acc (u & 1)
            auto batch = [&](int j, auto nb_tag) {
                constexpr int NB = decltype(nb_tag)::value;
                uint32_t c[NB], w[NB];
                float s[NB];
                const uint8_t* rowp[NB];
                Win4 win[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    c[u] = (uint32_t)__builtin_amdgcn_readlane(myc, j + u);
                    s[u] = SS ? readlane_f32(mys, j + u) : 1.f;
                    // a remote column reads row 0's word and ignores it
                    rowp[u] = pk + (uint64_t)(c[u] < nl ? c[u] : 0u) * st;
                    w[u] = *reinterpret_cast<const uint16_t*>(rowp[u] + 2 * g);
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const bool loc = c[u] < nl;
                    const bool dense = !loc || (w[u] & 0x8000u);
                    const float* dp = (loc ? xl : xr)
                        + (uint64_t)(loc ? c[u] : c[u] - nl) * Fu + f0;
                    const uint8_t* pp = rowp[u] + mt + 4 * (w[u] & 0xFFu);
                    win[u] = *reinterpret_cast<const Win4*>(
                        dense ? reinterpret_cast<const uint8_t*>(dp) : pp);
                    w[u] = dense ? 0xFu : (w[u] >> 8) & 0xFu;
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    uint32_t t0 = win[u].w[0], t1 = win[u].w[1];
                    uint32_t t2 = win[u].w[2], t3 = win[u].w[3];
                    float v[VE];
                    const bool b0 = w[u] & 1u, b1 = w[u] & 2u;
                    const bool b2 = w[u] & 4u, b3 = w[u] & 8u;
                    v[0] = __uint_as_float(b0 ? t0 : 0u);
                    t0 = b0 ? t1 : t0; t1 = b0 ? t2 : t1; t2 = b0 ? t3 : t2;
                    v[1] = __uint_as_float(b1 ? t0 : 0u);
                    t0 = b1 ? t1 : t0; t1 = b1 ? t2 : t1;
                    v[2] = __uint_as_float(b2 ? t0 : 0u);
                    t0 = b2 ? t1 : t0;
                    v[3] = __uint_as_float(b3 ? t0 : 0u);
#pragma unroll
                    for (int k = 0; k < VE; ++k) {
                        if (u & 1) acc1[k] = fmaf(v[k], s[u], acc1[k]);
                        else acc0[k] = fmaf(v[k], s[u], acc0[k]);
                    }
                }
            };
            int j = 0;
            if constexpr (NE >= 8)
                for (; j + 7 < n; j += 8) batch(j, std::integral_constant<int, 8>{});
            for (; j + 3 < n; j += 4) batch(j, std::integral_constant<int, 4>{});
            for (; j + 1 < n; j += 2) batch(j, std::integral_constant<int, 2>{});
            if (j < n) batch(j, std::integral_constant<int, 1>{});
        }
        if (!active) continue;
        using Raw = typename RawVec<16>::type;
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
            float* pp = part + (int64_t)slot * F + f0;
#pragma unroll
            for (int k = 0; k < VE; ++k)
                pp[k] = (acc0[k] + acc1[k]) * ds;
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
bool spmm_packable(int64_t F) { return F > 0 && F % 4 == 0 && F <= 256; }

int64_t packed_meta_bytes(int64_t F) { return pack_meta_bytes(F); }
int64_t packed_row_stride(int64_t F) { return pack_stride(F); }
int64_t packed_buffer_bytes(int64_t n, int64_t F) {
    return n * pack_stride(F) + PACK_TAIL;
}

static inline int sub_wave(int64_t F) {
    int sw = 16;
    while (sw < 64 && (int64_t)sw * 4 < F) sw *= 2;
    return sw;
}

torch::Tensor pack_rows(torch::Tensor x) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2,
                "pack_rows expects a contiguous [N, F] GPU tensor");
    TORCH_CHECK(x.scalar_type() == torch::kFloat32 && spmm_packable(x.size(1)),
                "pack_rows expects fp32 with F % 4 == 0 and F <= 256");
    const int64_t n = x.size(0), F = x.size(1);
    torch::Tensor pk = torch::empty({packed_buffer_bytes(n, F)},
                                    x.options().dtype(torch::kUInt8));
    if (n == 0) return pk;
    const int sw = sub_wave(F);
    const int block_threads = WAVE * 4;
    const int rows_per_block = block_threads / sw;
    const dim3 grid((n + rows_per_block - 1) / rows_per_block), block(block_threads);
    auto s = at::cuda::getCurrentHIPStream().stream();
#define LAUNCH(SWC) pack_rows_kernel<SWC><<<grid, block, 0, s>>>( \
        x.data_ptr<float>(), pk.data_ptr<uint8_t>(), n, (int)F, \
        (int)pack_meta_bytes(F), pack_stride(F))
    switch (sw) {
        case 64: LAUNCH(64); break;
        case 32: LAUNCH(32); break;
        default: LAUNCH(16); break;
    }
#undef LAUNCH
    return pk;
}

// called by spmm_csr (kernels.hip) with the grid it computed for the dense
// kernel; the checks on shapes and dtypes are made there
void launch_spmm_packed(
    dim3 grid, dim3 block, hipStream_t s, int depth,
    const int32_t* indices, const float* xl, const float* xr,
    const uint8_t* pk, float* y, const float* src_scale,
    const float* dst_scale, const int32_t* seg_row, const int32_t* seg_e0,
    const int32_t* seg_e1, const int32_t* seg_part, float* part,
    const float* addend, int64_t n_seg, int64_t F, int64_t n_local) {
    TORCH_CHECK(depth == 4 || depth == 8, "packed SpMM depth must be 4 or 8");
    TORCH_CHECK(n_local < (1ll << 31), "packed spmm: n_local must fit 31 bits");
    // SW == 64 runs the wave-uniform kernel, narrower rows the per-lane one
    const int sw = sub_wave(F);
#define LAUNCH(SWC, NEC, SSC) spmm_packed_kernel<SWC, NEC, SSC><<<grid, block, 0, s>>>( \
        indices, xl, xr, pk, y, src_scale, dst_scale, seg_row, seg_e0, \
        seg_e1, seg_part, part, addend, n_seg, F, n_local, \
        pack_meta_bytes(F), pack_stride(F))
#define BY_DEPTH(SWC) do { \
        if (src_scale) { if (depth == 8) LAUNCH(SWC, 8, true); else LAUNCH(SWC, 4, true); } \
        else { if (depth == 8) LAUNCH(SWC, 8, false); else LAUNCH(SWC, 4, false); } \
    } while (0)
#define LAUNCH_W(NEC, SSC) spmm_packed_wave_kernel<NEC, SSC><<<grid, block, 0, s>>>( \
        indices, xl, xr, pk, y, src_scale, dst_scale, seg_row, seg_e0, \
        seg_e1, seg_part, part, addend, n_seg, F, n_local, \
        pack_meta_bytes(F), pack_stride(F))
    switch (sw) {
        case 64:
            if (src_scale) { if (depth == 8) LAUNCH_W(8, true); else LAUNCH_W(4, true); }
            else { if (depth == 8) LAUNCH_W(8, false); else LAUNCH_W(4, false); }
            break;
        case 32: BY_DEPTH(32); break;
        default: BY_DEPTH(16); break;
    }
#undef LAUNCH_W
#undef BY_DEPTH
#undef LAUNCH
}
