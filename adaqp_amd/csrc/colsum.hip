// colsum: out[f] = sum_n g[n, f] for a contiguous [N, F] fp32 / bf16 matrix
// — the bias gradient of a linear layer — in ONE pass over g.
//
// Two stages, both in a fixed order (no float atomics), so two calls on the
// same input give the same bits:
//   1. colsum_partial_kernel: block b owns a contiguous row range. Its 256
//      threads form `rl` row lanes x `cols_t` column groups of VE features;
//      a thread adds rows rb + rlane, rb + rlane + rl, ... into fp32
//      registers (vector loads of VE * sizeof(T) bytes, eight in flight),
//      then the row lanes are added in lane order through LDS and the
//      block's [F] partial is stored.
//   2. colsum_final_kernel: 64 columns x 4 partial lanes per block; lane p
//      adds partials p, p + 4, ..., the four lanes are added in order and
//      the sum is rounded once to g's dtype.
// VE is the largest of {4,2,1} (fp32) / {8,4,2,1} (bf16) dividing F, so
// every row-base load is aligned (F = 47 or any odd F: scalar loads).
//
// Built for gfx950 only.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <cstdint>

#include "device_common.h"

namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_UNROLL = 8;          // row loads in flight per thread
constexpr int CS_MAX_BLOCKS = 1024;   // stage-1 partials
constexpr int CS_MIN_ROWS = 64;       // rows per stage-1 block, at least

template <int NB> struct CsVec;
template <> struct CsVec<16> { using type = uint4; };
template <> struct CsVec<8>  { using type = uint2; };
template <> struct CsVec<4>  { using type = unsigned; };
template <> struct CsVec<2>  { using type = ushort; };

template <typename T, int VE>
__global__ void __launch_bounds__(CS_THREADS)
colsum_partial_kernel(const T* __restrict__ g, float* __restrict__ part,
                      int64_t N, int64_t F, int64_t rows_per_block,
                      int cols_t, int rl) {
    using Raw = typename CsVec<VE * sizeof(T)>::type;
    __shared__ float red[CS_THREADS * VE];
    const int64_t CG = F / VE;                  // column groups per row
    const int rlane = threadIdx.x / cols_t;
    const int ct = threadIdx.x % cols_t;
    const int64_t rb = (int64_t)blockIdx.x * rows_per_block;
    const int64_t re = min(rb + rows_per_block, N);
    const int64_t step = (int64_t)rl * F;       // elements between my rows

    for (int64_t c0 = 0; c0 < CG; c0 += cols_t) {
        const int64_t c = c0 + ct;
        const bool valid = rlane < rl && c < CG;
        float acc[VE];
#pragma unroll
        for (int k = 0; k < VE; ++k) acc[k] = 0.f;
        if (valid) {
            int64_t row = rb + rlane;
            const T* p = g + row * F + c * VE;
            for (; row + (int64_t)(CS_UNROLL - 1) * rl < re;
                 row += (int64_t)CS_UNROLL * rl, p += CS_UNROLL * step) {
                Raw v[CS_UNROLL];
#pragma unroll
                for (int u = 0; u < CS_UNROLL; ++u)
                    v[u] = *reinterpret_cast<const Raw*>(p + u * step);
#pragma unroll
                for (int u = 0; u < CS_UNROLL; ++u) {
                    const T* e = reinterpret_cast<const T*>(&v[u]);
#pragma unroll
                    for (int k = 0; k < VE; ++k) acc[k] += to_f32<T>(e[k]);
                }
            }
            for (; row < re; row += rl, p += step) {
                const Raw v = *reinterpret_cast<const Raw*>(p);
                const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
                for (int k = 0; k < VE; ++k) acc[k] += to_f32<T>(e[k]);
            }
        }
        if (rl > 1) {
            if (valid) {
#pragma unroll
                for (int k = 0; k < VE; ++k)
                    red[(rlane * cols_t + ct) * VE + k] = acc[k];
            }
            __syncthreads();
            if (valid && rlane == 0) {
                for (int j = 1; j < rl; ++j) {
#pragma unroll
                    for (int k = 0; k < VE; ++k)
                        acc[k] += red[(j * cols_t + ct) * VE + k];
                }
            }
            __syncthreads();            // red is reused by the next c0
        }
        if (valid && rlane == 0) {
            float* o = part + (int64_t)blockIdx.x * F + c * VE;
#pragma unroll
            for (int k = 0; k < VE; ++k) o[k] = acc[k];
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(CS_THREADS)
colsum_final_kernel(const float* __restrict__ part, T* __restrict__ out,
                    int64_t B, int64_t F) {
    __shared__ float red[CS_THREADS];
    const int cl = threadIdx.x & 63, pl = threadIdx.x >> 6;
    const int64_t col = (int64_t)blockIdx.x * 64 + cl;
    float acc = 0.f;
    if (col < F)
        for (int64_t b = pl; b < B; b += CS_THREADS / 64)
            acc += part[b * F + col];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (pl == 0 && col < F) {
        float s = red[cl];
        s += red[64 + cl];
        s += red[128 + cl];
        s += red[192 + cl];
        if constexpr (sizeof(T) == 2) out[col] = f32_to_bf16(s);
        else out[col] = s;
    }
}

template <typename T, int VE>
void launch_partial(const torch::Tensor& g, torch::Tensor& part, int64_t N,
                    int64_t F, int64_t B, int64_t rows_per_block,
                    hipStream_t s) {
    const int64_t CG = F / VE;
    const int cols_t = (int)std::min<int64_t>(CG, CS_THREADS);
    const int rl = CS_THREADS / cols_t;
    colsum_partial_kernel<T, VE><<<dim3(B), dim3(CS_THREADS), 0, s>>>(
        reinterpret_cast<const T*>(g.data_ptr()), part.data_ptr<float>(),
        N, F, rows_per_block, cols_t, rl);
}

}  // namespace

torch::Tensor colsum(torch::Tensor g) {
    TORCH_CHECK(g.is_cuda(), "g must be on the GPU");
    TORCH_CHECK(g.dim() == 2 && g.is_contiguous(),
                "colsum expects a contiguous [N, F] matrix");
    const bool bf16 = g.scalar_type() == torch::kBFloat16;
    TORCH_CHECK(bf16 || g.scalar_type() == torch::kFloat32,
                "colsum expects fp32 or bf16");
    const int64_t N = g.size(0), F = g.size(1);
    TORCH_CHECK(F >= 1, "colsum needs at least one column");
    auto s = at::cuda::getCurrentHIPStream().stream();
    torch::Tensor out = torch::empty({F}, g.options());

    const int64_t B = N == 0 ? 0 : std::min<int64_t>(
        (N + CS_MIN_ROWS - 1) / CS_MIN_ROWS, CS_MAX_BLOCKS);
    torch::Tensor part = torch::empty({B, F}, g.options().dtype(torch::kFloat32));
    if (B) {
        const int64_t rows_per_block = (N + B - 1) / B;
        const int es = bf16 ? 2 : 4;
        int ve = bf16 ? 8 : 4;
        // widest load that divides F and keeps the base pointer aligned
        while (ve > 1 && (F % ve ||
               reinterpret_cast<uintptr_t>(g.data_ptr()) % (ve * es)))
            ve >>= 1;
        if (bf16) {
            switch (ve) {
                case 8: launch_partial<ushort, 8>(g, part, N, F, B, rows_per_block, s); break;
                case 4: launch_partial<ushort, 4>(g, part, N, F, B, rows_per_block, s); break;
                case 2: launch_partial<ushort, 2>(g, part, N, F, B, rows_per_block, s); break;
                default: launch_partial<ushort, 1>(g, part, N, F, B, rows_per_block, s); break;
            }
        } else {
            switch (ve) {
                case 4: launch_partial<float, 4>(g, part, N, F, B, rows_per_block, s); break;
                case 2: launch_partial<float, 2>(g, part, N, F, B, rows_per_block, s); break;
                default: launch_partial<float, 1>(g, part, N, F, B, rows_per_block, s); break;
            }
        }
    }
    const dim3 fg((F + 63) / 64), fb(CS_THREADS);
    if (bf16)
        colsum_final_kernel<ushort><<<fg, fb, 0, s>>>(
            part.data_ptr<float>(), reinterpret_cast<ushort*>(out.data_ptr()),
            B, F);
    else
        colsum_final_kernel<float><<<fg, fb, 0, s>>>(
            part.data_ptr<float>(), out.data_ptr<float>(), B, F);
    return out;
}
