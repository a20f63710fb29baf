// Masked training loss for the node-classification head (gfx950): softmax
// cross-entropy (single-label) and BCE-with-logits (multilabel) summed over
// the rows of z [N,C] whose mask bit is set, and the gradient with respect
// to z, without materialising z[mask].
//
//   CE :  m_r = max_c z[r,c]   s_r = sum_c exp(z[r,c]-m_r)
//         L = sum_{r: mask[r]} (m_r + log s_r - z[r, y_r])
//         dz[r,c] = g * (exp(z[r,c]-m_r)/s_r - [c == y_r])
//   BCE:  L = (1/C) sum_{r: mask[r]} sum_c (max(z,0) - z*y + log1p(exp(-|z|)))
//         dz[r,c] = (g/C) * (1/(1+exp(-z)) - y)
//         (a class with y == 0 contributes no z*y term, so z = -inf there
//          gives its limit 0 instead of inf*0)
//   rows with mask[r] == false are never read; their dz is +0.0.
//
// Layout: 256-thread blocks cut into sub-wavefronts of SW lanes, SW the
// power of two >= C clamped to [8,64] (as the SpMM picks its width from F).
// A sub-wavefront owns one row at a time, lane l the classes l, l+SW, ...,
// so a row is read with coalesced scalar loads whatever its alignment
// (rows are C elements apart and C is usually odd). It works on ML_UNROLL
// rows at once so that many row loads are in flight. Class l of each row
// stays in a register: C <= 64 is one pass over memory; the strided tail of
// a wider row is read again from cache for the exp sum.
//
// CE forward saves (m_r, s_r), 8 bytes per masked row, and backward forms
// exp(z-m_r)/s_r from them in one pass. Saving lse_r = m_r + log s_r alone
// would round the exponent z - lse_r to |lse_r|*2^-24, a relative softmax
// error of that size (1e-3 at a logit of 1e4). BCE saves nothing.
//
// Loss sum: no float atomics. Lane 0 of a sub-wavefront (CE) or every lane
// (BCE) adds its terms in row order, the block adds its sub-wavefronts in
// order through LDS into partial[block], and masked_loss_final_kernel adds
// the partials in a fixed order. The grid depends on N and C alone, so two
// calls on the same input give the same bits.
//
// Backward reads g from device memory and writes every element of dz,
// zeros included: no fill pass and no host read.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "device_common.h"

#define ML_THREADS 256                   // threads per block
#define ML_UNROLL 4                      // rows in flight per sub-wavefront
#define ML_MAX_BLOCKS 2048               // grid cap (= partial count cap)
#define ML_MIN_SW 8                      // narrowest sub-wavefront
#define ML_MAX_CLASSES 1024

namespace {

template <typename T>
__device__ __forceinline__ void put(T* p, float v) {
    if constexpr (sizeof(T) == 2) *p = f32_to_bf16(v);
    else *p = v;
}

// butterflies inside an aligned group of SW lanes: every lane of the group
// ends with the same value
template <int SW>
__device__ __forceinline__ float sub_sum(float v) {
#pragma unroll
    for (int o = SW / 2; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <int SW>
__device__ __forceinline__ float sub_max(float v) {
#pragma unroll
    for (int o = SW / 2; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// sub-wavefront partials -> partial[block], added in sub-wavefront order
template <int S>
__device__ __forceinline__ void block_partial(float acc, int sub, int lane,
                                              float* red,
                                              float* __restrict__ partial) {
    if (lane == 0) red[sub] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = red[0];
        for (int i = 1; i < S; ++i) t += red[i];
        partial[blockIdx.x] = t;
    }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <typename T, int SW>
__global__ void __launch_bounds__(ML_THREADS)
masked_ce_fwd_kernel(const T* __restrict__ z, const int64_t* __restrict__ labels,
                     const bool* __restrict__ mask, float2* __restrict__ stats,
                     float* __restrict__ partial, int64_t N, int C) {
    constexpr int S = ML_THREADS / SW, R = S * ML_UNROLL;
    __shared__ float red[S];
    const int sub = threadIdx.x / SW, lane = threadIdx.x % SW;
    float acc = 0.f;                     // lane 0: this sub-wavefront's rows
    for (int64_t t = blockIdx.x; t * R < N; t += gridDim.x) {
        const T* zr[ML_UNROLL];
        bool on[ML_UNROLL];
        float z0[ML_UNROLL], zy[ML_UNROLL], m[ML_UNROLL], s[ML_UNROLL];
        int64_t y[ML_UNROLL];
        // the label is fetched beside the mask bit, not after it, and the
        // label's logit beside the row: two dependent round trips per
        // batch of rows instead of four
#pragma unroll
        for (int u = 0; u < ML_UNROLL; ++u) {
            const int64_t row = t * R + u * S + sub;
            y[u] = row < N ? labels[row] : 0;
            on[u] = row < N && mask[row];
            zr[u] = z + (on[u] ? row : 0) * C;
        }
#pragma unroll
        for (int u = 0; u < ML_UNROLL; ++u) {
            z0[u] = (on[u] && lane < C) ? to_f32<T>(zr[u][lane]) : -INFINITY;
            // a label outside [0, C) is never used as an index
            zy[u] = (on[u] && y[u] >= 0 && y[u] < C) ? to_f32<T>(zr[u][y[u]])
                                                      : NAN;
            m[u] = z0[u];
        }
        for (int c = lane + SW; c < C; c += SW) {
#pragma unroll
            for (int u = 0; u < ML_UNROLL; ++u)
                if (on[u]) m[u] = fmaxf(m[u], to_f32<T>(zr[u][c]));
        }
#pragma unroll
        for (int u = 0; u < ML_UNROLL; ++u) {
            m[u] = sub_max<SW>(m[u]);
            s[u] = (on[u] && lane < C) ? expf(z0[u] - m[u]) : 0.f;
        }
        for (int c = lane + SW; c < C; c += SW) {
#pragma unroll
            for (int u = 0; u < ML_UNROLL; ++u)
                if (on[u]) s[u] += expf(to_f32<T>(zr[u][c]) - m[u]);
        }
#pragma unroll
        for (int u = 0; u < ML_UNROLL; ++u) s[u] = sub_sum<SW>(s[u]);
        if (lane == 0) {
#pragma unroll
            for (int u = 0; u < ML_UNROLL; ++u) {
                if (!on[u]) continue;
                const int64_t row = t * R + u * S + sub;
                stats[row] = make_float2(m[u], s[u]);
                acc += (m[u] + logf(s[u])) - zy[u];
            }
        }
    }
    block_partial<S>(acc, sub, lane, red, partial);
}

template <typename T, int SW>
__global__ void __launch_bounds__(ML_THREADS)
masked_bce_fwd_kernel(const T* __restrict__ z, const float* __restrict__ y,
                      const bool* __restrict__ mask,
                      float* __restrict__ partial, int64_t N, int C) {
    constexpr int S = ML_THREADS / SW, R = S * ML_UNROLL;
    __shared__ float red[S];
    const int sub = threadIdx.x / SW, lane = threadIdx.x % SW;
    float acc = 0.f;                     // this lane's classes, in row order
    for (int64_t t = blockIdx.x; t * R < N; t += gridDim.x) {
        int64_t base[ML_UNROLL];
        bool on[ML_UNROLL];
#pragma unroll
        for (int u = 0; u < ML_UNROLL; ++u) {
            const int64_t row = t * R + u * S + sub;
            on[u] = row < N && mask[row];
            base[u] = (on[u] ? row : 0) * C;
        }
        for (int c = lane; c < C; c += SW) {
            float zv[ML_UNROLL], yv[ML_UNROLL];
#pragma unroll
            for (int u = 0; u < ML_UNROLL; ++u) {
                zv[u] = on[u] ? to_f32<T>(z[base[u] + c]) : 0.f;
                yv[u] = on[u] ? y[base[u] + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < ML_UNROLL; ++u) {
                if (!on[u]) continue;
                const float zy = yv[u] == 0.f ? 0.f : zv[u] * yv[u];
                acc += fmaxf(zv[u], 0.f) - zy + log1pf(expf(-fabsf(zv[u])));
            }
        }
    }
    acc = sub_sum<SW>(acc);
    block_partial<S>(acc, sub, lane, red, partial);
}

// out = (sum of partial[0..n)) / div. Thread i adds partials i, i+256, ...
// and thread 0 adds the 256 sums in thread order.
__global__ void __launch_bounds__(ML_THREADS)
masked_loss_final_kernel(const float* __restrict__ partial, int n, float div,
                         float* __restrict__ out) {
    __shared__ float red[ML_THREADS];
    float a = 0.f;
    for (int i = threadIdx.x; i < n; i += ML_THREADS) a += partial[i];
    red[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = red[0];
        for (int i = 1; i < ML_THREADS; ++i) t += red[i];
        out[0] = t / div;
    }
}

// ---------------------------------------------------------------------------
// backward: every element of dz is written exactly once
// ---------------------------------------------------------------------------
template <typename T, int SW>
__global__ void __launch_bounds__(ML_THREADS)
masked_ce_bwd_kernel(const T* __restrict__ z, const int64_t* __restrict__ labels,
                     const bool* __restrict__ mask,
                     const float2* __restrict__ stats,
                     const float* __restrict__ g, T* __restrict__ dz,
                     int64_t N, int C) {
    constexpr int S = ML_THREADS / SW, R = S * ML_UNROLL;
    const int sub = threadIdx.x / SW, lane = threadIdx.x % SW;
    const float gv = g[0];
    for (int64_t t = blockIdx.x; t * R < N; t += gridDim.x) {
        int64_t base[ML_UNROLL];
        bool in[ML_UNROLL], on[ML_UNROLL];
        float m[ML_UNROLL], s[ML_UNROLL];
        int yc[ML_UNROLL];
#pragma unroll
        for (int u = 0; u < ML_UNROLL; ++u) {
            const int64_t row = t * R + u * S + sub;
            in[u] = row < N;
            on[u] = in[u] && mask[row];
            base[u] = (in[u] ? row : 0) * C;
            m[u] = 0.f; s[u] = 1.f; yc[u] = -1;
            if (on[u]) {
                const float2 st = stats[row];
                const int64_t y = labels[row];
                m[u] = st.x; s[u] = st.y;
                yc[u] = (y >= 0 && y < C) ? (int)y : -1;
            }
        }
        for (int c = lane; c < C; c += SW) {
            float zv[ML_UNROLL];
#pragma unroll
            for (int u = 0; u < ML_UNROLL; ++u)
                zv[u] = on[u] ? to_f32<T>(z[base[u] + c]) : 0.f;
#pragma unroll
            for (int u = 0; u < ML_UNROLL; ++u) {
                if (!in[u]) continue;
                float o = 0.f;
                if (on[u])
                    o = gv * (expf(zv[u] - m[u]) / s[u] - (c == yc[u] ? 1.f : 0.f));
                put<T>(dz + base[u] + c, o);
            }
        }
    }
}

template <typename T, int SW>
__global__ void __launch_bounds__(ML_THREADS)
masked_bce_bwd_kernel(const T* __restrict__ z, const float* __restrict__ y,
                      const bool* __restrict__ mask,
                      const float* __restrict__ g, T* __restrict__ dz,
                      int64_t N, int C) {
    constexpr int S = ML_THREADS / SW, R = S * ML_UNROLL;
    const int sub = threadIdx.x / SW, lane = threadIdx.x % SW;
    const float gc = g[0] / (float)C;
    for (int64_t t = blockIdx.x; t * R < N; t += gridDim.x) {
        int64_t base[ML_UNROLL];
        bool in[ML_UNROLL], on[ML_UNROLL];
#pragma unroll
        for (int u = 0; u < ML_UNROLL; ++u) {
            const int64_t row = t * R + u * S + sub;
            in[u] = row < N;
            on[u] = in[u] && mask[row];
            base[u] = (in[u] ? row : 0) * C;
        }
        for (int c = lane; c < C; c += SW) {
            float zv[ML_UNROLL], yv[ML_UNROLL];
#pragma unroll
            for (int u = 0; u < ML_UNROLL; ++u) {
                zv[u] = on[u] ? to_f32<T>(z[base[u] + c]) : 0.f;
                yv[u] = on[u] ? y[base[u] + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < ML_UNROLL; ++u) {
                if (!in[u]) continue;
                float o = 0.f;
                if (on[u]) o = gc * (1.f / (1.f + expf(-zv[u])) - yv[u]);
                put<T>(dz + base[u] + c, o);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int pick_sw(int64_t C) {
    int sw = ML_MIN_SW;
    while (sw < WAVE && sw < C) sw <<= 1;
    return sw;
}

int64_t grid_blocks(int64_t N, int sw) {
    const int64_t R = (int64_t)(ML_THREADS / sw) * ML_UNROLL;
    return std::min<int64_t>((N + R - 1) / R, ML_MAX_BLOCKS);
}

void check_inputs(const torch::Tensor& logits, const torch::Tensor& labels,
                  const torch::Tensor& mask, bool multilabel) {
    TORCH_CHECK(logits.is_cuda(), "logits must be on the GPU");
    TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(),
                "logits must be a contiguous [N, C] matrix");
    TORCH_CHECK(logits.scalar_type() == torch::kFloat32 ||
                logits.scalar_type() == torch::kBFloat16,
                "logits must be fp32 or bf16");
    const int64_t N = logits.size(0), C = logits.size(1);
    TORCH_CHECK(C >= 1 && C <= ML_MAX_CLASSES, "masked_loss handles 1 <= C <= ",
                ML_MAX_CLASSES, ", got C = ", C);
    TORCH_CHECK(mask.device() == logits.device() &&
                mask.scalar_type() == torch::kBool && mask.dim() == 1 &&
                mask.size(0) == N && mask.is_contiguous(),
                "mask must be a contiguous bool [N] on logits' device");
    TORCH_CHECK(labels.device() == logits.device() && labels.is_contiguous(),
                "labels must be contiguous on logits' device");
    if (multilabel) {
        TORCH_CHECK(labels.scalar_type() == torch::kFloat32 &&
                    labels.dim() == 2 && labels.size(0) == N &&
                    labels.size(1) == C,
                    "multilabel labels must be fp32 [N, C]");
    } else {
        TORCH_CHECK(labels.scalar_type() == torch::kInt64 &&
                    labels.dim() == 1 && labels.size(0) == N,
                    "single-label labels must be int64 [N]");
    }
}

hipStream_t cur_stream() {
    return at::cuda::getCurrentHIPStream().stream();
}

}  // namespace

// CALL(T, SW) for the element type and sub-wavefront width
#define ML_DISPATCH(bf16, sw, CALL)                                       \
    do {                                                                  \
        if (bf16) {                                                       \
            switch (sw) {                                                 \
                case 8: CALL(ushort, 8); break;                           \
                case 16: CALL(ushort, 16); break;                         \
                case 32: CALL(ushort, 32); break;                         \
                default: CALL(ushort, 64); break;                         \
            }                                                             \
        } else {                                                          \
            switch (sw) {                                                 \
                case 8: CALL(float, 8); break;                            \
                case 16: CALL(float, 16); break;                          \
                case 32: CALL(float, 32); break;                          \
                default: CALL(float, 64); break;                          \
            }                                                             \
        }                                                                 \
    } while (0)

int64_t masked_loss_max_blocks() { return ML_MAX_BLOCKS; }
int64_t masked_loss_max_classes() { return ML_MAX_CLASSES; }
// rows one block handles per trip of its row loop, for C classes
int64_t masked_loss_rows_per_block(int64_t C) {
    return (int64_t)(ML_THREADS / pick_sw(C)) * ML_UNROLL;
}

// -> {loss (0-dim fp32, the raw sum), stats ([N,2] fp32 (m_r, s_r) for the
// single-label loss, written for masked rows only; empty for multilabel)}
std::vector<torch::Tensor> masked_loss_fwd(torch::Tensor logits,
                                           torch::Tensor labels,
                                           torch::Tensor mask,
                                           bool multilabel) {
    check_inputs(logits, labels, mask, multilabel);
    const int64_t N = logits.size(0), C = logits.size(1);
    const auto f32 = logits.options().dtype(torch::kFloat32);
    torch::Tensor stats = torch::empty({multilabel ? 0 : N, 2}, f32);
    if (N == 0) return {torch::zeros({}, f32), stats};
    torch::Tensor loss = torch::empty({}, f32);
    const bool bf16 = logits.scalar_type() == torch::kBFloat16;
    const int sw = pick_sw(C);
    const int64_t blocks = grid_blocks(N, sw);
    torch::Tensor partial = torch::empty({blocks}, f32);
    const dim3 block(ML_THREADS), grid(blocks);
    auto st = cur_stream();
    if (multilabel) {
#define CALL(T, SW) masked_bce_fwd_kernel<T, SW><<<grid, block, 0, st>>>(     \
        reinterpret_cast<const T*>(logits.data_ptr()),                        \
        labels.data_ptr<float>(), mask.data_ptr<bool>(),                      \
        partial.data_ptr<float>(), N, (int)C)
        ML_DISPATCH(bf16, sw, CALL);
#undef CALL
    } else {
#define CALL(T, SW) masked_ce_fwd_kernel<T, SW><<<grid, block, 0, st>>>(      \
        reinterpret_cast<const T*>(logits.data_ptr()),                        \
        labels.data_ptr<int64_t>(), mask.data_ptr<bool>(),                    \
        reinterpret_cast<float2*>(stats.data_ptr()),                          \
        partial.data_ptr<float>(), N, (int)C)
        ML_DISPATCH(bf16, sw, CALL);
#undef CALL
    }
    masked_loss_final_kernel<<<dim3(1), block, 0, st>>>(
        partial.data_ptr<float>(), (int)blocks, multilabel ? (float)C : 1.0f,
        loss.data_ptr<float>());
    return {loss, stats};
}

// dz [N,C] in logits' dtype; g is the upstream gradient, one fp32 on the GPU
torch::Tensor masked_loss_bwd(torch::Tensor logits, torch::Tensor labels,
                              torch::Tensor mask, torch::Tensor stats,
                              torch::Tensor g, bool multilabel) {
    check_inputs(logits, labels, mask, multilabel);
    const int64_t N = logits.size(0), C = logits.size(1);
    TORCH_CHECK(g.device() == logits.device() &&
                g.scalar_type() == torch::kFloat32 && g.numel() == 1,
                "g must be one fp32 value on logits' device");
    if (!multilabel) {
        TORCH_CHECK(stats.device() == logits.device() &&
                    stats.scalar_type() == torch::kFloat32 &&
                    stats.dim() == 2 && stats.size(0) == N &&
                    stats.size(1) == 2 && stats.is_contiguous(),
                    "stats must be the contiguous fp32 [N, 2] of the forward");
    }
    torch::Tensor dz = torch::empty_like(logits);
    if (N == 0) return dz;
    const bool bf16 = logits.scalar_type() == torch::kBFloat16;
    const int sw = pick_sw(C);
    const dim3 block(ML_THREADS), grid(grid_blocks(N, sw));
    auto st = cur_stream();
    if (multilabel) {
#define CALL(T, SW) masked_bce_bwd_kernel<T, SW><<<grid, block, 0, st>>>(     \
        reinterpret_cast<const T*>(logits.data_ptr()),                        \
        labels.data_ptr<float>(), mask.data_ptr<bool>(),                      \
        g.data_ptr<float>(), reinterpret_cast<T*>(dz.data_ptr()), N, (int)C)
        ML_DISPATCH(bf16, sw, CALL);
#undef CALL
    } else {
#define CALL(T, SW) masked_ce_bwd_kernel<T, SW><<<grid, block, 0, st>>>(      \
        reinterpret_cast<const T*>(logits.data_ptr()),                        \
        labels.data_ptr<int64_t>(), mask.data_ptr<bool>(),                    \
        reinterpret_cast<const float2*>(stats.data_ptr()),                    \
        g.data_ptr<float>(), reinterpret_cast<T*>(dz.data_ptr()), N, (int)C)
        ML_DISPATCH(bf16, sw, CALL);
#undef CALL
    }
    return dz;
}
