// Fused LayerNorm -> ReLU -> dropout for the inter-layer chain (gfx950).
//
//   mean_r = mean_f x[r,f]          var_r = mean_f (x[r,f]-mean_r)^2
//   rstd_r = 1/sqrt(var_r+eps)      xhat = (x-mean_r)*rstd_r
//   z = xhat*weight + bias          keep = uniform01(seed, r, f) >= p
//   y = relu(z) * keep * s          s = 1/(1-p)
//
// Forward reads x once and writes y once; backward reads dy and x and
// writes dx. Nothing else of size [N,F] exists: the dropout mask is the
// counter hash of (seed, row, feature), recomputed in backward, and the
// ReLU gate is recomputed from x, mean and rstd with the same fp32
// expression as forward.
//
// Layout: one wavefront per row, 4 waves per block (as quant_pack). Lane l
// owns VE consecutive features per chunk of 64*VE; the row is staged in
// registers (16 floats per lane, so F <= 1024). VE is picked host-side as
// the largest vector width that divides F and keeps every pointer aligned,
// so all row loads and stores are single vector instructions.
//
// dweight/dbias: a lane owns the same columns for every row it visits and
// accumulates them in registers over a grid-stride loop; a block's 4 waves
// are added in wave order through LDS into the block's own slab, and
// norm_act_reduce_kernel adds the slabs in a fixed order. No atomics, so
// the result is bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <cstdint>

#include "device_common.h"

#define NA_WAVES 4                       // waves (rows) per block
#define NA_MAXV 16                       // staged floats per lane
#define NA_MAX_FEATS (WAVE * NA_MAXV)    // register staging limit
#define NA_BWD_MAX_BLOCKS 1024           // backward grid cap (= slab count cap)
#define NA_RED_GROUPS 4                  // slab ranges summed in parallel

template <int NB> struct NaRaw;
template <> struct NaRaw<16> { using type = uint4; };
template <> struct NaRaw<8>  { using type = uint2; };
template <> struct NaRaw<4>  { using type = unsigned; };
template <> struct NaRaw<2>  { using type = ushort; };

// VE elements of T (one vector load) -> fp32
template <typename T, int VE>
__device__ __forceinline__ void load_vec(const T* __restrict__ p, float* out) {
    using Raw = typename NaRaw<VE * sizeof(T)>::type;
    const Raw r = *reinterpret_cast<const Raw*>(p);
    const T* v = reinterpret_cast<const T*>(&r);
#pragma unroll
    for (int k = 0; k < VE; ++k) out[k] = to_f32<T>(v[k]);
}

// fp32 -> VE elements of T (one vector store; bf16 rounded once, here)
template <typename T, int VE>
__device__ __forceinline__ void store_vec(T* __restrict__ p, const float* v) {
    using Raw = typename NaRaw<VE * sizeof(T)>::type;
    T o[VE];
#pragma unroll
    for (int k = 0; k < VE; ++k) {
        if constexpr (sizeof(T) == 2) o[k] = f32_to_bf16(v[k]);
        else o[k] = v[k];
    }
    *reinterpret_cast<Raw*>(p) = *reinterpret_cast<const Raw*>(o);
}

// VE fp32 parameters / partials; 16-byte pieces when VE >= 4
template <int VE>
__device__ __forceinline__ void load_f32(const float* __restrict__ p, float* out) {
    if constexpr (VE >= 4) {
#pragma unroll
        for (int j = 0; j < VE / 4; ++j) load_vec<float, 4>(p + 4 * j, out + 4 * j);
    } else {
        load_vec<float, VE>(p, out);
    }
}
template <int VE>
__device__ __forceinline__ void store_f32(float* __restrict__ p, const float* v) {
    if constexpr (VE >= 4) {
#pragma unroll
        for (int j = 0; j < VE / 4; ++j) store_vec<float, 4>(p + 4 * j, v + 4 * j);
    } else {
        store_vec<float, VE>(p, v);
    }
}

// butterfly: every lane ends with the same sum
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <typename T, int VE>
__global__ void __launch_bounds__(WAVE * NA_WAVES)
norm_act_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w,
                    const float* __restrict__ b, T* __restrict__ y,
                    float* __restrict__ mean_o, float* __restrict__ rstd_o,
                    int64_t N, int F, float eps, float p, float s,
                    uint32_t seed, bool masked) {
    constexpr int MAXCH = NA_MAXV / VE;
    const int64_t row = (int64_t)blockIdx.x * NA_WAVES + threadIdx.x / WAVE;
    if (row >= N) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const T* xr = x + row * F;

    float v[NA_MAXV];
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < MAXCH; ++c) {
        const int f0 = (lane + c * WAVE) * VE;
        if (f0 < F) {                    // VE | F: the whole vector is in range
            load_vec<T, VE>(xr + f0, &v[c * VE]);
#pragma unroll
            for (int k = 0; k < VE; ++k) sum += v[c * VE + k];
        } else {
#pragma unroll
            for (int k = 0; k < VE; ++k) v[c * VE + k] = 0.f;
        }
    }
    const float mean = wave_sum(sum) / (float)F;
    // second pass over the staged row: sum (x-mean)^2, never E[x^2]-mean^2
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < MAXCH; ++c) {
        const int f0 = (lane + c * WAVE) * VE;
        if (f0 < F) {
#pragma unroll
            for (int k = 0; k < VE; ++k) {
                const float d = v[c * VE + k] - mean;
                sq = fmaf(d, d, sq);
            }
        }
    }
    const float var = wave_sum(sq) / (float)F;
    const float rstd = 1.0f / sqrtf(var + eps);
    if (mean_o != nullptr && lane == 0) {
        mean_o[row] = mean;
        rstd_o[row] = rstd;
    }

    T* yr = y + row * F;
#pragma unroll
    for (int c = 0; c < MAXCH; ++c) {
        const int f0 = (lane + c * WAVE) * VE;
        if (f0 < F) {
            float wv[VE], bv[VE], o[VE];
            load_f32<VE>(w + f0, wv);
            load_f32<VE>(b + f0, bv);
#pragma unroll
            for (int k = 0; k < VE; ++k) {
                const float xhat = (v[c * VE + k] - mean) * rstd;
                const float z = fmaf(xhat, wv[k], bv[k]);
                bool on = z > 0.f;
                if (masked)
                    on = on && uniform01(seed, (uint32_t)row, (uint32_t)(f0 + k)) >= p;
                o[k] = on ? z * s : 0.f;
            }
            store_vec<T, VE>(yr + f0, o);
        }
    }
}

// ---------------------------------------------------------------------------
// backward: dx per row; dweight/dbias partials per block slab
//   slabs[block][0][F] = sum over the block's rows of dy*s*gate*xhat
//   slabs[block][1][F] = sum over the block's rows of dy*s*gate
// ---------------------------------------------------------------------------
template <typename T, int VE>
__global__ void __launch_bounds__(WAVE * NA_WAVES)
norm_act_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                    const float* __restrict__ mean, const float* __restrict__ rstd,
                    const float* __restrict__ w, const float* __restrict__ b,
                    T* __restrict__ dx, float* __restrict__ slabs,
                    int64_t N, int F, float p, float s, uint32_t seed,
                    bool masked) {
    constexpr int MAXCH = NA_MAXV / VE;
    extern __shared__ float lds[];       // [NA_WAVES-1][2][F]
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);

    float dw[NA_MAXV], db[NA_MAXV];
#pragma unroll
    for (int i = 0; i < NA_MAXV; ++i) { dw[i] = 0.f; db[i] = 0.f; }

    const int64_t stride = (int64_t)gridDim.x * NA_WAVES;
    for (int64_t row = (int64_t)blockIdx.x * NA_WAVES + wave; row < N; row += stride) {
        const float mu = mean[row], rs = rstd[row];
        const T* xr = x + row * F;
        const T* gr = dy + row * F;
        float a[NA_MAXV], xh[NA_MAXV];
        float sa = 0.f, sax = 0.f;
#pragma unroll
        for (int c = 0; c < MAXCH; ++c) {
            const int f0 = (lane + c * WAVE) * VE;
            if (f0 < F) {
                float xv[VE], gv[VE], wv[VE], bv[VE];
                load_vec<T, VE>(xr + f0, xv);
                load_vec<T, VE>(gr + f0, gv);
                load_f32<VE>(w + f0, wv);
                load_f32<VE>(b + f0, bv);
#pragma unroll
                for (int k = 0; k < VE; ++k) {
                    // the forward expression, so the gate matches forward's
                    const float xhat = (xv[k] - mu) * rs;
                    const float z = fmaf(xhat, wv[k], bv[k]);
                    bool on = z > 0.f;
                    if (masked)
                        on = on && uniform01(seed, (uint32_t)row, (uint32_t)(f0 + k)) >= p;
                    const float g = on ? gv[k] * s : 0.f;
                    dw[c * VE + k] = fmaf(g, xhat, dw[c * VE + k]);
                    db[c * VE + k] += g;
                    const float av = g * wv[k];
                    a[c * VE + k] = av;
                    xh[c * VE + k] = xhat;
                    sa += av;
                    sax = fmaf(av, xhat, sax);
                }
            } else {
#pragma unroll
                for (int k = 0; k < VE; ++k) { a[c * VE + k] = 0.f; xh[c * VE + k] = 0.f; }
            }
        }
        const float m1 = wave_sum(sa) / (float)F;
        const float m2 = wave_sum(sax) / (float)F;
        T* dr = dx + row * F;
#pragma unroll
        for (int c = 0; c < MAXCH; ++c) {
            const int f0 = (lane + c * WAVE) * VE;
            if (f0 < F) {
                float o[VE];
#pragma unroll
                for (int k = 0; k < VE; ++k)
                    o[k] = rs * (a[c * VE + k] - m1 - xh[c * VE + k] * m2);
                store_vec<T, VE>(dr + f0, o);
            }
        }
    }

    // waves 1..3 park their partials in LDS; wave 0 adds them in wave order
    if (wave > 0) {
        float* mine = lds + (int64_t)(wave - 1) * 2 * F;
#pragma unroll
        for (int c = 0; c < MAXCH; ++c) {
            const int f0 = (lane + c * WAVE) * VE;
            if (f0 < F) {
#pragma unroll
                for (int k = 0; k < VE; ++k) {
                    mine[f0 + k] = dw[c * VE + k];
                    mine[F + f0 + k] = db[c * VE + k];
                }
            }
        }
    }
    __syncthreads();
    if (wave == 0) {
        float* slab = slabs + (int64_t)blockIdx.x * 2 * F;
#pragma unroll
        for (int c = 0; c < MAXCH; ++c) {
            const int f0 = (lane + c * WAVE) * VE;
            if (f0 < F) {
#pragma unroll
                for (int q = 0; q < NA_WAVES - 1; ++q) {
                    const float* other = lds + (int64_t)q * 2 * F;
#pragma unroll
                    for (int k = 0; k < VE; ++k) {
                        dw[c * VE + k] += other[f0 + k];
                        db[c * VE + k] += other[F + f0 + k];
                    }
                }
                store_f32<VE>(slab + f0, &dw[c * VE]);
                store_f32<VE>(slab + F + f0, &db[c * VE]);
            }
        }
    }
}

// out[col] = sum of slabs[.][col], col in [0, 2F). The slabs are cut into
// NA_RED_GROUPS contiguous ranges; each is summed in slab order by one
// wave and the range sums are added in range order: a fixed association,
// bit-identical from run to run.
__global__ void __launch_bounds__(WAVE * NA_RED_GROUPS)
norm_act_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ out,
                       int n_slabs, int C) {
    __shared__ float part[NA_RED_GROUPS][WAVE];
    const int lane = threadIdx.x & (WAVE - 1);
    const int g = threadIdx.x / WAVE;
    const int col = blockIdx.x * WAVE + lane;
    const int per = (n_slabs + NA_RED_GROUPS - 1) / NA_RED_GROUPS;
    const int s0 = g * per, s1 = min(s0 + per, n_slabs);
    float acc = 0.f;
    if (col < C) {
#pragma unroll 8
        for (int sl = s0; sl < s1; ++sl) acc += slabs[(int64_t)sl * C + col];
    }
    part[g][lane] = acc;
    __syncthreads();
    if (g == 0 && col < C) {
        float t = part[0][lane];
#pragma unroll
        for (int q = 1; q < NA_RED_GROUPS; ++q) t += part[q][lane];
        out[col] = t;
    }
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
int64_t norm_act_bwd_max_blocks() { return NA_BWD_MAX_BLOCKS; }
int64_t norm_act_waves_per_block() { return NA_WAVES; }
int64_t norm_act_max_feats() { return NA_MAX_FEATS; }

namespace {

bool aligned_to(const void* p, size_t nbytes) {
    return reinterpret_cast<uintptr_t>(p) % nbytes == 0;
}

void check_rows(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on the GPU");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(t.dim() == 2, name, " must be [N, F]");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32 ||
                t.scalar_type() == torch::kBFloat16,
                name, " must be fp32 or bf16");
}

void check_param(const torch::Tensor& t, const char* name, int64_t F,
                 const torch::Tensor& like) {
    TORCH_CHECK(t.is_cuda() && t.device() == like.device(), name,
                " must be on x's device");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, name,
                " must be fp32 (got ", t.scalar_type(), ")");
    TORCH_CHECK(t.dim() == 1 && t.size(0) == F && t.is_contiguous(), name,
                " must be a contiguous [F] vector");
}

// largest vector width that divides F and keeps every pointer aligned
int pick_ve(bool bf16, int64_t F, std::initializer_list<const void*> rows,
            std::initializer_list<const void*> params) {
    const size_t esz = bf16 ? 2 : 4;
    int ve = bf16 ? 8 : 4;
    auto ok = [&](int v) {
        if (F % v) return false;
        for (const void* p : rows)
            if (p && !aligned_to(p, v * esz)) return false;
        for (const void* p : params)
            if (p && !aligned_to(p, std::min<size_t>(v * 4, 16))) return false;
        return true;
    };
    while (ve > 1 && !ok(ve)) ve >>= 1;
    return ve;
}

struct DropCfg { float p, s; bool masked; };

DropCfg drop_cfg(double p, bool training) {
    TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout p must be in [0, 1), got ", p);
    const float pf = (float)p;
    const bool masked = training && pf > 0.f;
    return {pf, masked ? 1.0f / (1.0f - pf) : 1.0f, masked};
}

hipStream_t cur_stream() {
    return at::cuda::getCurrentHIPStream().stream();
}

}  // namespace

// VE dispatch shared by both launchers: CALL(T, VE)
#define NA_DISPATCH(bf16, ve, CALL)                                       \
    do {                                                                  \
        if (bf16) {                                                       \
            switch (ve) {                                                 \
                case 8: CALL(ushort, 8); break;                           \
                case 4: CALL(ushort, 4); break;                           \
                case 2: CALL(ushort, 2); break;                           \
                default: CALL(ushort, 1); break;                          \
            }                                                             \
        } else {                                                          \
            switch (ve) {                                                 \
                case 4: CALL(float, 4); break;                            \
                case 2: CALL(float, 2); break;                            \
                default: CALL(float, 1); break;                           \
            }                                                             \
        }                                                                 \
    } while (0)

void norm_act_fwd(torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
                  double eps, double p, int64_t seed, bool training,
                  torch::Tensor y, torch::Tensor mean, torch::Tensor rstd) {
    check_rows(x, "x");
    check_rows(y, "y");
    const int64_t N = x.size(0), F = x.size(1);
    TORCH_CHECK(y.sizes() == x.sizes() && y.scalar_type() == x.scalar_type() &&
                y.device() == x.device(), "y must match x");
    TORCH_CHECK(F >= 1 && F <= NA_MAX_FEATS, "norm_act handles 1 <= F <= ",
                NA_MAX_FEATS, ", got F = ", F);
    check_param(weight, "weight", F, x);
    check_param(bias, "bias", F, x);
    const bool stats = mean.numel() > 0 || rstd.numel() > 0;
    if (stats) {
        for (const auto* t : {&mean, &rstd})
            TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32 &&
                        t->dim() == 1 && t->size(0) == N && t->is_contiguous(),
                        "mean/rstd must be contiguous fp32 [N] on the GPU");
    }
    const DropCfg d = drop_cfg(p, training);
    if (N == 0) return;
    const bool bf16 = x.scalar_type() == torch::kBFloat16;
    const int ve = pick_ve(bf16, F, {x.data_ptr(), y.data_ptr()},
                           {weight.data_ptr(), bias.data_ptr()});
    const bool have_stats = mean.numel() > 0;
    const dim3 block(WAVE * NA_WAVES), grid((N + NA_WAVES - 1) / NA_WAVES);
    auto st = cur_stream();
#define CALL(T, VE) norm_act_fwd_kernel<T, VE><<<grid, block, 0, st>>>(       \
        reinterpret_cast<const T*>(x.data_ptr()), weight.data_ptr<float>(),   \
        bias.data_ptr<float>(), reinterpret_cast<T*>(y.data_ptr()),           \
        have_stats ? mean.data_ptr<float>() : nullptr,                        \
        have_stats ? rstd.data_ptr<float>() : nullptr,                        \
        N, (int)F, (float)eps, d.p, d.s, (uint32_t)seed, d.masked)
    NA_DISPATCH(bf16, ve, CALL);
#undef CALL
}

torch::Tensor norm_act_bwd(torch::Tensor dy, torch::Tensor x,
                           torch::Tensor mean, torch::Tensor rstd,
                           torch::Tensor weight, torch::Tensor bias,
                           double p, int64_t seed, bool training,
                           torch::Tensor dx) {
    check_rows(x, "x");
    check_rows(dy, "dy");
    check_rows(dx, "dx");
    const int64_t N = x.size(0), F = x.size(1);
    for (const auto* t : {&dy, &dx})
        TORCH_CHECK(t->sizes() == x.sizes() && t->scalar_type() == x.scalar_type() &&
                    t->device() == x.device(), "dy/dx must match x");
    TORCH_CHECK(F >= 1 && F <= NA_MAX_FEATS, "norm_act handles 1 <= F <= ",
                NA_MAX_FEATS, ", got F = ", F);
    check_param(weight, "weight", F, x);
    check_param(bias, "bias", F, x);
    for (const auto* t : {&mean, &rstd})
        TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32 &&
                    t->dim() == 1 && t->size(0) == N && t->is_contiguous(),
                    "mean/rstd must be contiguous fp32 [N] on the GPU");
    const DropCfg d = drop_cfg(p, training);
    const auto f32 = x.options().dtype(torch::kFloat32);
    if (N == 0) return torch::zeros({2, F}, f32);
    const bool bf16 = x.scalar_type() == torch::kBFloat16;
    const int ve = pick_ve(bf16, F, {x.data_ptr(), dy.data_ptr(), dx.data_ptr()},
                           {weight.data_ptr(), bias.data_ptr()});
    // the grid depends on N alone, so the summation order does too
    const int64_t blocks = std::min<int64_t>((N + NA_WAVES - 1) / NA_WAVES,
                                             NA_BWD_MAX_BLOCKS);
    torch::Tensor slabs = torch::empty({blocks, 2, F}, f32);
    torch::Tensor out = torch::empty({2, F}, f32);
    const dim3 block(WAVE * NA_WAVES), grid(blocks);
    const size_t lds = (size_t)(NA_WAVES - 1) * 2 * F * sizeof(float);
    auto st = cur_stream();
#define CALL(T, VE) norm_act_bwd_kernel<T, VE><<<grid, block, lds, st>>>(     \
        reinterpret_cast<const T*>(dy.data_ptr()),                            \
        reinterpret_cast<const T*>(x.data_ptr()), mean.data_ptr<float>(),     \
        rstd.data_ptr<float>(), weight.data_ptr<float>(),                     \
        bias.data_ptr<float>(), reinterpret_cast<T*>(dx.data_ptr()),          \
        slabs.data_ptr<float>(), N, (int)F, d.p, d.s, (uint32_t)seed, d.masked)
    NA_DISPATCH(bf16, ve, CALL);
#undef CALL
    const int C = (int)(2 * F);
    norm_act_reduce_kernel<<<dim3((C + WAVE - 1) / WAVE),
                             dim3(WAVE * NA_RED_GROUPS), 0, st>>>(
        slabs.data_ptr<float>(), out.data_ptr<float>(), (int)blocks, C);
    return out;
}
