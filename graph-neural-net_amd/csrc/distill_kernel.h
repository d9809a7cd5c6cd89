// distill_kernel.h -- a teacher's outputs blended into a student's resident expected rows (distill.hip: gnn_mlp_distill_range,
// gnn_mlp_group_distill_range), and the gather that makes a lone net's padded output rows dense (gnn_mlp_propagate_set_range).
//   blend_targets_kernel   y'[r][c] = keep * y[r][c] + (1 - keep) * t[r][c] for c < d_out, in f32, each product and the sum
//                          rounded on its own (no contraction into an fma): t dense [rows][d_out], y rows of stride ldy.  The two
//                          ends are exact whatever the values: keep == 0 stores t's bits, keep == 1 is never launched.  Columns
//                          d_out .. ldy - 1 (the padding) are neither read nor written.
//   gather_rows_dense_kernel   dst[r][c] = src[r * ld + c] for c < d: the padded rows of `prob` as dense rows.
// Both are memory bound and element-wise: VEC4 moves 16 bytes per lane (d_out a multiple of 4, both bases 16-byte aligned,
// stride a multiple of 4 -- every shipped 10-class net misses it, d_out = 20 / 16 / 4 take it), the scalar form one float.
// Grid-stride loops over 64-bit indices; no atomics, no LDS, nothing but plain loads and stores.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gnn {

struct BlendParams {
    const float *t;   // teacher rows of the block, dense [rows][d_out]
    float *y; int ldy; // the student's expected rows of the block
    int d_out; long long rows;
    float keep;
};

__device__ inline float blend_value(float keep, float omk, float y, float t) {
#pragma clang fp contract(off) // (the build contracts a * b + c into an fma by default: one rounding less than the formula states)
    const float a = keep * y;
    const float b = omk * t;
    return a + b;
}

template <bool VEC4>
static __global__ __launch_bounds__(256) void blend_targets_kernel(BlendParams p) {
    const float keep = p.keep, omk = 1.f - p.keep;
    const bool copy = keep == 0.f; // (uniform)
    if constexpr (VEC4) {
        const int q = p.d_out / 4;
        const long long total = p.rows * q;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
            const long long r = i / q;
            const int c = (int)(i - r * q);
            const float4 t = reinterpret_cast<const float4 *>(p.t)[i];
            float4 *const dst = reinterpret_cast<float4 *>(p.y + (size_t)r * p.ldy) + c;
            if (copy) { *dst = t; continue; }
            const float4 y = *dst;
            *dst = make_float4(blend_value(keep, omk, y.x, t.x), blend_value(keep, omk, y.y, t.y),
                               blend_value(keep, omk, y.z, t.z), blend_value(keep, omk, y.w, t.w));
        }
    } else {
        const long long total = p.rows * p.d_out;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
            const long long r = i / p.d_out;
            const int c = (int)(i - r * p.d_out);
            float *const dst = p.y + (size_t)r * p.ldy + c;
            const float t = p.t[i];
            *dst = copy ? t : blend_value(keep, omk, *dst, t);
        }
    }
}

template <bool VEC4>
static __global__ __launch_bounds__(256) void gather_rows_dense_kernel(const float *__restrict__ src, int ld, int d, long long rows,
                                                                       float *__restrict__ dst) {
    if constexpr (VEC4) {
        const int q = d / 4;
        const long long total = rows * q;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
            const long long r = i / q;
            const int c = (int)(i - r * q);
            reinterpret_cast<float4 *>(dst)[i] = reinterpret_cast<const float4 *>(src + (size_t)r * ld)[c];
        }
    } else {
        const long long total = rows * d;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
            const long long r = i / d;
            const int c = (int)(i - r * d);
            dst[i] = src[(size_t)r * ld + c];
        }
    }
}

#ifndef __HIPCC_RTC__
inline bool distill_vec4_ok(const void *a, const void *b, int d, int ld) {
    return d % 4 == 0 && ld % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0;
}
inline unsigned distill_grid(long long n) {
    long long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > 2048 ? 2048 : b);
}
// one launch over the block's rows (keep == 1 changes nothing: the caller launches nothing)
inline hipError_t launch_blend(const BlendParams &p, hipStream_t stream) {
    if (distill_vec4_ok(p.t, p.y, p.d_out, p.ldy))
        hipLaunchKernelGGL(blend_targets_kernel<true>, dim3(distill_grid(p.rows * (p.d_out / 4))), dim3(256), 0, stream, p);
    else
        hipLaunchKernelGGL(blend_targets_kernel<false>, dim3(distill_grid(p.rows * p.d_out)), dim3(256), 0, stream, p);
    return hipGetLastError();
}
inline hipError_t launch_gather_dense(const float *src, int ld, int d, long long rows, float *dst, hipStream_t stream) {
    if (distill_vec4_ok(src, dst, d, ld))
        hipLaunchKernelGGL(gather_rows_dense_kernel<true>, dim3(distill_grid(rows * (d / 4))), dim3(256), 0, stream, src, ld, d, rows, dst);
    else
        hipLaunchKernelGGL(gather_rows_dense_kernel<false>, dim3(distill_grid(rows * d)), dim3(256), 0, stream, src, ld, d, rows, dst);
    return hipGetLastError();
}
#endif

} // namespace gnn
