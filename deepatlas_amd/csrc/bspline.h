// Uniform B-spline support and contraction over a control grid staged in LDS, orders 1..3 (ITK BSplineTransformInitializer geometry:
// DESIGN.md 4.18).  One definition for the displacement of da_spatial_resample (augment.hip) and the bias field of da_intensity_augment
// (intensity.hip).
#pragma once
#include <hip/hip_runtime.h>

// B-spline support along one axis at output index i of an axis of `size` voxels (domain: voxel centres [0, size - 1], M mesh cells).
// Grid coordinate g = i M / (size - 1) + (O - 1) / 2; start = floor(g - (O - 1) / 2) = floor(i M / (size - 1)), clamped to M - 1 (ITK's
// upper-face nudge); u = g - (O - 1) / 2 - start in [0, 1], exact numerator, one rounding.  wt[k] = B_O(g - start - k).
template <int O>
__device__ __forceinline__ int bspline_axis(int i, int M, int size, float (&wt)[O + 1]) {
    const int num = i * M;
    int s = num / (size - 1);
    if (s > M - 1) s = M - 1;
    const float u = (float)(num - s * (size - 1)) / (float)(size - 1);
    const float v = 1.f - u;
    if constexpr (O == 1) {
        wt[0] = v; wt[1] = u;
    } else if constexpr (O == 2) {
        wt[0] = 0.5f * v * v; wt[1] = 0.75f - (u - 0.5f) * (u - 0.5f); wt[2] = 0.5f * u * u;
    } else {
        const float u2 = u * u, u3 = u2 * u;
        wt[0] = v * v * v * (1.f / 6.f);
        wt[1] = (3.f * u3 - 6.f * u2 + 4.f) * (1.f / 6.f);
        wt[2] = (-3.f * u3 + 3.f * u2 + 3.f * u + 1.f) * (1.f / 6.f);
        wt[3] = u3 * (1.f / 6.f);
    }
    return s;
}

// one scalar component: sum over the (O+1)^3 support of wz wy wx * coef[sz + a][sy + b][sx + k] (coef: one component's grid in LDS)
template <int O>
__device__ __forceinline__ float bspline_contract(const float* cg, int gx, int gy, int sx, int sy, int sz,
                                                  const float (&wx)[O + 1], const float (&wy)[O + 1], const float (&wz)[O + 1]) {
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a <= O; ++a) {
        float accy = 0.f;
#pragma unroll
        for (int b = 0; b <= O; ++b) {
            const float* row = cg + ((sz + a) * gy + sy + b) * gx + sx;
            float accx = 0.f;
#pragma unroll
            for (int k = 0; k <= O; ++k) accx = fmaf(wx[k], row[k], accx);
            accy = fmaf(wy[b], accx, accy);
        }
        acc = fmaf(wz[a], accy, acc);
    }
    return acc;
}
