// Affine pre-alignment: the warp of a volume under a 3 x 4 matrix, the gradient of that warp with respect to the matrix, and the
// composition of the matrix with a displacement field.  theta[N][3][4] fp32 on the device, in the convention of
//     torch.nn.functional.affine_grid(theta, size, align_corners=True) + grid_sample(src, grid, 'bilinear', 'zeros', align_corners=True):
// normalised coordinates, rows and columns in (x, y, z) = (W, H, D) order, the frame of da_warp_fwd's `deform`.  The V x 3 grid never
// exists.  NDHWC: src / out / g [N][D][H][W][C], disp [N][D][H][W][3].
// The arithmetic runs in centred index space (as augment.hip's): with s_k = (size_k - 1) / 2 the sample point of output voxel i is
//     q_k = sum_j a_kj (i_j - s_j) + b_k,        a_kj = theta_kj s_k / s_j,   b_k = theta_k3 s_k + s_k,
// the twelve coefficients formed once per thread in double and q evaluated in double (i_j - s_j is exact, a half-integer), so the
// identity returns i itself and a whole-voxel shift whose theta entry is exact in fp32 returns i + t: tap weights (1, 0), bit-exact output.
// The taps are grid_sample's: floor(q), floor(q) + 1 with weights (1 - f, f), taps outside the volume dropped (zeros padding).  Weights and
// the eight-tap sums stay in double (the vector fp64 rate of this chip equals its fp32 rate and both kernels wait for memory): an output
// voxel is rounded once.
// d_theta (the hot path): with G_k(x) = sum_c g_c(x) d out_c / d q_k (x) (eight taps of src, the derivative of the trilinear weights),
//     d theta_kj = s_k / s_j sum_x G_k(x) (i_j - s_j),        d theta_k3 = s_k sum_x G_k(x),
// twelve sums per sample, reduced in the order of jacpen.hip / invcons.hip: per-thread doubles -> wave butterfly -> the four waves in order
// -> twelve partials per workgroup -> a finalize kernel adding each entry's partials in workgroup order.  No atomics: two runs are bit-identical.
// A sample coordinate that is NaN, infinite or >= 1e9 in magnitude samples nothing (output 0) and makes its sample's d_theta NaN.
#include "common.h"

namespace {

constexpr int kAfBlocks = 2048;    // partial rows per sample (multiple of 8: XCD-contiguous split), the launch of jacpen.hip / invcons.hip
constexpr int kAfTerms = 12;       // the matrix entries, row-major [3][4]

struct AfCoef { double a[3][3], b[3], s[3]; };

// the index-space coefficients of one sample (s: half extents (x, y, z))
__device__ __forceinline__ AfCoef af_coef(const float* __restrict__ th, int D, int H, int W) {
    AfCoef c;
    c.s[0] = (double)(W - 1) * 0.5; c.s[1] = (double)(H - 1) * 0.5; c.s[2] = (double)(D - 1) * 0.5;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c.a[k][j] = (double)th[k * 4 + j] * c.s[k] / c.s[j];
        c.b[k] = (double)th[k * 4 + 3] * c.s[k] + c.s[k];
    }
    return c;
}

struct AfTaps {
    int x0, y0, z0;
    double fx0, fx1, fy0, fy1, fz0, fz1;  // f?0 = q - floor(q), f?1 = 1 - f?0
    bool fin;
};

// sample point and taps of output voxel (w, h, d); c0 = (w - s_x, h - s_y, d - s_z).  A refused coordinate puts every tap out of range.
__device__ __forceinline__ AfTaps af_taps(const AfCoef& c, double cx, double cy, double cz) {
    const double qx = fma(c.a[0][0], cx, fma(c.a[0][1], cy, fma(c.a[0][2], cz, c.b[0])));
    const double qy = fma(c.a[1][0], cx, fma(c.a[1][1], cy, fma(c.a[1][2], cz, c.b[1])));
    const double qz = fma(c.a[2][0], cx, fma(c.a[2][1], cy, fma(c.a[2][2], cz, c.b[2])));
    AfTaps t;
    t.fin = fabs(qx) < 1e9 && fabs(qy) < 1e9 && fabs(qz) < 1e9;          // false for NaN
    const double ux = t.fin ? qx : -4.0, uy = t.fin ? qy : -4.0, uz = t.fin ? qz : -4.0;
    const double x0 = floor(ux), y0 = floor(uy), z0 = floor(uz);
    t.x0 = (int)x0; t.y0 = (int)y0; t.z0 = (int)z0;
    t.fx0 = ux - x0; t.fx1 = 1.0 - t.fx0;
    t.fy0 = uy - y0; t.fy1 = 1.0 - t.fy0;
    t.fz0 = uz - z0; t.fz1 = 1.0 - t.fz0;
    return t;
}

__global__ void __launch_bounds__(256)
affine_warp_fwd_kernel(const float* __restrict__ src, const float* __restrict__ theta, float* __restrict__ out, int D, int H, int W, int C) {
    const int n = blockIdx.y;
    const int V = D * H * W;
    const float* s = src + (long long)n * V * C;
    float* o = out + (long long)n * V * C;
    const AfCoef cf = af_coef(theta + n * kAfTerms, D, H, W);
    for (DaXcdLoop L = da_xcd_loop(V, 256); L.i < L.end; L.i += L.step) {
        const int v = (int)L.i;
        int d, h, w; da_vox3(v, H, W, d, h, w);
        const AfTaps t = af_taps(cf, (double)w - cf.s[0], (double)h - cf.s[1], (double)d - cf.s[2]);
        long long off[8];
        double wgt[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int cz = k >> 2, cy = (k >> 1) & 1, cx = k & 1;
            const int x = t.x0 + cx, y = t.y0 + cy, z = t.z0 + cz;
            const bool in = x >= 0 && x < W && y >= 0 && y < H && z >= 0 && z < D;
            off[k] = in ? (long long)((z * H + y) * W + x) * C : -1;
            wgt[k] = (cx ? t.fx0 : t.fx1) * (cy ? t.fy0 : t.fy1) * (cz ? t.fz0 : t.fz1);
        }
        float* ov = o + (long long)v * C;
        for (int c = 0; c < C; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (off[k] >= 0) acc = fma((double)s[off[k] + c], wgt[k], acc);
            ov[c] = (float)acc;
        }
    }
}

// 12 doubles per workgroup: sum_x G_k (i_j - s_j) (j < 3) and sum_x G_k (j = 3), the scales applied by the finalize kernel
__global__ void __launch_bounds__(256)
affine_warp_bwd_theta_kernel(const float* __restrict__ g, const float* __restrict__ src, const float* __restrict__ theta, int D, int H, int W,
                             int C, double* __restrict__ partial) {
    __shared__ double red[4][kAfTerms];
    const int n = blockIdx.y;
    const int V = D * H * W;
    const float* s = src + (long long)n * V * C;
    const float* gs = g + (long long)n * V * C;
    const AfCoef cf = af_coef(theta + n * kAfTerms, D, H, W);
    double acc[kAfTerms];
#pragma unroll
    for (int i = 0; i < kAfTerms; ++i) acc[i] = 0.0;
    for (DaXcdLoop L = da_xcd_loop(V, 256); L.i < L.end; L.i += L.step) {
        const int v = (int)L.i;
        int d, h, w; da_vox3(v, H, W, d, h, w);
        const double c0[3] = {(double)w - cf.s[0], (double)h - cf.s[1], (double)d - cf.s[2]};
        const AfTaps t = af_taps(cf, c0[0], c0[1], c0[2]);
        double G[3] = {0.0, 0.0, 0.0};
        const float* gv = gs + (long long)v * C;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int cz = k >> 2, cy = (k >> 1) & 1, cx = k & 1;
            const int x = t.x0 + cx, y = t.y0 + cy, z = t.z0 + cz;
            if (x >= 0 && x < W && y >= 0 && y < H && z >= 0 && z < D) {
                const double wx = cx ? t.fx0 : t.fx1, wy = cy ? t.fy0 : t.fy1, wz = cz ? t.fz0 : t.fz1;
                const float* sp = s + (long long)((z * H + y) * W + x) * C;
                double dot = 0.0;                                       // sum_c src[corner][c] g_c
                for (int c = 0; c < C; ++c) dot = fma((double)sp[c], (double)gv[c], dot);
                G[0] += (cx ? dot : -dot) * wy * wz;
                G[1] += (cy ? dot : -dot) * wx * wz;
                G[2] += (cz ? dot : -dot) * wx * wy;
            }
        }
        // a coordinate the warp refuses samples nothing and would add a finite 0: it makes the sample's gradient NaN instead
        if (!t.fin) { G[0] = (double)NAN; G[1] = (double)NAN; G[2] = (double)NAN; }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double Gk = G[k];
            acc[k * 4 + 0] += Gk * c0[0]; acc[k * 4 + 1] += Gk * c0[1]; acc[k * 4 + 2] += Gk * c0[2]; acc[k * 4 + 3] += Gk;
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < kAfTerms; ++i) {
        const double r = da_wave_sum(acc[i]);
        if (lane == 0) red[wid][i] = r;
    }
    __syncthreads();
    if (threadIdx.x < kAfTerms) {
        const int i = threadIdx.x;
        partial[((size_t)n * kAfTerms + i) * gridDim.x + blockIdx.x] = da_sum4(red, i);
    }
}

// one wave per (entry, sample), grid (12, N): lane l adds the entry's partials of workgroups l, l + 64, ... in that order, then the fixed
// butterfly.  The partials lie entry-major, [N][12][nblocks], so a wave reads consecutive doubles.  (One wave per sample walking the twelve
// entries in turn through rows of 12 doubles took 0.07 ms, more than the sweep itself at 80 x 96 x 80.)
__global__ void affine_theta_finalize_kernel(const double* __restrict__ partial, int nblocks, int D, int H, int W, float* __restrict__ d_theta) {
    const int i = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
    const double* p = partial + ((size_t)n * kAfTerms + i) * nblocks;
    double a = 0.0;
#pragma unroll 8
    for (int b = lane; b < nblocks; b += 64) a += p[b];
    a = da_wave_sum(a);
    const double s[3] = {(double)(W - 1) * 0.5, (double)(H - 1) * 0.5, (double)(D - 1) * 0.5};
    const int k = i >> 2, j = i & 3;
    if (lane == 0) d_theta[n * kAfTerms + i] = (float)(j < 3 ? a * s[k] / s[j] : a * s[k]);
}

// out(x) = theta (x_n + disp(x), 1) - x_n, written as (theta_lin - I) x_n + theta_lin disp + theta_3 in double: no cancellation against x_n
__global__ void __launch_bounds__(256)
affine_compose_kernel(const float* __restrict__ theta, const float* __restrict__ disp, float* __restrict__ out, int D, int H, int W) {
    const int n = blockIdx.y;
    const int V = D * H * W;
    const float* th = theta + n * kAfTerms;
    double m[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) m[k][j] = (double)th[k * 4 + j];
    const double sx = (double)(W - 1) * 0.5, sy = (double)(H - 1) * 0.5, sz = (double)(D - 1) * 0.5;
    const float* u = disp ? disp + (long long)n * V * 3 : nullptr;
    float* o = out + (long long)n * V * 3;
    for (DaXcdLoop L = da_xcd_loop(V, 256); L.i < L.end; L.i += L.step) {
        const int v = (int)L.i;
        int d, h, w; da_vox3(v, H, W, d, h, w);
        const double xn[3] = {((double)w - sx) / sx, ((double)h - sy) / sy, ((double)d - sz) / sz};
        double uu[3] = {0.0, 0.0, 0.0};
        if (u) { uu[0] = (double)u[(long long)v * 3]; uu[1] = (double)u[(long long)v * 3 + 1]; uu[2] = (double)u[(long long)v * 3 + 2]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double r = m[k][3];
#pragma unroll
            for (int j = 0; j < 3; ++j) r += (m[k][j] - (j == k ? 1.0 : 0.0)) * xn[j] + m[k][j] * uu[j];
            o[(long long)v * 3 + k] = (float)r;
        }
    }
}

int af_blocks(long long V) {
    long long g = da_cdiv(V, 256);
    if (g > kAfBlocks) g = kAfBlocks;
    if (g >= 8) g = g / 8 * 8;          // a multiple of 8 takes the XCD-contiguous split
    return (int)(g < 1 ? 1 : g);
}

bool af_args_ok(int N, int D, int H, int W) { return N >= 1 && N <= 65535 && D >= 2 && H >= 2 && W >= 2; }

}  // namespace

extern "C" int da_affine_warp_fwd(const float* src, const float* theta, float* out, int N, int D, int H, int W, int C, void* stream) {
    if (!src || !theta || !out || !af_args_ok(N, D, H, W) || C < 1) return DA_ERR_BADARG;
    const long long V = (long long)D * H * W;
    if (V >= 0x7FFFFFFFLL / 4) return DA_ERR_UNSUPPORTED;                  // 32-bit voxel offsets inside a sample
    hipLaunchKernelGGL(affine_warp_fwd_kernel, dim3(af_blocks(V), N), dim3(256), 0, da_stream(stream), src, theta, out, D, H, W, C);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t da_affine_warp_ws_bytes(int N, int D, int H, int W) {
    (void)D; (void)H; (void)W;
    return da_align((size_t)(N > 0 ? N : 1) * kAfBlocks * kAfTerms * sizeof(double));
}

extern "C" int da_affine_warp_bwd_theta(const float* g, const float* src, const float* theta, float* d_theta, int N, int D, int H, int W, int C,
                                        void* ws, size_t ws_bytes, void* stream) {
    if (!g || !src || !theta || !d_theta || !ws || !af_args_ok(N, D, H, W) || C < 1) return DA_ERR_BADARG;
    if (ws_bytes < da_affine_warp_ws_bytes(N, D, H, W)) return DA_ERR_WS_SMALL;
    const long long V = (long long)D * H * W;
    if (V >= 0x7FFFFFFFLL / 4) return DA_ERR_UNSUPPORTED;
    hipStream_t st = da_stream(stream);
    const int nblocks = af_blocks(V);
    hipLaunchKernelGGL(affine_warp_bwd_theta_kernel, dim3(nblocks, N), dim3(256), 0, st, g, src, theta, D, H, W, C, (double*)ws);
    DA_LAUNCH_CHECK();
    hipLaunchKernelGGL(affine_theta_finalize_kernel, dim3(kAfTerms, N), dim3(64), 0, st, (const double*)ws, nblocks, D, H, W, d_theta);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_affine_compose_disp(const float* theta, const float* disp, float* out, int N, int D, int H, int W, void* stream) {
    if (!theta || !out || !af_args_ok(N, D, H, W)) return DA_ERR_BADARG;
    const long long V = (long long)D * H * W;
    if (V >= 0x7FFFFFFFLL / 4) return DA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(affine_compose_kernel, dim3(af_blocks(V), N), dim3(256), 0, da_stream(stream), theta, disp, out, D, H, W);
    DA_LAUNCH_CHECK();
    return 0;
}
