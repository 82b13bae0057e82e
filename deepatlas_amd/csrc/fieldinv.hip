// Inverse of a displacement field and transport of points through it.  The net's field u is the pull-back map x -> x + u(x) (fixed frame ->
// moving frame); carrying a moving-frame point q into the fixed frame means solving x + u(x) = q, and the inverse field v = (id + u)^-1 - id is
// that solution at the grid nodes.  Both are the fixed point of
//     v_0 = 0,   v_{k+1} = -B[u](g + v_k)
// with g the point's normalised coordinate (da_id_coord for a grid node) and B the trilinear sample with BORDER padding,
// F.grid_sample(u, p, 'bilinear', 'border', align_corners=True): the unnormalised coordinate is clamped to [0, size - 1] before the taps are
// formed, a tap of index `size` has weight 0 and is not read.  (With the warp's zeros the field drops from u to 0 within a voxel of every face
// the map leaves and the iteration 2-cycles there.)  The iteration at one element reads only u and its own v_k: all its updates run in
// registers in one launch; an element stops after the first update d_k = |s (v_{k+1} - v_k)| <= tol_vox (Euclidean norm in voxels,
// s_c = (size_c - 1) / 2) or after max_iters updates.
// NDHWC: disp[N][D][H][W][3], channel order (x, y, z) = (W, H, D) axis, normalised units.  points / out [N][P][3] in voxel index coordinates.
// fi_solve is the one device function behind both entries: the dense kernel stores v, the points kernel q + s v (inverse) or, after a single
// update, p - s v = p + s B[u](p) (forward); at a grid node the two agree bit for bit (the iteration's arithmetic is compiled without FMA
// contraction, so that both kernels round every operation alike).
// The update loop is wave-uniform, `while (__any(!done) && k < max_iters)` with finished lanes predicated: a wave leaves when its slowest lane
// has converged and no lane returns before the wave reductions of the statistics.
// Statistics per sample, four doubles in the reduction order of invcons.hip (per-thread -> wave butterfly -> the four waves in order -> one
// partial row per workgroup -> a finalize kernel adding the rows in index order; no atomics, bit-identical from run to run): the largest final
// update in voxels (infinite if an element is non-finite), the number of elements not converged (final update > tol_vox, or non-finite), the
// number of updates performed, the number of elements whose last sample point leaves [0, size - 1] on some axis (extrapolated) or is not finite.
#include "common.h"

namespace {

constexpr int kFiBlocks = 2048;    // partial rows per sample (multiple of 8: XCD-contiguous split), the launch of invcons.hip
constexpr int kFiStats = 4;

using FiDims = DaFieldDims;      // common.h: B[u] is shared with the native-grid warp (regapply.hip)

struct FiResult {
    float vx, vy, vz;      // v after the last update, normalised units; NaN where `bad`
    float last;            // the last update's size in voxels
    int iters;             // updates performed
    bool bad;              // a coordinate failed da_is_finite_coord (no memory was read for it), or the update itself is not finite
    bool outside;          // the last sample point left [0, size - 1] on some axis
};

// the updates of one element whose normalised base coordinate is (g0x, g0y, g0z); a lane that is not `live` takes part in the loop condition only
__device__ __forceinline__ FiResult fi_solve(const float* __restrict__ u, const FiDims& m, float g0x, float g0y, float g0z, bool live,
                                             int max_iters, float tol_vox) {
#pragma clang fp contract(off)
    FiResult r;
    r.vx = 0.f; r.vy = 0.f; r.vz = 0.f; r.last = 0.f; r.iters = 0; r.bad = false; r.outside = false;
    bool done = !live;
    int k = 0;
    while (__any(!done) && k < max_iters) {
        if (!done) {
            const float gx = g0x + r.vx, gy = g0y + r.vy, gz = g0z + r.vz;
            if (!da_is_finite_coord(gx, gy, gz)) { r.bad = true; done = true; }
            else {
                float bx, by, bz;
                r.outside = da_field_sample_border(u, m, gx, gy, gz, bx, by, bz);
                const float nx = 0.f - bx, ny = 0.f - by, nz = 0.f - bz;           // (0 - b: a zero field gives +0)
                const float ex = m.sx * (nx - r.vx), ey = m.sy * (ny - r.vy), ez = m.sz * (nz - r.vz);
                r.last = sqrtf(ex * ex + ey * ey + ez * ez);
                r.vx = nx; r.vy = ny; r.vz = nz;
                ++r.iters;
                done = r.last <= tol_vox;                                        // (false for a NaN update: the next coordinate is refused)
            }
        }
        ++k;
    }
    if (live && !(fabsf(r.last) < INFINITY)) r.bad = true;                       // the last permitted update sampled a non-finite value
    if (r.bad) { r.vx = NAN; r.vy = NAN; r.vz = NAN; r.outside = true; }
    return r;
}

// q + s v (inverse) or q - s v (forward) with the product and the sum rounded separately: the host can restate it from the dense inverse
__device__ __forceinline__ float fi_point_out(float q, float s, float v, int inverse) {
#pragma clang fp contract(off)
    const float sv = s * v;
    return inverse ? q + sv : q - sv;
}

struct FiAcc { double mx, unconv, iters, out; };

__device__ __forceinline__ void fi_count(FiAcc& a, const FiResult& r, float tol_vox) {
    if (r.bad) { a.mx = INFINITY; a.unconv += 1.0; }
    else { a.mx = fmax(a.mx, (double)r.last); if (r.last > tol_vox) a.unconv += 1.0; }
    a.iters += (double)r.iters;
    if (r.outside) a.out += 1.0;
}

// every lane of the workgroup calls this; row: the workgroup's partial row (may be NULL)
__device__ __forceinline__ void fi_block_reduce(FiAcc a, double (*red)[kFiStats], double* __restrict__ row) {
    a.mx = da_wave_max(a.mx); a.unconv = da_wave_sum(a.unconv); a.iters = da_wave_sum(a.iters); a.out = da_wave_sum(a.out);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[wid][0] = a.mx; red[wid][1] = a.unconv; red[wid][2] = a.iters; red[wid][3] = a.out; }
    __syncthreads();
    if (threadIdx.x == 0 && row) {
        row[0] = da_max4(red, 0);
        row[1] = da_sum4(red, 1);
        row[2] = da_sum4(red, 2);
        row[3] = da_sum4(red, 3);
    }
}

// one lane per voxel, every update in registers, one 12-byte store per voxel.  The loop over the voxels is wave-uniform as well: a wave's 64
// voxels are consecutive and its lanes past the end of the range are not `live`.
__global__ void __launch_bounds__(256)
fieldinv_dense_kernel(const float* __restrict__ disp, float* __restrict__ out, unsigned char* __restrict__ iters, int D, int H, int W,
                      int max_iters, float tol_vox, double* __restrict__ partial) {
    __shared__ double red[4][kFiStats];
    const int n = blockIdx.y;
    const int V = D * H * W;
    const float* u = disp + (long long)n * V * 3;
    const FiDims m = da_field_dims(D, H, W);
    const int lane = threadIdx.x & 63;
    FiAcc acc = {0.0, 0.0, 0.0, 0.0};
    for (DaXcdLoop L = da_xcd_loop(V, 256); L.i - lane < L.end; L.i += L.step) {
        const bool live = L.i < L.end;
        const int v = live ? (int)L.i : 0;
        int d, h, w; da_vox3(v, H, W, d, h, w);
        const FiResult r = fi_solve(u, m, da_id_coord(w, W), da_id_coord(h, H), da_id_coord(d, D), live, max_iters, tol_vox);
        if (live) {
            float* o = out + ((long long)n * V + v) * 3;
            o[0] = r.vx; o[1] = r.vy; o[2] = r.vz;
            if (iters) iters[(long long)n * V + v] = (unsigned char)r.iters;
            fi_count(acc, r, tol_vox);
        }
    }
    fi_block_reduce(acc, red, partial ? partial + ((size_t)n * gridDim.x + blockIdx.x) * kFiStats : nullptr);
}

// one lane per point: sample n = blockIdx.y, a grid-stride over its P points (N P lanes' worth of work over the grid), so that the
// statistics stay per sample in a fixed order.  The normalised coordinate of a point is da_id_coord at a real index.
// inverse: x = q + s v.  forward: one update from v = 0 gives v = -B[u](p), and p + s B[u](p) = p - s v.  The products and sums of the output
// are not contracted, so that the host can restate them from the dense inverse.
__global__ void __launch_bounds__(256)
fieldinv_points_kernel(const float* __restrict__ disp, const float* __restrict__ points, float* __restrict__ out, int D, int H, int W, int P,
                       int inverse, int max_iters, float tol_vox, double* __restrict__ partial) {
    __shared__ double red[4][kFiStats];
    const int n = blockIdx.y;
    const int V = D * H * W;
    const float* u = disp + (long long)n * V * 3;
    const FiDims m = da_field_dims(D, H, W);
    const int lane = threadIdx.x & 63;
    const long long step = (long long)gridDim.x * 256;
    FiAcc acc = {0.0, 0.0, 0.0, 0.0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i - lane < P; i += step) {
        const bool live = i < P;
        const float* q = points + ((long long)n * P + (live ? i : 0)) * 3;
        const float qx = q[0], qy = q[1], qz = q[2];
        const float gx = da_id_coord(qx, W), gy = da_id_coord(qy, H), gz = da_id_coord(qz, D);
        const FiResult r = fi_solve(u, m, gx, gy, gz, live, max_iters, tol_vox);
        if (live) {
            float* o = out + ((long long)n * P + i) * 3;
            o[0] = fi_point_out(qx, m.sx, r.vx, inverse); o[1] = fi_point_out(qy, m.sy, r.vy, inverse); o[2] = fi_point_out(qz, m.sz, r.vz, inverse);
            fi_count(acc, r, tol_vox);
        }
    }
    fi_block_reduce(acc, red, partial ? partial + ((size_t)n * gridDim.x + blockIdx.x) * kFiStats : nullptr);
}

// one wave: sample by sample, lane l takes rows l, l + 64, ... of the sample's nblocks partial rows in that order, then the fixed butterfly
__global__ void fieldinv_finalize_kernel(const double* __restrict__ partial, int N, int nblocks, double* __restrict__ stats) {
    const int lane = threadIdx.x;
    for (int n = 0; n < N; ++n) {
        const double* p = partial + (size_t)n * nblocks * kFiStats;
        double mx = 0.0, un = 0.0, it = 0.0, out = 0.0;
        for (int b = lane; b < nblocks; b += 64) {
            mx = fmax(mx, p[(size_t)b * kFiStats]); un += p[(size_t)b * kFiStats + 1];
            it += p[(size_t)b * kFiStats + 2]; out += p[(size_t)b * kFiStats + 3];
        }
        mx = da_wave_max(mx); un = da_wave_sum(un); it = da_wave_sum(it); out = da_wave_sum(out);
        if (lane == 0) { double* o = stats + (size_t)n * kFiStats; o[0] = mx; o[1] = un; o[2] = it; o[3] = out; }
    }
}

int fi_blocks(long long items) {
    long long g = da_cdiv(items, 256);
    if (g > kFiBlocks) g = kFiBlocks;
    if (g >= 8) g = g / 8 * 8;          // a multiple of 8 takes the XCD-contiguous split
    return (int)(g < 1 ? 1 : g);
}

bool fi_args_ok(int N, int D, int H, int W, int max_iters, float tol_vox) {
    return N >= 1 && N <= 65535 && D >= 2 && H >= 2 && W >= 2 && max_iters >= 1 && max_iters <= 255 && tol_vox >= 0.f;
}

}  // namespace

extern "C" size_t da_field_invert_ws_bytes(int N, int D, int H, int W) {
    (void)D; (void)H; (void)W;
    return da_align((size_t)(N > 0 ? N : 1) * kFiBlocks * kFiStats * sizeof(double));
}

extern "C" size_t da_field_points_ws_bytes(int N, int P) {
    (void)P;
    return da_field_invert_ws_bytes(N, 0, 0, 0);          // the same per-sample statistics partials
}

extern "C" int da_field_invert(const float* disp, float* out, unsigned char* iters, int N, int D, int H, int W, int max_iters, float tol_vox,
                               double* stats, void* ws, size_t ws_bytes, void* stream) {
    if (!disp || !out || !fi_args_ok(N, D, H, W, max_iters, tol_vox)) return DA_ERR_BADARG;
    if (stats && !ws) return DA_ERR_BADARG;
    if (stats && ws_bytes < da_field_invert_ws_bytes(N, D, H, W)) return DA_ERR_WS_SMALL;
    const long long V = (long long)D * H * W;
    if (V >= 0x7FFFFFFFLL / 4) return DA_ERR_UNSUPPORTED;                  // 32-bit voxel and element offsets inside a sample
    hipStream_t st = da_stream(stream);
    const int nblocks = fi_blocks(V);
    hipLaunchKernelGGL(fieldinv_dense_kernel, dim3(nblocks, N), dim3(256), 0, st, disp, out, iters, D, H, W, max_iters, tol_vox,
                       stats ? (double*)ws : (double*)nullptr);
    DA_LAUNCH_CHECK();
    if (stats) {
        hipLaunchKernelGGL(fieldinv_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, N, nblocks, stats);
        DA_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int da_field_transport_points(const float* disp, const float* points, float* out, int N, int D, int H, int W, int P, int inverse,
                                         int max_iters, float tol_vox, double* stats, void* ws, size_t ws_bytes, void* stream) {
    if (!disp || !points || !out || P < 1 || !fi_args_ok(N, D, H, W, max_iters, tol_vox)) return DA_ERR_BADARG;
    if (stats && !ws) return DA_ERR_BADARG;
    if (stats && ws_bytes < da_field_points_ws_bytes(N, P)) return DA_ERR_WS_SMALL;
    const long long V = (long long)D * H * W;
    if (V >= 0x7FFFFFFFLL / 4) return DA_ERR_UNSUPPORTED;
    hipStream_t st = da_stream(stream);
    const int nblocks = fi_blocks(P);
    // forward: the single update from v = 0; it is the displacement itself, so only a non-finite point counts as not converged
    hipLaunchKernelGGL(fieldinv_points_kernel, dim3(nblocks, N), dim3(256), 0, st, disp, points, out, D, H, W, P, inverse ? 1 : 0,
                       inverse ? max_iters : 1, inverse ? tol_vox : INFINITY, stats ? (double*)ws : (double*)nullptr);
    DA_LAUNCH_CHECK();
    if (stats) {
        hipLaunchKernelGGL(fieldinv_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, N, nblocks, stats);
        DA_LAUNCH_CHECK();
    }
    return 0;
}
