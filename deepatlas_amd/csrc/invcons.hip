// Inverse-consistency penalty of two displacement fields: the composition residual r(x) = u_a(x) + T[u_b](x + u_a(x)) of ICON / GradICON,
// L(u_a, u_b) = 1 / (N V) sum_n sum_x sum_c (s_c r_c(x))^2 in voxels^2, s_c = (size_c - 1) / 2.  T is the warp's own trilinear sample (zeros
// outside, align_corners=True) at the warp's own fp32 coordinate (da_id_coord / da_make_taps, common.h): the point the penalty composes at
// is the point the warp reads.
// NDHWC: disp[N][D][H][W][3], channel order (x, y, z) = (W, H, D) axis, normalised units.
// Forward: one pass per voxel (12-byte read of u_a, eight 12-byte taps of u_b), r saved for the backward, the voxel deal and the reduction
// order of jacpen.hip (per-thread doubles -> wave butterfly -> the four waves in order -> one partial row per workgroup -> a finalize kernel
// adding the rows in index order): bit-identical from run to run.
// Backward, with g_c(x) = dloss 2 s_c^2 r_c(x) / (N V), one kernel per wanted gradient:
//   d u_a,k(x) = g_k(x) + s_k sum_c g_c(x) dT[u_b,c] / d(voxel coordinate k)      a gather local to x, one lane per voxel
//   d u_b,c(y) += w(x -> y) g_c(x)                                                  the adjoint of the gather: fp32 atomic adds, one lane per
//                                                                                   ELEMENT (x, c), g formed from the saved residual
// or, deterministic, g is stored and da_warp_bwd_dsrc_det's fixed-point accumulation (warp.hip) scatters it.
// (The scatter had one lane per voxel inside the gather kernel first: a wave's atomic instruction then covered 64 dwords at a 12-byte stride and
// the adds ran at 0.08 - 0.20 TB/s; with one lane per element neighbouring lanes add to neighbouring dwords wherever neighbouring voxels land on
// neighbouring rows.)
#include "common.h"

namespace {

constexpr int kIcBlocks = 2048;    // partial rows per sample (multiple of 8: XCD-contiguous split), the launch of jacpen.hip
constexpr int kIcStats = 4;        // per-block partials: sum |s r|^2, sum |s r|, max |s r|, voxels sampled outside the volume

struct IcPoint { float gx, gy, gz; bool fin; DaTaps t; };

// the sample point of voxel (d, h, w): the warp's deform and taps; a non-finite / huge coordinate puts every tap out of range (-4)
__device__ __forceinline__ IcPoint ic_point(const float* __restrict__ ua, int d, int h, int w, int D, int H, int W) {
    IcPoint p;
    p.gx = ua[0] + da_id_coord(w, W); p.gy = ua[1] + da_id_coord(h, H); p.gz = ua[2] + da_id_coord(d, D);
    p.fin = da_is_finite_coord(p.gx, p.gy, p.gz);
    p.t = da_make_taps(p.fin ? p.gx : -4.f, p.fin ? p.gy : -4.f, p.fin ? p.gz : -4.f, D, H, W);
    return p;
}

// does the sample point leave [0, size - 1] on some axis?  (da_unnormalize's expression, written out: the call gave the forward kernel
// another register allocation)
__device__ __forceinline__ bool ic_outside(const IcPoint& p, int D, int H, int W) {
    if (!p.fin) return true;
    const float ix = ((p.gx + 1.f) / 2.f) * (float)(W - 1), iy = ((p.gy + 1.f) / 2.f) * (float)(H - 1), iz = ((p.gz + 1.f) / 2.f) * (float)(D - 1);
    return !(ix >= 0.f && ix <= (float)(W - 1) && iy >= 0.f && iy <= (float)(H - 1) && iz >= 0.f && iz <= (float)(D - 1));
}

__global__ void __launch_bounds__(256)
invcons_fwd_kernel(const float* __restrict__ disp_a, const float* __restrict__ disp_b, int D, int H, int W, float* __restrict__ resid,
                   double* __restrict__ partial) {
    __shared__ double red[4][kIcStats];
    const int n = blockIdx.y;
    const int V = D * H * W;
    const float* ua = disp_a + (long long)n * V * 3;
    const float* ub = disp_b + (long long)n * V * 3;
    const float sx = da_vox_scale(W), sy = da_vox_scale(H), sz = da_vox_scale(D);
    double s2 = 0.0, s1 = 0.0, mx = 0.0, out = 0.0;
    for (DaXcdLoop L = da_xcd_loop(V, 256); L.i < L.end; L.i += L.step) {
        const int v = (int)L.i;
        int d, h, w; da_vox3(v, H, W, d, h, w);
        const float* a = ua + (long long)v * 3;
        const IcPoint p = ic_point(a, d, h, w, D, H, W);
        float tx = 0.f, ty = 0.f, tz = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int cz = k >> 2, cy = (k >> 1) & 1, cx = k & 1;
            const int x = p.t.x0 + cx, y = p.t.y0 + cy, z = p.t.z0 + cz;
            if (x >= 0 && x < W && y >= 0 && y < H && z >= 0 && z < D) {
                const float wgt = (cx ? p.t.fx0 : p.t.fx1) * (cy ? p.t.fy0 : p.t.fy1) * (cz ? p.t.fz0 : p.t.fz1);
                const float* b = ub + ((z * H + y) * W + x) * 3;
                tx += b[0] * wgt; ty += b[1] * wgt; tz += b[2] * wgt;
            }
        }
        const float rx = a[0] + tx, ry = a[1] + ty, rz = a[2] + tz;
        if (resid) { float* o = resid + ((long long)n * V + v) * 3; o[0] = rx; o[1] = ry; o[2] = rz; }
        const float ex = sx * rx, ey = sy * ry, ez = sz * rz;
        float q = ex * ex + ey * ey + ez * ez;
        float e = sqrtf(q);
        // a coordinate the warp refuses (NaN, inf, >= 1e9) samples nothing: r = u_a there, which for a huge finite value would be a finite
        // number.  Such a voxel makes the sums NaN and the maximum infinite: a bad field never passes as consistent.
        if (!p.fin) { q = NAN; e = NAN; mx = INFINITY; }
        s2 += (double)q; s1 += (double)e;
        mx = fmax(mx, (double)e);                                   // (fmax drops a NaN operand; the sums carry it)
        if (ic_outside(p, D, H, W)) out += 1.0;
    }
    s2 = da_wave_sum(s2); s1 = da_wave_sum(s1); mx = da_wave_max(mx); out = da_wave_sum(out);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[wid][0] = s2; red[wid][1] = s1; red[wid][2] = mx; red[wid][3] = out; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* o = partial + ((size_t)n * gridDim.x + blockIdx.x) * kIcStats;
        o[0] = da_sum4(red, 0);
        o[1] = da_sum4(red, 1);
        o[2] = da_max4(red, 2);
        o[3] = da_sum4(red, 3);
    }
}

// one wave: sample by sample, lane l adds rows l, l + 64, ... of the sample's nblocks partial rows in that order, then the fixed butterfly;
// the loss adds the samples' sums in index order
__global__ void invcons_finalize_kernel(const double* __restrict__ partial, int N, int nblocks, double count, float* __restrict__ loss,
                                        double* __restrict__ stats) {
    const int lane = threadIdx.x;
    double total = 0.0;
    for (int n = 0; n < N; ++n) {
        const double* p = partial + (size_t)n * nblocks * kIcStats;
        double s2 = 0.0, s1 = 0.0, mx = 0.0, out = 0.0;
        for (int b = lane; b < nblocks; b += 64) {
            s2 += p[(size_t)b * kIcStats]; s1 += p[(size_t)b * kIcStats + 1];
            mx = fmax(mx, p[(size_t)b * kIcStats + 2]); out += p[(size_t)b * kIcStats + 3];
        }
        s2 = da_wave_sum(s2); s1 = da_wave_sum(s1); mx = da_wave_max(mx); out = da_wave_sum(out);
        total += s2;
        if (stats && lane == 0) { double* o = stats + (size_t)n * kIcStats; o[0] = s2; o[1] = s1; o[2] = mx; o[3] = out; }
    }
    if (lane == 0) loss[0] = (float)(total / count);
}

// d u_a: one thread per voxel x, its three components together: the taps and the eight u_b rows are shared by the components.  gmat (may be
// NULL): g is stored there for the deterministic scatter.  A voxel whose coordinate the warp refuses gets a NaN gradient, as its loss term is NaN.
__global__ void __launch_bounds__(256)
invcons_bwd_kernel(const float* __restrict__ disp_a, const float* __restrict__ disp_b, const float* __restrict__ resid,
                   const float* __restrict__ dloss, float* __restrict__ d_disp_a, float* __restrict__ gmat, int D, int H, int W, float inv_count) {
    const int n = blockIdx.y;
    const int V = D * H * W;
    const long long sb = (long long)n * V * 3;
    const float* ua = disp_a + sb;
    const float* ub = disp_b + sb;
    const float sx = da_vox_scale(W), sy = da_vox_scale(H), sz = da_vox_scale(D);
    const float gl = dloss[0] * inv_count * 2.f;
    for (DaXcdLoop L = da_xcd_loop(V, 256); L.i < L.end; L.i += L.step) {
        const int v = (int)L.i;
        int d, h, w; da_vox3(v, H, W, d, h, w);
        const IcPoint p = ic_point(ua + (long long)v * 3, d, h, w, D, H, W);
        const float* r = resid + sb + (long long)v * 3;
        const float g0 = gl * (sx * sx) * r[0], g1 = gl * (sy * sy) * r[1], g2 = gl * (sz * sz) * r[2];
        if (gmat) { float* o = gmat + sb + (long long)v * 3; o[0] = g0; o[1] = g1; o[2] = g2; }
        if (!d_disp_a) continue;
        float gix = 0.f, giy = 0.f, giz = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int cz = k >> 2, cy = (k >> 1) & 1, cx = k & 1;
            const int x = p.t.x0 + cx, y = p.t.y0 + cy, z = p.t.z0 + cz;
            if (x >= 0 && x < W && y >= 0 && y < H && z >= 0 && z < D) {
                const float wx = cx ? p.t.fx0 : p.t.fx1, wy = cy ? p.t.fy0 : p.t.fy1, wz = cz ? p.t.fz0 : p.t.fz1;
                const float* b = ub + ((z * H + y) * W + x) * 3;
                const float dot = b[0] * g0 + b[1] * g1 + b[2] * g2;      // sum_c u_b[corner][c] g_c
                gix += (cx ? dot : -dot) * wy * wz;
                giy += (cy ? dot : -dot) * wx * wz;
                giz += (cz ? dot : -dot) * wx * wy;
            }
        }
        float* o = d_disp_a + sb + (long long)v * 3;
        if (p.fin) { o[0] = g0 + gix * sx; o[1] = g1 + giy * sy; o[2] = g2 + giz * sz; }
        else { o[0] = NAN; o[1] = NAN; o[2] = NAN; }
    }
}

// d u_b: one lane per element (x, c) of the sample, V * 3 < 2^31.  Consecutive lanes hold consecutive floats of g, and where neighbouring voxels
// land on neighbouring rows a wave's atomic instruction adds to consecutive dwords of d_disp_b.  The taps are derived per lane (three times per
// voxel: cheap next to eight atomics).  A refused coordinate has no tap in range and adds nothing.
__global__ void __launch_bounds__(256)
invcons_scatter_kernel(const float* __restrict__ disp_a, const float* __restrict__ resid, const float* __restrict__ dloss,
                       float* __restrict__ d_disp_b, int D, int H, int W, float inv_count) {
    const int n = blockIdx.y;
    const int V = D * H * W;
    const long long sb = (long long)n * V * 3;
    const float* ua = disp_a + sb;
    const float gl = dloss[0] * inv_count * 2.f;
    for (DaXcdLoop L = da_xcd_loop((long long)V * 3, 256); L.i < L.end; L.i += L.step) {
        const int i = (int)L.i;
        const int v = (int)((unsigned)i / 3u), c = i - v * 3;
        int d, h, w; da_vox3(v, H, W, d, h, w);
        const IcPoint p = ic_point(ua + (long long)v * 3, d, h, w, D, H, W);
        const float sc = da_vox_scale(c == 0 ? W : (c == 1 ? H : D));
        const float g = gl * (sc * sc) * resid[sb + i];
        float* base = d_disp_b + sb + c;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int cz = k >> 2, cy = (k >> 1) & 1, cx = k & 1;
            const int x = p.t.x0 + cx, y = p.t.y0 + cy, z = p.t.z0 + cz;
            if (x >= 0 && x < W && y >= 0 && y < H && z >= 0 && z < D) {
                const float wgt = (cx ? p.t.fx0 : p.t.fx1) * (cy ? p.t.fy0 : p.t.fy1) * (cz ? p.t.fz0 : p.t.fz1);
                atomicAdd(base + ((z * H + y) * W + x) * 3, wgt * g);
            }
        }
    }
}

int ic_blocks(long long V) {
    long long g = da_cdiv(V, 256);
    if (g > kIcBlocks) g = kIcBlocks;
    if (g >= 8) g = g / 8 * 8;          // a multiple of 8 takes the XCD-contiguous split
    return (int)(g < 1 ? 1 : g);
}

bool ic_args_ok(int N, int D, int H, int W) { return N >= 1 && N <= 65535 && D >= 2 && H >= 2 && W >= 2; }

}  // namespace

extern "C" size_t da_invcons_ws_bytes(int N, int D, int H, int W) {
    (void)D; (void)H; (void)W;
    return da_align((size_t)(N > 0 ? N : 1) * kIcBlocks * kIcStats * sizeof(double));
}

extern "C" int da_invcons_fwd(const float* disp_a, const float* disp_b, int N, int D, int H, int W, float* loss, double* stats,
                              float* resid, void* ws, size_t ws_bytes, void* stream) {
    if (!disp_a || !disp_b || !loss || !ws || !ic_args_ok(N, D, H, W)) return DA_ERR_BADARG;
    if (ws_bytes < da_invcons_ws_bytes(N, D, H, W)) return DA_ERR_WS_SMALL;
    const long long V = (long long)D * H * W;
    if (V >= 0x7FFFFFFFLL / 4) return DA_ERR_UNSUPPORTED;                  // 32-bit voxel and element offsets inside a sample
    hipStream_t st = da_stream(stream);
    const int nblocks = ic_blocks(V);
    hipLaunchKernelGGL(invcons_fwd_kernel, dim3(nblocks, N), dim3(256), 0, st, disp_a, disp_b, D, H, W, resid, (double*)ws);
    DA_LAUNCH_CHECK();
    hipLaunchKernelGGL(invcons_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, N, nblocks, (double)N * (double)V, loss, stats);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_invcons_bwd(const float* disp_a, const float* disp_b, const float* resid, const float* dloss, float* d_disp_a,
                              float* d_disp_b, int N, int D, int H, int W, int deterministic, void* ws, size_t ws_bytes, void* stream) {
    if (!disp_a || !disp_b || !resid || !dloss || !ic_args_ok(N, D, H, W)) return DA_ERR_BADARG;
    const long long V = (long long)D * H * W;
    if (V >= 0x7FFFFFFFLL / 4) return DA_ERR_UNSUPPORTED;
    if (!d_disp_a && !d_disp_b) return 0;
    hipStream_t st = da_stream(stream);
    const float inv_count = (float)(1.0 / ((double)N * (double)V));
    const dim3 grid(ic_blocks(V), N);
    if (deterministic && d_disp_b) {
        if (!ws) return DA_ERR_BADARG;
        if (ws_bytes < da_warp_bwd_dsrc_det_ws_bytes(N, D, H, W, 3)) return DA_ERR_WS_SMALL;
        // g is stored in d_disp_b itself: da_warp_bwd_dsrc_det has read all of `dout` into its fixed-point accumulator before its last
        // kernel writes d_src, and the three kernels are ordered on the stream
        hipLaunchKernelGGL(invcons_bwd_kernel, grid, dim3(256), 0, st, disp_a, disp_b, resid, dloss, d_disp_a, d_disp_b, D, H, W, inv_count);
        DA_LAUNCH_CHECK();
        return da_warp_bwd_dsrc_det(d_disp_b, disp_a, d_disp_b, N, D, H, W, 3, ws, ws_bytes, stream);
    }
    if (d_disp_a) {
        hipLaunchKernelGGL(invcons_bwd_kernel, grid, dim3(256), 0, st, disp_a, disp_b, resid, dloss, d_disp_a, (float*)nullptr, D, H, W, inv_count);
        DA_LAUNCH_CHECK();
    }
    if (d_disp_b) {
        hipLaunchKernelGGL(invcons_scatter_kernel, dim3(ic_blocks(V * 3), N), dim3(256), 0, st, disp_a, resid, dloss, d_disp_b, D, H, W, inv_count);
        DA_LAUNCH_CHECK();
    }
    return 0;
}
