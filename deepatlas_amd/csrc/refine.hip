// Instance refinement of a displacement field: descend on 1 - NCC(moving o (identity + disp), fixed) for this very pair, the warped image
// never written.  One iteration is da_refine_moments (the five sums of NCC through the warp), the caller's regulariser gradient
// (da_bending_bwd into a scratch field) and da_refine_step (similarity gradient + that field -> Adam on disp in place).
// Conventions are da_warp_fwd's: moving / fixed [N][D][H][W] fp32 (one channel), disp [N][D][H][W][3] with channels (x, y, z) = (W, H, D) axis
// in normalised units, sample point identity + disp, trilinear, zeros outside, align_corners=True, the taps and their order those of
// warp_fwd_kernel<1>, the derivative those of warp_bwd_kernel<1> (floor-based taps: at an integer coordinate the cell above it).
// Differences from the warp: an axis of extent 1 is legal (its identity coordinate is 0, every finite coordinate samples index 0, its
// gradient is 0), and a sample coordinate that is NaN, infinite or >= 1e9 in magnitude -- the warp samples nothing there -- makes the sums of
// its sample, and its own three gradient / update elements, NaN: a broken field never passes as converged.
// Both kernels are gathers: 12 bytes of disp, 4 of fixed and eight taps of moving per voxel, the taps of neighbouring voxels in the same or
// adjacent lines (L2 / L1 hits for a smooth field).  No scatter, no atomics, no workgroup waits for another: the sums go thread -> wave
// butterfly -> the four waves in order -> one partial per workgroup and entry -> a finalize kernel adding them in workgroup order, so two
// runs are bit-identical.  In place is safe in the step: a voxel's lane reads moving at x + u(x) and reads / writes disp, m, v at x only.
#include "common.h"

namespace {

constexpr int kRfBlocks = 2048;    // workgroups per sample at most (multiple of 8: XCD-contiguous split), the launch of affine.hip / jacpen.hip
constexpr int kRfSums = 5;         // sum w', sum f', sum w' f', sum w'^2, sum f'^2 with w' = w - moving[n][0], f' = f - fixed[n][0] (da_ncc_fwd's pivots)

struct RfSample { float w, gx, gy, gz; bool fin; };   // w and d w / d (x, y, z) in voxel coordinates

__device__ __forceinline__ float rf_id_coord(int k, int size) { return size > 1 ? da_id_coord(k, size) : 0.f; }

// the warp's sample of voxel (d, h, w) of one sample's volume `mv`, u = the voxel's three displacements; GRAD: also the derivative
template <bool GRAD>
__device__ __forceinline__ RfSample rf_sample(const float* __restrict__ mv, float ux, float uy, float uz, int d, int h, int w, int D, int H, int W) {
    const float gx = ux + rf_id_coord(w, W), gy = uy + rf_id_coord(h, H), gz = uz + rf_id_coord(d, D);
    RfSample s;
    s.fin = da_is_finite_coord(gx, gy, gz);
    const DaTaps t = da_make_taps(s.fin ? gx : -4.f, s.fin ? gy : -4.f, s.fin ? gz : -4.f, D, H, W);
    float acc = 0.f, gix = 0.f, giy = 0.f, giz = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int cz = k >> 2, cy = (k >> 1) & 1, cx = k & 1;
        const int x = t.x0 + cx, y = t.y0 + cy, z = t.z0 + cz;
        if (x >= 0 && x < W && y >= 0 && y < H && z >= 0 && z < D) {
            const float wx = cx ? t.fx0 : t.fx1, wy = cy ? t.fy0 : t.fy1, wz = cz ? t.fz0 : t.fz1;
            const float a = mv[(z * H + y) * W + x];
            acc += a * (wx * wy * wz);
            if (GRAD) {
                gix += (cx ? a : -a) * wy * wz;
                giy += (cy ? a : -a) * wx * wz;
                giz += (cz ? a : -a) * wx * wy;
            }
        }
    }
    s.w = acc; s.gx = gix; s.gy = giy; s.gz = giz;
    return s;
}

__global__ void __launch_bounds__(256)
refine_moments_kernel(const float* __restrict__ moving, const float* __restrict__ fixed, const float* __restrict__ disp, int D, int H, int W,
                      double* __restrict__ partial /* [N][5][gridDim.x] */) {
    __shared__ double red[4][kRfSums];
    const int n = blockIdx.y;
    const int V = D * H * W;
    const float* mv = moving + (long long)n * V;
    const float* fx = fixed + (long long)n * V;
    const float* u = disp + (long long)n * V * 3;
    const float pw = mv[0], pf = fx[0];
    double acc[kRfSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (DaXcdLoop L = da_xcd_loop(V, 256); L.i < L.end; L.i += L.step) {
        const int v = (int)L.i;
        int d, h, w; da_vox3(v, H, W, d, h, w);
        const RfSample s = rf_sample<false>(mv, u[(long long)v * 3], u[(long long)v * 3 + 1], u[(long long)v * 3 + 2], d, h, w, D, H, W);
        const double p = s.fin ? (double)(s.w - pw) : (double)NAN, q = (double)(fx[v] - pf);
        acc[0] += p; acc[1] += q; acc[2] = fma(p, q, acc[2]); acc[3] = fma(p, p, acc[3]); acc[4] = fma(q, q, acc[4]);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kRfSums; ++k) {
        const double r = da_wave_sum(acc[k]);
        if (lane == 0) red[wid][k] = r;
    }
    __syncthreads();
    if (threadIdx.x < kRfSums) {
        const int k = threadIdx.x;
        partial[((size_t)n * kRfSums + k) * gridDim.x + blockIdx.x] = da_sum4(red, k);
    }
}

// grid (N), 5 waves: wave k adds entry k's partials (lane l: workgroups l, l + 64, ... in that order, then the fixed butterfly); thread 0
// forms the row of da_ncc_fwd's finalize kernel: {mean_w, mean_f, cov, var_w, var_f, ncc, M, 0}
__global__ void __launch_bounds__(64 * kRfSums)
refine_moments_finalize_kernel(const double* __restrict__ partial, int nblocks, int V, const float* __restrict__ moving, const float* __restrict__ fixed,
                               double* __restrict__ stats) {
    __shared__ double s[kRfSums];
    const int n = blockIdx.x, k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double* p = partial + ((size_t)n * kRfSums + k) * nblocks;
    double a = 0.0;
    for (int b = lane; b < nblocks; b += 64) a += p[b];
    a = da_wave_sum(a);
    if (lane == 0) s[k] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double M = (double)V;
        const double mw = s[0] / M, mf = s[1] / M;
        const double cov = s[2] / M - mw * mf;
        const double vw = s[3] / M - mw * mw, vf = s[4] / M - mf * mf;
        double* o = stats + (size_t)n * 8;
        o[0] = mw + (double)moving[(long long)n * V]; o[1] = mf + (double)fixed[(long long)n * V]; o[2] = cov; o[3] = vw; o[4] = vf;
        o[5] = cov / (sqrt(vw) * sqrt(vf)); o[6] = M; o[7] = 0.0;
    }
}

// state (DA_REFINE_STATE_FLOATS floats, device): {1 / bc1, beta1, beta2, eps, 1 / sqrt(bc2), grad_scale, lambda_sim, lr_x / bc1, lr_y / bc1, lr_z / bc1, iter, 0}
// -- da_adam_step_dev's state6 with lr = 1, then the similarity weight, the per-channel step sizes and the slot of `hist` this launch writes.
// One element of Adam, optim.hip's adam_update on values (contraction off: the same roundings as da_adam_step given the same scalars).
__device__ __forceinline__ void rf_adam(float& p, float& m, float& v, float g, float lr_over_bc1, float beta1, float beta2, float eps, float inv_sqrt_bc2, float gscale) {
#pragma clang fp contract(off)
    const float gi = g * gscale;
    const float mi = beta1 * m + (1.f - beta1) * gi;
    const float vi = beta2 * v + (1.f - beta2) * gi * gi;
    m = mi; v = vi;
    const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
    p = p - lr_over_bc1 * (mi / denom);
}

template <bool UPDATE>
__global__ void __launch_bounds__(256)
refine_step_kernel(const float* __restrict__ moving, const float* __restrict__ fixed, float* disp, const float* g_extra, const double* __restrict__ stats,
                   const float* __restrict__ state, float* m, float* v, float* grad_out, float* __restrict__ hist, int hist_len, int N, int D, int H, int W) {
    __shared__ float coef[4];          // d (1 - mean NCC) / d w(x) = A (w - mean_w) + B (f - mean_f); mean_w, mean_f
    const int n = blockIdx.y;
    const int V = D * H * W;
    if (threadIdx.x == 0) {
        const double* s = stats + (size_t)n * 8;
        const double k = -1.0 / ((double)N * s[6]);           // da_ncc_bwd's expressions with dloss = 1
        const double sxy = sqrt(s[3]) * sqrt(s[4]);
        coef[0] = (float)(-k * s[5] / s[3]); coef[1] = (float)(k / sxy); coef[2] = (float)s[0]; coef[3] = (float)s[1];
        if (hist && blockIdx.x == 0 && n == 0) {
            const int it = (int)state[10];
            double t = 0.0;
            for (int i = 0; i < N; ++i) t += stats[(size_t)i * 8 + 5];
            if (it >= 0 && it < hist_len) hist[it] = (float)(1.0 - t / (double)N);
        }
    }
    __syncthreads();
    const float A = coef[0], B = coef[1], mw = coef[2], mf = coef[3];
    const float beta1 = state[1], beta2 = state[2], eps = state[3], inv_sqrt_bc2 = state[4], gscale = state[5], lam = state[6];
    const float lr[3] = {state[7], state[8], state[9]};
    const float sc[3] = {da_vox_scale(W), da_vox_scale(H), da_vox_scale(D)};
    const float* mv = moving + (long long)n * V;
    const float* fx = fixed + (long long)n * V;
    for (DaXcdLoop L = da_xcd_loop(V, 256); L.i < L.end; L.i += L.step) {
        const int v0 = (int)L.i;
        int d, h, w; da_vox3(v0, H, W, d, h, w);
        const long long e = ((long long)n * V + v0) * 3;
        float u[3] = {disp[e], disp[e + 1], disp[e + 2]};
        const RfSample s = rf_sample<true>(mv, u[0], u[1], u[2], d, h, w, D, H, W);
        const float dw = lam * (A * (s.w - mw) + B * (fx[v0] - mf));
        float g[3] = {dw * s.gx * sc[0], dw * s.gy * sc[1], dw * s.gz * sc[2]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (!s.fin) g[c] = NAN;
            else if (g_extra) g[c] += g_extra[e + c];
            if (grad_out) grad_out[e + c] = g[c];
            if (UPDATE) {
                float mi = m[e + c], vi = v[e + c];
                rf_adam(u[c], mi, vi, g[c], lr[c], beta1, beta2, eps, inv_sqrt_bc2, gscale);
                m[e + c] = mi; v[e + c] = vi; disp[e + c] = u[c];
            }
        }
    }
}

int rf_blocks(long long V) {
    int g = da_grid(V, 256, kRfBlocks);
    if (g >= 8) g = g / 8 * 8;          // a multiple of 8 takes the XCD-contiguous split
    return g;
}

bool rf_args_ok(int N, int D, int H, int W) { return N >= 1 && N <= 64 && D >= 1 && H >= 1 && W >= 1; }
bool rf_size_ok(int D, int H, int W) { return (long long)D * H * W < 0x7FFFFFFFLL / 4; }      // 32-bit voxel offsets inside a sample

struct RfMomentsWs { double* partial; size_t bytes; };
RfMomentsWs rf_moments_layout(void* ws, int N) { DaCarve c(ws); return RfMomentsWs{c.take<double>((size_t)(N > 0 ? N : 1) * kRfSums * kRfBlocks), c.off}; }

}  // namespace

extern "C" size_t da_refine_moments_ws_bytes(int N, int D, int H, int W) {
    (void)D; (void)H; (void)W;
    return rf_moments_layout(nullptr, N).bytes;
}

extern "C" int da_refine_moments(const float* moving, const float* fixed, const float* disp, int N, int D, int H, int W, double* stats,
                                 void* ws, size_t ws_bytes, void* stream) {
    if (!moving || !fixed || !disp || !stats || !ws || !rf_args_ok(N, D, H, W)) return DA_ERR_BADARG;
    if (!rf_size_ok(D, H, W)) return DA_ERR_UNSUPPORTED;
    const RfMomentsWs L = rf_moments_layout(ws, N);
    if (ws_bytes < L.bytes) return DA_ERR_WS_SMALL;
    hipStream_t st = da_stream(stream);
    const int V = D * H * W, nblocks = rf_blocks(V);
    hipLaunchKernelGGL(refine_moments_kernel, dim3(nblocks, N), dim3(256), 0, st, moving, fixed, disp, D, H, W, L.partial);
    DA_LAUNCH_CHECK();
    hipLaunchKernelGGL(refine_moments_finalize_kernel, dim3(N), dim3(64 * kRfSums), 0, st, (const double*)L.partial, nblocks, V, moving, fixed, stats);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_refine_host_state(const float* lr3, float beta1, float beta2, float eps, int step, float grad_scale, float lambda_sim, int iter,
                                    float* state_host) {
    if (!lr3 || !state_host || step < 1 || iter < 0) return DA_ERR_BADARG;
    const int rc = da_adam_host_state(1.f, beta1, beta2, eps, step, grad_scale, state_host);
    if (rc != 0) return rc;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);          // da_adam_step's lr / bc1, per channel
    state_host[6] = lambda_sim;
    for (int c = 0; c < 3; ++c) state_host[7 + c] = (float)((double)lr3[c] / bc1);
    state_host[10] = (float)iter; state_host[11] = 0.f;
    return 0;
}

extern "C" int da_refine_step(const float* moving, const float* fixed, float* disp, const float* g_extra, const double* stats, const float* state,
                              float* m, float* v, float* grad_out, float* hist, int hist_len, int N, int D, int H, int W, int update, void* stream) {
    if (!moving || !fixed || !disp || !stats || !state || !rf_args_ok(N, D, H, W)) return DA_ERR_BADARG;
    if (update ? (!m || !v) : !grad_out) return DA_ERR_BADARG;           // nothing to write
    if (hist && hist_len < 1) return DA_ERR_BADARG;
    if (!rf_size_ok(D, H, W)) return DA_ERR_UNSUPPORTED;
    const dim3 grid(rf_blocks((long long)D * H * W), N);
    if (update) hipLaunchKernelGGL(refine_step_kernel<true>, grid, dim3(256), 0, da_stream(stream), moving, fixed, disp, g_extra, stats, state, m, v, grad_out, hist, hist_len, N, D, H, W);
    else hipLaunchKernelGGL(refine_step_kernel<false>, grid, dim3(256), 0, da_stream(stream), moving, fixed, disp, g_extra, stats, state, m, v, grad_out, hist, hist_len, N, D, H, W);
    DA_LAUNCH_CHECK();
    return 0;
}
