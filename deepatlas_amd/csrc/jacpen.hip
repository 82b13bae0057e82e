// Jacobian folding penalty: L = 1 / (N V) sum_n sum_x max(0, eps - det J_n(x))^p, p in {1, 2}, the differentiable companion of the folding
// fraction da_jacobian_det reports (regeval.hip).  det J is that kernel's (da_jac_at / da_jac_det, common.h): u_c = disp_c (size_c - 1) / 2 voxels, numpy.gradient differences at
// unit spacing (central inside, one-sided on the faces, zero along an axis of extent 1), cofactor expansion in fp32.
// NDHWC: disp[N][D][H][W][3], channel order (x, y, z) = (W, H, D) axis, normalised units.
// Forward: one pass, the voxel deal and the reduction order of jacobian_det_kernel (per-thread doubles -> wave butterfly -> the four waves
// in order -> one partial row per workgroup -> a finalize kernel adding the rows in index order); it saves det per voxel for the backward.
// Backward: a gather.  d det(x) / d J_ca(x) = cofactor_ca(x), and J_ca(x) = delta_ca + k_a(x) (u_c(x + e_a) - u_c(x - e_a)) with the
// neighbours clamped to the volume, k_a = 1/2 inside and 1 on a face; so voxel y collects, per axis a, from x = y - e_a (+k_a(x)),
// x = y + e_a (-k_a(x)) and, when y lies on a face of a, from itself (-1 on the low face, +1 on the high face).  The saved det of the up
// to seven candidates is read first; the Jacobian of a candidate is formed again only when it is active (det < eps), which a realistic
// field is at a small share of its voxels.  No atomics anywhere: two runs are bit-identical.
#include "common.h"

namespace {

constexpr int kPenBlocks = 2048;   // partial rows per sample (multiple of 8: XCD-contiguous split), the launch of jacobian_det_kernel
constexpr int kPenStats = 2;       // per-block partials: sum of the penalties, number of active voxels

// d pen / d det of pen = max(0, eps - det)^p: 0 where det >= eps; a non-finite det gives NaN (the forward makes the loss NaN there too)
__device__ __forceinline__ float pen_factor(float det, float eps, int power) {
    if (!(fabsf(det) < INFINITY)) return NAN;
    const float t = eps - det;
    return t > 0.f ? (power == 1 ? -1.f : -2.f * t) : 0.f;
}

__global__ void __launch_bounds__(256)
jacdet_penalty_fwd_kernel(const float* __restrict__ disp, int D, int H, int W, float eps, int power, float* __restrict__ det_out,
                          double* __restrict__ partial) {
    __shared__ double red[4][kPenStats];
    const int n = blockIdx.y;
    const int V = D * H * W;
    const float* u = disp + (long long)n * V * 3;
    const float sx = da_vox_scale(W), sy = da_vox_scale(H), sz = da_vox_scale(D);
    double s = 0.0, cnt = 0.0;
    for (DaXcdLoop L = da_xcd_loop(V, 256); L.i < L.end; L.i += L.step) {
        const int v = (int)L.i;
        int d, h, w; da_vox3(v, H, W, d, h, w);
        const DaJac9 J = da_jac_at(u + (long long)v * 3, d, h, w, D, H, W, sx, sy, sz);
        const float det = da_jac_det(J);
        det_out[(long long)n * V + v] = det;
        const float t = eps - det;
        float pen = t > 0.f ? (power == 1 ? t : t * t) : 0.f;
        const bool bad = !(fabsf(det) < INFINITY);              // a non-finite displacement must not pass as "no fold"
        if (bad) pen = NAN;
        s += (double)pen;
        if (bad || det < eps) cnt += 1.0;
    }
    s = da_wave_sum(s); cnt = da_wave_sum(cnt);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[wid][0] = s; red[wid][1] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* p = partial + ((size_t)n * gridDim.x + blockIdx.x) * kPenStats;
        p[0] = da_sum4(red, 0);
        p[1] = da_sum4(red, 1);
    }
}

// one wave: lane l adds rows l, l + 64, ... of the N x nblocks partial rows in that order, then the fixed butterfly
__global__ void jacdet_penalty_finalize_kernel(const double* __restrict__ partial, int nrows, double count, float* __restrict__ loss,
                                               double* __restrict__ stats) {
    const int lane = threadIdx.x;
    double s = 0.0, cnt = 0.0;
    for (int b = lane; b < nrows; b += 64) { s += partial[(size_t)b * kPenStats]; cnt += partial[(size_t)b * kPenStats + 1]; }
    s = da_wave_sum(s); cnt = da_wave_sum(cnt);
    if (lane == 0) {
        loss[0] = (float)(s / count);
        if (stats) { stats[0] = s; stats[1] = cnt; }
    }
}

// One thread per voxel y, its three components together: the candidates' cofactors are shared by the components.
__global__ void __launch_bounds__(256)
jacdet_penalty_bwd_kernel(const float* __restrict__ disp, const float* __restrict__ det, const float* __restrict__ dloss,
                          float* __restrict__ d_disp, int D, int H, int W, float eps, int power, float inv_count) {
    const int n = blockIdx.y;
    const int V = D * H * W;
    const float* u = disp + (long long)n * V * 3;
    const float* dt = det + (long long)n * V;
    float* du = d_disp + (long long)n * V * 3;
    const float sx = da_vox_scale(W), sy = da_vox_scale(H), sz = da_vox_scale(D);
    const float gl = dloss[0] * inv_count;
    const int HW = H * W;
    for (DaXcdLoop L = da_xcd_loop(V, 256); L.i < L.end; L.i += L.step) {
        const int v = (int)L.i;
        int d, h, w; da_vox3(v, H, W, d, h, w);
        const int wl = w > 0 ? 1 : 0, wh = w < W - 1 ? 1 : 0;
        const int hl = h > 0 ? 1 : 0, hh = h < H - 1 ? 1 : 0;
        const int dl = d > 0 ? 1 : 0, dh = d < D - 1 ? 1 : 0;
        // the seven saved values first (a missing neighbour reads the voxel itself and is masked below)
        const float t0 = dt[v], txa = dt[v - wl], txb = dt[v + wh], tya = dt[v - hl * W], tyb = dt[v + hh * W], tza = dt[v - dl * HW], tzb = dt[v + dh * HW];
        // y's own row holds y only on a face: -1 on the low face, +1 on the high one (extent 1: both, 0)
        const float cx = (w == 0 ? -1.f : 0.f) + (w == W - 1 ? 1.f : 0.f);
        const float cy = (h == 0 ? -1.f : 0.f) + (h == H - 1 ? 1.f : 0.f);
        const float cz = (d == 0 ? -1.f : 0.f) + (d == D - 1 ? 1.f : 0.f);
        const float g0 = (cx != 0.f || cy != 0.f || cz != 0.f) ? pen_factor(t0, eps, power) : 0.f;
        const float gxa = wl ? pen_factor(txa, eps, power) : 0.f, gxb = wh ? pen_factor(txb, eps, power) : 0.f;
        const float gya = hl ? pen_factor(tya, eps, power) : 0.f, gyb = hh ? pen_factor(tyb, eps, power) : 0.f;
        const float gza = dl ? pen_factor(tza, eps, power) : 0.f, gzb = dh ? pen_factor(tzb, eps, power) : 0.f;
        float ax = 0.f, ay = 0.f, az = 0.f;
        // candidate x = y + (od, oh, ow) with factor g; (kx, ky, kz) = the signed stencil weights of y in x's differences along (x, y, z)
        auto gather = [&](float g, int od, int oh, int ow, float kx, float ky, float kz) {
            if (g != 0.f) {                                     // (NaN compares unequal: a non-finite det reaches the gradient)
                const int xv = v + od * HW + oh * W + ow;
                const DaJac9 J = da_jac_at(u + (long long)xv * 3, d + od, h + oh, w + ow, D, H, W, sx, sy, sz);
                const float c00 = J.j11 * J.j22 - J.j12 * J.j21, c01 = -(J.j10 * J.j22 - J.j12 * J.j20), c02 = J.j10 * J.j21 - J.j11 * J.j20;
                const float c10 = -(J.j01 * J.j22 - J.j02 * J.j21), c11 = J.j00 * J.j22 - J.j02 * J.j20, c12 = -(J.j00 * J.j21 - J.j01 * J.j20);
                const float c20 = J.j01 * J.j12 - J.j02 * J.j11, c21 = -(J.j00 * J.j12 - J.j02 * J.j10), c22 = J.j00 * J.j11 - J.j01 * J.j10;
                ax += g * (c00 * kx + c01 * ky + c02 * kz);
                ay += g * (c10 * kx + c11 * ky + c12 * kz);
                az += g * (c20 * kx + c21 * ky + c22 * kz);
            }
        };
        // k_a(x) = 1/2 where x is inside along a, 1 where x lies on a face of a
        gather(g0, 0, 0, 0, cx, cy, cz);
        gather(gxa, 0, 0, -1, (w - 1 > 0) ? 0.5f : 1.f, 0.f, 0.f);
        gather(gxb, 0, 0, 1, (w + 1 < W - 1) ? -0.5f : -1.f, 0.f, 0.f);
        gather(gya, 0, -1, 0, 0.f, (h - 1 > 0) ? 0.5f : 1.f, 0.f);
        gather(gyb, 0, 1, 0, 0.f, (h + 1 < H - 1) ? -0.5f : -1.f, 0.f);
        gather(gza, -1, 0, 0, 0.f, 0.f, (d - 1 > 0) ? 0.5f : 1.f);
        gather(gzb, 1, 0, 0, 0.f, 0.f, (d + 1 < D - 1) ? -0.5f : -1.f);
        float* o = du + (long long)v * 3;
        o[0] = gl * sx * ax; o[1] = gl * sy * ay; o[2] = gl * sz * az;
    }
}

int pen_blocks(long long V) {
    long long g = da_cdiv(V, 256);
    if (g > kPenBlocks) g = kPenBlocks;
    if (g >= 8) g = g / 8 * 8;          // a multiple of 8 takes the XCD-contiguous split
    return (int)(g < 1 ? 1 : g);
}

bool pen_args_ok(int N, int D, int H, int W, float eps, int power) {
    return N >= 1 && N <= 65535 && D >= 1 && H >= 1 && W >= 1 && (power == 1 || power == 2) && eps >= 0.f && eps <= 1.f;      // (a NaN eps fails both comparisons)
}

}  // namespace

extern "C" size_t da_jacdet_penalty_ws_bytes(int N, int D, int H, int W) {
    (void)D; (void)H; (void)W;
    return da_align((size_t)(N > 0 ? N : 1) * kPenBlocks * kPenStats * sizeof(double));
}

extern "C" int da_jacdet_penalty_fwd(const float* disp, int N, int D, int H, int W, float eps, int power, float* loss, double* stats,
                                     float* det, void* ws, size_t ws_bytes, void* stream) {
    if (!disp || !loss || !det || !ws || !pen_args_ok(N, D, H, W, eps, power)) return DA_ERR_BADARG;
    if (ws_bytes < da_jacdet_penalty_ws_bytes(N, D, H, W)) return DA_ERR_WS_SMALL;
    const long long V = (long long)D * H * W;
    if (V >= 0x7FFFFFFFLL / 4) return DA_ERR_UNSUPPORTED;                  // 32-bit voxel and element offsets inside a sample
    hipStream_t st = da_stream(stream);
    const int nblocks = pen_blocks(V);
    hipLaunchKernelGGL(jacdet_penalty_fwd_kernel, dim3(nblocks, N), dim3(256), 0, st, disp, D, H, W, eps, power, det, (double*)ws);
    DA_LAUNCH_CHECK();
    hipLaunchKernelGGL(jacdet_penalty_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, nblocks * N, (double)N * (double)V, loss, stats);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_jacdet_penalty_bwd(const float* disp, const float* det, const float* dloss, float* d_disp, int N, int D, int H, int W,
                                     float eps, int power, void* stream) {
    if (!disp || !det || !dloss || !d_disp || !pen_args_ok(N, D, H, W, eps, power)) return DA_ERR_BADARG;
    const long long V = (long long)D * H * W;
    if (V >= 0x7FFFFFFFLL / 4) return DA_ERR_UNSUPPORTED;
    const float inv_count = (float)(1.0 / ((double)N * (double)V));
    hipLaunchKernelGGL(jacdet_penalty_bwd_kernel, dim3(pen_blocks(V), N), dim3(256), 0, da_stream(stream), disp, det, dloss, d_disp, D, H, W,
                       eps, power, inv_count);
    DA_LAUNCH_CHECK();
    return 0;
}
