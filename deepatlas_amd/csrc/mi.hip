// Mutual-information similarity (gfx950): VoxelMorph's global `MutualInformation` -- Gaussian Parzen windows over `bins` intensity centres.
//   c_i = linspace(vmin, vmax, B),  sigma = (vmax - vmin) / (B - 1) * sigma_ratio,  p = 1 / (2 sigma^2),  xh = clamp(x, vmin, vmax)
//   e_i(x) = exp(-p (xh - c_i)^2),  w_i = e_i / sum_k e_k,  P = (1/V) sum_v w(x_v) w(y_v)^T,  a = (1/V) sum_v w(x_v),  b likewise
//   Q = a b^T + 1e-6,  R = P / Q + 1e-6,  MI = sum_ij P_ij log R_ij,  loss = -mean_n MI
// The torch form materialises the two V x B weight matrices (and autograd keeps them); here they only ever exist as operands of the fp32
// matrix instruction v_mfma_f32_32x32x2_f32, generated in registers: both directions are skinny GEMMs (B x V by V x B forward, B x B by
// B x V backward) with bins padded to 32.
//
// forward   mi_partial_kernel: a wave takes 64 voxels (one per lane: clamp, the two normalisers sum_k e_k as a loop over the bins), then
//           32 matrix instructions, two voxels each: lane l generates bin l & 31 of voxel 2 s + (l >> 5) for both operands (one exponential
//           per operand per lane per instruction; the voxel's value and 1 / (s_x s_y) arrive by a lane shuffle; the (x, y) pair is a float2, so
//           the arithmetic around the two exponentials is packed; a padding bin generates bin 0's weights times zero).  The 32 x 32 sums go to
//           per-lane doubles every 4 tiles; the four waves are added in wave order through LDS: one double partial per workgroup.
//           mi_reduce_kernel sums the partials in a fixed order, mi_finalize_kernel (one workgroup, double) forms MI, G, ga, gb.
//           The marginals are the row / column sums of P (sum_j w_j = 1): no separate accumulation.  No atomics anywhere.
// backward  mi_bwd_kernel: a wave takes 32 voxels; both halves of the wave hold the same voxel and half of its bins.  U = G W_y + ga is 16
//           matrix instructions (A = G, constant, 16 registers; B = w(y_v); the accumulator starts at ga), likewise G^T W_x + gb.  The
//           contraction index is ordered like the accumulator's rows (bin 4 h + (t & 3) + 8 (t >> 2) at step t in half h), so the weights a
//           lane generates as the B operand are the ones it meets again in its 16 accumulator rows.
// Loads are single dwords (coalesced, 256 bytes per wave): 8 bytes per voxel against >= 64 exponentials, so there is no vector-load form and
// no alignment requirement beyond float (a sample base with V % 4 != 0 is as good as any other).
#include "common.h"

namespace {

constexpr int kMiTile = 256;            // voxels per workgroup tile (4 waves x 64)
constexpr int kMiMaxBlocks = 512;       // workgroups per sample (each >= 2 tiles when there are that many): 2 per CU, what the registers allow
constexpr int kMiFlush = 4;             // tiles between flushes of the fp32 accumulators into doubles
constexpr int kMiStats = DA_MI_STATS_FLOATS;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));      // the (x, y) pair of a voxel: one v_pk_* instruction per arithmetic step of the two

struct MiP {
    double vmin, delta;                 // centres c_i = vmin + i delta, rounded once to fp32
    float lo, hi, negp;                 // clamp range, -1 / (2 sigma^2)
    int bins;
};

// exp(t) for t <= 0 on the hardware exp2 with the rounding of t * log2(e) carried along: about 1 ulp for every t (the plain
// exp2(t * log2e) loses |t| * 2^-24 relative, 1e-6 at t = -12)
__device__ __forceinline__ f32x2 mi_exp(f32x2 t) {
    const f32x2 L = {1.44269502162933349609375f, 1.44269502162933349609375f}, Ll = {1.925963033500011e-8f, 1.925963033500011e-8f};      // log2(e) = L + Ll
    const f32x2 hi = t * L;
    f32x2 lo = __builtin_elementwise_fma(t, L, -hi);
    lo = __builtin_elementwise_fma(t, Ll, lo);
    const f32x2 e = {__builtin_amdgcn_exp2f(hi.x), __builtin_amdgcn_exp2f(hi.y)};
    return __builtin_elementwise_fma(e, lo * 0.693147180559945f, e);
}
// exp(negp d^2) of the pair
__device__ __forceinline__ f32x2 mi_gauss(f32x2 d, float negp) { return mi_exp(negp * d * d); }
// NaN passes through (fminf / fmaxf would drop it), +-inf is clamped
__device__ __forceinline__ float mi_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
__device__ __forceinline__ float mi_centre(const MiP& p, int i) { return (float)(p.vmin + (double)i * p.delta); }

__global__ void __launch_bounds__(256) mi_partial_kernel(const float* __restrict__ x, const float* __restrict__ y, long long V, MiP p,
                                                         double* __restrict__ partial /* [N][gridDim.x][1024] */) {
    __shared__ double comb[1024];
    __shared__ float cen[32];
    if (threadIdx.x < 32) cen[threadIdx.x] = mi_centre(p, threadIdx.x < p.bins ? threadIdx.x : 0);
    __syncthreads();
    const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane & 31, h = lane >> 5;
    const float* xs = x + (long long)n * V; const float* ys = y + (long long)n * V;
    const float cb = cen[b];
    const float bin_ok = b < p.bins ? 1.f : 0.f;      // a padding lane generates the (finite) weights of bin 0 times zero
    const long long ntiles = (V + kMiTile - 1) / kMiTile;
    double acc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0;
    f32x16 c0, c1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { c0[r] = 0.f; c1[r] = 0.f; }
    int since = 0;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long v = tile * kMiTile + wave * 64 + lane;
        const bool ok = v < V;
        // a voxel past the end has scale 0 (and a finite value): zero weight, not the weight of x = 0
        const float xv = mi_clamp(ok ? xs[v] : p.lo, p.lo, p.hi), yv = mi_clamp(ok ? ys[v] : p.lo, p.lo, p.hi);
        const f32x2 xy = {xv, yv};
        f32x2 sxy = {0.f, 0.f};
        for (int k = 0; k < p.bins; ++k) sxy += mi_gauss(xy - cen[k], p.negp);
        const float sc = ok ? 1.f / (sxy.x * sxy.y) : 0.f;
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const int src = 2 * s + h;
            const f32x2 va = {__shfl(xv, src), __shfl(yv, src)};
            const f32x2 scale = {__shfl(sc, src) * bin_ok, bin_ok};
            const f32x2 e = mi_gauss(va - cb, p.negp) * scale;
            if (s & 1) c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(e.x, e.y, c1, 0, 0, 0);
            else c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(e.x, e.y, c0, 0, 0, 0);
        }
        if (++since == kMiFlush) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[r] += (double)c0[r] + (double)c1[r]; c0[r] = 0.f; c1[r] = 0.f; }
            since = 0;
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] += (double)c0[r] + (double)c1[r];
    // accumulator register r of lane l is P[i][j], i = (r & 3) + 8 (r >> 2) + 4 (l >> 5), j = l & 31; the waves add in wave order
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
                if (w == 0) comb[i * 32 + b] = acc[r]; else comb[i * 32 + b] += acc[r];
            }
        }
        __syncthreads();
    }
    double* out = partial + ((size_t)n * gridDim.x + blockIdx.x) * 1024;
    for (int e = threadIdx.x; e < 1024; e += 256) out[e] = comb[e];
}

// psum[n][e] = sum_b partial[n][b][e]: 64 consecutive entries x 4 interleaved slices of the partial list per workgroup, slices added in order
__global__ void __launch_bounds__(256) mi_reduce_kernel(const double* __restrict__ partial, int nblocks, double* __restrict__ psum) {
    __shared__ double red[4][64];
    const int n = blockIdx.y, e = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
    const double* src = partial + (size_t)n * nblocks * 1024 + e;
    double s = 0.0;
#pragma unroll 4
    for (int bk = q; bk < nblocks; bk += 4) s += src[(size_t)bk * 1024];
    red[q][threadIdx.x & 63] = s;
    __syncthreads();
    if (q == 0) psum[(size_t)n * 1024 + e] = da_sum4(red, threadIdx.x);
}

// one workgroup of 1024 threads, thread (i, j); samples one after the other.  stats[n] = G[32][32] | ga[32] | gb[32] | MI, 0...
__global__ void __launch_bounds__(1024) mi_finalize_kernel(const double* __restrict__ psum, int N, long long V, int bins,
                                                           float* __restrict__ loss, float* __restrict__ stats) {
    __shared__ double Pm[32][33], Hm[32][33], a[32], bm[32], red[1024];
    const int t = threadIdx.x, i = t >> 5, j = t & 31;
    const bool in = i < bins && j < bins;
    double total = 0.0;
    for (int n = 0; n < N; ++n) {
        const double P = in ? psum[(size_t)n * 1024 + t] / (double)V : 0.0;
        Pm[i][j] = P;
        __syncthreads();
        if (t < 32) { double s = 0.0; for (int k = 0; k < 32; ++k) s += Pm[t][k]; a[t] = s; }
        else if (t < 64) { double s = 0.0; for (int k = 0; k < 32; ++k) s += Pm[k][t - 32]; bm[t - 32] = s; }
        __syncthreads();
        double term = 0.0, G = 0.0, H = 0.0;
        if (in) {
            const double Q = a[i] * bm[j] + 1e-6, R = P / Q + 1e-6, lr = log(R);
            term = P * lr; G = lr + P / (R * Q); H = -(P * P) / (R * Q * Q);
        }
        Hm[i][j] = H; red[t] = term;
        __syncthreads();
        for (int o = 512; o > 0; o >>= 1) { if (t < o) red[t] += red[t + o]; __syncthreads(); }
        float* st = stats + (size_t)n * kMiStats;
        st[t] = (float)G;
        if (t < 32) { double s = 0.0; for (int k = 0; k < 32; ++k) s += Hm[t][k] * bm[k]; st[1024 + t] = (float)s; }
        else if (t < 64) { double s = 0.0; for (int k = 0; k < 32; ++k) s += Hm[k][t - 32] * a[k]; st[1056 + t - 32] = (float)s; }
        else if (t < 72) st[1088 + t - 64] = t == 64 ? (float)red[0] : 0.f;
        if (t == 0) total += red[0];
        __syncthreads();
    }
    if (t == 0) loss[0] = (float)(-total / (double)N);
}

__global__ void __launch_bounds__(256) mi_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ stats,
                                                     const float* __restrict__ dloss, float* __restrict__ dx, float* __restrict__ dy,
                                                     int N, long long V, MiP p) {
    const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int vl = lane & 31, h = lane >> 5;
    const float* xs = x + (long long)n * V; const float* ys = y + (long long)n * V;
    const float* st = stats + (size_t)n * kMiStats;
    const float gs = -dloss[0] / ((float)N * (float)V);
    // step t of this half contracts bin jb(t) = 4 h + (t & 3) + 8 (t >> 2): the accumulator's row of register t
    float Ga[16], Gt[16], cbin[16], ga[16], gb[16];
    bool okb[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int jb = 4 * h + (t & 3) + 8 * (t >> 2);
        Ga[t] = st[vl * 32 + jb];               // A[i = vl][k] = G[vl][jb]
        Gt[t] = st[jb * 32 + vl];               // A[i = vl][k] = G^T[vl][jb]
        okb[t] = jb < p.bins;
        cbin[t] = mi_centre(p, okb[t] ? jb : 0);
        ga[t] = st[1024 + jb]; gb[t] = st[1056 + jb];
    }
    const float d2 = 2.f * p.negp;              // d_i = -2 p (xh - c_i)
    const long long ntiles = (V + 31) / 32;
    for (long long tile = (long long)blockIdx.x * 4 + wave; tile < ntiles; tile += (long long)gridDim.x * 4) {
        const long long v = tile * 32 + vl;
        const bool ok = v < V;
        const float xr = ok ? xs[v] : p.lo, yr = ok ? ys[v] : p.lo;
        const float xv = mi_clamp(xr, p.lo, p.hi), yv = mi_clamp(yr, p.lo, p.hi);
        float wx[16], wy[16], ddx[16], ddy[16];
        float sx = 0.f, sy = 0.f;
        const f32x2 xy = {xv, yv};
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const f32x2 d = xy - cbin[t], e = mi_gauss(d, p.negp);
            ddx[t] = d.x; ddy[t] = d.y;
            wx[t] = okb[t] ? e.x : 0.f;
            wy[t] = okb[t] ? e.y : 0.f;
            sx += wx[t]; sy += wy[t];
        }
        sx += __shfl_xor(sx, 32); sy += __shfl_xor(sy, 32);
        const float ix = 1.f / sx, iy = 1.f / sy;
        f32x16 ux, uy;
#pragma unroll
        for (int t = 0; t < 16; ++t) { wx[t] *= ix; wy[t] *= iy; ux[t] = ga[t]; uy[t] = gb[t]; }
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            ux = __builtin_amdgcn_mfma_f32_32x32x2f32(Ga[t], wy[t], ux, 0, 0, 0);
            uy = __builtin_amdgcn_mfma_f32_32x32x2f32(Gt[t], wx[t], uy, 0, 0, 0);
        }
        float mx = 0.f, my = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) { mx += wx[t] * ux[t]; my += wy[t] * uy[t]; }
        mx += __shfl_xor(mx, 32); my += __shfl_xor(my, 32);
        float gx = 0.f, gy = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) { gx += wx[t] * ddx[t] * (ux[t] - mx); gy += wy[t] * ddy[t] * (uy[t] - my); }
        gx += __shfl_xor(gx, 32); gy += __shfl_xor(gy, 32);
        if (ok && h == 0) {
            // the clamp's derivative: zero outside (vmin, vmax); a NaN voxel keeps its NaN
            if (dx) dx[(long long)n * V + v] = (xr <= p.lo || xr >= p.hi) ? 0.f : gs * d2 * gx;
            if (dy) dy[(long long)n * V + v] = (yr <= p.lo || yr >= p.hi) ? 0.f : gs * d2 * gy;
        }
    }
}

static bool mi_args_ok(int N, long long V, int bins, float vmin, float vmax, float sigma_ratio) {
    return N > 0 && V > 0 && bins >= 2 && bins <= 32 && vmin < vmax && sigma_ratio > 0.f && vmin - vmin == 0.f && vmax - vmax == 0.f && sigma_ratio - sigma_ratio == 0.f;
}
static MiP mi_params(int bins, float vmin, float vmax, float sigma_ratio) {
    MiP p;
    p.vmin = (double)vmin; p.delta = ((double)vmax - (double)vmin) / (double)(bins - 1);
    const double sigma = p.delta * (double)sigma_ratio;
    p.lo = vmin; p.hi = vmax; p.negp = (float)(-1.0 / (2.0 * sigma * sigma)); p.bins = bins;
    return p;
}
static int mi_blocks(long long V) {
    const long long ntiles = (V + kMiTile - 1) / kMiTile;
    long long nb = (ntiles + 1) / 2;
    if (nb > kMiMaxBlocks) nb = kMiMaxBlocks;
    return (int)(nb < 1 ? 1 : nb);
}

}  // namespace

// per-workgroup joint histograms [N][blocks][32 x 32], then their sum per sample
struct MiWs { double *partial, *psum; size_t bytes; };
static MiWs mi_layout(int N, long long V, void* ws) { DaCarve c(ws); return MiWs{c.take<double>((size_t)N * mi_blocks(V) * 1024), c.take<double>((size_t)N * 1024), c.off}; }
extern "C" size_t da_mi_ws_bytes(int N, long long V, int bins) {
    if (N <= 0 || V <= 0 || bins < 2 || bins > 32) return 0;
    return mi_layout(N, V, nullptr).bytes;
}

extern "C" int da_mi_fwd(const float* x, const float* y, int N, long long V, int bins, float vmin, float vmax, float sigma_ratio,
                         float* loss, float* stats, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !y || !loss || !stats || !ws || !mi_args_ok(N, V, bins, vmin, vmax, sigma_ratio) || N > 65535) return DA_ERR_BADARG;
    if (ws_bytes < da_mi_ws_bytes(N, V, bins)) return DA_ERR_WS_SMALL;
    hipStream_t st = da_stream(stream);
    const MiP p = mi_params(bins, vmin, vmax, sigma_ratio);
    const int nb = mi_blocks(V);
    const auto [partial, psum, need] = mi_layout(N, V, ws);
    hipLaunchKernelGGL(mi_partial_kernel, dim3(nb, N), dim3(256), 0, st, x, y, V, p, partial);
    DA_LAUNCH_CHECK();
    hipLaunchKernelGGL(mi_reduce_kernel, dim3(16, N), dim3(256), 0, st, (const double*)partial, nb, psum);
    DA_LAUNCH_CHECK();
    hipLaunchKernelGGL(mi_finalize_kernel, dim3(1), dim3(1024), 0, st, (const double*)psum, N, V, bins, loss, stats);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_mi_bwd(const float* x, const float* y, const float* stats, const float* dloss, float* dx, float* dy,
                         int N, long long V, int bins, float vmin, float vmax, float sigma_ratio, void* stream) {
    if (!x || !y || !stats || !dloss || !mi_args_ok(N, V, bins, vmin, vmax, sigma_ratio) || N > 65535) return DA_ERR_BADARG;
    if (!dx && !dy) return 0;
    const MiP p = mi_params(bins, vmin, vmax, sigma_ratio);
    const long long ntiles = (V + 31) / 32;
    long long nb = (ntiles + 3) / 4;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(mi_bwd_kernel, dim3((unsigned)nb, N), dim3(256), 0, da_stream(stream), x, y, stats, dloss, dx, dy, N, V, p);
    DA_LAUNCH_CHECK();
    return 0;
}
