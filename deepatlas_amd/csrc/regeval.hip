// Registration evaluation: nearest-neighbour label warp fused with the integer overlap counts (the DeepAtlas registration Dice: warp the moving
// segmentation with the predicted deformation, overlap it with the target segmentation), and the Jacobian determinant of the deformation with
// its per-sample statistics (folding fraction).  The reference has neither metric (README.md:15-19 lists registration as TODO); the deformation
// is the one its registration net builds: deform = disp + identity, sampled with align_corners=True (voxel_morph.py:85-91, lib/utils.py:89-102).
// NDHWC: disp[N][D][H][W][3], channel order (x, y, z) = (W, H, D) axis, normalised units, identity generated in-kernel.
// Multi-atlas label fusion (registration-based segmentation: K atlas label maps warped with K such fields and voted per voxel) and the
// weights of locally weighted voting share the nearest-coordinate routine and live here too.
#include "common.h"

namespace {

constexpr int kJacBlocks = 2048;   // Jacobian partial blocks per sample (multiple of 8: XCD-contiguous split)
constexpr int kJacStats = 5;       // per-block partials: sum(det - 1), sum((det - 1)^2), min, max, #(det <= 0)

// index of the moving voxel the target voxel (d, h, w) reads, or -1 (outside the volume, or a non-finite coordinate): the training warp's
// own coordinate (da_id_coord / da_unnormalize, common.h), every axis rounded half-to-even (rintf in the default rounding mode = ATen's
// nearbyint), then the bounds test of padding_mode='zeros'.  (The finiteness test is da_is_finite_coord's, written out: the call gave the
// fusion kernels another register allocation.)
__device__ __forceinline__ int nearest_source(float ux, float uy, float uz, int d, int h, int w, int D, int H, int W) {
    const float gx = ux + da_id_coord(w, W), gy = uy + da_id_coord(h, H), gz = uz + da_id_coord(d, D);
    if (!(fabsf(gx) < 1e9f && fabsf(gy) < 1e9f && fabsf(gz) < 1e9f)) return -1;      // NaN / inf: reads 0
    const float x = rintf(da_unnormalize(gx, W)), y = rintf(da_unnormalize(gy, H)), z = rintf(da_unnormalize(gz, D));
    if (!(x >= 0.f && x <= (float)(W - 1) && y >= 0.f && y <= (float)(H - 1) && z >= 0.f && z <= (float)(D - 1))) return -1;
    return ((int)z * H + (int)y) * W + (int)x;
}

// Each thread takes RUN consecutive target voxels: their displacement is 3 x 16 bytes, their target labels and warped labels 4 bytes when the
// layout allows (VEC), and runs of equal (warped, target) pairs are merged in registers before the per-wave LDS histograms are touched, as in
// label_overlap_counts_kernel (losses.hip).  One 64-bit global atomic per (workgroup, class, kind) at the end: integer counts, exact and
// independent of the order.  The runs are dealt out XCD-contiguously (da_xcd_loop): a target neighbourhood gathers its moving labels through one L2.
template <bool VEC, bool COUNTS>
__global__ void __launch_bounds__(256)
warp_nearest_counts_kernel(const void* __restrict__ lab_m, int m_bytes, const void* __restrict__ lab_t, int t_bytes,
                           const float* __restrict__ disp, int D, int H, int W, int C,
                           unsigned long long* __restrict__ counts, unsigned char* __restrict__ warped) {
    extern __shared__ unsigned int shc[];   // [4 waves][3][C]
    constexpr int RUN = 4;
    const int n = blockIdx.y;
    const int V = D * H * W;
    if (COUNTS) {
        for (int c = threadIdx.x; c < 4 * 3 * C; c += blockDim.x) shc[c] = 0u;
        __syncthreads();
    }
    unsigned int* hist = shc + (threadIdx.x >> 6) * 3 * C;
    auto flush = [&](int pl, int tl, unsigned int len) {
        if (len == 0u) return;
        if (pl >= 0 && pl < C) atomicAdd(&hist[pl], len);
        if (tl >= 0 && tl < C) atomicAdd(&hist[C + tl], len);
        if (pl == tl && pl >= 0 && pl < C) atomicAdd(&hist[2 * C + pl], len);
    };
    const long long sample = (long long)n * V;
    const float* u = disp + sample * 3;
    const int nruns = (V + RUN - 1) / RUN;
    for (DaXcdLoop L = da_xcd_loop(nruns, 64); L.i < L.end; L.i += L.step) {
        const int v0 = (int)L.i * RUN;
        const int cnt = (V - v0) < RUN ? (V - v0) : RUN;
        float uu[RUN * 3];
        if (VEC) {
            const float4* q = reinterpret_cast<const float4*>(u + (long long)v0 * 3);
            const float4 a = q[0], b = q[1], c = q[2];
            uu[0] = a.x; uu[1] = a.y; uu[2] = a.z; uu[3] = a.w; uu[4] = b.x; uu[5] = b.y; uu[6] = b.z; uu[7] = b.w;
            uu[8] = c.x; uu[9] = c.y; uu[10] = c.z; uu[11] = c.w;
        } else {
#pragma unroll
            for (int k = 0; k < RUN * 3; ++k) uu[k] = (k < cnt * 3) ? u[(long long)v0 * 3 + k] : 0.f;
        }
        int d, h, w; da_vox3(v0, H, W, d, h, w);
        int src[RUN];
#pragma unroll
        for (int k = 0; k < RUN; ++k) {
            src[k] = (k < cnt) ? nearest_source(uu[3 * k], uu[3 * k + 1], uu[3 * k + 2], d, h, w, D, H, W) : -1;
            if (++w == W) { w = 0; if (++h == H) { h = 0; ++d; } }
        }
        unsigned char m[RUN];
#pragma unroll
        for (int k = 0; k < RUN; ++k)      // (the RUN gathers are independent: issued back to back)
            m[k] = src[k] >= 0 ? (unsigned char)da_load_label(lab_m, m_bytes, sample + src[k]) : (unsigned char)0;
        if (warped) {
            if (VEC) {
                *reinterpret_cast<uchar4*>(warped + sample + v0) = make_uchar4(m[0], m[1], m[2], m[3]);
            } else {
#pragma unroll
                for (int k = 0; k < RUN; ++k) if (k < cnt) warped[sample + v0 + k] = m[k];
            }
        }
        if (COUNTS) {
            int t[RUN];
            if (VEC && t_bytes == 1) {
                const uchar4 tt = *reinterpret_cast<const uchar4*>((const unsigned char*)lab_t + sample + v0);
                t[0] = tt.x; t[1] = tt.y; t[2] = tt.z; t[3] = tt.w;
            } else {
#pragma unroll
                for (int k = 0; k < RUN; ++k) t[k] = (k < cnt) ? (int)da_load_label(lab_t, t_bytes, sample + v0 + k) : -1;
            }
            int pl = -1, tl = -1; unsigned int len = 0u;
#pragma unroll
            for (int k = 0; k < RUN; ++k) {
                if (k < cnt) {
                    const int a = (int)m[k], b = t[k];
                    if (a != pl || b != tl) { flush(pl, tl, len); pl = a; tl = b; len = 0u; }
                    ++len;
                }
            }
            flush(pl, tl, len);
        }
    }
    if (COUNTS) {
        __syncthreads();
        for (int c = threadIdx.x; c < 3 * C; c += blockDim.x) {
            const unsigned int s = shc[c] + shc[3 * C + c] + shc[6 * C + c] + shc[9 * C + c];
            const int k = c / C, cc = c % C;
            if (s) atomicAdd(&counts[((size_t)n * C + cc) * 3 + k], (unsigned long long)s);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Jacobian determinant of x -> x + u(x), u_c = disp_c (size_c - 1) / 2 in voxels; numpy.gradient differences with unit spacing (central
// inside, one-sided on the faces), determinant by cofactor expansion in fp32.  A direct 6-neighbour gather like bending_bwd_kernel: the
// voxels are dealt out XCD-contiguously so that the +-1 plane neighbours are found in the XCD's own L2.  Statistics: per-thread doubles ->
// wave butterfly -> the four waves in order -> one partial row per workgroup; jacobian_finalize_kernel adds the rows in index order.
// No atomics anywhere: two runs are bit-identical.  The sums are taken of det - 1 (exact in double), so that the variance of a
// nearly-rigid field does not cancel.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
jacobian_det_kernel(const float* __restrict__ disp, int D, int H, int W, float* __restrict__ det_out, double* __restrict__ partial) {
    __shared__ double red[4][kJacStats];
    const int n = blockIdx.y;
    const int V = D * H * W;
    const float* u = disp + (long long)n * V * 3;
    const float sx = da_vox_scale(W), sy = da_vox_scale(H), sz = da_vox_scale(D);
    double s1 = 0.0, s2 = 0.0, cnt = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (DaXcdLoop L = da_xcd_loop(V, 256); L.i < L.end; L.i += L.step) {
        const int v = (int)L.i;
        int d, h, w; da_vox3(v, H, W, d, h, w);
        const float det = da_jac_det(da_jac_at(u + (long long)v * 3, d, h, w, D, H, W, sx, sy, sz));
        if (det_out) det_out[(long long)n * V + v] = det;
        const double e = (double)det - 1.0;
        s1 += e; s2 += e * e;
        mn = fminf(mn, det); mx = fmaxf(mx, det);
        if (det <= 0.f) cnt += 1.0;
    }
    s1 = da_wave_sum(s1); s2 = da_wave_sum(s2); cnt = da_wave_sum(cnt);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[wid][0] = s1; red[wid][1] = s2; red[wid][2] = (double)mn; red[wid][3] = (double)mx; red[wid][4] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* p = partial + ((size_t)n * gridDim.x + blockIdx.x) * kJacStats;
        p[0] = da_sum4(red, 0);
        p[1] = da_sum4(red, 1);
        p[2] = fmin(fmin(red[0][2], red[1][2]), fmin(red[2][2], red[3][2]));
        p[3] = da_max4(red, 3);
        p[4] = da_sum4(red, 4);
    }
}

// one wave per sample: lane l adds rows l, l + 64, ... in that order, then the fixed butterfly.  stats[n][8] =
// (sum det, sum det^2, min, max, #(det <= 0), mean, population variance, 0)
__global__ void jacobian_finalize_kernel(const double* __restrict__ partial, int nblocks, long long V, double* __restrict__ stats) {
    const int n = blockIdx.x, lane = threadIdx.x;
    double s1 = 0.0, s2 = 0.0, cnt = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int b = lane; b < nblocks; b += 64) {
        const double* p = partial + ((size_t)n * nblocks + b) * kJacStats;
        s1 += p[0]; s2 += p[1]; mn = fmin(mn, p[2]); mx = fmax(mx, p[3]); cnt += p[4];
    }
    s1 = da_wave_sum(s1); s2 = da_wave_sum(s2); cnt = da_wave_sum(cnt);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mn = fmin(mn, __shfl_xor(mn, o)); mx = fmax(mx, __shfl_xor(mx, o)); }
    if (lane == 0) {
        const double v = (double)V, m1 = s1 / v;
        double var = s2 / v - m1 * m1;
        if (var < 0.0) var = 0.0;
        double* o = stats + (size_t)n * 8;
        o[0] = s1 + v; o[1] = s2 + 2.0 * s1 + v; o[2] = mn; o[3] = mx; o[4] = cnt; o[5] = 1.0 + m1; o[6] = var; o[7] = 0.0;
    }
}

// ------------------------------------------------------------------------------------------------
// Multi-atlas label fusion: K atlas label maps warped to one target grid (the gather of warp_nearest_counts_kernel, coordinate by
// nearest_source) and voted per voxel.  A thread owns RUN = 4 consecutive target voxels; per atlas 3 x 16 bytes of displacement and four
// 1-byte gathers issued back to back.  The K labels of a voxel stay packed four to a register (and the K weights of the per-voxel form
// in registers): the kernel is instantiated per bucket KB in {4, 8, 16, 32} with every loop fully unrolled and a guard on k < K, so no
// array is indexed at run time and nothing goes to scratch.  Vote by comparing pairs: s_k = sum over m in atlas order of w_m [l_m = l_k]
// is the score of atlas k's class, added in fp32 exactly as the definition adds it (w = 1: integer counts); the winner is the largest
// score, ties to the smallest label; an absent atlas (k >= K) carries weight 0.  conf = winning score / sum_k w_k, (0, 0) for a zero total.
// WMODE 0: majority vote, 1: w_atlas[N][K], 2: w_voxel[N][K][V].  No atomics: two runs are bit-identical.
// ------------------------------------------------------------------------------------------------
// the vote of one voxel: pk = its K labels packed four to a register, wa / wv = the per-atlas / this voxel's per-voxel weights
template <int KB, int WMODE, int KW, int NA, int NV>
__device__ __forceinline__ void fusion_vote_one(const unsigned (&pk)[KW], const float (&wa)[NA], const float (&wv)[NV], int K,
                                                unsigned& best_lab, float& best_s, float& total) {
    unsigned lab[KB];
    float wt[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        lab[k] = (pk[k >> 2] >> ((k & 3) * 8)) & 0xFFu;
        wt[k] = WMODE == 0 ? (k < K ? 1.f : 0.f) : WMODE == 1 ? wa[k < NA ? k : 0] : wv[k < NV ? k : 0];
    }
    float tot = 0.f, bs = 0.f;
    unsigned bl = 0u;
#pragma unroll
    for (int k = 0; k < KB; ++k) tot += wt[k];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        if (k < K) {
            float s = 0.f;
#pragma unroll
            for (int m = 0; m < KB; ++m) s += (lab[m] == lab[k]) ? wt[m] : 0.f;
            if (s > bs || (s == bs && lab[k] < bl)) { bs = s; bl = lab[k]; }
        }
    }
    best_lab = bl; best_s = bs; total = tot;
}

template <int KB, int WMODE, bool VEC>
__global__ void __launch_bounds__(256)
label_fusion_vote_kernel(const void* __restrict__ labels, int label_bytes, long long label_sample_stride, const float* __restrict__ disp,
                         const float* __restrict__ w_atlas, const float* __restrict__ w_voxel, int K, int D, int H, int W,
                         unsigned char* __restrict__ fused, float* __restrict__ conf) {
    constexpr int RUN = 4;
    constexpr int KW = (KB + 3) / 4;         // registers of packed labels per voxel
    const int n = blockIdx.y;
    const int V = D * H * W;
    const long long nk0 = (long long)n * K;
    float wa[WMODE == 1 ? KB : 1];
    if (WMODE == 1) {
#pragma unroll
        for (int k = 0; k < KB; ++k) wa[k] = (k < K) ? w_atlas[nk0 + k] : 0.f;
    }
    const int nruns = (V + RUN - 1) / RUN;
    for (DaXcdLoop L = da_xcd_loop(nruns, 64); L.i < L.end; L.i += L.step) {
        const int v0 = (int)L.i * RUN;
        const int cnt = (V - v0) < RUN ? (V - v0) : RUN;
        int d0, h0, w0; da_vox3(v0, H, W, d0, h0, w0);
        unsigned pk[RUN][KW];
        float wv[WMODE == 2 ? RUN : 1][WMODE == 2 ? KB : 1];
#pragma unroll
        for (int j = 0; j < RUN; ++j)
#pragma unroll
            for (int q = 0; q < KW; ++q) pk[j][q] = 0u;
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            if (k < K) {
                const long long field = (nk0 + k) * (long long)V;                  // 64-bit: [N][K][V][3] passes 2^31 elements
                const float* u = disp + (field + v0) * 3;
                float uu[RUN * 3];
                if (VEC) {
                    const float4* q = reinterpret_cast<const float4*>(u);
                    const float4 a = q[0], b = q[1], c = q[2];
                    uu[0] = a.x; uu[1] = a.y; uu[2] = a.z; uu[3] = a.w; uu[4] = b.x; uu[5] = b.y; uu[6] = b.z; uu[7] = b.w;
                    uu[8] = c.x; uu[9] = c.y; uu[10] = c.z; uu[11] = c.w;
                } else {
#pragma unroll
                    for (int e = 0; e < RUN * 3; ++e) uu[e] = (e < cnt * 3) ? u[e] : 0.f;
                }
                int d = d0, h = h0, w = w0;
                int src[RUN];
#pragma unroll
                for (int j = 0; j < RUN; ++j) {
                    src[j] = (j < cnt) ? nearest_source(uu[3 * j], uu[3 * j + 1], uu[3 * j + 2], d, h, w, D, H, W) : -1;
                    if (++w == W) { w = 0; if (++h == H) { h = 0; ++d; } }
                }
                const long long lab0 = (long long)n * label_sample_stride + (long long)k * V;
                unsigned m[RUN];
#pragma unroll
                for (int j = 0; j < RUN; ++j)      // (independent gathers: issued back to back)
                    m[j] = src[j] >= 0 ? (unsigned)(unsigned char)da_load_label(labels, label_bytes, lab0 + src[j]) : 0u;
#pragma unroll
                for (int j = 0; j < RUN; ++j) pk[j][k >> 2] |= m[j] << ((k & 3) * 8);
                if (WMODE == 2) {
                    const float* wp = w_voxel + field + v0;
                    if (VEC) {
                        const float4 t = *reinterpret_cast<const float4*>(wp);
                        wv[0][k] = t.x; wv[1][k] = t.y; wv[2][k] = t.z; wv[3][k] = t.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < RUN; ++j) wv[j][k] = (j < cnt) ? wp[j] : 0.f;
                    }
                }
            } else if (WMODE == 2) {
#pragma unroll
                for (int j = 0; j < RUN; ++j) wv[j][k] = 0.f;
            }
        }
        // (one call per voxel, not a loop: a fully unrolled 4 x KB x KB body passes the unroller's size limit at KB = 32 and the arrays
        // would then be indexed at run time)
        unsigned best_lab[RUN];
        float best_s[RUN], total[RUN];
        fusion_vote_one<KB, WMODE>(pk[0], wa, wv[0], K, best_lab[0], best_s[0], total[0]);
        fusion_vote_one<KB, WMODE>(pk[1], wa, wv[WMODE == 2 ? 1 : 0], K, best_lab[1], best_s[1], total[1]);
        fusion_vote_one<KB, WMODE>(pk[2], wa, wv[WMODE == 2 ? 2 : 0], K, best_lab[2], best_s[2], total[2]);
        fusion_vote_one<KB, WMODE>(pk[3], wa, wv[WMODE == 2 ? 3 : 0], K, best_lab[3], best_s[3], total[3]);
        const long long o = (long long)n * V + v0;
        if (VEC) {
            *reinterpret_cast<uchar4*>(fused + o) = make_uchar4((unsigned char)best_lab[0], (unsigned char)best_lab[1], (unsigned char)best_lab[2], (unsigned char)best_lab[3]);
            if (conf) {
                float4 c;
                c.x = total[0] > 0.f ? best_s[0] / total[0] : 0.f; c.y = total[1] > 0.f ? best_s[1] / total[1] : 0.f;
                c.z = total[2] > 0.f ? best_s[2] / total[2] : 0.f; c.w = total[3] > 0.f ? best_s[3] / total[3] : 0.f;
                *reinterpret_cast<float4*>(conf + o) = c;
            }
        } else {
#pragma unroll
            for (int j = 0; j < RUN; ++j) {
                if (j < cnt) {
                    fused[o + j] = (unsigned char)best_lab[j];
                    if (conf) conf[o + j] = total[j] > 0.f ? best_s[j] / total[j] : 0.f;
                }
            }
        }
    }
}

template <int KB, int WMODE>
void launch_fusion_vote(bool vec, dim3 grid, hipStream_t st, const void* labels, int label_bytes, long long stride, const float* disp,
                        const float* w_atlas, const float* w_voxel, int K, int D, int H, int W, unsigned char* fused, float* conf) {
    if (vec) hipLaunchKernelGGL((label_fusion_vote_kernel<KB, WMODE, true>), grid, dim3(256), 0, st, labels, label_bytes, stride, disp, w_atlas, w_voxel, K, D, H, W, fused, conf);
    else hipLaunchKernelGGL((label_fusion_vote_kernel<KB, WMODE, false>), grid, dim3(256), 0, st, labels, label_bytes, stride, disp, w_atlas, w_voxel, K, D, H, W, fused, conf);
}

template <int WMODE>
void launch_fusion_vote_bucket(bool vec, dim3 grid, hipStream_t st, const void* labels, int label_bytes, long long stride, const float* disp,
                               const float* w_atlas, const float* w_voxel, int K, int D, int H, int W, unsigned char* fused, float* conf) {
    if (K <= 4) launch_fusion_vote<4, WMODE>(vec, grid, st, labels, label_bytes, stride, disp, w_atlas, w_voxel, K, D, H, W, fused, conf);
    else if (K <= 8) launch_fusion_vote<8, WMODE>(vec, grid, st, labels, label_bytes, stride, disp, w_atlas, w_voxel, K, D, H, W, fused, conf);
    else if (K <= 16) launch_fusion_vote<16, WMODE>(vec, grid, st, labels, label_bytes, stride, disp, w_atlas, w_voxel, K, D, H, W, fused, conf);
    else launch_fusion_vote<32, WMODE>(vec, grid, st, labels, label_bytes, stride, disp, w_atlas, w_voxel, K, D, H, W, fused, conf);
}

// ------------------------------------------------------------------------------------------------
// Weights of locally weighted voting: w = exp(-beta m), m = (2r+1)^-3 x the box sum of (warped - target)^2 over the (2r+1)^3 window,
// voxels outside the volume contributing 0.  Separable like the LNCC box sums (reglosses.hip box_axis_kernel): along W (the squared
// difference formed on the fly), along H, along D; each axis adds its 2r+1 terms directly in window order -- no sliding sum, so no
// cancellation.  STAGE 0 reads (warped, target) and sums along W; 1 sums along H; 2 sums along D, divides by the window size and takes
// expf.  Fields are [N K][D][H][W]; the voxels are dealt out XCD-contiguously so the +-r rows / planes are found in the XCD's own L2.
// ------------------------------------------------------------------------------------------------
template <int STAGE>
__global__ void __launch_bounds__(256)
msd_axis_kernel(const float* __restrict__ in, const float* __restrict__ target, float* __restrict__ out, long long total, int K,
                int D, int H, int W, int r, float n3, float beta) {
    const long long V = (long long)D * H * W;
    for (DaXcdLoop L = da_xcd_loop(total, 256); L.i < L.end; L.i += L.step) {
        const long long i = L.i;
        const long long f = i / V;                      // field (n, k)
        const int v = (int)(i - f * V);
        int d, h, w; da_vox3(v, H, W, d, h, w);
        float s = 0.f;
        if (STAGE == 0) {
            const float* a = in + i - w;                // row start
            const float* b = target + (f / K) * V + (v - w);
            const int lo = w - r < 0 ? 0 : w - r, hi = w + r > W - 1 ? W - 1 : w + r;
            for (int x = lo; x <= hi; ++x) { const float e = a[x] - b[x]; s += e * e; }
            out[i] = s;
        } else if (STAGE == 1) {
            const float* a = in + i - (long long)h * W;
            const int lo = h - r < 0 ? 0 : h - r, hi = h + r > H - 1 ? H - 1 : h + r;
            for (int y = lo; y <= hi; ++y) s += a[(long long)y * W];
            out[i] = s;
        } else {
            const long long HW = (long long)H * W;
            const float* a = in + i - (long long)d * HW;
            const int lo = d - r < 0 ? 0 : d - r, hi = d + r > D - 1 ? D - 1 : d + r;
            for (int z = lo; z <= hi; ++z) s += a[(long long)z * HW];
            out[i] = expf(-beta * (s / n3));
        }
    }
}

int jac_blocks(long long V) {
    long long g = da_cdiv(V, 256);
    if (g > kJacBlocks) g = kJacBlocks;
    if (g >= 8) g = g / 8 * 8;          // a multiple of 8 takes the XCD-contiguous split
    return (int)(g < 1 ? 1 : g);
}

}  // namespace

extern "C" int da_warp_labels_nearest_counts(const void* lab_m, int m_bytes, const void* lab_t, int t_bytes, const float* disp,
                                             int N, int D, int H, int W, int C, unsigned long long* counts, unsigned char* warped, void* stream) {
    if (!lab_m || !disp || (!counts && !warped) || N < 1 || D < 1 || H < 1 || W < 1 || (m_bytes != 1 && m_bytes != 8)) return DA_ERR_BADARG;
    if (counts && (!lab_t || C < 1 || C > 1024 || (t_bytes != 1 && t_bytes != 8))) return DA_ERR_BADARG;
    const long long V = (long long)D * H * W;
    if (V >= 0x7FFFFFFFLL / 4) return DA_ERR_UNSUPPORTED;                  // 32-bit voxel and element offsets inside a sample
    hipStream_t st = da_stream(stream);
    const long long nruns = (V + 3) / 4;
    int g = da_grid(da_cdiv(nruns, 2), 256, 2048);                          // two runs (8 voxels) per thread where the volume is large enough
    if (g >= 8) g = g / 8 * 8;
    // the 16-byte / 4-byte forms need every sample's first voxel aligned
    const bool vec = (V % 4 == 0) && (((size_t)disp & 15) == 0) && (!warped || ((size_t)warped & 3) == 0) &&
                     (!counts || t_bytes != 1 || ((size_t)lab_t & 3) == 0);
    const dim3 grid(g, N), block(256);
    if (counts) {
        const size_t lds = (size_t)4 * 3 * C * sizeof(unsigned int);
        if (vec) hipLaunchKernelGGL((warp_nearest_counts_kernel<true, true>), grid, block, lds, st, lab_m, m_bytes, lab_t, t_bytes, disp, D, H, W, C, counts, warped);
        else hipLaunchKernelGGL((warp_nearest_counts_kernel<false, true>), grid, block, lds, st, lab_m, m_bytes, lab_t, t_bytes, disp, D, H, W, C, counts, warped);
    } else {
        if (vec) hipLaunchKernelGGL((warp_nearest_counts_kernel<true, false>), grid, block, 0, st, lab_m, m_bytes, lab_t, t_bytes, disp, D, H, W, 0, counts, warped);
        else hipLaunchKernelGGL((warp_nearest_counts_kernel<false, false>), grid, block, 0, st, lab_m, m_bytes, lab_t, t_bytes, disp, D, H, W, 0, counts, warped);
    }
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t da_jacobian_det_ws_bytes(int N, int D, int H, int W) {
    (void)D; (void)H; (void)W;
    return da_align((size_t)(N > 0 ? N : 1) * kJacBlocks * kJacStats * sizeof(double));
}

extern "C" int da_jacobian_det(const float* disp, int N, int D, int H, int W, double* stats, float* det_out,
                               void* ws, size_t ws_bytes, void* stream) {
    if (!disp || !stats || !ws || N < 1 || D < 2 || H < 2 || W < 2) return DA_ERR_BADARG;
    if (ws_bytes < da_jacobian_det_ws_bytes(N, D, H, W)) return DA_ERR_WS_SMALL;
    const long long V = (long long)D * H * W;
    if (V >= 0x7FFFFFFFLL / 4) return DA_ERR_UNSUPPORTED;
    hipStream_t st = da_stream(stream);
    const int nblocks = jac_blocks(V);
    hipLaunchKernelGGL(jacobian_det_kernel, dim3(nblocks, N), dim3(256), 0, st, disp, D, H, W, det_out, (double*)ws);
    DA_LAUNCH_CHECK();
    hipLaunchKernelGGL(jacobian_finalize_kernel, dim3(N), dim3(64), 0, st, (const double*)ws, nblocks, V, stats);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_label_fusion_vote(const void* labels, int label_bytes, long long label_sample_stride, const float* disp,
                                    const float* w_atlas, const float* w_voxel, int N, int K, int D, int H, int W,
                                    unsigned char* fused, float* conf, void* stream) {
    if (!labels || !disp || !fused || N < 1 || K < 1 || D < 1 || H < 1 || W < 1 || (label_bytes != 1 && label_bytes != 8)) return DA_ERR_BADARG;
    if (w_atlas && w_voxel) return DA_ERR_BADARG;                          // one weight form at most
    const long long V = (long long)D * H * W;
    if (label_sample_stride != 0 && label_sample_stride < (long long)K * V) return DA_ERR_BADARG;      // shared maps, or one [K][V] block per target
    if (K > 32) return DA_ERR_UNSUPPORTED;
    if (V >= 0x7FFFFFFFLL / 4) return DA_ERR_UNSUPPORTED;                  // 32-bit voxel offsets inside a volume (field offsets are 64-bit)
    hipStream_t st = da_stream(stream);
    const long long nruns = (V + 3) / 4;
    int g = da_grid(da_cdiv(nruns, 2), 256, 2048);
    if (g >= 8) g = g / 8 * 8;
    const bool vec = (V % 4 == 0) && (((size_t)disp & 15) == 0) && (((size_t)fused & 3) == 0) && (!conf || ((size_t)conf & 15) == 0) &&
                     (!w_voxel || ((size_t)w_voxel & 15) == 0);
    const dim3 grid(g, N);
    if (w_voxel) launch_fusion_vote_bucket<2>(vec, grid, st, labels, label_bytes, label_sample_stride, disp, w_atlas, w_voxel, K, D, H, W, fused, conf);
    else if (w_atlas) launch_fusion_vote_bucket<1>(vec, grid, st, labels, label_bytes, label_sample_stride, disp, w_atlas, w_voxel, K, D, H, W, fused, conf);
    else launch_fusion_vote_bucket<0>(vec, grid, st, labels, label_bytes, label_sample_stride, disp, w_atlas, w_voxel, K, D, H, W, fused, conf);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t da_local_msd_weights_ws_bytes(int N, int K, int D, int H, int W) {
    const size_t n = (size_t)(N > 0 ? N : 1) * (size_t)(K > 0 ? K : 1) * (size_t)(D > 0 ? D : 1) * (size_t)(H > 0 ? H : 1) * (size_t)(W > 0 ? W : 1);
    return da_align(n * sizeof(float));
}

extern "C" int da_local_msd_weights(const float* warped, const float* target, int N, int K, int D, int H, int W, int radius, float beta,
                                    float* weights, void* ws, size_t ws_bytes, void* stream) {
    if (!warped || !target || !weights || !ws || N < 1 || K < 1 || D < 1 || H < 1 || W < 1 || radius < 1 || radius > 4 || !(beta >= 0.f))
        return DA_ERR_BADARG;
    if (ws_bytes < da_local_msd_weights_ws_bytes(N, K, D, H, W)) return DA_ERR_WS_SMALL;
    const long long V = (long long)D * H * W;
    if (V >= 0x7FFFFFFFLL / 4) return DA_ERR_UNSUPPORTED;
    hipStream_t st = da_stream(stream);
    const long long total = (long long)N * K * V;
    int g = da_grid(total, 256, 4096);
    if (g >= 8) g = g / 8 * 8;
    const int F = 2 * radius + 1;
    float* tmp = (float*)ws;
    hipLaunchKernelGGL(msd_axis_kernel<0>, dim3(g), dim3(256), 0, st, warped, target, weights, total, K, D, H, W, radius, 0.f, 0.f);
    DA_LAUNCH_CHECK();
    hipLaunchKernelGGL(msd_axis_kernel<1>, dim3(g), dim3(256), 0, st, (const float*)weights, (const float*)nullptr, tmp, total, K, D, H, W, radius, 0.f, 0.f);
    DA_LAUNCH_CHECK();
    hipLaunchKernelGGL(msd_axis_kernel<2>, dim3(g), dim3(256), 0, st, (const float*)tmp, (const float*)nullptr, weights, total, K, D, H, W, radius, (float)(F * F * F), beta);
    DA_LAUNCH_CHECK();
    return 0;
}
