// Nearest x2 up-sampling folded into the 3x3x3 convolution that consumes it (the registration decoder: voxel_morph.py:72-80,
// `F.interpolate(x, size=skip.shape)` followed by modules.convBlock), split matrix mode.
//
// U[u] = S[u >> 1] (exact x2, every axis even) and Y[u] = b + sum_{t in {0,1,2}^3} U[u + t - 1] . W[t].  A fine voxel u = 2 c + p only
// ever sees the 2 x 2 x 2 coarse voxels c + p + j - 1 (j in {0,1}^3), so per output parity class p the layer is a 2 x 2 x 2-tap
// convolution ON THE COARSE GRID with pre-summed weights (per axis: p 0: j 0 <- W[0], j 1 <- W[1] + W[2];  p 1: j 0 <- W[0] + W[1],
// j 1 <- W[2]):   Y[2 c + p] = b + sum_j S[c + p + j - 1] . Weff[p][j].
// 64 tap evaluations per coarse voxel instead of 216, and neither the up-sampled tensor (8 x the source) nor its gradient ever exists:
//   forward   8 classes x 8 taps from one coarse halo tile (4 x 6 x 18 voxels per 8-channel chunk); a wave owns two classes and all
//             8 M-tiles of the 2 x 4 x 16 coarse tile (= 4 x 8 x 32 fine outputs per workgroup), bias + ReLU fused, two source tensors
//             (the decoder's concat of two up-sampled tensors, voxel_morph.py:74,76) as two pointers;
//   dgrad     dS[c] = sum_{f in {-1..2}^3} dY[2 c + f] . K4[f]: the adjoint is ONE stride-2 convolution with a 4 x 4 x 4 kernel of summed
//             weights (per axis f -1 <- W[2], 0 <- W[1] + W[2], 1 <- W[0] + W[1], 2 <- W[0]) over the fine gradient: the 8-to-1
//             reduction of the up-sampling's backward happens inside the K loop.  Fine halo tile 6 x 10 x 34 per 8-channel chunk, x
//             de-interleaved by parity as in conv3d_s2n.hip;
//   wgrad     G[p][j] = sum_c S[c + p + j - 1]^T dY[2 c + p] (64 small GEMMs over COARSE voxels, one workgroup column per class p), then
//             dW[t] = sum of the 8 (p, j) pairs that contain tap t, folded into the fixed-order double-precision partial reduction.
// The weight sums are formed in double and rounded to fp32 once (one extra rounding per weight, the size of one fp32 product rounding),
// then scaled and split into two fp16 planes like every other split-mode operand (split_f16.h; conv3d_mfma.hip "SP": per-tile power-of-two
// scales for activations / gradients, per-chunk scales for the summed weights, accumulators rescaled by exact factors between chunks).
#include "common.h"
#include "conv3d_internal.h"
#include "split_f16.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int CTZ = 2, CTY = 4, CTX = 16;                       // coarse tile
constexpr int SZ = CTZ + 2, SY = CTY + 2, SX = CTX + 2;         // coarse halo of the forward / weight gradient: 4 x 6 x 18
constexpr int SV = SZ * SY * SX;                                // 432 voxels
constexpr int SPLANE_B = SV * 16;                               // bytes per plane of one 8-channel chunk
constexpr int S_NIT = (SV * 2 + 255) / 256;                     // 4 staging iterations (two 16-byte quads per voxel)

constexpr int NPLN = 2;                                         // operand planes (h, l)

// per axis: original taps that feed coarse tap j of parity p (forward / weight gradient)
__host__ __device__ inline int up_taps_of(int p, int j, int* t) {
    if (p == 0) { if (j == 0) { t[0] = 0; return 1; } t[0] = 1; t[1] = 2; return 2; }
    if (j == 0) { t[0] = 0; t[1] = 1; return 2; }
    t[0] = 2; return 1;
}
// per axis: original taps summed into the adjoint's tap f = fi - 1 (fi 0..3)
__host__ __device__ inline int up_taps_of_f(int fi, int* t) {
    if (fi == 0) { t[0] = 2; return 1; }
    if (fi == 1) { t[0] = 1; t[1] = 2; return 2; }
    if (fi == 2) { t[0] = 0; t[1] = 1; return 2; }
    t[0] = 0; return 1;
}

// ------------------------------------------------------------------------------------------------------------------------------
// coarse halo staging (forward, weight gradient): 432 voxels x 8 channels
// ------------------------------------------------------------------------------------------------------------------------------
struct SMap {
    int hv[S_NIT]; int c4;
    __device__ __forceinline__ void init() {
        c4 = (int)threadIdx.x & 1;
#pragma unroll
        for (int it = 0; it < S_NIT; ++it) { const int v = ((int)threadIdx.x + it * 256) >> 1; hv[it] = v < SV ? v : -1; }
    }
    __device__ __forceinline__ unsigned offset(int it, int zb, int yb, int xb, int D, int H, int W, int Cs, int choff) const {
        const int v = hv[it];
        const int hx = v % SX, t = v / SX, hy = t % SY, hz = t / SY;
        const int z = zb + hz, y = yb + hy, x = xb + hx;
        const bool inb = v >= 0 && (unsigned)z < (unsigned)D && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        return inb ? (unsigned)((((z * H + y) * W + x) * Cs + choff + c4 * 4) * 4) : 0xFFFFFFFFu;
    }
    __device__ __forceinline__ void write(unsigned char* lds, const float4* pre, const float scale) const {
#pragma unroll
        for (int it = 0; it < S_NIT; ++it) {
            if (hv[it] >= 0) da_split_store4(pre[it], scale, reinterpret_cast<uint2*>(lds) + hv[it] * 2 + c4, SPLANE_B / 8);
        }
    }
};

// ------------------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------------------
struct FwdP {
    const float* s1; const float* s2; int C1, C2;
    const unsigned char* wp; const int* wexp; const float* bias; float* out;
    int N, Dc, Hc, Wc, Cout, ntz, nty, ntx, nchunks, NTall;
    float slope;
};

// Scale exponent of a chunk of SUMMED weights from the largest original |w| of the chunk: a sum has at most 8 terms, so 8 max|w| bounds it
// (the three bits of headroom this costs come out of the 18 spare binades of the two-term split).
__device__ __forceinline__ int up_sum_exp(float maxw) { return da_scale_exp(maxw * 8.f); }

// packed B operand: [chunk][class][step 2][N-tile][plane][lane][8]; lane (g, n): coarse tap 4 step + g, cin chunk * 8 + e, cout 16 nt + n.
// Grid (chunks, PY): every workgroup of a chunk finds the chunk's largest |w| (scale exponent -> wexp[chunk]) and packs its share.
__global__ void __launch_bounds__(256) up_pack_fwd_kernel(const float* __restrict__ w, unsigned short* __restrict__ wp, int* __restrict__ wexp, int Cin, int Cout, int NT) {
    __shared__ float red[4];
    const int ch = blockIdx.x;
    float m = 0.f;
    for (int idx = threadIdx.x; idx < 27 * 8 * Cout; idx += 256) { const int co = idx % Cout, r = idx / Cout; m = fmaxf(m, fabsf(w[((size_t)(r >> 3) * Cin + ch * 8 + (r & 7)) * Cout + co])); }
    const int ew = up_sum_exp(da_block_max4(m, red, (int)threadIdx.x >> 6, (int)threadIdx.x & 63));
    if (blockIdx.y == 0 && threadIdx.x == 0) wexp[ch] = ew;
    const float sc = da_pow2(ew);
    const int units = 16 * NT * 64;                              // (class, step, N-tile, lane)
    for (int u = blockIdx.y * 256 + threadIdx.x; u < units; u += gridDim.y * 256) {
        const int lane = u & 63, nt = (u >> 6) % NT, cs = (u >> 6) / NT, s = cs & 1, cls = cs >> 1;
        const int g = lane >> 4, n = lane & 15;
        const int jt = 4 * s + g, co = nt * 16 + n;
        int tz[2], ty[2], tx[2];
        const int nz = up_taps_of((cls >> 2) & 1, (jt >> 2) & 1, tz), ny = up_taps_of((cls >> 1) & 1, (jt >> 1) & 1, ty), nx = up_taps_of(cls & 1, jt & 1, tx);
        float v[8];
        int toff[8];                                             // the (up to) eight folded taps; an absent one re-reads a present tap and adds nothing
#pragma unroll
        for (int j = 0; j < 8; ++j) { const int a = j >> 2, b = (j >> 1) & 1, c = j & 1; toff[j] = tz[a < nz ? a : 0] * 9 + ty[b < ny ? b : 0] * 3 + tx[c < nx ? c : 0]; }
        const int coc = co < Cout ? co : Cout - 1;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ci = ch * 8 + e, cic = ci < Cin ? ci : Cin - 1;
            float t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = w[((size_t)toff[j] * Cin + cic) * Cout + coc];
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < 8; ++j) { const int a = j >> 2, b = (j >> 1) & 1, c = j & 1; if (a < nz && b < ny && c < nx) acc += (double)t[j]; }
            v[e] = (ci < Cin && co < Cout) ? (float)acc : 0.f;
        }
        da_split_store8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), sc, reinterpret_cast<uint4*>(wp + ((size_t)(((ch * 8 + cls) * 2 + s) * NT + nt) * NPLN) * 512) + lane, 64);
    }
}

template <int NT>
__global__ void __launch_bounds__(256, 2) up_fwd_kernel(FwdP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = lane & 15, g = lane >> 4, q = lane & 3, a4 = (lane & 15) >> 2;
    const int nt0 = blockIdx.y * NT;
    int n, tz, ty, tx;
    da_tile_zyx(da_xcd_item_of_block(blockIdx.x, gridDim.x), p.ntz, p.nty, p.ntx, n, tz, ty, tx);
    const int z0 = tz * CTZ, y0 = ty * CTY, x0 = tx * CTX;
    const long long vox = (long long)p.Dc * p.Hc * p.Wc;
    const __amdgpu_buffer_rsrc_t r1 = da_rsrc(p.s1 + (long long)n * vox * p.C1, (unsigned)(vox * p.C1 * sizeof(float)));
    const __amdgpu_buffer_rsrc_t r2 = da_rsrc(p.C2 ? p.s2 + (long long)n * vox * p.C2 : p.s1, (unsigned)(p.C2 ? vox * p.C2 * sizeof(float) : 0));
    const __amdgpu_buffer_rsrc_t rsw = da_rsrc(p.wp, (unsigned)((size_t)p.nchunks * 16 * p.NTall * NPLN * 1024));
    SMap sm; sm.init();
    float4 pre[S_NIT];
    auto issue = [&](int ch) {
        const int cb = ch * 8;
        const bool first = cb < p.C1;
#pragma unroll
        for (int it = 0; it < S_NIT; ++it)
            pre[it] = da_buf_load4(first ? r1 : r2, sm.offset(it, z0 - 1, y0 - 1, x0 - 1, p.Dc, p.Hc, p.Wc, first ? p.C1 : p.C2, first ? cb : cb - p.C1));
    };
    auto ld = [&](int off) -> f16x8 { return *reinterpret_cast<const f16x8*>(lds + off); };
    // scale bookkeeping (DaSplitScale)
    float* smax = reinterpret_cast<float*>(lds + NPLN * SPLANE_B);
    DaSplitScale sc;
    auto stage = [&](int ch) -> int {                            // publish the tile's largest magnitude, barrier, split + write; returns the chunk's E
        const float m = da_block_max4(stage_absmax<S_NIT>(pre), smax, wave, lane);
        const int ew = p.wexp[ch];
        const int E = sc.admit(da_scale_exp(m) + ew, ch == 0);
        sm.write(lds, pre, da_pow2(E - ew));
        return E;
    };
    f32x4 acc[2][CTZ * CTY][NT];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int m = 0; m < CTZ * CTY; ++m)
#pragma unroll
            for (int nn = 0; nn < NT; ++nn) acc[c][m][nn] = (f32x4){0.f, 0.f, 0.f, 0.f};
    issue(0);
    int Ecur = stage(0);
    __syncthreads();
#pragma unroll 1
    for (int ch = 0; ch < p.nchunks; ++ch) {
        const bool more = ch + 1 < p.nchunks;
        if (more) issue(ch + 1);
        {
            const float f = sc.enter(Ecur);                      // the running sums into this chunk's unit (exact)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int m = 0; m < CTZ * CTY; ++m)
#pragma unroll
                    for (int nn = 0; nn < NT; ++nn) acc[c][m][nn] = acc[c][m][nn] * f;
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int cls = 2 * wave + c;
            const int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int jt = 4 * s + g;                        // this lane group's coarse tap
                const int abase = (((pz + ((jt >> 2) & 1)) * SY + py + ((jt >> 1) & 1)) * SX + px + (jt & 1) + i) * 16;
                f16x8 B[NT][NPLN];
#pragma unroll
                for (int nn = 0; nn < NT; ++nn)
#pragma unroll
                    for (int pl = 0; pl < NPLN; ++pl)
                        B[nn][pl] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rsw, (unsigned)lane * 16u,
                                        (unsigned)(((((ch * 8 + cls) * 2 + s) * p.NTall + nt0 + nn) * NPLN + pl) * 1024), 0));
#pragma unroll
                for (int mz = 0; mz < CTZ; ++mz) {
                    f16x8 A[CTY][NPLN];
#pragma unroll
                    for (int my = 0; my < CTY; ++my)
#pragma unroll
                        for (int pl = 0; pl < NPLN; ++pl) A[my][pl] = ld(pl * SPLANE_B + abase + ((mz * SY + my) * SX) * 16);
#pragma unroll
                    for (int pr = 0; pr < 3; ++pr)
#pragma unroll
                        for (int nn = 0; nn < NT; ++nn)
#pragma unroll
                            for (int my = 0; my < CTY; ++my)
                                acc[c][mz * CTY + my][nn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[my][kSplitPA[pr]], B[nn][kSplitPB[pr]], acc[c][mz * CTY + my][nn], 0, 0, 0);
                }
            }
        }
        if (more) {
            Ecur = stage(ch + 1);                                // (its barrier: every wave is done reading this chunk's tile)
            __syncthreads();
        }
    }
    float inv1, inv2; sc.leave(inv1, inv2);                      // the sums back to the true unit
    // epilogue: fine voxel (2 (z0 + mz) + pz, 2 (y0 + my) + py, 2 (x0 + 4 g + q) + px), couts 16 (nt0 + nn) + 4 a4 .. + 3
    const int Df = 2 * p.Dc, Hf = 2 * p.Hc, Wf = 2 * p.Wc;
    const long long osample = (long long)Df * Hf * Wf * p.Cout;
    const __amdgpu_buffer_rsrc_t ro = da_rsrc(p.out + (long long)n * osample, (unsigned)(osample * sizeof(float)));
    const int xc = x0 + 4 * g + q;
#pragma unroll
    for (int nn = 0; nn < NT; ++nn) {
        const int co0 = (nt0 + nn) * 16 + 4 * a4;
        float bv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = (p.bias && co0 + j < p.Cout) ? p.bias[co0 + j] : 0.f;
        const bool cok = co0 + 3 < p.Cout && xc < p.Wc;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int cls = 2 * wave + c;
            const int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
#pragma unroll
            for (int mz = 0; mz < CTZ; ++mz)
#pragma unroll
                for (int my = 0; my < CTY; ++my) {
                    const f32x4 o = da_bias_act4(da_quad_transpose(acc[c][mz * CTY + my][nn] * inv1 * inv2, q), bv, p.slope);
                    const int zc = z0 + mz, yc = y0 + my;
                    const bool ok = cok && zc < p.Dc && yc < p.Hc;
                    da_buf_store4(ro, ok ? (unsigned)(((((2 * zc + pz) * Hf + 2 * yc + py) * Wf + 2 * xc + px) * p.Cout + co0) * 4) : 0xFFFFFFFFu, o);
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// data gradient: stride-2 convolution of the fine gradient with the 4 x 4 x 4 summed kernel
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int FZ = 2 * CTZ + 2, FY = 2 * CTY + 2, FXV = 2 * CTX + 2;   // fine halo 6 x 10 x 34
constexpr int FXS = 34;                                                // x slots: 17 even columns then 17 odd
constexpr int FV = FZ * FY * FXV;                                      // 2040 voxels
constexpr int FPLANE_B = FZ * FY * FXS * 16;
constexpr int F_NIT = (FV * 2 + 255) / 256;                            // 16

struct DgP {
    const float* dy; const unsigned char* wp; const int* wexp; float* dx1; float* dx2; int C1, C2;
    int N, Dc, Hc, Wc, Cout, ntz, nty, ntx, nchunks, NTN;      // nchunks = Cout / 8 (K chunks), NTN = N-tiles over Cin
};

// packed B operand: [chunk (8 couts)][step 16][N-tile][plane][lane][8]; lane (g, n): adjoint tap 4 step + g (fz*16 + fy*4 + fx), K = cout chunk*8+e, N = cin 16 nt + n.
// Grid (chunks, PY), per-chunk scale exponent in wexp[chunk] as in up_pack_fwd_kernel.
__global__ void __launch_bounds__(256) up_pack_dgrad_kernel(const float* __restrict__ w, unsigned short* __restrict__ wp, int* __restrict__ wexp, int Cin, int Cout, int NTN) {
    __shared__ float red[4];
    const int ch = blockIdx.x;
    float m = 0.f;
    const bool vec = (Cout & 3) == 0 && ch * 8 + 8 <= Cout && (reinterpret_cast<size_t>(w) & 15) == 0;
    if (vec) {                                                   // quad loads, four in flight per lane (the largest |w| does not depend on the order)
        const int nq = 27 * Cin * 2;
        float m1 = 0.f, m2 = 0.f, m3 = 0.f;
        int idx = threadIdx.x;
        for (; idx + 768 < nq; idx += 1024) {
            const float4 a = *reinterpret_cast<const float4*>(w + (size_t)(idx >> 1) * Cout + ch * 8 + (idx & 1) * 4);
            const float4 b = *reinterpret_cast<const float4*>(w + (size_t)((idx + 256) >> 1) * Cout + ch * 8 + (idx & 1) * 4);
            const float4 c = *reinterpret_cast<const float4*>(w + (size_t)((idx + 512) >> 1) * Cout + ch * 8 + (idx & 1) * 4);
            const float4 d = *reinterpret_cast<const float4*>(w + (size_t)((idx + 768) >> 1) * Cout + ch * 8 + (idx & 1) * 4);
            m = da_absmax4(m, a); m1 = da_absmax4(m1, b); m2 = da_absmax4(m2, c); m3 = da_absmax4(m3, d);
        }
        for (; idx < nq; idx += 256) m = da_absmax4(m, *reinterpret_cast<const float4*>(w + (size_t)(idx >> 1) * Cout + ch * 8 + (idx & 1) * 4));
        m = fmaxf(fmaxf(m, m1), fmaxf(m2, m3));
    } else {
        for (int idx = threadIdx.x; idx < 27 * Cin * 8; idx += 256) { const int e = idx & 7, r = idx >> 3; const int co = ch * 8 + e; if (co < Cout) m = fmaxf(m, fabsf(w[(size_t)r * Cout + co])); }
    }
    const int ew = up_sum_exp(da_block_max4(m, red, (int)threadIdx.x >> 6, (int)threadIdx.x & 63));
    if (blockIdx.y == 0 && threadIdx.x == 0) wexp[ch] = ew;
    const float sc = da_pow2(ew);
    const int units = 16 * NTN * 64;                             // (step, N-tile, lane)
    for (int u = blockIdx.y * 256 + threadIdx.x; u < units; u += gridDim.y * 256) {
        const int lane = u & 63, nt = (u >> 6) % NTN, st = (u >> 6) / NTN;
        const int g = lane >> 4, n = lane & 15;
        const int ft = 4 * st + g, ci = nt * 16 + n;
        int tz[2], ty[2], tx[2];
        const int nz = up_taps_of_f((ft >> 4) & 3, tz), ny = up_taps_of_f((ft >> 2) & 3, ty), nx = up_taps_of_f(ft & 3, tx);
        // the 8 couts of the chunk are contiguous in w: two quad loads per folded tap when the layout allows it (same summation order either way)
        double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (vec) {                                               // all sixteen quad loads issued before the first sum (absent taps re-read a present one and add 0)
            const int cic = ci < Cin ? ci : Cin - 1;
            float4 p0[8], p1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int a = j >> 2, b = (j >> 1) & 1, c = j & 1;
                const float* src = w + ((size_t)(tz[a < nz ? a : 0] * 9 + ty[b < ny ? b : 0] * 3 + tx[c < nx ? c : 0]) * Cin + cic) * Cout + ch * 8;
                p0[j] = *reinterpret_cast<const float4*>(src); p1[j] = *reinterpret_cast<const float4*>(src + 4);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int a = j >> 2, b = (j >> 1) & 1, c = j & 1;
                if (ci < Cin && a < nz && b < ny && c < nx) {
                    acc[0] += (double)p0[j].x; acc[1] += (double)p0[j].y; acc[2] += (double)p0[j].z; acc[3] += (double)p0[j].w;
                    acc[4] += (double)p1[j].x; acc[5] += (double)p1[j].y; acc[6] += (double)p1[j].z; acc[7] += (double)p1[j].w;
                }
            }
        } else if (ci < Cin)
            for (int a = 0; a < nz; ++a) for (int b = 0; b < ny; ++b) for (int c = 0; c < nx; ++c) {
                const float* src = w + ((size_t)(tz[a] * 9 + ty[b] * 3 + tx[c]) * Cin + ci) * Cout + ch * 8;
#pragma unroll
                for (int e = 0; e < 8; ++e) if (ch * 8 + e < Cout) acc[e] += (double)src[e];
            }
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)acc[e];
        da_split_store8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), sc, reinterpret_cast<uint4*>(wp + ((size_t)((ch * 16 + st) * NTN + nt) * NPLN) * 512) + lane, 64);
    }
}

template <int NTN>      // N-tiles over Cin: 1, 2 or 4; wave -> (N-tile w % NTN, M group w / NTN), 8 NTN / 4 M-tiles per wave
__global__ void __launch_bounds__(256, 1) up_dgrad_kernel(DgP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int MPW = 2 * NTN;                                 // M-tiles per wave
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = lane & 15, g = lane >> 4, q = lane & 3, a4 = (lane & 15) >> 2;
    const int nt = wave % NTN, mg = wave / NTN;
    int n, tz, ty, tx;
    da_tile_zyx(da_xcd_item_of_block(blockIdx.x, gridDim.x), p.ntz, p.nty, p.ntx, n, tz, ty, tx);
    const int z0 = tz * CTZ, y0 = ty * CTY, x0 = tx * CTX;
    const int Df = 2 * p.Dc, Hf = 2 * p.Hc, Wf = 2 * p.Wc;
    const long long ysample = (long long)Df * Hf * Wf * p.Cout;
    const __amdgpu_buffer_rsrc_t ry = da_rsrc(p.dy + (long long)n * ysample, (unsigned)(ysample * sizeof(float)));
    const __amdgpu_buffer_rsrc_t rsw = da_rsrc(p.wp, (unsigned)((size_t)p.nchunks * 16 * NTN * NPLN * 1024));
    // staging map: iteration it covers halo voxel v = (tid + 256 it) / 2 = (hz, hy, hx), quad tid & 1; LDS slot de-interleaves x by parity
    const int c4 = (int)threadIdx.x & 1;
    unsigned pk[F_NIT]; int slot[F_NIT];
#pragma unroll
    for (int it = 0; it < F_NIT; ++it) {
        const int v = ((int)threadIdx.x + it * 256) >> 1;
        const int hx = v % FXV, t2 = v / FXV, hy = t2 % FY, hz = t2 / FY;
        const bool ok = v < FV;
        pk[it] = ok ? ((unsigned)hz << 16 | (unsigned)hy << 8 | (unsigned)hx) : 0xFFFF0000u;
        const int xpos = (hx & 1) ? 17 + (hx >> 1) : (hx >> 1);
        slot[it] = ok ? ((t2 * FXS + xpos) * 2 + c4) : -1;
    }
    // (two half-size register arrays: one 256-byte array is left in scratch memory by hipcc's alloca promotion)
    constexpr int FH = F_NIT / 2;
    float4 preA[FH], preB[FH];
    auto issue = [&](int ch) {
#pragma unroll
        for (int it = 0; it < F_NIT; ++it) {
            const int hz = (int)(pk[it] >> 16), hy = (int)((pk[it] >> 8) & 255u), hx = (int)(pk[it] & 255u);
            const int z = 2 * z0 - 1 + hz, y = 2 * y0 - 1 + hy, x = 2 * x0 - 1 + hx;
            const bool inb = hz != 0xFFFF && (unsigned)z < (unsigned)Df && (unsigned)y < (unsigned)Hf && (unsigned)x < (unsigned)Wf;
            const float4 v = da_buf_load4(ry, inb ? (unsigned)((((z * Hf + y) * Wf + x) * p.Cout + ch * 8 + c4 * 4) * 4) : 0xFFFFFFFFu);
            if (it < FH) preA[it < FH ? it : 0] = v; else preB[it >= FH ? it - FH : 0] = v;
        }
    };
    // scale bookkeeping: chunk = 8 output channels of dY.  DaSplitScale's rule on two plain ints: with the struct hipcc spills a fifth SGPR here.
    float* smax = reinterpret_cast<float*>(lds + NPLN * FPLANE_B);
    int Eacc = 0, Emin = 0;
    auto stage = [&](int ch) -> int {                            // publish the tile's largest magnitude, barrier, split + write; returns the chunk's E
        float m = 0.f;
#pragma unroll
        for (int it = 0; it < FH; ++it) { m = da_absmax4(m, preA[it]); m = da_absmax4(m, preB[it]); }
        m = da_block_max4(m, smax, wave, lane);
        const int ew = p.wexp[ch];
        const int E = da_split_admit(da_scale_exp(m) + ew, ch == 0, Emin);
        const float sy = da_pow2(E - ew);
#pragma unroll
        for (int it = 0; it < F_NIT; ++it) {
            if (slot[it] >= 0) da_split_store4(it < FH ? preA[it < FH ? it : 0] : preB[it >= FH ? it - FH : 0], sy, reinterpret_cast<uint2*>(lds) + slot[it], FPLANE_B / 8);
        }
        return E;
    };
    auto ld = [&](int off) -> f16x8 { return *reinterpret_cast<const f16x8*>(lds + off); };
    f32x4 acc[MPW];
#pragma unroll
    for (int m = 0; m < MPW; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    issue(0);
    int Ecur = stage(0);
    __syncthreads();
#pragma unroll 1
    for (int ch = 0; ch < p.nchunks; ++ch) {
        const bool more = ch + 1 < p.nchunks;
        if (more) issue(ch + 1);
        {
            const float f = da_acc_factor(Ecur - Eacc);          // the running sums into this chunk's unit (exact)
#pragma unroll
            for (int m = 0; m < MPW; ++m) acc[m] = acc[m] * f;
            Eacc = Ecur;
        }
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
            const int ft = 4 * s + g;                            // adjoint tap of this lane group: fi = f + 1 per axis
            const int fz = (ft >> 4) & 3, fy = (ft >> 2) & 3, fx = ft & 3;
            const int xp = (fx & 1) ? 17 + (fx >> 1) : (fx >> 1);     // halo column 2 i + fx: even fx -> slot i + fx / 2, odd -> 17 + i + fx / 2
            const int abase = ((fz * FY + fy) * FXS + xp + i) * 16;
            f16x8 B[NPLN];
#pragma unroll
            for (int pl = 0; pl < NPLN; ++pl)
                B[pl] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rsw, (unsigned)lane * 16u, (unsigned)((((ch * 16 + s) * NTN + nt) * NPLN + pl) * 1024), 0));
            f16x8 A[MPW][NPLN];
#pragma unroll
            for (int m = 0; m < MPW; ++m) {
                const int mt = mg * MPW + m, mz = mt / CTY, my = mt % CTY;
#pragma unroll
                for (int pl = 0; pl < NPLN; ++pl) A[m][pl] = ld(pl * FPLANE_B + abase + ((2 * mz * FY + 2 * my) * FXS) * 16);
            }
#pragma unroll
            for (int pr = 0; pr < 3; ++pr)
#pragma unroll
                for (int m = 0; m < MPW; ++m)
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[m][kSplitPA[pr]], B[kSplitPB[pr]], acc[m], 0, 0, 0);
        }
        if (more) {
            Ecur = stage(ch + 1);                                // (its barrier: every wave is done reading this chunk's tile)
            __syncthreads();
        }
    }
    float inv1, inv2; da_unscale_factors(Eacc, inv1, inv2);      // the sums back to the true unit
    // stores: coarse voxel (z0 + mz, y0 + my, x0 + 4 g + q), input channels 16 nt + 4 a4 .. + 3 of dx1 | dx2
    const int ci0 = nt * 16 + 4 * a4;
    const bool first = ci0 < p.C1;
    const int Cd = first ? p.C1 : p.C2, cd = first ? ci0 : ci0 - p.C1;
    const long long vox = (long long)p.Dc * p.Hc * p.Wc;
    const __amdgpu_buffer_rsrc_t rd = da_rsrc((first ? p.dx1 : p.dx2) + (long long)n * vox * Cd, (unsigned)(vox * Cd * sizeof(float)));
    const int xc = x0 + 4 * g + q;
    const bool cok = ci0 + 3 < p.C1 + p.C2 && xc < p.Wc;
#pragma unroll
    for (int m = 0; m < MPW; ++m) {
        const int mt = mg * MPW + m, zc = z0 + mt / CTY, yc = y0 + mt % CTY;
        const f32x4 v = da_quad_transpose(acc[m] * inv1 * inv2, q);
        da_buf_store4(rd, (cok && zc < p.Dc && yc < p.Hc) ? (unsigned)((((zc * p.Hc + yc) * p.Wc + xc) * Cd + cd) * 4) : 0xFFFFFFFFu, v);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// weight gradient: G[p][j][ci][co] per class, then dW[t] = sum of the (p, j) pairs containing tap t
// ------------------------------------------------------------------------------------------------------------------------------
struct WgP {
    const float* s1; const float* s2; int C1, C2;
    const float* dy; float* partial;
    int N, Dc, Hc, Wc, Cout, ntz, nty, ntx, ntiles, nslabs, O;       // O = 64 * Cin * Cout (one partial set: [class][j][ci][co])
};
constexpr int YV = CTZ * CTY * CTX;                              // 128 dY voxels of one class per tile
constexpr int YPLANE_B = YV * 32 * 2;                            // [voxel][32 couts] bf16

__global__ void __launch_bounds__(256, 2) up_wgrad_kernel(WgP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned char* ldsY = lds + NPLN * SPLANE_B;
    typedef s16x4 __attribute__((address_space(3))) * lds_frag_ptr;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = lane & 15, g = lane >> 4, q = i & 3, vq = i >> 2;
    const int ch = blockIdx.y, cls = blockIdx.z;
    const int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
    const int zi = g >> 1;
    const int cb = ch * 8;
    const bool first = cb < p.C1;
    const float* src = first ? p.s1 : p.s2;
    const int Cs = first ? p.C1 : p.C2, choff = first ? cb : cb - p.C1;
    auto tr8 = [&](const unsigned char* a, int step_bytes) -> f16x8 {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_frag_ptr)a);
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_frag_ptr)(a + step_bytes));
        return __builtin_bit_cast(f16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    };
    // S fragment of tap-pair slot s (taps 2 s, 2 s + 1; this lane: tap 2 s + (q >> 1), channel quad q & 1) for output row `wave`
    int aoff[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int jt = 2 * s + (q >> 1);
        aoff[s] = ((((zi + pz + ((jt >> 2) & 1)) * SY + wave + py + ((jt >> 1) & 1)) * SX + px + (jt & 1) + 8 * (g & 1) + vq) * 8 + (q & 1) * 4) * 2;
    }
    const int yoff = (((zi * CTY + wave) * CTX + 8 * (g & 1) + vq) * 32 + q * 4) * 2;
    struct F3 { f16x8 p[NPLN]; };
    auto loadF = [&](int s) -> F3 { F3 f;
#pragma unroll
        for (int pl = 0; pl < NPLN; ++pl) f.p[pl] = tr8(lds + pl * SPLANE_B + aoff[s], 4 * 8 * 2);
        return f; };
    auto loadY = [&](int nn) -> F3 { F3 f;
#pragma unroll
        for (int pl = 0; pl < NPLN; ++pl) f.p[pl] = tr8(ldsY + pl * YPLANE_B + yoff + nn * 32, 4 * 32 * 2);
        return f; };
    f32x4 acc[4][2];
#pragma unroll
    for (int s = 0; s < 4; ++s) { acc[s][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[s][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    SMap sm; sm.init();
    float4 preA[S_NIT], preY[4];
    const int yv0 = (int)threadIdx.x >> 3, yq = (int)threadIdx.x & 7;
    const int Df = 2 * p.Dc, Hf = 2 * p.Hc, Wf = 2 * p.Wc;
    auto issue = [&](int pos) {
        int n, tz, ty, tx;
        da_tile_zyx(pos, p.ntz, p.nty, p.ntx, n, tz, ty, tx);
        const int z0 = tz * CTZ, y0 = ty * CTY, x0 = tx * CTX;
        const long long vox = (long long)p.Dc * p.Hc * p.Wc;
        const __amdgpu_buffer_rsrc_t rs = da_rsrc(src + (long long)n * vox * Cs, (unsigned)(vox * Cs * sizeof(float)));
#pragma unroll
        for (int it = 0; it < S_NIT; ++it) preA[it] = da_buf_load4(rs, sm.offset(it, z0 - 1, y0 - 1, x0 - 1, p.Dc, p.Hc, p.Wc, Cs, choff));
        const long long ysample = (long long)Df * Hf * Wf * p.Cout;
        const __amdgpu_buffer_rsrc_t ry = da_rsrc(p.dy + (long long)n * ysample, (unsigned)(ysample * sizeof(float)));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int v = yv0 + 32 * u;
            const int vx = v & 15, vy = (v >> 4) & 3, vz = v >> 6;
            const int zc = z0 + vz, yc = y0 + vy, xc = x0 + vx, co = yq * 4;
            const bool inb = zc < p.Dc && yc < p.Hc && xc < p.Wc && co < p.Cout;
            preY[u] = da_buf_load4(ry, inb ? (unsigned)(((((2 * zc + pz) * Hf + 2 * yc + py) * Wf + 2 * xc + px) * p.Cout + co) * 4) : 0xFFFFFFFFu);
        }
    };
    // scale bookkeeping (DaSplitScale, over this workgroup's walk): a tile is staged at E = S exponent + dY exponent
    float* smax = reinterpret_cast<float*>(ldsY + NPLN * YPLANE_B);      // [2][4]
    DaSplitScale sc; int Enext = 0; bool first_tile = true;
    auto write_lds = [&]() {                                     // (starts with the barrier that retires the tile in LDS)
        const DaMax2 m = da_block_max4x2(stage_absmax<S_NIT>(preA), stage_absmax<4>(preY), smax, wave, lane);
        const int ey = da_scale_exp(m.b);
        Enext = sc.admit(da_scale_exp(m.a) + ey, first_tile);
        first_tile = false;
        const float sy = da_pow2(ey);
        sm.write(lds, preA, da_pow2(Enext - ey));
#pragma unroll
        for (int u = 0; u < 4; ++u) da_split_store4(preY[u], sy, reinterpret_cast<uint2*>(ldsY) + (yv0 + 32 * u) * 8 + yq, YPLANE_B / 8);
    };
    const int slab = blockIdx.x;
    const int cnt = (p.ntiles > slab) ? (p.ntiles - slab + p.nslabs - 1) / p.nslabs : 0;
    if (cnt > 0) { issue(slab); write_lds(); }
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < cnt; ++k) {
        const bool more = k + 1 < cnt;
        if (more) issue(slab + (k + 1) * p.nslabs);
        {
            const float f = sc.enter(Enext);                     // the running sums into this tile's unit (exact)
#pragma unroll
            for (int s = 0; s < 4; ++s) { acc[s][0] = acc[s][0] * f; acc[s][1] = acc[s][1] * f; }
        }
        const F3 Y0 = loadY(0), Y1 = loadY(1);
        F3 F = loadF(0), Fn;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s + 1 < 4) Fn = loadF(s + 1);
#pragma unroll
            for (int pr = 0; pr < 3; ++pr) {
                acc[s][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(F.p[kSplitPA[pr]], Y0.p[kSplitPB[pr]], acc[s][0], 0, 0, 0);
                acc[s][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(F.p[kSplitPA[pr]], Y1.p[kSplitPB[pr]], acc[s][1], 0, 0, 0);
            }
            if (s + 1 < 4) F = Fn;
        }
        if (more) {
            write_lds();
            __syncthreads();
        }
    }
    {
        float inv1, inv2; sc.leave(inv1, inv2);                  // back to the true unit
#pragma unroll
        for (int s = 0; s < 4; ++s) { acc[s][0] = acc[s][0] * inv1 * inv2; acc[s][1] = acc[s][1] * inv1 * inv2; }
    }
    // reduce the four waves (rows) through LDS, wave 0 writes G[cls][j][cb + ci][co] of this slab
    __syncthreads();
    float4* red = reinterpret_cast<float4*>(lds);
    if (wave > 0) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nn = 0; nn < 2; ++nn) red[(((wave - 1) * 4 + s) * 2 + nn) * 64 + lane] = make_float4(acc[s][nn][0], acc[s][nn][1], acc[s][nn][2], acc[s][nn][3]);
    }
    __syncthreads();
    if (wave == 0) {
        const int Cin = p.C1 + p.C2;
        float* part = p.partial + (size_t)blockIdx.x * p.O + (size_t)cls * 8 * Cin * p.Cout;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nn = 0; nn < 2; ++nn) {
                f32x4 a = acc[s][nn];
#pragma unroll
                for (int w = 0; w < 3; ++w) { const float4 v = red[((w * 4 + s) * 2 + nn) * 64 + lane]; a[0] += v.x; a[1] += v.y; a[2] += v.z; a[3] += v.w; }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int row = 4 * g + reg;
                    const int jt = 2 * s + (row >> 3), ci = cb + (row & 7), co = nn * 16 + i;
                    if (co < p.Cout) part[((size_t)jt * Cin + ci) * p.Cout + co] = a[reg];
                }
            }
    }
}

// dW[t][ci][co] = sum over the 8 (class, coarse tap) pairs that contain original tap t and over the slabs, in double, fixed order
// eight lanes per output (one per (class, coarse tap) pair holding the tap), the slabs four loads at a time; fixed order: per pair over the slabs, then the pairs
__global__ void __launch_bounds__(256) up_wgrad_reduce_kernel(const float* __restrict__ partial, int nslabs, int Cin, int Cout, float* __restrict__ dw) {
    const int IO = Cin * Cout;
    const int total = 27 * IO;
    const int k = threadIdx.x & 7;
    for (int base = blockIdx.x * 32; base < total; base += gridDim.x * 32) {      // (block-uniform trip count: the shuffles below need whole waves)
        const int o = base + ((int)threadIdx.x >> 3);
        const bool live = o < total;
        const int oo = live ? o : 0;
        const int tap = oo / IO, r = oo - tap * IO;
        const int t3[3] = {tap / 9, (tap / 3) % 3, tap % 3};
        // per axis the two (p, j) pairs holding tap t: t 0: (0,0) (1,0); t 1: (0,1) (1,0); t 2: (0,1) (1,1)
        int cls = 0, jt = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int sel = (k >> (2 - a)) & 1;
            const int pa = sel, ja = sel ? (t3[a] == 2 ? 1 : 0) : (t3[a] == 0 ? 0 : 1);
            cls = cls * 2 + pa; jt = jt * 2 + ja;
        }
        const float* src = partial + (size_t)(cls * 8 + jt) * IO + r;
        const size_t bs = (size_t)64 * IO;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int b = 0;
        for (; b + 4 <= nslabs; b += 4) {
            const float v0 = src[(size_t)b * bs], v1 = src[(size_t)(b + 1) * bs], v2 = src[(size_t)(b + 2) * bs], v3 = src[(size_t)(b + 3) * bs];
            s0 += (double)v0; s1 += (double)v1; s2 += (double)v2; s3 += (double)v3;
        }
        for (; b < nslabs; ++b) s0 += (double)src[(size_t)b * bs];
        double s = (s0 + s1) + (s2 + s3);
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
        if (live && k == 0) dw[o] = (float)s;
    }
}

struct Plan { int ntz, nty, ntx, ntiles; };
Plan up_plan(int N, int Dc, int Hc, int Wc) {
    Plan q;
    q.ntz = (Dc + CTZ - 1) / CTZ; q.nty = (Hc + CTY - 1) / CTY; q.ntx = (Wc + CTX - 1) / CTX;
    q.ntiles = N * q.ntz * q.nty * q.ntx;
    return q;
}
int up_wgrad_slabs(int ntiles, int nchunks) {
    int s = 512 / (nchunks * 8);                                 // two workgroups per CU over (slab, chunk, class)
    s = s / 8 * 8; if (s < 8) s = 8;
    if (s > ntiles) s = ntiles;
    return s < 1 ? 1 : s;
}

}  // namespace

// C1 / C2: channels of the one or two COARSE source tensors (multiples of 8; C1 a multiple of 16 when C2 > 0 so that a 16-wide gradient
// tile never straddles the two tensors); Cout a multiple of 8, at most 32; split matrix mode only (the arithmetic of these kernels).
extern "C" int da_upconv3d_k3_supported(int C1, int C2, int Cout) {
    if (da_matrix_mode() != 2) return 0;
    if (C1 <= 0 || C2 < 0 || C1 % 8 || C2 % 8 || (C2 > 0 && C1 % 16) || C1 + C2 > 64) return 0;
    if (Cout % 8 || Cout <= 0 || Cout > 32) return 0;
    return 1;
}

extern "C" size_t da_upconv3d_k3_ws_bytes(int N, int Dc, int Hc, int Wc, int Cin, int Cout) {
    const Plan q = up_plan(N, Dc, Hc, Wc);
    const int NT = (Cout + 15) / 16, NTN = (Cin + 15) / 16;
    const size_t pack_f = (size_t)(Cin / 8) * 16 * NT * NPLN * 1024;
    const size_t pack_d = (size_t)((Cout + 7) / 8) * 16 * (NTN == 3 ? 4 : NTN) * NPLN * 1024;
    const size_t part = (size_t)up_wgrad_slabs(q.ntiles, Cin / 8) * 64 * Cin * Cout * sizeof(float);
    size_t m = pack_f > pack_d ? pack_f : pack_d;
    if (part > m) m = part;
    DaCarve c(nullptr); da_exp_pack(c); c.take<char>(m);      // (the weight gradient's partials reuse the same bytes from the start)
    return c.off;
}

static bool up_sizes_ok(int N, int Dc, int Hc, int Wc, int Cin, int Cout) {
    const long long fine = 8ll * Dc * Hc * Wc;
    return fine * Cout * 4 < (1ll << 32) && (long long)Dc * Hc * Wc * Cin * 4 < (1ll << 32) && (long long)N * fine < (1ll << 31);
}

extern "C" int da_upconv3d_k3_fwd(const float* s1, int C1, const float* s2, int C2, const float* w_tio, const float* bias, float* out,
                                  int N, int Dc, int Hc, int Wc, int Cout, float act_slope, void* ws, size_t ws_bytes, void* stream) {
    if (!s1 || !w_tio || !out || (C2 > 0 && !s2) || N <= 0 || Dc <= 0 || Hc <= 0 || Wc <= 0) return DA_ERR_BADARG;
    const int Cin = C1 + C2;
    if (!da_upconv3d_k3_supported(C1, C2, Cout) || !up_sizes_ok(N, Dc, Hc, Wc, Cin, Cout)) return DA_ERR_UNSUPPORTED;
    if (ws_bytes < da_upconv3d_k3_ws_bytes(N, Dc, Hc, Wc, Cin, Cout)) return DA_ERR_WS_SMALL;
    hipStream_t st = da_stream(stream);
    const Plan q = up_plan(N, Dc, Hc, Wc);
    FwdP p;
    p.nchunks = Cin / 8; p.NTall = (Cout + 15) / 16; p.slope = act_slope;
    DaCarve c(ws); const DaExpPack pk = da_exp_pack(c); p.s1 = s1; p.s2 = s2; p.C1 = C1; p.C2 = C2; p.wexp = pk.wexp; p.wp = pk.wp; p.bias = bias; p.out = out;
    p.N = N; p.Dc = Dc; p.Hc = Hc; p.Wc = Wc; p.Cout = Cout; p.ntz = q.ntz; p.nty = q.nty; p.ntx = q.ntx;
    hipLaunchKernelGGL(up_pack_fwd_kernel, dim3(p.nchunks, 4 * p.NTall), dim3(256), 0, st, w_tio, (unsigned short*)pk.wp, pk.wexp, Cin, Cout, p.NTall);
    DA_LAUNCH_CHECK();
    const size_t shm = NPLN * SPLANE_B + 16;
    if (p.NTall == 1) return da_launch_lds<up_fwd_kernel<1>>(dim3(q.ntiles, 1), dim3(256), shm, st, p);
    return da_launch_lds<up_fwd_kernel<2>>(dim3(q.ntiles, 1), dim3(256), shm, st, p);
}

extern "C" int da_upconv3d_k3_dgrad(const float* dy, const float* w_tio, float* dx1, int C1, float* dx2, int C2,
                                    int N, int Dc, int Hc, int Wc, int Cout, void* ws, size_t ws_bytes, void* stream) {
    if (!dy || !w_tio || !dx1 || (C2 > 0 && !dx2) || N <= 0 || Dc <= 0 || Hc <= 0 || Wc <= 0) return DA_ERR_BADARG;
    const int Cin = C1 + C2;
    if (!da_upconv3d_k3_supported(C1, C2, Cout) || !up_sizes_ok(N, Dc, Hc, Wc, Cin, Cout)) return DA_ERR_UNSUPPORTED;
    if (ws_bytes < da_upconv3d_k3_ws_bytes(N, Dc, Hc, Wc, Cin, Cout)) return DA_ERR_WS_SMALL;
    hipStream_t st = da_stream(stream);
    const Plan q = up_plan(N, Dc, Hc, Wc);
    DgP p;
    p.nchunks = Cout / 8;
    int NTN = (Cin + 15) / 16; if (NTN == 3) NTN = 4;            // (48 input channels: a fourth, empty tile)
    p.NTN = NTN;
    DaCarve c(ws); const DaExpPack pk = da_exp_pack(c); p.dy = dy; p.wexp = pk.wexp; p.wp = pk.wp; p.dx1 = dx1; p.dx2 = dx2; p.C1 = C1; p.C2 = C2;
    p.N = N; p.Dc = Dc; p.Hc = Hc; p.Wc = Wc; p.Cout = Cout; p.ntz = q.ntz; p.nty = q.nty; p.ntx = q.ntx;
    hipLaunchKernelGGL(up_pack_dgrad_kernel, dim3(p.nchunks, 4 * NTN), dim3(256), 0, st, w_tio, (unsigned short*)pk.wp, pk.wexp, Cin, Cout, NTN);
    DA_LAUNCH_CHECK();
    const size_t shm = NPLN * FPLANE_B + 16;
    switch (NTN) {
        case 1: return da_launch_lds<up_dgrad_kernel<1>>(dim3(q.ntiles), dim3(256), shm, st, p);
        case 2: return da_launch_lds<up_dgrad_kernel<2>>(dim3(q.ntiles), dim3(256), shm, st, p);
        case 4: return da_launch_lds<up_dgrad_kernel<4>>(dim3(q.ntiles), dim3(256), shm, st, p);
        default: return DA_ERR_UNSUPPORTED;
    }
}

extern "C" int da_upconv3d_k3_wgrad(const float* s1, int C1, const float* s2, int C2, const float* dy, float* dw_tio,
                                    int N, int Dc, int Hc, int Wc, int Cout, void* ws, size_t ws_bytes, void* stream) {
    if (!s1 || !dy || !dw_tio || (C2 > 0 && !s2) || N <= 0 || Dc <= 0 || Hc <= 0 || Wc <= 0) return DA_ERR_BADARG;
    const int Cin = C1 + C2;
    if (!da_upconv3d_k3_supported(C1, C2, Cout) || !up_sizes_ok(N, Dc, Hc, Wc, Cin, Cout)) return DA_ERR_UNSUPPORTED;
    if (ws_bytes < da_upconv3d_k3_ws_bytes(N, Dc, Hc, Wc, Cin, Cout)) return DA_ERR_WS_SMALL;
    hipStream_t st = da_stream(stream);
    const Plan q = up_plan(N, Dc, Hc, Wc);
    WgP p;
    p.s1 = s1; p.s2 = s2; p.C1 = C1; p.C2 = C2; p.dy = dy; p.partial = (float*)ws;
    p.N = N; p.Dc = Dc; p.Hc = Hc; p.Wc = Wc; p.Cout = Cout; p.ntz = q.ntz; p.nty = q.nty; p.ntx = q.ntx; p.ntiles = q.ntiles;
    const int nchunks = Cin / 8;
    p.nslabs = up_wgrad_slabs(q.ntiles, nchunks); p.O = 64 * Cin * Cout;
    const size_t shm = (size_t)NPLN * SPLANE_B + NPLN * YPLANE_B + 32;
    if (const int rc = da_launch_lds<up_wgrad_kernel>(dim3(p.nslabs, nchunks, 8), dim3(256), shm, st, p)) return rc;
    hipLaunchKernelGGL(up_wgrad_reduce_kernel, dim3(da_grid((long long)27 * Cin * Cout * 8, 256, 2048)), dim3(256), 0, st, p.partial, p.nslabs, Cin, Cout, dw_tio);
    DA_LAUNCH_CHECK();
    return 0;
}
