// Blended sliding-window inference (include/deepatlas_hip.h, "blended sliding-window inference"): the probabilities of Partition's overlapping
// tiles, weighted by a separable window, summed per voxel in a fixed order, and the argmax / confidence of the sums.
// Both kernels stream runs of K floats per voxel.  L lanes share a voxel: with K = 4 L (L a power of two) lane s holds channels 4 s ... 4 s + 3
// as one 16-byte access (QUAD, as the boundary-loss kernels do); any other K takes L = min(64, next power of two >= K) lanes that hold channels
// s, s + L, s + 2 L, s + 3 L as 4-byte accesses, consecutive lanes on consecutive addresses.
// Accumulate is launched over (tile of the call, voxel of the tile): the lanes of the call's lowest-numbered covering tile own the volume voxel,
// read its sums once, add the call's covering tiles in ascending order and store once; all other lanes leave.  Nothing races, there is no atomic,
// every tile logit is read exactly once and no launch sweeps the whole volume.
#include "common.h"
#include "tile_geom.h"

namespace {

constexpr int kBlendMaxK = DA_BLEND_MAX_CLASSES;

// channel of register r of lane `sub`
template <int L, bool QUAD> __device__ __forceinline__ int bd_channel(int sub, int r) { return QUAD ? 4 * sub + r : sub + r * L; }

// the K floats at p, this lane's share; channels >= K read as `fill`
template <int L, bool QUAD> __device__ __forceinline__ void bd_load(const float* __restrict__ p, int sub, int K, float fill, float (&v)[4]) {
    if (QUAD) {
        const float4 q = reinterpret_cast<const float4*>(p)[sub];
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int c = sub + r * L; v[r] = c < K ? p[c] : fill; }
    }
}
template <int L, bool QUAD> __device__ __forceinline__ void bd_store(float* __restrict__ p, int sub, int K, const float (&v)[4]) {
    if (QUAD) reinterpret_cast<float4*>(p)[sub] = make_float4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int c = sub + r * L; if (c < K) p[c] = v[r]; }
    }
}

struct BlendCall { TileGeom g; int K, tile0, n_tiles, flip; };

// tiles a with a e - o <= x < a e - o + t, a in [0, g): [lo, hi]
__device__ __forceinline__ void bd_cover(int x, int t, int o, int e, int g, int& lo, int& hi) {
    const int num = x + o - t + 1;
    lo = num > 0 ? (num + e - 1) / e : 0;
    hi = min(g - 1, (x + o) / e);
}

// whether tile `cur` is the first tile of the call in the voxel's covering box (the box is walked in ascending raster order, and `cur` is in it)
__device__ __forceinline__ bool bd_owns(int cur, int tile0, int gy, int gx, int zl, int zh, int yl, int yh, int xl, int xh) {
    for (int a = zl; a <= zh; ++a)
        for (int b = yl; b <= yh; ++b)
            for (int c = xl; c <= xh; ++c) {
                const int r = (a * gy + b) * gx + c;
                if (r >= tile0) return r == cur;
            }
    return false;
}

template <int L, bool QUAD>
__global__ void __launch_bounds__(256)
blend_accumulate_kernel(const float* __restrict__ logits, float* __restrict__ acc, const float* __restrict__ wz, const float* __restrict__ wy,
                        const float* __restrict__ wx, BlendCall a) {
    const TileGeom g = a.g;
    const int K = a.K;
    const int ez = g.tz - 2 * g.oz, ey = g.ty - 2 * g.oy, ex = g.tx - 2 * g.ox;
    const int sub = (int)threadIdx.x & (L - 1);
    const long long groups = (long long)a.n_tiles * g.tz * g.ty * g.tx;
    const long long gpb = 256 / L, passes = (groups + gpb - 1) / gpb;
    for (long long ps = blockIdx.x; ps < passes; ps += gridDim.x) {
        const long long i = ps * gpb + (long long)(threadIdx.x / L);          // (tile of the call, voxel of the tile): the same for the L lanes of a group
        if (i >= groups) continue;
        int jt, lz, ly, lx;
        da_vox4(i, g.tz, g.ty, g.tx, jt, lz, ly, lx);
        const int cur = a.tile0 + jt;
        const int ck = cur % g.gx, cj = (cur / g.gx) % g.gy, ci = cur / (g.gx * g.gy);
        const int z = ci * ez - g.oz + lz, y = cj * ey - g.oy + ly, x = ck * ex - g.ox + lx;
        if (z < 0 || z >= g.D || y < 0 || y >= g.H || x < 0 || x >= g.W) continue;      // the reflect padding
        int zl, zh, yl, yh, xl, xh;
        bd_cover(z, g.tz, g.oz, ez, g.gz, zl, zh);
        bd_cover(y, g.ty, g.oy, ey, g.gy, yl, yh);
        bd_cover(x, g.tx, g.ox, ex, g.gx, xl, xh);
        if (!bd_owns(cur, a.tile0, g.gy, g.gx, zl, zh, yl, yh, xl, xh)) continue;
        float* av = acc + (((long long)z * g.H + y) * g.W + x) * K;
        float s[4];
        bd_load<L, QUAD>(av, sub, K, 0.f, s);
        for (int ta = zl; ta <= zh; ++ta)
            for (int tb = yl; tb <= yh; ++tb)
                for (int tc = xl; tc <= xh; ++tc) {
                    const int r = (ta * g.gy + tb) * g.gx + tc;
                    if (r < a.tile0 || r >= a.tile0 + a.n_tiles) continue;
                    const int mz = z - (ta * ez - g.oz), my = y - (tb * ey - g.oy), mx = x - (tc * ex - g.ox);      // local position in tile r
                    const int fz = (a.flip & 1) ? g.tz - 1 - mz : mz, fy = (a.flip & 2) ? g.ty - 1 - my : my, fx = (a.flip & 4) ? g.tx - 1 - mx : mx;
                    const float* lv = logits + ((((long long)(r - a.tile0) * g.tz + fz) * g.ty + fy) * g.tx + fx) * K;
                    float v[4];
                    bd_load<L, QUAD>(lv, sub, K, -INFINITY, v);
                    const float mxv = da_group_max<L>(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
                    float e[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) e[q] = expf(v[q] - mxv);
                    const float se = da_group_sum<L>((e[0] + e[1]) + (e[2] + e[3]));
                    {
#pragma clang fp contract(off)                                   // w, w p and the sum are rounded one by one: the formula the header states
                        const float w = (wz[mz] * wy[my]) * wx[mx];
#pragma unroll
                        for (int q = 0; q < 4; ++q) { const float wp = w * (e[q] / se); s[q] = s[q] + wp; }
                    }
                }
        bd_store<L, QUAD>(av, sub, K, s);
    }
}

template <int L, bool QUAD>
__global__ void __launch_bounds__(256)
blend_finalize_kernel(const float* __restrict__ acc, long long V, int K, unsigned char* __restrict__ labels, float* __restrict__ conf) {
    const int sub = (int)threadIdx.x & (L - 1);
    const long long gpb = 256 / L, passes = (V + gpb - 1) / gpb;
    for (long long ps = blockIdx.x; ps < passes; ps += gridDim.x) {
        const long long i = ps * gpb + (long long)(threadIdx.x / L);
        if (i >= V) continue;
        float v[4];
        bd_load<L, QUAD>(acc + i * K, sub, K, 0.f, v);
        // first maximum of this lane's channels (ascending), then of the group: the larger value, on a tie the smaller channel
        float best = -INFINITY; int idx = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = bd_channel<L, QUAD>(sub, r);
            if (c < K && (idx == 0x7fffffff || v[r] > best || (v[r] == best && c < idx))) { best = v[r]; idx = c; }
        }
#pragma unroll
        for (int m = 1; m < L; m <<= 1) {
            const float ob = __shfl_xor(best, m); const int oi = __shfl_xor(idx, m);
            if (oi != 0x7fffffff && (idx == 0x7fffffff || ob > best || (ob == best && oi < idx))) { best = ob; idx = oi; }
        }
        // sum in class order, in double (the confidence then carries the sums' own error alone): the running sum goes from holder to holder
        double run = 0.0;
        if (conf) {
            if (QUAD) {
                for (int sl = 0; sl < L; ++sl) {
                    const double t = (((run + (double)v[0]) + (double)v[1]) + (double)v[2]) + (double)v[3];
                    run = __shfl(t, sl, L);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    for (int sl = 0; sl < L && sl + r * L < K; ++sl) {
                        const double t = run + (double)v[r];
                        run = __shfl(t, sl, L);
                    }
            }
        }
        if (sub == 0) {
            const int lab = (idx >= 0 && idx < K) ? idx : 0;
            labels[i] = (unsigned char)lab;
            if (conf) conf[i] = (float)((double)best / run);
        }
    }
}

// lanes per voxel and the access form for K channels at these addresses
int bd_lanes(int K, const void* p0, const void* p1, bool& quad) {
    const int q = K / 4;
    quad = K % 4 == 0 && (q & (q - 1)) == 0 && q <= 64 && (((size_t)p0 | (size_t)p1) & 15) == 0;
    if (quad) return q;
    int L = 2;
    while (L < K && L < 64) L <<= 1;
    return L;
}

}  // namespace

#define BD_DISPATCH(KERNEL, L, quad, grid, st, ...)                                                                                       \
    do {                                                                                                                                  \
        if (quad) switch (L) {                                                                                                            \
            case 1: hipLaunchKernelGGL((KERNEL<1, true>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                                \
            case 2: hipLaunchKernelGGL((KERNEL<2, true>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                                \
            case 4: hipLaunchKernelGGL((KERNEL<4, true>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                                \
            case 8: hipLaunchKernelGGL((KERNEL<8, true>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                                \
            case 16: hipLaunchKernelGGL((KERNEL<16, true>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                              \
            case 32: hipLaunchKernelGGL((KERNEL<32, true>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                              \
            default: hipLaunchKernelGGL((KERNEL<64, true>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                              \
        } else switch (L) {                                                                                                               \
            case 2: hipLaunchKernelGGL((KERNEL<2, false>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                               \
            case 4: hipLaunchKernelGGL((KERNEL<4, false>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                               \
            case 8: hipLaunchKernelGGL((KERNEL<8, false>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                               \
            case 16: hipLaunchKernelGGL((KERNEL<16, false>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                             \
            case 32: hipLaunchKernelGGL((KERNEL<32, false>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                             \
            default: hipLaunchKernelGGL((KERNEL<64, false>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                             \
        }                                                                                                                                 \
    } while (0)

extern "C" int da_blend_accumulate(const float* logits, float* acc, int D, int H, int W, int K, const int* tile3, const int* overlap3, int tile0,
                                   int n_tiles, const float* wz, const float* wy, const float* wx, int flip, void* stream) {
    BlendCall a;
    if (!logits || !acc || !tile3 || !overlap3 || !wz || !wy || !wx || tile_geom(a.g, D, H, W, tile3, overlap3)) return DA_ERR_BADARG;
    if (K < 2 || K > kBlendMaxK || flip < 0 || flip > 7 || tile0 < 0 || n_tiles < 1) return DA_ERR_BADARG;
    if ((long long)tile0 + n_tiles > (long long)a.g.gz * a.g.gy * a.g.gx) return DA_ERR_BADARG;
    a.K = K; a.tile0 = tile0; a.n_tiles = n_tiles; a.flip = flip;
    bool quad;
    const int L = bd_lanes(K, logits, acc, quad);
    const long long groups = (long long)n_tiles * a.g.tz * a.g.ty * a.g.tx;
    const int grid = da_grid(groups * L, 256);
    BD_DISPATCH(blend_accumulate_kernel, L, quad, grid, da_stream(stream), logits, acc, wz, wy, wx, a);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_blend_finalize(const float* acc, long long V, int K, unsigned char* labels, float* conf, void* stream) {
    if (!acc || !labels || V < 1 || K < 2 || K > kBlendMaxK) return DA_ERR_BADARG;
    bool quad;
    const int L = bd_lanes(K, acc, acc, quad);
    const int grid = da_grid(V * L, 256);
    BD_DISPATCH(blend_finalize_kernel, L, quad, grid, da_stream(stream), acc, V, K, labels, conf);
    DA_LAUNCH_CHECK();
    return 0;
}
