// Applying a registration on the files' own grids: the cubic B-spline prefilter and the warp through frames (include/deepatlas_hip.h).
// The net's field lives on the prepared grid (resampled, flipped, cropped); the scans live on their files' grids.  da_warp_frames pushes one
// sample position per output voxel of the FIXED file's grid through fixed frame -> field -> moving frame and interpolates the native moving
// data once: no resample of the moving scan before the warp, none of the result after it.  Frames are per-axis pairs (a, b), native index =
// a * prepared index + b (lib/inference.py frame_of), carried in double: a crop offset of hundreds of voxels next to a sub-voxel displacement.
// The field is sampled by da_field_sample_border (common.h), the B[u] of fieldinv.hip.
// Prefilter: three launches, W, then H, then D.  Along W a lane cannot own a line and stay coalesced, so the pass sums the filter's two-sided
// impulse response h_k = sqrt(3) z^|k| directly (DA_BSPLINE_HORIZON taps per side, |z|^25 = 5e-15) from an LDS copy of the flattened elements
// e0 - K ... e0 + 255 + K around the workgroup's 256 outputs: a mirrored tap of element (row, w) lies in the same row at a distance < K, hence
// inside that copy whatever W is, and rows shorter than the workgroup need no case of their own.  Along H and D one lane owns a line, lanes
// along W, and runs the two recursions in place, 16 independent loads ahead of each dependent chain.
#include <string.h>
#include "common.h"

namespace {

constexpr int kK = DA_BSPLINE_HORIZON;
constexpr int kRowBlock = 256;
constexpr int kLineBlock = 64;       // one wave per workgroup: a 160 x 384 x 384 volume has 61440 H lines, 960 waves for 256 CUs
constexpr int kAhead = 16;
constexpr float kPole = -0.26794919243112270647f;             // sqrt(3) - 2
constexpr float kRowGain = 1.73205080756887729353f;           // sqrt(3) = 6 * (-z / (1 - z^2)): h_0, the gain 6 included
constexpr float kLastGain = 0.28867513459481288225f;          // z / (z^2 - 1) = 1 / (2 sqrt(3))

// whole-sample mirror of any integer onto 0 ... n - 1 (period 2 n - 2; n = 1: 0)
__device__ __forceinline__ int ra_mirror(int i, int n) {
    if (n == 1) return 0;
    const int per = 2 * n - 2;
    i %= per;
    if (i < 0) i += per;
    return i < n ? i : per - i;
}

__global__ void __launch_bounds__(kRowBlock)
bspline_row_kernel(const void* __restrict__ src, int dtype, float* __restrict__ dst, long long total, int W, int filter) {
    __shared__ float tile[kRowBlock + 2 * kK];
    const long long e0 = (long long)blockIdx.x * kRowBlock;
    for (int j = threadIdx.x; j < kRowBlock + 2 * kK; j += kRowBlock) {
        const long long e = e0 - kK + j;
        tile[j] = (e >= 0 && e < total) ? da_load_as_f32(src, dtype, e) : 0.f;
    }
    __syncthreads();
    const long long e = e0 + threadIdx.x;
    if (e >= total) return;
    const float* c = tile + kK + threadIdx.x;
    if (!filter) { dst[e] = c[0]; return; }
    const int w = (int)((unsigned)e % (unsigned)W);        // total < 2^31
    float acc = 0.f;
    if (w >= kK && w + kK < W) {
#pragma unroll
        for (int k = kK; k >= 1; --k) acc = kPole * (acc + (c[-k] + c[k]));
    } else {
        for (int k = kK; k >= 1; --k) acc = kPole * (acc + (c[ra_mirror(w - k, W) - w] + c[ra_mirror(w + k, W) - w]));
    }
    dst[e] = kRowGain * (c[0] + acc);
}

// line L = (outer, in): elements base + k * inner, k < n, base = outer * n * inner + in; neighbouring lanes neighbouring `in`
__global__ void __launch_bounds__(kLineBlock)
bspline_line_kernel(float* __restrict__ v, long long lines, int n, long long inner) {
    const long long L = (long long)blockIdx.x * kLineBlock + threadIdx.x;
    if (L >= lines) return;
    const long long outer = L / inner;
    float* p = v + outer * n * inner + (L - outer * inner);
    // causal start under the mirror: c+[0] = 6 sum_k z^k x[mirror(k)], Horner from the outermost term
    float cp = p[ra_mirror(kK, n) * inner];
    for (int k = kK - 1; k >= 0; --k) cp = cp * kPole + p[ra_mirror(k, n) * inner];
    cp *= 6.f;
    float prev = cp;                 // c+[k - 2] once the causal pass is done
    p[0] = cp;
    for (int k0 = 1; k0 < n; k0 += kAhead) {
        float x[kAhead];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) x[j] = (k0 + j < n) ? p[(k0 + j) * inner] : 0.f;
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            if (k0 + j < n) { prev = cp; cp = 6.f * x[j] + kPole * cp; p[(k0 + j) * inner] = cp; }
        }
    }
    // anticausal: c[n - 1] = z / (z^2 - 1) (c+[n - 1] + z c+[n - 2]), c[k] = z (c[k + 1] - c+[k])
    float c = kLastGain * (cp + kPole * prev);
    p[(long long)(n - 1) * inner] = c;
    for (int k0 = n - 2; k0 >= 0; k0 -= kAhead) {
        float x[kAhead];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) x[j] = (k0 - j >= 0) ? p[(k0 - j) * inner] : 0.f;
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            if (k0 - j >= 0) { c = kPole * (c - x[j]); p[(k0 - j) * inner] = c; }
        }
    }
}

// ---- the warp through frames ------------------------------------------------------------------------------------------------------------
struct WfParams {
    double inv_af[3], bf[3], am[3], bm[3];      // (D, H, W)
    double Mf[9], Mm[9], t[3];                  // world: M_m y - M_f x + t, acting on (w, h, d)
    int C, Dm, Hm, Wm, Dp, Hp, Wp, Do, Ho, Wo;
};

// y (D, H, W) of output voxel (d, h, w); false: the position is refused and no memory may be read for it
__device__ __forceinline__ bool wf_position(const WfParams& P, const float* __restrict__ disp, const DaFieldDims& m, int d, int h, int w, double (&y)[3]) {
    const double pd = ((double)d - P.bf[0]) * P.inv_af[0], ph = ((double)h - P.bf[1]) * P.inv_af[1], pw = ((double)w - P.bf[2]) * P.inv_af[2];
    const float fd = (float)pd, fh = (float)ph, fw = (float)pw;
    if (!da_is_finite_coord(fw, fh, fd)) return false;
    float bx, by, bz;
    da_field_sample_border(disp, m, da_id_coord(fw, m.W), da_id_coord(fh, m.H), da_id_coord(fd, m.D), bx, by, bz);
    const float ux = bx * m.sx, uy = by * m.sy, uz = bz * m.sz;
    y[0] = P.am[0] * (pd + (double)uz) + P.bm[0];
    y[1] = P.am[1] * (ph + (double)uy) + P.bm[1];
    y[2] = P.am[2] * (pw + (double)ux) + P.bm[2];
    return fabs(y[0]) < 1e9 && fabs(y[1]) < 1e9 && fabs(y[2]) < 1e9;
}

__device__ __forceinline__ bool wf_inside(const double (&y)[3], int Dm, int Hm, int Wm) {
    return y[0] >= -0.5 && y[0] < (double)Dm - 0.5 && y[1] >= -0.5 && y[1] < (double)Hm - 0.5 && y[2] >= -0.5 && y[2] < (double)Wm - 0.5;
}

__device__ __forceinline__ void wf_world(const WfParams& P, float* __restrict__ world, long long V, long long v, int d, int h, int w, bool ok,
                                         const double (&y)[3]) {
    if (!world) return;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double val = (P.Mm[3 * r] * y[2] + P.Mm[3 * r + 1] * y[1] + P.Mm[3 * r + 2] * y[0])
                         - (P.Mf[3 * r] * (double)w + P.Mf[3 * r + 1] * (double)h + P.Mf[3 * r + 2] * (double)d) + P.t[r];
        world[r * V + v] = ok ? (float)val : NAN;
    }
}

// linear taps of one axis by ops.resample_axis_table's rule; y is inside
__device__ __forceinline__ void wf_linear_taps(double y, int n, int& lo, int& hi, float& t) {
    const double f = floor(y);
    lo = min(max((int)f, 0), n - 1);
    hi = min(lo + 1, n - 1);
    t = y < 0.0 ? 0.f : (float)(y - f);
}

// order 0: T = an unsigned type of the element's width, copied bit for bit; `refused` = what a refused position stores (NaN bits or the default)
template <typename T>
__global__ void __launch_bounds__(256)
warp_frames_nearest_kernel(const T* __restrict__ mov, const float* __restrict__ disp, T* __restrict__ out, float* __restrict__ world, WfParams P,
                           T dflt, T refused) {
    const long long V = (long long)P.Do * P.Ho * P.Wo, Vm = (long long)P.Dm * P.Hm * P.Wm;
    const DaFieldDims m = da_field_dims(P.Dp, P.Hp, P.Wp);
    for (DaXcdLoop L = da_xcd_loop(V, 256); L.i < L.end; L.i += L.step) {
        int d, h, w; da_vox3(L.i, P.Ho, P.Wo, d, h, w);
        double y[3];
        const bool ok = wf_position(P, disp, m, d, h, w, y);
        wf_world(P, world, V, L.i, d, h, w, ok, y);
        long long at = -1;
        if (ok && wf_inside(y, P.Dm, P.Hm, P.Wm)) {
            const int zd = min(max((int)floor(y[0] + 0.5), 0), P.Dm - 1), zh = min(max((int)floor(y[1] + 0.5), 0), P.Hm - 1),
                      zw = min(max((int)floor(y[2] + 0.5), 0), P.Wm - 1);
            at = ((long long)zd * P.Hm + zh) * P.Wm + zw;
        }
        for (int c = 0; c < P.C; ++c) out[c * V + L.i] = at >= 0 ? mov[c * Vm + at] : (ok ? dflt : refused);
    }
}

template <int ORDER>
__global__ void __launch_bounds__(256)
warp_frames_kernel(const void* __restrict__ mov, int dtype, const float* __restrict__ disp, float* __restrict__ out, float* __restrict__ world,
                   WfParams P, float dflt) {
    const long long V = (long long)P.Do * P.Ho * P.Wo, Vm = (long long)P.Dm * P.Hm * P.Wm;
    const DaFieldDims m = da_field_dims(P.Dp, P.Hp, P.Wp);
    for (DaXcdLoop L = da_xcd_loop(V, 256); L.i < L.end; L.i += L.step) {
        int d, h, w; da_vox3(L.i, P.Ho, P.Wo, d, h, w);
        double y[3];
        const bool ok = wf_position(P, disp, m, d, h, w, y);
        wf_world(P, world, V, L.i, d, h, w, ok, y);
        if (!ok || !wf_inside(y, P.Dm, P.Hm, P.Wm)) {
            for (int c = 0; c < P.C; ++c) out[c * V + L.i] = ok ? dflt : NAN;
            continue;
        }
        if (ORDER == 1) {
            int d0, d1, h0, h1, w0, w1; float td, th, tw;
            wf_linear_taps(y[0], P.Dm, d0, d1, td); wf_linear_taps(y[1], P.Hm, h0, h1, th); wf_linear_taps(y[2], P.Wm, w0, w1, tw);
            for (int c = 0; c < P.C; ++c) {
                const long long b = c * Vm;
                float plane[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const long long r0 = b + ((long long)(i ? d1 : d0) * P.Hm + h0) * P.Wm, r1 = b + ((long long)(i ? d1 : d0) * P.Hm + h1) * P.Wm;
                    const float a0 = da_load_as_f32(mov, dtype, r0 + w0), a1 = da_load_as_f32(mov, dtype, r0 + w1);
                    const float b0 = da_load_as_f32(mov, dtype, r1 + w0), b1 = da_load_as_f32(mov, dtype, r1 + w1);
                    const float ra = fmaf(tw, a1 - a0, a0), rb = fmaf(tw, b1 - b0, b0);
                    plane[i] = fmaf(th, rb - ra, ra);
                }
                out[c * V + L.i] = fmaf(td, plane[1] - plane[0], plane[0]);
            }
        } else {
            const float* coef = (const float*)mov;
            int id[4], ih[4], iw[4]; float gd[4], gh[4], gw[4];
            const double fy[3] = {floor(y[0]), floor(y[1]), floor(y[2])};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float t = (float)(y[a] - fy[a]), t2 = t * t, t3 = t2 * t, s = 1.f - t;
                float* g = a == 0 ? gd : (a == 1 ? gh : gw);
                int* ix = a == 0 ? id : (a == 1 ? ih : iw);
                const int n = a == 0 ? P.Dm : (a == 1 ? P.Hm : P.Wm);
                g[0] = s * s * s * (1.f / 6.f);
                g[1] = (3.f * t3 - 6.f * t2 + 4.f) * (1.f / 6.f);
                g[2] = (-3.f * t3 + 3.f * t2 + 3.f * t + 1.f) * (1.f / 6.f);
                g[3] = t3 * (1.f / 6.f);
#pragma unroll
                for (int k = 0; k < 4; ++k) ix[k] = ra_mirror((int)fy[a] - 1 + k, n);
            }
            for (int c = 0; c < P.C; ++c) {
                const float* b = coef + c * Vm;
                float sd = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float sh = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float* r = b + ((long long)id[i] * P.Hm + ih[j]) * P.Wm;
                        float sw = gw[0] * r[iw[0]];
                        sw = fmaf(gw[1], r[iw[1]], sw); sw = fmaf(gw[2], r[iw[2]], sw); sw = fmaf(gw[3], r[iw[3]], sw);
                        sh = fmaf(gh[j], sw, sh);
                    }
                    sd = fmaf(gd[i], sh, sd);
                }
                out[c * V + L.i] = sd;
            }
        }
    }
}

int wf_blocks(long long V) {
    int g = da_grid(V, 256);
    if (g >= 8) g = g / 8 * 8;          // a multiple of 8 takes the XCD-contiguous split
    return g;
}

template <typename T>
int wf_launch_nearest(const void* mov, const float* disp, void* out, float* world, const WfParams& P, T dflt, T refused, long long V, hipStream_t st) {
    hipLaunchKernelGGL((warp_frames_nearest_kernel<T>), dim3(wf_blocks(V)), dim3(256), 0, st, (const T*)mov, disp, (T*)out, world, P, dflt, refused);
    DA_LAUNCH_CHECK();
    return 0;
}

bool ra_finite(double v) { return v == v && v - v == 0.0; }

}  // namespace

extern "C" int da_bspline3_prefilter(const void* src, int src_dtype, float* dst, int C, int D, int H, int W, int axes, void* stream) {
    if (!src || !dst || (const void*)src == (const void*)dst || src_dtype < 0 || src_dtype > 4 || C < 1 || D < 1 || H < 1 || W < 1 || axes < 0 || axes > 7)
        return DA_ERR_BADARG;
    const long long total = (long long)C * D * H * W;
    if (total >= 0x7FFFFFFFLL) return DA_ERR_UNSUPPORTED;
    hipStream_t st = da_stream(stream);
    hipLaunchKernelGGL(bspline_row_kernel, dim3((unsigned)da_cdiv(total, kRowBlock)), dim3(kRowBlock), 0, st, src, src_dtype, dst, total, W,
                       ((axes & 1) && W > 1) ? 1 : 0);
    DA_LAUNCH_CHECK();
    if ((axes & 2) && H > 1) {
        const long long lines = (long long)C * D * W;
        hipLaunchKernelGGL(bspline_line_kernel, dim3((unsigned)da_cdiv(lines, kLineBlock)), dim3(kLineBlock), 0, st, dst, lines, H, (long long)W);
        DA_LAUNCH_CHECK();
    }
    if ((axes & 4) && D > 1) {
        const long long lines = (long long)C * H * W;
        hipLaunchKernelGGL(bspline_line_kernel, dim3((unsigned)da_cdiv(lines, kLineBlock)), dim3(kLineBlock), 0, st, dst, lines, D, (long long)H * W);
        DA_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int da_warp_frames(const void* moving, int src_dtype, const float* disp, void* out, float* world, int C, int Dm, int Hm, int Wm,
                              int Dp, int Hp, int Wp, int Do, int Ho, int Wo, const double* frames, const double* affines, int order,
                              double default_value, void* stream) {
    if (!moving || !disp || !out || !frames || src_dtype < 0 || src_dtype > 4 || C < 1 || Dm < 1 || Hm < 1 || Wm < 1 || Dp < 2 || Hp < 2 || Wp < 2 ||
        Do < 1 || Ho < 1 || Wo < 1 || (order != 0 && order != 1 && order != 3) || (order == 3 && src_dtype != 0) || (world && !affines))
        return DA_ERR_BADARG;
    WfParams P;
    for (int a = 0; a < 3; ++a) {
        const double af = frames[2 * a], bf = frames[2 * a + 1], am = frames[6 + 2 * a], bm = frames[6 + 2 * a + 1];
        if (!ra_finite(af) || !ra_finite(bf) || !ra_finite(am) || !ra_finite(bm) || af == 0.0 || am == 0.0) return DA_ERR_BADARG;
        P.inv_af[a] = 1.0 / af; P.bf[a] = bf; P.am[a] = am; P.bm[a] = bm;
        if (!ra_finite(P.inv_af[a])) return DA_ERR_BADARG;
    }
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) { P.Mf[3 * r + k] = affines ? affines[4 * r + k] : 0.0; P.Mm[3 * r + k] = affines ? affines[12 + 4 * r + k] : 0.0; }
        P.t[r] = affines ? affines[12 + 4 * r + 3] - affines[4 * r + 3] : 0.0;
    }
    const long long V = (long long)Do * Ho * Wo, Vm = (long long)Dm * Hm * Wm, Vp = (long long)Dp * Hp * Wp;
    if (C * V >= 0x7FFFFFFFLL || C * Vm >= 0x7FFFFFFFLL || Vp >= 0x7FFFFFFFLL / 4) return DA_ERR_UNSUPPORTED;
    P.C = C; P.Dm = Dm; P.Hm = Hm; P.Wm = Wm; P.Dp = Dp; P.Hp = Hp; P.Wp = Wp; P.Do = Do; P.Ho = Ho; P.Wo = Wo;
    hipStream_t st = da_stream(stream);
    if (order == 0) {
        if (src_dtype == 0) {
            const float f = (float)default_value; unsigned bits; memcpy(&bits, &f, 4);
            return wf_launch_nearest<unsigned>(moving, disp, out, world, P, bits, 0x7FC00000u, V, st);
        }
        if (src_dtype == 1) {
            unsigned long long bits; memcpy(&bits, &default_value, 8);
            return wf_launch_nearest<unsigned long long>(moving, disp, out, world, P, bits, 0x7FF8000000000000ULL, V, st);
        }
        if (src_dtype == 2) return wf_launch_nearest<unsigned short>(moving, disp, out, world, P, (unsigned short)(short)default_value, (unsigned short)(short)default_value, V, st);
        if (src_dtype == 3) return wf_launch_nearest<unsigned char>(moving, disp, out, world, P, (unsigned char)default_value, (unsigned char)default_value, V, st);
        return wf_launch_nearest<unsigned>(moving, disp, out, world, P, (unsigned)(int)default_value, (unsigned)(int)default_value, V, st);
    }
    if (order == 1)
        hipLaunchKernelGGL((warp_frames_kernel<1>), dim3(wf_blocks(V)), dim3(256), 0, st, moving, src_dtype, disp, (float*)out, world, P, (float)default_value);
    else
        hipLaunchKernelGGL((warp_frames_kernel<3>), dim3(wf_blocks(V)), dim3(256), 0, st, moving, src_dtype, disp, (float*)out, world, P, (float)default_value);
    DA_LAUNCH_CHECK();
    return 0;
}
