// Intensity augmentation on the device: the reference's two image filters GaussianBlur and BilateralFilter (lib/transforms.py:293-320:
// sitk.DiscreteGaussian / sitk.Bilateral) and the project's own fused pointwise pass (bias field, gamma, gain / offset, noise, clamp).
// Images are [N][C][D][H][W] fp32, planar; every kernel reads a per-sample `apply` flag (or flag word) and copies an untouched sample
// through bit for bit in the same launch.  No atomics, fixed summation orders: results are bit-identical from run to run.
// Definitions, bytes moved and measurements: DESIGN.md 4.30.
#include "common.h"
#include "bspline.h"
#include "counter_hash.h"

namespace {

constexpr int kBlock = 256;

// ---- separable Gaussian blur -----------------------------------------------------------------------------------------------------
// Three line passes (W, H, D), one voxel per thread, consecutive threads on consecutive W in every pass, so the H and D passes read 64
// neighbouring lines per wave with full 256-byte rows.  out[i] = sum_k taps[axis][k] * in[clamp(i + k - R)], k ascending (ZeroFluxNeumann).
// Pass 1 writes `out`, pass 2 `tmp`, pass 3 `out` again; a sample whose flag is 0 is copied by pass 1 and skipped by the other two.
template <int AXIS>
__global__ __launch_bounds__(kBlock) void blur_axis_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ taps,
                                                           const int* __restrict__ apply, int R, int C, int D, int H, int W, int first) {
    __shared__ float t[2 * DA_BLUR_MAX_RADIUS + 1];
    const int nc = blockIdx.y;
    const bool on = apply[nc / C] != 0;
    if (!on && !first) return;
    const int K = 2 * R + 1;
    if (threadIdx.x < K) t[threadIdx.x] = taps[AXIS * K + threadIdx.x];
    __syncthreads();
    const long long vol = (long long)D * H * W;
    const float* s = src + (long long)nc * vol;
    float* o = dst + (long long)nc * vol;
    const int len = AXIS == 0 ? W : (AXIS == 1 ? H : D);
    const int stride = AXIS == 0 ? 1 : (AXIS == 1 ? W : H * W);
    for (DaXcdLoop L = da_xcd_loop(vol); L.i < L.end; L.i += L.step) {
        const int v = (int)L.i;
        if (!on) { o[v] = s[v]; continue; }
        int d, h, w; da_vox3(L.i, H, W, d, h, w);
        const int i = AXIS == 0 ? w : (AXIS == 1 ? h : d);
        const int base = v - i * stride;
        float acc = 0.f;
        for (int k = 0; k < K; ++k) {
            const int j = min(max(i + k - R, 0), len - 1);
            acc = fmaf(t[k], s[base + j * stride], acc);
        }
        o[v] = acc;
    }
}

template <int AXIS>
int launch_blur(const float* src, float* dst, const float* taps, const int* apply, int R, int N, int C, int D, int H, int W, int first, hipStream_t st) {
    const long long vol = (long long)D * H * W;
    long long bx = da_cdiv(da_cdiv(vol, kBlock), 8) * 8;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(blur_axis_kernel<AXIS>, dim3((unsigned)bx, (unsigned)(N * C)), dim3(kBlock), 0, st, src, dst, taps, apply, R, C, D, H, W, first);
    DA_LAUNCH_CHECK();
    return 0;
}

// ---- bilateral filter ------------------------------------------------------------------------------------------------------------
// One workgroup per DA_BILATERAL_TILE_D x _H x _W output tile of one (sample, channel) volume.  The tile plus its halo (indices clamped to
// the volume) is staged once in LDS with the range table and the domain weights; thread (th, tw) owns the TD outputs of its (h, w) column
// and walks the taps in (z, y, x) order with the domain weight read once (a broadcast) per offset for all TD outputs.  Per tap: one LDS
// read of the neighbour, one of the table, a subtract, |.|, compare, multiply, floor, convert, two fused multiply-adds.  The sums run over
// the differences b - a: out = a + sum w (b - a) / sum w, the same quotient as sum w b / sum w and exact on a constant neighbourhood.
constexpr int TD = DA_BILATERAL_TILE_D, TH = DA_BILATERAL_TILE_H, TW = DA_BILATERAL_TILE_W;
static_assert(TH * TW == kBlock, "one thread per (h, w) column of the tile");

struct BilGeom {
    int C, D, H, W;
    int rx, ry, rz, S;
    int ntx, nty, ntz;
    float cutoff, scale;
};

__global__ __launch_bounds__(kBlock) void bilateral_kernel(const float* __restrict__ img, float* __restrict__ out, const float* __restrict__ wd,
                                                           const float* __restrict__ table, const int* __restrict__ apply, BilGeom g) {
    extern __shared__ float lds[];
    const int PW = TW + 2 * g.rx, PH = TH + 2 * g.ry, PD = TD + 2 * g.rz;
    const int KX = 2 * g.rx + 1, KY = 2 * g.ry + 1, KZ = 2 * g.rz + 1;
    float* tile = lds;
    float* sT = tile + PD * PH * PW;
    float* sW = sT + g.S;
    const int nc = blockIdx.y;
    int t = blockIdx.x;
    const int tx = t % g.ntx; t /= g.ntx;
    const int ty = t % g.nty;
    const int tz = t / g.nty;
    const int w0 = tx * TW, h0 = ty * TH, d0 = tz * TD;
    const int D = g.D, H = g.H, W = g.W;
    const long long vol = (long long)D * H * W;
    const float* s = img + (long long)nc * vol;
    float* o = out + (long long)nc * vol;
    const int tw = threadIdx.x % TW, th = threadIdx.x / TW;
    const int w = w0 + tw, h = h0 + th;
    const bool inside = w < W && h < H;
    if (apply[nc / g.C] == 0) {
        if (inside)
            for (int j = 0; j < TD && d0 + j < D; ++j) { const int v = ((d0 + j) * H + h) * W + w; o[v] = s[v]; }
        return;
    }
    for (int i = threadIdx.x; i < PD * PH * PW; i += kBlock) {
        const int x = i % PW, r = i / PW;
        const int y = r % PH, z = r / PH;
        const int gw = min(max(w0 - g.rx + x, 0), W - 1);
        const int gh = min(max(h0 - g.ry + y, 0), H - 1);
        const int gd = min(max(d0 - g.rz + z, 0), D - 1);
        tile[i] = s[(gd * H + gh) * W + gw];
    }
    for (int i = threadIdx.x; i < g.S; i += kBlock) sT[i] = table[i];
    for (int i = threadIdx.x; i < KZ * KY * KX; i += kBlock) sW[i] = wd[i];
    __syncthreads();
    const int plane = PH * PW;
    float a[TD], num[TD], den[TD];
#pragma unroll
    for (int j = 0; j < TD; ++j) {
        a[j] = tile[(j + g.rz) * plane + (th + g.ry) * PW + tw + g.rx];
        num[j] = 0.f; den[j] = 0.f;
    }
    const float cutoff = g.cutoff, scale = g.scale;
    const int last = g.S - 1;
    for (int dz = 0; dz < KZ; ++dz) {
        for (int dy = 0; dy < KY; ++dy) {
            const float* row = tile + dz * plane + (th + dy) * PW + tw;
            const float* wrow = sW + (dz * KY + dy) * KX;
            for (int dx = 0; dx < KX; ++dx) {
                const float wdv = wrow[dx];
#pragma unroll
                for (int j = 0; j < TD; ++j) {
                    const float diff = row[j * plane + dx] - a[j];
                    const float delta = fabsf(diff);
                    if (delta < cutoff) {                                   // false for a NaN neighbour or centre: the tap is skipped
                        const int idx = min((int)floorf(delta * scale), last);
                        const float wgt = wdv * sT[idx];
                        num[j] = fmaf(wgt, diff, num[j]);
                        den[j] += wgt;
                    }
                }
            }
        }
    }
    if (inside) {
#pragma unroll
        for (int j = 0; j < TD; ++j)
            if (d0 + j < D) o[((d0 + j) * H + h) * W + w] = a[j] + num[j] / den[j];     // NaN centre: 0 / 0
    }
}

// ---- fused pointwise pass --------------------------------------------------------------------------------------------------------
// grid: x = workgroups per sample, y = sample.  Each thread owns 4 consecutive W voxels of every channel.  Per-sample parameters:
// DA_INTENSITY_PARAM_STRIDE 32-bit words [flags, gamma, gain, offset, sigma, seed, -, -].  A stage whose bit is off does no arithmetic.
constexpr int kVec = 4;

struct PwGeom {
    int C, D, H, W;
    int Mx, My, Mz, gx, gy, gz;
    int sample0;
};

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

template <int O>
__global__ __launch_bounds__(kBlock) void intensity_kernel(const float* __restrict__ img, float* __restrict__ out, const float* __restrict__ params,
                                                           const float* __restrict__ coef, PwGeom g) {
    extern __shared__ float cg[];
    const int n = blockIdx.y;
    const float* P = params + (long long)n * DA_INTENSITY_PARAM_STRIDE;
    unsigned flags = __float_as_uint(P[0]);
    if constexpr (O == 0) flags &= ~(unsigned)DA_INTENSITY_BIAS;
    const float gamma = P[1], gain = P[2], offset = P[3], sigma = P[4];
    const unsigned seed = __float_as_uint(P[5]);
    const int D = g.D, H = g.H, W = g.W;
    const long long vol = (long long)D * H * W;
    if constexpr (O > 0) {
        if (flags & DA_INTENSITY_BIAS) {
            const int gp = g.gx * g.gy * g.gz;
            const float* src = coef + (long long)n * gp;
            for (int k = threadIdx.x; k < gp; k += kBlock) cg[k] = src[k];
            __syncthreads();
        }
    }
    const float* im = img + (long long)n * g.C * vol;
    float* io = out + (long long)n * g.C * vol;
    const unsigned long long ctr0 = (unsigned long long)((long long)g.sample0 + n) * (unsigned long long)(g.C * vol);
    const int QW = (W + kVec - 1) / kVec;
    const bool vec = (W % kVec) == 0;
    const long long items = (long long)D * H * QW;
    for (DaXcdLoop L = da_xcd_loop(items); L.i < L.end; L.i += L.step) {
        int d, h, qw; da_vox3(L.i, H, QW, d, h, qw);
        const int w0 = qw * kVec;
        float fac[kVec];
        if constexpr (O > 0) {
            if (flags & DA_INTENSITY_BIAS) {
                float wy[O + 1], wz[O + 1];
                const int sy = bspline_axis<O>(h, g.My, H, wy), sz = bspline_axis<O>(d, g.Mz, D, wz);
#pragma unroll
                for (int j = 0; j < kVec; ++j) {
                    float wx[O + 1];
                    const int sx = bspline_axis<O>(min(w0 + j, W - 1), g.Mx, W, wx);
                    fac[j] = expf(bspline_contract<O>(cg, g.gx, g.gy, sx, sy, sz, wx, wy, wz));
                }
            }
        }
        const long long row = ((long long)d * H + h) * W + w0;
        for (int c = 0; c < g.C; ++c) {
            const float* p = im + c * vol + row;
            float x[kVec];
            if (vec) {
                const float4 q = *reinterpret_cast<const float4*>(p);
                x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < kVec; ++j) x[j] = p[min(j, W - 1 - w0)];       // (a tail lane repeats the last voxel; it is not stored)
            }
            if constexpr (O > 0) {
                if (flags & DA_INTENSITY_BIAS) {
#pragma unroll
                    for (int j = 0; j < kVec; ++j) x[j] *= fac[j];
                }
            }
            if (flags & DA_INTENSITY_GAMMA) {
#pragma unroll
                for (int j = 0; j < kVec; ++j) {
                    const float xc = clamp01(x[j]);
                    x[j] = (flags & DA_INTENSITY_INVERT) ? 1.f - powf(1.f - xc, gamma) : powf(xc, gamma);
                }
            }
            if (flags & DA_INTENSITY_LINEAR) {
#pragma unroll
                for (int j = 0; j < kVec; ++j) x[j] = fmaf(gain, x[j], offset);
            }
            if (flags & DA_INTENSITY_NOISE) {
#pragma unroll
                for (int j = 0; j < kVec; ++j) {
                    const unsigned long long ctr = ctr0 + (unsigned long long)(c * vol + row + j);
                    // two 24-bit uniforms in (0, 1): (k + 0.5) 2^-24, one rounding
                    const float u1 = fmaf((float)(da_synth_bits(seed, ctr, DA_INTENSITY_STREAM_U1) >> 8), 0x1p-24f, 0x1p-25f);
                    const float u2 = fmaf((float)(da_synth_bits(seed, ctr, DA_INTENSITY_STREAM_U2) >> 8), 0x1p-24f, 0x1p-25f);
                    const float nrm = sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
                    x[j] = fmaf(sigma, nrm, x[j]);
                }
            }
            if (flags & DA_INTENSITY_CLAMP) {
#pragma unroll
                for (int j = 0; j < kVec; ++j) x[j] = clamp01(x[j]);
            }
            float* q = io + c * vol + row;
            if (vec) {
                *reinterpret_cast<float4*>(q) = make_float4(x[0], x[1], x[2], x[3]);
            } else {
#pragma unroll
                for (int j = 0; j < kVec; ++j)
                    if (w0 + j < W) q[j] = x[j];
            }
        }
    }
}

template <int O>
int launch_intensity(const float* img, float* out, const float* params, const float* coef, const PwGeom& g, int N, hipStream_t st) {
    const long long items = (long long)g.D * g.H * ((g.W + kVec - 1) / kVec);
    long long bx = da_cdiv(da_cdiv(items, kBlock), 8) * 8;
    if (bx > 1024) bx = 1024;
    const size_t lds = O > 0 ? (size_t)g.gx * g.gy * g.gz * sizeof(float) : 0;
    hipLaunchKernelGGL(intensity_kernel<O>, dim3((unsigned)bx, (unsigned)N), dim3(kBlock), lds, st, img, out, params, coef, g);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int da_gauss_blur3d(const float* img, float* out, float* tmp, const float* taps, int radius, const int* apply,
                               int N, int C, int D, int H, int W, void* stream) {
    if (!img || !out || !tmp || !taps || !apply || img == out || img == tmp || out == tmp) return DA_ERR_BADARG;
    if (N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || radius < 0) return DA_ERR_BADARG;
    if (radius > DA_BLUR_MAX_RADIUS || (long long)N * C > 65535) return DA_ERR_UNSUPPORTED;
    if ((long long)D * H * W > 0x7FFFFFFFLL) return DA_ERR_UNSUPPORTED;                     // 32-bit offsets inside one volume
    hipStream_t st = da_stream(stream);
    int rc = launch_blur<0>(img, out, taps, apply, radius, N, C, D, H, W, 1, st);
    if (rc) return rc;
    rc = launch_blur<1>(out, tmp, taps, apply, radius, N, C, D, H, W, 0, st);
    if (rc) return rc;
    return launch_blur<2>(tmp, out, taps, apply, radius, N, C, D, H, W, 0, st);
}

extern "C" int da_bilateral3d(const float* img, float* out, const float* domain_w, const float* table, int rx, int ry, int rz, int n_samples,
                              float cutoff, float scale, const int* apply, int N, int C, int D, int H, int W, void* stream) {
    if (!img || !out || !domain_w || !table || !apply || img == out) return DA_ERR_BADARG;
    if (N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || rx < 0 || ry < 0 || rz < 0 || n_samples < 1 || !(cutoff > 0.f) || !(scale > 0.f)) return DA_ERR_BADARG;
    if (rx > DA_BILATERAL_MAX_RADIUS || ry > DA_BILATERAL_MAX_RADIUS || rz > DA_BILATERAL_MAX_RADIUS || n_samples > DA_BILATERAL_MAX_SAMPLES) return DA_ERR_UNSUPPORTED;
    if ((long long)D * H * W > 0x7FFFFFFFLL || (long long)N * C > 65535) return DA_ERR_UNSUPPORTED;
    BilGeom g;
    g.C = C; g.D = D; g.H = H; g.W = W; g.rx = rx; g.ry = ry; g.rz = rz; g.S = n_samples;
    g.ntx = (int)da_cdiv(W, TW); g.nty = (int)da_cdiv(H, TH); g.ntz = (int)da_cdiv(D, TD);
    g.cutoff = cutoff; g.scale = scale;
    const long long tiles = (long long)g.ntx * g.nty * g.ntz;
    if (tiles > 0x7FFFFFFFLL) return DA_ERR_UNSUPPORTED;
    const size_t lds = ((size_t)(TD + 2 * rz) * (TH + 2 * ry) * (TW + 2 * rx) + n_samples + (size_t)(2 * rx + 1) * (2 * ry + 1) * (2 * rz + 1)) * sizeof(float);
    static_assert(((TD + 2 * DA_BILATERAL_MAX_RADIUS) * (TH + 2 * DA_BILATERAL_MAX_RADIUS) * (TW + 2 * DA_BILATERAL_MAX_RADIUS) + DA_BILATERAL_MAX_SAMPLES
                   + (2 * DA_BILATERAL_MAX_RADIUS + 1) * (2 * DA_BILATERAL_MAX_RADIUS + 1) * (2 * DA_BILATERAL_MAX_RADIUS + 1)) * 4 <= 64 * 1024,
                  "the largest tile, table and weights fit the default 64 KiB of dynamic LDS");
    hipLaunchKernelGGL(bilateral_kernel, dim3((unsigned)tiles, (unsigned)(N * C)), dim3(kBlock), lds, da_stream(stream), img, out, domain_w, table, apply, g);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_intensity_augment(const float* img, float* out, const float* params, const float* bias_coef, int order, int gx, int gy, int gz,
                                    int sample0, int N, int C, int D, int H, int W, void* stream) {
    if (!img || !out || !params || img == out) return DA_ERR_BADARG;
    if (N <= 0 || N > 65535 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || sample0 < 0 || order < 0 || order > 3) return DA_ERR_BADARG;
    if (order > 0 && (!bias_coef || D < 2 || H < 2 || W < 2 || gx < order + 1 || gy < order + 1 || gz < order + 1)) return DA_ERR_BADARG;
    if ((long long)D * H * W > 0x7FFFFFFFLL) return DA_ERR_UNSUPPORTED;
    if (order > 0 && (long long)gx * gy * gz > DA_AUG_MAX_GRID_POINTS) return DA_ERR_UNSUPPORTED;
    if (order > 0 && ((long long)W * (gx - order) > 0x7FFFFFFFLL || (long long)H * (gy - order) > 0x7FFFFFFFLL
                      || (long long)D * (gz - order) > 0x7FFFFFFFLL)) return DA_ERR_UNSUPPORTED;   // i M in 32 bits
    PwGeom g;
    g.C = C; g.D = D; g.H = H; g.W = W;
    g.gx = gx; g.gy = gy; g.gz = gz;
    g.Mx = gx - order; g.My = gy - order; g.Mz = gz - order;
    g.sample0 = sample0;
    hipStream_t st = da_stream(stream);
    switch (order) {
        case 0: return launch_intensity<0>(img, out, params, bias_coef, g, N, st);
        case 1: return launch_intensity<1>(img, out, params, bias_coef, g, N, st);
        case 2: return launch_intensity<2>(img, out, params, bias_coef, g, N, st);
        default: return launch_intensity<3>(img, out, params, bias_coef, g, N, st);
    }
}
