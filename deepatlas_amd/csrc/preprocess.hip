// Device preprocessing of raw volumes (include/deepatlas_hip.h, "Volume preprocessing"): the SimpleITK half of lib/transforms.py -- Resample to a
// voxel size (:9-57), Normalization (:59-68), LeftToRight (:269-284), SegmentationLabelFilter (:692-706) -- and the project's percentile rescale,
// as kernels on the raw [C][D][H][W] array a loader uploads once.
//
// Every kernel here: 256-thread workgroups, lanes consecutive along W (the linear index), no workgroup waits for another; what one launch reads
// from another goes through stream order (separate launches).  Reductions accumulate in double in a fixed order (thread -> workgroup -> one
// finishing launch) with a grid that depends on the element count alone; the only atomics are integer adds.  Results are bit-identical from run to
// run.
#include "common.h"

#include <math.h>
#include <string.h>

namespace {

constexpr int PP_BLOCK = 256;
constexpr int PP_MAX_PARTS = 1024;          // workgroups of the reduction passes
constexpr int PP_HIST_GROUPS = 512;         // workgroups of the histogram passes
constexpr int PP_BINS = 2048;               // 11-bit digits (the last digit has 10 bits)
constexpr int PP_MAX_RANKS = 4;             // two percentiles, two neighbouring order statistics each

__device__ __forceinline__ double pp_load_f64(const void* src, int dtype, long long i) {
    return dtype == 1 ? ((const double*)src)[i] : (double)da_load_as_f32(src, dtype, i);
}

// ---- 3a. axis-aligned resample ---------------------------------------------------------------------------------------------------
// tab: int32 [Do + Ho + Wo][3] (D entries, then H, then W): lower tap, upper tap, bits of the float32 fraction; lower tap -1 = outside.
template <typename T>
__global__ void resample_nearest_kernel(const T* __restrict__ src, T* __restrict__ dst, const int* __restrict__ tab, int C, int D, int H, int W,
                                        int Do, int Ho, int Wo, T fill) {
    const long long total = (long long)C * Do * Ho * Wo;
    const int* td = tab; const int* th = tab + 3 * Do; const int* tw = tab + 3 * (Do + Ho);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int c, d, h, w;
        da_vox4(i, Do, Ho, Wo, c, d, h, w);
        const int sd = td[3 * d], sh = th[3 * h], sw = tw[3 * w];
        T v = fill;
        if ((sd | sh | sw) >= 0) v = src[(((long long)c * D + sd) * H + sh) * W + sw];
        dst[i] = v;
    }
}

__global__ void resample_linear_kernel(const void* __restrict__ src, int dtype, float* __restrict__ dst, const int* __restrict__ tab, int C, int D,
                                       int H, int W, int Do, int Ho, int Wo, float fill) {
    const long long total = (long long)C * Do * Ho * Wo;
    const int* td = tab; const int* th = tab + 3 * Do; const int* tw = tab + 3 * (Do + Ho);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int c, d, h, w;
        da_vox4(i, Do, Ho, Wo, c, d, h, w);
        const int d0 = td[3 * d], d1 = td[3 * d + 1], h0 = th[3 * h], h1 = th[3 * h + 1], w0 = tw[3 * w], w1 = tw[3 * w + 1];
        float v = fill;
        if ((d0 | h0 | w0) >= 0) {
            const float fd = __int_as_float(td[3 * d + 2]), fh = __int_as_float(th[3 * h + 2]), fw = __int_as_float(tw[3 * w + 2]);
            const long long base = (long long)c * D;
            const long long r00 = ((base + d0) * H + h0) * W, r01 = ((base + d0) * H + h1) * W;
            const long long r10 = ((base + d1) * H + h0) * W, r11 = ((base + d1) * H + h1) * W;
            float a, b;
            a = da_load_as_f32(src, dtype, r00 + w0); b = da_load_as_f32(src, dtype, r00 + w1); const float x00 = fmaf(fw, b - a, a);
            a = da_load_as_f32(src, dtype, r01 + w0); b = da_load_as_f32(src, dtype, r01 + w1); const float x01 = fmaf(fw, b - a, a);
            a = da_load_as_f32(src, dtype, r10 + w0); b = da_load_as_f32(src, dtype, r10 + w1); const float x10 = fmaf(fw, b - a, a);
            a = da_load_as_f32(src, dtype, r11 + w0); b = da_load_as_f32(src, dtype, r11 + w1); const float x11 = fmaf(fw, b - a, a);
            const float y0 = fmaf(fh, x01 - x00, x00), y1 = fmaf(fh, x11 - x10, x10);
            v = fmaf(fd, y1 - y0, y0);
        }
        dst[i] = v;
    }
}

// ---- 3b. moments -------------------------------------------------------------------------------------------------------------------
// fixed-order tree over the workgroup's 256 per-thread values (LDS, halving strides); result in thread 0
__device__ __forceinline__ double pp_block_tree(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = PP_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// pass 1: part[2 b] = number of finite voxels, part[2 b + 1] = their sum
__global__ void moments_sum_kernel(const void* __restrict__ src, int dtype, long long n, double* __restrict__ part) {
    __shared__ double sh[PP_BLOCK];
    double cnt = 0.0, sum = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const double x = pp_load_f64(src, dtype, i);
        if (isfinite(x)) { cnt += 1.0; sum += x; }
    }
    cnt = pp_block_tree(cnt, sh);
    sum = pp_block_tree(sum, sh);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = cnt; part[2 * blockIdx.x + 1] = sum; }
}
// one workgroup: out[0] = count, out[1] = mean (0 for an empty set)
__global__ void moments_mean_kernel(const double* __restrict__ part, int nparts, double* __restrict__ out) {
    __shared__ double sh[PP_BLOCK];
    double cnt = 0.0, sum = 0.0;
    for (int b = threadIdx.x; b < nparts; b += PP_BLOCK) { cnt += part[2 * b]; sum += part[2 * b + 1]; }
    cnt = pp_block_tree(cnt, sh);
    sum = pp_block_tree(sum, sh);
    if (threadIdx.x == 0) { out[0] = cnt; out[1] = cnt > 0.0 ? sum / cnt : 0.0; }
}
// pass 2: part[b] = sum over the finite voxels of (x - mean)^2
__global__ void moments_dev_kernel(const void* __restrict__ src, int dtype, long long n, const double* __restrict__ stats, double* __restrict__ part) {
    __shared__ double sh[PP_BLOCK];
    const double mean = stats[1];
    double m2 = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const double x = pp_load_f64(src, dtype, i);
        if (isfinite(x)) { const double e = x - mean; m2 += e * e; }
    }
    m2 = pp_block_tree(m2, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = m2;
}
// one workgroup: out[2] = unbiased variance (0 when fewer than two finite voxels)
__global__ void moments_var_kernel(const double* __restrict__ part, int nparts, double* __restrict__ out) {
    __shared__ double sh[PP_BLOCK];
    double m2 = 0.0;
    for (int b = threadIdx.x; b < nparts; b += PP_BLOCK) m2 += part[b];
    m2 = pp_block_tree(m2, sh);
    if (threadIdx.x == 0) out[2] = out[0] > 1.0 ? m2 / (out[0] - 1.0) : 0.0;
}

// ---- 3c. percentiles: three-digit radix select on monotone keys -------------------------------------------------------------------
struct SelectState {
    unsigned n_valid, n_nan;
    unsigned rank[PP_MAX_RANKS];      // rank still to be found among the keys that share prefix[r]
    unsigned prefix[PP_MAX_RANKS];    // the digits chosen so far
    double frac[2];
};

__device__ __forceinline__ unsigned pp_key(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pp_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// shift / bits of digit `pass`: 11 + 11 + 10 bits from the top
__host__ __device__ inline int pp_digit_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__host__ __device__ inline int pp_digit_bits(int pass) { return pass == 2 ? 10 : 11; }

// histogram of digit `pass` of the keys matching each rank's prefix (pass 0: one histogram of every key, and the NaN count)
__global__ void select_hist_kernel(const void* __restrict__ src, int dtype, long long n, int pass, int nranks, const SelectState* __restrict__ st,
                                   unsigned* __restrict__ hist, unsigned* __restrict__ nan_count) {
    __shared__ unsigned lh[PP_MAX_RANKS * PP_BINS];
    __shared__ unsigned lnan;
    const int nh = pass == 0 ? 1 : nranks;
    for (int k = threadIdx.x; k < nh * PP_BINS; k += PP_BLOCK) lh[k] = 0u;
    if (threadIdx.x == 0) lnan = 0u;
    __syncthreads();
    const int shift = pp_digit_shift(pass), bits = pp_digit_bits(pass);
    const unsigned mask = (1u << bits) - 1u;
    unsigned pre[PP_MAX_RANKS];
    for (int r = 0; r < PP_MAX_RANKS; ++r) pre[r] = (pass > 0 && r < nranks) ? st->prefix[r] : 0u;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float x = da_load_as_f32(src, dtype, i);
        if (x != x) { if (pass == 0) atomicAdd(&lnan, 1u); continue; }
        const unsigned key = pp_key(x);
        const unsigned digit = (key >> shift) & mask;
        if (pass == 0) { atomicAdd(&lh[digit], 1u); continue; }
        const unsigned upper = key >> (shift + bits);
#pragma unroll
        for (int r = 0; r < PP_MAX_RANKS; ++r)
            if (r < nranks && upper == pre[r]) atomicAdd(&lh[r * PP_BINS + digit], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nh * PP_BINS; k += PP_BLOCK) { const unsigned v = lh[k]; if (v) atomicAdd(&hist[k], v); }
    if (pass == 0 && threadIdx.x == 0 && lnan) atomicAdd(nan_count, lnan);
}

// one workgroup: pick digit `pass` of every rank, clear the histograms for the next pass; after the last digit write the results.
// out: [p0, p1, order statistic 0..3, number of non-NaN values, number of NaNs], all double.
__global__ void select_pick_kernel(int pass, int npct, double p0, double p1, SelectState* __restrict__ st, unsigned* __restrict__ hist,
                                   const unsigned* __restrict__ nan_count, double* __restrict__ out) {
    __shared__ unsigned total;
    const int nranks = 2 * npct;
    if (pass == 0) {
        if (threadIdx.x == 0) {
            unsigned t = 0u;
            for (int b = 0; b < PP_BINS; ++b) t += hist[b];
            total = t;
            st->n_valid = t; st->n_nan = *nan_count;
            for (int j = 0; j < npct; ++j) {
                const double p = j == 0 ? p0 : p1;
                const double rk = t > 0u ? p / 100.0 * (double)(t - 1u) : 0.0;
                double lo = floor(rk);
                if (t > 0u && lo > (double)(t - 1u)) lo = (double)(t - 1u);
                const unsigned ilo = (unsigned)lo, ihi = (t > 0u && ilo + 1u < t) ? ilo + 1u : ilo;
                st->rank[2 * j] = ilo; st->rank[2 * j + 1] = ihi; st->frac[j] = rk - lo;
                st->prefix[2 * j] = 0u; st->prefix[2 * j + 1] = 0u;
            }
        }
        __syncthreads();
    } else {
        if (threadIdx.x == 0) total = st->n_valid;
        __syncthreads();
    }
    const int bits = pp_digit_bits(pass), nbins = 1 << bits;
    if ((int)threadIdx.x < nranks && total > 0u) {
        const int r = threadIdx.x;
        const unsigned* h = hist + (pass == 0 ? 0 : r * PP_BINS);
        unsigned rank = st->rank[r], cum = 0u;
        int b = 0;
        for (; b < nbins - 1; ++b) {
            const unsigned c = h[b];
            if (rank < cum + c) break;
            cum += c;
        }
        st->rank[r] = rank - cum;
        st->prefix[r] = (st->prefix[r] << bits) | (unsigned)b;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < PP_MAX_RANKS * PP_BINS; k += PP_BLOCK) hist[k] = 0u;
    if (pass == 2 && threadIdx.x == 0) {
        const double nanv = __longlong_as_double(0x7FF8000000000000LL);
        double os[PP_MAX_RANKS];
        for (int r = 0; r < PP_MAX_RANKS; ++r) os[r] = (r < nranks && total > 0u) ? (double)pp_unkey(st->prefix[r]) : nanv;
        for (int j = 0; j < 2; ++j) {
            double v = nanv;
            if (j < npct && total > 0u) {
                const double a = os[2 * j], b = os[2 * j + 1], t = st->frac[j];
                v = (a == b || t == 0.0) ? a : a + (b - a) * t;      // (t == 0: the order statistic itself, also when it is infinite)
            }
            out[j] = v;
        }
        for (int r = 0; r < PP_MAX_RANKS; ++r) out[2 + r] = os[r];
        out[6] = (double)st->n_valid; out[7] = (double)st->n_nan;
    }
}

// ---- 3d / 3e ------------------------------------------------------------------------------------------------------------------------
__global__ void affine_intensity_kernel(const void* __restrict__ src, int dtype, float* __restrict__ dst, long long n, float a, float b, int clamp01) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float y = 0.f;
        if (b != 0.f) {
            const float x = da_load_as_f32(src, dtype, i);
            y = (x - a) / b;
            if (clamp01) { y = y > 1.f ? 1.f : y; y = y < 0.f ? 0.f : y; }
        }
        dst[i] = y;
    }
}

template <typename T>
__global__ void label_lut_kernel(const T* __restrict__ src, T* __restrict__ dst, long long n, const int* __restrict__ lut, int nlut) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long l = (long long)src[i];
        dst[i] = (l >= 0 && l < nlut) ? (T)lut[l] : (T)0;
    }
}

constexpr long long PP_MAX_V = 1LL << 31;
inline int pp_parts(long long n) { return (int)(da_cdiv(n, PP_BLOCK) < PP_MAX_PARTS ? da_cdiv(n, PP_BLOCK) : PP_MAX_PARTS); }
// the selection's state, its histograms and the NaN counter in a 256-byte slot of its own; zeroed together
struct SelectWs { SelectState* state; unsigned *hist, *nan_count; size_t bytes; };
inline SelectWs pp_select_layout(void* ws) { DaCarve c(ws); return SelectWs{c.take<SelectState>(1), c.take<unsigned>((size_t)PP_MAX_RANKS * PP_BINS), c.take<unsigned>(1), c.off}; }

}  // namespace

extern "C" int da_resample_axes(const void* src, int src_dtype, void* dst, int interpolator, int C, int D, int H, int W, int Do, int Ho, int Wo,
                                const int* tables, double default_value, void* stream) {
    if (!src || !dst || !tables || src_dtype < 0 || src_dtype > 4 || (interpolator != 0 && interpolator != 1)) return DA_ERR_BADARG;
    if (C <= 0 || D <= 0 || H <= 0 || W <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0) return DA_ERR_BADARG;
    const long long vin = (long long)C * D * H * W, total = (long long)C * Do * Ho * Wo;
    if (vin >= PP_MAX_V || total >= PP_MAX_V) return DA_ERR_UNSUPPORTED;
    const dim3 grid(da_grid(total, PP_BLOCK)), block(PP_BLOCK);
    hipStream_t st = da_stream(stream);
    if (interpolator == 0) {
        hipLaunchKernelGGL(resample_linear_kernel, grid, block, 0, st, src, src_dtype, (float*)dst, tables, C, D, H, W, Do, Ho, Wo, (float)default_value);
    } else if (src_dtype == 0) {
        const float f = (float)default_value; unsigned bitsv; memcpy(&bitsv, &f, 4);
        hipLaunchKernelGGL((resample_nearest_kernel<unsigned>), grid, block, 0, st, (const unsigned*)src, (unsigned*)dst, tables, C, D, H, W, Do, Ho, Wo, bitsv);
    } else if (src_dtype == 1) {
        unsigned long long bitsv; memcpy(&bitsv, &default_value, 8);
        hipLaunchKernelGGL((resample_nearest_kernel<unsigned long long>), grid, block, 0, st, (const unsigned long long*)src, (unsigned long long*)dst, tables, C, D, H, W, Do, Ho, Wo, bitsv);
    } else if (src_dtype == 2) {
        hipLaunchKernelGGL((resample_nearest_kernel<short>), grid, block, 0, st, (const short*)src, (short*)dst, tables, C, D, H, W, Do, Ho, Wo, (short)default_value);
    } else if (src_dtype == 3) {
        hipLaunchKernelGGL((resample_nearest_kernel<unsigned char>), grid, block, 0, st, (const unsigned char*)src, (unsigned char*)dst, tables, C, D, H, W, Do, Ho, Wo, (unsigned char)default_value);
    } else {
        hipLaunchKernelGGL((resample_nearest_kernel<int>), grid, block, 0, st, (const int*)src, (int*)dst, tables, C, D, H, W, Do, Ho, Wo, (int)default_value);
    }
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t da_volume_moments_ws_bytes(long long n) {
    if (n <= 0 || n >= PP_MAX_V) return 0;
    return da_align(sizeof(double) * 2 * PP_MAX_PARTS);
}

extern "C" int da_volume_moments(const void* src, int src_dtype, long long n, double* out3, void* ws, size_t ws_bytes, void* stream) {
    if (!src || !out3 || !ws || src_dtype < 0 || src_dtype > 4 || n <= 0) return DA_ERR_BADARG;
    if (n >= PP_MAX_V) return DA_ERR_UNSUPPORTED;
    if (ws_bytes < da_volume_moments_ws_bytes(n)) return DA_ERR_WS_SMALL;
    hipStream_t st = da_stream(stream);
    double* part = (double*)ws;
    const int nparts = pp_parts(n);
    hipLaunchKernelGGL(moments_sum_kernel, dim3(nparts), dim3(PP_BLOCK), 0, st, src, src_dtype, n, part);
    hipLaunchKernelGGL(moments_mean_kernel, dim3(1), dim3(PP_BLOCK), 0, st, (const double*)part, nparts, out3);
    hipLaunchKernelGGL(moments_dev_kernel, dim3(nparts), dim3(PP_BLOCK), 0, st, src, src_dtype, n, (const double*)out3, part);
    hipLaunchKernelGGL(moments_var_kernel, dim3(1), dim3(PP_BLOCK), 0, st, (const double*)part, nparts, out3);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t da_volume_percentiles_ws_bytes(long long n) {
    if (n <= 0 || n >= PP_MAX_V) return 0;
    return pp_select_layout(nullptr).bytes;
}

extern "C" int da_volume_percentiles(const void* src, int src_dtype, long long n, const double* percentiles, int n_percentiles, double* out8,
                                     void* ws, size_t ws_bytes, void* stream) {
    if (!src || !out8 || !ws || !percentiles || src_dtype < 0 || src_dtype > 4 || n <= 0 || n_percentiles < 1 || n_percentiles > 2) return DA_ERR_BADARG;
    for (int j = 0; j < n_percentiles; ++j)
        if (!(percentiles[j] >= 0.0 && percentiles[j] <= 100.0)) return DA_ERR_BADARG;
    if (n >= PP_MAX_V) return DA_ERR_UNSUPPORTED;
    if (ws_bytes < da_volume_percentiles_ws_bytes(n)) return DA_ERR_WS_SMALL;
    hipStream_t st = da_stream(stream);
    const auto [state, hist, nan_count, bytes] = pp_select_layout(ws);
    hipError_t e = hipMemsetAsync(ws, 0, bytes, st);
    if (e != hipSuccess) return (int)e;
    const long long per_group = (long long)PP_BLOCK * 16;
    const int groups = (int)(da_cdiv(n, per_group) < PP_HIST_GROUPS ? da_cdiv(n, per_group) : PP_HIST_GROUPS);
    const double p0 = percentiles[0], p1 = n_percentiles > 1 ? percentiles[1] : percentiles[0];
    for (int pass = 0; pass < 3; ++pass) {
        hipLaunchKernelGGL(select_hist_kernel, dim3(groups), dim3(PP_BLOCK), 0, st, src, src_dtype, n, pass, 2 * n_percentiles, (const SelectState*)state, hist, nan_count);
        hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(PP_BLOCK), 0, st, pass, n_percentiles, p0, p1, state, hist, (const unsigned*)nan_count, out8);
    }
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_affine_intensity_to_f32(const void* src, int src_dtype, float* dst, long long n, float a, float b, int clamp01, void* stream) {
    if (!src || !dst || src_dtype < 0 || src_dtype > 4 || n <= 0 || (clamp01 != 0 && clamp01 != 1)) return DA_ERR_BADARG;
    if (n >= PP_MAX_V) return DA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(affine_intensity_kernel, dim3(da_grid(n, PP_BLOCK)), dim3(PP_BLOCK), 0, da_stream(stream), src, src_dtype, dst, n, a, b, clamp01);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_label_lut(const void* src, int src_dtype, void* dst, long long n, const int* lut, int n_lut, void* stream) {
    if (!src || !dst || !lut || (src_dtype != 3 && src_dtype != 4) || n <= 0 || n_lut < 1 || n_lut > 65536) return DA_ERR_BADARG;
    if (n >= PP_MAX_V) return DA_ERR_UNSUPPORTED;
    const dim3 grid(da_grid(n, PP_BLOCK)), block(PP_BLOCK);
    if (src_dtype == 3) hipLaunchKernelGGL((label_lut_kernel<unsigned char>), grid, block, 0, da_stream(stream), (const unsigned char*)src, (unsigned char*)dst, n, lut, n_lut);
    else hipLaunchKernelGGL((label_lut_kernel<int>), grid, block, 0, da_stream(stream), (const int*)src, (int*)dst, n, lut, n_lut);
    DA_LAUNCH_CHECK();
    return 0;
}
