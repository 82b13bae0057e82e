// Patch sampling on the device (include/deepatlas_hip.h, "Random crops"): lib/transforms.py:322-505 -- RandomCrop, BalancedRandomCrop and
// random_3d_coordinates.  The reference draws a start, counts one class inside the crop and repeats until the share passes a threshold; here
// the class count of EVERY crop window is a separable sliding-window sum, the admissible starts are those whose count passes, and a draw is
// the k-th admissible start in raster order, k from the project's counter hash: the distribution the rejection loop converges to, in a
// bounded number of launches and without a host round trip.
//
//   row pass    one wave per row of W labels: ballots of (label == cls) into an LDS bit row, a wave prefix sum over the words' popcounts,
//               then count(x) = rank(x + ww) - rank(x), uint16 (ww <= 32768)
//   H pass      running sums with lanes along x (coalesced), int32
//   D pass      the same along z; the counts op writes them, the sampler compares them with min_count and emits one bit per start
//               (wave ballot = one 64-bit word) and the largest count with its first raster index (integer atomic max on a packed
//               64-bit key); one small launch then counts the admissible starts of each z plane by popcount
//   pick        one workgroup per (sample, draw): plane by the per-plane counts, word by popcounts, bit inside the word
//   gather      image and labels of every (sample, draw) in one launch, 16-byte loads along W where the source is aligned
//
// 256-thread workgroups, no workgroup waits for another, what one launch reads from another goes through stream order; the only atomics are
// integer maxima, so results are bit-identical from run to run.
#include "common.h"
#include "counter_hash.h"

namespace {

constexpr int CR_BLOCK = 256;
constexpr int CR_WAVES = CR_BLOCK / DA_WAVE;
constexpr int CR_MAX_W = 32768;                      // a row's bits live in LDS; a row count fits uint16
constexpr int CR_MAX_WORDS = CR_MAX_W / 64;
constexpr long long CR_MAX_V = 1LL << 31;
constexpr int CR_MAX_DRAWS = 65536;

typedef unsigned long long u64;

__device__ __forceinline__ unsigned cr_rank(const u64* bits, const unsigned* pre, int p) {
    const int w = p >> 6, b = p & 63;
    return pre[w] + (unsigned)__popcll(bits[w] & ((1ull << b) - 1ull));
}

// ---- row pass: out[r][x] = #{label == cls} in lab[r][x .. x + ww), x < Wd -------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(CR_BLOCK) crop_row_kernel(const T* __restrict__ lab, unsigned short* __restrict__ out, long long rows,
                                                            int W, int ww, int Wd, long long cls) {
    __shared__ u64 s_bits[CR_WAVES][CR_MAX_WORDS + 1];
    __shared__ unsigned s_pre[CR_WAVES][CR_MAX_WORDS + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nwords = (W + 63) >> 6;
    const int per = (nwords + 1 + 63) / 64;                      // words of the prefix sum each lane owns (contiguous)
    const long long trips = da_cdiv(rows, CR_WAVES);
    u64* bits = s_bits[wv];
    unsigned* pre = s_pre[wv];
    for (long long it = blockIdx.x; it < trips; it += gridDim.x) {            // (the trip count is uniform over the workgroup)
        const long long r = it * CR_WAVES + wv;
        const bool live = r < rows;
        const T* src = lab + (live ? r : 0) * (long long)W;
        for (int w = 0; w < nwords; ++w) {
            const int x = w * 64 + lane;
            const bool hit = live && x < W && (long long)src[x] == cls;
            const u64 m = __ballot(hit);
            if (lane == 0) bits[w] = m;
        }
        if (lane == 0) bits[nwords] = 0ull;
        __syncthreads();
        unsigned local = 0u;
        for (int j = 0; j < per; ++j) {
            const int w = lane * per + j;
            if (w <= nwords) local += (unsigned)__popcll(bits[w]);
        }
        unsigned incl = local;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        unsigned run = incl - local;
        for (int j = 0; j < per; ++j) {
            const int w = lane * per + j;
            if (w <= nwords) { pre[w] = run; run += (unsigned)__popcll(bits[w]); }
        }
        __syncthreads();
        if (live) {
            unsigned short* dst = out + r * (long long)Wd;
            for (int x = lane; x < Wd; x += 64) dst[x] = (unsigned short)(cr_rank(bits, pre, x + ww) - cr_rank(bits, pre, x));
        }
        __syncthreads();
    }
}

// ---- running sums along the middle axis of [outer][L][inner] -> [outer][Lo][inner], window w, Lo <= L - w + 1 ------------------------------
// grid: x over inner (lanes consecutive along it), y over segments of `seg` outputs, z strides over outer
template <typename TI>
__global__ void __launch_bounds__(CR_BLOCK) crop_slide_kernel(const TI* __restrict__ in, int* __restrict__ out, long long outer, int L, int w,
                                                              int Lo, long long inner, int seg) {
    const long long i = (long long)blockIdx.x * CR_BLOCK + threadIdx.x;
    if (i >= inner) return;
    const int l0 = blockIdx.y * seg, l1 = min(l0 + seg, Lo);
    if (l0 >= Lo) return;
    for (long long o = blockIdx.z; o < outer; o += gridDim.z) {
        const TI* p = in + o * L * inner + i;
        int* q = out + o * Lo * inner + i;
        int s = 0;
        for (int k = 0; k < w; ++k) s += (int)p[(long long)(l0 + k) * inner];
        q[(long long)l0 * inner] = s;
        for (int l = l0 + 1; l < l1; ++l) {
            s += (int)p[(long long)(l + w - 1) * inner] - (int)p[(long long)(l - 1) * inner];
            q[(long long)l * inner] = s;
        }
    }
}

// ---- the sampler's D pass: one bit per start of the domain, the largest count and its first raster index ------------------------------------
// hs [N][D][inner] (inner = Hd Wd); mask [N][Dd][nW] 64-bit words, bit i & 63 of word i >> 6 of plane z = start (z, i);
// best [N]: (count << 32) | (0xFFFFFFFF - raster index).  grid: x over inner, y over z segments, z = sample.
__global__ void __launch_bounds__(CR_BLOCK) crop_select_kernel(const int* __restrict__ hs, u64* __restrict__ mask, u64* __restrict__ best, int D, int wd,
                                                               int Dd, long long inner, int nW, int seg, int min_count) {
    const int n = blockIdx.z, lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * CR_BLOCK + threadIdx.x;
    const bool live = i < inner;
    const long long word = i >> 6;
    const int l0 = blockIdx.y * seg, l1 = min(l0 + seg, Dd);
    if (l0 >= Dd) return;
    const int* p = hs + (long long)n * D * inner + (live ? i : 0);
    int s = 0;
    if (live)
        for (int k = 0; k < wd; ++k) s += p[(long long)(l0 + k) * inner];
    u64 key = 0ull;
    for (int l = l0; l < l1; ++l) {
        if (live && l > l0) s += p[(long long)(l + wd - 1) * inner] - p[(long long)(l - 1) * inner];
        const u64 m = __ballot(live && s >= min_count);
        if (live) {
            const u64 k = ((u64)(unsigned)s << 32) | (u64)(0xFFFFFFFFu - (unsigned)((long long)l * inner + i));
            key = k > key ? k : key;
        }
        if (lane == 0 && word < nW) mask[((long long)n * Dd + l) * nW + word] = m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = __shfl_xor((unsigned)(key >> 32), o), lo = __shfl_xor((unsigned)key, o);
        const u64 other = ((u64)hi << 32) | lo;
        key = other > key ? other : key;
    }
    if (lane == 0 && key) atomicMax(&best[n], key);
}

// admissible starts of every z plane: one workgroup per (plane, sample) adds the popcounts of the plane's words in a fixed order
__global__ void __launch_bounds__(CR_BLOCK) crop_plane_count_kernel(const u64* __restrict__ mask, unsigned* __restrict__ zcount, int Dd, int nW) {
    __shared__ unsigned s_part[CR_BLOCK];
    const int z = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const u64* words = mask + ((long long)n * Dd + z) * nW;
    unsigned c = 0u;
    for (int w = tid; w < nW; w += CR_BLOCK) c += (unsigned)__popcll(words[w]);
    s_part[tid] = c;
    __syncthreads();
    for (int s = CR_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) s_part[tid] += s_part[tid + s];
        __syncthreads();
    }
    if (tid == 0) zcount[(long long)n * Dd + z] = s_part[0];
}

__device__ __forceinline__ u64 cr_pick_k(unsigned seed, int sample0, int n, int p, u64 count) {
    const unsigned bits = da_synth_bits(seed, (u64)(long long)(sample0 + n) * 65536ull + (u64)p, DA_CROP_STREAM);
    return ((u64)bits * count) >> 32;
}

// unconditioned draws: uniform over the domain.  One thread per (sample, draw).
__global__ void crop_pick_uniform_kernel(const int* __restrict__ draw_cond, int N, int P, int Dd, int Hd, int Wd, unsigned seed, int sample0,
                                         int* __restrict__ starts, int* __restrict__ info) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)N * P) return;
    const int n = (int)(t / P), p = (int)(t % P);
    if (draw_cond[p] >= 0) return;
    const u64 dom = (u64)Dd * Hd * Wd;
    const u64 k = cr_pick_k(seed, sample0, n, p, dom);
    int z, y, x;
    da_vox3((long long)k, Hd, Wd, z, y, x);
    starts[3 * t] = z; starts[3 * t + 1] = y; starts[3 * t + 2] = x;
    info[2 * t] = (int)dom; info[2 * t + 1] = -1;
}

// conditioned draws of condition q: one workgroup per (draw, sample)
__global__ void __launch_bounds__(CR_BLOCK) crop_pick_kernel(const int* __restrict__ draw_cond, int q, const int* __restrict__ hs,
                                                             const u64* __restrict__ mask, const unsigned* __restrict__ zcount,
                                                             const u64* __restrict__ best, int P, int D, int wd, int Dd, int Hd, int Wd, int nW,
                                                             unsigned seed, int sample0, int* __restrict__ starts, int* __restrict__ info) {
    const int p = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    if (draw_cond[p] != q) return;
    __shared__ unsigned s_part[CR_BLOCK];
    __shared__ unsigned s_total, s_krem;
    __shared__ int s_z, s_found;
    const long long inner = (long long)Hd * Wd;
    const unsigned* zc = zcount + (long long)n * Dd;
    unsigned part = 0u;
    for (int z = tid; z < Dd; z += CR_BLOCK) part += zc[z];
    s_part[tid] = part;
    __syncthreads();
    if (tid == 0) {
        unsigned t = 0u;
        for (int k = 0; k < CR_BLOCK; ++k) t += s_part[k];
        s_total = t;
    }
    __syncthreads();
    const unsigned total = s_total;
    const long long t = (long long)n * P + p;
    long long idx = -1;                                          // raster index of the chosen start (set by one thread)
    if (total == 0u) {                                           // no admissible start: the largest count, first in raster order
        if (tid == 0) idx = (long long)(0xFFFFFFFFu - (unsigned)best[n]);
    } else {
        if (tid == 0) { s_krem = (unsigned)cr_pick_k(seed, sample0, n, p, (u64)total); s_found = 0; s_z = Dd - 1; }
        for (int base = 0; base < Dd; base += CR_BLOCK) {        // the plane of k: 256 plane counts at a time through LDS
            __syncthreads();
            s_part[tid] = base + tid < Dd ? zc[base + tid] : 0u;
            __syncthreads();
            if (tid == 0 && !s_found) {
                unsigned k = s_krem;
                for (int j = 0; j < CR_BLOCK && base + j < Dd; ++j) {
                    if (k < s_part[j]) { s_z = base + j; s_found = 1; break; }
                    k -= s_part[j];
                }
                s_krem = k;
            }
        }
        __syncthreads();
        const int z = s_z;
        const unsigned krem = s_krem;
        const u64* words = mask + ((long long)n * Dd + z) * nW;
        const int per = (int)da_cdiv(nW, CR_BLOCK);
        const int w0 = tid * per, w1 = min(w0 + per, nW);
        unsigned mine = 0u;
        for (int w = w0; w < w1; ++w) mine += (unsigned)__popcll(words[w]);
        __syncthreads();
        s_part[tid] = mine;
        __syncthreads();
        unsigned before = 0u;
        for (int k = 0; k < tid; ++k) before += s_part[k];
        if (krem >= before && krem < before + mine) {            // exactly one thread
            unsigned r = krem - before;
            for (int w = w0; w < w1; ++w) {
                u64 m = words[w];
                const unsigned c = (unsigned)__popcll(m);
                if (r >= c) { r -= c; continue; }
                for (unsigned j = 0; j < r; ++j) m &= m - 1ull;  // drop the r lowest set bits
                idx = (long long)z * inner + (long long)w * 64 + (__ffsll((long long)m) - 1);
                break;
            }
        }
    }
    if (idx >= 0) {
        int z, y, x;
        da_vox3(idx, Hd, Wd, z, y, x);
        const int* col = hs + ((long long)n * D + z) * inner + (long long)y * Wd + x;
        int cnt = 0;
        for (int k = 0; k < wd; ++k) cnt += col[(long long)k * inner];
        starts[3 * t] = z; starts[3 * t + 1] = y; starts[3 * t + 2] = x;
        info[2 * t] = (int)total; info[2 * t + 1] = cnt;
    }
}

// ---- gather ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cr_clamp_start(int s, int S, int w) { s = s < 0 ? 0 : s; return s > S - w ? S - w : s; }

// items: first the image's groups of VEC consecutive voxels along W, then the labels'.  VEC = 4 needs ww % 4 == 0 (aligned stores); a
// source group that is 16-byte aligned (4 bytes for 1-byte labels) is read with one load, any other with VEC scalar loads.
template <typename TL, int VEC>
__global__ void __launch_bounds__(CR_BLOCK) crop_gather_kernel(const float* __restrict__ img, float* __restrict__ img_out, int C,
                                                               const TL* __restrict__ lab, TL* __restrict__ lab_out, const int* __restrict__ starts,
                                                               long long NP, int P, int D, int H, int W, int wd, int wh, int ww) {
    const int gw = ww / VEC;
    const long long per_vol = (long long)wd * wh * gw;
    const long long n_img = img ? NP * C * per_vol : 0, n_lab = lab ? NP * per_vol : 0;
    for (long long it = (long long)blockIdx.x * CR_BLOCK + threadIdx.x; it < n_img + n_lab; it += (long long)gridDim.x * CR_BLOCK) {
        const bool is_img = it < n_img;
        long long r = is_img ? it : it - n_img;
        const int g = (int)(r % gw); r /= gw;
        const int y = (int)(r % wh); r /= wh;
        const int z = (int)(r % wd); r /= wd;
        int c = 0;
        if (is_img) { c = (int)(r % C); r /= C; }
        const long long np = r;
        const int n = (int)(np / P);
        const int z0 = cr_clamp_start(starts[3 * np], D, wd), y0 = cr_clamp_start(starts[3 * np + 1], H, wh),
                  x0 = cr_clamp_start(starts[3 * np + 2], W, ww);
        const long long plane = is_img ? (long long)n * C + c : (long long)n;
        const long long src = ((plane * D + z0 + z) * H + y0 + y) * W + x0 + (long long)g * VEC;
        const long long dst = (((is_img ? np * C + c : np) * wd + z) * wh + y) * ww + (long long)g * VEC;
        if (is_img) {
            if (VEC == 4) {
                float4 v;
                if ((reinterpret_cast<uintptr_t>(img + src) & 15) == 0) v = *reinterpret_cast<const float4*>(img + src);
                else v = make_float4(img[src], img[src + 1], img[src + 2], img[src + 3]);
                *reinterpret_cast<float4*>(img_out + dst) = v;
            } else {
                img_out[dst] = img[src];
            }
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) lab_out[dst + k] = lab[src + k];
        }
    }
}

inline int cr_label_code_ok(int code) { return code == 3 || code == 4 || code == 5; }

struct CrGeom {
    int wd, wh, ww, Dd, Hd, Wd;
};
// counts op: every start (S - w + 1 per axis); sampler: the domain (max(S - w, 1), or S - w + 1 with include_last)
inline bool cr_geom(int D, int H, int W, const int* win, int mode, CrGeom& g) {
    if (!win) return false;
    g.wd = win[0]; g.wh = win[1]; g.ww = win[2];
    if (g.wd < 1 || g.wh < 1 || g.ww < 1 || g.wd > D || g.wh > H || g.ww > W) return false;
    const bool all = mode != 0;
    g.Dd = all ? D - g.wd + 1 : (D - g.wd > 1 ? D - g.wd : 1);
    g.Hd = all ? H - g.wh + 1 : (H - g.wh > 1 ? H - g.wh : 1);
    g.Wd = all ? W - g.ww + 1 : (W - g.ww > 1 ? W - g.ww : 1);
    return true;
}

inline int cr_words(const CrGeom& g) { return (int)da_cdiv((long long)g.Hd * g.Wd, 64); }
// one class's row and H passes (all da_window_label_counts needs: counts_bytes), then the selection's candidate mask, per-plane counts and best keys
struct CrWs { unsigned short* rows; int* hs; size_t counts_bytes; u64* mask; unsigned* zcount; u64* best; size_t bytes; };
inline CrWs cr_layout(int N, int D, int H, const CrGeom& g, void* ws) {
    DaCarve c(ws); return CrWs{c.take<unsigned short>((size_t)N * D * H * g.Wd), c.take<int>((size_t)N * D * g.Hd * g.Wd), c.off,
                c.take<u64>((size_t)N * g.Dd * cr_words(g)), c.take<unsigned>((size_t)N * g.Dd), c.take<u64>((size_t)N), c.off};
}
inline int cr_seg(int w) { return w > 16 ? w : 16; }

// row pass + H pass of one class into rows / hs
int cr_class_passes(const void* labels, int code, int N, int D, int H, int W, const CrGeom& g, long long cls, unsigned short* rows, int* hs,
                    hipStream_t st) {
    const long long nrows = (long long)N * D * H;
    const dim3 rgrid(da_grid(da_cdiv(nrows, CR_WAVES), 1)), block(CR_BLOCK);
    if (code == 3) hipLaunchKernelGGL((crop_row_kernel<unsigned char>), rgrid, block, 0, st, (const unsigned char*)labels, rows, nrows, W, g.ww, g.Wd, cls);
    else if (code == 4) hipLaunchKernelGGL((crop_row_kernel<int>), rgrid, block, 0, st, (const int*)labels, rows, nrows, W, g.ww, g.Wd, cls);
    else hipLaunchKernelGGL((crop_row_kernel<long long>), rgrid, block, 0, st, (const long long*)labels, rows, nrows, W, g.ww, g.Wd, cls);
    DA_LAUNCH_CHECK();
    const int seg = cr_seg(g.wh);
    const long long outer = (long long)N * D;
    const dim3 hgrid((unsigned)da_cdiv(g.Wd, CR_BLOCK), (unsigned)da_cdiv(g.Hd, seg), (unsigned)(outer < 4096 ? outer : 4096));
    hipLaunchKernelGGL((crop_slide_kernel<unsigned short>), hgrid, block, 0, st, (const unsigned short*)rows, hs, outer, H, g.wh, g.Hd, (long long)g.Wd, seg);
    DA_LAUNCH_CHECK();
    return 0;
}

inline bool cr_dims_ok(int N, int D, int H, int W) { return N > 0 && N <= 65535 && D > 0 && H > 0 && W > 0; }

}  // namespace

extern "C" size_t da_window_label_counts_ws_bytes(int N, int D, int H, int W, const int* window3) {
    CrGeom g;
    if (!cr_dims_ok(N, D, H, W) || (long long)D * H * W >= CR_MAX_V || W > CR_MAX_W || !cr_geom(D, H, W, window3, 1, g)) return 0;
    return cr_layout(N, D, H, g, nullptr).counts_bytes;
}

extern "C" int da_window_label_counts(const void* labels, int label_dtype, int N, int D, int H, int W, const int* window3, long long cls,
                                      int* counts, void* ws, size_t ws_bytes, void* stream) {
    CrGeom g;
    if (!labels || !counts || !ws || !cr_label_code_ok(label_dtype) || !cr_dims_ok(N, D, H, W) || !cr_geom(D, H, W, window3, 1, g)) return DA_ERR_BADARG;
    if ((long long)D * H * W >= CR_MAX_V) return DA_ERR_BADARG;
    if (W > CR_MAX_W) return DA_ERR_UNSUPPORTED;
    if (ws_bytes < da_window_label_counts_ws_bytes(N, D, H, W, window3)) return DA_ERR_WS_SMALL;
    hipStream_t st = da_stream(stream);
    const CrWs l = cr_layout(N, D, H, g, ws);
    unsigned short* rows = l.rows; int* hs = l.hs;
    const int rc = cr_class_passes(labels, label_dtype, N, D, H, W, g, cls, rows, hs, st);
    if (rc) return rc;
    const long long inner = (long long)g.Hd * g.Wd;
    const int seg = cr_seg(g.wd);
    const dim3 grid((unsigned)da_cdiv(inner, CR_BLOCK), (unsigned)da_cdiv(g.Dd, seg), (unsigned)N);
    hipLaunchKernelGGL((crop_slide_kernel<int>), grid, dim3(CR_BLOCK), 0, st, (const int*)hs, counts, (long long)N, D, g.wd, g.Dd, inner, seg);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t da_crop_sample_starts_ws_bytes(int N, int D, int H, int W, const int* window3, int include_last) {
    CrGeom g;
    if (!cr_dims_ok(N, D, H, W) || (long long)D * H * W >= CR_MAX_V || W > CR_MAX_W || !cr_geom(D, H, W, window3, include_last ? 1 : 0, g)) return 0;
    return cr_layout(N, D, H, g, nullptr).bytes;
}

extern "C" int da_crop_sample_starts(const void* labels, int label_dtype, int N, int D, int H, int W, const int* window3, int include_last,
                                     int P, const int* conds, int n_conds, const int* draw_cond, unsigned int seed, int sample0,
                                     int* starts, int* info, void* ws, size_t ws_bytes, void* stream) {
    CrGeom g;
    if (!labels || !starts || !info || !draw_cond || !cr_label_code_ok(label_dtype) || !cr_dims_ok(N, D, H, W)) return DA_ERR_BADARG;
    if (!cr_geom(D, H, W, window3, include_last ? 1 : 0, g) || P < 1 || P > CR_MAX_DRAWS || n_conds < 0 || n_conds > P || (n_conds > 0 && !conds))
        return DA_ERR_BADARG;
    if (sample0 < 0 || (long long)sample0 + N > 0x7FFFFFFFLL) return DA_ERR_BADARG;
    for (int q = 0; q < n_conds; ++q)
        if (conds[2 * q + 1] < 0) return DA_ERR_BADARG;
    if ((long long)D * H * W >= CR_MAX_V) return DA_ERR_BADARG;
    if (W > CR_MAX_W) return DA_ERR_UNSUPPORTED;
    if (n_conds > 0 && (!ws || ws_bytes < da_crop_sample_starts_ws_bytes(N, D, H, W, window3, include_last))) return DA_ERR_WS_SMALL;
    hipStream_t st = da_stream(stream);
    const long long NP = (long long)N * P;
    hipLaunchKernelGGL(crop_pick_uniform_kernel, dim3((unsigned)da_cdiv(NP, CR_BLOCK)), dim3(CR_BLOCK), 0, st, draw_cond, N, P, g.Dd, g.Hd, g.Wd,
                       seed, sample0, starts, info);
    DA_LAUNCH_CHECK();
    if (n_conds == 0) return 0;
    const int nW = cr_words(g);
    const CrWs l = cr_layout(N, D, H, g, ws);
    unsigned short* rows = l.rows; int* hs = l.hs; u64* mask = l.mask; unsigned* zcount = l.zcount; u64* best = l.best;
    const long long inner = (long long)g.Hd * g.Wd;
    const int seg = cr_seg(g.wd);
    const dim3 sgrid((unsigned)da_cdiv(inner, CR_BLOCK), (unsigned)da_cdiv(g.Dd, seg), (unsigned)N);
    for (int q = 0; q < n_conds; ++q) {
        if (q == 0 || conds[2 * q] != conds[2 * (q - 1)]) {                       // draws that share a class share its row and H passes
            const int rc = cr_class_passes(labels, label_dtype, N, D, H, W, g, (long long)conds[2 * q], rows, hs, st);
            if (rc) return rc;
        }
        const hipError_t e = hipMemsetAsync(best, 0, sizeof(u64) * (size_t)N, st);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(crop_select_kernel, sgrid, dim3(CR_BLOCK), 0, st, (const int*)hs, mask, best, D, g.wd, g.Dd, inner, nW, seg, conds[2 * q + 1]);
        DA_LAUNCH_CHECK();
        hipLaunchKernelGGL(crop_plane_count_kernel, dim3((unsigned)g.Dd, (unsigned)N), dim3(CR_BLOCK), 0, st, (const u64*)mask, zcount, g.Dd, nW);
        DA_LAUNCH_CHECK();
        hipLaunchKernelGGL(crop_pick_kernel, dim3((unsigned)P, (unsigned)N), dim3(CR_BLOCK), 0, st, draw_cond, q, (const int*)hs, (const u64*)mask,
                           (const unsigned*)zcount, (const u64*)best, P, D, g.wd, g.Dd, g.Hd, g.Wd, nW, seed, sample0, starts, info);
        DA_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int da_crop_gather(const float* img, float* img_out, int C, const void* labels, void* labels_out, int label_bytes, const int* starts,
                              int N, int P, int D, int H, int W, const int* window3, void* stream) {
    CrGeom g;
    if (!starts || (!img && !labels) || (img && (!img_out || C < 1)) || (labels && !labels_out) || !cr_dims_ok(N, D, H, W)) return DA_ERR_BADARG;
    if (labels && label_bytes != 1 && label_bytes != 4 && label_bytes != 8) return DA_ERR_BADARG;
    if (!cr_geom(D, H, W, window3, 1, g) || P < 1 || P > CR_MAX_DRAWS) return DA_ERR_BADARG;
    if ((long long)D * H * W >= CR_MAX_V) return DA_ERR_BADARG;
    const long long NP = (long long)N * P;
    const bool vec = g.ww % 4 == 0;
    const long long items = (long long)(img ? C : 0) * NP * g.wd * g.wh * (g.ww / (vec ? 4 : 1)) + (labels ? NP * g.wd * g.wh * (g.ww / (vec ? 4 : 1)) : 0);
    const dim3 grid(da_grid(items, CR_BLOCK)), block(CR_BLOCK);
    hipStream_t st = da_stream(stream);
#define CR_GATHER(TL, V) hipLaunchKernelGGL((crop_gather_kernel<TL, V>), grid, block, 0, st, img, img_out, C, (const TL*)labels, (TL*)labels_out, \
                                            starts, NP, P, D, H, W, g.wd, g.wh, g.ww)
    if (!labels || label_bytes == 1) { if (vec) CR_GATHER(unsigned char, 4); else CR_GATHER(unsigned char, 1); }
    else if (label_bytes == 4) { if (vec) CR_GATHER(int, 4); else CR_GATHER(int, 1); }
    else { if (vec) CR_GATHER(long long, 4); else CR_GATHER(long long, 1); }
#undef CR_GATHER
    DA_LAUNCH_CHECK();
    return 0;
}
