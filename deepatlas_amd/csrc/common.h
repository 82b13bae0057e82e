// Shared device helpers for libdeepatlas_hip (gfx950 / CDNA4 only: wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/deepatlas_hip.h"

#define DA_WAVE 64

#define DA_LAUNCH_CHECK()                                   \
    do {                                                    \
        hipError_t e__ = hipGetLastError();                 \
        if (e__ != hipSuccess) return (int)e__;             \
    } while (0)

// Launch of a kernel whose dynamic LDS exceeds the default limit: hipFuncAttributeMaxDynamicSharedMemorySize is set once per kernel (the
// function-local static: one per instantiation, initialised thread-safely), then the launch and its check.  The attribute is LdsBound bytes,
// or, by default, the first launch's `lds`: a kernel whose LDS size varies from call to call passes the largest size it can ask for.
//   return da_launch_lds<my_kernel<8, 2>>(dim3(nb), dim3(256), lds, st, params);
template <auto Kern, int LdsBound = 0, typename... Args>
static inline int da_launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, LdsBound ? LdsBound : (int)lds);
    if (attr != hipSuccess) return (int)attr;
    hipLaunchKernelGGL(Kern, grid, block, lds, st, args...);
    DA_LAUNCH_CHECK();
    return 0;
}

static inline hipStream_t da_stream(void* s) { return (hipStream_t)s; }
__host__ __device__ static inline long long da_cdiv(long long a, long long b) { return (a + b - 1) / b; }
static inline size_t da_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// Workspace carving.  A workspace is described ONCE, by a layout function that walks a DaCarve over a base pointer: da_X_ws_bytes calls it with a null base and
// returns the total, the launcher calls it with `ws` and reads the pointers (`return L{c.take<A>(n), c.take<B>(m), c.off};` -- braces evaluate left to right).
// take<T>(n) is the next region (null when sizing) and moves `off` to the next multiple of `align` behind it; align = 1 packs the next region directly behind.
struct DaCarve {
    char* base; size_t off = 0;
    explicit DaCarve(void* ws) : base((char*)ws) {}
    template <typename T> T* take(size_t n, size_t align = 256) { T* p = base ? (T*)(base + off) : nullptr; off = da_align(off + n * sizeof(T), align); return p; }
};
// Nothing is located from the caller's ws_bytes.  The column-sum scratch of the weight gradients that also produce dbias (da_colsum's workspace, da_bn_ws_bytes(0, Cout)
// bytes) is the tail of the REQUIRED size `need` = da_X_ws_bytes(...); the `front` bytes before it are the budget of the weight gradient itself.
struct DaColsumTail { size_t front; void* ws; size_t bytes; };
static inline DaColsumTail da_colsum_tail(void* ws, size_t need, int Cout) {
    const size_t bytes = da_bn_ws_bytes(0, Cout);
    return DaColsumTail{need - bytes, ws ? (char*)ws + (need - bytes) : nullptr, bytes};
}
// the packed weights of the split-mode stride-2, up-sampling and flow convolutions: the weight scale exponents in a 256-byte slot, then the operand, which starts where
// `c` stands afterwards (the size function takes its bytes from there; a launcher needs the two pointers only)
struct DaExpPack { int* wexp; unsigned char* wp; };
static inline DaExpPack da_exp_pack(DaCarve& c) { int* e = c.take<int>(1); return DaExpPack{e, c.base ? (unsigned char*)c.base + c.off : nullptr}; }

// grid size for grid-stride elementwise kernels: enough workgroups to fill 256 CUs x 8, capped
static inline int da_grid(long long work_items, int block, int cap = 256 * 16) {
    long long g = da_cdiv(work_items, block);
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// XCD-contiguous grid-stride loop for kernels whose neighbouring items share cache lines (stencils, gathers).  Workgroup b runs on XCD b % 8 and every
// XCD has its own L2: with the plain loop `i = b * blockDim + t; i += gridDim * blockDim` all eight XCDs walk the same window of the tensor together and
// each of their L2s fetches every line of it -- 7 - 8 x the tensor's bytes over the fabric (measured: bending energy 410 + 730 MB per call for a 59 MB
// field, profiles/r06_step_traffic_reg.txt).  Here XCD x owns the contiguous eighth [total x / 8, total (x + 1) / 8) (rounded to `align` items) and its
// gridDim / 8 workgroups stride through it together.  Falls back to the plain loop when gridDim.x is not a multiple of 8.
//   for (DaXcdLoop L = da_xcd_loop(total); L.i < L.end; L.i += L.step) { ... L.i ... }
struct DaXcdLoop { long long i, end, step; };
__device__ __forceinline__ DaXcdLoop da_xcd_loop(long long total, long long align = 256) {
    DaXcdLoop L;
    const long long G = gridDim.x, b = blockIdx.x, T = blockDim.x;
    if ((G & 7) != 0) { L.i = b * T + threadIdx.x; L.end = total; L.step = G * T; return L; }
    const long long x = b & 7, j = b >> 3, J = G >> 3;
    const long long units = (total + align - 1) / align;
    const long long lo = units * x / 8 * align, hi = (x == 7) ? total : units * (x + 1) / 8 * align;
    L.i = lo + j * T + threadIdx.x; L.end = hi < total ? hi : total; L.step = J * T;
    return L;
}

// the same split for loops over work items (tiles, rows): `for (it = b; it < n; it += G)` becomes `for (DaXcdItems L = da_xcd_items(n, ...); L.i < L.end; L.i += L.step)`.
// sub / nsub: position of a wave inside its workgroup when the waves, not the workgroups, take the items.
struct DaXcdItems { long long i, end, step; };
__device__ __forceinline__ DaXcdItems da_xcd_items(long long n, int sub = 0, int nsub = 1) {
    DaXcdItems L;
    const long long G = gridDim.x, b = blockIdx.x;
    if ((G & 7) != 0) { L.i = b * nsub + sub; L.end = n; L.step = G * nsub; return L; }
    const long long x = b & 7, j = b >> 3, J = G >> 3;
    L.i = n * x / 8 + j * nsub + sub; L.end = n * (x + 1) / 8; L.step = J * nsub;
    return L;
}
// ... and for kernels that take ONE item per workgroup (grid = item count): the item of workgroup b, consecutive items on the same XCD (bijective)
__device__ __forceinline__ int da_xcd_item_of_block(int b, int n) {
    const int q = n / 8, r = n % 8;
    const int xcd = b % 8, loc = b / 8;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + loc;
}
// item t of a tile list -> sample n and tile indices, z fastest, then y, then x: z / y neighbours share the most halo and, behind
// da_xcd_item_of_block, run back to back on one XCD.  The caller multiplies by its own tile extents.
__device__ __forceinline__ void da_tile_zyx(int t, int ntz, int nty, int ntx, int& n, int& tz, int& ty, int& tx) {
    tz = t % ntz; t /= ntz;
    ty = t % nty; t /= nty;
    tx = t % ntx; n = t / ntx;
}

__device__ __forceinline__ float da_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double da_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float da_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double da_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// the same butterflies over the L lanes (a power of two, <= 64) that own one voxel's channels; every lane of the group gets the result
template <int L> __device__ __forceinline__ float da_group_max(float v) {
#pragma unroll
    for (int m = 1; m < L; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
template <int L> __device__ __forceinline__ float da_group_sum(float v) {
#pragma unroll
    for (int m = 1; m < L; m <<= 1) v += __shfl_xor(v, m);
    return v;
}
// softmax of one voxel in place: lpv lanes (a run-time power of two, <= 64) own the voxel, 4 channels each.  One definition for the Dice
// kernels (losses.hip) and the fused label-warp Dice (warp.hip): both phases of the joint step form the same probabilities.
__device__ __forceinline__ void da_group_softmax4(float (&x)[4], int lpv) {
    float m = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
    for (int o = 1; o < lpv; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { x[j] = expf(x[j] - m); s += x[j]; }
    for (int o = 1; o < lpv; o <<= 1) s += __shfl_xor(s, o);
    const float inv = 1.f / s;
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] *= inv;
}

// Entry k of the four waves' results staged in `double red[4][K]`, combined in wave order.  The order is fixed on purpose: it is part of the
// determinism contract of the statistics kernels (two runs are bit-identical), so it is written once.  Staging into `red`, and which
// thread combines, stay with each kernel.
template <int K> __device__ __forceinline__ double da_sum4(double (*red)[K], int k) { return ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]; }
template <int K> __device__ __forceinline__ double da_max4(double (*red)[K], int k) { return fmax(fmax(red[0][k], red[1][k]), fmax(red[2][k], red[3][k])); }

// block-wide sum of a double; result valid in thread 0.  `red` must hold blockDim.x/64 doubles.
__device__ __forceinline__ double da_block_sum(double v, double* red) {
    v = da_wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int i = 0; i < nw; ++i) r += red[i];
    }
    return r;
}

__device__ __forceinline__ float da_act(float z, float slope) {
    // slope < 0: identity; slope == 0: ReLU; slope > 0: LeakyReLU(slope)
    return (slope < 0.f) ? z : (z > 0.f ? z : z * slope);
}
__device__ __forceinline__ float da_act_grad(float z, float slope) {
    // derivative wrt pre-activation z; PyTorch: grad * (z > 0 ? 1 : slope)
    return (slope < 0.f) ? 1.f : (z > 0.f ? 1.f : slope);
}

// out[o] = sum_b partial[b][o] in double.  256 threads = 64 consecutive outputs x 4 slices of the partial list
// (coalesced 256-byte rows, 4x shorter serial chains, O/64 workgroups), combined through LDS.
int da_reduce_partials(const float* partial, int nparts, int O, float* out, hipStream_t st);
// losses.hip: Dice loss / coefficients from per-block partial sums (shared with the fused label-warp Dice in warp.hip)
int da_dice_finish(double* partial, int nblocks, int N, int C, int weight_type, int no_bg, float eps,
                   float* loss, float* coef, float* isc, hipStream_t st);
// its workspace, behind whatever `c` already holds: per-block partial sums [N][blocks][3][C] and da_dice_finish's 3*N*C floats of scratch
struct DaDiceWs { double* partial; float* isc; size_t bytes; };
static inline DaDiceWs da_dice_carve(DaCarve& c, int N, int blocks, int C) { return DaDiceWs{c.take<double>((size_t)N * blocks * 3 * C), c.take<float>((size_t)3 * N * C), c.off}; }
static inline DaDiceWs da_dice_layout(void* ws, int N, int blocks, int C) { DaCarve c(ws); return da_dice_carve(c, N, blocks, C); }
// ---------------------------------------------------------------------------------------------------
// bf16 ACTIVATION STORAGE (BASELINE configs[4]: "bf16 activations / MFMA, fp32 master weights, fp32 reductions").  The `_bf16` twins of
// the C-ABI entry points take the network-internal activation / gradient tensors as bf16 in HBM (same NDHWC layout, 2 bytes per
// element); everything a kernel computes with stays fp32 (or double for the reductions) and a value is rounded to nearest-even once,
// when it is stored.  Kernels are templates over the storage type T in {float, da_bf16} and touch memory only through these helpers.
// ---------------------------------------------------------------------------------------------------
struct da_bf16 { unsigned short v; };
template <typename T> struct DaEl;
template <> struct DaEl<float>   { static constexpr int bytes = 4; static constexpr bool bf = false; };
template <> struct DaEl<da_bf16> { static constexpr int bytes = 2; static constexpr bool bf = true; };

__device__ __forceinline__ unsigned da_pack_bf16x2(float lo, float hi) {      // round-to-nearest-even, one v_cvt_pk_bf16_f32 (element 0 in the low half)
    typedef float da_f32x2_t __attribute__((ext_vector_type(2)));
    typedef __bf16 da_bf16x2_t __attribute__((ext_vector_type(2)));
    const da_f32x2_t v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, da_bf16x2_t));
}
__device__ __forceinline__ float da_bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float da_bf16_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }
__device__ __forceinline__ float da_round_bf16(float v) { return da_bf16_lo(da_pack_bf16x2(v, 0.f)); }      // the value a bf16 store + load round trip yields
__device__ __forceinline__ float4 da_unpack_bf16x4(uint2 u) { return make_float4(da_bf16_lo(u.x), da_bf16_hi(u.x), da_bf16_lo(u.y), da_bf16_hi(u.y)); }
__device__ __forceinline__ uint2 da_pack_bf16x4(float4 v) { return make_uint2(da_pack_bf16x2(v.x, v.y), da_pack_bf16x2(v.z, v.w)); }

// quad (4 consecutive channels) number q of a tensor: 16-byte (fp32) / 8-byte (bf16) access
__device__ __forceinline__ float4 da_ldq(const float* p, long long q) { return reinterpret_cast<const float4*>(p)[q]; }
__device__ __forceinline__ float4 da_ldq(const da_bf16* p, long long q) { return da_unpack_bf16x4(reinterpret_cast<const uint2*>(p)[q]); }
__device__ __forceinline__ void da_stq(float* p, long long q, float4 v) { reinterpret_cast<float4*>(p)[q] = v; }
__device__ __forceinline__ void da_stq(da_bf16* p, long long q, float4 v) { reinterpret_cast<uint2*>(p)[q] = da_pack_bf16x4(v); }
// streaming forms (non-temporal: the line is not kept for this kernel's sake) for passes that touch every byte once
typedef float da_f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 da_ldq_nt(const float* p, long long q) { const da_f4v v = __builtin_nontemporal_load(reinterpret_cast<const da_f4v*>(p) + q); return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void da_stq_nt(float* p, long long q, float4 v) { __builtin_nontemporal_store((da_f4v){v.x, v.y, v.z, v.w}, reinterpret_cast<da_f4v*>(p) + q); }
__device__ __forceinline__ float4 da_ldq_nt(const da_bf16* p, long long q) { return da_ldq(p, q); }
__device__ __forceinline__ void da_stq_nt(da_bf16* p, long long q, float4 v) { da_stq(p, q, v); }
// single elements
__device__ __forceinline__ float da_ld1(const float* p, long long i) { return p[i]; }
__device__ __forceinline__ float da_ld1(const da_bf16* p, long long i) { return __uint_as_float((unsigned)p[i].v << 16); }
__device__ __forceinline__ void da_st1(float* p, long long i, float v) { p[i] = v; }
__device__ __forceinline__ void da_st1(da_bf16* p, long long i, float v) { p[i].v = (unsigned short)(da_pack_bf16x2(v, 0.f) & 0xFFFFu); }

// All-reduce over the four 16-lane rows of a wave (lane = 16 g + i: same i, every g) on the VALU.  v_permlane16_swap exchanges the odd
// rows of one register with the even rows of the other, v_permlane32_swap the upper half with the lower half (gfx950): called with the
// same value twice they return (even-row copy, odd-row copy) / (lower copy, upper copy), so one swap + one add is the xor-16 / xor-32
// butterfly step -- the same pairing, hence bit-identical sums, as two ds_bpermute shuffles at ~100 cycles each on the LDS path.
typedef unsigned da_u32x2 __attribute__((ext_vector_type(2)));
// (through inline asm: hipcc 7.2 folds r[0] + r[1] of __builtin_amdgcn_permlane16_swap(v, v) into r[0] + r[0] --
// tools/ubench/permlane_swap.hip; the s_nop cover the VALU-write -> swap and swap -> VALU-read hazards the compiler would have padded)
__device__ __forceinline__ void da_swap16(float v, float& a, float& b) {
    a = v; b = v;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void da_swap32(float v, float& a, float& b) {
    a = v; b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float da_rows_sum(float v) {
    float a, b;
    da_swap16(v, a, b); v = a + b;
    da_swap32(v, a, b); return a + b;
}
__device__ __forceinline__ float da_rows_max(float v) {
    float a, b;
    da_swap16(v, a, b); v = fmaxf(a, b);
    da_swap32(v, a, b); return fmaxf(a, b);
}

// Buffer descriptor over `bytes` bytes at `base` (raw buffer, 32-bit byte offsets).  A lane whose offset is out of range -- the kernels pass
// 0xFFFFFFFF for everything outside the volume or the tile -- loads zeros and stores nothing: the hardware range check replaces an
// exec-mask branch per access, so a tile's loads issue back to back.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t da_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, bytes, 0x00020000);
}
__device__ __forceinline__ float4 da_buf_load4(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}
__device__ __forceinline__ float da_buf_load1(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}
__device__ __forceinline__ void da_buf_store4(__amdgpu_buffer_rsrc_t r, unsigned byte_off, da_f4v v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, v), r, byte_off, 0, 0);
}
// lane ^ 1 / lane ^ 2 exchanges inside a lane quad as DPP quad_perm moves (VALU, no trip through the LDS crossbar like __shfl_xor)
__device__ __forceinline__ float da_quad_xor1(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true)); }   // quad_perm [1,0,3,2]
__device__ __forceinline__ float da_quad_xor2(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true)); }   // quad_perm [2,3,0,1]
// 4 x 4 transpose across a lane quad (q = lane & 3): in = (4 voxels x 1 channel) per lane (MFMA C layout: row = 4 g + reg), out = (1 voxel x 4 channels)
__device__ __forceinline__ da_f4v da_quad_transpose(da_f4v a, int q) {
    float t0 = a[0], t1 = a[1], t2 = a[2], t3 = a[3];
    {
        const bool odd = (q & 1) != 0;
        const float s01 = odd ? t0 : t1, s23 = odd ? t2 : t3;
        const float r01 = da_quad_xor1(s01), r23 = da_quad_xor1(s23);
        if (odd) { t0 = r01; t2 = r23; } else { t1 = r01; t3 = r23; }
    }
    {
        const bool hi2 = (q & 2) != 0;
        const float s02 = hi2 ? t0 : t2, s13 = hi2 ? t1 : t3;
        const float r02 = da_quad_xor2(s02), r13 = da_quad_xor2(s13);
        if (hi2) { t0 = r02; t1 = r13; } else { t2 = r02; t3 = r13; }
    }
    return (da_f4v){t0, t1, t2, t3};
}

// Label maps come in two width sets, and a loader reads whatever width it is not told about as int64: each launcher's own DA_ERR_BADARG
// test on label_bytes is what keeps a width out of a kernel that cannot read it.
//   1 | 8 bytes (uint8, int64): the training and evaluation kernels -- losses.hip, xent.hip, headdice.hip, warp.hip, regeval.hip.  R is the
//     type the label is used as (int in warp.hip); the cast sits in each branch, so that a narrow R never widens the byte load first.
template <typename R = long long>
__device__ __forceinline__ R da_load_label(const void* labels, int label_bytes, long long i) {
    return label_bytes == 1 ? (R)((const unsigned char*)labels)[i] : (R)((const long long*)labels)[i];
}
//   1 | 4 | 8 bytes (uint8, int32, int64): the volume utilities -- augment.hip (da_spatial_resample), cc.hip (da_cc_*), edt.hip (distance
//     maps, surfaces, surface distances).  The store writes the map back in the width it came in.
__device__ __forceinline__ long long da_load_vol_label(const void* __restrict__ p, int bytes, long long i) {
    if (bytes == 1) return (long long)((const unsigned char*)p)[i];
    if (bytes == 4) return (long long)((const int*)p)[i];
    return ((const long long*)p)[i];
}
__device__ __forceinline__ void da_store_vol_label(void* __restrict__ p, int bytes, long long i, long long v) {
    if (bytes == 1) ((unsigned char*)p)[i] = (unsigned char)v;
    else if (bytes == 4) ((int*)p)[i] = (int)v;
    else ((long long*)p)[i] = v;
}
// element i of a host-typed array as fp32, by the source-dtype code of the data path (ops.PREPROCESS_DTYPE_CODE): 0 float32, 1 float64,
// 2 int16, 3 uint8, 4 int32
__device__ __forceinline__ float da_load_as_f32(const void* src, int dtype, long long i) {
    switch (dtype) {
        case 0: return ((const float*)src)[i];
        case 1: return (float)((const double*)src)[i];
        case 2: return (float)((const short*)src)[i];
        case 3: return (float)((const unsigned char*)src)[i];
        default: return (float)((const int*)src)[i];
    }
}

// Linear voxel index -> coordinates.  In 32-bit arithmetic whenever the index fits: a 64-bit integer division costs the VALU roughly ten
// times the instructions of a 32-bit one, and the gather kernels (warps, label warps) did three per lane.
__device__ __forceinline__ void da_vox4(long long v, int D, int H, int W, int& n, int& d, int& h, int& w) {
    if (v < 0x7FFFFFFFLL) {
        unsigned r = (unsigned)v;
        const unsigned q1 = r / (unsigned)W; w = (int)(r - q1 * (unsigned)W);
        const unsigned q2 = q1 / (unsigned)H; h = (int)(q1 - q2 * (unsigned)H);
        const unsigned q3 = q2 / (unsigned)D; d = (int)(q2 - q3 * (unsigned)D);
        n = (int)q3;
    } else {
        long long r = v;
        w = (int)(r % W); r /= W;
        h = (int)(r % H); r /= H;
        d = (int)(r % D); n = (int)(r / D);
    }
}
// i -> (i / m, i % m) for a small positive m (lanes per voxel, channels): shift / mask for a power of two, 32-bit when the index fits
__device__ __forceinline__ void da_divmod(long long i, int m, long long& quot, int& rem) {
    if ((m & (m - 1)) == 0) { quot = i >> (__ffs(m) - 1); rem = (int)(i & (long long)(m - 1)); }
    else if (i < 0x7FFFFFFFLL) { const unsigned r = (unsigned)i, qq = r / (unsigned)m; quot = (long long)qq; rem = (int)(r - qq * (unsigned)m); }
    else { quot = i / m; rem = (int)(i % m); }
}
__device__ __forceinline__ void da_vox3(long long v, int H, int W, int& d, int& h, int& w) {
    if (v < 0x7FFFFFFFLL) {
        const unsigned r = (unsigned)v;
        const unsigned q1 = r / (unsigned)W; w = (int)(r - q1 * (unsigned)W);
        const unsigned q2 = q1 / (unsigned)H; h = (int)(q1 - q2 * (unsigned)H);
        d = (int)q2;
    } else {
        long long r = v;
        w = (int)(r % W); r /= W;
        h = (int)(r % H); d = (int)(r / H);
    }
}

// Jacobian of x -> x + u(x) at one voxel, u_c = disp_c (size_c - 1) / 2 voxels (the scales sx, sy, sz: da_vox_scale), disp[..][3] in NDHWC with channels
// (x, y, z) = (W, H, D) axis: J[c][a] = delta_ca + d u_c / d a with numpy.gradient's differences at unit spacing (central inside, one-sided on
// the faces, zero along an axis of extent 1).  q points to the voxel (d, h, w).  One definition for da_jacobian_det (regeval.hip) and the folding
// penalty (jacpen.hip): what is printed and what is trained cannot disagree.
struct DaF3 { float x, y, z; };
struct DaJac9 { float j00, j01, j02, j10, j11, j12, j20, j21, j22; };
__device__ __forceinline__ DaF3 da_ld3(const float* __restrict__ p, float sx, float sy, float sz) { DaF3 r; r.x = p[0] * sx; r.y = p[1] * sy; r.z = p[2] * sz; return r; }
__device__ __forceinline__ DaJac9 da_jac_at(const float* __restrict__ q, int d, int h, int w, int D, int H, int W, float sx, float sy, float sz) {
    const long long sW = 3, sH = (long long)W * 3, sD = (long long)H * W * 3;
    const int wl = w > 0 ? -1 : 0, wh = w < W - 1 ? 1 : 0;
    const int hl = h > 0 ? -1 : 0, hh = h < H - 1 ? 1 : 0;
    const int dl = d > 0 ? -1 : 0, dh = d < D - 1 ? 1 : 0;
    const DaF3 xa = da_ld3(q + wl * sW, sx, sy, sz), xb = da_ld3(q + wh * sW, sx, sy, sz);
    const DaF3 ya = da_ld3(q + hl * sH, sx, sy, sz), yb = da_ld3(q + hh * sH, sx, sy, sz);
    const DaF3 za = da_ld3(q + dl * sD, sx, sy, sz), zb = da_ld3(q + dh * sD, sx, sy, sz);
    const float kx = (wh - wl == 2) ? 0.5f : 1.f, ky = (hh - hl == 2) ? 0.5f : 1.f, kz = (dh - dl == 2) ? 0.5f : 1.f;
    DaJac9 J;
    J.j00 = 1.f + (xb.x - xa.x) * kx; J.j01 = (yb.x - ya.x) * ky; J.j02 = (zb.x - za.x) * kz;
    J.j10 = (xb.y - xa.y) * kx; J.j11 = 1.f + (yb.y - ya.y) * ky; J.j12 = (zb.y - za.y) * kz;
    J.j20 = (xb.z - xa.z) * kx; J.j21 = (yb.z - ya.z) * ky; J.j22 = 1.f + (zb.z - za.z) * kz;
    return J;
}
// det J by cofactor expansion along the first row, fp32
__device__ __forceinline__ float da_jac_det(const DaJac9& J) {
    return J.j00 * (J.j11 * J.j22 - J.j12 * J.j21) - J.j01 * (J.j10 * J.j22 - J.j12 * J.j20) + J.j02 * (J.j10 * J.j21 - J.j11 * J.j20);
}

// Trilinear sampling of a volume at identity + disp, as the warp defines it (warp.hip): `deform = disp + identity` with the identity of
// lib/utils.py:97 and grid_sample(bilinear, zeros, align_corners=True)'s unnormalisation, all in fp32.  One definition for the warp family
// (warp.hip), the inverse-consistency composition (invcons.hip), the nearest-neighbour evaluation warp and label fusion (regeval.hip) and the
// field inversion's grid nodes and points (fieldinv.hip): what is warped, composed, evaluated and inverted sample the same point.
struct DaTaps {
    int x0, y0, z0;
    float fx0, fx1, fy0, fy1, fz0, fz1;   // f?0 = coord - floor, f?1 = floor + 1 - coord
};

__device__ __forceinline__ float da_id_coord(float k, int size) {
    // lib/utils.py:97: arange(size).float() / (size - 1) * 2.0 - 1; a point between the nodes has a real index k
    return k / (float)(size - 1) * 2.0f - 1.0f;
}
__device__ __forceinline__ float da_id_coord(int k, int size) { return da_id_coord((float)k, size); }
__device__ __forceinline__ float da_unnormalize(float g, int size) {
    // grid_sampler_unnormalize(align_corners=True): ((coord + 1) / 2) * (size - 1)
    return ((g + 1.f) / 2.f) * (float)(size - 1);
}
// voxels per normalised unit along an axis of `size` nodes: a displacement (or a gradient with respect to one) changes units by this factor
__device__ __forceinline__ float da_vox_scale(int size) { return (float)(size - 1) / 2.f; }

__device__ __forceinline__ DaTaps da_make_taps(float gx, float gy, float gz, int D, int H, int W) {
    const float ix = da_unnormalize(gx, W), iy = da_unnormalize(gy, H), iz = da_unnormalize(gz, D);
    DaTaps t;
    const float x0 = floorf(ix), y0 = floorf(iy), z0 = floorf(iz);
    t.x0 = (int)x0; t.y0 = (int)y0; t.z0 = (int)z0;
    t.fx0 = ix - x0; t.fx1 = (x0 + 1.f) - ix;
    t.fy0 = iy - y0; t.fy1 = (y0 + 1.f) - iy;
    t.fz0 = iz - z0; t.fz1 = (z0 + 1.f) - iz;
    return t;
}

__device__ __forceinline__ bool da_is_finite_coord(float a, float b, float c) {
    // NaN / huge coordinates -> every tap out of range (int conversion of NaN is undefined)
    return fabsf(a) < 1e9f && fabsf(b) < 1e9f && fabsf(c) < 1e9f;
}

// B[u]: the displacement field u [D][H][W][3] (normalised units, channels (x, y, z) = (W, H, D) axis) sampled trilinearly with BORDER padding,
// F.grid_sample(u, p, 'bilinear', 'border', align_corners=True).  One definition for the field inversion and the transport of points
// (fieldinv.hip) and the native-grid warp (regapply.hip): a point carried through a field and a voxel warped through it sample the same value.
struct DaFieldDims { int D, H, W; float sx, sy, sz; };

__device__ __forceinline__ DaFieldDims da_field_dims(int D, int H, int W) {
    DaFieldDims m; m.D = D; m.H = H; m.W = W;
    m.sx = da_vox_scale(W); m.sy = da_vox_scale(H); m.sz = da_vox_scale(D);
    return m;
}

// B[u] at the normalised coordinate (gx, gy, gz), which has passed da_is_finite_coord.  After the clamp 0 <= x0 <= W - 1, so the low tap is
// always in range; the high tap is read only below the extent (its weight is 0 otherwise).
__device__ __forceinline__ bool da_field_sample_border(const float* __restrict__ u, const DaFieldDims& m, float gx, float gy, float gz, float& bx, float& by, float& bz) {
#pragma clang fp contract(off)       // every product and sum rounded on its own: the two kernels that inline this compute the same bits
    const float wx = (float)(m.W - 1), wy = (float)(m.H - 1), wz = (float)(m.D - 1);
    const float rx = ((gx + 1.f) / 2.f) * wx, ry = ((gy + 1.f) / 2.f) * wy, rz = ((gz + 1.f) / 2.f) * wz;
    const bool outside = !(rx >= 0.f && rx <= wx && ry >= 0.f && ry <= wy && rz >= 0.f && rz <= wz);
    const float ix = fminf(fmaxf(rx, 0.f), wx), iy = fminf(fmaxf(ry, 0.f), wy), iz = fminf(fmaxf(rz, 0.f), wz);
    const float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
    const int x0 = min(max((int)fx, 0), m.W - 1), y0 = min(max((int)fy, 0), m.H - 1), z0 = min(max((int)fz, 0), m.D - 1);
    const float ax1 = ix - fx, ax0 = (fx + 1.f) - ix, ay1 = iy - fy, ay0 = (fy + 1.f) - iy, az1 = iz - fz, az0 = (fz + 1.f) - iz;
    bx = 0.f; by = 0.f; bz = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int cz = k >> 2, cy = (k >> 1) & 1, cx = k & 1;
        const int x = x0 + cx, y = y0 + cy, z = z0 + cz;
        if (x < m.W && y < m.H && z < m.D) {
            const float wgt = (cx ? ax1 : ax0) * (cy ? ay1 : ay0) * (cz ? az1 : az0);
            const float* b = u + ((z * m.H + y) * m.W + x) * 3;
            bx += b[0] * wgt; by += b[1] * wgt; bz += b[2] * wgt;
        }
    }
    return outside;
}
