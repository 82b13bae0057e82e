// Connected-component labelling of a label map and the largest-component / minimum-size clean-up (no reference call site: it replaces
// scipy.ndimage.label on a host copy of the prediction, once per class and volume).
// Two voxels are connected when they hold the same non-zero label and are neighbours under the connectivity: 6 (faces), 18 (faces and
// edges) or 26 (faces, edges and corners).  Labels <= 0 are background, and so are labels >= n_class when n_class > 0.  Samples never interact.
// The canonical result is the ROOT MAP, int32 [N][D][H][W]: 0 on background, elsewhere 1 + the smallest raster index (d H + h) W + w of any
// voxel of the voxel's component.  It is a property of the input alone, so neither launch order nor the atomics below can change a bit of it.
//
// Union-find over the voxel grid, parent[v] <= v always, a root has parent[v] == v, background holds -1:
//   1. cc_local_kernel: one workgroup labels one kCcTD x kCcTH x kCcTW tile entirely in LDS (unions of every in-tile neighbour pair with the
//      min-linking loop below on LDS atomics, then every voxel walks to its tile root) and writes the tile root's GLOBAL raster index as the
//      voxel's parent.  Local index order = raster order inside a tile, so the tile root is the component's smallest raster index in the tile.
//   2. cc_seam_kernel: every voxel on a tile face unites with its forward neighbours (3 / 9 / 13 of them) that lie in another tile.
//      unite(a, b): find both roots; link the larger under the smaller with old = atomicMin(&parent[larger], smaller); done when old == larger
//      (it was still a root), otherwise go on from old.  Parents only ever decrease and only towards members of the same component, so a stale
//      read yields a former ancestor of the same component and the walk is still a walk towards the root.  The per-XCD L2s are not coherent
//      with each other and a CU's L1 is never refreshed by other CUs' stores: every read of `parent` in this launch is an agent-scope atomic
//      load, every write (path compression included) an agent-scope atomic min.  No plain load or store touches the array here.
//      No workgroup waits for another: there is no flag, no spin and no cooperative launch.
//   3. cc_flatten_kernel, a launch of its own (the kernel boundary is the only inter-workgroup hand-off): every voxel walks to its root,
//      stores root + 1, and the component sizes are counted with integer atomics at the root -- one add per run of lanes of a wave that are
//      consecutive in the raster and share a root, and for the root a wave meets first in a chunk one add per change of that root over eight
//      chunks, not one per voxel (a volume-filling component would put V adds on one address; it gets V / 512).
//   4. cc_select_kernel: per (sample, class) one 64-bit atomicMax of (size << 32) | (0xFFFFFFFF - root) over the roots -- the largest
//      component, ties to the smallest root -- plus the number of components and the class's voxel count, gathered per workgroup in LDS.
//   5. cc_filter_kernel: the cleaned map in the input's dtype.
// Integer adds, min and max commute: every output is bit-identical from run to run.
#include "common.h"

namespace {

constexpr int kCcTD = DA_CC_TILE_D, kCcTH = DA_CC_TILE_H, kCcTW = DA_CC_TILE_W;
constexpr int kCcTile = kCcTD * kCcTH * kCcTW;          // 1024 voxels per workgroup: 4 per lane
constexpr int kCcThreads = kCcTH * kCcTW;               // 256: lane t owns the column (lh, lw) = (t / TW, t % TW), one voxel per tile plane
constexpr int kCcFlatChunks = 8;                        // chunks of 64 voxels per wave of the flatten pass: 2048 voxels per workgroup
constexpr int kCcSelectBlocks = 1024;                   // workgroups per sample of the selection pass (each flushes <= 3 atomics per class)
static_assert(kCcThreads == 256, "one lane per (h, w) position of a tile plane");

// the class of a stored label: 0 = background
__device__ __forceinline__ long long cc_class(long long l, int n_class) { return (l <= 0 || (n_class > 0 && l >= (long long)n_class)) ? 0 : l; }

// neighbour offset number k = 0..26, (dd + 1) * 9 + (dh + 1) * 3 + (dw + 1): k < 13 precedes the voxel in raster order, k > 13 follows it
__device__ __forceinline__ void cc_offset(int k, int& dd, int& dh, int& dw, int& nz) {
    dd = k / 9 - 1; dh = (k / 3) % 3 - 1; dw = k % 3 - 1;
    nz = (dd != 0) + (dh != 0) + (dw != 0);
}

// Walk to the root.  Terminates: a non-root's parent is strictly smaller than the node, so x strictly decreases and is bounded by 0.
template <int Scope>
__device__ __forceinline__ int cc_find(int* p, int x) {
    int q;
    while ((q = __hip_atomic_load(p + x, __ATOMIC_RELAXED, Scope)) != x) x = q;
    return x;
}

// Min-linking union.  Terminates: an iteration that does not return replaces the larger of (a, b) by its former parent, which is strictly
// smaller (old <= parent[a] < a unless a was a root, and then old == a returns), and the finds only move down: max(a, b) strictly decreases.
template <int Scope>
__device__ __forceinline__ void cc_unite(int* p, int a, int b) {
    for (;;) {
        a = cc_find<Scope>(p, a);
        b = cc_find<Scope>(p, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, Scope);
        if (old == a) return;
        a = old;
    }
}

// Path compression after a find from x that ended at root r: every node of the path whose parent is not r yet gets min(parent, r).  r is a
// member of the node's component below the node, so the forest stays one.  Terminates: x moves to its former parent, strictly smaller, and
// the loop ends at the latest when x <= r.
__device__ __forceinline__ void cc_compress(int* p, int x, int r) {
    while (x > r) {
        const int q = __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (q <= r) return;
        x = __hip_atomic_fetch_min(p + x, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// 1. one workgroup per tile; grid (tiles, N)
__global__ void __launch_bounds__(kCcThreads)
cc_local_kernel(const void* __restrict__ labels, int bytes, int D, int H, int W, int n_class, int max_nz, int tiles_h, int tiles_w,
                int* __restrict__ parent, int* __restrict__ sizes) {
    __shared__ long long lab[kCcTile];
    __shared__ int par[kCcTile];
    const int t = threadIdx.x, lh = t / kCcTW, lw = t % kCcTW;
    const int tile = blockIdx.x;
    const int tw_i = tile % tiles_w, th_i = (tile / tiles_w) % tiles_h, td_i = tile / (tiles_w * tiles_h);
    const int d0 = td_i * kCcTD, h0 = th_i * kCcTH, w0 = tw_i * kCcTW;
    const int h = h0 + lh, w = w0 + lw;
    const long long base = (long long)blockIdx.y * D * H * W;
#pragma unroll
    for (int k = 0; k < kCcTD; ++k) {
        const int i = k * kCcThreads + t, d = d0 + k;
        long long l = 0;
        if (d < D && h < H && w < W) l = cc_class(da_load_vol_label(labels, bytes, base + ((long long)d * H + h) * W + w), n_class);
        lab[i] = l;                                    // a voxel of the tile outside the volume is background: nothing joins across the faces
        par[i] = l ? i : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kCcTD; ++k) {
        const int i = k * kCcThreads + t;
        const long long l = lab[i];
        if (l == 0) continue;
#pragma unroll
        for (int o = 0; o < 13; ++o) {                 // the 13 preceding neighbours: every in-tile pair once
            int dd, dh, dw, nz; cc_offset(o, dd, dh, dw, nz);
            if (nz > max_nz) continue;
            const int nd = k + dd, nh = lh + dh, nw = lw + dw;
            if (nd < 0 || nh < 0 || nh >= kCcTH || nw < 0 || nw >= kCcTW) continue;
            const int j = (nd * kCcTH + nh) * kCcTW + nw;
            if (lab[j] == l) cc_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i, j);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kCcTD; ++k) {
        const int i = k * kCcThreads + t, d = d0 + k;
        if (d < D && h < H && w < W) {
            int g = -1;
            if (lab[i] != 0) {
                const int r = cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i);
                g = ((d0 + r / kCcThreads) * H + (h0 + (r % kCcThreads) / kCcTW)) * W + (w0 + r % kCcTW);
            }
            const long long v = base + ((long long)d * H + h) * W + w;
            parent[v] = g;
            sizes[v] = 0;
        }
    }
}

// 2. one lane per voxel; grid (ceil(V / 256), N).  Neighbours are formed from (d, h, w), never from the raster index: a row's last voxel and
// the next row's first are not neighbours, nor are a sample's last voxel and the next sample's first.
__global__ void __launch_bounds__(256)
cc_seam_kernel(const void* __restrict__ labels, int bytes, int D, int H, int W, int n_class, int max_nz, int* __restrict__ parent_all) {
    const int V = D * H * W;
    const long long v64 = (long long)blockIdx.x * 256 + threadIdx.x;      // (the last workgroup's lanes may pass 2^31 when V is close to it)
    if (v64 >= V) return;
    const int v = (int)v64;
    const long long base = (long long)blockIdx.y * V;
    int d, h, w; da_vox3(v, H, W, d, h, w);
    const int ld = d % kCcTD, lh = h % kCcTH, lw = w % kCcTW;
    if (ld > 0 && ld < kCcTD - 1 && lh > 0 && lh < kCcTH - 1 && lw > 0 && lw < kCcTW - 1) return;      // every neighbour is in the same tile
    const long long l = cc_class(da_load_vol_label(labels, bytes, base + v), n_class);
    if (l == 0) return;
    int* parent = parent_all + base;
#pragma unroll
    for (int o = 14; o < 27; ++o) {                    // the 13 following neighbours
        int dd, dh, dw, nz; cc_offset(o, dd, dh, dw, nz);
        if (nz > max_nz) continue;
        const int nd = d + dd, nh = h + dh, nw = w + dw;
        if (nd >= D || nh < 0 || nh >= H || nw < 0 || nw >= W) continue;
        if (nd / kCcTD == d / kCcTD && nh / kCcTH == h / kCcTH && nw / kCcTW == w / kCcTW) continue;   // joined by the local pass
        const int u = (nd * H + nh) * W + nw;
        if (cc_class(da_load_vol_label(labels, bytes, base + u), n_class) != l) continue;
        cc_unite<__HIP_MEMORY_SCOPE_AGENT>(parent, v, u);
    }
    const int r = cc_find<__HIP_MEMORY_SCOPE_AGENT>(parent, v);
    cc_compress(parent, v, r);
}

// 3. a wave takes kCcFlatChunks consecutive chunks of 64 voxels; grid (ceil(V / (256 kCcFlatChunks)), N).  `parent` is only read in this launch.
// Sizes: in every chunk the root of the first foreground lane (the chunk's "dominant" root) is counted with one ballot and carried from chunk
// to chunk while it stays the same -- one add per change and one at the end; the other lanes add once per run of lanes that are consecutive in
// the raster and share a root.  Every loop trip and every wave operation is executed by all 64 lanes (lanes past the end hold -2).
__global__ void __launch_bounds__(256)
cc_flatten_kernel(const int* __restrict__ parent_all, int V, int* __restrict__ roots, int* __restrict__ sizes_all) {
    const long long base = (long long)blockIdx.y * V;
    const int* parent = parent_all + base;
    int* sizes = sizes_all + base;
    const int lane = threadIdx.x & 63;
    const long long first = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 * kCcFlatChunks);
    int carry_r = -1, carry_n = 0;                     // wave-uniform: the dominant root carried so far and its voxels not yet added
#pragma unroll 1
    for (int k = 0; k < kCcFlatChunks; ++k) {
        const long long v = first + k * 64 + lane;
        int r = -2;
        if (v < V) {
            int x = parent[v];
            if (x >= 0) {
                int q;
                while ((q = parent[x]) != x) x = q;    // terminates: q < x
            }
            r = x;                                     // -1 on background
            roots[base + v] = r + 1;
        }
        const unsigned long long fg = __ballot(r >= 0);
        if (fg == 0) continue;                         // wave-uniform
        const int dom = __shfl(r, __ffsll((long long)fg) - 1);
        if (dom != carry_r) {
            if (lane == 0 && carry_r >= 0) atomicAdd(sizes + carry_r, carry_n);
            carry_r = dom; carry_n = 0;
        }
        carry_n += __popcll(__ballot(r == dom));
        const int o = r == dom ? -1 : r;               // the others; a dominant lane ends a run like background does
        const int prev = __shfl_up(o, 1);
        const bool head = lane == 0 || prev != o;
        const unsigned long long heads = __ballot(head);
        if (head && o >= 0) {
            const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
            const int len = rest ? __ffsll((long long)rest) : 64 - lane;     // lanes up to the next run's head
            atomicAdd(sizes + o, len);
        }
    }
    if (lane == 0 && carry_r >= 0) atomicAdd(sizes + carry_r, carry_n);
}

// 4. grid (blocks, N), grid-stride over the sample; dynamic LDS: n_class x (u64 best, u64 voxels, u32 components)
__global__ void __launch_bounds__(256)
cc_select_kernel(const void* __restrict__ labels, int bytes, const int* __restrict__ sizes, int V, int n_class,
                 unsigned long long* __restrict__ best, unsigned long long* __restrict__ stats) {
    extern __shared__ unsigned long long cc_lds[];
    unsigned long long* sbest = cc_lds;
    unsigned long long* svox = cc_lds + n_class;
    unsigned int* scnt = (unsigned int*)(cc_lds + 2 * n_class);
    for (int c = threadIdx.x; c < n_class; c += 256) { sbest[c] = 0; svox[c] = 0; scnt[c] = 0; }
    __syncthreads();
    const long long base = (long long)blockIdx.y * V;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        const int s = sizes[base + i];
        if (s <= 0) continue;                          // not a root
        const long long l = cc_class(da_load_vol_label(labels, bytes, base + i), n_class);
        if (l == 0 || l >= n_class) continue;
        atomicMax(sbest + l, ((unsigned long long)(unsigned)s << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i));
        atomicAdd(svox + l, (unsigned long long)s);
        atomicAdd(scnt + l, 1u);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < n_class; c += 256) {
        if (scnt[c] == 0) continue;
        const size_t row = (size_t)blockIdx.y * n_class + c;
        atomicMax(best + row, sbest[c]);
        atomicAdd(stats + row * 3, (unsigned long long)scnt[c]);
        atomicAdd(stats + row * 3 + 2, svox[c]);
    }
}

// ... and the size of the winner, after the launch above
__global__ void cc_select_finish_kernel(const unsigned long long* __restrict__ best, int rows, unsigned long long* __restrict__ stats) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < rows) stats[(size_t)i * 3 + 1] = best[i] >> 32;
}

// 5. one lane per voxel; grid (ceil(V / 256), N).  mode 0: keep the class's largest component; mode 1: keep components of >= min_size voxels
__global__ void __launch_bounds__(256)
cc_filter_kernel(const void* __restrict__ labels, int bytes, const int* __restrict__ roots, const int* __restrict__ sizes,
                 const unsigned long long* __restrict__ best, int V, int n_class, int mode, int min_size, void* __restrict__ out) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const long long base = (long long)blockIdx.y * V;
    const long long raw = da_load_vol_label(labels, bytes, base + v);
    const long long l = cc_class(raw, n_class);
    const int r = roots[base + v];
    bool keep = false;
    if (l != 0 && r > 0) {
        if (mode == 0) {
            const unsigned long long b = best[(size_t)blockIdx.y * n_class + l];
            keep = b != 0 && (0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFull)) == (unsigned)(r - 1);
        } else {
            keep = sizes[base + r - 1] >= min_size;
        }
    }
    da_store_vol_label(out, bytes, base + v, keep ? raw : 0);
}

int cc_max_nz(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : connectivity == 26 ? 3 : 0; }
bool cc_bytes_ok(int b) { return b == 1 || b == 4 || b == 8; }

}  // namespace

extern "C" size_t da_cc_ws_bytes(int N, int D, int H, int W) {
    if (N < 1 || D < 1 || H < 1 || W < 1) return 0;
    return da_align((size_t)N * D * H * W * sizeof(int));
}

extern "C" int da_cc_label(const void* labels, int label_bytes, int N, int D, int H, int W, int n_class, int connectivity,
                           int* roots, int* sizes, void* ws, size_t ws_bytes, void* stream) {
    const int max_nz = cc_max_nz(connectivity);
    if (!labels || !roots || !sizes || !ws || !cc_bytes_ok(label_bytes) || N < 1 || N > 65535 || D < 1 || H < 1 || W < 1 || n_class < 0 || !max_nz)
        return DA_ERR_BADARG;
    const long long V = (long long)D * H * W;
    if (V >= 0x80000000LL) return DA_ERR_UNSUPPORTED;                      // raster indices, parents and sizes are int32
    if (ws_bytes < da_cc_ws_bytes(N, D, H, W)) return DA_ERR_WS_SMALL;
    hipStream_t st = da_stream(stream);
    const long long tiles_d = da_cdiv(D, kCcTD), tiles_h = da_cdiv(H, kCcTH), tiles_w = da_cdiv(W, kCcTW);
    const long long tiles = tiles_d * tiles_h * tiles_w;                   // <= V < 2^31
    const unsigned vblocks = (unsigned)da_cdiv(V, 256);
    int* parent = (int*)ws;
    hipLaunchKernelGGL(cc_local_kernel, dim3((unsigned)tiles, N), dim3(kCcThreads), 0, st, labels, label_bytes, D, H, W, n_class, max_nz,
                       (int)tiles_h, (int)tiles_w, parent, sizes);
    DA_LAUNCH_CHECK();
    if (tiles > 1) {
        hipLaunchKernelGGL(cc_seam_kernel, dim3(vblocks, N), dim3(256), 0, st, labels, label_bytes, D, H, W, n_class, max_nz, parent);
        DA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)da_cdiv(V, 256 * kCcFlatChunks), N), dim3(256), 0, st, (const int*)parent, (int)V, roots, sizes);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_cc_select(const void* labels, int label_bytes, const int* sizes, int N, long long V, int n_class,
                            unsigned long long* best, unsigned long long* stats, void* stream) {
    if (!labels || !sizes || !best || !stats || !cc_bytes_ok(label_bytes) || N < 1 || N > 65535 || V < 1 || n_class < 1) return DA_ERR_BADARG;
    if (V >= 0x80000000LL || n_class > DA_CC_MAX_CLASSES) return DA_ERR_UNSUPPORTED;
    hipStream_t st = da_stream(stream);
    long long blocks = da_cdiv(V, 256);
    if (blocks > kCcSelectBlocks) blocks = kCcSelectBlocks;
    const size_t lds = (size_t)n_class * (2 * sizeof(unsigned long long) + sizeof(unsigned int));      // <= 20 KB
    hipLaunchKernelGGL(cc_select_kernel, dim3((unsigned)blocks, N), dim3(256), lds, st, labels, label_bytes, sizes, (int)V, n_class, best, stats);
    DA_LAUNCH_CHECK();
    const int rows = N * n_class;
    hipLaunchKernelGGL(cc_select_finish_kernel, dim3((unsigned)da_cdiv(rows, 256)), dim3(256), 0, st, (const unsigned long long*)best, rows, stats);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_cc_filter(const void* labels, int label_bytes, const int* roots, const int* sizes, const unsigned long long* best,
                            int N, long long V, int n_class, int mode, int min_size, void* out, void* stream) {
    if (!labels || !roots || !out || !cc_bytes_ok(label_bytes) || N < 1 || N > 65535 || V < 1 || n_class < 1 || (mode != 0 && mode != 1))
        return DA_ERR_BADARG;
    if ((mode == 0 && !best) || (mode == 1 && (!sizes || min_size < 1))) return DA_ERR_BADARG;
    if (V >= 0x80000000LL || n_class > DA_CC_MAX_CLASSES) return DA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(cc_filter_kernel, dim3((unsigned)da_cdiv(V, 256), N), dim3(256), 0, da_stream(stream), labels, label_bytes, roots, sizes,
                       best, (int)V, n_class, mode, min_size, out);
    DA_LAUNCH_CHECK();
    return 0;
}
