// Exact Euclidean distance transform of 3-D volumes, signed distance maps of a label map and the boundary loss on them (no reference call
// site: it replaces a device-to-host copy and scipy.ndimage.distance_transform_edt once per class and volume; the loss is Kervadec et al.,
// "Boundary loss for highly unbalanced segmentation").
// A site set is the set of voxels a distance is measured to; the transform is  out(x) = min over sites y of sum_a (s_a (x_a - y_a))^2  with the
// spacing s = (sD, sH, sW) in float32.  It separates over the axes:
//   1. edt_row_kernel (W, the contiguous axis): one wave per row and site set.  Per chunk of 64 voxels one ballot of the site predicate; the
//      nearest site at or left of a lane is the highest set bit of the ballot below the lane (else the last site of the chunks before it), the
//      nearest at or right the lowest set bit above it (else the first site of the chunks behind).  A row without a site gets +inf.
//   2. edt_line_kernel along H, then along D:  out[i] = min_j g[j] + (s (i - j))^2.  A workgroup owns 64 neighbouring lines (lanes run along W,
//      so every global access is a coalesced 256-byte row), stages them in LDS in chunks of kEdtLineChunk entries, and its four waves share
//      the outputs i.  The minimum is the exhaustive one, walked outwards from j = i and pruned: it stops at the first k = |i - j| with
//      (s k)^2 >= the best value of every lane of the wave, which no later j can beat because g >= 0 and float32 rounding is
//      monotone; entries that are +inf in all 64 lanes (a ballot map of the chunk) are stepped over, and a lane whose whole line is +inf does
//      not keep the scan going.  No lower-envelope stacks, no divisions: the result IS the float32 minimum over all j.
// float32 throughout: inf + k^2 = inf needs no sentinel; with unit spacing every value is an integer below 2^24 (the entries refuse extents
// with D^2 + H^2 + W^2 >= 2^24), so the arithmetic is exact.  With another spacing a value takes two roundings per pass (s k, then the fused
// multiply-add) on non-negative terms: a relative error below 6 x 2^-24.
// Site sets come straight from the label map: set (n, c) = the voxels of sample n with label == c, or their complement.  No one-hot tensor.
// No atomics in the transform, no workgroup waits for another, every loop's trip count is bounded by an extent: outputs are functions of the input
// alone.
//
// Signed maps: phi_c = + distance to class c outside it, - distance to its complement inside it; two transforms per class, the last pass of
// each writes only the voxels of its side.  A side without a site (class absent from the sample, or filling it) yields +inf and is stored as 0.
//
// Boundary loss  L = 1 / (N K' V) sum_n sum_{c in classes} sum_x softmax(z)_c(x) phi_c(x)  on channels-last logits (one voxel = K contiguous
// floats, as xent.hip): K % 4 == 0 -> K / 4 lanes own a voxel, otherwise a thread owns it (K <= 64).  phi is PLANAR, [N][K'][D][H][W]: that is
// what the last transform pass stores coalesced, and a lane group reads 32-byte runs of a plane that the neighbouring groups complete to lines.
// A voxel's term is formed in float32 and summed in double: per thread -> per workgroup -> one finalising workgroup, a fixed order.
//
// Surface-distance metrics of two label maps (Hausdorff, its percentile, ASSD): the same transform with the SURFACE of a class as the site set
// (edt_surface_row_kernel, a sibling of edt_row_kernel on the shared edt_row_body), a gather at the other map's surface voxels and an exact
// radix select; described at the kernels, below the boundary loss.
#include "common.h"

namespace {

constexpr int kEdtLineChunk = DA_EDT_LINE_CHUNK;       // entries of a line staged in LDS at a time: 256 x 64 lanes x 4 bytes = 64 KiB
constexpr int kEdtLineFlags = (kEdtLineChunk + 4 * 64) * 4;      // bytes of the line pass's flag arrays behind the staged lines
constexpr int kEdtLineLdsMax = kEdtLineChunk * 64 * 4 + kEdtLineFlags;
static_assert(kEdtLineChunk == 256, "the line pass keeps the chunk's finite-entry map in four 64-bit ballots");
constexpr int kEdtMaxRowChunks = 64;                   // chunks of 64 voxels of a row: W < 4096 since W^2 < 2^24
constexpr size_t kEdtWsTarget = (size_t)128 << 20;     // bytes per ping-pong buffer the class groups of the signed maps are sized to
constexpr int kBlBlocks = 1024;                        // workgroups per sample of the loss kernels, at most
constexpr int kBlMaxC = 64;

// The W pass of one wave on one row: `site(w)` is the site predicate of voxel w of the row (called for w < W on a live wave only).  Shared by
// the row kernels below, which differ in the predicate alone.
template <typename Site>
__device__ __forceinline__ void edt_row_body(Site site, bool live, int q, int lane, int W, float s, float* __restrict__ out, long long dst,
                                             unsigned long long (*smask)[kEdtMaxRowChunks], int (*sleft)[kEdtMaxRowChunks]) {
    const int nch = (W + 63) >> 6;                     // <= kEdtMaxRowChunks (checked by the launchers)
    int carry = -1;                                    // wave-uniform: the last site before the chunk
    for (int c = 0; c < nch; ++c) {
        const int w = c * 64 + lane;
        bool is_site = false;
        if (live && w < W) is_site = site(w);
        const unsigned long long m = __ballot(is_site);
        if (lane == 0) { smask[q][c] = m; sleft[q][c] = carry; }
        if (m) carry = c * 64 + 63 - __clzll((long long)m);
    }
    __syncthreads();
    int rcarry = -1;                                   // wave-uniform: the first site behind the chunk
    for (int c = nch - 1; c >= 0; --c) {
        const int w = c * 64 + lane;
        const unsigned long long m = smask[q][c];
        const unsigned long long ml = m & (~0ull >> (63 - lane)), mr = m & (~0ull << lane);
        const int pl = ml ? c * 64 + 63 - __clzll((long long)ml) : sleft[q][c];
        const int pr = mr ? c * 64 + __ffsll((long long)mr) - 1 : rcarry;
        float d = INFINITY;
        if (pl >= 0) { const float dk = s * (float)(w - pl); d = dk * dk; }
        if (pr >= 0) { const float dk = s * (float)(pr - w); d = fminf(d, dk * dk); }
        if (live && w < W) out[dst + w] = d;
        if (m) rcarry = c * 64 + __ffsll((long long)m) - 1;
    }
}

// 1. grid: ceil(rows * G / 4) workgroups of 4 waves; wave id -> (row, g), g fastest so the G readers of a label row run together.
// labels [N][D][H][W]; out [N][G][D][H][W]; rows = N * D * H; classes == nullptr: the one site set `label == 0` (a mask's zero voxels).
__global__ void __launch_bounds__(256)
edt_row_kernel(const void* __restrict__ labels, int bytes, const int* __restrict__ classes, int g0, int G, int complement,
               long long rows, int DH, int W, float s, float* __restrict__ out) {
    __shared__ unsigned long long smask[4][kEdtMaxRowChunks];
    __shared__ int sleft[4][kEdtMaxRowChunks];
    const int lane = threadIdx.x & 63, q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long id = (long long)blockIdx.x * 4 + q;
    const bool live = id < rows * G;                   // (a dead wave walks the loops with an empty predicate: every wave reaches the barrier)
    const long long row = live ? id / G : 0;
    const int g = live ? (int)(id % G) : 0;
    const long long n = row / DH, dh = row % DH;
    const long long cls = classes ? (long long)classes[g0 + g] : 0;
    const long long src = row * W;                     // = (n DH + dh) W
    const long long dst = ((n * G + g) * DH + dh) * W;
    edt_row_body([&](int w) { return (da_load_vol_label(labels, bytes, src + w) == cls) != (complement != 0); }, live, q, lane, W, s, out, dst, smask, sleft);
}

// Surface voxel of class `cls` (the centre voxel (d, h, w) of sample `base` / V is known to carry it): some neighbour under the connectivity
// -- order 1 / 2 / 3 = 6 / 18 / 26 neighbours, scipy's generate_binary_structure(3, order) -- carries another label or lies outside the
// volume; = A & ~binary_erosion(A, structure, border_value=0).  Every index is formed from coordinates checked against the extents, so
// rows, planes and samples never wrap into each other.
__device__ __forceinline__ bool edt_on_surface(const void* __restrict__ labels, int bytes, long long base, int d, int h, int w,
                                               int D, int H, int W, int order, long long cls) {
    for (int dd = -1; dd <= 1; ++dd)
        for (int dh = -1; dh <= 1; ++dh)
            for (int dw = -1; dw <= 1; ++dw) {
                const int man = (dd != 0) + (dh != 0) + (dw != 0);
                if (man == 0 || man > order) continue;
                const int z = d + dd, y = h + dh, x = w + dw;
                if (z < 0 || z >= D || y < 0 || y >= H || x < 0 || x >= W) return true;
                if (da_load_vol_label(labels, bytes, base + ((long long)z * H + y) * W + x) != cls) return true;
            }
    return false;
}

// 1s. the sibling of edt_row_kernel whose site set (n, c) is the SURFACE of class c in sample n, straight from the label map.
__global__ void __launch_bounds__(256)
edt_surface_row_kernel(const void* __restrict__ labels, int bytes, const int* __restrict__ classes, int g0, int G, int order,
                       long long rows, int D, int H, int W, float s, float* __restrict__ out) {
    __shared__ unsigned long long smask[4][kEdtMaxRowChunks];
    __shared__ int sleft[4][kEdtMaxRowChunks];
    const int lane = threadIdx.x & 63, q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long id = (long long)blockIdx.x * 4 + q;
    const bool live = id < rows * G;
    const long long row = live ? id / G : 0;
    const int g = live ? (int)(id % G) : 0;
    const int DH = D * H;
    const long long n = row / DH;
    const int dh = (int)(row % DH), d = dh / H, h = dh % H;
    const long long cls = (long long)classes[g0 + g];
    const long long base = n * DH * W, src = row * W;
    const long long dst = ((n * G + g) * DH + dh) * W;
    edt_row_body([&](int w) { return da_load_vol_label(labels, bytes, src + w) == cls && edt_on_surface(labels, bytes, base, d, h, w, D, H, W, order, cls); },
                 live, q, lane, W, s, out, dst, smask, sleft);
}

// what the last pass does with a finished squared distance
struct EdtEpi {
    int mode;                    // 0: store the squared distance, 1: its square root, 2: one side of a signed map
    const void* labels;          // mode 2: [N][V]
    int bytes;
    const int* classes;          // mode 2: [Kp]
    int complement;              // mode 2: 0 = the sites were the class (store + sqrt outside it), 1 = its complement (store - sqrt inside it)
    int g0, G, Kp;               // the site sets g0 .. g0 + G - 1 of Kp are in flight: outer index o = n G + g -> plane n Kp + g0 + g
    long long V;
};

// 2. element (o, i, x) of `in` sits at (o len + i) inner + x: the H pass has o = (n, g, d), inner = W; the D pass o = (n, g), inner = H W.
// grid: outer * ceil(inner / 64) workgroups of 4 waves; dynamic LDS min(len, kEdtLineChunk) x 64 floats + kEdtLineFlags bytes.
// Lines longer than a chunk: the running minimum of output i lives in `tmp` between the chunks (the H pass passes its own output, the D pass
// the buffer the H pass has consumed); the value is final after the last chunk.
template <bool LAST>
__global__ void __launch_bounds__(256)
edt_line_kernel(const float* __restrict__ in, float* __restrict__ tmp, float* __restrict__ out, int tiles, int len, int inner, float s, EdtEpi e) {
    extern __shared__ float edt_lds[];                 // [chunk entry][lane]: a wave reads one 256-byte bank row per access; then the two flag arrays
    const int cap = len < kEdtLineChunk ? len : kEdtLineChunk;
    int* rowfin = (int*)(edt_lds + cap * 64);          // [kEdtLineChunk]: entry j of the chunk is finite in some lane
    int* lanefin = rowfin + kEdtLineChunk;             // [4][64]: the lane's line has a finite entry among those the wave staged
    const int lane = threadIdx.x & 63, q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long o = blockIdx.x / tiles;
    const int x = (int)(blockIdx.x % tiles) * 64 + lane;
    const bool valid = x < inner;
    const long long base = o * len * inner + x;
    long long obase = base;                            // of the final store
    bool keep = true, zero_inf = false;
    float sign = 1.f;
    long long vox0 = 0;
    if (LAST && e.mode == 2) {
        const long long n = o / e.G;
        const int g = (int)(o % e.G);
        obase = (n * e.Kp + e.g0 + g) * e.V + x;
        vox0 = n * e.V + x;
        sign = e.complement ? -1.f : 1.f;
        zero_inf = true;
    }
    for (int j0 = 0; j0 < len; j0 += kEdtLineChunk) {
        const int nj = len - j0 < kEdtLineChunk ? len - j0 : kEdtLineChunk;
        const int hi = j0 + nj - 1;
        const bool first = j0 == 0, last = hi == len - 1;
        if (!first) __syncthreads();                   // the previous chunk's readers are done
        int mine = 0;
        for (int j = q; j < nj; j += 4) {
            const float v = valid ? in[base + (long long)(j0 + j) * inner] : INFINITY;
            edt_lds[j * 64 + lane] = v;
            const bool fin = v < INFINITY;
            mine |= fin ? 1 : 0;
            const bool any_fin = __any(fin);
            if (lane == 0) rowfin[j] = any_fin ? 1 : 0;
        }
        lanefin[q * 64 + lane] = mine;
        __syncthreads();
        // a lane whose line is all +inf in this chunk can gain nothing: it does not keep the wave's scan going
        const bool has = (lanefin[lane] | lanefin[64 + lane] | lanefin[128 + lane] | lanefin[192 + lane]) != 0;
        // bit j of the 256-bit map m: entry j is finite in some lane.  The scans visit only those entries: all others are +inf in every lane.
        unsigned long long m[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) { const int j = w * 64 + lane; m[w] = __ballot(j < nj && rowfin[j] != 0); }
        const auto word = [&](int w) { return w == 0 ? m[0] : w == 1 ? m[1] : w == 2 ? m[2] : m[3]; };
        const auto prev_set = [&](int p) {             // the largest set position <= p, or -1; at most four words
            while (p >= 0) {
                const int w = p >> 6;
                const unsigned long long bits = word(w) & (~0ull >> (63 - (p & 63)));
                if (bits) return (w << 6) + 63 - __clzll((long long)bits);
                p = (w << 6) - 1;
            }
            return -1;
        };
        const auto next_set = [&](int p) {             // the smallest set position >= p, or nj
            while (p < nj) {
                const int w = p >> 6;
                const unsigned long long bits = word(w) & (~0ull << (p & 63));
                if (bits) return (w << 6) + __ffsll((long long)bits) - 1;
                p = (w + 1) << 6;
            }
            return nj;
        };
        const int first_set = next_set(0), last_set = prev_set(nj - 1);      // nj / -1: the chunk is +inf in every lane
        for (int i = q; i < len; i += 4) {             // i, r, k and the map are wave-uniform: so is every branch
            float best = INFINITY;
            if (!first && valid) best = tmp[base + (long long)i * inner];
            const int r = i - j0;                      // the output's position relative to the chunk, possibly outside it
            if (last_set >= 0) {
                // k = |r - j| runs from the nearest entry that is finite in some lane to the farthest, two steps a trip (four loads in flight),
                // and stops at the first k that is too far for every lane.  A candidate outside the chunk reads entry 0 at distance +inf.
                const int pl = prev_set(r < nj - 1 ? r : nj - 1), pr = next_set(r + 1 > 0 ? r + 1 : 0);
                const int kl = pl >= 0 ? r - pl : 0x7FFFFFFF, kr = pr < nj ? pr - r : 0x7FFFFFFF;
                const int kend = r - first_set > last_set - r ? r - first_set : last_set - r;
                for (int k = kl < kr ? kl : kr; k <= kend; k += 2) {
                    const float d0 = s * (float)k, d1 = s * (float)(k + 1);
                    if (!__any(has && d0 * d0 < best)) break;
                    const int a0 = r - k, b0 = r + k, a1 = a0 - 1, b1 = b0 + 1;
                    const bool ia0 = a0 >= 0 && a0 < nj, ib0 = b0 >= 0 && b0 < nj, ia1 = a1 >= 0 && a1 < nj, ib1 = b1 >= 0 && b1 < nj;
                    const float ga0 = edt_lds[(ia0 ? a0 : 0) * 64 + lane], gb0 = edt_lds[(ib0 ? b0 : 0) * 64 + lane];
                    const float ga1 = edt_lds[(ia1 ? a1 : 0) * 64 + lane], gb1 = edt_lds[(ib1 ? b1 : 0) * 64 + lane];
                    const float da0 = ia0 ? d0 : INFINITY, db0 = ib0 ? d0 : INFINITY, da1 = ia1 ? d1 : INFINITY, db1 = ib1 ? d1 : INFINITY;
                    best = fminf(fminf(best, fmaf(da0, da0, ga0)), fmaf(db0, db0, gb0));
                    best = fminf(fminf(best, fmaf(da1, da1, ga1)), fmaf(db1, db1, gb1));
                }
            }
            if (!valid) continue;
            if (!LAST || !last) {
                (last ? out : tmp)[base + (long long)i * inner] = best;
            } else {
                if (e.mode == 2) {
                    const bool inside = da_load_vol_label(e.labels, e.bytes, vox0 + (long long)i * inner) == (long long)e.classes[e.g0 + (int)(o % e.G)];
                    keep = inside == (e.complement != 0);
                }
                float r = best;
                if (e.mode != 0) r = sign * (float)sqrt((double)best);      // correctly rounded: the double root rounds to the float32 root (53 >= 2 x 24 + 2)
                if (zero_inf && best == INFINITY) r = 0.f;
                if (keep) out[obase + (long long)i * inner] = r;
            }
        }
    }
}

bool edt_bytes_ok(int b) { return b == 1 || b == 4 || b == 8; }
bool edt_spacing_ok(float s) { return s > 0.f && s < INFINITY; }

// 0 or the error code of the extents
int edt_extents(int N, int D, int H, int W) {
    if (N < 1 || N > 65535 || D < 1 || H < 1 || W < 1) return DA_ERR_BADARG;
    if ((long long)D * D + (long long)H * H + (long long)W * W >= (1LL << 24)) return DA_ERR_UNSUPPORTED;     // squared distances are exact float32 integers
    if ((long long)D * H * W >= 0x80000000LL) return DA_ERR_UNSUPPORTED;
    return 0;
}

// site sets per group of the signed maps: as many as fit kEdtWsTarget bytes per buffer, at least one
int edt_group(int N, long long V, int Kp) {
    const size_t per = (size_t)N * (size_t)V * sizeof(float);
    size_t G = kEdtWsTarget / per;
    if (G < 1) G = 1;
    return G > (size_t)Kp ? Kp : (int)G;
}

// the H and D line passes of G site sets: a (the row pass's output) -> b -> (epilogue) out
int edt_line_passes(int G, int N, int D, int H, int W, float sD, float sH, float* a, float* b, float* out, EdtEpi e, hipStream_t st) {
    const long long HW = (long long)H * W;
    const int tiles_h = (int)da_cdiv(W, 64), tiles_d = (int)da_cdiv(HW, 64);
    const long long h_blocks = (long long)N * G * D * tiles_h, d_blocks = (long long)N * G * tiles_d;
    if (h_blocks > 0x7FFFFFFFLL || d_blocks > 0x7FFFFFFFLL) return DA_ERR_UNSUPPORTED;
    const size_t lds_h = (size_t)(H < kEdtLineChunk ? H : kEdtLineChunk) * 64 * sizeof(float) + kEdtLineFlags;
    const size_t lds_d = (size_t)(D < kEdtLineChunk ? D : kEdtLineChunk) * 64 * sizeof(float) + kEdtLineFlags;
    int rc = da_launch_lds<edt_line_kernel<false>, kEdtLineLdsMax>(dim3((unsigned)h_blocks), dim3(256), lds_h, st, (const float*)a, b, b, tiles_h, H, W, sH, e);
    if (rc) return rc;
    return da_launch_lds<edt_line_kernel<true>, kEdtLineLdsMax>(dim3((unsigned)d_blocks), dim3(256), lds_d, st, (const float*)b, a, out, tiles_d, D, (int)HW, sD, e);
}

// the three passes of G site sets: labels -> a -> b -> (epilogue) out
int edt_passes(const void* labels, int bytes, const int* classes, int g0, int G, int complement, int N, int D, int H, int W,
               float sD, float sH, float sW, float* a, float* b, float* out, EdtEpi e, hipStream_t st) {
    const long long rows = (long long)N * D * H;
    const long long row_blocks = da_cdiv(rows * G, 4);
    if (row_blocks > 0x7FFFFFFFLL) return DA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(edt_row_kernel, dim3((unsigned)row_blocks), dim3(256), 0, st, labels, bytes, classes, g0, G, complement, rows, D * H, W, sW, a);
    DA_LAUNCH_CHECK();
    return edt_line_passes(G, N, D, H, W, sD, sH, a, b, out, e, st);
}

// ... and with the surfaces of the classes g0 .. g0 + G - 1 as the site sets; the squared distances end in `a` ([N][G][D][H][W])
int edt_surface_passes(const void* labels, int bytes, const int* classes, int g0, int G, int order, int N, int D, int H, int W,
                       float sD, float sH, float sW, float* a, float* b, hipStream_t st) {
    const long long rows = (long long)N * D * H;
    const long long row_blocks = da_cdiv(rows * G, 4);
    if (row_blocks > 0x7FFFFFFFLL) return DA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(edt_surface_row_kernel, dim3((unsigned)row_blocks), dim3(256), 0, st, labels, bytes, classes, g0, G, order, rows, D, H, W, sW, a);
    DA_LAUNCH_CHECK();
    EdtEpi e{0, nullptr, 0, nullptr, 0, 0, G, G, (long long)D * H * W};
    return edt_line_passes(G, N, D, H, W, sD, sH, a, b, a, e, st);
}

// ------------------------------------------------------------------------------------------------------------------------------
// boundary loss
// ------------------------------------------------------------------------------------------------------------------------------
// plane of class k in phi, or -1: the slot table is device data, so it is range-checked here
__device__ __forceinline__ int bl_slot(const int* __restrict__ slots, int k, int Kp) {
    const int s = slots[k];
    return (s >= 0 && s < Kp) ? s : -1;
}

// grid (blocks, N): L = K / 4 lanes own a voxel, 16 bytes of its logits each
template <int L>
__global__ void __launch_bounds__(256)
bl_fwd_quad_kernel(const float* __restrict__ x, const float* __restrict__ phi, const int* __restrict__ slots, long long V, int Kp, double* __restrict__ partial) {
    __shared__ double red[4];
    constexpr int C = 4 * L;
    const int sub = (int)threadIdx.x & (L - 1), n = blockIdx.y;
    const float* xn = x + (long long)n * V * C;
    const float* pj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int s = bl_slot(slots, 4 * sub + j, Kp); pj[j] = s >= 0 ? phi + ((long long)n * Kp + s) * V : nullptr; }
    const long long vpb = 256 / L, passes = (V + vpb - 1) / vpb;       // every lane of a group runs the same passes (shuffles inside)
    double dacc = 0.0;
    for (long long ps = blockIdx.x; ps < passes; ps += gridDim.x) {
        const long long i = ps * vpb + (long long)(threadIdx.x / L);
        const bool in = i < V;
        const long long ii = in ? i : V - 1;
        const float4 qv = reinterpret_cast<const float4*>(xn + ii * C)[sub];
        const float v[4] = {qv.x, qv.y, qv.z, qv.w};
        const float mx = da_group_max<L>(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
        float ex[4], t = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) { ex[j] = expf(v[j] - mx); t += (pj[j] ? pj[j][ii] : 0.f) * ex[j]; }
        const float se = da_group_sum<L>(ex[0] + ex[1] + ex[2] + ex[3]);
        if (in) dacc += (double)t / (double)se;
    }
    const double s = da_block_sum(dacc, red);
    if (threadIdx.x == 0) partial[(size_t)n * gridDim.x + blockIdx.x] = s;
}

// ... and a thread owns a voxel (K % 4 != 0 or K / 4 no power of two; K <= kBlMaxC)
__global__ void __launch_bounds__(256)
bl_fwd_kernel(const float* __restrict__ x, const float* __restrict__ phi, const int* __restrict__ slots, long long V, int C, int Kp, double* __restrict__ partial) {
    __shared__ double red[4];
    const int n = blockIdx.y;
    const float* xn = x + (long long)n * V * C;
    const float* pn = phi + (long long)n * Kp * V;
    double dacc = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        float v[kBlMaxC];
        float mx = -INFINITY;
        for (int c = 0; c < C; ++c) { v[c] = xn[i * C + c]; mx = fmaxf(mx, v[c]); }
        float se = 0.f, t = 0.f;
        for (int c = 0; c < C; ++c) {
            const float ex = expf(v[c] - mx);
            se += ex;
            const int s = bl_slot(slots, c, Kp);
            if (s >= 0) t += pn[(long long)s * V + i] * ex;
        }
        dacc += (double)t / (double)se;
    }
    const double s = da_block_sum(dacc, red);
    if (threadIdx.x == 0) partial[(size_t)n * gridDim.x + blockIdx.x] = s;
}

__global__ void bl_finalize_kernel(const double* __restrict__ partial, int nparts, double scale, float* __restrict__ loss) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) s += partial[i];
    s = da_block_sum(s, red);
    if (threadIdx.x == 0) loss[0] = (float)(s * scale);
}

// dz_k = g p_k (m_k phi_k - sum_c m_c p_c phi_c) / (N K' V), the softmax recomputed
template <int L>
__global__ void __launch_bounds__(256)
bl_bwd_quad_kernel(const float* __restrict__ x, const float* __restrict__ phi, const int* __restrict__ slots, const float* __restrict__ dloss,
                   float scale, long long V, int Kp, float* __restrict__ dx) {
    constexpr int C = 4 * L;
    const int sub = (int)threadIdx.x & (L - 1), n = blockIdx.y;
    const float* xn = x + (long long)n * V * C;
    float* dn = dx + (long long)n * V * C;
    const float* pj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int s = bl_slot(slots, 4 * sub + j, Kp); pj[j] = s >= 0 ? phi + ((long long)n * Kp + s) * V : nullptr; }
    const float gs = dloss[0] * scale;
    const long long vpb = 256 / L, passes = (V + vpb - 1) / vpb;
    for (long long ps = blockIdx.x; ps < passes; ps += gridDim.x) {
        const long long i = ps * vpb + (long long)(threadIdx.x / L);
        const bool in = i < V;
        const long long ii = in ? i : V - 1;
        const float4 qv = reinterpret_cast<const float4*>(xn + ii * C)[sub];
        const float v[4] = {qv.x, qv.y, qv.z, qv.w};
        const float mx = da_group_max<L>(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
        float ex[4], f[4], t = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) { ex[j] = expf(v[j] - mx); f[j] = pj[j] ? pj[j][ii] : 0.f; t += f[j] * ex[j]; }
        const float se = da_group_sum<L>(ex[0] + ex[1] + ex[2] + ex[3]);
        const float S = da_group_sum<L>(t) / se;
        float d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = gs * (ex[j] / se) * (f[j] - S);
        if (in) reinterpret_cast<float4*>(dn + i * C)[sub] = make_float4(d[0], d[1], d[2], d[3]);
    }
}

__global__ void __launch_bounds__(256)
bl_bwd_kernel(const float* __restrict__ x, const float* __restrict__ phi, const int* __restrict__ slots, const float* __restrict__ dloss,
              float scale, long long V, int C, int Kp, float* __restrict__ dx) {
    const int n = blockIdx.y;
    const float* xn = x + (long long)n * V * C;
    const float* pn = phi + (long long)n * Kp * V;
    float* dn = dx + (long long)n * V * C;
    const float gs = dloss[0] * scale;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        float v[kBlMaxC];
        float mx = -INFINITY;
        for (int c = 0; c < C; ++c) { v[c] = xn[i * C + c]; mx = fmaxf(mx, v[c]); }
        float se = 0.f, t = 0.f;
        for (int c = 0; c < C; ++c) {
            v[c] = expf(v[c] - mx);
            se += v[c];
            const int s = bl_slot(slots, c, Kp);
            if (s >= 0) t += pn[(long long)s * V + i] * v[c];
        }
        const float S = t / se;
        for (int c = 0; c < C; ++c) {
            const int s = bl_slot(slots, c, Kp);
            const float f = s >= 0 ? pn[(long long)s * V + i] : 0.f;
            dn[i * C + c] = gs * (v[c] / se) * (f - S);
        }
    }
}

int bl_lanes(int C, const float* a, const float* b) {      // lanes per voxel of the quad kernels, 0: thread-per-voxel form
    if (C % 4 != 0) return 0;
    const int L = C / 4;
    if (L != 1 && L != 2 && L != 4 && L != 8 && L != 16) return 0;
    if (((size_t)a | (size_t)b) & 15) return 0;
    return L;
}

int bl_args(const void* logits, const void* phi, const void* slots, int N, long long V, int K, int Kp) {
    if (!logits || !phi || !slots || N < 1 || N > 65535 || V < 1 || K < 1 || Kp < 1 || Kp > K) return DA_ERR_BADARG;
    if (K > kBlMaxC || V >= 0x80000000LL) return DA_ERR_UNSUPPORTED;
    return 0;
}

int bl_blocks(long long V, int L) {
    const long long work = L ? da_cdiv(V, 256 / L) : da_cdiv(V, 256);
    return work < kBlBlocks ? (int)work : kBlBlocks;
}

// ------------------------------------------------------------------------------------------------------------------------------
// surface-distance metrics of two label maps: Hausdorff, its percentile, ASSD
// ------------------------------------------------------------------------------------------------------------------------------
// Per sample n and class c = classes[j]:  d_PT = the distances of the surface voxels of P_c to the surface of T_c, d_TP the other way round.
//   1. sd_count_kernel: the surface voxels of every class in both maps, integer atomics -> cnt[n][j][2].
//   2. sd_scan_kernel: segment (n, j) of the pooled list holds cnt[n][j][0] + cnt[n][j][1] entries; the classes partition the voxels, so the
//      list has at most 2 N V entries.
//   3. per class group and direction: edt_surface_passes of the one map, then sd_gather_kernel reads the squared distances at the other map's
//      surface voxels: sum of sqrt((double) d2) per thread -> workgroup -> partial[n][j][dir][block], the maximum of d2 by an integer atomic
//      max on its bits, and the bits appended to the segment behind a slot range from the segment's integer cursor (one add per workgroup).
//      The order inside a segment varies from run to run; everything downstream is a function of the segment as a multiset.
//   4. sd_finish_kernel, one workgroup per segment: the partial sums in their fixed order, then a radix select on the bit patterns
//      (non-negative floats order like their bits; 11 + 10 + 10 bits below the sign) for the two order statistics floor(h) and ceil(h) of the
//      rank h = p / 100 (n - 1), both in one walk per round; roots and the interpolation in double.
// Integer atomics only, no workgroup waits for another, every trip count is an extent, a segment length or the three select rounds.
constexpr int kSdBlocks = 256;                         // workgroups per (sample, class) of the counting and gather passes, at most
constexpr int kSdVoxPerBlock = 4096;                   // ... each takes a contiguous run of at least this many voxels
constexpr int kSdBins = 2048;
constexpr int kSdFinishThreads = 1024;                 // of the one workgroup that walks a segment's list three times

__host__ __device__ inline int sd_blocks(long long V) {
    const long long b = da_cdiv(V, kSdVoxPerBlock);
    return b < kSdBlocks ? (int)b : kSdBlocks;
}
__host__ __device__ inline long long sd_run(long long V) { return da_cdiv(da_cdiv(V, sd_blocks(V)), 256) * 256; }     // voxels per workgroup

// is voxel v of sample n a surface voxel of class cls in this map?
__device__ __forceinline__ bool sd_surface_at(const void* __restrict__ labels, int bytes, long long n, long long v, long long V,
                                              int D, int H, int W, int order, long long cls) {
    if (da_load_vol_label(labels, bytes, n * V + v) != cls) return false;
    int d, h, w;
    da_vox3(v, H, W, d, h, w);
    return edt_on_surface(labels, bytes, n * V, d, h, w, D, H, W, order, cls);
}

// mask[n][v] = voxel v is a surface voxel of its own class.  grid-stride over N V.
__global__ void __launch_bounds__(256)
sd_label_surface_kernel(const void* __restrict__ labels, int bytes, long long total, int D, int H, int W, int order, unsigned char* __restrict__ mask) {
    const long long V = (long long)D * H * W;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i % V;
        mask[i] = sd_surface_at(labels, bytes, n, v, V, D, H, W, order, da_load_vol_label(labels, bytes, i)) ? 1 : 0;
    }
}

// 1. grid (sd_blocks, Kp, N); cnt [N][Kp][2] (0: pred, 1: truth), zeroed by the launcher
__global__ void __launch_bounds__(256)
sd_count_kernel(const void* __restrict__ pred, int pbytes, const void* __restrict__ truth, int tbytes, const int* __restrict__ classes, int Kp,
                int D, int H, int W, int order, unsigned* __restrict__ cnt) {
    __shared__ unsigned scnt[2];
    const long long V = (long long)D * H * W, run = sd_run(V);
    const int j = blockIdx.y;
    const long long n = blockIdx.z, cls = (long long)classes[j];
    if (threadIdx.x < 2) scnt[threadIdx.x] = 0;
    __syncthreads();
    const long long lo = (long long)blockIdx.x * run, hi = lo + run < V ? lo + run : V;
    unsigned cp = 0, ct = 0;
    for (long long v = lo + threadIdx.x; v < hi; v += 256) {
        cp += sd_surface_at(pred, pbytes, n, v, V, D, H, W, order, cls) ? 1u : 0u;
        ct += sd_surface_at(truth, tbytes, n, v, V, D, H, W, order, cls) ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cp += __shfl_xor(cp, o); ct += __shfl_xor(ct, o); }
    if ((threadIdx.x & 63) == 0) { if (cp) atomicAdd(&scnt[0], cp); if (ct) atomicAdd(&scnt[1], ct); }
    __syncthreads();
    if (threadIdx.x < 2 && scnt[threadIdx.x]) atomicAdd(cnt + ((size_t)n * Kp + j) * 2 + threadIdx.x, scnt[threadIdx.x]);
}

// 2. one workgroup: off[s] = the exclusive prefix sum of cnt[s][0] + cnt[s][1] over the S = N Kp segments; a thread owns a contiguous run of them
__global__ void __launch_bounds__(256)
sd_scan_kernel(const unsigned* __restrict__ cnt, long long S, unsigned long long* __restrict__ off) {
    __shared__ unsigned long long tot[256];
    const long long per = da_cdiv(S, 256), lo = (long long)threadIdx.x * per, hi = lo + per < S ? lo + per : S;
    unsigned long long t = 0;
    for (long long i = lo; i < hi; ++i) t += (unsigned long long)cnt[2 * i] + cnt[2 * i + 1];
    tot[threadIdx.x] = t;
    __syncthreads();
    unsigned long long base = 0;
    for (int i = 0; i < (int)threadIdx.x; ++i) base += tot[i];
    for (long long i = lo; i < hi; ++i) { off[i] = base; base += (unsigned long long)cnt[2 * i] + cnt[2 * i + 1]; }
}

// 3. grid (sd_blocks, G, N).  d2 [N][G][V]: the squared distance to the surface of class classes[g0 + g] in the OTHER map; labels: the map
// whose surface voxels are gathered (dir 0: pred, distances to truth; dir 1: truth, distances to pred).  Two walks over the workgroup's run of
// voxels: the first counts each wave's surface voxels (ballots: a scalar sum), then ONE add on the segment's cursor reserves the workgroup's
// slots -- a cursor shared by every workgroup of the segment takes about 88 adds a microsecond, and an add per wave and trip ran the pass at
// that rate -- and the second walk stores wave after wave, trip after trip, lane after lane behind it.
__global__ void __launch_bounds__(256)
sd_gather_kernel(const float* __restrict__ d2, const void* __restrict__ labels, int bytes, const int* __restrict__ classes, int g0, int Kp, int dir,
                 int D, int H, int W, int order, const unsigned* __restrict__ cnt, const unsigned long long* __restrict__ off,
                 unsigned* __restrict__ cursor, unsigned* __restrict__ list, unsigned* __restrict__ maxbits, double* __restrict__ partial) {
    __shared__ double red[4];
    __shared__ unsigned smax, swave[4], sbase;
    const long long V = (long long)D * H * W, run = sd_run(V);
    const int g = blockIdx.y, G = gridDim.y, j = g0 + g, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const long long n = blockIdx.z, cls = (long long)classes[j];
    const size_t seg = (size_t)n * Kp + j;
    const unsigned seg_len = cnt[2 * seg] + cnt[2 * seg + 1];
    unsigned* seg_list = list + off[seg];
    const float* dn = d2 + ((size_t)n * G + g) * V;
    if (threadIdx.x == 0) smax = 0;
    const long long lo = (long long)blockIdx.x * run;
    unsigned mine = 0;                                                     // wave-uniform: the wave's surface voxels
    for (long long v0 = lo; v0 < lo + run && v0 < V; v0 += 256) {
        const long long v = v0 + threadIdx.x;
        mine += (unsigned)__popcll(__ballot(v < V && sd_surface_at(labels, bytes, n, v, V, D, H, W, order, cls)));
    }
    if (lane == 0) swave[q] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = swave[0] + swave[1] + swave[2] + swave[3];
        sbase = total ? atomicAdd(cursor + seg, total) : 0;
    }
    __syncthreads();
    unsigned slot0 = sbase;                                                // wave-uniform: the wave's next free slot
    for (int i = 0; i < q; ++i) slot0 += swave[i];
    double sum = 0.0;
    unsigned mx = 0;
    for (long long v0 = lo; v0 < lo + run && v0 < V; v0 += 256) {
        const long long v = v0 + threadIdx.x;
        const bool on = v < V && sd_surface_at(labels, bytes, n, v, V, D, H, W, order, cls);
        const unsigned long long m = __ballot(on);
        if (on) {
            const float x = dn[v];
            const unsigned bits = __float_as_uint(x);
            const unsigned slot = slot0 + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            if (slot < seg_len) seg_list[slot] = bits;                     // (always true: the counting pass saw the same voxels)
            sum += sqrt((double)x);
            mx = bits > mx ? bits : mx;
        }
        slot0 += (unsigned)__popcll(m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = __shfl_xor(mx, o); mx = t > mx ? t : mx; }
    if (lane == 0 && mx) atomicMax(&smax, mx);
    const double bs = da_block_sum(sum, red);                              // (its barriers order smax too)
    if (threadIdx.x == 0) {
        partial[(seg * 2 + dir) * kSdBlocks + blockIdx.x] = bs;
        if (smax) atomicMax(maxbits + seg * 2 + dir, smax);
    }
}

// the bin of `hist` that holds rank r (0-based, below the histogram's total), by one wave: lane l owns the bins [32 l, 32 l + 32).
// Returns the bin and leaves the rank inside it in r.
__device__ __forceinline__ int sd_pick_bin(const unsigned* hist, unsigned& r, int lane) {
    constexpr int per = kSdBins / 64;
    unsigned own = 0;
    for (int i = 0; i < per; ++i) own += hist[lane * per + i];
    unsigned incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    const unsigned long long m = __ballot(r < incl);
    const int L = m ? __ffsll((long long)m) - 1 : 63;
    unsigned below = __shfl(incl - own, L);
    int bin = L * per;
    for (int i = 0; i < per - 1; ++i) {                                    // wave-uniform walk of lane L's bins
        const unsigned c = hist[L * per + i];
        if (r < below + c) break;
        below += c;
        bin = L * per + i + 1;
    }
    r -= below;
    return bin;
}

// 4. grid N Kp.  out [N][Kp][7] = n_pred, n_truth, hd, hd_pct, assd, asd_pred_truth, asd_truth_pred
__global__ void __launch_bounds__(kSdFinishThreads)
sd_finish_kernel(const unsigned* __restrict__ cnt, const unsigned long long* __restrict__ off, const unsigned* __restrict__ list,
                 const unsigned* __restrict__ maxbits, const double* __restrict__ partial, int nblocks, double pct, double* __restrict__ out) {
    __shared__ double red[kSdFinishThreads / 64];
    __shared__ unsigned hist[2][kSdBins];
    __shared__ unsigned sprefix[2], srank[2];
    __shared__ double ssum[2];
    const size_t seg = blockIdx.x;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const unsigned np = cnt[2 * seg], nt = cnt[2 * seg + 1];
    double* o = out + seg * 7;
    if (np == 0 || nt == 0) {                                              // (block-uniform) the class is absent from a map: no distance is defined
        if (threadIdx.x == 0) { o[0] = (double)np; o[1] = (double)nt; for (int i = 2; i < 7; ++i) o[i] = __longlong_as_double(0x7FF8000000000000LL); }
        return;
    }
    for (int dir = 0; dir < 2; ++dir) {
        double s = 0.0;
        for (int i = threadIdx.x; i < nblocks; i += kSdFinishThreads) s += partial[(seg * 2 + dir) * kSdBlocks + i];
        s = da_block_sum(s, red);
        if (threadIdx.x == 0) ssum[dir] = s;
    }
    const unsigned len = np + nt;
    const double h = pct / 100.0 * (double)(len - 1);
    const double hf = floor(h);
    if (threadIdx.x < 2) {
        unsigned r = (unsigned)hf + (threadIdx.x == 1 && h > hf ? 1u : 0u);
        srank[threadIdx.x] = r < len ? r : len - 1;
        sprefix[threadIdx.x] = 0;
    }
    const unsigned* x = list + off[seg];
    unsigned himask = 0;                                                   // the bits the earlier rounds have fixed
    for (int round = 0; round < 3; ++round) {
        const int shift = round == 0 ? 20 : round == 1 ? 10 : 0;
        const unsigned binmask = round == 0 ? 0x7FFu : 0x3FFu;
        for (int i = threadIdx.x; i < 2 * kSdBins; i += kSdFinishThreads) (&hist[0][0])[i] = 0;
        __syncthreads();
        const unsigned p0 = sprefix[0], p1 = sprefix[1];
        const bool same = p0 == p1;                                        // both ranks are still in one bucket: one histogram serves both
        for (unsigned i0 = 0; i0 < len; i0 += kSdFinishThreads) {
            const unsigned i = i0 + threadIdx.x;
            const bool in = i < len;
            const unsigned v = in ? x[i] : 0;
            const unsigned hi = v & himask, bin = (v >> shift) & binmask;
            const bool a0 = in && hi == p0, a1 = in && !same && hi == p1;
            // most entries of a wave fall into one bin (distances 0 and 1): its lanes are counted by a ballot, the others add on their own
            const unsigned long long m0 = __ballot(a0);
            if (m0) {
                const unsigned lead = (unsigned)__shfl((int)bin, __ffsll((long long)m0) - 1);
                const unsigned long long eq = __ballot(a0 && bin == lead);
                if (lane == 0) atomicAdd(&hist[0][lead], (unsigned)__popcll(eq));
                if (a0 && bin != lead) atomicAdd(&hist[0][bin], 1u);
            }
            if (a1) atomicAdd(&hist[1][bin], 1u);
        }
        __syncthreads();
        if (q < 2) {                                                       // wave 0 picks the lower rank's bin, wave 1 the upper's
            unsigned r = srank[q];
            const int bin = sd_pick_bin(hist[same ? 0 : q], r, lane);
            if (lane == 0) { srank[q] = r; sprefix[q] = (q == 0 ? p0 : p1) | ((unsigned)bin << shift); }
        }
        himask |= binmask << shift;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double xl = sqrt((double)__uint_as_float(sprefix[0])), xh = sqrt((double)__uint_as_float(sprefix[1]));
        const unsigned mb = maxbits[2 * seg] > maxbits[2 * seg + 1] ? maxbits[2 * seg] : maxbits[2 * seg + 1];
        const double apt = ssum[0] / (double)np, atp = ssum[1] / (double)nt;
        o[0] = (double)np;
        o[1] = (double)nt;
        o[2] = sqrt((double)__uint_as_float(mb));
        o[3] = xl + (h - hf) * (xh - xl);
        o[4] = (apt + atp) / 2.0;
        o[5] = apt;
        o[6] = atp;
    }
}

int sd_order(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : connectivity == 26 ? 3 : 0; }

// the two buffers the transform's passes alternate between, G site sets of N volumes each
struct EdtWs { float *a, *b; size_t bytes; };
EdtWs edt_carve(DaCarve& c, int N, int G, long long V) { return EdtWs{c.take<float>((size_t)N * G * (size_t)V), c.take<float>((size_t)N * G * (size_t)V), c.off}; }
EdtWs edt_layout(int N, int G, long long V, void* ws) { DaCarve c(ws); return edt_carve(c, N, G, V); }
// the surface distances' workspace: the transform buffers, then list | cnt | cursor | maxbits | off | partial; cnt, cursor and maxbits are packed: zeroed together
struct SdWs { EdtWs edt; unsigned *list, *cnt, *cursor, *maxbits; unsigned long long* off; double* partial; size_t total; };
SdWs sd_layout(int N, int Kp, long long V, void* ws) {
    const size_t S = (size_t)N * Kp;
    DaCarve c(ws); return SdWs{edt_carve(c, N, edt_group(N, V, Kp), V), c.take<unsigned>(2 * (size_t)N * (size_t)V), c.take<unsigned>(S * 2, 1), c.take<unsigned>(S, 1), c.take<unsigned>(S * 2),
                c.take<unsigned long long>(S), c.take<double>(S * 2 * kSdBlocks), c.off};
}

}  // namespace

extern "C" size_t da_edt_ws_bytes(int N, int Kp, int D, int H, int W) {
    if (Kp < 1 || edt_extents(N, D, H, W) != 0) return 0;
    const long long V = (long long)D * H * W;
    return edt_layout(N, edt_group(N, V, Kp), V, nullptr).bytes;
}

extern "C" int da_edt_sq(const void* mask, int mask_bytes, int N, int D, int H, int W, float sD, float sH, float sW, int take_sqrt,
                         float* out, void* ws, size_t ws_bytes, void* stream) {
    if (!mask || !out || !ws || !edt_bytes_ok(mask_bytes) || !edt_spacing_ok(sD) || !edt_spacing_ok(sH) || !edt_spacing_ok(sW)) return DA_ERR_BADARG;
    if (const int rc = edt_extents(N, D, H, W)) return rc;
    if (ws_bytes < da_edt_ws_bytes(N, 1, D, H, W)) return DA_ERR_WS_SMALL;
    const long long V = (long long)D * H * W;
    const auto [a, b, need] = edt_layout(N, 1, V, ws);
    EdtEpi e{take_sqrt ? 1 : 0, nullptr, 0, nullptr, 0, 0, 1, 1, V};
    return edt_passes(mask, mask_bytes, nullptr, 0, 1, 0, N, D, H, W, sD, sH, sW, a, b, out, e, da_stream(stream));
}

extern "C" int da_signed_distance_maps(const void* labels, int label_bytes, const int* classes, int Kp, int N, int D, int H, int W,
                                       float sD, float sH, float sW, float* phi, void* ws, size_t ws_bytes, void* stream) {
    if (!labels || !classes || !phi || !ws || Kp < 1 || !edt_bytes_ok(label_bytes) || !edt_spacing_ok(sD) || !edt_spacing_ok(sH) || !edt_spacing_ok(sW))
        return DA_ERR_BADARG;
    if (const int rc = edt_extents(N, D, H, W)) return rc;
    if (ws_bytes < da_edt_ws_bytes(N, Kp, D, H, W)) return DA_ERR_WS_SMALL;
    const long long V = (long long)D * H * W;
    const int G = edt_group(N, V, Kp);
    const auto [a, b, need] = edt_layout(N, G, V, ws);
    for (int g0 = 0; g0 < Kp; g0 += G) {
        const int g = Kp - g0 < G ? Kp - g0 : G;
        for (int complement = 0; complement < 2; ++complement) {
            EdtEpi e{2, labels, label_bytes, classes, complement, g0, g, Kp, V};
            if (const int rc = edt_passes(labels, label_bytes, classes, g0, g, complement, N, D, H, W, sD, sH, sW, a, b, phi, e, da_stream(stream))) return rc;
        }
    }
    return 0;
}

extern "C" size_t da_boundary_loss_ws_bytes(int N) {
    if (N < 1) return 0;
    return da_align((size_t)N * kBlBlocks * sizeof(double));
}

extern "C" int da_boundary_loss_fwd(const float* logits, const float* phi, const int* slots, int N, long long V, int K, int Kp,
                                    float* loss, void* ws, size_t ws_bytes, void* stream) {
    if (!loss || !ws) return DA_ERR_BADARG;
    if (const int rc = bl_args(logits, phi, slots, N, V, K, Kp)) return rc;
    if (ws_bytes < da_boundary_loss_ws_bytes(N)) return DA_ERR_WS_SMALL;
    hipStream_t st = da_stream(stream);
    const int L = bl_lanes(K, logits, nullptr);
    const int nblocks = bl_blocks(V, L);
#define BL_FWD(l) case l: hipLaunchKernelGGL((bl_fwd_quad_kernel<l>), dim3(nblocks, N), dim3(256), 0, st, logits, phi, slots, V, Kp, (double*)ws); break;
    switch (L) {
        BL_FWD(1) BL_FWD(2) BL_FWD(4) BL_FWD(8) BL_FWD(16)
        default: hipLaunchKernelGGL(bl_fwd_kernel, dim3(nblocks, N), dim3(256), 0, st, logits, phi, slots, V, K, Kp, (double*)ws);
    }
#undef BL_FWD
    DA_LAUNCH_CHECK();
    hipLaunchKernelGGL(bl_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, N * nblocks, 1.0 / ((double)N * Kp * (double)V), loss);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_boundary_loss_bwd(const float* logits, const float* phi, const int* slots, const float* dloss, int N, long long V, int K, int Kp,
                                    float* dlogits, void* stream) {
    if (!dloss || !dlogits) return DA_ERR_BADARG;
    if (const int rc = bl_args(logits, phi, slots, N, V, K, Kp)) return rc;
    hipStream_t st = da_stream(stream);
    const float scale = (float)(1.0 / ((double)N * Kp * (double)V));
    const int L = bl_lanes(K, logits, dlogits);
    const int nblocks = bl_blocks(V, L);
#define BL_BWD(l) case l: hipLaunchKernelGGL((bl_bwd_quad_kernel<l>), dim3(nblocks, N), dim3(256), 0, st, logits, phi, slots, dloss, scale, V, Kp, dlogits); break;
    switch (L) {
        BL_BWD(1) BL_BWD(2) BL_BWD(4) BL_BWD(8) BL_BWD(16)
        default: hipLaunchKernelGGL(bl_bwd_kernel, dim3(nblocks, N), dim3(256), 0, st, logits, phi, slots, dloss, scale, V, K, Kp, dlogits);
    }
#undef BL_BWD
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_label_surface(const void* labels, int label_bytes, int N, int D, int H, int W, int connectivity, unsigned char* mask, void* stream) {
    if (!labels || !mask || !edt_bytes_ok(label_bytes) || !sd_order(connectivity)) return DA_ERR_BADARG;
    if (const int rc = edt_extents(N, D, H, W)) return rc;
    const long long total = (long long)N * D * H * W;
    hipLaunchKernelGGL(sd_label_surface_kernel, dim3(da_grid(total, 256)), dim3(256), 0, da_stream(stream), labels, label_bytes, total, D, H, W,
                       sd_order(connectivity), mask);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t da_surface_dist_ws_bytes(int N, int Kp, int D, int H, int W) {
    const size_t edt_bytes = da_edt_ws_bytes(N, Kp, D, H, W);
    if (!edt_bytes || Kp > 65535 || (long long)N * Kp > 0x7FFFFFFFLL) return 0;
    return sd_layout(N, Kp, (long long)D * H * W, nullptr).total;
}

extern "C" int da_surface_dist_stats(const void* pred, int pred_bytes, const void* truth, int truth_bytes, const int* classes, int Kp,
                                     int N, int D, int H, int W, float sD, float sH, float sW, int connectivity, double percentile,
                                     double* stats, void* ws, size_t ws_bytes, void* stream) {
    if (!pred || !truth || !classes || !stats || !ws || Kp < 1 || !edt_bytes_ok(pred_bytes) || !edt_bytes_ok(truth_bytes) || !sd_order(connectivity) ||
        !edt_spacing_ok(sD) || !edt_spacing_ok(sH) || !edt_spacing_ok(sW) || !(percentile > 0.0 && percentile <= 100.0))
        return DA_ERR_BADARG;
    if (const int rc = edt_extents(N, D, H, W)) return rc;
    if (Kp > 65535 || (long long)N * Kp > 0x7FFFFFFFLL) return DA_ERR_UNSUPPORTED;      // grid dimensions of the counting and the finishing pass
    if (ws_bytes < da_surface_dist_ws_bytes(N, Kp, D, H, W)) return DA_ERR_WS_SMALL;
    hipStream_t st = da_stream(stream);
    const long long V = (long long)D * H * W;
    const int G = edt_group(N, V, Kp), order = sd_order(connectivity), nb = sd_blocks(V);
    const auto [edt, list, cnt, cursor, maxbits, off, partial, need] = sd_layout(N, Kp, V, ws);
    float *a = edt.a, *b = edt.b;
    const long long S = (long long)N * Kp;
    if (const hipError_t e = hipMemsetAsync(cnt, 0, (size_t)S * 5 * sizeof(unsigned), st)) return (int)e;
    hipLaunchKernelGGL(sd_count_kernel, dim3(nb, Kp, N), dim3(256), 0, st, pred, pred_bytes, truth, truth_bytes, classes, Kp, D, H, W, order, cnt);
    DA_LAUNCH_CHECK();
    hipLaunchKernelGGL(sd_scan_kernel, dim3(1), dim3(256), 0, st, (const unsigned*)cnt, S, off);
    DA_LAUNCH_CHECK();
    for (int g0 = 0; g0 < Kp; g0 += G) {
        const int g = Kp - g0 < G ? Kp - g0 : G;
        for (int dir = 0; dir < 2; ++dir) {                                // 0: sites on truth, gathered on pred; 1: the other way
            const void* site = dir ? pred : truth;
            const void* at = dir ? truth : pred;
            const int site_bytes = dir ? pred_bytes : truth_bytes, at_bytes = dir ? truth_bytes : pred_bytes;
            if (const int rc = edt_surface_passes(site, site_bytes, classes, g0, g, order, N, D, H, W, sD, sH, sW, a, b, st)) return rc;
            hipLaunchKernelGGL(sd_gather_kernel, dim3(nb, g, N), dim3(256), 0, st, (const float*)a, at, at_bytes, classes, g0, Kp, dir, D, H, W, order,
                               (const unsigned*)cnt, (const unsigned long long*)off, cursor, list, maxbits, partial);
            DA_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(sd_finish_kernel, dim3((unsigned)S), dim3(kSdFinishThreads), 0, st, (const unsigned*)cnt, (const unsigned long long*)off, (const unsigned*)list,
                       (const unsigned*)maxbits, (const double*)partial, nb, percentile, stats);
    DA_LAUNCH_CHECK();
    return 0;
}
