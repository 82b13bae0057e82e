// Random spatial augmentation: the resample behind lib/transforms.py's RandomRigidTransform (:202-259) and RandomBSplineTransform
// (:161-199), i.e. sitk.Resample(img, img, transform, interpolator, default) (:287-290) with the image as its own reference grid.
// One launch per batch.  Every output voxel i = (x, y, z) = (w, h, d) maps to a continuous input index
//     q = M (i - o) + b  [+ the B-spline displacement at i, in index units],     o = (W/2, H/2, D/2)
// and the image channels (trilinear or nearest) and the label map (nearest) are sampled from that same q.  Geometry and the ITK rules
// behind it: DESIGN.md 4.18.  HBM-bound gather: each thread owns 4 consecutive W voxels (16-byte image stores, 32-bit uint8 label stores).
#include "common.h"
#include "bspline.h"

namespace {

constexpr int kBlock = 256;
constexpr int kVec = 4;                 // consecutive W voxels per thread

struct AugGeom {
    int C, D, H, W;
    int ox, oy, oz;                     // o: the centre the matrix is applied about
    int Mx, My, Mz, gx, gy, gz;         // B-spline mesh and control grid (gx = Mx + order)
    int interp;                         // image: 0 linear, 1 nearest
    int label_bytes;
};

// (B-spline support and contraction: bspline.h, shared with intensity.hip)

// where one output voxel reads: inside flag, nearest offset, the two clamped neighbours per axis and the fractions
struct Tap {
    int in, nn;
    int x0, x1, y0, y1, z0, z1;          // x: element, y: row offset (y W), z: plane offset (z H W)
    float fx, fy, fz;
};

__device__ __forceinline__ Tap make_tap(float qx, float qy, float qz, int D, int H, int W) {
    Tap t;
    // inside: -0.5 <= q < size - 0.5 on every axis (false for NaN)
    t.in = (qx >= -0.5f && qx < (float)W - 0.5f && qy >= -0.5f && qy < (float)H - 0.5f && qz >= -0.5f && qz < (float)D - 0.5f);
    if (!t.in) { qx = qy = qz = 0.f; }
    // nearest: floor(q + 0.5) (ITK's round-half-up), clamped for safety against the rounding of q + 0.5
    const int nx = min(max((int)floorf(qx + 0.5f), 0), W - 1);
    const int ny = min(max((int)floorf(qy + 0.5f), 0), H - 1);
    const int nz = min(max((int)floorf(qz + 0.5f), 0), D - 1);
    t.nn = (nz * H + ny) * W + nx;
    // linear: neighbours floor(q), floor(q) + 1, each clamped to [0, size - 1] (ITK's linear interpolator in the half-voxel band)
    const float fx = floorf(qx), fy = floorf(qy), fz = floorf(qz);
    const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    t.fx = qx - fx; t.fy = qy - fy; t.fz = qz - fz;
    t.x0 = min(max(ix, 0), W - 1);         t.x1 = min(max(ix + 1, 0), W - 1);
    t.y0 = min(max(iy, 0), H - 1) * W;     t.y1 = min(max(iy + 1, 0), H - 1) * W;
    t.z0 = min(max(iz, 0), D - 1) * H * W; t.z1 = min(max(iz + 1, 0), D - 1) * H * W;
    return t;
}

// trilinear as three lerps a + f (b - a): a zero fraction returns the corner value bit for bit
__device__ __forceinline__ float trilinear(const float* __restrict__ p, const Tap& t) {
    const float c00 = fmaf(t.fx, p[t.z0 + t.y0 + t.x1] - p[t.z0 + t.y0 + t.x0], p[t.z0 + t.y0 + t.x0]);
    const float c01 = fmaf(t.fx, p[t.z0 + t.y1 + t.x1] - p[t.z0 + t.y1 + t.x0], p[t.z0 + t.y1 + t.x0]);
    const float c10 = fmaf(t.fx, p[t.z1 + t.y0 + t.x1] - p[t.z1 + t.y0 + t.x0], p[t.z1 + t.y0 + t.x0]);
    const float c11 = fmaf(t.fx, p[t.z1 + t.y1 + t.x1] - p[t.z1 + t.y1 + t.x0], p[t.z1 + t.y1 + t.x0]);
    const float c0 = fmaf(t.fy, c01 - c00, c00);
    const float c1 = fmaf(t.fy, c11 - c10, c10);
    return fmaf(t.fz, c1 - c0, c0);
}

// grid: x = workgroups per sample (XCD-contiguous split of the sample's rows), y = sample.  Dynamic LDS: the sample's 3 x gz x gy x gx
// coefficients when O > 0.
template <int O>
__global__ __launch_bounds__(kBlock) void resample_kernel(const float* __restrict__ img, float* __restrict__ img_out,
                                                          const void* __restrict__ lab, void* __restrict__ lab_out,
                                                          const float* __restrict__ affine, const float* __restrict__ coef, AugGeom g) {
    extern __shared__ float cg[];
    const int n = blockIdx.y;
    const float* A = affine + 12 * n;
    const float m00 = A[0], m01 = A[1], m02 = A[2], b0 = A[3];
    const float m10 = A[4], m11 = A[5], m12 = A[6], b1 = A[7];
    const float m20 = A[8], m21 = A[9], m22 = A[10], b2 = A[11];
    const int D = g.D, H = g.H, W = g.W;
    const long long vol = (long long)D * H * W;
    int use_x = 0, use_y = 0, use_z = 0;
    int gp = 0;
    if constexpr (O > 0) {
        gp = g.gx * g.gy * g.gz;
        const float* src = coef + (long long)n * 3 * gp;
        int nzx = 0, nzy = 0, nzz = 0;
        for (int k = threadIdx.x; k < 3 * gp; k += kBlock) {
            const float v = src[k];
            cg[k] = v;
            if (v != 0.f) { if (k < gp) nzx = 1; else if (k < 2 * gp) nzy = 1; else nzz = 1; }
        }
        // components whose coefficients are all zero add exactly 0 and are skipped (the reference zeroes the x third)
        use_x = __syncthreads_or(nzx); use_y = __syncthreads_or(nzy); use_z = __syncthreads_or(nzz);
    }
    const float* im = img ? img + (long long)n * g.C * vol : nullptr;
    float* io = img_out ? img_out + (long long)n * g.C * vol : nullptr;
    const int QW = (W + kVec - 1) / kVec;
    const bool vec = (W % kVec) == 0;
    const long long items = (long long)D * H * QW;
    for (DaXcdLoop L = da_xcd_loop(items); L.i < L.end; L.i += L.step) {
        int d, h, qw; da_vox3(L.i, H, QW, d, h, qw);
        const int w0 = qw * kVec;
        const float uy = (float)(h - g.oy), uz = (float)(d - g.oz);
        const float rx = fmaf(m01, uy, fmaf(m02, uz, b0));
        const float ry = fmaf(m11, uy, fmaf(m12, uz, b1));
        const float rz = fmaf(m21, uy, fmaf(m22, uz, b2));
        float wy[O + 1], wz[O + 1];
        int sy = 0, sz = 0;
        if constexpr (O > 0) { sy = bspline_axis<O>(h, g.My, H, wy); sz = bspline_axis<O>(d, g.Mz, D, wz); }
        Tap t[kVec];
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
            const int w = min(w0 + j, W - 1);              // (a tail lane repeats the last voxel; it is not stored)
            const float ux = (float)(w - g.ox);
            float qx = fmaf(m00, ux, rx), qy = fmaf(m10, ux, ry), qz = fmaf(m20, ux, rz);
            if constexpr (O > 0) {
                float wx[O + 1];
                const int sx = bspline_axis<O>(w, g.Mx, W, wx);
                if (use_x) qx += bspline_contract<O>(cg, g.gx, g.gy, sx, sy, sz, wx, wy, wz);
                if (use_y) qy += bspline_contract<O>(cg + gp, g.gx, g.gy, sx, sy, sz, wx, wy, wz);
                if (use_z) qz += bspline_contract<O>(cg + 2 * gp, g.gx, g.gy, sx, sy, sz, wx, wy, wz);
            }
            t[j] = make_tap(qx, qy, qz, D, H, W);
        }
        const long long row = ((long long)d * H + h) * W + w0;
        if (lab) {
            const long long ln = (long long)n * vol;
            long long v[kVec];
#pragma unroll
            for (int j = 0; j < kVec; ++j) v[j] = t[j].in ? da_load_vol_label(lab, g.label_bytes, ln + t[j].nn) : 0;
            if (vec && g.label_bytes == 1) {
                const unsigned pk = (unsigned)(v[0] & 0xFF) | ((unsigned)(v[1] & 0xFF) << 8) | ((unsigned)(v[2] & 0xFF) << 16) | ((unsigned)(v[3] & 0xFF) << 24);
                *reinterpret_cast<unsigned*>((unsigned char*)lab_out + ln + row) = pk;
            } else {
#pragma unroll
                for (int j = 0; j < kVec; ++j)
                    if (w0 + j < W) da_store_vol_label(lab_out, g.label_bytes, ln + row + j, v[j]);
            }
        }
        if (im) {
            for (int c = 0; c < g.C; ++c) {
                const float* p = im + c * vol;
                float r[kVec];
#pragma unroll
                for (int j = 0; j < kVec; ++j)
                    r[j] = !t[j].in ? 0.1f : (g.interp == 1 ? p[t[j].nn] : trilinear(p, t[j]));
                float* o = io + c * vol + row;
                if (vec) {
                    *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < kVec; ++j)
                        if (w0 + j < W) o[j] = r[j];
                }
            }
        }
    }
}

template <int O>
int launch(const float* img, float* img_out, const void* lab, void* lab_out, const float* affine, const float* coef,
           const AugGeom& g, int N, hipStream_t st) {
    const long long items = (long long)g.D * g.H * ((g.W + kVec - 1) / kVec);
    long long bx = da_cdiv(items, kBlock);
    bx = da_cdiv(bx, 8) * 8;                               // a multiple of 8: da_xcd_loop's contiguous per-XCD ranges
    if (bx > 1024) bx = 1024;
    const size_t lds = O > 0 ? (size_t)3 * g.gx * g.gy * g.gz * sizeof(float) : 0;
    hipLaunchKernelGGL(resample_kernel<O>, dim3((unsigned)bx, (unsigned)N), dim3(kBlock), lds, st,
                       img, img_out, lab, lab_out, affine, coef, g);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int da_spatial_resample(const float* img, float* img_out, int C, int interp,
                                   const void* labels, void* labels_out, int label_bytes,
                                   const float* affine, const float* coef, int order, int gx, int gy, int gz,
                                   int N, int D, int H, int W, void* stream) {
    if (N <= 0 || N > 65535 || D <= 0 || H <= 0 || W <= 0 || !affine) return DA_ERR_BADARG;
    if (!img && !labels) return DA_ERR_BADARG;
    if ((img == nullptr) != (img_out == nullptr) || (labels == nullptr) != (labels_out == nullptr)) return DA_ERR_BADARG;
    if (img && (C <= 0 || (interp != 0 && interp != 1) || (const void*)img == (const void*)img_out)) return DA_ERR_BADARG;
    if (labels && ((label_bytes != 1 && label_bytes != 4 && label_bytes != 8) || labels == labels_out)) return DA_ERR_BADARG;
    if (order < 0 || order > 3) return DA_ERR_BADARG;
    if (order > 0 && (!coef || D < 2 || H < 2 || W < 2 || gx < order + 1 || gy < order + 1 || gz < order + 1)) return DA_ERR_BADARG;
    if ((long long)D * H * W > 0x7FFFFFFFLL) return DA_ERR_UNSUPPORTED;                     // 32-bit offsets inside one volume
    if (order > 0 && (long long)gx * gy * gz > DA_AUG_MAX_GRID_POINTS) return DA_ERR_UNSUPPORTED;
    if (order > 0 && ((long long)W * (gx - order) > 0x7FFFFFFFLL || (long long)H * (gy - order) > 0x7FFFFFFFLL
                      || (long long)D * (gz - order) > 0x7FFFFFFFLL)) return DA_ERR_UNSUPPORTED;   // i M in 32 bits
    AugGeom g;
    g.C = img ? C : 0; g.D = D; g.H = H; g.W = W;
    g.ox = W / 2; g.oy = H / 2; g.oz = D / 2;
    g.gx = gx; g.gy = gy; g.gz = gz;
    g.Mx = gx - order; g.My = gy - order; g.Mz = gz - order;
    g.interp = interp; g.label_bytes = labels ? label_bytes : 1;
    hipStream_t st = da_stream(stream);
    switch (order) {
        case 0: return launch<0>(img, img_out, labels, labels_out, affine, coef, g, N, st);
        case 1: return launch<1>(img, img_out, labels, labels_out, affine, coef, g, N, st);
        case 2: return launch<2>(img, img_out, labels, labels_out, affine, coef, g, N, st);
        default: return launch<3>(img, img_out, labels, labels_out, affine, coef, g, N, st);
    }
}
