// Stride-2 3x3x3 convolutions (the registration encoder, voxel_morph.py:46-47, modules.py:48) on the MFMA kernels.
//
// out[o] = sum_t W[t] . X[2o - 1 + t].  Split X into its 8 parity sub-volumes X_r[q] = X[2q + r]: tap t = 0 reads the
// odd sub-volume at q = o - 1, t = 1 the even one at q = o, t = 2 the odd one at q = o.  Hence the stride-2 conv is a
// STRIDE-1 conv over the space-to-depth tensor S[q][r*Cin + ci] (8*Cin channels, half resolution) whose 27-tap kernel is
// zero except for (1|2)^3 taps per parity.  The MFMA kernels take a per-chunk tap mask and skip the zero K-steps, so
// the MFMA work equals the original 27*Cin*Cout per output voxel.  S is never materialised: the kernels address X (and dX) through
// the space-to-depth view.
#include "common.h"
#include "conv3d_internal.h"

namespace {

// W[27][Cin][Cout] -> W'[27][8*Cin][Cout]: offset index o_a (q offset o_a - 1) of parity r_a carries original tap
// (r_a = 0: o 1 <- t 1) (r_a = 1: o 0 <- t 0, o 1 <- t 2); everything else is zero.
__device__ __forceinline__ int orig_tap_axis(int r, int o) { return r == 0 ? (o == 1 ? 1 : -1) : (o == 0 ? 0 : (o == 1 ? 2 : -1)); }

__global__ void expand_weights_s2d_kernel(const float* __restrict__ w, float* __restrict__ we, int Cin, int Cout) {
    const int total = 27 * 8 * Cin * Cout;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int co = i % Cout; int t = i / Cout;
        const int ci = t % Cin; t /= Cin;
        const int r = t % 8; const int tp = t / 8;
        const int tz = orig_tap_axis((r >> 2) & 1, tp / 9), ty = orig_tap_axis((r >> 1) & 1, (tp / 3) % 3), tx = orig_tap_axis(r & 1, tp % 3);
        we[i] = (tz >= 0 && ty >= 0 && tx >= 0) ? w[((size_t)((tz * 3 + ty) * 3 + tx) * Cin + ci) * Cout + co] : 0.f;
    }
}

// dW[t][ci][co] = dW'[o(t)][r(t)*Cin + ci][co]:  t_a = 0 -> (r 1, o 0); 1 -> (r 0, o 1); 2 -> (r 1, o 1)
__global__ void extract_wgrad_s2d_kernel(const float* __restrict__ dwe, float* __restrict__ dw, int Cin, int Cout) {
    const int total = 27 * Cin * Cout;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int co = i % Cout; int t = i / Cout;
        const int ci = t % Cin; const int tap = t / Cin;
        const int ta[3] = {tap / 9, (tap / 3) % 3, tap % 3};
        int r = 0, o = 0;
        for (int a = 0; a < 3; ++a) { r = r * 2 + (ta[a] == 1 ? 0 : 1); o = o * 3 + (ta[a] == 0 ? 0 : 1); }
        dw[i] = dwe[((size_t)o * 8 * Cin + r * Cin + ci) * Cout + co];
    }
}

// the space-to-depth route's workspace: [W' expanded][dW' expanded][inner conv scratch]; kInnerPad: slack behind the inner call's own size, nothing is placed there (kept: sizes do not change)
constexpr size_t kInnerPad = 65536;
struct S2Plan { int Dq, Hq, Wq; size_t inner_bytes; float *We, *dWe; char* inner; size_t bytes; };
static S2Plan s2_plan(int N, int D, int H, int W, int Cin, int Cout, void* ws = nullptr) {
    const int Dq = (D + 1) / 2, Hq = (H + 1) / 2, Wq = (W + 1) / 2;
    const size_t inner = da_conv3_mfma_ws_bytes(N, Dq, Hq, Wq, 8 * Cin, Cout, 1) + kInnerPad, we = (size_t)27 * 8 * Cin * Cout;
    DaCarve c(ws); return S2Plan{Dq, Hq, Wq, inner, c.take<float>(we), c.take<float>(we), c.take<char>(inner, 1), c.off};
}

// split matrix mode: the native stride-2 kernels (conv3d_s2n.hip) take the shapes they support; the other modes take the masked route
bool s2_native(int Cin, int Cout, int N, int D, int H, int W) {
    return da_matrix_mode() == 2 && da_conv3_s2n_supported(Cin, Cout, N, D, H, W);
}

}  // namespace

bool da_conv3_s2_supported(int C1, int C2, int Cout) { return C2 == 0 && C1 % 16 == 0 && C1 <= 32 && Cout >= 8 && Cout % 4 == 0; }

size_t da_conv3_s2_ws_bytes(int N, int D, int H, int W, int Cin, int Cout) {
    size_t b = s2_plan(N, D, H, W, Cin, Cout).bytes;
    if (da_conv3_s2n_supported(Cin, Cout, N, D, H, W)) { const size_t nb = da_conv3_s2n_ws_bytes(N, D, H, W, Cin, Cout); if (nb > b) b = nb; }
    return b;
}

// The MFMA kernels read X / write dX through the space-to-depth view (DaS2dFuse).
int da_conv3_s2_fwd(const float* in, int Cin, const float* w_tio, const float* bias, float* out,
                    int N, int D, int H, int W, int Cout, float slope, void* ws, size_t ws_bytes, hipStream_t st, int act_bf16) {
    if (act_bf16 && da_matrix_mode() != 1) return DA_ERR_UNSUPPORTED;      // bf16 activation storage: bf16 matrix mode
    if (s2_native(Cin, Cout, N, D, H, W)) return da_conv3_s2n_fwd(in, Cin, w_tio, bias, out, N, D, H, W, Cout, slope, ws, ws_bytes, st);
    const S2Plan p = s2_plan(N, D, H, W, Cin, Cout, ws);
    if (ws_bytes < da_conv3_s2_ws_bytes(N, D, H, W, Cin, Cout)) return DA_ERR_WS_SMALL;
    float* We = p.We; char* inner = p.inner;
    hipLaunchKernelGGL(expand_weights_s2d_kernel, dim3(da_grid(27 * 8 * Cin * Cout, 256, 512)), dim3(256), 0, st, w_tio, We, Cin, Cout);
    DA_LAUNCH_CHECK();
    const DaS2dFuse f = {D, H, W};
    ConvGemm c = {}; c.in1 = in; c.C1 = 8 * Cin; c.w_tio = We; c.bias = bias; c.out1 = out; c.Cs1 = Cout; c.N = N; c.D = p.Dq; c.H = p.Hq; c.W = p.Wq; c.Cout = Cout; c.slope = slope;
    c.ws = inner; c.ws_bytes = p.inner_bytes; c.st = st; c.s2d_cin = Cin; c.s2f = &f; c.act_bf16 = act_bf16;
    return da_conv3_mfma_fwd(c);
}

int da_conv3_s2_dgrad(const float* dy, const float* w_tio, float* dx, int Cin, int N, int D, int H, int W, int Cout,
                      void* ws, size_t ws_bytes, hipStream_t st, int act_bf16) {
    if (act_bf16 && da_matrix_mode() != 1) return DA_ERR_UNSUPPORTED;
    if (s2_native(Cin, Cout, N, D, H, W)) return da_conv3_s2n_dgrad(dy, w_tio, dx, Cin, N, D, H, W, Cout, ws, ws_bytes, st);
    // the tap-masked kernels stage their input, here dY, in 16-channel chunks: Cout = 8, 24, ... goes back to the caller (da_conv3d_k3_dgrad: the direct kernel)
    if (Cout % 16 != 0) return DA_ERR_UNSUPPORTED;
    const S2Plan p = s2_plan(N, D, H, W, Cin, Cout, ws);
    if (ws_bytes < da_conv3_s2_ws_bytes(N, D, H, W, Cin, Cout)) return DA_ERR_WS_SMALL;
    float* We = p.We; char* inner = p.inner;
    hipLaunchKernelGGL(expand_weights_s2d_kernel, dim3(da_grid(27 * 8 * Cin * Cout, 256, 512)), dim3(256), 0, st, w_tio, We, Cin, Cout);
    DA_LAUNCH_CHECK();
    // dS = conv(dY, flip/transpose(W')) : logical Cin = Cout, logical Cout = 8*Cin, stored to dX through the inverse view
    const DaS2dFuse f = {D, H, W};
    ConvGemm c = {}; c.in1 = dy; c.C1 = Cout; c.w_tio = We; c.flipped_tr = 1; c.out1 = dx; c.Cs1 = 8 * Cin; c.N = N; c.D = p.Dq; c.H = p.Hq; c.W = p.Wq; c.Cout = 8 * Cin; c.slope = -1.f;
    c.ws = inner; c.ws_bytes = p.inner_bytes; c.st = st; c.s2d_cin = Cin; c.s2f = &f; c.act_bf16 = act_bf16;
    return da_conv3_mfma_fwd(c);
}

int da_conv3_s2_wgrad(const float* in, int Cin, const float* dy, float* dw_tio, int N, int D, int H, int W, int Cout,
                      void* ws, size_t ws_bytes, hipStream_t st, int act_bf16) {
    if (act_bf16 && da_matrix_mode() != 1) return DA_ERR_UNSUPPORTED;
    if (s2_native(Cin, Cout, N, D, H, W)) return da_conv3_s2n_wgrad(in, Cin, dy, dw_tio, N, D, H, W, Cout, ws, ws_bytes, st);
    const S2Plan p = s2_plan(N, D, H, W, Cin, Cout, ws);
    if (ws_bytes < da_conv3_s2_ws_bytes(N, D, H, W, Cin, Cout)) return DA_ERR_WS_SMALL;
    float* dWe = p.dWe; char* inner = p.inner;
    const DaS2dFuse f = {D, H, W};
    ConvWgrad c = {}; c.in1 = in; c.C1 = 8 * Cin; c.dy = dy; c.dw_tio = dWe; c.N = N; c.D = p.Dq; c.H = p.Hq; c.W = p.Wq; c.Cout = Cout; c.stride = 1;
    c.ws = inner; c.ws_bytes = p.inner_bytes; c.st = st; c.s2d_cin = Cin; c.s2f = &f; c.act_bf16 = act_bf16;
    int rc = da_conv3_mfma_wgrad(c);
    if (rc) return rc;
    hipLaunchKernelGGL(extract_wgrad_s2d_kernel, dim3(da_grid(27 * Cin * Cout, 256, 512)), dim3(256), 0, st, dWe, dw_tio, Cin, Cout);
    DA_LAUNCH_CHECK();
    return 0;
}
