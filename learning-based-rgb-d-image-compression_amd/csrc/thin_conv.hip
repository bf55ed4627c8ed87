// The two 3x3 convolutions of Feature_encoder / Feature_decoder (reference models/elic_master.py:15-53) that have an image on
// one side and a 64-channel map on the other, on gfx950: conv3x3(1|3 -> 64), which reads the image, and
// ConvTranspose2d(64 -> 1|3, 3, stride 1, pad 1), which writes it (a convolution with the channel axes exchanged and the taps
// turned by 180 degrees: the caller hands the weight over in convolution orientation).  On the MFMA implicit-GEMM path either
// one pads its thin side to 16 channels; here each costs one pass over the 64-channel map and nothing else.  Plain fp32 FMA
// (fmaf chains in a fixed order), no MFMA, no atomics, no workspace; stride 1, zero padding 1, no activation.
//
//   thin_in  (x [B,Cin,H,W] planes, Cin 1..4 -> y NHWC, Cout a multiple of 4 up to 64, channel stride ycs):
//     a workgroup owns TI_TH x TI_TW output pixels of one image.  The few input planes of that tile, with their halo, go
//     to LDS once (zeros outside the image), the whole weight tensor too.  Lane = (pixel slot, output-channel quad): the
//     Cout / 4 lanes of a pixel are neighbours, so a wave stores 16 bytes per lane over a contiguous run (four pixels x 256
//     bytes at Cout = ycs = 64).  A lane keeps the 36 * Cin weights of its quad in registers and walks the tile's pixels in
//     steps of 256 / (Cout / 4).  Per output: bias, then channel by channel, tap by tap.  Channels [Cout, ycs) are not written.
//   thin_out (x NHWC, Cin a multiple of 4 up to 64, channel stride xcs -> y [B,Cout,H,W] planes, Cout 1..4):
//     a workgroup owns TO_TH x TO_TW output pixels.  Its input tile with halo goes to LDS once, 16 bytes per lane along the
//     channel axis (contiguous runs of TO_TW + 2 pixels), zeros outside the image; channels [Cin, xcs) are never loaded.
//     Lane = (pixel slot, input-channel quad): a lane reduces its four channels over the nine taps for every output channel
//     (weights of its quad in registers), and the quads of a pixel -- NQ = Cin / 4 rounded up to a power of two, lanes of one
//     wave -- are combined by an exclusive-or butterfly (16, 8, 4, 2, 1 apart: a fixed tree), then the bias is added.
// Every output is a function of its own image alone and of nothing the launch geometry decides: two calls give the same bits,
// and an image gives the same bits alone or inside a batch.  Design and measurements: DESIGN.md 5.6.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TC_T = 256;                  // threads of both kernels
constexpr int TI_TH = 4, TI_TW = 64;       // thin_in: output pixels per workgroup
constexpr int TO_TH = 8, TO_TW = 16;       // thin_out
constexpr int TC_MAXC = 64;                // the wide side's channel limit

template <int CIN>
__global__ __launch_bounds__(TC_T) void thin_in_kernel(const float* __restrict__ x, int H, int W, const float* __restrict__ w,
                                                       const float* __restrict__ bias, int Cout, float* __restrict__ y, int ycs,
                                                       int ntx)
{
    __shared__ float tile[CIN][TI_TH + 2][TI_TW + 2];
    __shared__ float wl[TC_MAXC * CIN * 9];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int r0 = ty * TI_TH, c0 = tx * TI_TW;
    const size_t HW = (size_t)H * W;
    const float* xb = x + (size_t)b * CIN * HW;
    for (int i = tid; i < CIN * (TI_TH + 2) * (TI_TW + 2); i += TC_T) {
        const int ci = i / ((TI_TH + 2) * (TI_TW + 2)), rem = i - ci * ((TI_TH + 2) * (TI_TW + 2));
        const int rr = rem / (TI_TW + 2), cc = rem - rr * (TI_TW + 2);
        const int r = r0 + rr - 1, c = c0 + cc - 1;
        tile[ci][rr][cc] = (r >= 0 && r < H && c >= 0 && c < W) ? xb[(size_t)ci * HW + (size_t)r * W + c] : 0.f;
    }
    for (int i = tid; i < Cout * CIN * 9; i += TC_T) wl[i] = w[i];
    __syncthreads();
    const int nq = Cout >> 2, G = TC_T / nq;
    const int g = tid / nq, q = tid - g * nq;
    if (g >= G) return;
    float wr[4][CIN * 9];
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < CIN * 9; ++k) wr[j][k] = wl[(q * 4 + j) * CIN * 9 + k];
        if (bias) bv[j] = bias[q * 4 + j];
    }
    float* yb = y + (size_t)b * HW * ycs + q * 4;
    for (int i = g; i < TI_TH * TI_TW; i += G) {
        const int rr = i / TI_TW, cc = i - rr * TI_TW;
        const int r = r0 + rr, c = c0 + cc;
        if (r >= H || c >= W) continue;
        f32x4 acc = bv;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float v = tile[ci][rr + ky][cc + kx];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = fmaf(wr[j][ci * 9 + ky * 3 + kx], v, acc[j]);
                }
        *reinterpret_cast<f32x4*>(yb + ((size_t)r * W + c) * ycs) = acc;
    }
}

template <int COUT>
__global__ __launch_bounds__(TC_T) void thin_out_kernel(const float* __restrict__ x, int xcs, int H, int W, int Cin,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ y, int ntx, int NQ)
{
    __shared__ f32x4 tile[(TO_TH + 2) * (TO_TW + 2) * (TC_MAXC / 4)];
    __shared__ float wl[COUT * TC_MAXC * 9];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int r0 = ty * TO_TH, c0 = tx * TO_TW;
    const int nq = Cin >> 2;
    const size_t HW = (size_t)H * W;
    const float* xb = x + (size_t)b * HW * xcs;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < (TO_TH + 2) * (TO_TW + 2) * nq; i += TC_T) {
        const int px = i / nq, v = i - px * nq;
        const int rr = px / (TO_TW + 2), cc = px - rr * (TO_TW + 2);
        const int r = r0 + rr - 1, c = c0 + cc - 1;
        tile[i] = (r >= 0 && r < H && c >= 0 && c < W) ? *reinterpret_cast<const f32x4*>(xb + ((size_t)r * W + c) * xcs + v * 4) : z;
    }
    for (int i = tid; i < COUT * Cin * 9; i += TC_T) wl[i] = w[i];
    __syncthreads();
    const int G = TC_T / NQ;
    const int g = tid / NQ, q = tid - g * NQ;
    const bool live = q < nq;  // (lanes of the power-of-two padding add zeros)
    f32x4 wr[COUT][9];
#pragma unroll
    for (int o = 0; o < COUT; ++o)
#pragma unroll
        for (int k = 0; k < 9; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) wr[o][k][j] = live ? wl[(o * Cin + q * 4 + j) * 9 + k] : 0.f;
    float* yb = y + (size_t)b * COUT * HW;
    for (int i = g; i < TO_TH * TO_TW; i += G) {  // (G divides the tile or exceeds it: the lanes of a wave leave together)
        const int rr = i / TO_TW, cc = i - rr * TO_TW;
        float acc[COUT];
#pragma unroll
        for (int o = 0; o < COUT; ++o) acc[o] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const f32x4 v = live ? tile[((rr + ky) * (TO_TW + 2) + cc + kx) * nq + q] : z;
#pragma unroll
                for (int o = 0; o < COUT; ++o)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[o] = fmaf(wr[o][ky * 3 + kx][j], v[j], acc[o]);
            }
        for (int m = NQ >> 1; m >= 1; m >>= 1)
#pragma unroll
            for (int o = 0; o < COUT; ++o) acc[o] += __shfl_xor(acc[o], m);
        const int r = r0 + rr, c = c0 + cc;
        if (r < H && c < W) {  // every lane of the pixel holds the sums: lane o (modulo NQ) stores output channel o
#pragma unroll
            for (int o = 0; o < COUT; ++o)
                if ((o & (NQ - 1)) == q) yb[(size_t)o * HW + (size_t)r * W + c] = acc[o] + (bias ? bias[o] : 0.f);
        }
    }
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

bool map_ok(int B, int H, int W) { return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 30); }

}  // namespace

int launch_conv3x3_thin_in(const float* x, int B, int Cin, int H, int W, const float* w, const float* bias, int Cout, float* y,
                           int ycs, hipStream_t s)
{
    if (!x || !w || !y || !map_ok(B, H, W) || Cin < 1 || Cin > 4 || Cout < 4 || Cout > TC_MAXC || Cout % 4 || ycs < Cout || ycs % 4 ||
        !al16(y))
        return RGBD_EINVAL;
    const int ntx = (W + TI_TW - 1) / TI_TW, nty = (H + TI_TH - 1) / TI_TH;
    const dim3 grid((unsigned)(ntx * nty), (unsigned)B), block(TC_T);
    switch (Cin) {
    case 1: hipLaunchKernelGGL(thin_in_kernel<1>, grid, block, 0, s, x, H, W, w, bias, Cout, y, ycs, ntx); break;
    case 2: hipLaunchKernelGGL(thin_in_kernel<2>, grid, block, 0, s, x, H, W, w, bias, Cout, y, ycs, ntx); break;
    case 3: hipLaunchKernelGGL(thin_in_kernel<3>, grid, block, 0, s, x, H, W, w, bias, Cout, y, ycs, ntx); break;
    default: hipLaunchKernelGGL(thin_in_kernel<4>, grid, block, 0, s, x, H, W, w, bias, Cout, y, ycs, ntx); break;
    }
    HIP_TRY(hipGetLastError());
    return RGBD_OK;
}

int launch_conv3x3_thin_out(const float* x, int xcs, int B, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                            float* y, hipStream_t s)
{
    if (!x || !w || !y || !map_ok(B, H, W) || Cin < 4 || Cin > TC_MAXC || Cin % 4 || Cout < 1 || Cout > 4 || xcs < Cin || xcs % 4 ||
        !al16(x))
        return RGBD_EINVAL;
    int NQ = 1;
    while (NQ < Cin / 4) NQ <<= 1;
    const int ntx = (W + TO_TW - 1) / TO_TW, nty = (H + TO_TH - 1) / TO_TH;
    const dim3 grid((unsigned)(ntx * nty), (unsigned)B), block(TC_T);
    switch (Cout) {
    case 1: hipLaunchKernelGGL(thin_out_kernel<1>, grid, block, 0, s, x, xcs, H, W, Cin, w, bias, y, ntx, NQ); break;
    case 2: hipLaunchKernelGGL(thin_out_kernel<2>, grid, block, 0, s, x, xcs, H, W, Cin, w, bias, y, ntx, NQ); break;
    case 3: hipLaunchKernelGGL(thin_out_kernel<3>, grid, block, 0, s, x, xcs, H, W, Cin, w, bias, y, ntx, NQ); break;
    default: hipLaunchKernelGGL(thin_out_kernel<4>, grid, block, 0, s, x, xcs, H, W, Cin, w, bias, y, ntx, NQ); break;
    }
    HIP_TRY(hipGetLastError());
    return RGBD_OK;
}

extern "C" int rgbd_conv3x3_thin_in(const float* x_nchw, int32_t B, int32_t Cin, int32_t H, int32_t W, const float* w,
                                    const float* bias, int32_t Cout, float* y_nhwc, int32_t ycs, void* stream)
{
    return launch_conv3x3_thin_in(x_nchw, B, Cin, H, W, w, bias, Cout, y_nhwc, ycs, (hipStream_t)stream);
}

extern "C" int rgbd_conv3x3_thin_out(const float* x_nhwc, int32_t xcs, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w,
                                     const float* bias, int32_t Cout, float* y_nchw, void* stream)
{
    return launch_conv3x3_thin_out(x_nhwc, xcs, B, H, W, Cin, w, bias, Cout, y_nchw, (hipStream_t)stream);
}
