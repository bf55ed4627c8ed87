// AdaptiveAvgPool2d(1) of a zero-padded 3x3 convolution (reference modules/transform/channelAligner.py:19-22, 30-31, 35-36) on
// gfx950, without the convolution's output.  The mean over all output positions is linear in the input: for tap (di, dj) the
// sum over the output positions of the shifted input is the channel's total T, minus the border row the tap never reaches
// (di = 0: the last row, 1: none, 2: the first row), minus the border column (the same rule in dj), plus the corner both took
// out.  Nine numbers per (image, channel) -- the total, four border sums, four corners -- and a Cout x (Cin * 9) product give
//     out[b][o] = bias[o] + (1 / (H W)) * sum_c sum_tap w[o][c][tap] * S_c(tap)
// exactly; H = 1 and W = 1 included (a border then is the whole map, and the inclusion-exclusion still holds).
//
// Three launches on NHWC fp32 with a channel stride:
//   1. ph_partial_kernel: the map is read once, 16 bytes per lane along the channel axis.  A workgroup owns a chunk of P
//      consecutive pixels of one image, P a function of H * W alone (ph_chunk_pixels), so the sums of an image never depend on
//      the batch it is in.  A lane adds every G-th pixel of the chunk (G = 256 / (Cin / 4) pixel groups) into five fp32
//      accumulators -- runs of at most P / G <= 1024 terms -- and the G groups are added in ascending order through LDS.
//   2. ph_reduce_kernel: the chunks' partial sums are added in fp64 in a fixed order (16 interleaved chains per value, then
//      those in ascending order) and rounded once to sums[B][9][Cin]; the four corners are copied from the map.
//   3. ph_head_kernel: S_c(tap) and the product in fp64, a fixed tree over the channels, one rounding to fp32 at the end.
// No floating-point atomics; every partial sum goes through scratch with plain vector stores; two calls give the same bits.
// Channels Cin <= c < cs are never loaded.  Supported: Cin a multiple of 4 in [4, 1024], Cout in [1, 65535], cs a multiple
// of 4, x and ws 16-byte aligned, B <= 65535, H * W <= 2^30.  Design and measurements: DESIGN.md 5.5.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int PH_T = 256;        // threads of every workgroup here
constexpr int PH_SUMS = 9;       // total, first row, last row, first column, last column, corners (0,0) (0,W-1) (H-1,0) (H-1,W-1)
constexpr int PH_ACC = 5;        // of which accumulated: the corners are single values
constexpr int PH_LANES = 16;     // interleaved fp64 chains per value in ph_reduce_kernel

// pixels per workgroup of ph_partial_kernel: about a thousand chunks per image, between 64 and 4096 pixels each
int ph_chunk_pixels(int64_t HW)
{
    int64_t p = (HW + 1023) / 1024;
    p = (p + 63) / 64 * 64;
    return (int)(p < 64 ? 64 : (p > 4096 ? 4096 : p));
}

__global__ __launch_bounds__(PH_T) void ph_partial_kernel(const float* __restrict__ x, int cs, int H, int W, int C, int P, int nch,
                                                          float* __restrict__ part)
{
    __shared__ f32x4 red[PH_ACC][PH_T];
    const int nv = C >> 2, G = PH_T / nv;
    const int tid = threadIdx.x, g = tid / nv, v = tid - g * nv;
    const int b = blockIdx.y, ch = blockIdx.x;
    const int HW = H * W;
    const int p0 = ch * P, pe = p0 + P < HW ? p0 + P : HW;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 tot = z, r0 = z, rl = z, c0 = z, cl = z;
    if (g < G) {
        const float* xb = x + (size_t)b * HW * cs + v * 4;
        int p = p0 + g;
        int row = p / W, col = p - row * W;
        auto ld = [&](int q) { return *reinterpret_cast<const f32x4*>(xb + (size_t)q * cs); };
        auto add = [&](const f32x4 val) {  // the pixel at (row, col), then on to the lane's next one
            tot += val;
            if (row == 0) r0 += val;
            if (row == H - 1) rl += val;
            if (col == 0) c0 += val;
            if (col == W - 1) cl += val;
            col += G;
            if (col >= W) {
                const int q = col / W;
                row += q;
                col -= q * W;
            }
        };
        for (; p + 3 * G < pe; p += 4 * G) {  // four loads in flight per lane
            const f32x4 a0 = ld(p), a1 = ld(p + G), a2 = ld(p + 2 * G), a3 = ld(p + 3 * G);
            add(a0);
            add(a1);
            add(a2);
            add(a3);
        }
        for (; p < pe; p += G) add(ld(p));
    }
    red[0][tid] = tot;
    red[1][tid] = r0;
    red[2][tid] = rl;
    red[3][tid] = c0;
    red[4][tid] = cl;
    __syncthreads();
    if (tid < nv) {
        float* dst = part + ((size_t)b * nch + ch) * PH_ACC * C + tid * 4;
#pragma unroll
        for (int k = 0; k < PH_ACC; ++k) {
            f32x4 s = red[k][tid];
            for (int j = 1; j < G; ++j) s += red[k][j * nv + tid];
            *reinterpret_cast<f32x4*>(dst + (size_t)k * C) = s;
        }
    }
}

__global__ __launch_bounds__(PH_T) void ph_reduce_kernel(const float* __restrict__ x, int cs, int H, int W, int C, int nch,
                                                         const float* __restrict__ part, float* __restrict__ sums)
{
    __shared__ double red[PH_LANES][PH_T / PH_LANES];
    const int tid = threadIdx.x, el = tid % (PH_T / PH_LANES), j = tid / (PH_T / PH_LANES);
    const int e = blockIdx.x * (PH_T / PH_LANES) + el, b = blockIdx.y;
    const bool live = e < PH_SUMS * C;
    const int k = live ? e / C : 0, c = live ? e - k * C : 0;
    double acc = 0.0;
    if (live && k < PH_ACC) {
        const float* pp = part + ((size_t)b * nch * PH_ACC + k) * C + c;
        for (int i = j; i < nch; i += PH_LANES) acc += (double)pp[(size_t)i * PH_ACC * C];
    }
    red[j][el] = acc;
    __syncthreads();
    if (!live || j) return;
    float out;
    if (k < PH_ACC) {
        double s = red[0][el];
        for (int i = 1; i < PH_LANES; ++i) s += red[i][el];
        out = (float)s;
    } else {
        const int row = k < 7 ? 0 : H - 1, col = (k & 1) ? 0 : W - 1;  // k = 5 .. 8: (0,0) (0,W-1) (H-1,0) (H-1,W-1)
        out = x[((size_t)b * H * W + (size_t)row * W + col) * cs + c];
    }
    sums[((size_t)b * PH_SUMS + k) * C + c] = out;
}

__global__ __launch_bounds__(PH_T) void ph_head_kernel(const float* __restrict__ sums, int C, const float* __restrict__ w,
                                                       const float* __restrict__ bias, int Cout, double hw,
                                                       float* __restrict__ out)
{
    __shared__ double red[PH_T];
    const int o = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* sb = sums + (size_t)b * PH_SUMS * C;
    double acc = 0.0;
    for (int c = tid; c < C; c += PH_T) {
        const double T = sb[c];
        // what tap index 0 / 1 / 2 never reaches: the last row (column), nothing, the first row (column)
        const double R[3] = {(double)sb[2 * C + c], 0.0, (double)sb[C + c]};
        const double L[3] = {(double)sb[4 * C + c], 0.0, (double)sb[3 * C + c]};
        const double K[3][3] = {{(double)sb[8 * C + c], 0.0, (double)sb[7 * C + c]},
                                {0.0, 0.0, 0.0},
                                {(double)sb[6 * C + c], 0.0, (double)sb[5 * C + c]}};
        const float* wp = w + ((size_t)o * C + c) * 9;
#pragma unroll
        for (int di = 0; di < 3; ++di)
#pragma unroll
            for (int dj = 0; dj < 3; ++dj) acc += (double)wp[di * 3 + dj] * (T - R[di] - L[dj] + K[di][dj]);
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = PH_T / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) out[(size_t)b * Cout + o] = (float)((double)bias[o] + red[0] / hw);
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int64_t pooled_conv3x3_ws_floats(int B, int H, int W, int Cin)
{
    if (B < 1 || H < 1 || W < 1 || Cin < 4 || Cin > 1024 || Cin % 4 || B > 65535 || (int64_t)H * W > (1 << 30)) return RGBD_EINVAL;
    const int64_t HW = (int64_t)H * W, P = ph_chunk_pixels(HW), nch = (HW + P - 1) / P;
    return (int64_t)B * Cin * (PH_SUMS + PH_ACC * nch);
}

int launch_pooled_conv3x3(const float* x, int cs, int B, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                          float* out, float* ws, hipStream_t s)
{
    if (!x || !w || !bias || !out || !ws || Cout < 1 || Cout > 65535 || pooled_conv3x3_ws_floats(B, H, W, Cin) <= 0 || cs < Cin ||
        cs % 4 || !al16(x) || !al16(ws))
        return RGBD_EINVAL;
    const int HW = H * W, P = ph_chunk_pixels(HW), nch = (HW + P - 1) / P;
    float* sums = ws;
    float* part = ws + (size_t)B * PH_SUMS * Cin;
    hipLaunchKernelGGL(ph_partial_kernel, dim3((unsigned)nch, (unsigned)B), dim3(PH_T), 0, s, x, cs, H, W, Cin, P, nch, part);
    hipLaunchKernelGGL(ph_reduce_kernel, dim3((unsigned)((PH_SUMS * Cin + PH_T / PH_LANES - 1) / (PH_T / PH_LANES)), (unsigned)B),
                       dim3(PH_T), 0, s, x, cs, H, W, Cin, nch, (const float*)part, sums);
    hipLaunchKernelGGL(ph_head_kernel, dim3((unsigned)Cout, (unsigned)B), dim3(PH_T), 0, s, (const float*)sums, Cin, w, bias, Cout,
                       (double)HW, out);
    HIP_TRY(hipGetLastError());
    return RGBD_OK;
}

extern "C" int64_t rgbd_pooled_conv3x3_ws_floats(int32_t B, int32_t H, int32_t W, int32_t Cin)
{
    return pooled_conv3x3_ws_floats(B, H, W, Cin);
}

extern "C" int rgbd_pooled_conv3x3(const float* x, int32_t cs, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w,
                                   const float* bias, int32_t Cout, float* out, float* ws, void* stream)
{
    return launch_pooled_conv3x3(x, cs, B, H, W, Cin, w, bias, Cout, out, ws, (hipStream_t)stream);
}
