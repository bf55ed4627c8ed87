// The four-layer 1x1 stack of MLIC++'s EntropyParametersMLIC (modules/transform/entropy.py:31-53) as ONE launch on the fp32
// MFMA of gfx950:
//
//     out[p] = W3 g(W2 g(W1 g(W0 x[p] + b0) + b1) + b2) + b3,    widths in_dim -> 320 -> 256 -> 128 -> out_dim,
//     g = nn.GELU() in its erf form, 0.5 v (1 + erf(v / sqrt 2))
//
// per pixel p of NHWC tensors.  A workgroup of four waves owns a tile of 16 pixels.  It stages their input channels in LDS once
// -- from up to six channel segments, so that the codec's torch.cat([...], dim=1) is never formed -- and then runs the four
// layers back to back: the three intermediates live in LDS and never reach HBM, only the weights stream (from L2 after the
// first tile), layer by layer, as MFMA lane fragments (pixel_mlp4_pack).  A layer's 16-channel output tiles are dealt to the
// waves round robin; a wave keeps all of its tiles in accumulators while it walks the reduction once.
//
// Arithmetic: every output element of every layer is ONE fp32 chain.  It STARTS FROM THE BIAS (the accumulator is initialised
// with b[co]; there is no other place where a bias enters), then takes the products in increasing k, four at a time: step s of
// v_mfma_f32_16x16x4_f32 adds the channels 4s, 4s + 1, 4s + 2, 4s + 3.  To that end LDS holds channel 16c + 4j + g at position
// 16c + 4g + j (lane group g reads its operands of the four steps j of a 16-channel chunk as one 16-byte word), and the weight
// fragments are packed to match.  A chain never leaves its wave and depends on nothing but the pixel's own input: the bits of
// a pixel's result do not depend on the batch size, the map size, the pixel's place in its tile, the checkerboard half asked
// for, or on how the input channels are cut into segments.  Channels that are zero padding add exact zeros.
//
// parity: -1 every pixel; 0 the anchor pixels ((row + col) odd, utils/ckbd.py:37-48, as ckbd_part_kernel in entropy.hip takes
// them), 1 the others.  Under 0 / 1 the tiles are cut from the list of selected pixels, and only those are stored.
#include <math.h>
#include <string.h>

#include <mutex>

#include "../../include/rgbd_amd.h"
#include "engine_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int kP = 16;                         // pixels per workgroup (one MFMA column block)
constexpr int kWaves = 4;
constexpr int kH1 = 320, kH2 = 256, kH3 = 128;  // entropy.py:35-41
constexpr int kMaxIn = 960, kMaxOut = 128, kMaxSeg = PIXEL_MLP_MAX_SEGS;

// LDS rows are C + 4 floats: an odd multiple of four words, so that the 16 lanes of a group, which read the same 16-byte
// column of 16 consecutive rows, hit 16 different 16-byte slots of the 256-byte bank row (as gdn.hip)
__host__ __device__ constexpr int row_of(int c) { return c + 4; }

struct Layer {
    const float* w;     // fragments [cout / 16][cin / 16][64 lanes][4]
    const float* bias;  // [cout]
};

// One layer for the tile: in [kP][SI] (LDS, permuted positions) -> GELU -> out [kP][SO] (LDS, permuted), or, LAST, the plain
// result as 16-byte stores to y.  MAXT: the most output tiles a wave can own (ceil(cout / 16 / kWaves)).
template <int MAXT, bool LAST>
__device__ __forceinline__ void layer_run(const float* __restrict__ in, int SI, int cin, const Layer l, int cout, float* __restrict__ out,
                                          int SO, float* __restrict__ yrow, bool store)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, px = lane & 15;
    const int nch = cin >> 4, ntile = cout >> 4;
    const int nt = (ntile - wave + kWaves - 1) / kWaves;  // tiles wave, wave + kWaves, ... of this wave
    f32x4 acc[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t < nt) acc[t] = *(const f32x4*)(l.bias + 16 * (wave + kWaves * t) + 4 * g);  // the chain starts from the bias
    }
    const f32x4* wf = (const f32x4*)l.w + lane;
    const float* xr = in + px * SI + 4 * g;
    f32x4 av[MAXT], an[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        av[t] = an[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t < nt) av[t] = wf[(size_t)(wave + kWaves * t) * nch * 64];
    }
    for (int c = 0; c < nch; ++c) {
        const int cn = c + 1 < nch ? c + 1 : c;  // the next chunk's fragments are fetched under this chunk's MFMAs
#pragma unroll
        for (int t = 0; t < MAXT; ++t)
            if (t < nt) an[t] = wf[((size_t)(wave + kWaves * t) * nch + cn) * 64];
        const f32x4 xv = *(const f32x4*)(xr + 16 * c);
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            if (t < nt) {
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t].x, xv.x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t].y, xv.y, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t].z, xv.z, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t].w, xv.w, acc[t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < MAXT; ++t) av[t] = an[t];
    }
    // lane (g, px) holds channels 16 tile + 4 g + r, r = 0..3, of its pixel
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        if (t < nt) {
            const int c0 = 16 * (wave + kWaves * t);
            if (LAST) {
                if (store) *(f32x4*)(yrow + c0 + 4 * g) = acc[t];
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[t][r];
                    out[px * SO + c0 + 4 * r + g] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
                }
            }
        }
    }
}

struct Args {
    const float* seg[kMaxSeg];
    int seg_cs[kMaxSeg];
    int seg_end[kMaxSeg];  // first channel behind segment s in the concatenation
    int nseg;
    Layer l[4];
    int in_dim, out_dim;
    int H, W, parity;
    long nsel;  // selected pixels of the call
    float* y;
    int ycs;
};

__global__ __launch_bounds__(64 * kWaves) void pixel_mlp4_kernel(Args a)
{
    extern __shared__ float lds[];
    // bufA: the input, later h3; bufB: h1; bufC: h2
    const int SA = row_of(a.in_dim > kH3 ? a.in_dim : kH3), SB = row_of(kH1), SC = row_of(kH2);
    float* bufA = lds;
    float* bufB = bufA + kP * SA;
    float* bufC = bufB + kP * SB;
    const long sel0 = (long)blockIdx.x * kP;

    // where selected pixel number `sel` lies in the tensors
    const auto pixel_of = [&](long sel) -> long {
        if (a.parity < 0) return sel;
        const int w2 = a.W >> 1;
        const int k = (int)(sel % w2);
        const long t = sel / w2;
        const int row = (int)(t % a.H);
        const int col = 2 * k + ((a.parity == 0) ? (1 - (row & 1)) : (row & 1));
        return t * a.W + col;  // t = b * H + row
    };

    const int c4n = a.in_dim >> 2;
    for (int i = threadIdx.x; i < kP * c4n; i += 64 * kWaves) {
        const int p = i / c4n, c4 = i - p * c4n, c = 4 * c4;
        const long sel = sel0 + p;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (sel < a.nsel) {
            int s = 0;
            while (c >= a.seg_end[s]) ++s;
            const int first = s ? a.seg_end[s - 1] : 0;
            v = *(const f32x4*)(a.seg[s] + pixel_of(sel) * a.seg_cs[s] + (c - first));
        }
        // channels 16 ch + 4 q + j, j = 0..3  ->  positions 16 ch + 4 j + q
        float* d = bufA + p * SA + (c & ~15) + ((c >> 2) & 3);
        d[0] = v.x;
        d[4] = v.y;
        d[8] = v.z;
        d[12] = v.w;
    }
    __syncthreads();
    layer_run<kH1 / 16 / kWaves, false>(bufA, SA, a.in_dim, a.l[0], kH1, bufB, SB, nullptr, false);
    __syncthreads();
    layer_run<kH2 / 16 / kWaves, false>(bufB, SB, kH1, a.l[1], kH2, bufC, SC, nullptr, false);
    __syncthreads();
    layer_run<kH3 / 16 / kWaves, false>(bufC, SC, kH2, a.l[2], kH3, bufA, SA, nullptr, false);
    __syncthreads();
    const long sel = sel0 + (threadIdx.x & 15);
    const bool store = sel < a.nsel;
    float* yrow = store ? a.y + pixel_of(sel) * a.ycs : nullptr;
    layer_run<kMaxOut / 16 / kWaves, true>(bufA, SA, kH3, a.l[3], a.out_dim, nullptr, 0, yrow, store);
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

int pixel_mlp4_pack(const float* w, int cout, int cin, float* out)
{
    if (!w || !out || cout < 16 || cin < 16 || cout % 16 || cin % 16) return RGBD_EINVAL;
    const int nch = cin / 16;
    for (int t = 0; t < cout / 16; ++t)
        for (int c = 0; c < nch; ++c)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j)
                    out[(((size_t)t * nch + c) * 64 + lane) * 4 + j] = w[(size_t)(16 * t + (lane & 15)) * cin + 16 * c + 4 * j + (lane >> 4)];
    return RGBD_OK;
}

int launch_pixel_mlp4(const PixelMlp4& d, hipStream_t s)
{
    if (d.nseg < 1 || d.nseg > kMaxSeg || d.B < 1 || d.H < 1 || d.W < 1 || (long)d.B * d.H * d.W > ((long)1 << 30) || d.parity < -1 ||
        d.parity > 1 || (d.parity >= 0 && (d.W & 1)) || !d.y || !al16(d.y) || d.out_dim < 16 || d.out_dim > kMaxOut || d.out_dim % 16 ||
        d.ycs < d.out_dim || d.ycs % 4)
        return RGBD_EINVAL;
    Args a{};
    int in_dim = 0;
    for (int i = 0; i < d.nseg; ++i) {
        if (!d.seg[i] || !al16(d.seg[i]) || d.seg_c[i] < 16 || d.seg_c[i] % 16 || d.seg_cs[i] < d.seg_c[i] || d.seg_cs[i] % 4 ||
            d.seg[i] == d.y)
            return RGBD_EINVAL;
        in_dim += d.seg_c[i];
        if (in_dim > kMaxIn) return RGBD_EINVAL;
        a.seg[i] = d.seg[i];
        a.seg_cs[i] = d.seg_cs[i];
        a.seg_end[i] = in_dim;
    }
    for (int i = d.nseg; i < kMaxSeg; ++i) a.seg_end[i] = in_dim;
    for (int k = 0; k < 4; ++k) {
        if (!d.w[k] || !d.bias[k] || !al16(d.w[k]) || !al16(d.bias[k])) return RGBD_EINVAL;
        a.l[k] = {d.w[k], d.bias[k]};
    }
    a.nseg = d.nseg;
    a.in_dim = in_dim;
    a.out_dim = d.out_dim;
    a.H = d.H;
    a.W = d.W;
    a.parity = d.parity;
    a.nsel = (long)d.B * d.H * d.W / (d.parity >= 0 ? 2 : 1);
    a.y = d.y;
    a.ycs = d.ycs;
    static std::once_flag once;
    static hipError_t attr = hipSuccess;
    constexpr int kMaxLds = kP * (row_of(kMaxIn) + row_of(kH1) + row_of(kH2)) * (int)sizeof(float);
    std::call_once(once, [] {
        attr = hipFuncSetAttribute((const void*)pixel_mlp4_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
    });
    HIP_TRY(attr);
    const size_t lds = (size_t)kP * (row_of(std::max(in_dim, kH3)) + row_of(kH1) + row_of(kH2)) * sizeof(float);
    const long blocks = (a.nsel + kP - 1) / kP;
    hipLaunchKernelGGL(pixel_mlp4_kernel, dim3((unsigned)blocks), dim3(64 * kWaves), lds, s, a);
    HIP_TRY(hipGetLastError());
    return RGBD_OK;
}

extern "C" int rgbd_pixel_mlp4_pack(const float* w, int32_t cout, int32_t cin, float* out) { return pixel_mlp4_pack(w, cout, cin, out); }

extern "C" int rgbd_pixel_mlp4(const float* const* seg_dev, const int32_t* seg_channels, const int32_t* seg_stride, int32_t n_seg,
                               const float* const* w_dev, const float* const* bias_dev, int32_t out_dim, int32_t B, int32_t H,
                               int32_t W, int32_t parity, float* out_dev, int32_t out_stride, void* stream)
{
    if (!seg_dev || !seg_channels || !seg_stride || !w_dev || !bias_dev || n_seg < 1 || n_seg > kMaxSeg) return RGBD_EINVAL;
    PixelMlp4 d{};
    for (int i = 0; i < n_seg; ++i) {
        d.seg[i] = seg_dev[i];
        d.seg_c[i] = seg_channels[i];
        d.seg_cs[i] = seg_stride[i];
    }
    d.nseg = n_seg;
    for (int k = 0; k < 4; ++k) {
        d.w[k] = w_dev[k];
        d.bias[k] = bias_dev[k];
    }
    d.out_dim = out_dim;
    d.B = B;
    d.H = H;
    d.W = W;
    d.parity = parity;
    d.y = out_dev;
    d.ycs = out_stride;
    return launch_pixel_mlp4(d, (hipStream_t)stream);
}
