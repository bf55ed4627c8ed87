// GDN / IGDN (CompressAI/compressai/layers/gdn.py:22-67) as one fused launch on the fp32 MFMA of gfx950:
//
//     out[p][i] = x[p][i] * f(beta[i] + sum_j gamma[i][j] * x[p][j]^2)  (+ res[p][i]),   f = 1 / sqrt (GDN) or sqrt (IGDN)
//
// on the engine's NHWC tensors (channel stride a multiple of 16, pad channels zero).  A workgroup stages a tile of P pixels
// of x in LDS once: the squares of the staged values are the B operand of the per-pixel C x C GEMM (A = gamma), the values
// themselves the multiplicand of the epilogue, so x is read from HBM once per launch.  `res` is the identity / skip branch
// that ResidualBlockWithStride / ResidualBlockUpsample (layers.py:97,125) add right after the (I)GDN.
//
// Arithmetic: every output element is ONE fp32 chain that starts from beta[i] and takes the products in the fixed order
// j = 16 g + 4 q + e (g ascending, then e = 0..3, then q = 0..3: the k order of v_mfma_f32_16x16x4_f32 with lane group q
// holding channels 4q..4q+3 of a 16-channel chunk), then a correctly rounded sqrtf, an IEEE 1.0f / s (GDN only), the
// multiply and the residual add: one rounding per step.  Nothing in that chain depends on the pixel tile, the batch size or
// the caller -- a chain never leaves its wave --, so every tile gives the same bits (rgbd_debug_force_gdn_tile is the test
// hook for that).
#include <math.h>
#include <string.h>

#include <mutex>

#include "../../include/rgbd_amd.h"
#include "engine_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int kGdnIT = 12;     // 16-channel output tiles a wave accumulates at once (12 = all of N = 192)
constexpr int kGdnMaxC = 512;  // LDS: 64 pixels x (512 + 4) floats = 129 KiB of the 160 KiB of a CU

// P pixels per workgroup and WS waves per 16 pixels, each with its own range of 16-channel output tiles (WS = 4 with P = 16:
// small grids, where a wave that walked all output tiles alone would be the whole launch time; WS = 1 otherwise); LDS row = cs + 4 floats (16 lanes
// reading one 16-byte column of 16 consecutive rows then hit 64 different banks: the row stride is an odd multiple of 4 words)
template <int P, int WS>
__global__ __launch_bounds__(P * 4 * WS) void gdn_kernel(GdnArgs a)
{
    extern __shared__ float xs[];
    const int cs = a.cs, LS = cs + 4, c4n = cs >> 2, NT = cs >> 4;
    const long pix0 = (long)blockIdx.x * P;
    for (int i = threadIdx.x; i < P * c4n; i += P * 4 * WS) {
        const int p = i / c4n, c4 = i - p * c4n;
        const long gp = pix0 + p;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (gp < a.npix) v = *(const f32x4*)(a.x + gp * a.xcs + 4 * c4);
        *(f32x4*)(xs + p * LS + 4 * c4) = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wv = wave / WS, part = wave % WS, q = lane >> 4;
    const float* xr = xs + (wv * 16 + (lane & 15)) * LS;
    const long gp = pix0 + wv * 16 + (lane & 15);
    const f32x4* gw = (const f32x4*)a.gamma + lane;
    const int per = (NT + WS - 1) / WS, it_end = min(NT, (part + 1) * per);
    for (int it0 = part * per; it0 < it_end; it0 += kGdnIT) {
        const int nt = min(kGdnIT, it_end - it0);
        f32x4 acc[kGdnIT];
#pragma unroll
        for (int t = 0; t < kGdnIT; ++t) {
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (t < nt) acc[t] = *(const f32x4*)(a.beta + 16 * (it0 + t) + 4 * q);  // the chain starts from beta
        }
        for (int g = 0; g < NT; ++g) {
            const f32x4 xv = *(const f32x4*)(xr + 16 * g + 4 * q);
            const float b0 = __fmul_rn(xv.x, xv.x), b1 = __fmul_rn(xv.y, xv.y), b2 = __fmul_rn(xv.z, xv.z), b3 = __fmul_rn(xv.w, xv.w);
#pragma unroll
            for (int t = 0; t < kGdnIT; ++t) {
                if (t < nt) {
                    const f32x4 av = gw[((size_t)(it0 + t) * NT + g) * 64];
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b0, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b1, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, b2, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, b3, acc[t], 0, 0, 0);
                }
            }
        }
        // lane (q, pixel): channels 16 t + 4 q .. + 3 of its pixel
        if (gp < a.npix) {
#pragma unroll
            for (int t = 0; t < kGdnIT; ++t) {
                if (t < nt) {
                    const int c0 = 16 * (it0 + t) + 4 * q;
                    const f32x4 xv = *(const f32x4*)(xr + c0);
                    f32x4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float f = sqrtf(acc[t][r]);       // correctly rounded
                        if (!a.inverse) f = 1.0f / f;     // IEEE divide (torch.rsqrt on the CPU: sqrt, then divide)
                        o[r] = __fmul_rn(xv[r], f);
                    }
                    if (a.res) {
                        const f32x4 rv = *(const f32x4*)(a.res + gp * a.rcs + c0);
#pragma unroll
                        for (int r = 0; r < 4; ++r) o[r] = __fadd_rn(o[r], rv[r]);
                    }
                    *(f32x4*)(a.y + gp * a.ycs + c0) = o;
                }
            }
        }
    }
}

int g_gdn_force_tile = 0;

template <int P, int WS>
int gdn_launch_tile(const GdnArgs& a, hipStream_t s)
{
    static std::once_flag once;
    static hipError_t attr = hipSuccess;
    std::call_once(once, [] {
        attr = hipFuncSetAttribute((const void*)gdn_kernel<P, WS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   P * (kGdnMaxC + 4) * (int)sizeof(float));
    });
    HIP_TRY(attr);
    const size_t lds = (size_t)P * (a.cs + 4) * sizeof(float);
    const long blocks = (a.npix + P - 1) / P;
    hipLaunchKernelGGL((gdn_kernel<P, WS>), dim3((unsigned)blocks), dim3(P * 4 * WS), lds, s, a);
    HIP_TRY(hipGetLastError());
    return RGBD_OK;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

// pixels per workgroup: the largest tile that still gives every CU two workgroups; above 256 channels a 64-pixel tile would
// leave one workgroup per CU.  Small grids: 16 pixels, the output tiles spread over four waves.
int gdn_tile_for(long npix, int cs)
{
    if (g_gdn_force_tile) return g_gdn_force_tile;
    const int pmax = cs > 256 ? 32 : 64;
    for (int p = pmax; p > 16; p >>= 1)
        if (npix / p >= 512) return p;
    return 16;
}

int launch_gdn(const GdnArgs& a, hipStream_t s)
{
    if (!a.x || !a.y || !a.beta || !a.gamma || a.npix <= 0 || a.npix > ((long)1 << 30) || a.cs <= 0 || a.cs % 16 || a.cs > kGdnMaxC ||
        a.xcs < a.cs || a.ycs < a.cs || a.xcs % 4 || a.ycs % 4 || (a.res && (a.rcs < a.cs || a.rcs % 4)) || !aligned16(a.x) ||
        !aligned16(a.y) || !aligned16(a.res) || !aligned16(a.beta) || !aligned16(a.gamma))
        return RGBD_EINVAL;
    switch (gdn_tile_for(a.npix, a.cs)) {
    case 64: return gdn_launch_tile<64, 1>(a, s);
    case 32: return gdn_launch_tile<32, 1>(a, s);
    default: return gdn_launch_tile<16, 4>(a, s);
    }
}

// NonNegativeParametrizer.forward (CompressAI/compressai/ops/parametrizers.py:42-45) in fp32, as torch computes it:
// max(x, bound), square, subtract the pedestal 2^-36 -- two separately rounded operations (this file is built with
// -ffp-contract=off).  bound is the fp32 buffer lower_bound.bound = float((minimum + 2^-36) ** 0.5), minimum = 1e-6 for beta
// (gdn.py:42) and 0 for gamma (gdn.py:47).
void gdn_parametrize(const float* raw, int64_t n, int is_beta, float* out)
{
    const float pedestal = 0x1p-36f;
    const float bound = is_beta ? (float)sqrt(1e-6 + 0x1p-36) : 0x1p-18f;
    for (int64_t i = 0; i < n; ++i) {
        const float m = raw[i] < bound ? bound : raw[i];  // torch.max(x, bound); (NaN propagates: NaN < bound is false)
        const float sq = m * m;
        out[i] = sq - pedestal;
    }
}

// raw parameters of one layer -> the kernel's operands: beta[cs] (pad channels 1: their norm is 1, their output x * 1 = 0) and
// gamma as MFMA A fragments, [out tile it][in chunk g][lane][e] = gamma[16 it + (lane & 15)][16 g + 4 (lane >> 4) + e] (pad 0)
void gdn_pack(const float* beta_raw, const float* gamma_raw, int c, std::vector<float>* beta, std::vector<float>* gamma)
{
    const int cs = round_up(c, 16), NT = cs / 16;
    std::vector<float> g((size_t)c * c);
    beta->assign(cs, 1.0f);
    gdn_parametrize(beta_raw, c, 1, beta->data());
    gdn_parametrize(gamma_raw, (int64_t)c * c, 0, g.data());
    gamma->assign((size_t)cs * cs, 0.0f);
    for (int it = 0; it < NT; ++it)
        for (int gi = 0; gi < NT; ++gi)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 4; ++e) {
                    const int i = 16 * it + (l & 15), j = 16 * gi + 4 * (l >> 4) + e;
                    if (i < c && j < c) (*gamma)[(((size_t)it * NT + gi) * 64 + l) * 4 + e] = g[(size_t)i * c + j];
                }
}

// ================================================================================================
// C ABI (include/rgbd_amd.h)
// ================================================================================================
extern "C" {

int rgbd_gdn_parametrize(const float* raw, int64_t n, int32_t is_beta, float* out)
{
    if (!raw || !out || n < 0 || is_beta < 0 || is_beta > 1) return RGBD_EINVAL;
    gdn_parametrize(raw, n, is_beta, out);
    return RGBD_OK;
}

int rgbd_debug_force_gdn_tile(int32_t pixels)
{
    if (pixels != 0 && pixels != 16 && pixels != 32 && pixels != 64) return RGBD_EINVAL;
    g_gdn_force_tile = pixels;
    return RGBD_OK;
}

int rgbd_gdn_pack(const float* beta_raw, const float* gamma_raw, int32_t c, float* beta_out, float* gamma_out)
{
    if (!beta_raw || !gamma_raw || !beta_out || !gamma_out || c <= 0 || c > kGdnMaxC) return RGBD_EINVAL;
    std::vector<float> hb, hg;
    gdn_pack(beta_raw, gamma_raw, c, &hb, &hg);
    memcpy(beta_out, hb.data(), hb.size() * sizeof(float));
    memcpy(gamma_out, hg.data(), hg.size() * sizeof(float));
    return RGBD_OK;
}

int rgbd_gdn_nhwc(const float* x, int32_t xcs, int64_t npix, int32_t cs, const float* beta_dev, const float* gamma_dev, int32_t inverse,
                  const float* res, int32_t rcs, float* y, int32_t ycs, void* stream)
{
    GdnArgs a{};
    a.x = x;
    a.xcs = xcs;
    a.y = y;
    a.ycs = ycs;
    a.res = res;
    a.rcs = rcs;
    a.npix = (long)npix;
    a.cs = cs;
    a.beta = beta_dev;
    a.gamma = gamma_dev;
    a.inverse = inverse ? 1 : 0;
    return launch_gdn(a, (hipStream_t)stream);
}

int rgbd_gdn_nchw(const float* x_dev, int32_t n, int32_t c, int32_t h, int32_t w, const float* beta, const float* gamma,
                  int32_t inverse, const float* res_dev, float* y_dev, void* stream)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!x_dev || !beta || !gamma || !y_dev || c <= 0 || c > kGdnMaxC || n <= 0 || h <= 0 || w <= 0 || n > 64 || h > 65536 ||
        w > 65536 || inverse < 0 || inverse > 1 || (int64_t)n * round_up(c, 16) * h * w >= ((int64_t)1 << 28))
        return RGBD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int cs = round_up(c, 16);
    const size_t fl = (size_t)n * h * w * cs;
    std::vector<float> hb, hg;
    gdn_pack(beta, gamma, c, &hb, &hg);
    DevBufs b;
    float *x = b.get(fl), *y = b.get(fl), *r = res_dev ? b.get(fl) : nullptr, *db = b.get(hb.size()), *dg = b.get(hg.size());
    if (!x || !y || (res_dev && !r) || !db || !dg) return RGBD_ENOMEM;
    HIP_TRY(hipMemcpy(db, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dg, hg.data(), hg.size() * sizeof(float), hipMemcpyHostToDevice));
    int rc = launch_nchw_to_nhwc16(x_dev, n, c, h, w, x, cs, s);
    if (!rc && r) rc = launch_nchw_to_nhwc16(res_dev, n, c, h, w, r, cs, s);
    GdnArgs a{};
    a.x = x;
    a.xcs = cs;
    a.y = y;
    a.ycs = cs;
    a.res = r;
    a.rcs = r ? cs : 0;
    a.npix = (long)n * h * w;
    a.cs = cs;
    a.beta = db;
    a.gamma = dg;
    a.inverse = inverse;
    if (!rc) rc = launch_gdn(a, s);
    if (!rc) rc = launch_nhwc_to_nchw_clamp(y, n, c, h, w, cs, y_dev, 0, s);
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = RGBD_EHIP;
    return rc;
}

int rgbd_gdn_bench(int32_t n, int32_t c, int32_t h, int32_t w, int32_t inverse, int32_t with_residual, int32_t iters, float* ms_out)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!ms_out || n <= 0 || c <= 0 || c > kGdnMaxC || h <= 0 || w <= 0 || iters <= 0 || iters > 100000 || inverse < 0 || inverse > 1 ||
        (int64_t)n * round_up(c, 16) * h * w >= ((int64_t)1 << 28))
        return RGBD_EINVAL;
    const int cs = round_up(c, 16);
    const size_t fl = (size_t)n * h * w * cs;
    // GDN's init (gdn.py:43-50) as raw parameters: beta = 1, gamma = 0.1 on the diagonal plus a dense 0.001
    std::vector<float> rb(c, 1.0f), rg((size_t)c * c, sqrtf(0.001f)), hb, hg;
    for (int i = 0; i < c; ++i) rg[(size_t)i * c + i] = sqrtf(0.1f);
    gdn_pack(rb.data(), rg.data(), c, &hb, &hg);
    DevBufs b;
    float *x = b.get(fl), *y = b.get(fl), *r = with_residual ? b.get(fl) : nullptr, *db = b.get(hb.size()), *dg = b.get(hg.size());
    if (!x || !y || (with_residual && !r) || !db || !dg) return RGBD_ENOMEM;
    HIP_TRY(hipMemset(x, 0x3c, fl * sizeof(float)));  // small positive floats
    if (r) HIP_TRY(hipMemset(r, 0x3c, fl * sizeof(float)));
    HIP_TRY(hipMemcpy(db, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dg, hg.data(), hg.size() * sizeof(float), hipMemcpyHostToDevice));
    GdnArgs a{};
    a.x = x;
    a.xcs = cs;
    a.y = y;
    a.ycs = cs;
    a.res = r;
    a.rcs = r ? cs : 0;
    a.npix = (long)n * h * w;
    a.cs = cs;
    a.beta = db;
    a.gamma = dg;
    a.inverse = inverse;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    int rc = launch_gdn(a, nullptr);
    hipError_t he = hipDeviceSynchronize();
    float ms = 0.f;
    if (!rc && he == hipSuccess) {
        he = hipEventRecord(e0, nullptr);
        for (int i = 0; i < iters && !rc; ++i) rc = launch_gdn(a, nullptr);
        if (he == hipSuccess) he = hipEventRecord(e1, nullptr);
        if (he == hipSuccess) he = hipEventSynchronize(e1);
        if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (!rc && he != hipSuccess) rc = RGBD_EHIP;
    if (!rc) *ms_out = ms / iters;
    return rc;
}

}  // extern "C"
