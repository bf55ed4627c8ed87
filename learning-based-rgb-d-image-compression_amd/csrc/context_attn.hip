// The attention contexts of MLIC++ (reference modules/transform/context.py) on gfx950: the checkerboard-masked attention
// inside a 5x5 window around every latent position with its `fusion` convolution (LocalContext.forward :93-133), the
// linear attention of the two global contexts (:198-208, :250-259) and the depthwise 3x3 convolution both of them use.
// All on NHWC fp32 tensors with a channel stride; fp32 single-chain arithmetic (the float contract of the Swin path,
// swin.hip): every sum is one fma / add chain in a fixed order or a fixed tree of such chains, no floating-point atomics,
// so a result is the same bits on every run, and image b of a batch is computed exactly as it is alone (no launch
// parameter that shapes a sum depends on B).  Design and measurements: DESIGN.md 5.4.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

// ---------------------------------------------------------------------------------------------
// Local checkerboard attention.  One workgroup owns a tile of 2 x 4 positions: it stages the q, k, v of the tile and its
// 2-pixel halo (6 x 8 pixels, zeros outside the map: nn.Unfold's padding, context.py:44,96) in LDS once, with the channels
// of a head made contiguous (global channel d * heads + h, :102-110), and then runs 8 * heads * 25 row tasks, one per
// thread: the 25 scores of window row i, their softmax and the 16 outputs o_i = sum_j A_ij v_j, j ascending.  The o_i land
// in LDS in the order `fusion` reads them (channel h * 16 + d slow, window position fast: :127-133), and the second half
// of the kernel is the 800 -> 64 product per position: the weight goes through LDS in slabs of 32 k, transposed so that
// lanes read consecutive output channels, each output one fma chain over k ascending.
constexpr int LC_C = 32, LC_HEADS = 2, LC_HD = 16;  // MLIC++: slice_ch 32 (config/config.py:15-18), head_dim 16
constexpr int LC_TH = 2, LC_TW = 4, LC_NP = LC_TH * LC_TW;
constexpr int LC_EH = LC_TH + 4, LC_EW = LC_TW + 4;
constexpr int LC_PS = 100;            // floats per staged pixel: 3 * 32 and 4 of padding (rows stay 16-byte aligned)
constexpr int LC_K = LC_C * 25;       // fusion's reduction length per position
constexpr int LC_KC = 32;             // k per weight slab
constexpr int LC_CO = 2 * LC_C;
constexpr float LC_MASK = -100.0f;    // context.py:77: a finite number added to the score, not an exclusion

__global__ __launch_bounds__(256) void local_ckbd_attention_kernel(const float* __restrict__ qkv, int H, int W, int qcs,
                                                                   const float* __restrict__ table,
                                                                   const float* __restrict__ fw,
                                                                   const float* __restrict__ fb, float* __restrict__ out,
                                                                   int ocs)
{
    __shared__ __attribute__((aligned(16))) float s_qkv[LC_EH * LC_EW * LC_PS];
    __shared__ __attribute__((aligned(16))) float s_o[LC_NP * LC_K];
    __shared__ __attribute__((aligned(16))) float s_w[LC_KC * LC_CO];
    __shared__ float s_tab[81 * LC_HEADS];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * LC_TW, y0 = blockIdx.y * LC_TH;
    const size_t img = (size_t)blockIdx.z * H * W;

    for (int i = tid; i < 81 * LC_HEADS; i += 256) s_tab[i] = table[i];
    // stage: float4 of global channels c .. c + 3 = (d, h0), (d, h1), (d + 1, h0), (d + 1, h1)
    for (int i = tid; i < LC_EH * LC_EW * (3 * LC_C / 4); i += 256) {
        const int c4 = i % (3 * LC_C / 4), pix = i / (3 * LC_C / 4);
        const int ay = y0 - 2 + pix / LC_EW, ax = x0 - 2 + pix % LC_EW;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ay >= 0 && ay < H && ax >= 0 && ax < W)
            v = *reinterpret_cast<const f32x4*>(qkv + (img + (size_t)ay * W + ax) * qcs + c4 * 4);
        const int which = (c4 * 4) / LC_C, c = (c4 * 4) % LC_C;
        float* dst = s_qkv + pix * LC_PS + which * LC_C;
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[((c + e) % LC_HEADS) * LC_HD + (c + e) / LC_HEADS] = v[e];
    }
    __syncthreads();

    const float scale = 0.25f;  // head_dim ** -0.5 (:42)
    for (int task = tid; task < LC_NP * LC_HEADS * 25; task += 256) {
        const int i = task % 25, h = (task / 25) % LC_HEADS, p = task / (25 * LC_HEADS);
        const int ty = p / LC_TW, tx = p % LC_TW;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        const int iy = i / 5, ix = i % 5;
        const int aiy = y + iy - 2, aix = x + ix - 2;
        const bool row_ok = aiy >= 0 && aiy < H && aix >= 0 && aix < W && ((aiy + aix) & 1);
        float q[LC_HD];
        {
            const float* qp = s_qkv + ((ty + iy) * LC_EW + tx + ix) * LC_PS + h * LC_HD;
#pragma unroll
            for (int d = 0; d < LC_HD; ++d) q[d] = qp[d] * scale;  // q = q * scale before the product (:112)
        }
        float sc[25];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < 25; ++j) {
            const int jy = j / 5, jx = j % 5;
            const float* kp = s_qkv + ((ty + jy) * LC_EW + tx + jx) * LC_PS + LC_C + h * LC_HD;
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < LC_HD; ++d) s = fmaf(q[d], kp[d], s);
            s += s_tab[((iy - jy + 4) * 9 + (ix - jx + 4)) * LC_HEADS + h];  // build_position_index: i - j (:116-121)
            const int ajy = y + jy - 2, ajx = x + jx - 2;
            const bool col_ok = ajy >= 0 && ajy < H && ajx >= 0 && ajx < W && ((ajy + ajx) & 1);
            s += (row_ok && col_ok) ? 0.f : LC_MASK;  // :67-78, 123
            sc[j] = s;
            m = fmaxf(m, s);
        }
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 25; ++j) {
            sc[j] = expf(sc[j] - m);
            sum += sc[j];
        }
        float o[LC_HD];
#pragma unroll
        for (int d = 0; d < LC_HD; ++d) o[d] = 0.f;
#pragma unroll
        for (int j = 0; j < 25; ++j) {
            const int jy = j / 5, jx = j % 5;
            const float* vp = s_qkv + ((ty + jy) * LC_EW + tx + jx) * LC_PS + 2 * LC_C + h * LC_HD;
            const float a = sc[j] / sum;
#pragma unroll
            for (int d = 0; d < LC_HD; ++d) o[d] = fmaf(a, vp[d], o[d]);
        }
        float* op = s_o + p * LC_K + (h * LC_HD) * 25 + i;
#pragma unroll
        for (int d = 0; d < LC_HD; ++d) op[d * 25] = o[d];
    }

    // fusion (:133): out[co] = bias[co] + sum_k o[k] * w[co][k], k = (h * 16 + d) * 25 + i
    const int co = tid & (LC_CO - 1), pg = tid >> 6;  // one wavefront per pair of positions: s_o reads are broadcasts
    const int p0 = pg * 2, p1 = p0 + 1;
    float acc0 = 0.f, acc1 = 0.f;
    for (int k0 = 0; k0 < LC_K; k0 += LC_KC) {
        __syncthreads();  // the o rows (first pass) / the last slab's readers
        {
            const int r = tid >> 2, kq = (tid & 3) * 8;
            const float* src = fw + (size_t)r * LC_K + k0 + kq;
            const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s_w[(kq + e) * LC_CO + r] = a[e];
                s_w[(kq + 4 + e) * LC_CO + r] = b[e];
            }
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < LC_KC; ++kk) {
            const float w = s_w[kk * LC_CO + co];
            acc0 = fmaf(s_o[p0 * LC_K + k0 + kk], w, acc0);
            acc1 = fmaf(s_o[p1 * LC_K + k0 + kk], w, acc1);
        }
    }
    const float bias = fb[co];
    {
        const int y = y0 + p0 / LC_TW, x = x0 + p0 % LC_TW;
        if (y < H && x < W) out[(img + (size_t)y * W + x) * ocs + co] = acc0 + bias;
    }
    {
        const int y = y0 + p1 / LC_TW, x = x0 + p1 % LC_TW;
        if (y < H && x < W) out[(img + (size_t)y * W + x) * ocs + co] = acc1 + bias;
    }
}

// ---------------------------------------------------------------------------------------------
// Linear attention (context.py:198-208, 250-259).  Per image and head: Ks = softmax over the tokens of every key channel,
// Qs = softmax over the head's channels at every token, ctx[d1][d2] = sum_n Ks[d1][n] v[d2][n],
// out[d2][n] = sum_d1 ctx[d1][d2] Qs[d1][n].  The token axis is cut into chunks of LA_T tokens, one workgroup each.
// Stage one (la_partial) leaves per chunk c: m_c[d1] = max of the chunk's keys, s_c[d1] = sum_n exp(k - m_c) and
// ctx_c[d1][d2] = sum_n exp(k[d1][n] - m_c[d1]) v[d2][n], every sum one chain over the chunk's tokens in order.
// Stage two (la_apply) combines them in chunk order, M = max_c m_c, S = sum_c s_c exp(m_c - M),
// ctx = (sum_c ctx_c exp(m_c - M)) / S -- every workgroup for itself, the partials are a few KB -- and applies ctx to its
// chunk of query tokens.  The chunk length is a constant, so the tree does not depend on the batch.
// mode 1 (LinearGlobalIntraContext): the key / value tokens are the anchor positions ((row + col) odd), the query tokens the
// others, row by row (utils/ckbd.py:52-81); the output is written at the query positions and 0.0f at the anchor positions.
constexpr int LA_T = 128;

__device__ __forceinline__ size_t la_pixel(int mode, int anchor, int t, int W)
{
    if (!mode) return (size_t)t;
    const int hw = W >> 1, y = t / hw, xh = t - y * hw;
    return (size_t)y * W + 2 * xh + ((y & 1) ^ anchor);
}

template <int HD>
__global__ __launch_bounds__(256) void la_partial_kernel(const float* __restrict__ k, int kcs, const float* __restrict__ v,
                                                         int vcs, int H, int W, int ntok, int mode, float* __restrict__ ws)
{
    constexpr int REC = HD * HD + 2 * HD;
    constexpr int NPT = HD * HD / 256, G = HD / NPT, P = 256 / HD;
    __shared__ __attribute__((aligned(16))) float s_e[LA_T * HD];
    __shared__ __attribute__((aligned(16))) float s_v[LA_T * HD];
    __shared__ float s_red[256];
    __shared__ float s_m[HD];
    const int tid = threadIdx.x, chunk = blockIdx.x, head = blockIdx.y, heads = gridDim.y, b = blockIdx.z;
    const int t0 = chunk * LA_T, nt = min(LA_T, ntok - t0);
    const size_t img = (size_t)b * H * W;
    for (int i = tid; i < LA_T * HD / 4; i += 256) {
        const int tl = i / (HD / 4), c4 = i % (HD / 4);
        f32x4 kk = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
        if (tl < nt) {
            const size_t pix = img + la_pixel(mode, 1, t0 + tl, W);
            kk = *reinterpret_cast<const f32x4*>(k + pix * kcs + head * HD + c4 * 4);
            vv = *reinterpret_cast<const f32x4*>(v + pix * vcs + head * HD + c4 * 4);
        }
        *reinterpret_cast<f32x4*>(s_e + tl * HD + c4 * 4) = kk;
        *reinterpret_cast<f32x4*>(s_v + tl * HD + c4 * 4) = vv;
    }
    __syncthreads();
    {
        const int d = tid % HD, part = tid / HD;
        float m = -INFINITY;
        for (int tl = part; tl < nt; tl += P) m = fmaxf(m, s_e[tl * HD + d]);
        s_red[tid] = m;
    }
    __syncthreads();
    if (tid < HD) {
        float m = s_red[tid];
        for (int p = 1; p < P; ++p) m = fmaxf(m, s_red[p * HD + tid]);
        s_m[tid] = m;
    }
    __syncthreads();
    for (int i = tid; i < LA_T * HD; i += 256) s_e[i] = (i / HD) < nt ? expf(s_e[i] - s_m[i % HD]) : 0.f;
    __syncthreads();
    float* rec = ws + (((size_t)b * heads + head) * gridDim.x + chunk) * REC;
    {
        const int d1 = tid / G, d2 = (tid % G) * NPT;
        float acc[NPT];
#pragma unroll
        for (int j = 0; j < NPT; ++j) acc[j] = 0.f;
        for (int n = 0; n < nt; ++n) {
            const float e = s_e[n * HD + d1];
#pragma unroll
            for (int j = 0; j < NPT; ++j) acc[j] = fmaf(e, s_v[n * HD + d2 + j], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < NPT; ++j) rec[d1 * HD + d2 + j] = acc[j];
    }
    if (tid < HD) {
        float sum = 0.f;
        for (int n = 0; n < nt; ++n) sum += s_e[n * HD + tid];
        rec[HD * HD + tid] = s_m[tid];
        rec[HD * HD + HD + tid] = sum;
    }
}

template <int HD>
__global__ __launch_bounds__(LA_T) void la_apply_kernel(const float* __restrict__ q, int qcs, const float* __restrict__ ws,
                                                       int H, int W, int ntok, int mode, float* __restrict__ out, int ocs)
{
    constexpr int REC = HD * HD + 2 * HD;
    __shared__ __attribute__((aligned(16))) float s_ctx[HD * HD];
    __shared__ float s_M[HD], s_S[HD];
    const int tid = threadIdx.x, chunk = blockIdx.x, nch = gridDim.x, head = blockIdx.y, heads = gridDim.y, b = blockIdx.z;
    const float* rec = ws + ((size_t)b * heads + head) * nch * REC;
    if (tid < HD) {
        float M = -INFINITY, S = 0.f;
        for (int c = 0; c < nch; ++c) M = fmaxf(M, rec[(size_t)c * REC + HD * HD + tid]);
        for (int c = 0; c < nch; ++c)
            S = fmaf(rec[(size_t)c * REC + HD * HD + HD + tid], expf(rec[(size_t)c * REC + HD * HD + tid] - M), S);
        s_M[tid] = M;
        s_S[tid] = S;
    }
    __syncthreads();
    for (int i = tid; i < HD * HD; i += LA_T) {
        const int d1 = i / HD;
        float acc = 0.f;
        for (int c = 0; c < nch; ++c)
            acc = fmaf(rec[(size_t)c * REC + i], expf(rec[(size_t)c * REC + HD * HD + d1] - s_M[d1]), acc);
        s_ctx[i] = acc / s_S[d1];
    }
    __syncthreads();
    const int t = chunk * LA_T + tid;
    if (t >= ntok) return;
    const size_t img = (size_t)b * H * W;
    const size_t pix = img + la_pixel(mode, 0, t, W);
    float qs[HD];
    float m = -INFINITY;
#pragma unroll
    for (int c4 = 0; c4 < HD / 4; ++c4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(q + pix * qcs + head * HD + c4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            qs[c4 * 4 + e] = v[e];
            m = fmaxf(m, v[e]);
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) {
        qs[d] = expf(qs[d] - m);
        sum += qs[d];
    }
    float o[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) o[d] = 0.f;
#pragma unroll
    for (int d1 = 0; d1 < HD; ++d1) {
        const float a = qs[d1] / sum;
#pragma unroll
        for (int d2 = 0; d2 < HD; ++d2) o[d2] = fmaf(s_ctx[d1 * HD + d2], a, o[d2]);
    }
    float* op = out + pix * ocs + head * HD;
#pragma unroll
    for (int c4 = 0; c4 < HD / 4; ++c4) {
        const f32x4 v = {o[c4 * 4], o[c4 * 4 + 1], o[c4 * 4 + 2], o[c4 * 4 + 3]};
        *reinterpret_cast<f32x4*>(op + c4 * 4) = v;
    }
    if (mode) {
        float* zp = out + (img + la_pixel(1, 1, t, W)) * ocs + head * HD;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c4 = 0; c4 < HD / 4; ++c4) *reinterpret_cast<f32x4*>(zp + c4 * 4) = z;
    }
}

// ---------------------------------------------------------------------------------------------
// nn.Conv2d(C, C, 3, stride 1, padding 1, groups = C) on NHWC: one thread per (pixel, channel), the nine taps in (ky, kx) order
// as one fma chain (taps outside the map are left out: their products are exact zeros), then the bias, then nn.GELU() in
// the erf form of the conv reducer (conv_mfma.hip).
__global__ __launch_bounds__(256) void dwconv3x3_kernel(const float* __restrict__ x, int B, int H, int W, int C, int xcs,
                                                        const float* __restrict__ w, const float* __restrict__ bias, int gelu,
                                                        float* __restrict__ y, int ycs)
{
    const size_t total = (size_t)B * H * W * C;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const size_t pix = i / C;
        const int px = (int)(pix % W), py = (int)((pix / W) % H);
        const float* wp = w + (size_t)c * 9;
        float acc = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = py + ky - 1, ix = px + kx - 1;
                if (iy >= 0 && iy < H && ix >= 0 && ix < W)
                    acc = fmaf(x[(size_t)((ptrdiff_t)pix + (ky - 1) * W + (kx - 1)) * xcs + c], wp[ky * 3 + kx], acc);
            }
        }
        acc += bias[c];
        if (gelu) acc = 0.5f * acc * (1.0f + erff(acc * 0.70710678118654752f));
        y[pix * ycs + c] = acc;
    }
}

// utils/ckbd.py:37-48: xa = x at the anchor positions ((row + col) odd) and 0 elsewhere, xn the other half
__global__ __launch_bounds__(256) void ckbd_split_kernel(const float* __restrict__ x, size_t npix, int H, int W, int cs,
                                                         float* __restrict__ xa, float* __restrict__ xn)
{
    const int c4n = cs / 4;
    const size_t total = npix * c4n;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t pix = i / c4n;
        const int px = (int)(pix % W), py = (int)((pix / W) % H);
        const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
        const bool anchor = (px + py) & 1;
        reinterpret_cast<f32x4*>(xa)[i] = anchor ? v : z;
        reinterpret_cast<f32x4*>(xn)[i] = anchor ? z : v;
    }
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
unsigned grid_for(size_t total)
{
    const size_t g = (total + 255) / 256;
    return (unsigned)(g > 8192 ? 8192 : (g ? g : 1));
}

}  // namespace

int launch_local_ckbd_attention(const float* qkv, int qcs, int B, int H, int W, int C, int heads, const float* table,
                                const float* fusion_w, const float* fusion_b, float* out, int ocs, hipStream_t s)
{
    if (!qkv || !table || !fusion_w || !fusion_b || !out || B <= 0 || H <= 0 || W <= 0 || C != LC_C || heads != LC_HEADS ||
        qcs < 3 * C || qcs % 4 || ocs < 2 * C || !al16(qkv) || !al16(fusion_w) || B > 65535 || H > 65535 * LC_TH ||
        (int64_t)B * H * W > 0x7fffffff)
        return RGBD_EINVAL;
    const dim3 grid((unsigned)((W + LC_TW - 1) / LC_TW), (unsigned)((H + LC_TH - 1) / LC_TH), (unsigned)B);
    hipLaunchKernelGGL(local_ckbd_attention_kernel, grid, dim3(256), 0, s, qkv, H, W, qcs, table, fusion_w, fusion_b, out, ocs);
    HIP_TRY(hipGetLastError());
    return RGBD_OK;
}

int64_t linear_attention_ws_floats(int B, int H, int W, int heads, int head_dim, int mode)
{
    if (B <= 0 || H <= 0 || W <= 0 || heads <= 0 || (head_dim != 16 && head_dim != 32) || mode < 0 || mode > 1 || (mode && (W & 1)) ||
        (int64_t)B * H * W > 0x7fffffff)
        return RGBD_EINVAL;
    const int64_t ntok = (int64_t)H * W >> mode, nch = (ntok + LA_T - 1) / LA_T;
    return (int64_t)B * heads * nch * (head_dim * head_dim + 2 * head_dim);
}

int launch_linear_attention(const float* k, int kcs, const float* q, int qcs, const float* v, int vcs, int B, int H, int W,
                            int heads, int head_dim, int mode, float* out, int ocs, float* ws, int64_t ws_floats, hipStream_t s)
{
    const int64_t need = linear_attention_ws_floats(B, H, W, heads, head_dim, mode);
    if (need <= 0 || !k || !q || !v || !out || !ws || ws_floats < need) return RGBD_EINVAL;
    const int dim = heads * head_dim;
    if (kcs < dim || qcs < dim || vcs < dim || ocs < dim || kcs % 4 || qcs % 4 || vcs % 4 || ocs % 4 || !al16(k) || !al16(q) ||
        !al16(v) || !al16(out) || B > 65535 || heads > 65535)
        return RGBD_EINVAL;
    const int ntok = (int)((int64_t)H * W >> mode);
    const int nch = (ntok + LA_T - 1) / LA_T;
    const dim3 grid((unsigned)nch, (unsigned)heads, (unsigned)B);
    if (head_dim == 16) {
        hipLaunchKernelGGL(la_partial_kernel<16>, grid, dim3(256), 0, s, k, kcs, v, vcs, H, W, ntok, mode, ws);
        hipLaunchKernelGGL(la_apply_kernel<16>, grid, dim3(LA_T), 0, s, q, qcs, (const float*)ws, H, W, ntok, mode, out, ocs);
    } else {
        hipLaunchKernelGGL(la_partial_kernel<32>, grid, dim3(256), 0, s, k, kcs, v, vcs, H, W, ntok, mode, ws);
        hipLaunchKernelGGL(la_apply_kernel<32>, grid, dim3(LA_T), 0, s, q, qcs, (const float*)ws, H, W, ntok, mode, out, ocs);
    }
    HIP_TRY(hipGetLastError());
    return RGBD_OK;
}

int launch_dwconv3x3(const float* x, int B, int H, int W, int C, int xcs, const float* w, const float* bias, int gelu, float* y,
                     int ycs, hipStream_t s)
{
    if (!x || !w || !bias || !y || x == y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || xcs < C || ycs < C || gelu < 0 || gelu > 1 ||
        (int64_t)B * H * W > 0x7fffffff)
        return RGBD_EINVAL;
    hipLaunchKernelGGL(dwconv3x3_kernel, dim3(grid_for((size_t)B * H * W * C)), dim3(256), 0, s, x, B, H, W, C, xcs, w, bias, gelu,
                       y, ycs);
    HIP_TRY(hipGetLastError());
    return RGBD_OK;
}

int launch_ckbd_split(const float* x, int B, int H, int W, int cs, float* xa, float* xn, hipStream_t s)
{
    if (!x || !xa || !xn || B <= 0 || H <= 0 || W <= 0 || cs <= 0 || cs % 4 || !al16(x) || !al16(xa) || !al16(xn)) return RGBD_EINVAL;
    const size_t npix = (size_t)B * H * W;
    hipLaunchKernelGGL(ckbd_split_kernel, dim3(grid_for(npix * (cs / 4))), dim3(256), 0, s, x, npix, H, W, cs, xa, xn);
    HIP_TRY(hipGetLastError());
    return RGBD_OK;
}

extern "C" int rgbd_local_ckbd_attention(const float* qkv, int32_t qcs, int32_t B, int32_t H, int32_t W, int32_t C, int32_t heads,
                                         const float* table, const float* fusion_w, const float* fusion_b, float* out,
                                         int32_t ocs, void* stream)
{
    return launch_local_ckbd_attention(qkv, qcs, B, H, W, C, heads, table, fusion_w, fusion_b, out, ocs, (hipStream_t)stream);
}

extern "C" int64_t rgbd_linear_attention_ws_floats(int32_t B, int32_t H, int32_t W, int32_t heads, int32_t head_dim, int32_t mode)
{
    return linear_attention_ws_floats(B, H, W, heads, head_dim, mode);
}

extern "C" int rgbd_linear_attention(const float* k, int32_t kcs, const float* q, int32_t qcs, const float* v, int32_t vcs,
                                     int32_t B, int32_t H, int32_t W, int32_t heads, int32_t head_dim, int32_t mode, float* out,
                                     int32_t ocs, float* ws, int64_t ws_floats, void* stream)
{
    return launch_linear_attention(k, kcs, q, qcs, v, vcs, B, H, W, heads, head_dim, mode, out, ocs, ws, ws_floats,
                                   (hipStream_t)stream);
}

extern "C" int rgbd_dwconv3x3(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t xcs, const float* w,
                              const float* bias, int32_t gelu, float* y, int32_t ycs, void* stream)
{
    return launch_dwconv3x3(x, B, H, W, C, xcs, w, bias, gelu, y, ycs, (hipStream_t)stream);
}
