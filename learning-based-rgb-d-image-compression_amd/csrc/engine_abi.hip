// Host runtime of the gfx950 codec engine, part 3 of 3: the C ABI of include/rgbd_amd.h -- engine life cycle (create /
// finalize / clone / destroy), the codec entry points, the operator-level entry points (conv2d, pointwise ops, conv
// bench) and every test / debug hook.  The coder's stand-alone entry points live in coder_abi.hip.
#include "engine.h"

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

int rgbd_abi_version(void) { return RGBD_AMD_ABI_VERSION; }

// Host threads that wait for the GPU sleep instead of spinning (hipDeviceScheduleBlockingSync for the current device).
// The policy is a device flag of the process.  Work submitted under one policy and awaited under the other is what the two
// "hipFree never returns" records have in common (profiles/r03_hang_diagnosis.txt; round 4: an engine that had run under
// the spinning policy was garbage-collected -- rgbd_elic_destroy -> hipFree -> every stream of the device -- right after a
// CodecPool had switched the policy): so the device is drained under the OLD policy before the flag changes, and the Python
// side collects garbage engines first (pool.py).  (Measured and dropped: switching to the spinning policy around every
// hipFree -- with a pool's other threads launching in that window it produced exactly such mixed waits, and the suite hung.)
// Wait policy of the host threads (round 5; advisor findings on the round-4 `hipFree never returns` record).  The hang needs
// work submitted under one policy and waited for under the other, so the policy no longer moves while an engine exists: the
// FIRST engine created on a device switches that device to hipDeviceScheduleBlockingSync (sleeping waits: what every pooled
// or pipelined user wants, and ~1 ms of a 190 ms call for a lone one) before it has launched anything, and
// rgbd_set_blocking_sync() refuses (RGBD_ESTATE) to change the policy while any engine is alive.  RGBD_SPIN_WAIT=1 keeps the
// runtime's default (spinning) policy for the whole process instead.
static std::atomic<int> g_live_engines{0};
static std::mutex g_policy_mu;
static bool g_policy_done[64] = {false};

static int ensure_wait_policy()
{
    static const bool spin = getenv("RGBD_SPIN_WAIT") != nullptr;
    if (spin) return RGBD_OK;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(g_policy_mu);
    if (dev < 0 || dev >= 64 || g_policy_done[dev]) return RGBD_OK;
    if (g_live_engines.load() == 0) {
        std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);
        HIP_TRY(hipDeviceSynchronize());  // (whatever the caller's framework has in flight drains under the old policy)
        HIP_TRY(hipSetDeviceFlags(hipDeviceScheduleBlockingSync));
    }
    g_policy_done[dev] = true;
    return RGBD_OK;
}

int rgbd_get_blocking_sync(void);
int rgbd_set_blocking_sync(int32_t on)
{
    const int cur = rgbd_get_blocking_sync();
    if (cur < 0) return cur;
    if ((on ? 1 : 0) == cur) return RGBD_OK;
    if (g_live_engines.load() > 0) return RGBD_ESTATE;  // never under a live engine's feet
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // a device-wide wait: not while a stream of this process captures
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipSetDeviceFlags(on ? hipDeviceScheduleBlockingSync : hipDeviceScheduleAuto));
    if (!on) {
        std::lock_guard<std::mutex> g(g_policy_mu);
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) g_policy_done[dev] = false;  // the next first engine decides again
    }
    return RGBD_OK;
}

int rgbd_get_blocking_sync(void)
{
    unsigned flags = 0;
    HIP_TRY(hipGetDeviceFlags(&flags));
    return (flags & hipDeviceScheduleMask) == hipDeviceScheduleBlockingSync ? 1 : 0;
}

static int conv2d_nchw_impl(const float* x_dev, int32_t n, int32_t cin, int32_t h, int32_t w, const float* weight,
                            const float* bias, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t transposed,
                            int32_t act, const float* residual_dev, float* y_dev, void* stream, int refmode,
                            const int32_t* blocks, int32_t nblocks, int32_t bias_mode, int32_t flags);

int rgbd_conv2d_nchw(const float* x_dev, int32_t n, int32_t cin, int32_t h, int32_t w, const float* weight,
                     const float* bias, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t transposed,
                     int32_t act, const float* residual_dev, float* y_dev, void* stream)
{
    return conv2d_nchw_impl(x_dev, n, cin, h, w, weight, bias, cout, k, stride, pad, transposed, act, residual_dev, y_dev, stream,
                            0, nullptr, 0, 0, 0);
}

// The same layer in the reference's CPU arithmetic: channels stored permuted (rgbd_cperm), accumulation in
// blocks (`blocks`: channels per block, nullptr = one block per 16 channels), bias_mode as ConvArgs::bias_mode.
// flags bit 0: sigmoid as the reference's vector kernel computes it; bit 1: reduce the blocks as split-K ranges (1x1 layers)
int rgbd_conv2d_ref_nchw(const float* x_dev, int32_t n, int32_t cin, int32_t h, int32_t w, const float* weight,
                         const float* bias, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t transposed,
                         int32_t act, const float* residual_dev, float* y_dev, void* stream, const int32_t* blocks,
                         int32_t nblocks, int32_t bias_mode, int32_t flags)
{
    return conv2d_nchw_impl(x_dev, n, cin, h, w, weight, bias, cout, k, stride, pad, transposed, act, residual_dev, y_dev, stream,
                            1, blocks, nblocks, bias_mode, flags);
}

static int conv2d_nchw_impl(const float* x_dev, int32_t n, int32_t cin, int32_t h, int32_t w, const float* weight,
                            const float* bias, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t transposed,
                            int32_t act, const float* residual_dev, float* y_dev, void* stream, int refmode,
                            const int32_t* blocks, int32_t nblocks, int32_t bias_mode, int32_t flags)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!x_dev || !weight || !y_dev || n <= 0 || cin <= 0 || cout <= 0 || k <= 0 || k > 5 || stride < 1 || stride > 2)
        return RGBD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    HostTensor hw, hb;
    hw.shape = transposed ? std::vector<int64_t>{cin, cout, k, k} : std::vector<int64_t>{cout, cin, k, k};
    hw.v.assign(weight, weight + (size_t)cin * cout * k * k);
    if (bias) {
        hb.shape = {cout};
        hb.v.assign(bias, bias + cout);
    }
    const bool subpix = !refmode && transposed && g_subpix == 2 && cout <= 4 && k == 5 && stride == 2 && pad == 2 && !residual_dev;
    const int perm = refmode ? 1 : 0;
    DevBufs b;
    DevGen gen;  // (owns the packed weights: released on every way out)
    PackedConv pc;
    int rc = subpix ? pack_subpix(hw, bias ? &hb : nullptr, &pc, &gen)
                    : pack_conv(hw, bias ? &hb : nullptr, transposed != 0, &pc, &gen, perm, perm);
    if (rc) return rc;
    int OH, OW;
    conv_out_hw(h, w, k, stride, pad, transposed != 0, &OH, &OW);
    const size_t xf = (size_t)n * h * w * pc.cin_pad, yf = (size_t)n * OH * OW * pc.cout_pad;
    ConvArgs a{};
    a.cin_pad = pc.cin_pad;  // (what the block helpers measure the blocks against)
    a.splitk = (g_force_splitk > 0 && !refmode) ? std::min(g_force_splitk, pc.cin_pad / 16) : 1;
    if (refmode) {
        a.bias_mode = bias_mode;
        a.exact_math = flags & 1;
        if ((flags & 2) && blocks && nblocks > 1 && nblocks <= 16) {  // the blocks as split-K ranges of the single-chain kernel
            rc = conv_set_split_ranges(&a, blocks, nblocks);
            if (bias_mode == 1) rc = RGBD_EINVAL;
        } else if (blocks && nblocks == 1) {
            if (bias_mode == 1) a.bias_mode = 0;  // (one block: S_0 + bias is the epilogue's add)
        } else {
            rc = conv_set_blocks(&a, blocks, nblocks);
        }
        if (rc) return rc;
    }
    float *xin = b.get(xf), *yout = b.get(yf), *res = residual_dev ? b.get(yf) : nullptr;
    float* part = a.splitk > 1 ? b.get((size_t)a.splitk * yf) : nullptr;  // (read by the reducer: released after the stream has drained)
    if (!xin || !yout || (residual_dev && !res) || (a.splitk > 1 && !part)) return RGBD_ENOMEM;
    conv_args_geometry(&a, pc, xin, n, h, w, pc.cin_pad, yout, pc.cout_pad, OH, OW, stride, pad);
    conv_args_epilogue(&a, act, g_force_ckbd, res, pc.cout_pad, nullptr, 0, nullptr, 0, nullptr, 0);
    a.partial = part;
    rc = launch_nchw_to_nhwc16(x_dev, n, cin, h, w, xin, pc.cin_pad, s, perm);
    if (!rc && res) rc = launch_nchw_to_nhwc16(residual_dev, n, cout, OH, OW, res, pc.cout_pad, s, perm);
    // (the sub-pixel form does not write channels 4..15; the half a checkerboard launch does not compute reads as zero)
    if (!rc && (subpix || a.ckbd)) HIP_TRY(hipMemsetAsync(yout, 0, yf * sizeof(float), s));
    if (!rc) rc = launch_conv(a, s);
    if (!rc) rc = launch_nhwc_to_nchw_clamp(yout, n, cout, OH, OW, pc.cout_pad, y_dev, 0, s, perm);
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = RGBD_EHIP;
    return rc;
}

// Pointwise operators of Bi-SPF / ESA / SE_Block alone (modules/transform/attention.py:52-97), NCHW in, NCHW out: what
// tests/test_gpu_pointwise.py compares with torch's F.max_pool2d / F.interpolate / the SE_Block arithmetic.
//   op 0: max_pool2d(kernel 7, stride 3) -> y [n, c, (h-7)/3+1, (w-7)/3+1]
//   op 1: interpolate(bilinear, align_corners=False) to (oh, ow)
//   op 2: SE_Block: y = x * sigmoid(fc2(relu(fc0(mean_hw(x)))))   (w0 [c/16][c], w1 [c][c/16], no biases)
//   op 3: the engine's residual form x + x * gate (entropy.py:75)
int rgbd_pointwise_nchw(int32_t op, const float* x_dev, int32_t n, int32_t c, int32_t h, int32_t w, int32_t oh, int32_t ow,
                        const float* w0, const float* w1, float* y_dev, void* stream)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!x_dev || !y_dev || n <= 0 || c <= 0 || h <= 0 || w <= 0 || op < 0 || op > 3) return RGBD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int cs = round_up(c, 16);
    if (op == 0) {
        oh = (h - 7) / 3 + 1;
        ow = (w - 7) / 3 + 1;
        if (h < 7 || w < 7) return RGBD_EINVAL;
    } else if (op >= 2) {
        oh = h;
        ow = w;
        if (!w0 || !w1 || c % 16) return RGBD_EINVAL;
    } else if (oh <= 0 || ow <= 0) {
        return RGBD_EINVAL;
    }
    DevBufs b;  // (test / tool entry point, not the codec path: every buffer is released on every way out)
    float *xin = b.get((size_t)n * h * w * cs), *yout = b.get((size_t)n * oh * ow * cs);
    if (!xin || !yout) return RGBD_ENOMEM;
    // (the operators as the codec runs them: channels stored permuted, the reference's CPU arithmetic -- DESIGN.md 4a)
    int rc = launch_nchw_to_nhwc16(x_dev, n, c, h, w, xin, cs, s, 1);
    if (!rc && op == 0) rc = launch_maxpool7s3(xin, n, h, w, cs, yout, oh, ow, s);
    if (!rc && op == 1) rc = launch_bilinear(xin, n, h, w, cs, yout, oh, ow, s, nullptr, nullptr, c);
    if (!rc && op >= 2) {
        const int hid = c / 16;
        float *aux = b.get((size_t)n * (2 * c + hid + 1)), *dw0 = b.get((size_t)c * hid), *dw1 = b.get((size_t)c * hid);
        if (!aux || !dw0 || !dw1) return RGBD_ENOMEM;
        HIP_TRY(hipMemcpy(dw0, w0, (size_t)c * hid * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dw1, w1, (size_t)c * hid * sizeof(float), hipMemcpyHostToDevice));
        float *mean = aux, *sc = aux + (size_t)n * c, *hd = aux + (size_t)2 * n * c;
        rc = launch_channel_mean_ref(xin, n, h * w, cs, c, mean, c, s);
        if (!rc) rc = launch_se_fc_ref(mean, n, c, hid, dw0, dw1, nullptr, nullptr, hd, sc, s);  // (every row in the main order)
        if (!rc) rc = launch_channel_scale_to(xin, n, h * w, cs, c, sc, op == 3 ? 1 : 0, yout, cs, s);
    }
    if (!rc) rc = launch_nhwc_to_nchw_clamp(yout, n, c, oh, ow, cs, y_dev, 0, s, 1);
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = RGBD_EHIP;
    return rc;
}

// ---- the reference-arithmetic pointwise kernels alone (test hooks: tests/test_gpu_refpointwise.py) ---------------------------
// Each hook validates every argument on the host before anything is allocated or launched, converts its logical NCHW / logical
// channel-order tensors to the engine's layout (NHWC, channels permuted: rgbd_cperm), calls the launcher the engine calls with
// the engine's permutation arguments, and converts back.  Device scratch is released on every way out.
namespace {
// deconv_s2_ref_run's scratch outside an engine: one device allocation per take, all released when the hook returns
struct MallocScratch {
    DevBufs& b;
    size_t mark() const { return 0; }
    float* take(size_t bytes) { return b.get((bytes + 3) / 4); }
    void release(size_t) {}
};
// sizes only (the validation pass of the recipe: nothing is allocated, nothing launched)
struct NoScratch {
    size_t mark() const { return 0; }
    float* take(size_t) { return nullptr; }
    void release(size_t) {}
};
inline bool tensor_ok(int64_t n, int64_t c, int64_t h, int64_t w)
{
    return n > 0 && c > 0 && h > 0 && w > 0 && n <= 64 && c <= 65536 && h <= 65536 && w <= 65536 &&
           n * round_up((int)c, 16) * h * w < ((int64_t)1 << 28);
}
}  // namespace

int rgbd_ref_channel_mean(const float* x_dev, int32_t n, int32_t c, int32_t h, int32_t w, float* mean_dev, int32_t mstride,
                          void* stream)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);
    if (!x_dev || !mean_dev || !tensor_ok(n, c, h, w) || c % 16 || mstride < c || mstride > (1 << 20)) return RGBD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    DevBufs b;
    const size_t mfloats = (size_t)(n - 1) * mstride + c;
    float* xin = b.get((size_t)n * h * w * c);
    float* mean = b.get(mfloats);
    if (!xin || !mean) return RGBD_ENOMEM;
    int rc = launch_nchw_to_nhwc16(x_dev, n, c, h, w, xin, c, s, 1);
    if (!rc) rc = launch_channel_mean_ref(xin, n, h * w, c, c, mean, mstride, s);  // (mean[image * mstride + channel POSITION])
    std::vector<float> hm(mfloats), row(c);
    if (!rc) HIP_TRY(hipMemcpyAsync(hm.data(), mean, mfloats * sizeof(float), hipMemcpyDeviceToHost, s));
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = RGBD_EHIP;
    for (int i = 0; i < n && !rc; ++i) {  // only the c means of every image are written: the rest of a row is the caller's
        for (int ch = 0; ch < c; ++ch) row[ch] = hm[(size_t)i * mstride + rgbd_cperm(ch)];
        HIP_TRY(hipMemcpy(mean_dev + (size_t)i * mstride, row.data(), (size_t)c * sizeof(float), hipMemcpyHostToDevice));
    }
    return rc;
}

int rgbd_ref_linear(const float* weight, const float* x_dev, int32_t n, int32_t K, int32_t J, const int32_t* row_class, int32_t form,
                    int32_t act, int32_t stage, float* y_dev, void* stream)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);
    if (!weight || !x_dev || !y_dev || n <= 0 || n > 64 || K <= 0 || J <= 0 || K > 65536 || J > 65536) return RGBD_EINVAL;
    if ((form != -1 && form != 3) || (act != ACT_NONE && act != ACT_RELU && act != ACT_SIGMOID) || stage < 0 || stage > 1) return RGBD_EINVAL;
    if ((stage == 0 ? K : J) % 16) return RGBD_EINVAL;  // the side that lives in the permuted layout
    if (row_class)
        for (int j = 0; j < J; ++j)
            if (row_class[j] < 0 || row_class[j] > 2) return RGBD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    DevBufs b;
    float* dw = b.get((size_t)J * K);
    float* xp = b.get((size_t)n * K);
    float* yp = b.get((size_t)n * J);
    int* cls = row_class ? (int*)b.get(J) : nullptr;
    if (!dw || !xp || !yp || (row_class && !cls)) return RGBD_ENOMEM;
    HIP_TRY(hipMemcpy(dw, weight, (size_t)J * K * sizeof(float), hipMemcpyHostToDevice));
    if (cls) HIP_TRY(hipMemcpy(cls, row_class, (size_t)J * sizeof(int), hipMemcpyHostToDevice));
    int rc;
    if (stage == 0) {  // fc.0: the input is the mean vector (by position), the output the hidden vector (plain)
        rc = launch_nchw_to_nhwc16(x_dev, n, K, 1, 1, xp, K, s, 1);
        if (!rc) rc = launch_se_linear_ref(dw, xp, n, K, J, K, 1, cls, act, y_dev, J, 0, form, s);
    } else {           // fc.2: the input is the hidden vector (plain), the output the gate vector (by position)
        rc = launch_se_linear_ref(dw, x_dev, n, K, J, K, 0, cls, act, yp, J, 1, form, s);
        if (!rc) rc = launch_nhwc_to_nchw_clamp(yp, n, J, 1, 1, J, y_dev, 0, s, 1);
    }
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = RGBD_EHIP;
    return rc;
}

int rgbd_ref_sigmoid_gate(const float* t_dev, const float* mul_dev, const float* res_dev, int32_t n, int32_t c, int32_t h, int32_t w,
                          int32_t per_image, int32_t threads, float* y_dev, void* stream)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);
    if (!t_dev || !y_dev || !tensor_ok(n, c, h, w) || threads < 1 || threads > 1024 || per_image < 0 || per_image > 1) return RGBD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int cs = round_up(c, 16);
    const size_t fl = (size_t)n * h * w * cs;
    DevBufs b;
    float *t = b.get(fl), *y = b.get(fl), *m = mul_dev ? b.get(fl) : nullptr, *r = res_dev ? b.get(fl) : nullptr;
    if (!t || !y || (mul_dev && !m) || (res_dev && !r)) return RGBD_ENOMEM;
    int rc = launch_nchw_to_nhwc16(t_dev, n, c, h, w, t, cs, s, 1);
    if (!rc && m) rc = launch_nchw_to_nhwc16(mul_dev, n, c, h, w, m, cs, s, 1);
    if (!rc && r) rc = launch_nchw_to_nhwc16(res_dev, n, c, h, w, r, cs, s, 1);
    if (!rc) rc = launch_sigmoid_gate_ref(t, cs, m, m ? cs : 0, r, r ? cs : 0, y, cs, n, h * w, c, per_image, threads, s);
    if (!rc) rc = launch_nhwc_to_nchw_clamp(y, n, c, h, w, cs, y_dev, 0, s, 1);
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = RGBD_EHIP;
    return rc;
}

int rgbd_ref_small_conv_nchw(const float* x_dev, int32_t n, int32_t cin, int32_t h, int32_t w, const float* weight, const float* bias,
                             int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t act, int32_t ckbd, const int32_t* kblocks,
                             int32_t nkblocks, const float* res1_dev, const float* mul_dev, const float* res2_dev, float* y_dev,
                             float* y2_dev, void* stream)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);
    if (!x_dev || !weight || !y_dev || !tensor_ok(n, cin, h, w) || cout <= 0 || cout > 65536 || k < 1 || k > 3 || stride < 1 ||
        stride > 2 || pad < 0 || pad > k || act < ACT_NONE || act > ACT_SIGMOID || ckbd < 0 || ckbd > 2 || (ckbd && stride != 1))
        return RGBD_EINVAL;
    if (h + 2 * pad < k || w + 2 * pad < k) return RGBD_EINVAL;
    int OH, OW;
    conv_out_hw(h, w, k, stride, pad, false, &OH, &OW);
    if (!tensor_ok(n, cout, OH, OW)) return RGBD_EINVAL;
    SmallConvArgs a{};
    if (small_conv_set_kblocks(&a, kblocks, nkblocks, cin * k * k)) return RGBD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    HostTensor hw, hb;
    hw.shape = {cout, cin, k, k};
    hw.v.assign(weight, weight + (size_t)cin * cout * k * k);
    if (bias) {
        hb.shape = {cout};
        hb.v.assign(bias, bias + cout);
    }
    DevBufs b;
    DevGen gen;  // (owns the packed weights: released on every way out)
    PackedConv pc;
    int rc = pack_conv(hw, bias ? &hb : nullptr, false, &pc, &gen, 1, 1);
    if (rc) return rc;
    const size_t xf = (size_t)n * h * w * pc.cin_pad, yf = (size_t)n * OH * OW * pc.cout_pad;
    float *xin = b.get(xf), *y = b.get(yf), *y2 = y2_dev ? b.get(yf) : nullptr;
    float *r1 = res1_dev ? b.get(yf) : nullptr, *m = mul_dev ? b.get(yf) : nullptr, *r2 = res2_dev ? b.get(yf) : nullptr;
    if (!xin || !y || (y2_dev && !y2) || (res1_dev && !r1) || (mul_dev && !m) || (res2_dev && !r2)) return RGBD_ENOMEM;
    rc = launch_nchw_to_nhwc16(x_dev, n, cin, h, w, xin, pc.cin_pad, s, 1);
    if (!rc && r1) rc = launch_nchw_to_nhwc16(res1_dev, n, cout, OH, OW, r1, pc.cout_pad, s, 1);
    if (!rc && m) rc = launch_nchw_to_nhwc16(mul_dev, n, cout, OH, OW, m, pc.cout_pad, s, 1);
    if (!rc && r2) rc = launch_nchw_to_nhwc16(res2_dev, n, cout, OH, OW, r2, pc.cout_pad, s, 1);
    // (the kernel writes the real channels of the computed positions only: pad channels and the other checkerboard half read 0)
    if (!rc) rc = launch_fill_zero(y, yf, s);
    if (!rc && y2) rc = launch_fill_zero(y2, yf, s);
    a.x = xin;
    a.w = pc.w;
    a.bias = pc.bias;
    a.y = y;
    a.N = n;
    a.H = h;
    a.W = w;
    a.xcs = pc.cin_pad;
    a.C = cin;
    a.cin_pad = pc.cin_pad;
    a.O = cout;
    a.OH = OH;
    a.OW = OW;
    a.ycs = pc.cout_pad;
    a.K = k;
    a.stride = stride;
    a.pad = pad;
    a.act = act;
    a.ckbd = ckbd;
    if (r1) a.res1 = r1, a.r1cs = pc.cout_pad;
    if (m) a.mul = m, a.mcs = pc.cout_pad;
    if (r2) a.res2 = r2, a.r2cs = pc.cout_pad;
    if (y2) a.y2 = y2, a.y2cs = pc.cout_pad;
    if (!rc) rc = launch_small_conv_ref(a, s);
    if (!rc) rc = launch_nhwc_to_nchw_clamp(y, n, cout, OH, OW, pc.cout_pad, y_dev, 0, s, 1);
    if (!rc && y2) rc = launch_nhwc_to_nchw_clamp(y2, n, cout, OH, OW, pc.cout_pad, y2_dev, 0, s, 1);
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = RGBD_EHIP;
    return rc;
}

int rgbd_ref_deconv_s2_nchw(const float* x_dev, int32_t n, int32_t cin, int32_t h, int32_t w, const float* weight, const float* bias,
                            int32_t cout, int32_t act, const int32_t* recipe, int32_t nrecipe, float* y_dev, void* stream)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);
    if (!x_dev || !weight || !y_dev || !recipe || nrecipe <= 0 || !tensor_ok(n, cin, h, w) || !tensor_ok(n, cout, 2 * (int64_t)h, 2 * (int64_t)w) ||
        cout > 65536 || (act != ACT_NONE && act != ACT_LEAKY && act != ACT_RELU))
        return RGBD_EINVAL;
    if (cin > 4096) return RGBD_EINVAL;  // (16 taps x cin_pad / 16 chunks must fit ConvArgs::split_c16)
    PackedConv shape;  // the recipe is checked against the layer's shape before anything touches the device
    shape.cin = cin, shape.cout = cout, shape.k = 5, shape.transposed = true;
    shape.cin_pad = round_up(cin, 16), shape.cout_pad = round_up(cout, 16);
    NoScratch none;
    int rc = deconv_s2_ref_run(shape, recipe, (size_t)nrecipe, nullptr, n, h, w, act, nullptr, shape.cout_pad, 0, false, nullptr, none);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    HostTensor hw, hb;
    hw.shape = {cin, cout, 5, 5};
    hw.v.assign(weight, weight + (size_t)cin * cout * 25);
    if (bias) {
        hb.shape = {cout};
        hb.v.assign(bias, bias + cout);
    }
    DevBufs b;
    DevGen gen;  // (owns the packed weights: released on every way out)
    PackedConv pc;
    rc = pack_conv(hw, bias ? &hb : nullptr, true, &pc, &gen, 1, 1);
    if (rc) return rc;
    const size_t xf = (size_t)n * h * w * pc.cin_pad, yf = (size_t)n * 4 * h * w * pc.cout_pad;
    float *xin = b.get(xf), *y = b.get(yf);
    if (!xin || !y) return RGBD_ENOMEM;
    rc = launch_nchw_to_nhwc16(x_dev, n, cin, h, w, xin, pc.cin_pad, s, 1);
    MallocScratch scratch{b};
    if (!rc) rc = deconv_s2_ref_run(pc, recipe, (size_t)nrecipe, xin, n, h, w, act, y, pc.cout_pad, 0, true, s, scratch);
    if (!rc) rc = launch_nhwc_to_nchw_clamp(y, n, cout, 2 * h, 2 * w, pc.cout_pad, y_dev, 0, s, 1);
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = RGBD_EHIP;
    return rc;
}

// ---- the single-chain pointwise and layout kernels alone (test hooks: tests/test_gpu_pointwise_forms.py) ---------------------
// Operator boundaries on the engine's own layout, like the entropy and Swin hooks: NHWC fp32 device pointers with the caller's
// channel strides, nothing staged, nothing converted.  Each checks on the host what its kernel assumes, then calls the
// launcher the engine calls.  Asynchronous on `stream` (rgbd_pw_se_gate, which uploads its weights, returns when done).
namespace {
inline bool pw_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// [n][pix][cs] holding c channels: positive extents, n within a grid's y range, a stride that holds c and keeps 16-byte
// vectors aligned, fewer than 2^31 elements
inline bool pw_tensor_ok(int64_t n, int64_t pix, int64_t c, int64_t cs)
{
    return n > 0 && n <= 65535 && pix > 0 && pix < ((int64_t)1 << 31) && c > 0 && cs >= c && cs % 4 == 0 && cs <= (1 << 20) &&
           n * pix * cs < ((int64_t)1 << 31);
}
inline bool pw_hw_ok(int64_t h, int64_t w) { return h > 0 && w > 0 && h <= 65536 && w <= 65536; }
}  // namespace

int rgbd_pw_channel_mean(const float* x_dev, int32_t N, int32_t HW, int32_t cs, int32_t C, float* mean_dev, int32_t mstride,
                         void* stream)
{
    if (!x_dev || !mean_dev || !pw_tensor_ok(N, HW, C, cs) || mstride < C || mstride % 4 || mstride > (1 << 20)) return RGBD_EINVAL;
    return launch_channel_mean_strided(x_dev, N, HW, cs, C, mean_dev, mstride, (hipStream_t)stream);
}

int rgbd_pw_se_gate(const float* mean_dev, int32_t N, int32_t C, const float* w0, const float* w1, int32_t mstride, int32_t perm,
                    float* gate_dev, void* stream)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!mean_dev || !w0 || !w1 || !gate_dev || N <= 0 || N > 65535 || C <= 0 || C % 16 || C > 65536 || mstride < C || mstride % 4 ||
        mstride > (1 << 20) || perm < 0 || perm > 1)
        return RGBD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int hidden = C / 16;
    const size_t wf = (size_t)C * hidden;
    std::vector<float> w1t(wf);
    se_pack_fc2(w1, (size_t)C, (size_t)hidden, w1t.data());
    DevBufs b;
    float *dw0 = b.get(wf), *dw1 = b.get(wf), *hid = b.get((size_t)N * hidden);
    if (!dw0 || !dw1 || !hid) return RGBD_ENOMEM;
    HIP_TRY(hipMemcpy(dw0, w0, wf * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dw1, w1t.data(), wf * sizeof(float), hipMemcpyHostToDevice));
    int rc = launch_se_fc(mean_dev, N, C, hidden, dw0, dw1, hid, gate_dev, s, mstride, perm);
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = RGBD_EHIP;
    return rc;
}

int rgbd_pw_bilinear(const float* x_dev, int32_t N, int32_t h, int32_t w, int32_t cs, float* y_dev, int32_t H, int32_t W,
                     const float* x1_dev, float* y1_dev, int32_t ref_channels, void* stream)
{
    if (!x_dev || !y_dev || !pw_hw_ok(h, w) || !pw_hw_ok(H, W) || !pw_tensor_ok(N, (int64_t)h * w, cs, cs) ||
        !pw_tensor_ok(N, (int64_t)H * W, cs, cs) || ref_channels < 0 || ref_channels > cs || !x1_dev != !y1_dev || !pw_al16(x_dev) ||
        !pw_al16(y_dev) || !pw_al16(x1_dev) || !pw_al16(y1_dev))
        return RGBD_EINVAL;
    return launch_bilinear(x_dev, N, h, w, cs, y_dev, H, W, (hipStream_t)stream, x1_dev, y1_dev, ref_channels);
}

int rgbd_pw_maxpool7s3(const float* x_dev, int32_t N, int32_t H, int32_t W, int32_t cs, float* y_dev, const float* x1_dev,
                       float* y1_dev, void* stream)
{
    if (!x_dev || !y_dev || !pw_hw_ok(H, W) || H < 7 || W < 7 || !pw_tensor_ok(N, (int64_t)H * W, cs, cs) || !x1_dev != !y1_dev ||
        !pw_al16(x_dev) || !pw_al16(y_dev) || !pw_al16(x1_dev) || !pw_al16(y1_dev))
        return RGBD_EINVAL;
    return launch_maxpool7s3(x_dev, N, H, W, cs, y_dev, (H - 7) / 3 + 1, (W - 7) / 3 + 1, (hipStream_t)stream, x1_dev, y1_dev);
}

int rgbd_pw_channel_scale(const float* x_dev, int32_t N, int32_t HW, int32_t xcs, int32_t C, const float* scale_dev, int32_t sstride,
                          int32_t mode, float* y_dev, int32_t ycs, void* stream)
{
    if (!x_dev || !scale_dev || !y_dev || !pw_tensor_ok(N, HW, C, xcs) || !pw_tensor_ok(N, HW, C, ycs) || C % 4 || sstride < C ||
        sstride % 4 || sstride > (1 << 20) || mode < 0 || mode > 1 || !pw_al16(x_dev) || !pw_al16(scale_dev) || !pw_al16(y_dev))
        return RGBD_EINVAL;
    return launch_channel_scale_to_strided(x_dev, N, HW, xcs, C, scale_dev, sstride, mode, y_dev, ycs, (hipStream_t)stream);
}

int rgbd_pw_copy_channels(const float* src_dev, int32_t scs, float* dst_dev, int32_t dcs, int32_t npix, int32_t C, void* stream)
{
    if (!src_dev || !dst_dev || !pw_tensor_ok(1, npix, C, scs) || !pw_tensor_ok(1, npix, C, dcs) || C % 4 || !pw_al16(src_dev) ||
        !pw_al16(dst_dev))
        return RGBD_EINVAL;
    return launch_copy_channels(src_dev, scs, dst_dev, dcs, npix, C, (hipStream_t)stream);
}

int rgbd_pw_im2col5s2(const float* x_dev, int32_t N, int32_t H, int32_t W, int32_t cs, int32_t C, float* y_dev, int32_t KP,
                      void* stream)
{
    if (!x_dev || !y_dev || !pw_hw_ok(H, W) || !pw_tensor_ok(N, (int64_t)H * W, C, cs) || KP <= 0 || KP % 16 || 25 * (int64_t)C > KP ||
        !pw_tensor_ok(N, (int64_t)((H + 1) / 2) * ((W + 1) / 2), KP, KP) || !pw_al16(y_dev))
        return RGBD_EINVAL;
    return launch_im2col5s2(x_dev, N, H, W, cs, C, y_dev, (H + 1) / 2, (W + 1) / 2, KP, (hipStream_t)stream);
}

int rgbd_pw_fill_zero(float* p_dev, int64_t n, void* stream)
{
    if (!p_dev || n <= 0 || n >= ((int64_t)1 << 31)) return RGBD_EINVAL;
    return launch_fill_zero(p_dev, (size_t)n, (hipStream_t)stream);
}

int rgbd_pw_nchw_to_nhwc(const float* src_dev, int32_t N, int32_t C, int32_t H, int32_t W, float* dst_dev, int32_t cs, int32_t perm,
                         void* stream)
{
    if (!src_dev || !dst_dev || !pw_hw_ok(H, W) || !pw_tensor_ok(N, (int64_t)H * W, C, cs) || perm < 0 || perm > 1 ||
        (perm && cs % 16) || !pw_al16(dst_dev))
        return RGBD_EINVAL;
    return launch_nchw_to_nhwc16(src_dev, N, C, H, W, dst_dev, cs, (hipStream_t)stream, perm);
}

int rgbd_pw_nhwc_to_nchw(const float* src_dev, int32_t N, int32_t C, int32_t H, int32_t W, int32_t cs, float* dst_dev, int32_t clamp01,
                         int32_t perm, void* stream)
{
    if (!src_dev || !dst_dev || !pw_hw_ok(H, W) || !pw_tensor_ok(N, (int64_t)H * W, C, cs) || perm < 0 || perm > 1 ||
        (perm && cs % 16) || clamp01 < 0 || clamp01 > 1)
        return RGBD_EINVAL;
    return launch_nhwc_to_nchw_clamp(src_dev, N, C, H, W, cs, dst_dev, clamp01, (hipStream_t)stream, perm);
}

// ---- the conv launchers in every form the engine issues (test hook: tests/test_gpu_convforms.py; include/rgbd_amd.h) ---------
// conv2d_nchw_impl above always builds the plainest ConvArgs.  This one builds, from the helpers the engine's planner builds
// its launches from (conv_args.h), every other form -- fused tail, lead layer, gate / skip operands, second destination,
// channel-slice placement, second operand set -- and calls launch_conv / launch_conv_fused, the functions conv_issue calls.
namespace {
// channels [off, off + c) of a tensor of `total` channels as a destination of `store` channels: in bounds, and what is
// stored past the slice lands in the buffer's own pad channels (permuted layout: whole groups of 16 only)
inline bool forms_dst_ok(int off, int c, int total, int store, bool perm)
{
    if (total <= 0 || total > 65536 || off < 0 || off % (perm ? 16 : 4) || c <= 0 || off + c > total) return false;
    if (store != c && off + c != total) return false;
    if (perm && store != round_up(c, 16)) return false;
    return off + store <= round_up(total, 16);
}
struct FormsSet {
    PackedConv pc, pc2, pc3;
    float *x = nullptr, *y = nullptr, *y2 = nullptr, *y3 = nullptr, *r1 = nullptr, *m = nullptr, *r2 = nullptr, *part = nullptr;
};
}  // namespace

int rgbd_conv_forms_nchw(const rgbd_conv_forms_desc* d, void* stream)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    // ---- host checks: nothing is allocated or launched before all of them have passed -----------------------------------------
    if (!d || d->groups < 0 || d->groups > 2) return RGBD_EINVAL;
    const int G = d->groups == 2 ? 2 : 1;
    const int n = d->n, cin = d->cin, h = d->h, w = d->w, cout = d->cout, k = d->k, stride = d->stride, pad = d->pad;
    const bool tr = d->transposed != 0, refmode = d->refmode != 0, fused = d->cout2 > 0, lead = d->cout3 > 0;
    if (!tensor_ok(n, cin, h, w) || cout <= 0 || cout > 65536 || k < 1 || k > 5 || stride < 1 || stride > 2 || pad < 0 || pad > k ||
        d->act < ACT_NONE || d->act > ACT_GELU || d->cout2 < 0 || d->cout2 > 65536 || d->cout3 < 0 || d->cout3 > 65536 ||
        (lead && !fused))
        return RGBD_EINVAL;
    // GELU is the reducer's (launch_conv): the plain form outside refmode, one destination
    const bool gelu = d->act == ACT_GELU;
    if (gelu && (fused || refmode || d->set[0].y2_dev || (d->groups == 2 && d->set[1].y2_dev))) return RGBD_EINVAL;
    if (!tr && (h + 2 * pad < k || w + 2 * pad < k)) return RGBD_EINVAL;
    int OH, OW;
    conv_out_hw(h, w, k, stride, pad, tr, &OH, &OW);
    const int cy = fused ? d->cout2 : cout;  // channels of y
    if (OH <= 0 || OW <= 0 || !tensor_ok(n, cy, OH, OW) || !tensor_ok(n, cout, OH, OW)) return RGBD_EINVAL;
    const int perm = refmode ? 1 : 0;
    const int cin_pad = round_up(cin, 16), cout_pad = round_up(cout, 16), cout2_pad = round_up(d->cout2, 16), cout3_pad = round_up(d->cout3, 16);
    // placement
    if (d->x_total <= 0 || d->x_total > 65536 || d->x_off < 0 || d->x_off % 16 || d->x_off + cin > d->x_total || !tensor_ok(n, d->x_total, h, w))
        return RGBD_EINVAL;
    const int xcs = round_up(d->x_total, 16), ycs = round_up(std::max(d->y_total, 1), 16), y2cs = round_up(std::max(d->y2_total, 1), 16),
              y3cs = round_up(std::max(d->y3_total, 1), 16);
    const int cout_store = conv_cout_store(cy, ycs);
    if (!forms_dst_ok(d->y_off, cy, d->y_total, cout_store, perm) || !tensor_ok(n, d->y_total, OH, OW)) return RGBD_EINVAL;
    const bool dup = d->set[0].y2_dev != nullptr;
    if (dup && (conv_cout_store(cy, y2cs) != cout_store || !forms_dst_ok(d->y2_off, cy, d->y2_total, cout_store, perm) ||
                !tensor_ok(n, d->y2_total, OH, OW)))
        return RGBD_EINVAL;
    if (lead && (!forms_dst_ok(d->y3_off, d->cout3, d->y3_total, cout3_pad, perm) || !tensor_ok(n, d->y3_total, OH, OW))) return RGBD_EINVAL;
    // operand sets: required pointers, and a twin for every pointer of a grouped call (conv_groups_ok's rule, on the host tensors)
    for (int g = 0; g < G; ++g) {
        const rgbd_conv_forms_ops& o = d->set[g];
        if (!o.x_dev || !o.weight || !o.y_dev || (fused && !o.w2) || (!fused && (o.w2 || o.bias2)) || (lead && (!o.w3 || !o.y3_dev)) ||
            (!lead && (o.w3 || o.bias3 || o.y3_dev)))
            return RGBD_EINVAL;
        const rgbd_conv_forms_ops& z = d->set[0];
        if (!o.bias != !z.bias || !o.bias2 != !z.bias2 || !o.bias3 != !z.bias3 || !o.res1_dev != !z.res1_dev || !o.mul_dev != !z.mul_dev ||
            !o.res2_dev != !z.res2_dev || !o.y2_dev != !z.y2_dev)
            return RGBD_EINVAL;
    }
    const rgbd_conv_forms_ops& o0 = d->set[0];
    // what the launchers refuse (launch_conv / launch_conv_fused / launch_cfg)
    ConvArgs a{};  // (what the checks decide is kept: reference-arithmetic fields, blocks, split ranges)
    a.cin_pad = cin_pad;
    a.splitk = 1;
    int cls = 0;
    const int ckbd = g_force_ckbd;
    const int nphase = tr ? stride * stride : 1, IS = tr ? 1 : stride, OS = tr ? stride : 1;
    if (ckbd && (nphase != 1 || IS != 1 || OS != 1)) return RGBD_EINVAL;
    if (refmode) {
        if (d->bias_mode < 0 || d->bias_mode > 2 || d->nblocks < 0 || d->nblocks > 256 || (d->nblocks > 0 && !d->blocks) || (tr && stride != 1))
            return RGBD_EINVAL;
        a.bias_mode = d->bias_mode;
        a.exact_math = d->flags & 1;
        if ((d->flags & 2) && d->blocks && d->nblocks > 1 && d->nblocks <= 16) {  // the blocks as split-K ranges (as conv2d_nchw_impl)
            for (int b = 0; b < d->nblocks; ++b)
                if (d->blocks[b] % 16) return RGBD_EINVAL;
            if (conv_set_split_ranges(&a, d->blocks, d->nblocks)) return RGBD_EINVAL;
            if (d->bias_mode == 1 || fused || a.split_c16[d->nblocks] != cin_pad / 16) return RGBD_EINVAL;
        } else if (d->blocks && d->nblocks == 1) {
            if (d->blocks[0] != cin) return RGBD_EINVAL;
            if (a.bias_mode == 1) a.bias_mode = 0;  // (one block: S_0 + bias is the epilogue's add)
        } else if (conv_set_blocks(&a, d->blocks, d->nblocks)) {
            return RGBD_EINVAL;
        }
        if (a.blocked && d->blocks) {  // (the table was checked against the padded width: the blocks must add up to cin itself)
            long pos = 0;
            for (int b = 0; b < d->nblocks; ++b) pos += d->blocks[b];
            if (pos != cin) return RGBD_EINVAL;
        }
    } else {
        if (d->nblocks || d->blocks || d->bias_mode || d->flags) return RGBD_EINVAL;
        if (g_force_splitk > 0 && !fused) a.splitk = std::max(1, std::min(g_force_splitk, cin_pad / 16));
    }
    if (fused) {
        if (tr || stride != 1 || k * k > 9 || cout_pad != 96 || cout2_pad % 96 || ckbd || o0.mul_dev || o0.res2_dev || dup ||
            (d->act != ACT_NONE && d->act != ACT_RELU && d->act != ACT_LEAKY) || (d->act_mid != ACT_NONE && d->act_mid != ACT_RELU))
            return RGBD_EINVAL;
        if (lead && (cout3_pad != 96 || cout2_pad % 32)) return RGBD_EINVAL;
        cls = conv_fused_plan(cout_pad, cout2_pad, k * k, n * G, OH, OW, 0);
        if (cls != 1 && cls != 2 && cls != 4) return RGBD_EINVAL;  // (0: the plan would not fuse this pair on this grid)
    } else {
        if (d->act_mid) return RGBD_EINVAL;
        if (dup && a.splitk > 1) return RGBD_EINVAL;  // the reducer has one destination
        if (a.blocked && a.splitk > 1) return RGBD_EINVAL;
    }
    if ((size_t)cout_pad * k * k * cin_pad * 4 >= ((size_t)1 << 32)) return RGBD_EINVAL;

    // ---- device side --------------------------------------------------------------------------------------------------------
    hipStream_t s = (hipStream_t)stream;
    DevBufs b;
    DevGen gen;  // (owns the packed weights: released on every way out)
    FormsSet fs[2];
    const size_t opx = (size_t)n * OH * OW;
    int rc = RGBD_OK;
    // every destination is followed by a guard band of one output row and one pixel, checked after the launch: a store predicate
    // that lets a tile run past the last image's last row or pixel is reported (RGBD_ESTATE), not left to land in foreign memory
    // (the partial planes of a split-K / GELU launch too: `px` pixels of `cs` channels, then the band)
    const std::vector<uint32_t> guard_pat((size_t)(OW + 1) * std::max(std::max(ycs, cout_pad), std::max(y2cs, y3cs)), 0xC0FFEE42u);
    auto guard_arm = [&](float* p, int cs, size_t px) {
        return hipMemcpy(p + px * cs, guard_pat.data(), (size_t)(OW + 1) * cs * 4, hipMemcpyHostToDevice) == hipSuccess ? RGBD_OK : RGBD_EHIP;
    };
    auto guard_intact = [&](const float* p, int cs, size_t px) {
        std::vector<uint32_t> back((size_t)(OW + 1) * cs);
        if (hipMemcpy(back.data(), p + px * cs, back.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return RGBD_EHIP;
        return memcmp(back.data(), guard_pat.data(), back.size() * 4) ? RGBD_ESTATE : RGBD_OK;
    };
    for (int g = 0; g < G && !rc; ++g) {
        const rgbd_conv_forms_ops& o = d->set[g];
        FormsSet& f = fs[g];
        HostTensor hw, hb;
        hw.shape = tr ? std::vector<int64_t>{cin, cout, k, k} : std::vector<int64_t>{cout, cin, k, k};
        hw.v.assign(o.weight, o.weight + (size_t)cin * cout * k * k);
        if (o.bias) hb.shape = {cout}, hb.v.assign(o.bias, o.bias + cout);
        rc = pack_conv(hw, o.bias ? &hb : nullptr, tr, &f.pc, &gen, perm, perm);
        if (!rc && fused) {
            HostTensor hw2, hb2;
            hw2.shape = {d->cout2, cout, 1, 1};
            hw2.v.assign(o.w2, o.w2 + (size_t)d->cout2 * cout);
            if (o.bias2) hb2.shape = {d->cout2}, hb2.v.assign(o.bias2, o.bias2 + d->cout2);
            rc = pack_conv(hw2, o.bias2 ? &hb2 : nullptr, false, &f.pc2, &gen, perm, perm);
        }
        if (!rc && lead) {
            HostTensor hw3, hb3;
            hw3.shape = {d->cout3, d->cout2, 1, 1};
            hw3.v.assign(o.w3, o.w3 + (size_t)d->cout3 * d->cout2);
            if (o.bias3) hb3.shape = {d->cout3}, hb3.v.assign(o.bias3, o.bias3 + d->cout3);
            rc = pack_conv(hw3, o.bias3 ? &hb3 : nullptr, false, &f.pc3, &gen, perm, perm);
        }
        if (rc) return rc;
        const int cyp = round_up(cy, 16);
        f.x = b.get((size_t)n * h * w * xcs);
        f.y = b.get((opx + OW + 1) * ycs);
        if (o.y2_dev) f.y2 = b.get((opx + OW + 1) * y2cs);
        if (lead) f.y3 = b.get((opx + OW + 1) * y3cs);
        if (o.res1_dev) f.r1 = b.get((opx + OW + 1) * cyp);  // (the same slack as behind the destinations: what is read there is not used)
        if (o.mul_dev) f.m = b.get((opx + OW + 1) * cyp);
        if (o.res2_dev) f.r2 = b.get((opx + OW + 1) * cyp);
        const bool planes = a.splitk > 1 || gelu;  // (Engine::conv_plan's partial_bytes: a GELU layer books one plane)
        if (planes) f.part = b.get(((size_t)a.splitk * opx + OW + 1) * cout_pad);
        if (!f.x || !f.y || (o.y2_dev && !f.y2) || (lead && !f.y3) || (o.res1_dev && !f.r1) || (o.mul_dev && !f.m) || (o.res2_dev && !f.r2) ||
            (planes && !f.part))
            return RGBD_ENOMEM;
        rc = guard_arm(f.y, ycs, opx);
        if (!rc && f.y2) rc = guard_arm(f.y2, y2cs, opx);
        if (!rc && f.y3) rc = guard_arm(f.y3, y3cs, opx);
        if (!rc && f.part) rc = guard_arm(f.part, cout_pad, (size_t)a.splitk * opx);
        if (!rc) rc = launch_nchw_to_nhwc16(o.x_dev, n, d->x_total, h, w, f.x, xcs, s, perm);
        if (!rc) rc = launch_nchw_to_nhwc16(o.y_dev, n, d->y_total, OH, OW, f.y, ycs, s, perm);
        if (!rc && f.y2) rc = launch_nchw_to_nhwc16(o.y2_dev, n, d->y2_total, OH, OW, f.y2, y2cs, s, perm);
        if (!rc && f.y3) rc = launch_nchw_to_nhwc16(o.y3_dev, n, d->y3_total, OH, OW, f.y3, y3cs, s, perm);
        if (!rc && f.r1) rc = launch_nchw_to_nhwc16(o.res1_dev, n, cy, OH, OW, f.r1, cyp, s, perm);
        if (!rc && f.m) rc = launch_nchw_to_nhwc16(o.mul_dev, n, cy, OH, OW, f.m, cyp, s, perm);
        if (!rc && f.r2) rc = launch_nchw_to_nhwc16(o.res2_dev, n, cy, OH, OW, f.r2, cyp, s, perm);
    }
    if (!rc) {
        const int cyp = round_up(cy, 16);
        const ConvArgs checked = a;
        auto args_of = [&](const FormsSet& f) {  // one operand set's launch, on top of what the host checks decided
            ConvArgs r = checked;
            conv_args_geometry(&r, f.pc, f.x + d->x_off, n, h, w, xcs, f.y + d->y_off, ycs, OH, OW, stride, pad);
            r.cout_store = cout_store;
            conv_args_epilogue(&r, d->act, ckbd, f.r1, cyp, f.m, cyp, f.r2, cyp, f.y2 ? f.y2 + d->y2_off : nullptr, y2cs);
            r.partial = f.part;
            if (fused) conv_args_tail(&r, f.pc2, d->act_mid, refmode);
            if (lead) conv_args_lead(&r, f.pc3, f.y3 + d->y3_off, y3cs);
            return r;
        };
        a = args_of(fs[0]);
        if (G == 2) {
            const ConvArgs q = args_of(fs[1]);
            conv_args_group1(&a, q);
            a.g1.partial = q.partial;
        }
        rc = fused ? launch_conv_fused(a, s) : launch_conv(a, s);
    }
    for (int g = 0; g < G && !rc; ++g) {
        const rgbd_conv_forms_ops& o = d->set[g];
        const FormsSet& f = fs[g];
        rc = launch_nhwc_to_nchw_clamp(f.y, n, d->y_total, OH, OW, ycs, o.y_dev, 0, s, perm);
        if (!rc && f.y2) rc = launch_nhwc_to_nchw_clamp(f.y2, n, d->y2_total, OH, OW, y2cs, o.y2_dev, 0, s, perm);
        if (!rc && f.y3) rc = launch_nhwc_to_nchw_clamp(f.y3, n, d->y3_total, OH, OW, y3cs, o.y3_dev, 0, s, perm);
    }
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = RGBD_EHIP;
    for (int g = 0; g < G && !rc; ++g) {
        const FormsSet& f = fs[g];
        rc = guard_intact(f.y, ycs, opx);
        if (!rc && f.y2) rc = guard_intact(f.y2, y2cs, opx);
        if (!rc && f.y3) rc = guard_intact(f.y3, y3cs, opx);
        if (!rc && f.part) rc = guard_intact(f.part, cout_pad, (size_t)a.splitk * opx);
    }
    return rc;
}

int rgbd_debug_force_tile(const char* cfg)
{
    snprintf(g_conv_force, sizeof(g_conv_force), "%s", cfg ? cfg : "");
    ++g_cfg_epoch;
    return RGBD_OK;
}

int rgbd_debug_tile_override(const char* csv)
{
    ++g_cfg_epoch;  // cached HIP graphs have the old kernel choices baked in
    return conv_tile_override(csv);
}

int rgbd_debug_conv_log(int32_t on) { return conv_log_enable(on); }
int64_t rgbd_debug_conv_log_read(char* buf, int64_t cap) { return conv_log_read(buf, (long)cap); }
long rgbd_debug_tile_list(int32_t blocked, char* buf, long cap) { return conv_tile_list(blocked, buf, cap); }

int rgbd_elic_set_tile_mode(rgbd_elic* m, int32_t mode)
{
    if (!m || mode < 0 || mode > 1) return RGBD_EINVAL;
    m->tile_mode = mode;
    return RGBD_OK;
}

int rgbd_debug_bench_streams(int32_t n)
{
    if (n < 1 || n > 32) return RGBD_EINVAL;
    g_bench_streams = n;
    return RGBD_OK;
}

int rgbd_debug_force_blocked(int32_t on)
{
    g_force_blocked = on ? 1 : 0;
    return RGBD_OK;
}

int rgbd_debug_force_ckbd(int32_t part)
{
    if (part < 0 || part > 2) return RGBD_EINVAL;
    g_force_ckbd = part;
    ++g_cfg_epoch;
    return RGBD_OK;
}

// -1: fuse where the plan says so (default), 0: never, 1 / 2 / 4: always, with 64 / 128 / 256-pixel tiles
int rgbd_debug_force_fuse(int32_t mode)
{
    const int lead_off = mode >= 15 ? 1 : 0;  // + 16: tails only, the next block's leading 1x1 stays a launch of its own
    if (lead_off) mode -= 16;
    if (mode != -1 && mode != 0 && mode != 1 && mode != 2 && mode != 4) return RGBD_EINVAL;
    g_fuse_force = mode;
    g_fuse_lead_off = lead_off;
    ++g_cfg_epoch;
    return RGBD_OK;
}

int rgbd_debug_fail_captures(int32_t n)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);
    if (n < 0) return RGBD_EINVAL;
    g_fail_captures = n;
    return RGBD_OK;
}

int rgbd_debug_force_pair(int32_t mode)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);
    if (mode != 0 && mode != 1) return RGBD_EINVAL;
    g_pair = mode;
    ++g_cfg_epoch;
    return RGBD_OK;
}

// 0: per-phase form, 1: sub-pixel form inside the codec (default), 2: also in rgbd_conv2d_nchw (tests)
int rgbd_debug_force_subpix(int32_t mode)
{
    if (mode < 0 || mode > 2) return RGBD_EINVAL;
    g_subpix = mode;
    ++g_cfg_epoch;
    return RGBD_OK;
}

int rgbd_debug_force_splitk(int32_t s)
{
    g_force_splitk = s;
    ++g_cfg_epoch;
    return RGBD_OK;
}

// Kernel-only timing of one conv shape on NHWC buffers (tools/conv_sweep.py); not part of the codec path.
int rgbd_conv_bench(int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t k, int32_t stride, int32_t pad,
                    int32_t transposed, int32_t with_residual, int32_t iters, float* ms_out)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!ms_out || n <= 0 || iters <= 0) return RGBD_EINVAL;
    HostTensor hw;
    hw.shape = transposed ? std::vector<int64_t>{cin, cout, k, k} : std::vector<int64_t>{cout, cin, k, k};
    hw.v.assign((size_t)cin * cout * k * k, 0.01f);
    DevBufs b;
    DevGen gen;  // (owns the packed weights: released on every way out)
    struct Sync {  // the call's events and streams: destroyed on every way out (before the buffers go)
        std::vector<hipEvent_t> ev;
        std::vector<hipStream_t> st;
        ~Sync()
        {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
            for (hipStream_t q : st)
                if (q) (void)hipStreamDestroy(q);
        }
    } sync;
    PackedConv pc;
    int rc = pack_conv(hw, nullptr, transposed != 0, &pc, &gen);
    if (rc) return rc;
    int OH, OW;
    conv_out_hw(h, w, k, stride, pad, transposed != 0, &OH, &OW);
    const size_t xf = (size_t)n * h * w * pc.cin_pad, yf = (size_t)n * OH * OW * pc.cout_pad;
    float *x = b.get(xf), *y = b.get(yf), *r = with_residual ? b.get(yf) : nullptr;
    if (!x || !y || (with_residual && !r)) return RGBD_ENOMEM;
    HIP_TRY(hipMemset(x, 0x3c, xf * sizeof(float)));  // small positive floats
    if (r) HIP_TRY(hipMemset(r, 0x3c, yf * sizeof(float)));
    ConvArgs a{};
    conv_args_geometry(&a, pc, x, n, h, w, pc.cin_pad, y, pc.cout_pad, OH, OW, stride, pad);
    conv_args_epilogue(&a, ACT_RELU, g_force_ckbd, r, pc.cout_pad, nullptr, 0, nullptr, 0, nullptr, 0);
    a.splitk = g_force_splitk > 0 ? std::min(g_force_splitk, pc.cin_pad / 16)
                                  : (g_force_splitk < 0 ? conv_splitk_for(pc.cin_pad, pc.cout_pad, conv_max_taps(a), (long)OH * OW, a.nphase) : 1);
    if (a.splitk > 1) {
        a.partial = b.get((size_t)a.splitk * yf);
        if (!a.partial) return RGBD_ENOMEM;
    }
    a.loaded = g_bench_streams > 1 ? 1 : 0;
    if (g_force_blocked && a.splitk == 1) {  // blocked accumulation: a block per 16 channels (multi-tap) / per 96 (1x1)
        std::vector<int32_t> bl;
        if (k == 1)
            for (int c = 0; c < pc.cin_pad; c += 96) bl.push_back(std::min(96, pc.cin_pad - c));
        rc = conv_set_blocks(&a, bl.empty() ? nullptr : bl.data(), (int)bl.size());
        a.bias_mode = k == 1 ? 2 : (transposed ? 0 : 1);
        if (rc) return rc;
    }
    const int S = g_bench_streams > 1 ? g_bench_streams : 0;  // loaded mode: the same launch on S streams at once
    sync.ev.resize(2 + S, nullptr);
    sync.st.resize(S, nullptr);
    hipEvent_t &e0 = sync.ev[0], &e1 = sync.ev[1];
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    rc = launch_conv(a, nullptr);
    HIP_TRY(hipDeviceSynchronize());
    float ms = 0.f;
    if (!S) {
        HIP_TRY(hipEventRecord(e0, nullptr));
        for (int i = 0; i < iters && !rc; ++i) rc = launch_conv(a, nullptr);
        HIP_TRY(hipEventRecord(e1, nullptr));
        HIP_TRY(hipEventSynchronize(e1));
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        *ms_out = ms / iters;
    } else {
        // (rgbd_debug_bench_streams) what a launch costs in CU time when the chip is shared with other engine instances, the
        // regime the job throughput is measured in
        hipStream_t* st = sync.st.data();
        hipEvent_t* done = sync.ev.data() + 2;
        for (int k = 0; k < S; ++k) {
            HIP_TRY(hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
        }
        HIP_TRY(hipEventRecord(e0, nullptr));
        for (int k = 0; k < S; ++k) HIP_TRY(hipStreamWaitEvent(st[k], e0, 0));
        for (int i = 0; i < iters && !rc; ++i)
            for (int k = 0; k < S && !rc; ++k) rc = launch_conv(a, st[k]);
        for (int k = 0; k < S; ++k) {
            HIP_TRY(hipEventRecord(done[k], st[k]));
            HIP_TRY(hipStreamWaitEvent(nullptr, done[k], 0));
        }
        HIP_TRY(hipEventRecord(e1, nullptr));
        HIP_TRY(hipEventSynchronize(e1));
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        *ms_out = ms / (iters * S);
    }
    return rc;
}

// ---- codec ------------------------------------------------------------------------------------
int rgbd_elic_create(int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, rgbd_elic** out)
{
    if (!out || !slice_ch || n_slices <= 0 || N % 16 || M % 16) return RGBD_EINVAL;
    int sum = 0;
    for (int i = 0; i < n_slices; ++i) {
        if (slice_ch[i] <= 0 || slice_ch[i] % 8) return RGBD_EINVAL;  // 16-byte channel views; STF_united has 24-wide slices
        sum += slice_ch[i];
    }
    if (sum != M) return RGBD_EINVAL;
    if (const int pr = ensure_wait_policy()) return pr;
    rgbd_elic* m = new rgbd_elic();
    m->N = N;
    m->M = M;
    m->slice_ch.assign(slice_ch, slice_ch + n_slices);
    *out = m;
    ++g_live_engines;
    return RGBD_OK;
}

static int check_ready(const rgbd_elic* m);

int rgbd_elic_create_r2d(int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, rgbd_elic** out)
{
    const int r = rgbd_elic_create(N, M, slice_ch, n_slices, out);
    if (r) return r;
    (*out)->variant = 3;
    return RGBD_OK;
}

int rgbd_elic_create_stf(int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, rgbd_elic** out)
{
    if (M != 384) return RGBD_EINVAL;  // embed_dim 48 * 8 (models/stf_united.py:640)
    const int r = rgbd_elic_create(N, M, slice_ch, n_slices, out);
    if (r) return r;
    (*out)->variant = 2;
    (*out)->refnum = false;  // (Swin transforms: channel slices that are not 16-aligned; the single-chain arithmetic of rounds 1-4)
    return RGBD_OK;
}

int rgbd_elic_create_single(int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, int32_t in_ch, rgbd_elic** out)
{
    if (in_ch < 1 || in_ch > 16) return RGBD_EINVAL;
    const int r = rgbd_elic_create(N, M, slice_ch, n_slices, out);
    if (r) return r;
    (*out)->variant = 1;
    (*out)->in_ch = in_ch;
    return RGBD_OK;
}

int rgbd_elic_create_stf_single(int32_t in_ch, rgbd_elic** out)
{
    if (in_ch < 1 || in_ch > 16) return RGBD_EINVAL;
    int32_t slices[rgbd_elic::kStfSlices];
    for (int32_t& c : slices) c = rgbd_elic::kStfSliceCh;
    const int r = rgbd_elic_create(192, rgbd_elic::kStfSlices * rgbd_elic::kStfSliceCh, slices, rgbd_elic::kStfSlices, out);  // stf.py:431,418
    if (r) return r;
    (*out)->variant = 4;
    (*out)->in_ch = in_ch;
    (*out)->refnum = false;  // (single-chain arithmetic, as STF_united; nothing sets it later: perm() is 0 in the call paths)
    return RGBD_OK;
}

// Cheng2020AnchorwithCheckerboard (models/Cheng2020withCKBD.py:46-50): M = N, one slice of N channels
int rgbd_elic_create_ckbd(int32_t N, int32_t in_ch, rgbd_elic** out)
{
    if ((N != 128 && N != 192) || (in_ch != 3 && in_ch != 1)) return RGBD_EINVAL;
    const int32_t slice = N;
    const int r = rgbd_elic_create(N, N, &slice, 1, out);
    if (r) return r;
    (*out)->variant = 5;
    (*out)->in_ch = in_ch;
    (*out)->refnum = false;  // (this family keeps the single-chain arithmetic, like STF: DESIGN.md 4a; perm() is 0, as there)
    return RGBD_OK;
}

int rgbd_elic_compress_single(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, int32_t per_image_streams,
                              void* stream)
{
    int r = check_ready(m);
    if (r) return r;
    if (!m->single() || !x_dev || B <= 0 || H <= 0 || W <= 0 || H % 64 || W % 64) return RGBD_EINVAL;
    if (const int ur = m->use_stream(stream)) return ur;
    const int per_image = (per_image_streams || B == 1) ? 1 : 0;
    char key[96];
    snprintf(key, sizeof(key), "c1|%d|%d|%d|%d", B, H, W, per_image);
    r = run_sized(m, key, [&]() { return m->run_compress(1, {x_dev}, B, H, W, per_image); });
    if (m->profile) m->profile_collect();
    return r;
}

int rgbd_elic_forward_single(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, float* xhat_dev, float* lik_y,
                             float* lik_z, void* stream)
{
    int r = check_ready(m);
    if (r) return r;
    if (!m->single() || !x_dev || !xhat_dev || !lik_y || !lik_z || B <= 0 || H <= 0 || W <= 0 || H % 64 || W % 64)
        return RGBD_EINVAL;
    if (const int ur = m->use_stream(stream)) return ur;
    char key[96];
    snprintf(key, sizeof(key), "f1|%d|%d|%d", B, H, W);
    return run_sized(m, key, [&]() { return m->run_forward(1, {x_dev}, B, H, W, {xhat_dev}, {lik_y}, {lik_z}); });
}

int rgbd_elic_decompress_single(rgbd_elic* m, const uint8_t* const* y, const int64_t* y_len, int32_t n_y,
                                const uint8_t* const* z, const int64_t* z_len, int32_t B, int32_t zh, int32_t zw,
                                float* x_dev, void* stream)
{
    int r = check_ready(m);
    if (r) return r;
    if (!m->single() || !y || !y_len || !z || !z_len || !x_dev || B <= 0 || zh <= 0 || zw <= 0) return RGBD_EINVAL;
    if (n_y != 1 && n_y != B) return RGBD_EINVAL;
    if (const int ur = m->use_stream(stream)) return ur;
    char key[96];
    snprintf(key, sizeof(key), "d1|%d|%d|%d|%d", B, zh, zw, n_y);
    r = run_sized(m, key, [&]() { return m->run_decompress(1, &y, &y_len, n_y, &z, &z_len, B, zh * 4, zw * 4, {x_dev}); });
    if (!r) r = m->wait_stream();  // (the work may sit on the engine's own stream: return when x_hat is there)
    if (m->profile && !r) m->profile_collect();
    return r;
}

// return_mid (models/elic.py:159-170, 318-329): the two calls above plus up1..up3; call shapes of their own in the graph cache
// (their bodies hold three more copies)
int rgbd_elic_forward_single_mid(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, float* xhat_dev, float* lik_y,
                                 float* lik_z, float* up1, float* up2, float* up3, void* stream)
{
    int r = check_ready(m);
    if (r) return r;
    if (m->variant != 1 || !x_dev || !xhat_dev || !lik_y || !lik_z || !up1 || !up2 || !up3 || B <= 0 || H <= 0 || W <= 0 ||
        H % 64 || W % 64)
        return RGBD_EINVAL;
    if (const int ur = m->use_stream(stream)) return ur;
    const rgbd_elic::Mid3 up = {up1, up2, up3};
    char key[96];
    snprintf(key, sizeof(key), "f1m|%d|%d|%d", B, H, W);
    return run_sized(m, key, [&]() { return m->run_forward(1, {x_dev}, B, H, W, {xhat_dev}, {lik_y}, {lik_z}, &up); });
}

int rgbd_elic_decompress_single_mid(rgbd_elic* m, const uint8_t* const* y, const int64_t* y_len, int32_t n_y,
                                    const uint8_t* const* z, const int64_t* z_len, int32_t B, int32_t zh, int32_t zw,
                                    float* x_dev, float* up1, float* up2, float* up3, void* stream)
{
    int r = check_ready(m);
    if (r) return r;
    if (m->variant != 1 || !y || !y_len || !z || !z_len || !x_dev || !up1 || !up2 || !up3 || B <= 0 || zh <= 0 || zw <= 0)
        return RGBD_EINVAL;
    if (n_y != 1 && n_y != B) return RGBD_EINVAL;
    if (const int ur = m->use_stream(stream)) return ur;
    const rgbd_elic::Mid3 up = {up1, up2, up3};
    char key[96];
    snprintf(key, sizeof(key), "d1m|%d|%d|%d|%d", B, zh, zw, n_y);
    r = run_sized(m, key, [&]() { return m->run_decompress(1, &y, &y_len, n_y, &z, &z_len, B, zh * 4, zw * 4, {x_dev}, nullptr, &up); });
    if (!r) r = m->wait_stream();
    if (m->profile && !r) m->profile_collect();
    return r;
}

// Spatial_aligner alone (modules/transform/spatialAligner.py:341-390): embed_dim 96, 3 heads, 4x4 windows
int rgbd_aligner_create(int32_t in_ch, int32_t out_ch, rgbd_elic** out)
{
    if (!out || in_ch < 1 || in_ch > 1024 || out_ch < 1 || out_ch > 1024) return RGBD_EINVAL;
    const int32_t slice = 96;
    const int r = rgbd_elic_create(96, 96, &slice, 1, out);
    if (r) return r;
    (*out)->variant = 6;
    (*out)->in_ch = in_ch;
    (*out)->out_ch = out_ch;
    (*out)->refnum = false;  // (a float block behind the entropy decoder: the single-chain arithmetic of the Swin path)
    return RGBD_OK;
}

int rgbd_aligner_forward(rgbd_elic* m, const float* x_dev, const float* guided_dev, int32_t B, int32_t H, int32_t W,
                         float* out_dev, void* stream)
{
    if (!m || m->variant != 6) return RGBD_EINVAL;
    if (!m->finalized) return RGBD_ESTATE;
    if (!x_dev || !guided_dev || !out_dev || B <= 0 || H <= 0 || W <= 0 || H % 8 || W % 8) return RGBD_EINVAL;
    if (const int ur = m->use_stream(stream)) return ur;
    char key[96];
    snprintf(key, sizeof(key), "al|%d|%d|%d", B, H, W);
    return run_sized(m, key, [&]() { return m->run_aligner(x_dev, guided_dev, B, H, W, out_dev); });
}

// The attention contexts of MLIC++ alone (modules/transform/context.py): handles of the aligner's kind (no codec, no tables)
static int context_create(int variant, int32_t dim, int32_t out_ch, int32_t heads, rgbd_elic** out)
{
    const int32_t slice = 96;
    const int r = rgbd_elic_create(96, 96, &slice, 1, out);
    if (r) return r;
    (*out)->variant = variant;
    (*out)->in_ch = dim;
    (*out)->out_ch = out_ch;
    (*out)->ctx_heads = heads;
    (*out)->refnum = false;  // the single-chain arithmetic of the Swin path
    return RGBD_OK;
}

int rgbd_local_context_create(int32_t dim, rgbd_elic** out)
{
    if (!out || dim != 32) return RGBD_EINVAL;  // window 5, 2 heads of 16: the one form MLIC++ builds (context_attn.hip)
    return context_create(7, dim, 2 * dim, 2, out);
}

int rgbd_linear_inter_create(int32_t dim, int32_t out_dim, int32_t heads, rgbd_elic** out)
{
    if (!out || heads < 1 || dim < 1 || dim > 1024 || dim % heads || (dim / heads != 16 && dim / heads != 32) || out_dim < 32 ||
        out_dim > 1024 || out_dim % 32)
        return RGBD_EINVAL;
    return context_create(8, dim, out_dim, heads, out);
}

int rgbd_linear_intra_create(int32_t dim, int32_t heads, rgbd_elic** out)
{
    if (!out || heads < 1 || dim < 1 || dim > 1024 || dim % heads || (dim / heads != 16 && dim / heads != 32)) return RGBD_EINVAL;
    return context_create(9, dim, 2 * dim, heads, out);
}

static int context_forward(rgbd_elic* m, int variant, const float* x1_dev, const float* x2_dev, int32_t B, int32_t H, int32_t W,
                           float* out_dev, void* stream)
{
    if (!m || m->variant != variant) return RGBD_EINVAL;
    if (!m->finalized) return RGBD_ESTATE;
    if (!x1_dev || (variant == 9 && !x2_dev) || !out_dev || B <= 0 || H <= 0 || W <= 0 || (variant == 9 && (W & 1)) ||
        (int64_t)B * H * W > 0x7fffffff)
        return RGBD_EINVAL;
    if (const int ur = m->use_stream(stream)) return ur;
    char key[96];
    snprintf(key, sizeof(key), "cx%d|%d|%d|%d", variant, B, H, W);
    return run_sized(m, key, [&]() { return m->run_context(x1_dev, x2_dev, B, H, W, out_dev); });
}

int rgbd_local_context_forward(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, float* out_dev, void* stream)
{
    return context_forward(m, 7, x_dev, nullptr, B, H, W, out_dev, stream);
}

int rgbd_linear_inter_forward(rgbd_elic* m, const float* x1_dev, int32_t B, int32_t H, int32_t W, float* out_dev, void* stream)
{
    return context_forward(m, 8, x1_dev, nullptr, B, H, W, out_dev, stream);
}

int rgbd_linear_intra_forward(rgbd_elic* m, const float* x1_dev, const float* x2_dev, int32_t B, int32_t H, int32_t W,
                              float* out_dev, void* stream)
{
    return context_forward(m, 9, x1_dev, x2_dev, B, H, W, out_dev, stream);
}

int rgbd_elic_clone_shared(const rgbd_elic* src, rgbd_elic** out)
{
    if (!src || !out || !src->finalized) return RGBD_EINVAL;
    rgbd_elic* m = new rgbd_elic();
    m->N = src->N;
    m->M = src->M;
    m->slice_ch = src->slice_ch;
    m->variant = src->variant;
    m->in_ch = src->in_ch;
    m->out_ch = src->out_ch;
    m->ctx_heads = src->ctx_heads;
    m->refnum = src->refnum;
    m->ref_threads = src->ref_threads;
    m->ref_tab = src->ref_tab;
    m->convs = src->convs;    // device pointers are shared, read-only; the generations below keep them alive
    m->dense = src->dense;
    m->gen_w = src->gen_w;
    for (int i = 0; i < 4; ++i) m->tables[i] = src->tables[i];
    m->scale_table = src->scale_table;
    m->scale_tab = src->scale_tab;
    m->gen_scale = src->gen_scale;
    m->finalized = true;
    m->is_clone = true;
    *out = m;
    ++g_live_engines;
    return RGBD_OK;
}

void rgbd_elic_destroy(rgbd_elic* m)
{
    const bool dbg = g_dbg_destroy;
    if (dbg) fprintf(stderr, "[destroy %p] wait lock\n", (void*)m);
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!m) return;
    if (dbg) fprintf(stderr, "[destroy %p] locked, graphs %zu\n", (void*)m, m->graphs.size());
    // weights, tables and the scale table belong to shared generations (DevGen) that go when their last user does
    m->graphs_invalidate();
    if (dbg) fprintf(stderr, "[destroy %p] graphs gone\n", (void*)m);
    if (dbg) {
        std::lock_guard<std::mutex> g(g_live_mu);
        g_live_streams.erase(m);
    }
    {
        HangWatch w("hipFree(arena) in rgbd_elic_destroy", 20, true);
        if (m->arena.base) (void)hipFree(m->arena.base);
    }
    if (dbg) fprintf(stderr, "[destroy %p] arena freed\n", (void*)m);
    if (m->pin) (void)hipHostFree(m->pin);
    if (m->res_pin) (void)hipHostFree(m->res_pin);
    if (m->pin_ev) (void)hipEventDestroy(m->pin_ev);
    if (m->done_ev) (void)hipEventDestroy(m->done_ev);
    for (hipEvent_t e : m->ev_pool) (void)hipEventDestroy(e);
    if (dbg) fprintf(stderr, "[destroy %p] events/streams gone\n", (void*)m);
    delete m;
    --g_live_engines;
    if (dbg) fprintf(stderr, "[destroy] done\n");
}

int rgbd_elic_set_tensor(rgbd_elic* m, const char* name, const float* data, const int64_t* shape, int32_t ndim)
{
    if (!m || !name || !data || !shape || ndim < 1 || ndim > 4) return RGBD_EINVAL;
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] <= 0) return RGBD_EINVAL;
        t.shape.push_back(shape[i]);
        n *= (size_t)shape[i];
    }
    t.v.assign(data, data + n);
    m->raw[name] = std::move(t);
    m->finalized = false;
    return RGBD_OK;
}

int rgbd_elic_set_tables(rgbd_elic* m, int32_t which, const int32_t* cdf, int32_t cdf_stride, const int32_t* cdf_sizes,
                         const int32_t* offsets, int32_t n_cdf)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!m || which < 0 || which > 3) return RGBD_EINVAL;
    TableSet fresh;
    const int r = build_tables(cdf, cdf_stride, cdf_sizes, offsets, n_cdf, &fresh);
    if (r) {
        if (fresh.blob) (void)hipFree(fresh.blob);
        return r;
    }
    fresh.hold = std::make_shared<DevGen>();
    fresh.hold->p.push_back(fresh.blob);
    m->tables[which] = fresh;  // the previous blob goes when no clone points at it any more
    m->graphs_invalidate();
    return RGBD_OK;
}

int rgbd_elic_set_scale_table(rgbd_elic* m, const float* table, int32_t n)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!m || !table || n != 64) return RGBD_EINVAL;
    float* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, 64 * sizeof(float)));
    auto g = std::make_shared<DevGen>();
    g->p.push_back(d);
    HIP_TRY(hipMemcpy(d, table, 64 * sizeof(float), hipMemcpyHostToDevice));
    m->scale_table = d;
    memcpy(m->scale_tab.v, table, sizeof(m->scale_tab.v));
    m->gen_scale = g;
    m->graphs_invalidate();
    return RGBD_OK;
}

static bool ends_with(const std::string& s, const char* suf)
{
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

int rgbd_elic_set_ref_blocks(rgbd_elic* m, int32_t kind, int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t batch,
                             const int32_t* blocks, int32_t nblocks)
{
    if (m && kind == 4 && blocks && nblocks == 1 && blocks[0] >= 1 && blocks[0] <= 4096) {  // CPU threads of the reference run
        m->ref_threads = blocks[0];
        m->graphs_invalidate();
        return RGBD_OK;
    }
    if (!m || !blocks || nblocks <= 0 || nblocks > (kind >= 2 ? 65536 : 64) || kind < 0 || kind > 3) return RGBD_EINVAL;
    int sum = 0;
    for (int i = 0; i < nblocks; ++i) {
        if (kind == 3 ? blocks[i] < 0 : (kind == 2 ? (blocks[i] < 0 || blocks[i] > 2) : blocks[i] <= 0)) return RGBD_EINVAL;
        sum += blocks[i];
    }
    if (kind == 0 && sum != cin) return RGBD_EINVAL;
    if (kind == 1 && nblocks > 16) return RGBD_EINVAL;
    if (kind == 2 && nblocks != cout) return RGBD_EINVAL;  // (one class per output row)
    m->ref_tab->blocks[{kind, cin, cout, h, w, batch}] = std::vector<int>(blocks, blocks + nblocks);
    m->graphs_invalidate();
    return RGBD_OK;
}

int rgbd_elic_get_refnum(const rgbd_elic* m) { return m ? (m->refnum ? 1 : 0) : RGBD_EINVAL; }
int rgbd_elic_ref_table_misses(const rgbd_elic* m) { return m ? m->ref_tab->misses : RGBD_EINVAL; }

int rgbd_elic_finalize(rgbd_elic* m)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!m) return RGBD_EINVAL;
    // a shared-weight clone has no host tensors of its own: re-finalising it would only drop the weights it borrows
    if (m->is_clone && m->raw.empty()) return RGBD_ESTATE;
    // the new weights are packed into a fresh generation and swapped in at the end; the old generation is released
    // here but lives on for as long as a clone still points into it (no use-after-free between parent and clones)
    auto gen = std::make_shared<DevGen>();
    std::map<std::string, PackedConv> convs;
    std::map<std::string, float*> dense;
    auto dev_copy = [&](const float* src, size_t n, float** out) -> int {
        float* d = nullptr;
        HIP_TRY(hipMalloc((void**)&d, n * sizeof(float)));
        gen->p.push_back(d);
        HIP_TRY(hipMemcpy(d, src, n * sizeof(float), hipMemcpyHostToDevice));
        *out = d;
        return RGBD_OK;
    };
    for (auto& kv : m->raw) {
        const std::string& name = kv.first;
        const HostTensor& t = kv.second;
        if (ends_with(name, "recovery.weight") && t.shape.size() == 4 && t.shape[2] == 2 && t.shape[3] == 2) {
            // Spatial_aligner.recovery = ConvTranspose2d(96, out, 2, 2) (spatialAligner.py:372-374): its taps do not overlap, so
            // it is a 1x1 convolution to output channel co * 4 + dy * 2 + dx followed by a pixel shuffle (spatial_aligner()).
            // Packed in plain channel order: the aligner runs the single-chain arithmetic.
            const int ci_n = (int)t.shape[0], co_n = (int)t.shape[1];
            HostTensor w1, b1;
            w1.shape = {4 * co_n, ci_n, 1, 1};
            w1.v.resize((size_t)4 * co_n * ci_n);
            for (int ci = 0; ci < ci_n; ++ci)
                for (int co = 0; co < co_n; ++co)
                    for (int tap = 0; tap < 4; ++tap) w1.v[(size_t)(co * 4 + tap) * ci_n + ci] = t.v[((size_t)ci * co_n + co) * 4 + tap];
            auto bit = m->raw.find(name.substr(0, name.size() - 6) + "bias");
            if (bit != m->raw.end()) {
                if ((int)bit->second.v.size() != co_n) return RGBD_EINVAL;
                b1.shape = {4 * co_n};
                b1.v.resize((size_t)4 * co_n);
                for (int i = 0; i < 4 * co_n; ++i) b1.v[i] = bit->second.v[i / 4];
            }
            PackedConv pc;
            const int r = pack_conv(w1, bit == m->raw.end() ? nullptr : &b1, false, &pc, gen.get(), 0, 0);
            if (r) return r;
            convs[name] = pc;
        } else if (m->variant >= 7 && ends_with(name, ".weight") && t.shape.size() == 4 &&
                   (name == "fusion.weight" || (t.shape[1] == 1 && t.shape[2] == 3 && t.shape[3] == 3))) {
            // the contexts of MLIC++: LocalContext.fusion (read by the attention launch in the reference's [2C][C][5][5]
            // layout) and the depthwise 3x3 layers ([C][1][3][3]) go to the device as they are, with their biases
            auto bit = m->raw.find(name.substr(0, name.size() - 6) + "bias");
            if (bit == m->raw.end() || (int64_t)bit->second.v.size() != t.shape[0]) return RGBD_EINVAL;
            float *dw = nullptr, *db = nullptr;
            if (const int r = dev_copy(t.v.data(), t.v.size(), &dw)) return r;
            if (const int r = dev_copy(bit->second.v.data(), bit->second.v.size(), &db)) return r;
            dense[name] = dw;
            dense[bit->first] = db;
        } else if (ends_with(name, ".weight") && t.shape.size() == 4) {
            // ConvTranspose2d layers of this model: g_s stages 1/6/12/17 and the h_s deconvs
            // (single-modal ELIC: g_s stages 1/5/10/14 and h_s.increase.*; stage numbers that are not a bare
            //  "<stage>.weight" in the other variant belong to blocks with sub-names, so the union is unambiguous)
            bool transposed = name.find(".deconv.") != std::string::npos || name.rfind("h_s.increase.", 0) == 0;
            if (name.rfind("g_s.", 0) == 0)
                for (const char* suf : {"_transform.1.weight", "_transform.6.weight", "_transform.12.weight",
                                        "_transform.17.weight", "_transform.5.weight", "_transform.10.weight",
                                        "_transform.14.weight"})
                    transposed = transposed || ends_with(name, suf);
            const std::string bname = name.substr(0, name.size() - 6) + "bias";
            auto bit = m->raw.find(bname);
            PackedConv pc;
            // refnum: activations store their channels permuted (rgbd_cperm) -- except the network's input (read channel by
            // channel by the K-packing gather) and its output images (<= 4 channels, converted straight to NCHW)
            const int pm = m->perm();
            const int k0 = (int)t.shape[2];
            const int cin0 = transposed ? (int)t.shape[0] : (int)t.shape[1], cout0 = transposed ? (int)t.shape[1] : (int)t.shape[0];
            const bool image_in = !transposed && cin0 <= 3 && k0 == 5, image_out = transposed && cout0 <= 4 && k0 == 5;
            const HostTensor* src = &t;
            HostTensor masked;
            if (m->variant == 5 && name == "context_prediction.weight") {
                // CheckerboardContext (Cheng2020withCKBD.py:28-35): the state_dict holds the unmasked weight, the reference
                // multiplies it by the mask at every call; only the taps with (ky + kx) odd survive
                masked = t;
                const size_t kk = (size_t)k0 * k0;
                for (size_t i = 0; i < masked.v.size(); ++i) {
                    const size_t tap = i % kk;
                    if (!((tap / k0 + tap % k0) & 1)) masked.v[i] = 0.f;
                }
                src = &masked;
            }
            const int r = pack_conv(*src, bit == m->raw.end() ? nullptr : &bit->second, transposed, &pc, gen.get(), image_in ? 0 : pm,
                                    image_out ? 0 : pm);
            if (r) return r;
            convs[name] = pc;
            if (m->variant == 5 && name == "entropy_parameters.0.weight") {
                // the anchor pass (Cheng2020withCKBD.py:122-123) feeds zeros into the context half of this layer's input
                // channels [ctx 2M | hyper 2M]: the same layer on the hyper half alone
                const int half = cin0 / 2;
                HostTensor hw;
                hw.shape = {cout0, half, 1, 1};
                hw.v.resize((size_t)cout0 * half);
                for (int co = 0; co < cout0; ++co)
                    for (int ci = 0; ci < half; ++ci) hw.v[(size_t)co * half + ci] = t.v[(size_t)co * cin0 + half + ci];
                PackedConv ph;
                const int r5 = pack_conv(hw, bit == m->raw.end() ? nullptr : &bit->second, false, &ph, gen.get(), 0, 0);
                if (r5) return r5;
                convs["entropy_parameters.0.hyper.weight"] = ph;
            }
            if (!transposed && pc.cin <= 3 && pc.k == 5) {  // the image-consuming layer: also as a 1x1 over a K-packed input
                PackedConv pk;
                const int r4 = pack_kpack(t, bit == m->raw.end() ? nullptr : &bit->second, &pk, gen.get(), pm);
                if (r4) return r4;
                convs[name.substr(0, name.size() - 6) + "kpack.weight"] = pk;
            }
            if (transposed && pc.cout <= 4 && pc.k == 5) {  // the image-producing layer: also in its sub-pixel form
                PackedConv ps;
                const int r3 = pack_subpix(t, bit == m->raw.end() ? nullptr : &bit->second, &ps, gen.get(), pm);
                if (r3) return r3;
                convs[name.substr(0, name.size() - 6) + "subpix.weight"] = ps;
            }
        } else if (ends_with(name, ".gamma") && t.shape.size() == 2 && t.shape[0] == t.shape[1]) {
            // GDN / IGDN (layers/gdn.py): NonNegativeParametrizer.forward applied once here, in fp32; packed for gdn.hip
            const std::string bname = name.substr(0, name.size() - 5) + "beta";
            auto bit = m->raw.find(bname);
            const int C = (int)t.shape[0];
            if (bit == m->raw.end() || (int)bit->second.v.size() != C || C > 512) return RGBD_EINVAL;
            std::vector<float> hb, hg;
            gdn_pack(bit->second.v.data(), t.v.data(), C, &hb, &hg);
            float *db = nullptr, *dg = nullptr;
            if (const int r = dev_copy(hb.data(), hb.size(), &db)) return r;
            if (const int r = dev_copy(hg.data(), hg.size(), &dg)) return r;
            dense[bname] = db;
            dense[name] = dg;
        } else if (ends_with(name, ".weight") && t.shape.size() == 2) {
            // SE_Block linears; fc.2 ([C][hidden]) is kept transposed so the gate kernel reads it coalesced
            std::vector<float> hv = t.v;
            if (m->refnum && (ends_with(name, ".fc.0.weight") || ends_with(name, ".fc.2.weight"))) {
                // the reference's Linear on one vector: per-row accumulation class, measured per layer shape
                const int J = (int)t.shape[0], K = (int)t.shape[1];
                auto ct = m->ref_tab->blocks.find({2, K, J, 0, 0, 1});
                if (ct != m->ref_tab->blocks.end() && (int)ct->second.size() == J) {
                    float* dcls = nullptr;
                    if (const int r = dev_copy(reinterpret_cast<const float*>(ct->second.data()), (size_t)J, &dcls)) return r;
                    dense[name + ".rowclass"] = dcls;
                }
            }
            if (ends_with(name, ".fc.2.weight") && !m->refnum) se_pack_fc2(t.v.data(), (size_t)t.shape[0], (size_t)t.shape[1], hv.data());
            float* d = nullptr;
            if (const int r = dev_copy(hv.data(), hv.size(), &d)) return r;
            dense[name] = d;
        } else if ((t.shape.size() == 1 && (name.find(".norm") != std::string::npos || (m->variant == 7 && name.rfind("norm", 0) == 0))) ||
                   ends_with(name, "relative_position_bias_table") || (m->variant == 7 && name == "relative_position_table")) {
            // Swin LayerNorm affine parameters and relative position bias tables: plain device arrays
            float* d = nullptr;
            if (const int r = dev_copy(t.v.data(), t.v.size(), &d)) return r;
            dense[name] = d;
        } else if (ends_with(name, "entropy_bottleneck.quantiles")) {
            // medians = quantiles[:, 0, 1]  (entropy_models.py:316-318)
            const int C = (int)t.shape[0];
            std::vector<float> med(C);
            for (int c = 0; c < C; ++c) med[c] = t.v[(size_t)c * 3 + 1];
            float* d = nullptr;
            if (const int r = dev_copy(med.data(), (size_t)C, &d)) return r;
            dense[name.substr(0, name.size() - 9) + "medians"] = d;
            // softplus(matrix_i) / bias_i / tanh(factor_i) per channel for the eval-mode likelihood (58 floats/channel)
            const std::string pre = name.substr(0, name.size() - 9);
            std::vector<float> prm((size_t)C * 58, 0.f);
            const int fi[6] = {1, 3, 3, 3, 3, 1};
            const float *mat[5] = {}, *bias[5] = {}, *fac[4] = {};
            bool ok = true;
            for (int i = 0; i < 5 && ok; ++i) {
                auto mi = m->raw.find(pre + "_matrix" + std::to_string(i));
                auto bi = m->raw.find(pre + "_bias" + std::to_string(i));
                auto fa = i < 4 ? m->raw.find(pre + "_factor" + std::to_string(i)) : m->raw.end();
                if (mi == m->raw.end() || bi == m->raw.end() || (i < 4 && fa == m->raw.end())) {
                    ok = false;
                    break;
                }
                const size_t no = (size_t)fi[i + 1], ni = (size_t)fi[i];
                if (mi->second.v.size() != C * no * ni || bi->second.v.size() != C * no || (i < 4 && fa->second.v.size() != C * no))
                    return RGBD_EINVAL;
                mat[i] = mi->second.v.data();
                bias[i] = bi->second.v.data();
                if (i < 4) fac[i] = fa->second.v.data();
            }
            if (ok) {
                eb_pack_cumulative(mat, bias, fac, C, prm.data());
                float* dp = nullptr;
                if (const int r = dev_copy(prm.data(), prm.size(), &dp)) return r;
                dense[pre + "cumulative"] = dp;
            }
        }
    }
    m->convs.swap(convs);
    m->dense.swap(dense);
    m->gen_w = gen;
    m->graphs_invalidate();
    m->finalized = true;
    return RGBD_OK;
}

static int check_ready(const rgbd_elic* m)
{
    if (m && m->variant >= 6) return RGBD_EINVAL;  // a Spatial_aligner or context handle has no codec calls
    if (!m || !m->finalized || !m->scale_table) return RGBD_ESTATE;
    for (int i = 0; i < 4; ++i)
        if (!m->tables[i].ready && !(m->single() && (i & 1))) return RGBD_ESTATE;  // single-modal: slots 0 and 2
    return RGBD_OK;
}

int rgbd_elic_compress(rgbd_elic* m, const float* rgb_dev, const float* depth_dev, int32_t B, int32_t H, int32_t W,
                       int32_t per_image_streams, void* stream)
{
    int r = check_ready(m);
    if (r) return r;
    if (!rgb_dev || !depth_dev || B <= 0 || H <= 0 || W <= 0 || H % 64 || W % 64) return RGBD_EINVAL;
    if (const int ur = m->use_stream(stream)) return ur;
    const int per_image = (per_image_streams || B == 1) ? 1 : 0;
    char key[96];
    snprintf(key, sizeof(key), "c|%d|%d|%d|%d", B, H, W, per_image);
    r = run_sized(m, key, [&]() { return m->run_compress(2, {rgb_dev, depth_dev}, B, H, W, per_image); });
    if (m->profile) m->profile_collect();  // run_compress ends with a stream synchronise
    return r;
}

int rgbd_elic_forward(rgbd_elic* m, const float* rgb_dev, const float* depth_dev, int32_t B, int32_t H, int32_t W,
                      float* xr_dev, float* xd_dev, float* lik_y_rgb, float* lik_y_depth, float* lik_z_rgb,
                      float* lik_z_depth, void* stream)
{
    int r = check_ready(m);
    if (r) return r;
    if (!rgb_dev || !depth_dev || !xr_dev || !xd_dev || !lik_y_rgb || !lik_y_depth || !lik_z_rgb || !lik_z_depth || B <= 0 ||
        H <= 0 || W <= 0 || H % 64 || W % 64)
        return RGBD_EINVAL;
    if (const int ur = m->use_stream(stream)) return ur;
    char key[96];
    snprintf(key, sizeof(key), "f|%d|%d|%d", B, H, W);
    return run_sized(m, key, [&]() {
        return m->run_forward(2, {rgb_dev, depth_dev}, B, H, W, {xr_dev, xd_dev}, {lik_y_rgb, lik_y_depth},
                              {lik_z_rgb, lik_z_depth});
    });
}

int rgbd_elic_stream_count(const rgbd_elic* m, int32_t modality, int32_t kind)
{
    if (!m || modality < 0 || modality > 1 || kind < 0 || kind > 1) return RGBD_EINVAL;
    return (int)m->streams[modality][kind].size();
}

int rgbd_elic_stream(const rgbd_elic* m, int32_t modality, int32_t kind, int32_t index, const uint8_t** data,
                     int64_t* nbytes)
{
    if (!m || !data || !nbytes || modality < 0 || modality > 1 || kind < 0 || kind > 1) return RGBD_EINVAL;
    const auto& v = m->streams[modality][kind];
    if (index < 0 || index >= (int)v.size()) return RGBD_EINVAL;
    *data = v[index].data();
    *nbytes = (int64_t)v[index].size();
    return RGBD_OK;
}

int rgbd_elic_decompress(rgbd_elic* m, const uint8_t* const* y_rgb, const int64_t* y_rgb_len, int32_t n_y,
                         const uint8_t* const* y_depth, const int64_t* y_depth_len, const uint8_t* const* z_rgb,
                         const int64_t* z_rgb_len, const uint8_t* const* z_depth, const int64_t* z_depth_len, int32_t B,
                         int32_t zh, int32_t zw, float* xr_dev, float* xd_dev, void* stream)
{
    int r = check_ready(m);
    if (r) return r;
    if (!y_rgb || !y_depth || !z_rgb || !z_depth || !xr_dev || !xd_dev || B <= 0 || zh <= 0 || zw <= 0) return RGBD_EINVAL;
    if (n_y != 1 && n_y != B) return RGBD_EINVAL;
    if (const int ur = m->use_stream(stream)) return ur;
    const uint8_t* const* ys[2] = {y_rgb, y_depth};
    const int64_t* yl[2] = {y_rgb_len, y_depth_len};
    const uint8_t* const* zs[2] = {z_rgb, z_depth};
    const int64_t* zl[2] = {z_rgb_len, z_depth_len};
    char key[96];
    snprintf(key, sizeof(key), "d|%d|%d|%d|%d", B, zh, zw, n_y);
    r = run_sized(m, key, [&]() { return m->run_decompress(2, ys, yl, n_y, zs, zl, B, zh * 4, zw * 4, {xr_dev, xd_dev}); });
    // the caller's wait for x_hat happens here, on an event the host thread sleeps on (a pooled rank has 16 of them)
    if (!r) r = m->wait_stream();
    if (m->profile && !r) m->profile_collect();
    return r;
}

int rgbd_elic_compress_united(rgbd_elic* m, const float* y_rgb_dev, const float* hyper_rgb_dev, const float* y_depth_dev,
                              const float* hyper_depth_dev, int32_t B, int32_t h, int32_t w, int32_t per_image_streams,
                              void* stream)
{
    int r = check_ready(m);
    if (r) return r;
    if (!y_rgb_dev || !hyper_rgb_dev || !y_depth_dev || !hyper_depth_dev || B <= 0 || h <= 0 || w <= 0 || (w & 1))
        return RGBD_EINVAL;
    if (const int ur = m->use_stream(stream)) return ur;
    const int per_image = (per_image_streams || B == 1) ? 1 : 0;
    rgbd_elic::Latents lat = {{y_rgb_dev, y_depth_dev}, {hyper_rgb_dev, hyper_depth_dev}, {nullptr, nullptr}};
    char key[96];
    snprintf(key, sizeof(key), "cu|%d|%d|%d|%d", B, h, w, per_image);
    r = run_sized(m, key, [&]() { return m->run_compress(2, {}, B, h * 16, w * 16, per_image, &lat); });
    if (m->profile) m->profile_collect();
    return r;
}

int rgbd_elic_decompress_united(rgbd_elic* m, const uint8_t* const* y_rgb, const int64_t* y_rgb_len, int32_t n_y,
                                const uint8_t* const* y_depth, const int64_t* y_depth_len, const float* hyper_rgb_dev,
                                const float* hyper_depth_dev, int32_t B, int32_t h, int32_t w, float* yhat_rgb_dev,
                                float* yhat_depth_dev, void* stream)
{
    int r = check_ready(m);
    if (r) return r;
    if (!y_rgb || !y_depth || !hyper_rgb_dev || !hyper_depth_dev || !yhat_rgb_dev || !yhat_depth_dev || B <= 0 || h <= 0 ||
        w <= 0 || (w & 1))
        return RGBD_EINVAL;
    if (n_y != 1 && n_y != B) return RGBD_EINVAL;
    if (const int ur = m->use_stream(stream)) return ur;
    const uint8_t* const* ys[2] = {y_rgb, y_depth};
    const int64_t* yl[2] = {y_rgb_len, y_depth_len};
    const uint8_t* const* zs[2] = {nullptr, nullptr};
    const int64_t* zl[2] = {nullptr, nullptr};
    rgbd_elic::Latents lat = {{nullptr, nullptr}, {hyper_rgb_dev, hyper_depth_dev}, {yhat_rgb_dev, yhat_depth_dev}};
    char key[96];
    snprintf(key, sizeof(key), "du|%d|%d|%d|%d", B, h, w, n_y);
    r = run_sized(m, key, [&]() { return m->run_decompress(2, ys, yl, n_y, zs, zl, B, h, w, {}, &lat); });
    if (!r) r = m->wait_stream();
    if (m->profile && !r) m->profile_collect();
    return r;
}

int64_t rgbd_elic_workspace_bytes(const rgbd_elic* m) { return m ? (int64_t)m->arena.cap : -1; }

int rgbd_elic_graph_count(const rgbd_elic* m)
{
    if (!m) return RGBD_EINVAL;
    int n = 0;
    for (const auto& kv : m->graphs) n += kv.second.exec ? 1 : 0;
    return n;
}

int rgbd_elic_set_profile(rgbd_elic* m, int32_t on)
{
    if (!m) return RGBD_EINVAL;
    m->profile = on != 0;
    m->profile_keys = on == 2;
    m->ev_used = 0;
    m->prof_flops = 0.0;
    m->prof_flops_exec = 0.0;
    m->prof_ms = 0.0;
    m->prof_launches = 0;
    m->prof_layers.clear();
    m->prof_counts.clear();
    m->ev_names.clear();
    return RGBD_OK;
}

int rgbd_elic_profile_dump(rgbd_elic* m, const char* path)
{
    if (!m || !path) return RGBD_EINVAL;
    FILE* f = fopen(path, "w");
    if (!f) return RGBD_EINVAL;
    fprintf(f, "layer,launches,ms,gflop,tflops,gflop_executed,tflops_executed\n");
    for (const auto& kv : m->prof_layers)
        fprintf(f, "%s,%d,%.4f,%.3f,%.2f,%.3f,%.2f\n", kv.first.c_str(), m->prof_counts[kv.first], kv.second.first,
                kv.second.second / 1e9, kv.second.first > 0 ? kv.second.second / kv.second.first / 1e9 : 0.0,
                kv.second.exec / 1e9, kv.second.first > 0 ? kv.second.exec / kv.second.first / 1e9 : 0.0);
    fclose(f);
    return RGBD_OK;
}

int rgbd_elic_profile_read(rgbd_elic* m, double* conv_ms, int64_t* launches, double* flops)
{
    if (!m || !conv_ms || !launches || !flops) return RGBD_EINVAL;
    *conv_ms = m->prof_ms;
    *launches = m->prof_launches;
    *flops = m->prof_flops;
    return RGBD_OK;
}

int rgbd_elic_profile_read_executed(rgbd_elic* m, double* flops_executed)
{
    if (!m || !flops_executed) return RGBD_EINVAL;
    *flops_executed = m->prof_flops_exec;
    return RGBD_OK;
}

int rgbd_elic_debug_tensor(rgbd_elic* m, const char* name, float* data, int64_t cap_floats, int32_t* shape_out)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!m || !name || !shape_out) return RGBD_EINVAL;
    auto it = m->named.find(name);
    if (it == m->named.end()) return RGBD_EINVAL;
    const Act& a = it->second;
    shape_out[0] = a.n;
    shape_out[1] = a.c;
    shape_out[2] = a.h;
    shape_out[3] = a.w;
    if (!data) return RGBD_OK;
    const int64_t need = (int64_t)a.n * a.c * a.h * a.w;
    if (cap_floats < need) return RGBD_ENOSPC;
    float* tmp = nullptr;
    HIP_TRY(hipMalloc((void**)&tmp, (size_t)need * sizeof(float)));
    // (x_hat tensors come out of the image-producing layers in channel order; everything else is stored permuted)
    const int pm = (m->perm() && a.c > 4) ? 1 : 0;
    int r = launch_nhwc_to_nchw_clamp(a.p, a.n, a.c, a.h, a.w, a.cs, tmp, 0, m->s, pm);
    if (!r && hipStreamSynchronize(m->s) != hipSuccess) r = RGBD_EHIP;  // (the stream may be non-blocking: hipMemcpy would not wait for it)
    if (!r && hipMemcpy(data, tmp, (size_t)need * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) r = RGBD_EHIP;
    (void)hipFree(tmp);
    return r;
}

int rgbd_elic_set_debug_floats(rgbd_elic* m, int32_t on)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);
    if (!m) return RGBD_EINVAL;
    if (m->debug_floats != (on != 0)) m->graphs_invalidate();  // the workspace layout changes
    m->debug_floats = on != 0;
    return RGBD_OK;
}

int rgbd_elic_set_forced_symbols(rgbd_elic* m, int32_t modality, const int32_t* y_sym, int64_t n_y, const int32_t* z_sym, int64_t n_z)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);
    if (!m || modality < 0 || modality > 1 || n_y < 0 || n_z < 0 || (n_y && !y_sym) || (n_z && !z_sym)) return RGBD_EINVAL;
    if (m->single() && (m->variant != 5 || modality != 0)) return RGBD_EINVAL;  // (the two-modality codecs, and modality 0 of the checkerboard Cheng2020 model)
    m->graphs_invalidate();  // the workspace layout and the launch list change
    m->force_y[modality].assign(y_sym, y_sym + n_y);
    m->force_z[modality].assign(z_sym, z_sym + n_z);
    return RGBD_OK;
}

int rgbd_elic_debug_floats(rgbd_elic* m, int32_t modality, float* x, float* scale, int64_t cap, int64_t* n)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!m || !n || modality < 0 || modality > 1 || !m->dbg_x || !m->dbg_s) return RGBD_EINVAL;
    if (m->single() && modality != 0) return RGBD_EINVAL;  // the single-modal models keep one modality's floats
    *n = m->dbg_per_mod;
    if (!x || !scale) return RGBD_OK;
    if (cap < m->dbg_per_mod) return RGBD_ENOSPC;
    HIP_TRY(hipStreamSynchronize(m->s));
    const size_t bytes = sizeof(float) * (size_t)m->dbg_per_mod;
    HIP_TRY(hipMemcpy(x, m->dbg_x + (size_t)modality * m->dbg_per_mod, bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(scale, m->dbg_s + (size_t)modality * m->dbg_per_mod, bytes, hipMemcpyDeviceToHost));
    return RGBD_OK;
}

int rgbd_elic_debug_symbols(rgbd_elic* m, int32_t modality, int32_t* symbols, int32_t* indexes, int64_t cap, int64_t* n)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!m || !n || modality < 0 || modality > 1 || !m->dbg_sym) return RGBD_EINVAL;
    *n = m->dbg_per_mod;
    if (!symbols || !indexes) return RGBD_OK;
    if (cap < m->dbg_per_mod) return RGBD_ENOSPC;
    HIP_TRY(hipStreamSynchronize(m->s));
    HIP_TRY(hipMemcpy(symbols, m->dbg_sym + (size_t)modality * m->dbg_per_mod, sizeof(int32_t) * (size_t)m->dbg_per_mod,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(indexes, m->dbg_idx + (size_t)modality * m->dbg_per_mod, sizeof(int32_t) * (size_t)m->dbg_per_mod,
                      hipMemcpyDeviceToHost));
    return RGBD_OK;
}

}  // extern "C"
