// Host runtime of the gfx950 codec engine: the C ABI of include/rgbd_amd.h outside the engine's life cycle --
// the operator-level entry points (conv2d, pointwise ops), the test hooks that put one launcher behind an operator boundary,
// the process-wide debug switches and the conv benchmark.  None of this is on the codec path.
#include "engine.h"

namespace {
// weight (+ bias) of one conv layer as the state dict holds them, in the form the packers take
struct HostConv {
    HostTensor w, b;
    const HostTensor* bias() const { return b.v.empty() ? nullptr : &b; }
};
HostConv host_conv(const float* weight, const float* bias, int cin, int cout, int k, bool transposed)
{
    HostConv c;
    c.w.shape = transposed ? std::vector<int64_t>{cin, cout, k, k} : std::vector<int64_t>{cout, cin, k, k};
    c.w.v.assign(weight, weight + (size_t)cin * cout * k * k);
    if (bias) c.b.shape = {cout}, c.b.v.assign(bias, bias + cout);
    return c;
}

// The device side of one hook call on NCHW tensors: the staged copies in the engine's layout (NHWC, channels permuted when
// `perm`), the packed weights, and the way in and out.  A hook takes every buffer first (RGBD_ENOMEM comes before the first
// kernel), converts its operands in, launches through step(), names its results and ends with finish().  The first error
// stops every later launch; buffers and weights are released on every way out.
struct Stage {
    hipStream_t s;
    int perm;
    DevBufs b;
    DevGen gen;  // (owns the packed weights)
    int rc = RGBD_OK;
    struct Result { const float* staged; int n, c, h, w, cs; float* dst; };
    std::vector<Result> results;

    Stage(void* stream, int perm_) : s((hipStream_t)stream), perm(perm_) {}
    float* get(size_t floats) { return b.get(floats); }
    float* get_if(const void* wanted, size_t floats) { return wanted ? b.get(floats) : nullptr; }
    template <class F>
    void step(F&& launch) { if (!rc) rc = launch(); }  // launch() -> RGBD_* code; skipped after an error
    // a caller's NCHW operand into its staged buffer (a null operand is none)
    void in(const float* src, int n, int c, int h, int w, float* staged, int cs)
    {
        if (src) step([&]() { return launch_nchw_to_nhwc16(src, n, c, h, w, staged, cs, s, perm); });
    }
    // a staged result that finish() converts back into the caller's NCHW tensor (a null destination is none)
    void out(const float* staged, int n, int c, int h, int w, int cs, float* dst) { if (dst) results.push_back({staged, n, c, h, w, cs, dst}); }
    // results back, the stream drained, a HIP error folded into the code
    int finish()
    {
        for (const Result& r : results) step([&]() { return launch_nhwc_to_nchw_clamp(r.staged, r.n, r.c, r.h, r.w, r.cs, r.dst, 0, s, perm); });
        const hipError_t e = hipStreamSynchronize(s);
        if (!rc && e != hipSuccess) rc = RGBD_EHIP;
        return rc;
    }
};

int conv2d_nchw_impl(const float* x_dev, int32_t n, int32_t cin, int32_t h, int32_t w, const float* weight, const float* bias,
                     int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t transposed, int32_t act,
                     const float* residual_dev, float* y_dev, void* stream, int refmode, const int32_t* blocks, int32_t nblocks,
                     int32_t bias_mode, int32_t flags)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!x_dev || !weight || !y_dev || n <= 0 || cin <= 0 || cout <= 0 || k <= 0 || k > 5 || stride < 1 || stride > 2)
        return RGBD_EINVAL;
    const HostConv hc = host_conv(weight, bias, cin, cout, k, transposed != 0);
    const bool subpix = !refmode && transposed && g_subpix == 2 && cout <= 4 && k == 5 && stride == 2 && pad == 2 && !residual_dev;
    Stage st(stream, refmode ? 1 : 0);
    PackedConv pc;
    int rc = subpix ? pack_subpix(hc.w, hc.bias(), &pc, &st.gen) : pack_conv(hc.w, hc.bias(), transposed != 0, &pc, &st.gen, st.perm, st.perm);
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
    float *xin = st.get(xf), *yout = st.get(yf), *res = st.get_if(residual_dev, yf);
    float* part = a.splitk > 1 ? st.get((size_t)a.splitk * yf) : nullptr;  // (read by the reducer: released after the stream has drained)
    if (!xin || !yout || (residual_dev && !res) || (a.splitk > 1 && !part)) return RGBD_ENOMEM;
    conv_args_geometry(&a, pc, xin, n, h, w, pc.cin_pad, yout, pc.cout_pad, OH, OW, stride, pad);
    conv_args_epilogue(&a, act, g_force_ckbd, res, pc.cout_pad, nullptr, 0, nullptr, 0, nullptr, 0);
    a.partial = part;
    st.in(x_dev, n, cin, h, w, xin, pc.cin_pad);
    st.in(residual_dev, n, cout, OH, OW, res, pc.cout_pad);
    // (the sub-pixel form does not write channels 4..15; the half a checkerboard launch does not compute reads as zero)
    if (!st.rc && (subpix || a.ckbd)) HIP_TRY(hipMemsetAsync(yout, 0, yf * sizeof(float), st.s));
    st.step([&]() { return launch_conv(a, st.s); });
    st.out(yout, n, cout, OH, OW, pc.cout_pad, y_dev);
    return st.finish();
}
}  // namespace

extern "C" {

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
    // (the operators as the codec runs them: channels stored permuted, the reference's CPU arithmetic -- DESIGN.md 4a)
    Stage st(stream, 1);
    float *xin = st.get((size_t)n * h * w * cs), *yout = st.get((size_t)n * oh * ow * cs);
    if (!xin || !yout) return RGBD_ENOMEM;
    st.in(x_dev, n, c, h, w, xin, cs);
    if (op == 0) st.step([&]() { return launch_maxpool7s3(xin, n, h, w, cs, yout, oh, ow, st.s); });
    if (op == 1) st.step([&]() { return launch_bilinear(xin, n, h, w, cs, yout, oh, ow, st.s, nullptr, nullptr, c); });
    if (!st.rc && op >= 2) {
        const int hid = c / 16;
        float *aux = st.get((size_t)n * (2 * c + hid + 1)), *dw0 = st.get((size_t)c * hid), *dw1 = st.get((size_t)c * hid);
        if (!aux || !dw0 || !dw1) return RGBD_ENOMEM;
        HIP_TRY(hipMemcpy(dw0, w0, (size_t)c * hid * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dw1, w1, (size_t)c * hid * sizeof(float), hipMemcpyHostToDevice));
        float *mean = aux, *sc = aux + (size_t)n * c, *hd = aux + (size_t)2 * n * c;
        st.step([&]() { return launch_channel_mean_ref(xin, n, h * w, cs, c, mean, c, st.s); });
        st.step([&]() { return launch_se_fc_ref(mean, n, c, hid, dw0, dw1, nullptr, nullptr, hd, sc, st.s); });  // (every row in the main order)
        st.step([&]() { return launch_channel_scale_to(xin, n, h * w, cs, c, sc, op == 3 ? 1 : 0, yout, cs, st.s); });
    }
    st.out(yout, n, c, oh, ow, cs, y_dev);
    return st.finish();
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
    Stage st(stream, 1);
    const size_t mfloats = (size_t)(n - 1) * mstride + c;
    float* xin = st.get((size_t)n * h * w * c);
    float* mean = st.get(mfloats);
    if (!xin || !mean) return RGBD_ENOMEM;
    st.in(x_dev, n, c, h, w, xin, c);
    st.step([&]() { return launch_channel_mean_ref(xin, n, h * w, c, c, mean, mstride, st.s); });  // (mean[image * mstride + channel POSITION])
    std::vector<float> hm(mfloats), row(c);
    if (!st.rc) HIP_TRY(hipMemcpyAsync(hm.data(), mean, mfloats * sizeof(float), hipMemcpyDeviceToHost, st.s));
    const int rc = st.finish();
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
    Stage st(stream, 1);
    float* dw = st.get((size_t)J * K);
    float* xp = st.get((size_t)n * K);
    float* yp = st.get((size_t)n * J);
    int* cls = (int*)st.get_if(row_class, J);
    if (!dw || !xp || !yp || (row_class && !cls)) return RGBD_ENOMEM;
    HIP_TRY(hipMemcpy(dw, weight, (size_t)J * K * sizeof(float), hipMemcpyHostToDevice));
    if (cls) HIP_TRY(hipMemcpy(cls, row_class, (size_t)J * sizeof(int), hipMemcpyHostToDevice));
    if (stage == 0) {  // fc.0: the input is the mean vector (by position), the output the hidden vector (plain)
        st.in(x_dev, n, K, 1, 1, xp, K);
        st.step([&]() { return launch_se_linear_ref(dw, xp, n, K, J, K, 1, cls, act, y_dev, J, 0, form, st.s); });
    } else {           // fc.2: the input is the hidden vector (plain), the output the gate vector (by position)
        st.step([&]() { return launch_se_linear_ref(dw, x_dev, n, K, J, K, 0, cls, act, yp, J, 1, form, st.s); });
        st.out(yp, n, J, 1, 1, J, y_dev);
    }
    return st.finish();
}

int rgbd_ref_sigmoid_gate(const float* t_dev, const float* mul_dev, const float* res_dev, int32_t n, int32_t c, int32_t h, int32_t w,
                          int32_t per_image, int32_t threads, float* y_dev, void* stream)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);
    if (!t_dev || !y_dev || !tensor_ok(n, c, h, w) || threads < 1 || threads > 1024 || per_image < 0 || per_image > 1) return RGBD_EINVAL;
    Stage st(stream, 1);
    const int cs = round_up(c, 16);
    const size_t fl = (size_t)n * h * w * cs;
    float *t = st.get(fl), *y = st.get(fl), *m = st.get_if(mul_dev, fl), *r = st.get_if(res_dev, fl);
    if (!t || !y || (mul_dev && !m) || (res_dev && !r)) return RGBD_ENOMEM;
    st.in(t_dev, n, c, h, w, t, cs);
    st.in(mul_dev, n, c, h, w, m, cs);
    st.in(res_dev, n, c, h, w, r, cs);
    st.step([&]() { return launch_sigmoid_gate_ref(t, cs, m, m ? cs : 0, r, r ? cs : 0, y, cs, n, h * w, c, per_image, threads, st.s); });
    st.out(y, n, c, h, w, cs, y_dev);
    return st.finish();
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
    const HostConv hc = host_conv(weight, bias, cin, cout, k, false);
    Stage st(stream, 1);
    PackedConv pc;
    if (const int rc = pack_conv(hc.w, hc.bias(), false, &pc, &st.gen, 1, 1)) return rc;
    const int xcs = pc.cin_pad, ycs = pc.cout_pad;
    const size_t xf = (size_t)n * h * w * xcs, yf = (size_t)n * OH * OW * ycs;
    float *xin = st.get(xf), *y = st.get(yf), *y2 = st.get_if(y2_dev, yf);
    float *r1 = st.get_if(res1_dev, yf), *m = st.get_if(mul_dev, yf), *r2 = st.get_if(res2_dev, yf);
    if (!xin || !y || (y2_dev && !y2) || (res1_dev && !r1) || (mul_dev && !m) || (res2_dev && !r2)) return RGBD_ENOMEM;
    st.in(x_dev, n, cin, h, w, xin, xcs);
    st.in(res1_dev, n, cout, OH, OW, r1, ycs);
    st.in(mul_dev, n, cout, OH, OW, m, ycs);
    st.in(res2_dev, n, cout, OH, OW, r2, ycs);
    // (the kernel writes the real channels of the computed positions only: pad channels and the other checkerboard half read 0)
    st.step([&]() { return launch_fill_zero(y, yf, st.s); });
    if (y2) st.step([&]() { return launch_fill_zero(y2, yf, st.s); });
    a.x = xin, a.N = n, a.H = h, a.W = w, a.xcs = xcs, a.C = cin, a.cin_pad = pc.cin_pad;
    a.w = pc.w, a.bias = pc.bias, a.K = k, a.stride = stride, a.pad = pad, a.act = act, a.ckbd = ckbd;
    a.y = y, a.O = cout, a.OH = OH, a.OW = OW, a.ycs = ycs;
    if (r1) a.res1 = r1, a.r1cs = ycs;
    if (m) a.mul = m, a.mcs = ycs;
    if (r2) a.res2 = r2, a.r2cs = ycs;
    if (y2) a.y2 = y2, a.y2cs = ycs;
    st.step([&]() { return launch_small_conv_ref(a, st.s); });
    st.out(y, n, cout, OH, OW, ycs, y_dev);
    st.out(y2, n, cout, OH, OW, ycs, y2_dev);
    return st.finish();
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
    if (const int rc = deconv_s2_ref_run(shape, recipe, (size_t)nrecipe, nullptr, n, h, w, act, nullptr, shape.cout_pad, 0, false, nullptr, none))
        return rc;
    const HostConv hc = host_conv(weight, bias, cin, cout, 5, true);
    Stage st(stream, 1);
    PackedConv pc;
    if (const int rc = pack_conv(hc.w, hc.bias(), true, &pc, &st.gen, 1, 1)) return rc;
    const size_t xf = (size_t)n * h * w * pc.cin_pad, yf = (size_t)n * 4 * h * w * pc.cout_pad;
    float *xin = st.get(xf), *y = st.get(yf);
    if (!xin || !y) return RGBD_ENOMEM;
    st.in(x_dev, n, cin, h, w, xin, pc.cin_pad);
    MallocScratch scratch{st.b};
    st.step([&]() { return deconv_s2_ref_run(pc, recipe, (size_t)nrecipe, xin, n, h, w, act, y, pc.cout_pad, 0, true, st.s, scratch); });
    st.out(y, n, cout, 2 * h, 2 * w, pc.cout_pad, y_dev);
    return st.finish();
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
    const int hidden = C / 16;
    const size_t wf = (size_t)C * hidden;
    std::vector<float> w1t(wf);
    se_pack_fc2(w1, (size_t)C, (size_t)hidden, w1t.data());
    Stage st(stream, perm);  // (nothing staged: the operands are in the engine's layout already)
    float *dw0 = st.get(wf), *dw1 = st.get(wf), *hid = st.get((size_t)N * hidden);
    if (!dw0 || !dw1 || !hid) return RGBD_ENOMEM;
    HIP_TRY(hipMemcpy(dw0, w0, wf * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dw1, w1t.data(), wf * sizeof(float), hipMemcpyHostToDevice));
    st.step([&]() { return launch_se_fc(mean_dev, N, C, hidden, dw0, dw1, hid, gate_dev, st.s, mstride, perm); });
    return st.finish();
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

int rgbd_pw_half_tanh(const float* x_dev, int32_t xcs, float* y_dev, int32_t ycs, int64_t npix, int32_t C, void* stream)
{
    if (!x_dev || !y_dev || !pw_tensor_ok(1, npix, C, xcs) || !pw_tensor_ok(1, npix, C, ycs) || C % 4 || !pw_al16(x_dev) || !pw_al16(y_dev))
        return RGBD_EINVAL;
    return launch_half_tanh(x_dev, xcs, y_dev, ycs, (size_t)npix, C, (hipStream_t)stream);
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
    Stage st(stream, perm);
    FormsSet fs[2];
    const size_t opx = (size_t)n * OH * OW;
    const int cyp = round_up(cy, 16);
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
    // the four guarded buffers of one operand set, armed before and checked after the launch
    auto guards = [&](const FormsSet& f, auto&& each) {
        st.step([&]() { return each(f.y, ycs, opx); });
        if (f.y2) st.step([&]() { return each(f.y2, y2cs, opx); });
        if (f.y3) st.step([&]() { return each(f.y3, y3cs, opx); });
        if (f.part) st.step([&]() { return each(f.part, cout_pad, (size_t)a.splitk * opx); });
    };
    for (int g = 0; g < G && !st.rc; ++g) {
        const rgbd_conv_forms_ops& o = d->set[g];
        FormsSet& f = fs[g];
        const HostConv hc = host_conv(o.weight, o.bias, cin, cout, k, tr);
        int rc = pack_conv(hc.w, hc.bias(), tr, &f.pc, &st.gen, perm, perm);
        if (!rc && fused) {
            const HostConv h2 = host_conv(o.w2, o.bias2, cout, d->cout2, 1, false);
            rc = pack_conv(h2.w, h2.bias(), false, &f.pc2, &st.gen, perm, perm);
        }
        if (!rc && lead) {
            const HostConv h3 = host_conv(o.w3, o.bias3, d->cout2, d->cout3, 1, false);
            rc = pack_conv(h3.w, h3.bias(), false, &f.pc3, &st.gen, perm, perm);
        }
        if (rc) return rc;
        f.x = st.get((size_t)n * h * w * xcs);
        f.y = st.get((opx + OW + 1) * ycs);
        f.y2 = st.get_if(o.y2_dev, (opx + OW + 1) * y2cs);
        if (lead) f.y3 = st.get((opx + OW + 1) * y3cs);
        f.r1 = st.get_if(o.res1_dev, (opx + OW + 1) * cyp);  // (the same slack as behind the destinations: what is read there is not used)
        f.m = st.get_if(o.mul_dev, (opx + OW + 1) * cyp);
        f.r2 = st.get_if(o.res2_dev, (opx + OW + 1) * cyp);
        const bool planes = a.splitk > 1 || gelu;  // (Engine::conv_plan's partial_bytes: a GELU layer books one plane)
        if (planes) f.part = st.get(((size_t)a.splitk * opx + OW + 1) * cout_pad);
        if (!f.x || !f.y || (o.y2_dev && !f.y2) || (lead && !f.y3) || (o.res1_dev && !f.r1) || (o.mul_dev && !f.m) || (o.res2_dev && !f.r2) ||
            (planes && !f.part))
            return RGBD_ENOMEM;
        guards(f, guard_arm);
        st.in(o.x_dev, n, d->x_total, h, w, f.x, xcs);
        st.in(o.y_dev, n, d->y_total, OH, OW, f.y, ycs);
        st.in(o.y2_dev, n, d->y2_total, OH, OW, f.y2, y2cs);
        st.in(o.y3_dev, n, d->y3_total, OH, OW, f.y3, y3cs);
        st.in(o.res1_dev, n, cy, OH, OW, f.r1, cyp);
        st.in(o.mul_dev, n, cy, OH, OW, f.m, cyp);
        st.in(o.res2_dev, n, cy, OH, OW, f.r2, cyp);
    }
    if (!st.rc) {
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
        st.step([&]() { return fused ? launch_conv_fused(a, st.s) : launch_conv(a, st.s); });
    }
    for (int g = 0; g < G; ++g) {
        const rgbd_conv_forms_ops& o = d->set[g];
        st.out(fs[g].y, n, d->y_total, OH, OW, ycs, o.y_dev);
        st.out(fs[g].y2, n, d->y2_total, OH, OW, y2cs, o.y2_dev);
        st.out(fs[g].y3, n, d->y3_total, OH, OW, y3cs, o.y3_dev);
    }
    st.finish();
    for (int g = 0; g < G; ++g) guards(fs[g], guard_intact);
    return st.rc;
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

}  // extern "C"
