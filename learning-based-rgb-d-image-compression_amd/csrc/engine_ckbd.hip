// Host runtime of the gfx950 codec engine: the layer graph of the checkerboard Cheng2020 family (declared in engine.h) -- GDN
// and pixel shuffle, its residual blocks, the four transforms, and the two-pass checkerboard entropy model (two_pass_ckbd).
#include "engine.h"

Act rgbd_elic::gdn(const std::string& name, const Act& x, bool inverse, const Act* res)
{
    Act y = alloc(x.n, x.h, x.w, x.c);
    if (dry() || rc) return y;
    float* beta = dense_of(name + ".beta");
    float* gamma = dense_of(name + ".gamma");
    if (!beta || !gamma) return y;
    GdnArgs a{};
    a.x = x.p;
    a.xcs = x.cs;
    a.y = y.p;
    a.ycs = y.cs;
    a.res = res ? res->p : nullptr;
    a.rcs = res ? res->cs : 0;
    a.npix = (long)x.n * x.h * x.w;
    a.cs = round_up(x.c, 16);
    a.beta = beta;
    a.gamma = gamma;
    a.inverse = inverse ? 1 : 0;
    hipEvent_t e1 = nullptr;
    if (profile && !prof_begin(&e1)) return y;
    const int r = launch_gdn(a, s);
    if (profile) prof_end(e1, name, 2.0 * (double)a.npix * x.c * x.c, 2.0 * (double)a.npix * x.c * x.c);
    if (r) fail(r);
    return y;
}

Act rgbd_elic::pixel_shuffle(const Act& t)
{
    Act u = alloc(t.n, 2 * t.h, 2 * t.w, t.c / 4);
    if (!dry() && !rc) {
        const int q = launch_pixel_shuffle2(t.p, t.n, t.h, t.w, t.c / 4, t.cs, u.p, u.cs, s);
        if (q) fail(q);
    }
    return u;
}

Act rgbd_elic::ck_res_block(const std::string& p, const Act& x)
{
    Epi e1, e2;
    e1.act = e2.act = ACT_LEAKY;
    e2.res2 = &x;
    return conv(p + ".conv2", conv(p + ".conv1", x, 1, 1, e1), 1, 1, e2);
}

Act rgbd_elic::ck_res_block_stride(const std::string& p, const Act& x)
{
    Epi leaky;
    leaky.act = ACT_LEAKY;
    const Act t = conv(p + ".conv2", conv(p + ".conv1", x, 2, 1, leaky), 1, 1);
    const Act id = conv(p + ".skip", x, 2, 0);
    return gdn(p + ".gdn", t, false, &id);
}

Act rgbd_elic::ck_res_block_up(const std::string& p, const Act& x)
{
    const std::string n[2] = {p + ".subpel_conv.0", p + ".upsample.0"};
    const Act xin[2] = {x, x};
    Epi ep[2];
    ep[0].act = ACT_LEAKY;
    Act t[2];
    conv2(2, n, xin, 1, 1, ep, nullptr, t);
    const Act u = conv(p + ".conv", pixel_shuffle(t[0]), 1, 1);
    const Act id = pixel_shuffle(t[1]);
    return gdn(p + ".igdn", u, true, &id);
}

Act rgbd_elic::ck_stage(const Act& x, const std::function<Act(const Act&)>& f, int oh, int ow, int oc)
{
    Act out = alloc(x.n, oh, ow, oc);
    const size_t mark = arena.top;
    copy_ch(f(x), out);
    arena.top = mark;
    return out;
}

Act rgbd_elic::g_a_ckbd(const Act& img)
{
    Act x = img;
    for (int i = 0; i < 3; ++i) {
        const std::string a = "g_a." + std::to_string(2 * i), b = "g_a." + std::to_string(2 * i + 1);
        x = ck_stage(x, [&](const Act& t) { return ck_res_block(b, ck_res_block_stride(a, t)); }, x.h / 2, x.w / 2, N);
    }
    return conv("g_a.6", x, 2, 1);
}

Act rgbd_elic::g_s_ckbd(const Act& yhat)
{
    Act x = yhat;
    for (int i = 0; i < 3; ++i) {
        const std::string a = "g_s." + std::to_string(2 * i), b = "g_s." + std::to_string(2 * i + 1);
        x = ck_stage(x, [&](const Act& t) { return ck_res_block_up(b, ck_res_block(a, t)); }, 2 * x.h, 2 * x.w, N);
    }
    return pixel_shuffle(conv("g_s.7.0", ck_res_block("g_s.6", x), 1, 1));
}

Act rgbd_elic::h_a_ckbd(const Act& y)
{
    static const int strides[5] = {1, 1, 2, 1, 2};
    Epi leaky;
    leaky.act = ACT_LEAKY;
    Act t = y;
    for (int k = 0; k < 5; ++k) t = conv("h_a." + std::to_string(2 * k), t, strides[k], 1, k < 4 ? leaky : Epi());
    return t;
}

void rgbd_elic::h_s_ckbd(const Act& zhat, const Act& dst)
{
    Epi leaky;
    leaky.act = ACT_LEAKY;
    const size_t mark = arena.top;
    Act t = conv("h_s.0", zhat, 1, 1, leaky);
    t = pixel_shuffle(conv("h_s.2.0", t, 1, 1, leaky));
    t = conv("h_s.4", t, 1, 1, leaky);
    t = pixel_shuffle(conv("h_s.6.0", t, 1, 1, leaky));
    conv("h_s.8", t, 1, 1, Epi(), &dst);
    arena.top = mark;
}

void rgbd_elic::ck_entropy_params(const Act& cat, int part, const Act& out)
{
    Epi leaky, lin;
    leaky.act = ACT_LEAKY;
    leaky.ckbd = lin.ckbd = g_ckbd_conv ? part : 0;
    const size_t mark = arena.top;
    Act t = part == 1 ? conv("entropy_parameters.0.hyper", view(cat, 2 * M, 2 * M), 1, 0, leaky)
                      : conv("entropy_parameters.0", cat, 1, 0, leaky);
    t = conv("entropy_parameters.2", t, 1, 0, leaky);
    conv("entropy_parameters.4", t, 1, 0, lin, &out);
    arena.top = mark;
}

void rgbd_elic::ck_context(const Act& yhat, const Act& dst)
{
    Epi e;
    e.ckbd = 2;
    ConvPlan cp = conv_plan("context_prediction", yhat, 1, 2, e, &dst);
    if (!dry() && cp.ok && cp.a.nphase == 1) {
        const int all = cp.a.taps.n[0], n = keep_taps(cp.a.taps, 1);
        cp.flops_exec = cp.flops * 0.5 * n / std::max(1, all);
    }
    conv_issue(cp);
}

void rgbd_elic::two_pass_ckbd(Coding& cd, const Act* y, const Act& cat, const Act& params, const Act& yhat)
{
    yhat_base[0] = yhat.p;
    const int64_t part_syms = (int64_t)M * cat.h * (cat.w / 2);
    const Act ys = y ? *y : Act();
    ck_entropy_params(cat, 1, params);
    code_part(cd, 0, 1, params, ys, yhat, 0);
    ck_context(yhat, view(cat, 0, 2 * M));
    ck_entropy_params(cat, 2, params);
    code_part(cd, 0, 0, params, ys, yhat, part_syms);
}
