// Host runtime of the gfx950 codec engine: the layer graphs built from Swin blocks (declared in engine.h) -- LayerNorm and
// the Swin block for nm modalities, Spatial_aligner, the attention contexts of MLIC++, the transforms of STF_united and of
// the single-modal STF, and the latter's channel-slice entropy model (code_slice, slice_loop).
#include "engine.h"

Act rgbd_elic::layernorm(const std::string& p, const Act& x)
{
    Act y = alloc(x.n, x.h, x.w, x.c);
    float* w = dense_of(p + ".weight");
    float* b = dense_of(p + ".bias");
    if (dry() || rc || !w || !b) return y;
    const int r = launch_layernorm(x.p, (size_t)x.n * x.h * x.w, x.c, x.cs, w, b, y.p, y.cs, s);
    if (r) fail(r);
    return y;
}

void rgbd_elic::layernorm2(int nm, const std::string p[2], const Act x[2], Act y[2])
{
    float *w[2] = {}, *b[2] = {};
    for (int m = 0; m < nm; ++m) {
        y[m] = alloc(x[m].n, x[m].h, x[m].w, x[m].c);
        w[m] = dense_of(p[m] + ".weight");
        b[m] = dense_of(p[m] + ".bias");
    }
    if (dry() || rc || !w[0] || !b[0] || !w[nm - 1] || !b[nm - 1]) return;
    pair_or_each(nm, x, y, [&](int m, bool pair) {
        return launch_layernorm(x[m].p, (size_t)x[m].n * x[m].h * x[m].w, x[m].c, x[m].cs, w[m], b[m], y[m].p, y[m].cs, s,
                                pair ? x[1].p : nullptr, pair ? w[1] : nullptr, pair ? b[1] : nullptr, pair ? y[1].p : nullptr);
    });
}

void rgbd_elic::swin_block_tail2(int nm, const std::string p[2], const Act x[2], const Act a[2], const Act out[2])
{
    auto names = [&](const char* suf, std::string n[2]) {
        for (int m = 0; m < nm; ++m) n[m] = p[m] + suf;
    };
    std::string n[2];
    Act x1[2], t2[2], hdn[2], o[2];
    Epi e1[2];
    e1[0].res1 = &x[0];
    e1[1].res1 = &x[1];
    names(".attn.proj", n);
    conv2(nm, n, a, 1, 0, e1, nullptr, x1);
    names(".norm2", n);
    layernorm2(nm, n, x1, t2);
    Epi g[2];
    g[0].act = g[1].act = ACT_GELU;
    names(".mlp.fc1", n);
    conv2(nm, n, t2, 1, 0, g, nullptr, hdn);
    Epi e2[2];
    e2[0].res1 = &x1[0];
    e2[1].res1 = &x1[1];
    const Act* odst[2] = {&out[0], &out[1]};
    names(".mlp.fc2", n);
    conv2(nm, n, hdn, 1, 0, e2, odst, o);
}

void rgbd_elic::swin_block2(int nm, const std::string p[2], const Act x[2], int shift, int heads, Act out[2])
{
    for (int m = 0; m < nm; ++m) out[m] = alloc(x[m].n, x[m].h, x[m].w, x[m].c);
    const size_t mark = arena.top;
    const std::string n1[2] = {p[0] + ".norm1", p[nm - 1] + ".norm1"}, nq[2] = {p[0] + ".attn.qkv", p[nm - 1] + ".attn.qkv"};
    const Epi none[2];
    Act t[2], qkv[2], a[2];
    layernorm2(nm, n1, x, t);
    conv2(nm, nq, t, 1, 0, none, nullptr, qkv);
    float* rpb[2] = {};
    for (int m = 0; m < nm; ++m) {
        a[m] = alloc(x[m].n, x[m].h, x[m].w, x[m].c);
        rpb[m] = dense_of(p[m] + ".attn.relative_position_bias_table");
    }
    if (!dry() && !rc && rpb[0] && rpb[nm - 1])
        pair_or_each(nm, qkv, a, [&](int m, bool pair) {
            return launch_window_attention(qkv[m].p, x[m].n, x[m].h, x[m].w, x[m].c, qkv[m].cs, heads, shift, rpb[m], a[m].p,
                                           a[m].cs, s, pair ? qkv[1].p : nullptr, pair ? rpb[1] : nullptr,
                                           pair ? a[1].p : nullptr);
        });
    swin_block_tail2(nm, p, x, a, out);
    arena.top = mark;
}

Act rgbd_elic::spatial_aligner(const std::string& prefix, const Act& x, const Act& guided)
{
    const std::string p = prefix.empty() ? std::string() : prefix + ".";
    Act ex = conv(p + "patch_embeding1", x, 2, 0);
    const Act eg = conv(p + "patch_embeding2", guided, 2, 0);
    const int heads = 3;  // :346; embed_dim 96 = 3 * 32
    for (int k = 0; k < 2; ++k) {
        const std::string pb = p + "blocks." + std::to_string(k);
        const Act out = alloc(ex.n, ex.h, ex.w, ex.c);
        const size_t mark = arena.top;
        const Act t = layernorm(pb + ".norm1", ex);
        const Act tg = layernorm(pb + ".norm1", eg);
        const Act q = conv(pb + ".attn.qkv1", t, 1, 0);
        const Act kv = conv(pb + ".attn.qkv2", tg, 1, 0);
        const Act a = alloc(ex.n, ex.h, ex.w, ex.c);
        float* rpb = dense_of(pb + ".attn.relative_position_bias_table");
        if (!dry() && !rc && rpb) {
            const int r = launch_guided_window_attention(q.p, q.cs, kv.p, kv.cs, ex.n, ex.h, ex.w, ex.c, heads, k ? 2 : 0, rpb,
                                                         a.p, a.cs, s);
            if (r) fail(r);
        }
        swin_block_tail2(1, &pb, &ex, &a, &out);  // (nm == 1: arrays of one)
        arena.top = mark;
        ex = out;
    }
    return pixel_shuffle(conv(p + "recovery", ex, 1, 0));
}

Act rgbd_elic::dwconv(const std::string& name, const Act& x, bool gelu)
{
    const Act y = alloc(x.n, x.h, x.w, x.c);
    float* w = dense_of(name + ".weight");
    float* b = dense_of(name + ".bias");
    if (dry() || rc || !w || !b) return y;
    const int r = launch_dwconv3x3(x.p, x.n, x.h, x.w, x.c, x.cs, w, b, gelu ? 1 : 0, y.p, y.cs, s);
    if (r) fail(r);
    return y;
}

Act rgbd_elic::local_context(const Act& x, const std::string& p, int heads)
{
    if (heads < 0) heads = ctx_heads;
    const Act t = layernorm(p + "norm1", x);
    const Act qkv = conv(p + "qkv_proj", t, 1, 0);
    const Act a = alloc(x.n, x.h, x.w, 2 * x.c);
    float* tab = dense_of(p + "relative_position_table");
    float* fw = dense_of(p + "fusion.weight");
    float* fb = dense_of(p + "fusion.bias");
    if (!dry() && !rc && tab && fw && fb) {
        const int r = launch_local_ckbd_attention(qkv.p, qkv.cs, x.n, x.h, x.w, x.c, heads, tab, fw, fb, a.p, a.cs, s);
        if (r) fail(r);
    }
    const Act x1 = conv(p + "proj", a, 1, 0);
    const Act t2 = layernorm(p + "norm2", x1);
    Epi g;
    g.act = ACT_GELU;
    const Act hdn = conv(p + "mlp.fc1", t2, 1, 0, g);
    Epi e;
    e.res1 = &x1;
    return conv(p + "mlp.fc2", hdn, 1, 0, e);
}

Act rgbd_elic::linear_context(const Act& xk, const Act& xq, const Act& xv, int mode, bool skip, const std::string& p, int heads)
{
    if (heads < 0) heads = ctx_heads;
    const Act k = dwconv(p + "keys.1", conv(p + "keys.0", xk, 1, 0), false);
    const Act q = dwconv(p + "queries.1", conv(p + "queries.0", xq, 1, 0), false);
    const Act v = dwconv(p + "values.1", conv(p + "values.0", xv, 1, 0), false);
    const Act a = alloc(k.n, k.h, k.w, k.c);
    const int hd = k.c / heads;
    const int64_t wsf = linear_attention_ws_floats(k.n, k.h, k.w, heads, hd, mode);
    if (wsf <= 0) {
        fail(RGBD_EINVAL);
        return a;
    }
    float* ws = (float*)arena.take((size_t)wsf * sizeof(float));
    if (!dry() && !rc) {
        const int r = launch_linear_attention(k.p, k.cs, q.p, q.cs, v.p, v.cs, k.n, k.h, k.w, heads, hd, mode, a.p, a.cs, ws,
                                              wsf, s);
        if (r) fail(r);
    }
    const Act att = conv(p + "reprojection", a, 1, 2);
    Epi g;
    g.act = ACT_GELU;
    const Act h1 = conv(p + "mlp.0", att, 1, 0, g);
    const Act h2 = dwconv(p + "mlp.2", h1, true);
    const Act sk = skip ? conv(p + "skip", att, 1, 0) : att;
    Epi e;
    e.res1 = &sk;
    return conv(p + "mlp.4", h2, 1, 0, e);
}

Act rgbd_elic::entropy_params_mlic(const Act* seg, int nseg, int part, const Act* dst, const std::string& p, int out_dim)
{
    if (out_dim < 0) out_dim = out_ch;
    const Act& x0 = seg[0];
    const Act out = dst ? *dst : alloc(x0.n, x0.h, x0.w, out_dim);
    const size_t mark = arena.top;
    if (mlp_fused) {
        PixelMlp4 d{};
        for (int i = 0; i < nseg; ++i) {
            d.seg[i] = seg[i].p;
            d.seg_c[i] = seg[i].c;
            d.seg_cs[i] = seg[i].cs;
        }
        d.nseg = nseg;
        bool have = true;
        for (int l = 0; l < 4; ++l) {
            const std::string n = p + "fusion." + std::to_string(2 * l);
            const PackedConv* pc = conv_of(n + ".weight");  // (its bias: plain channel order, cout a multiple of 16)
            d.w[l] = dense_of(n + ".fragments");
            d.bias[l] = pc ? pc->bias : nullptr;
            have = have && pc && d.w[l];
        }
        d.out_dim = out_dim;
        d.B = x0.n;
        d.H = x0.h;
        d.W = x0.w;
        d.parity = part - 1;
        d.y = out.p;
        d.ycs = out.cs;
        if (!dry() && !rc && have) {
            const int r = launch_pixel_mlp4(d, s);
            if (r) fail(r);
        }
        return out;
    }
    Act t = x0;
    if (nseg > 1) {  // torch.cat([...], dim=1), written out
        int in_dim = 0;
        for (int i = 0; i < nseg; ++i) in_dim += seg[i].c;
        t = alloc(x0.n, x0.h, x0.w, in_dim);
        for (int i = 0, c0 = 0; i < nseg; c0 += seg[i].c, ++i) copy_ch(seg[i], view(t, c0, seg[i].c));
    }
    Epi gelu;
    gelu.act = ACT_GELU;
    for (int l = 0; l < 3; ++l) t = conv(p + "fusion." + std::to_string(2 * l), t, 1, 0, gelu);
    Epi last;
    last.ckbd = part;
    conv(p + "fusion.6", t, 1, 0, last, &out);
    arena.top = mark;
    return out;
}

Act rgbd_elic::channel_context_mlic(const Act& x, const std::string& p)
{
    Epi gelu;
    gelu.act = ACT_GELU;
    return conv(p + "fushion.4", conv(p + "fushion.2", conv(p + "fushion.0", x, 1, 1, gelu), 1, 1, gelu), 1, 1);
}

Act rgbd_elic::lrp_mlic(const Act& x, const std::string& p, bool tanh)
{
    Epi gelu;
    gelu.act = ACT_GELU;
    Act t = x;
    for (int l = 0; l < 3; ++l) t = conv(p + "lrp_transform." + std::to_string(2 * l), t, 1, 1, gelu);
    const Act out = conv(p + "lrp_transform.6", t, 1, 1);
    if (tanh && !dry() && !rc) {
        const int r = launch_half_tanh(out.p, out.cs, out.p, out.cs, (size_t)out.n * out.h * out.w, out.cs, s);
        if (r) fail(r);
    }
    return out;
}

void rgbd_elic::basic_layer2(int nm, const std::string p[2], const Act x_in[2], int depth, int heads, int down, Act out[2])
{
    Act x[2] = {x_in[0], x_in[nm - 1]};
    for (int k = 0; k < depth; ++k) {
        const std::string pb[2] = {p[0] + ".blocks." + std::to_string(k), p[nm - 1] + ".blocks." + std::to_string(k)};
        Act o[2];
        swin_block2(nm, pb, x, (k & 1) ? 2 : 0, heads, o);
        x[0] = o[0];
        x[1] = o[1];
    }
    const std::string pn[2] = {p[0] + ".downsample.norm", p[nm - 1] + ".downsample.norm"};
    const std::string prd[2] = {p[0] + ".downsample.reduction", p[nm - 1] + ".downsample.reduction"};
    const Epi none[2];
    if (down == 1) {
        Act g4[2], t[2];
        for (int m = 0; m < nm; ++m) {
            g4[m] = alloc(x[m].n, x[m].h / 2, x[m].w / 2, 4 * x[m].c);
            if (!dry() && !rc) {
                const int r = launch_patch_merge_gather(x[m].p, x[m].n, x[m].h, x[m].w, x[m].c, x[m].cs, g4[m].p, g4[m].cs, s);
                if (r) fail(r);
            }
        }
        layernorm2(nm, pn, g4, t);
        conv2(nm, prd, t, 1, 0, none, nullptr, out);
        return;
    }
    if (down == 2) {
        Act t[2], r2[2];
        layernorm2(nm, pn, x, t);
        conv2(nm, prd, t, 1, 0, none, nullptr, r2);
        for (int m = 0; m < nm; ++m) {
            out[m] = alloc(x[m].n, 2 * x[m].h, 2 * x[m].w, x[m].c / 2);
            if (!dry() && !rc) {
                const int r = launch_pixel_shuffle2(r2[m].p, x[m].n, x[m].h, x[m].w, x[m].c / 2, r2[m].cs, out[m].p, out[m].cs, s);
                if (r) fail(r);
            }
        }
        return;
    }
    out[0] = x[0];
    out[1] = x[1];
}

void rgbd_elic::stf_stack(const std::string& root, const char* kind, const Act& r_in, const Act& d_in, const int* depths,
                          const int* heads, int down, Act* r_out, Act* d_out)
{
    Act r = r_in, d = d_in;
    int li = 0;
    for (int i = 0; i < 4; ++i) {
        const int dn = i < 3 ? down : 0;
        const std::string pl[2] = {root + ".rgb_" + kind + "_layers." + std::to_string(li),
                                   root + ".depth_" + kind + "_layers." + std::to_string(li)};
        const Act xin[2] = {r, d};
        Act o[2];
        basic_layer2(2, pl, xin, depths[i], heads[i], dn, o);
        r = o[0];
        d = o[1];
        ++li;
        if (i < 3) {  // Bi-CPT fusion added to the streams (stf_united.py:481-489 / 581-589)
            Act r2 = alloc(r.n, r.h, r.w, r.c), d2 = alloc(d.n, d.h, d.w, d.c);
            bi_spf(root + ".rgb_" + kind + "_layers." + std::to_string(li), r, d, r2, d2, true);
            r = r2;
            d = d2;
            ++li;
        }
    }
    *r_out = r;
    *d_out = d;
}

void rgbd_elic::g_a_stf(const Act& rgb, const Act& depth, Act* y_r, Act* y_d)
{
    static const int depths[4] = {2, 2, 6, 2}, heads[4] = {3, 6, 12, 24};
    Act r = layernorm("g_a.rgb_patch_embed.norm", conv("g_a.rgb_patch_embed.proj", rgb, 2, 0));
    Act d = layernorm("g_a.depth_patch_embed.norm", conv("g_a.depth_patch_embed.proj", depth, 2, 0));
    stf_stack("g_a", "ana", r, d, depths, heads, 1, y_r, y_d);
}

void rgbd_elic::g_s_stf(const Act& yr, const Act& yd, Act* xr, Act* xd)
{
    static const int depths[4] = {2, 6, 2, 2}, heads[4] = {24, 12, 6, 3};
    Act r, d;
    stf_stack("g_s", "syn", yr, yd, depths, heads, 2, &r, &d);
    // stf_united.py:550-559; the first end conv has the same shape in both modalities (one grouped launch), the last differs
    const std::string n0[2] = {"g_s.rgb_end_conv.0", "g_s.depth_end_conv.0"};
    const Act in[2] = {r, d};
    const Epi none[2];
    Act t[2];
    conv2(2, n0, in, 1, 2, none, nullptr, t);
    const char* mods[2] = {"rgb", "depth"};
    Act* out[2] = {xr, xd};
    for (int m = 0; m < 2; ++m) {
        Act u = alloc(t[m].n, 2 * t[m].h, 2 * t[m].w, t[m].c / 4);
        if (!dry() && !rc) {
            const int q = launch_pixel_shuffle2(t[m].p, t[m].n, t[m].h, t[m].w, t[m].c / 4, t[m].cs, u.p, u.cs, s);
            if (q) fail(q);
        }
        *out[m] = conv(std::string("g_s.") + mods[m] + "_end_conv.2", u, 1, 1);
    }
}

Act rgbd_elic::swin_stack1(const std::string& root, const Act& x_in, const int* depths, const int* heads, int down)
{
    Act x[2] = {x_in, Act()};
    for (int i = 0; i < 4; ++i) {
        const std::string pl[2] = {root + "." + std::to_string(i), std::string()};
        Act o[2];
        basic_layer2(1, pl, x, depths[i], heads[i], i < 3 ? down : 0, o);
        x[0] = o[0];
    }
    return x[0];
}

Act rgbd_elic::g_a_stf1(const Act& img)
{
    static const int depths[4] = {2, 2, 6, 2}, heads[4] = {3, 6, 12, 24};
    return swin_stack1("layers", layernorm("patch_embed.norm", conv("patch_embed.proj", img, 2, 0)), depths, heads, 1);
}

Act rgbd_elic::g_s_stf1(const Act& yhat)
{
    static const int depths[4] = {2, 6, 2, 2}, heads[4] = {24, 12, 6, 3};
    const Act r = swin_stack1("syn_layers", yhat, depths, heads, 2);
    const Act t = conv("end_conv.0", r, 1, 2);
    Act u = alloc(t.n, 2 * t.h, 2 * t.w, t.c / 4);
    if (!dry() && !rc) {
        const int q = launch_pixel_shuffle2(t.p, t.n, t.h, t.w, t.c / 4, t.cs, u.p, u.cs, s);
        if (q) fail(q);
    }
    return conv("end_conv.2", u, 1, 1);
}

Act rgbd_elic::h_a_stf1(const Act& y)
{
    static const int strides[5] = {1, 1, 2, 1, 2};
    Epi gelu;
    gelu.act = ACT_GELU;
    Act t = y;
    for (int k = 0; k < 5; ++k) t = conv("h_a." + std::to_string(2 * k), t, strides[k], 1, k < 4 ? gelu : Epi());
    return t;
}

void rgbd_elic::h_s_stf1(const Act& zhat, const Act& means_dst, const Act& scales_dst)
{
    Epi gelu[2];
    gelu[0].act = gelu[1].act = ACT_GELU;
    const Epi none[2];
    auto names = [](const char* suf, std::string n[2]) {
        n[0] = std::string("h_mean_s.") + suf;
        n[1] = std::string("h_scale_s.") + suf;
    };
    std::string n[2];
    Act x[2] = {zhat, zhat}, t[2];
    static const char* const layer[4] = {"0", "2.0", "4", "6.0"};
    for (int k = 0; k < 4; ++k) {
        names(layer[k], n);
        conv2(2, n, x, 1, 1, gelu, nullptr, t);
        if (k & 1) {
            for (int m = 0; m < 2; ++m) {
                x[m] = alloc(t[m].n, 2 * t[m].h, 2 * t[m].w, t[m].c / 4);
                if (!dry() && !rc) {
                    const int q = launch_pixel_shuffle2(t[m].p, t[m].n, t[m].h, t[m].w, t[m].c / 4, t[m].cs, x[m].p, x[m].cs, s);
                    if (q) fail(q);
                }
            }
        } else {
            x[0] = t[0];
            x[1] = t[1];
        }
    }
    names("8", n);
    const Act* dst[2] = {&means_dst, &scales_dst};
    conv2(2, n, x, 1, 1, none, dst, t);
}

void rgbd_elic::code_slice(Coding& cd, int i, const Act& mu, const Act& sg, const Act& y_slice, const Act& slot)
{
    if (dry() || rc) return;
    SliceGeom g{};
    g.B = mu.n;
    g.h = mu.h;
    g.w = mu.w;
    g.C = kStfSliceCh;
    g.per_image = cd.per_image;
    const int64_t slice_off = (int64_t)i * g.C * g.h * g.w;
    int r;
    if (cd.estimate) {
        const Act lk = view(cd.lik[0], i * g.C, g.C);
        r = launch_slice_estimate(y_slice.p, y_slice.cs, mu.p, mu.cs, sg.p, sg.cs, g, lk.p, lk.cs, slot.p, slot.cs, nullptr, 0, s);
    } else if (cd.encode) {
        r = launch_slice_encode(y_slice.p, y_slice.cs, mu.p, mu.cs, sg.p, sg.cs, scale_tab, g, cd.sym, cd.idx, cd.stream_base,
                                slice_off, slot.p, slot.cs, nullptr, 0, s, dbg_x, dbg_s);
    } else {
        r = launch_slice_index(sg.p, sg.cs, scale_tab, g, cd.idx, cd.stream_base, slice_off, s);
        const int64_t count = (int64_t)g.C * g.h * g.w * (cd.per_image ? 1 : g.B);
        if (!r)
            r = launch_rans_decode(cd.words, cd.stream_off, cd.stream_len, cd.nstreams, cd.state, cd.first[0] ? 1 : 0, cd.idx,
                                   cd.sym, cd.stream_base, cd.per_image ? slice_off : slice_off * g.B, count, tables[0].d, s);
        cd.first[0] = false;
        if (!r) r = launch_slice_decode(mu.p, mu.cs, g, cd.sym, cd.stream_base, slice_off, slot.p, slot.cs, nullptr, 0, s);
    }
    if (r) fail(r);
}

void rgbd_elic::slice_loop(Coding& cd, const Act* y, const Act& ctxm, const Act& ctxs, const Act& yhat)
{
    const int C = kStfSliceCh, M0 = M;
    Epi gelu[2];
    gelu[0].act = gelu[1].act = ACT_GELU;
    const Epi none[2];
    for (int i = 0; i < kStfSlices; ++i) {
        const size_t mark = arena.top;
        const int k = std::min(i, kStfSupport), sup = M0 + C * k;
        const std::string si = std::to_string(i);
        Act x[2] = {view(ctxm, 0, sup), view(ctxs, 0, sup)}, t[2];
        for (int l = 0; l < 5; ++l) {  // cc_mean_transforms[i] and cc_scale_transforms[i]: one grouped launch per layer
            const std::string n[2] = {"cc_mean_transforms." + si + "." + std::to_string(2 * l),
                                      "cc_scale_transforms." + si + "." + std::to_string(2 * l)};
            conv2(2, n, x, 1, 1, l < 4 ? gelu : none, nullptr, t);
            x[0] = t[0];
            x[1] = t[1];
        }
        const Act slot = view(ctxm, sup, C);
        code_slice(cd, i, x[0], x[1], y ? view(*y, i * C, C) : Act(), slot);
        Act l1 = view(ctxm, 0, sup + C);
        for (int l = 0; l < 5; ++l) l1 = conv("lrp_transforms." + si + "." + std::to_string(2 * l), l1, 1, 1, l < 4 ? gelu[0] : Epi());
        if (!dry() && !rc) {
            const Act out = view(yhat, i * C, C), sslot = view(ctxs, sup, C);
            const bool ctx = i < kStfSupport;  // later slices are nobody's context
            const int r = launch_lrp_update(l1.p, l1.cs, slot.p, slot.cs, (size_t)slot.n * slot.h * slot.w, C, out.p, out.cs,
                                            ctx ? slot.p : nullptr, slot.cs, ctx ? sslot.p : nullptr, sslot.cs, s);
            if (r) fail(r);
        }
        arena.top = mark;
    }
}
