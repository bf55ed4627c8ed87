// Host runtime of the gfx950 codec engine: the layer graphs of the ELIC families (declared in engine.h) -- the blocks of
// nm modalities (bottleneck, residual unit, attention, ESA, Bi-SPF), the stage walk of the analysis / synthesis transforms,
// the hyper transforms of ELIC_united, ELIC_united_R2D and single-modal ELIC, the entropy-parameter and channel-context
// nets, and the checkerboard slice loop (slice_loop_ckbd) with the coder's side of one part (code_part).
#include "engine.h"

void rgbd_elic::take_lead2(int nm, const std::string n[2], const Act x[2], Act t[2])
{
    int found = 0;
    for (int m = 0; m < nm; ++m) found += (int)pre_leads.count(n[m]);
    if (found == nm) {
        for (int m = 0; m < nm; ++m) {
            t[m] = pre_leads[n[m]];
            pre_leads.erase(n[m]);
        }
        return;
    }
    if (found) {  // (never planned that way; stay correct)
        for (int m = 0; m < nm; ++m) take_lead2(1, n + m, x + m, t + m);
        return;
    }
    Epi relu[2];
    relu[0].act = relu[1].act = ACT_RELU;
    conv2(nm, n, x, 1, 0, relu, nullptr, t);
}

void rgbd_elic::bottleneck2(int nm, const std::string p[2], const Act x[2], const Act* const dst[2], const std::string next_lead[2],
                            Act out[2])
{
    const PackedConv* last[2] = {};
    for (int m = 0; m < nm; ++m) last[m] = conv_of(p[m] + ".branch.4.weight");
    if (!last[0] || !last[nm - 1]) return;
    const int G = (g_pair && nm == 2) ? 2 : 1;
    std::string last_name[2], mid[2], lead0[2];
    bool fuse = true, lead = true;
    int skips = 0;
    for (int m = 0; m < nm; ++m) {
        out[m] = (dst && dst[m]) ? *dst[m] : alloc(x[m].n, x[m].h, x[m].w, last[m]->cout);
        last_name[m] = p[m] + ".branch.4";
        mid[m] = p[m] + ".branch.2";
        lead0[m] = p[m] + ".branch.0";
        skips += (int)convs.count(p[m] + ".skip.weight");
        // the pair is planned at 2N; should the two plans not share a launch after all (conv2 falls back to two launches
        // when pairable() fails), each of them is re-planned at N -- so fusing has to be possible at both sizes
        fuse = fuse && fusable(mid[m], last_name[m], x[m], G) && (nm == 1 || fusable(mid[m], last_name[m], x[m], 1));
    }
    for (int m = 0; m < nm; ++m) lead = lead && fuse && lead_fusable(last_name[m], next_lead[m], x[m]);
    Act lead_out[2];
    if (lead)
        for (int m = 0; m < nm; ++m)
            lead_out[m] = alloc(x[m].n, x[m].h, x[m].w, convs.find(next_lead[m] + ".weight")->second.cout);  // outlives this block
    const size_t mark = arena.top;
    Act t1[2], idn[2];
    take_lead2(nm, lead0, x, t1);
    for (int m = 0; m < nm; ++m) idn[m] = x[m];
    if (skips == nm) {
        // the skip path lands in the block's output buffer and the last layer adds to it in place (each element is read
        // and written by the one thread that owns it): no 2 x 252 MB identity tensor at the workspace's peak stage
        std::string sk[2];
        for (int m = 0; m < nm; ++m) sk[m] = p[m] + ".skip";
        const Epi none[2];
        const Act* sdst[2] = {&out[0], &out[1]};
        conv2(nm, sk, x, 1, 0, none, sdst, idn);
    } else if (skips) {
        fail(RGBD_EINVAL);  // (the two branches are built alike)
        return;
    }
    Epi e[2];
    for (int m = 0; m < nm; ++m) e[m].res1 = &idn[m];
    const Act* odst[2] = {&out[0], &out[1]};
    Act o[2];
    if (fuse) {
        const std::string* f1[2] = {&last_name[0], &last_name[1]};
        const std::string* l1[2] = {&next_lead[0], &next_lead[1]};
        const Act* ld[2] = {&lead_out[0], &lead_out[1]};
        conv2(nm, mid, t1, 1, 1, e, odst, o, f1, lead ? l1 : nullptr, lead ? ld : nullptr);
        if (lead)
            for (int m = 0; m < nm; ++m) pre_leads[next_lead[m]] = lead_out[m];
    } else {
        Epi relu[2];
        relu[0].act = relu[1].act = ACT_RELU;
        Act t2[2];
        conv2(nm, mid, t1, 1, 1, relu, nullptr, t2);
        conv2(nm, last_name, t2, 1, 0, e, odst, o);
    }
    arena.top = mark;
}

void rgbd_elic::res_unit2(int nm, const std::string p[2], const Act x[2], const std::string next_lead[2], Act out[2])
{
    const int G = (g_pair && nm == 2) ? 2 : 1;
    std::string last_name[2], mid[2], lead0[2];
    bool fuse = true, lead = true;
    for (int m = 0; m < nm; ++m) {
        out[m] = alloc(x[m].n, x[m].h, x[m].w, x[m].c);
        last_name[m] = p[m] + ".conv.4";
        mid[m] = p[m] + ".conv.2";
        lead0[m] = p[m] + ".conv.0";
        fuse = fuse && fusable(mid[m], last_name[m], x[m], G) && (nm == 1 || fusable(mid[m], last_name[m], x[m], 1));  // (see bottleneck2)
    }
    for (int m = 0; m < nm; ++m) lead = lead && fuse && lead_fusable(last_name[m], next_lead[m], x[m]);
    Act lead_out[2];
    if (lead)
        for (int m = 0; m < nm; ++m)
            lead_out[m] = alloc(x[m].n, x[m].h, x[m].w, convs.find(next_lead[m] + ".weight")->second.cout);
    const size_t mark = arena.top;
    Act t1[2];
    take_lead2(nm, lead0, x, t1);
    Epi e[2];
    for (int m = 0; m < nm; ++m) {
        e[m].act = ACT_RELU;
        e[m].res1 = &x[m];
    }
    const Act* odst[2] = {&out[0], &out[1]};
    Act o[2];
    if (fuse) {
        const std::string* f1[2] = {&last_name[0], &last_name[1]};
        const std::string* l1[2] = {&next_lead[0], &next_lead[1]};
        const Act* ld[2] = {&lead_out[0], &lead_out[1]};
        conv2(nm, mid, t1, 1, 1, e, odst, o, f1, lead ? l1 : nullptr, lead ? ld : nullptr);
        if (lead)
            for (int m = 0; m < nm; ++m) pre_leads[next_lead[m]] = lead_out[m];
    } else {
        Epi relu[2];
        relu[0].act = relu[1].act = ACT_RELU;
        Act t2[2];
        conv2(nm, mid, t1, 1, 1, relu, nullptr, t2);
        conv2(nm, last_name, t2, 1, 0, e, odst, o);
    }
    arena.top = mark;
}

void rgbd_elic::attention2(int nm, const std::string p[2], const Act x[2], const Act* const dst[2], Act out[2])
{
    for (int m = 0; m < nm; ++m) out[m] = (dst && dst[m]) ? *dst[m] : alloc(x[m].n, x[m].h, x[m].w, x[m].c);
    const size_t mark = arena.top;
    Act a[2], b[2];
    for (int m = 0; m < nm; ++m) a[m] = b[m] = x[m];
    for (int br = 0; br < 2; ++br) {
        const char* tag = br ? ".conv_b." : ".conv_a.";
        Act* cur = br ? b : a;
        for (int u = 0; u < 3; ++u) {
            std::string n[2], nl[2];
            for (int m = 0; m < nm; ++m) {
                n[m] = p[m] + tag + std::to_string(u);
                nl[m] = u < 2 ? p[m] + tag + std::to_string(u + 1) + ".conv.0" : std::string();
            }
            Act o[2];
            res_unit2(nm, n, cur, nl, o);
            cur[0] = o[0];
            cur[1] = o[1];
        }
    }
    Epi e[2];
    std::string n[2];
    for (int m = 0; m < nm; ++m) {
        e[m].act = ACT_SIGMOID;
        e[m].mul = &a[m];
        e[m].res2 = &x[m];
        n[m] = p[m] + ".conv_b.3";
    }
    const Act* odst[2] = {&out[0], &out[1]};
    Act o[2];
    conv2(nm, n, b, 1, 0, e, odst, o);
    arena.top = mark;
}

void rgbd_elic::esa2(int nm, const std::string p[2], const Act x[2], const Act dst[2], const Act* const add[2])
{
    const size_t mark = arena.top;
    const Epi none[2];
    Epi relu[2];
    relu[0].act = relu[1].act = ACT_RELU;
    auto names = [&](const char* suf, std::string n[2]) {
        for (int m = 0; m < nm; ++m) n[m] = p[m] + suf;
    };
    std::string n[2];
    Act c1_[2], c1[2];
    names(".conv1", n);
    conv2(nm, n, x, 1, 0, none, nullptr, c1_);
    names(".conv2", n);
    conv2(nm, n, c1_, 2, 0, none, nullptr, c1);
    if (c1[0].h < 7 || c1[0].w < 7) {
        fail(RGBD_EINVAL);
        return;
    }
    const int ph = (c1[0].h - 7) / 3 + 1, pw = (c1[0].w - 7) / 3 + 1;
    Act v[2];
    for (int m = 0; m < nm; ++m) v[m] = alloc(x[m].n, ph, pw, c1[m].c);
    const bool same = nm == 2 && g_pair && c1[0].n == c1[1].n && c1[0].h == c1[1].h && c1[0].w == c1[1].w &&
                      c1[0].cs == c1[1].cs;
    if (!dry() && !rc) {  // both modalities' pooled branches in one launch when they have the same shape (they do)
        int r = launch_maxpool7s3(c1[0].p, c1[0].n, c1[0].h, c1[0].w, c1[0].cs, v[0].p, ph, pw, s, same ? c1[1].p : nullptr,
                                  same ? v[1].p : nullptr);
        if (!r && nm == 2 && !same) r = launch_maxpool7s3(c1[1].p, c1[1].n, c1[1].h, c1[1].w, c1[1].cs, v[1].p, ph, pw, s);
        if (r) fail(r);
    }
    Act vr[2], c3[2], c3b[2], up[2], sum[2], o[2];
    names(".conv_max", n);
    conv2(nm, n, v, 1, 1, relu, nullptr, vr);
    names(".conv3", n);
    conv2(nm, n, vr, 1, 1, relu, nullptr, c3);
    names(".conv3_", n);
    conv2(nm, n, c3, 1, 1, none, nullptr, c3b);
    for (int m = 0; m < nm; ++m) up[m] = alloc(x[m].n, x[m].h, x[m].w, c3b[m].c);
    if (!dry() && !rc) {
        const bool same2 = same && x[0].h == x[1].h && x[0].w == x[1].w && c3b[0].cs == c3b[1].cs && up[0].cs == up[1].cs;
        const int rc0 = refnum ? c3b[0].c : 0, rc1 = refnum ? c3b[1].c : 0;
        int r = launch_bilinear(c3b[0].p, c3b[0].n, c3b[0].h, c3b[0].w, c3b[0].cs, up[0].p, x[0].h, x[0].w, s,
                                same2 ? c3b[1].p : nullptr, same2 ? up[1].p : nullptr, rc0);
        if (!r && nm == 2 && !same2)
            r = launch_bilinear(c3b[1].p, c3b[1].n, c3b[1].h, c3b[1].w, c3b[1].cs, up[1].p, x[1].h, x[1].w, s, nullptr, nullptr, rc1);
        if (r) fail(r);
    }
    Epi addup[2], gate[2];
    for (int m = 0; m < nm; ++m) {
        addup[m].res1 = &up[m];
        gate[m].act = ACT_SIGMOID;
        gate[m].mul = &x[m];
        gate[m].res2 = add ? add[m] : nullptr;
    }
    names(".conv_f", n);
    conv2(nm, n, c1_, 1, 0, addup, nullptr, sum);
    const Act* odst[2] = {&dst[0], &dst[1]};
    names(".conv4", n);
    conv2(nm, n, sum, 1, 0, gate, odst, o);
    arena.top = mark;
}

void rgbd_elic::bi_spf(const std::string& p, const Act& rgb, const Act& depth, const Act& r_dst, const Act& d_dst,
                       bool residual)
{
    const size_t mark = arena.top;
    const int half = rgb.c / 2;
    Act rd = alloc(rgb.n, rgb.h, rgb.w, rgb.c);  // cat(rf, df)
    Act dr = alloc(rgb.n, rgb.h, rgb.w, rgb.c);  // cat(df, rf)
    Epi relu;
    relu.act = ACT_RELU;
    Act rf = view(rd, 0, half), df = view(rd, half, half);
    // each extractor writes its features into both concat buffers (cat(rf, df) and cat(df, rf)) from its epilogue
    const Act rf2 = view(dr, half, half), df2 = view(dr, 0, half);
    Epi er = relu, ed = relu;
    er.dup = &rf2;
    ed.dup = &df2;
    {
        const std::string n[2] = {p + ".r_ext", p + ".d_ext"};
        const Act x[2] = {rgb, depth};
        const Epi ep[2] = {er, ed};
        const Act* dst[2] = {&rf, &df};
        Act o[2];
        conv2(2, n, x, 1, 1, ep, dst, o);
    }
    {
        const std::string n[2] = {p + ".r_esa", p + ".d_esa"};
        const Act x[2] = {rd, dr};
        const Act dst[2] = {r_dst, d_dst};
        const Act* add[2] = {residual ? &rgb : nullptr, residual ? &depth : nullptr};
        esa2(2, n, x, dst, add);
    }
    arena.top = mark;
}

void rgbd_elic::stages(const Stages& sd, const Act in[2], Act out[2])
{
    const int nm = sd.nm;
    Act x[2];
    for (int m = 0; m < nm; ++m) x[m] = in[m];
    Ends ends;
    if (sd.ends) ends = ends_begin();
    for (int i = 0; i < sd.n; ++i) {
        const std::string k = sd.kinds[i], si = std::to_string(i);
        const bool next_spf = (i + 1 < sd.n) && std::string(sd.kinds[i + 1]) == "spf";
        if (sd.ends) ends_stage(ends, k != "spf");
        if (k == "spf") {  // the widened branches are 2N-channel concat buffers whose first half is filled
            if (sd.fusion == kBiSpf)
                bi_spf(sd.prefix[0] + si, view(x[0], 0, N), view(x[1], 0, N), view(x[0], N, N), view(x[1], N, N));
            else
                bi_spf_single(sd.prefix[0] + si, x[0], view(x[1], 0, N), view(x[1], N, N));
            continue;
        }
        // the stage feeding a fusion writes into the first half of the concat buffer of every branch the fusion widens
        Act cat[2], half[2];
        const Act* dsts[2] = {nullptr, nullptr};
        if (next_spf)
            for (int m = sd.fusion == kBiSpfDepth ? 1 : 0; m < nm; ++m) {
                const int oh = (k == "deconv") ? x[m].h * 2 : (k == "conv" ? x[m].h / 2 : x[m].h);
                const int ow = (k == "deconv") ? x[m].w * 2 : (k == "conv" ? x[m].w / 2 : x[m].w);
                cat[m] = alloc(x[m].n, oh, ow, 2 * N);
                half[m] = view(cat[m], 0, N);
                dsts[m] = &half[m];
            }
        const bool next_rb = sd.leads && (i + 1 < sd.n) && std::string(sd.kinds[i + 1]) == "rb";
        std::string names[2], nl[2];
        for (int m = 0; m < nm; ++m) {
            names[m] = sd.prefix[m] + si;
            if (next_rb) nl[m] = sd.prefix[m] + std::to_string(i + 1) + ".branch.0";
        }
        const Epi none[2];
        Act o[2];
        const int g = sd.grouped ? nm : 1;  // branches per launch
        for (int m = 0; m < nm; m += g) {
            if (k == "conv" || k == "deconv") conv2(g, names + m, x + m, 2, 2, none, dsts + m, o + m);
            else if (k == "rb") bottleneck2(g, names + m, x + m, dsts + m, nl + m, o + m);
            else attention2(g, names + m, x + m, dsts + m, o + m);
        }
        for (int m = 0; m < nm; ++m) x[m] = dsts[m] ? cat[m] : o[m];
        if (sd.mids && (i == 1 || i == 5 || i == 10)) copy_ch(x[0], sd.mids[i == 1 ? 0 : (i == 5 ? 1 : 2)]);
        if (sd.guides && (i == 1 || i == 5 || i == 10)) {  // in front of the bottlenecks of 2, 7, 11 and the attention of 6
            const int k = i == 1 ? 0 : (i == 5 ? 1 : 2);
            x[0] = spatial_aligner(std::string(sd.sp_prefix) + "sp" + std::to_string(k + 1), x[0], sd.guides[k]);
        }
    }
    if (sd.ends) ends_finish(ends);
    for (int m = 0; m < nm; ++m) out[m] = x[m];
}

void rgbd_elic::g_a(const Act x[2], Act y[2])
{
    const Stages sd = {kAna18, 18, 2, {"g_a.rgb_analysis_transform.", "g_a.depth_analysis_transform."},
                       kBiSpf, true, true, true};
    stages(sd, x, y);
}

void rgbd_elic::g_s(const Act yhat[2], Act xhat[2])
{
    const Stages sd = {kSyn18, 18, 2, {"g_s.rgb_synthesis_transform.", "g_s.depth_synthesis_transform."},
                       kBiSpf, true, true, true};
    stages(sd, yhat, xhat);
}

void rgbd_elic::h_a(const Act& yr, const Act& yd, Act* zr, Act* zd)
{
    Epi relu;
    relu.act = ACT_RELU;
    const char* mods[2] = {"rgb", "depth"};
    const Act* in[2] = {&yr, &yd};
    Act* out[2] = {zr, zd};
    const std::string p[2] = {std::string("h_a.") + mods[0] + "_reduction.", std::string("h_a.") + mods[1] + "_reduction."};
    const Epi relu2[2] = {relu, relu}, none[2];
    const Act x0[2] = {*in[0], *in[1]};
    Act t0[2], t1[2], t2[2];
    const std::string n0[2] = {p[0] + "0", p[1] + "0"}, n2[2] = {p[0] + "2", p[1] + "2"}, n4[2] = {p[0] + "4", p[1] + "4"};
    conv2(2, n0, x0, 1, 1, relu2, nullptr, t0);
    conv2(2, n2, t0, 2, 2, relu2, nullptr, t1);
    conv2(2, n4, t1, 2, 2, none, nullptr, t2);
    *out[0] = t2[0];
    *out[1] = t2[1];
}

void rgbd_elic::hs_block2(int nm, const std::string p[2], const Act own[2], const Act other[2], bool last, Act out[2])
{
    Act f[2];
    std::string n[2];
    for (int m = 0; m < nm; ++m) {
        f[m] = alloc(own[m].n, own[m].h, own[m].w, own[m].c + other[m].c);
        se_cat_to(p[m] + ".se", own[m], other[m], f[m]);
        if (rc) return;
        n[m] = p[m] + ".deconv";
    }
    Epi e[2];
    e[0].act = e[1].act = last ? ACT_NONE : ACT_LEAKY;
    // a stride-2 layer with a measured recipe runs deconv_s2_ref per modality: the pair refuses to go without it, the
    // single branch's conv() takes that route itself and falls back to the sub-pixel kernel
    const PackedConv* pc0 = conv_of(n[0] + ".weight");
    if (nm == 2 && !last && refnum && pc0 && ref_blocks(3, pc0->cin, pc0->cout, f[0].h, f[0].w)) {
        bool ok = true;
        for (int m = 0; m < 2; ++m) ok = deconv_s2_ref(n[m], f[m], ACT_LEAKY, &out[m]) && ok;
        if (!ok) fail(RGBD_ESTATE);
        return;
    }
    conv2(nm, n, f, last ? 1 : 2, last ? 1 : 2, e, nullptr, out);
}

void rgbd_elic::h_s(const Act& zr, const Act& zd, Act* hr, Act* hd)
{
    Act cur[2] = {zr, zd};
    for (int st = 1; st <= 3; ++st) {
        const std::string p[2] = {"h_s.r_h_s" + std::to_string(st), "h_s.d_h_s" + std::to_string(st)};
        const Act other[2] = {cur[1], cur[0]};
        Act o[2];
        hs_block2(2, p, cur, other, st == 3, o);
        cur[0] = o[0];
        cur[1] = o[1];
    }
    *hr = cur[0];
    *hd = cur[1];
}

Act rgbd_elic::entropy_params(const SliceLoop& d, const std::string& p, const Act& ctx, int part, const Act* dst,
                              const float* means, int mstride)
{
    const PackedConv* last = conv_of(p + ".fusion.4.weight");
    if (!last) return Act();
    Act out = dst ? *dst : alloc(ctx.n, ctx.h, ctx.w, last->cout);
    const size_t mark = arena.top;
    Act t = ctx;
    if (d.se) {
        t = alloc(ctx.n, ctx.h, ctx.w, ctx.c);
        se_scale_to(p + ".se", ctx, 1, t, means, mstride);
    }
    for (int l = 0; l < 3; ++l) {
        const std::string n = p + ".fusion." + std::to_string(2 * l);
        const PackedConv* pc = conv_of(n + ".weight");
        Epi e;
        if (l < 2) e.act = ACT_RELU;
        if (g_ckbd_conv && (l == 2 || d.ckbd_all)) e.ckbd = part;
        t = conv(n, t, 1, pc ? pc->k / 2 : 0, e, l == 2 ? &out : nullptr);
    }
    arena.top = mark;
    return out;
}

void rgbd_elic::channel_context2(int nm, const std::string p[2], const Act x[2], const Act dst[2])
{
    const size_t mark = arena.top;
    Epi relu[2];
    relu[0].act = relu[1].act = ACT_RELU;
    const Epi none[2];
    std::string n0[2], n2[2], n4[2];
    for (int m = 0; m < nm; ++m) {
        n0[m] = p[m] + ".fushion.0";
        n2[m] = p[m] + ".fushion.2";
        n4[m] = p[m] + ".fushion.4";
    }
    Act t0[2], t1[2], o[2];
    conv2(nm, n0, x, 1, 2, relu, nullptr, t0);
    conv2(nm, n2, t0, 1, 2, relu, nullptr, t1);
    const Act* odst[2] = {&dst[0], &dst[1]};
    conv2(nm, n4, t1, 1, 2, none, odst, o);
    arena.top = mark;
}

void rgbd_elic::code_part(Coding& cd, int mod, int anchor, const Act& params, const Act& y_slice, const Act& yhat_slice,
                          int64_t part_off)
{
    if (dry() || rc) return;
    PartGeom g;
    g.B = params.n;
    g.h = params.h;
    g.w = params.w;
    g.C = yhat_slice.c;
    g.anchor = anchor;
    g.per_image = cd.per_image;
    g.perm = perm();
    const int64_t mod_off = (int64_t)mod * g.B * cd.per_image_total;
    int32_t* sym = cd.sym + mod_off;
    int32_t* idx = cd.idx + mod_off;
    const int64_t* sb = cd.stream_base;  // relative to the modality's region
    int r;
    if (cd.estimate) {
        const Act lk = view(cd.lik[mod], (int)(yhat_slice.p - (mod ? yhat_base[1] : yhat_base[0])), g.C);
        r = launch_ckbd_estimate_part(y_slice.p, y_slice.cs, params.p, params.cs, yhat_slice.p, yhat_slice.cs, lk.p, lk.cs,
                                      g, s);
    } else if (cd.encode) {
        r = launch_ckbd_encode_part(y_slice.p, y_slice.cs, params.p, params.cs, yhat_slice.p, yhat_slice.cs,
                                    scale_table, g, sym, idx, sb, part_off, s, dbg_x ? dbg_x + mod_off : nullptr,
                                    dbg_s ? dbg_s + mod_off : nullptr);
        if (!r && coder_lanes && mod == 0) {  // the parts become the wide encoder's segments (the same for every modality)
            const int64_t count = (int64_t)g.C * g.h * (g.w / 2) * (cd.per_image ? 1 : g.B);
            const int64_t poff = cd.per_image ? part_off : part_off * g.B;
            if (poff != y_seg_next) r = RGBD_ESTATE;
            else if (y_segs.n >= WIDE_MAX_SEGS) r = RGBD_ENOSPC;
            else {
                y_segs.count[y_segs.n++] = count;
                y_seg_next += count;
            }
        }
        if (!r && cd.force)  // y_hat of this part again, from the forced symbols (symbol + mean, as the decoder forms it)
            r = launch_ckbd_decode_part(params.p, params.cs, yhat_slice.p, yhat_slice.cs, g, cd.force + mod_off, sb, part_off, s);
    } else {
        r = launch_ckbd_index_part(params.p, params.cs, scale_table, g, idx, sb, part_off, s);
        const int64_t count = (int64_t)g.C * g.h * (g.w / 2) * (cd.per_image ? 1 : g.B);
        const int64_t poff = cd.per_image ? part_off : part_off * g.B;
        if (!r && coder_lanes)
            r = launch_rans_wide_decode(cd.words, cd.stream_off + (size_t)mod * cd.nstreams,
                                        cd.stream_len + (size_t)mod * cd.nstreams, cd.nstreams, coder_lanes,
                                        cd.state + (size_t)mod * cd.nstreams * y_state_words(), cd.first[mod] ? 1 : 0, idx,
                                        sym, sb, poff, count, tables[mod].d, cd.err, s);
        else if (!r)
            r = launch_rans_decode(cd.words, cd.stream_off + (size_t)mod * cd.nstreams,
                                   cd.stream_len + (size_t)mod * cd.nstreams, cd.nstreams,
                                   cd.state + (size_t)mod * cd.nstreams * 2, cd.first[mod] ? 1 : 0, idx, sym, sb, poff,
                                   count, tables[mod].d, s);
        cd.first[mod] = false;
        if (!r) r = launch_ckbd_decode_part(params.p, params.cs, yhat_slice.p, yhat_slice.cs, g, sym, sb, part_off, s);
    }
    if (r) fail(r);
}

void rgbd_elic::slice_loop_ckbd(Coding& cd, const SliceLoop& d, int nm, const Act* y, const Act hyp[2], const Act yhat[2])
{
    for (int m = 0; m < nm; ++m) yhat_base[m] = yhat[m].p;
    int c0 = 0;
    int64_t part_off = 0;
    const int B = hyp[0].n, h = hyp[0].h, w = hyp[0].w, HC = hyp[0].c;  // HC = 2M
    // SE gates of the entropy-parameter nets (entropy.py:75) need the channel means of their whole input -- 1280 ... 2816
    // channels, of which 2 x 2M are the hyper parameters, the same tensor for all 20 nets of a call.  A mean is a function
    // of its own channel only (channel_mean_kernel: one fixed chain per channel), so the means are kept per segment of
    // the context buffer and only what changed is recomputed: the hyper parameters' once per call, the channel contexts'
    // once per slice, the local contexts' (2C channels) per part -- the same floats as a pass over the whole input, for
    // 1/10 of the traffic (round 4; 1.6 GB per c3 step).  hm: [B][nm HC] hyper means; sm[b]: [B][wide] in buffer b's layout.
    static const bool mean_cache_on = getenv("RGBD_NO_MEAN_CACHE") == nullptr;  // A/B switch (the workspace stays as it is)
    const bool mc = d.mean_cache && mean_cache_on;
    float* hm = d.mean_cache ? (float*)arena.take((size_t)B * nm * HC * sizeof(float)) : nullptr;
    auto means_of = [&](const Act& t, float* dstm, int stride) {
        if (dry() || rc || !mc) return;
        const int r = refnum ? launch_channel_mean_ref(t.p, t.n, t.h * t.w, t.cs, t.c, dstm, stride, s)
                             : launch_channel_mean_strided(t.p, t.n, t.h * t.w, t.cs, t.c, dstm, stride, s);
        if (r) fail(r);
    };
    auto copy_means = [&](const float* src, int sstride, float* dstm, int dstride, int n) {
        if (dry() || rc || !mc) return;
        const int r = launch_copy_channels(src, sstride, dstm, dstride, B, n, s);
        if (r) fail(r);
    };
    for (int m = 0; m < nm && d.mean_cache; ++m) means_of(hyp[m], hm + m * HC, nm * HC);
    for (size_t i = 0; i < slice_ch.size(); ++i) {
        const int C = slice_ch[i];
        const size_t mark = arena.top;
        const std::string si = std::to_string(i);
        const int width[3] = {2 * C, HC, i ? 2 * C : 0};  // of a local-context, a hyper, a channel-context segment
        Act buf[2];
        float* sm[2] = {nullptr, nullptr};
        int nbuf = 0, wide[2] = {0, 0}, off[2][6];
        for (; nbuf < 2 && d.layout[nbuf][0] != kSegEnd; ++nbuf) {
            for (int& o : off[nbuf]) o = -1;  // (segment not in this buffer)
            for (const Seg* sg = d.layout[nbuf]; *sg != kSegEnd; ++sg) {
                off[nbuf][*sg] = wide[nbuf];
                wide[nbuf] += width[*sg / 2];
            }
            buf[nbuf] = alloc(B, h, w, wide[nbuf]);
            if (d.mean_cache) sm[nbuf] = (float*)arena.take((size_t)B * wide[nbuf] * sizeof(float));
        }
        auto seg = [&](int b, int sg) { return view(buf[b], off[b][sg], width[sg / 2]); };
        for (int b = 0; b < nbuf; ++b) {
            for (int m = 0; m < nm; ++m)
                if (off[b][kHypR + m] >= 0) copy_ch(hyp[m], seg(b, kHypR + m));
            if (d.mean_cache) copy_means(hm, nm * HC, sm[b] + off[b][kHypR], wide[b], nm * HC);
        }
        if (i) {  // the channel contexts go into the last buffer; an earlier one that has the segment gets a copy
            const int home = nbuf - 1;
            std::string cn[2];
            Act cx[2], cdst[2];
            for (int m = 0; m < nm; ++m) {
                cn[m] = d.prefix[m] + ("channel_context." + si);
                cx[m] = view(yhat[m], 0, c0);
                cdst[m] = seg(home, kChR + m);
            }
            if (d.grouped_ch) channel_context2(nm, cn, cx, cdst);
            else
                for (int m = 0; m < nm; ++m) channel_context2(1, cn + m, cx + m, cdst + m);
            for (int b = 0; b < home; ++b)
                for (int m = 0; m < nm; ++m)
                    if (off[b][kChR + m] >= 0) copy_ch(cdst[m], seg(b, kChR + m));
            for (int b = 0; b < nbuf && d.mean_cache; ++b)  // all modalities' channel contexts: adjacent
                means_of(view(buf[b], off[b][kChR], nm * 2 * C), sm[b] + off[b][kChR], wide[b]);
        }
        Act ys[2], hs[2];
        for (int m = 0; m < nm; ++m) {
            ys[m] = y ? view(y[m], c0, C) : Act();
            hs[m] = view(yhat[m], c0, C);
        }
        const int64_t part_syms = (int64_t)C * h * (w / 2);
        for (int part = 0; part < 2; ++part)  // anchor, non-anchor
            for (int m = 0; m < nm; ++m) {
                const CtxNet& n = d.net[part][m];
                const std::string pn = d.prefix[m] + ((part ? "entropy_parameters_nonanchor." : "entropy_parameters_anchor.") + si);
                const int o = off[n.buf][n.first], wd = wide[n.buf] - o;
                const Act suffix = view(buf[n.buf], o, wd);
                Act prm;
                if (n.gathered) {
                    prm = alloc(B, h, w, 2 * C);
                    const size_t m2 = arena.top;
                    Act in = alloc(B, h, w, 2 * C + wd);
                    copy_ch(seg(0, kLocR), view(in, 0, 2 * C));
                    copy_ch(suffix, view(in, 2 * C, wd));
                    float* im = nullptr;  // the gathered input's means, gathered alike
                    if (d.mean_cache) {
                        im = (float*)arena.take((size_t)B * (2 * C + wd) * sizeof(float));
                        copy_means(sm[0] + off[0][kLocR], wide[0], im, 2 * C + wd, 2 * C);
                        copy_means(sm[n.buf] + o, wide[n.buf], im + 2 * C, 2 * C + wd, wd);
                    }
                    entropy_params(d, pn, in, part + 1, &prm, mc ? im : nullptr, 2 * C + wd);
                    arena.top = m2;
                } else {
                    prm = entropy_params(d, pn, suffix, part + 1, nullptr, mc ? sm[n.buf] + o : nullptr, wide[n.buf]);
                }
                code_part(cd, m, 1 - part, prm, ys[m], hs[m], part_off + part * part_syms);
                // the local context of what is decoded by now, for the nets that follow: the modality's own after its
                // anchor part (hs holds the anchor half only so far), RGB's again after its non-anchor part when a depth net
                // follows
                if (part && (m || nm == 1)) continue;
                const int lb = d.loc_buf[part ? 2 : m], ls = part ? kLocR : kLocR + m;
                const Act loc = seg(lb, ls);
                const std::string ln = d.prefix[m] + ((part ? "local_context_anchor_with_nonanchor." : "local_context.") + si);
                if (!part && d.anchor_taps) conv_anchor_in(ln, hs[m], 2, loc);
                else conv(ln, hs[m], 1, 2, Epi(), &loc);
                if (d.mean_cache) means_of(loc, sm[lb] + off[lb][ls], wide[lb]);
            }
        part_off += 2 * part_syms;
        c0 += C;
        arena.top = mark;
    }
}

void rgbd_elic::bi_spf_single(const std::string& p, const Act& rgb, const Act& depth, const Act& d_dst)
{
    const size_t mark = arena.top;
    const int half = rgb.c / 2;
    Act dr = alloc(rgb.n, rgb.h, rgb.w, rgb.c);  // cat(df, rf)
    Epi relu;
    relu.act = ACT_RELU;
    Act df = view(dr, 0, half), rf = view(dr, half, half);
    conv(p + ".d_ext", depth, 1, 1, relu, &df);
    conv(p + ".r_ext", rgb, 1, 1, relu, &rf);
    const std::string n = p + ".d_esa";
    esa2(1, &n, &dr, &d_dst, nullptr);
    arena.top = mark;
}

void rgbd_elic::g_a_r2d(const Act x[2], Act y[2])
{
    const Stages sd = {kAna18, 18, 2, {"g_a.rgb_analysis_transform.", "g_a.depth_analysis_transform."},
                       kBiSpfDepth, false, false, false};
    stages(sd, x, y);
}

void rgbd_elic::g_s_r2d(const Act yhat[2], Act xhat[2])
{
    const Stages sd = {kSyn18, 18, 2, {"g_s.rgb_synthesis_transform.", "g_s.depth_synthesis_transform."},
                       kBiSpfDepth, false, false, false};
    stages(sd, yhat, xhat);
}

Act rgbd_elic::hs_block_single(const std::string& p, const Act& x, bool last)
{
    Act f = alloc(x.n, x.h, x.w, x.c);
    se_scale_to(p + ".se", x, 0, f);
    Epi e;
    e.act = last ? ACT_NONE : ACT_LEAKY;
    Act o;
    if (!last && deconv_s2_ref(p + ".deconv", f, ACT_LEAKY, &o)) return o;
    return conv(p + ".deconv", f, last ? 1 : 2, last ? 1 : 2, e);
}

void rgbd_elic::h_s_r2d(const Act& zr, const Act& zd, Act* hr, Act* hd)
{
    Act r = zr, d = zd;
    for (int st = 1; st <= 3; ++st) {
        const std::string pd = "h_s.d_h_s" + std::to_string(st);
        const Act r_next = hs_block_single("h_s.r_h_s" + std::to_string(st), r, st == 3);
        Act d_next;
        hs_block2(1, &pd, &d, &r, st == 3, &d_next);
        r = r_next;
        d = d_next;
    }
    *hr = r;
    *hd = d;
}

Act rgbd_elic::g_a1(const Act& x)
{
    Act y[2];
    stages({kAna15, 15, 1, {"g_a.analysis_transform.", ""}, kNoFusion, false, false, false}, &x, y);
    return y[0];
}

Act rgbd_elic::g_s1(const Act& yhat)
{
    Act xhat[2];
    stages({kSyn15, 15, 1, {"g_s.synthesis_transform.", ""}, kNoFusion, false, false, false, mid_dst}, &yhat, xhat);
    return xhat[0];
}

Act rgbd_elic::g_s_master(const Act& yhat)
{
    if (!guide_src) {  // (the entry points refuse a call without guides before anything runs)
        fail(RGBD_ESTATE);
        return Act();
    }
    Act xhat[2];
    stages({kSyn15, 15, 1, {"g_s.synthesis_transform.", ""}, kNoFusion, false, false, false, nullptr, guide_src, "g_s."}, &yhat, xhat);
    return xhat[0];
}

Act rgbd_elic::h_a1(const Act& y)
{
    Epi relu;
    relu.act = ACT_RELU;
    Act t = conv("h_a.reduction.0", y, 1, 1, relu);
    t = conv("h_a.reduction.2", t, 2, 2, relu);
    return conv("h_a.reduction.4", t, 2, 2);
}

Act rgbd_elic::h_s1(const Act& zhat, const Act* dst)
{
    Epi relu;
    relu.act = ACT_RELU;
    Act t = conv("h_s.increase.0", zhat, 2, 2, relu);
    t = conv("h_s.increase.2", t, 2, 2, relu);
    return conv("h_s.increase.4", t, 1, 1, Epi(), dst);
}
