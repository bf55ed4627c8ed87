// Host runtime of the gfx950 codec engine: the conv planner (declared in engine.h).  Layer lookup, the plan of one launch
// (tiles, split-K, the reference arithmetic's block structure), pairing two plans into one grouped launch, issue and
// profiling, the special routes (K-packed first layer, small-tensor route, sigmoid gate in its own pass, measured stride-2
// deconv recipes, anchor-input half taps), the fusion decisions of the block tails and the SE gates.
#include "engine.h"

const std::vector<int>* rgbd_elic::ref_blocks(int kind, int cin, int cout, int h, int w, int last) const
{
    auto it = ref_tab->blocks.find({kind, cin, cout, h, w, last < 0 ? ref_batch : last});
    if (it == ref_tab->blocks.end()) {
        ++ref_tab->misses;
        static const bool warn = getenv("RGBD_REFARITH_DEBUG") != nullptr;
        if (warn) fprintf(stderr, "[rgbd_amd] no reference block table for kind %d cin %d cout %d %dx%d batch %d\n", kind, cin, cout, h, w, ref_batch);
        return nullptr;
    }
    return &it->second;
}

const PackedConv* rgbd_elic::conv_of(const std::string& name)
{
    auto it = convs.find(name);
    if (it == convs.end()) {
        fprintf(stderr, "[rgbd_amd] missing layer %s\n", name.c_str());
        fail(RGBD_ESTATE);
        return nullptr;
    }
    return &it->second;
}

const int* rgbd_elic::cls_of(const std::string& wname)
{
    auto it = dense.find(wname + ".rowclass");
    return (it == dense.end() || ref_batch != 1) ? nullptr : reinterpret_cast<const int*>(it->second);
}

float* rgbd_elic::dense_of(const std::string& name)
{
    auto it = dense.find(name);
    if (it == dense.end()) {
        fprintf(stderr, "[rgbd_amd] missing tensor %s\n", name.c_str());
        fail(RGBD_ESTATE);
        return nullptr;
    }
    return it->second;
}

rgbd_elic::ConvPlan rgbd_elic::conv_plan(const std::string& name, const Act& x, int stride, int pad, Epi ep, const Act* dst,
                                         const std::string* fuse1x1, const std::string* lead1x1,
                                         const Act* lead_dst)
{
    ConvPlan cp;
    cp.name = name;
    const PackedConv* pc = conv_of(name + ".weight");
    if (!pc) return cp;
    const PackedConv* pc2 = fuse1x1 ? conv_of(*fuse1x1 + ".weight") : nullptr;
    if (fuse1x1 && !pc2) return cp;
    const PackedConv* pc3 = (pc2 && lead1x1 && lead_dst) ? conv_of(*lead1x1 + ".weight") : nullptr;
    if (lead1x1 && !pc3) {
        fail(RGBD_EINVAL);
        return cp;
    }
    const int k = pc->k;
    int OH, OW;
    conv_out_hw(x.h, x.w, k, stride, pad, pc->transposed, &OH, &OW);
    const PackedConv* pcy = pc2 ? pc2 : pc;  // the layer that produces y
    Act y = dst ? *dst : alloc(x.n, OH, OW, pcy->cout);
    cp.y = y;
    if (round_up(x.c, 16) != pc->cin_pad || y.h != OH || y.w != OW || y.n != x.n || y.c != pcy->cout ||
        (pc2 && (pc2->k != 1 || pc2->cin_pad != pc->cout_pad || pc2->transposed)) ||
        (pc3 && (pc3->k != 1 || pc3->cin_pad != pc2->cout_pad || pc3->transposed || lead_dst->c != pc3->cout ||
                 lead_dst->h != OH || lead_dst->w != OW || lead_dst->n != x.n))) {
        fprintf(stderr, "[rgbd_amd] shape mismatch at %s: x.c=%d cin=%d y=(%d,%d,%d) expect (%d,%d,%d)\n", name.c_str(),
                x.c, pc->cin, y.h, y.w, y.c, OH, OW, pc->cout);
        fail(RGBD_EINVAL);
        return cp;
    }
    if (rc) return cp;
    // (the sizing pass runs through the same planning -- pointers are placeholders there -- so that it books exactly the
    //  split-K planes the launch will use: a flat "8 planes per layer" used to be most of the workspace, 2 GB per big-map layer)
    ConvArgs& a = cp.a;
    // the last transposed conv (N -> 3 / 1): one 9-tap sub-pixel conv instead of four phases of padded couts
    const PackedConv* sp = nullptr;
    if (pc->transposed && g_subpix && !pc2 && stride == 2 && pad == 2 && k == 5 && !ep.res1 && !ep.mul && !ep.res2) {
        auto it = convs.find(name + ".subpix.weight");
        if (it != convs.end()) sp = &it->second;
    }
    conv_args_geometry(&a, sp ? *sp : *pc, x.p, x.n, x.h, x.w, x.cs, y.p, y.cs, OH, OW, stride, pad);
    a.cout_store = sp ? 16 : conv_cout_store(pcy->cout, y.cs);
    if (pc2) conv_args_tail(&a, *pc2, ACT_RELU, refnum);  // (reference arithmetic: one reduce block, fusable() has checked)
    if (pc3) conv_args_lead(&a, *pc3, lead_dst->p, lead_dst->cs);
    const auto ptr = [](const Act* t) { return t ? t->p : nullptr; };
    const auto cs = [](const Act* t) { return t ? t->cs : 0; };
    conv_args_epilogue(&a, ep.act, ep.ckbd, ptr(ep.res1), cs(ep.res1), ptr(ep.mul), cs(ep.mul), ptr(ep.res2), cs(ep.res2),
                       ptr(ep.dup), cs(ep.dup));
    a.loaded = tile_mode;
    // weight-heavy layers on the small latent grid (entropy model, hyper synthesis): split the reduction
    static const char* const kSplitPrefixes[] = {"rgb_entropy_parameters", "depth_entropy_parameters",
                                                 "rgb_channel_context", "depth_channel_context", "rgb_local_context",
                                                 "depth_local_context", "h_s."};
    a.splitk = 1;
    {
        const int mt = conv_max_taps(a);
        bool listed = false;
        for (const char* pre : kSplitPrefixes) listed = listed || name.rfind(pre, 0) == 0;
        // a measured entry (csrc/splitk_table.h) applies to any layer of that shape; the rule only to the listed families.
        // Fused tails, the packed image-facing layers and checkerboard-less sub-pixel forms run unsplit.
        const bool splittable = !pc2 && !sp;
        if (g_force_splitk > 0 && listed) a.splitk = g_force_splitk;
        else if (listed) a.splitk = conv_splitk_for(a.cin_pad, a.cout_pad, mt, (long)OH * OW, a.nphase);
        else if (splittable && g_force_splitk >= 0)
            if (const int t = conv_splitk_table(a.cin_pad, a.cout_pad, mt, (long)OH * OW, a.nphase)) a.splitk = t;
    }
    if (refnum) plan_refnum(cp, name, pc, pc2, sp != nullptr, x, stride, OH, OW);
    // split-K partial planes; a GELU layer (STF_united's MLP) also goes through the reducer, with a single plane
    cp.partial_bytes = (a.splitk > 1 || a.act == ACT_GELU) ? (size_t)a.splitk * x.n * OH * OW * pc->cout_pad * sizeof(float) : 0;
    cp.flops = 2.0 * (double)x.n * OH * OW * (double)pc->cout * pc->cin * k * k /
                   (pc->transposed ? (double)(stride * stride) : 1.0) +
               (pc2 ? 2.0 * (double)x.n * OH * OW * (double)pc2->cout * pc2->cin : 0.0) +
               (pc3 ? 2.0 * (double)x.n * OH * OW * (double)pc3->cout * pc3->cin : 0.0);
    cp.flops_exec = a.ckbd ? 0.5 * cp.flops : cp.flops;
    cp.fused = pc2 != nullptr;
    cp.ok = !dry();
    return cp;
}

void rgbd_elic::plan_refnum(ConvPlan& cp, const std::string& name, const PackedConv* pc, const PackedConv* pc2, bool subpix, const Act& x,
                            int stride, int OH, int OW)
{
    ConvArgs& a = cp.a;
    a.exact_math = 1;
    const bool kpacked = name.size() > 6 && name.compare(name.size() - 6, 6, ".kpack") == 0;
    if (subpix || kpacked || (pc->transposed && stride != 1)) return;  // (single chain, bias in the epilogue)
    if (pc->k == 1 && !pc->transposed) {
        a.bias_mode = 2;
        const std::vector<int>* bl = ref_blocks(0, pc->cin, pc->cout, x.h, x.w);
        if (!bl || bl->size() <= 1) {
            a.splitk = 1;  // one block: the single-chain kernel with the bias in front
            return;
        }
        const int nb = (int)bl->size();
        // small grids: the blocks as split-K ranges (the ordered reducer adds the block sums); large maps: in the kernel
        const bool split = (long)OH * OW <= 2048 && nb <= 16 && !pc2;
        if (split) {
            if (conv_set_split_ranges(&a, bl->data(), nb)) fail(RGBD_EINVAL);
        } else {
            a.splitk = 1;
            if (conv_set_blocks(&a, bl->data(), nb)) fail(RGBD_EINVAL);
        }
        return;
    }
    a.splitk = 1;
    a.bias_mode = pc->transposed ? 0 : 1;
    if (conv_set_blocks(&a, nullptr, 0)) fail(RGBD_EINVAL);
}

bool rgbd_elic::pairable(const ConvPlan& p, const ConvPlan& q)
{
    if (!p.ok || !q.ok || p.fused != q.fused) return false;
    const ConvArgs &a = p.a, &b = q.a;
    return a.N == b.N && a.H == b.H && a.W == b.W && a.xcs == b.xcs && a.cin_pad == b.cin_pad &&
           a.ntaps_total == b.ntaps_total && a.OH == b.OH && a.OW == b.OW && a.ycs == b.ycs && a.cout_pad == b.cout_pad &&
           a.cout_store == b.cout_store && a.GH == b.GH && a.GW == b.GW && a.IS == b.IS && a.OS == b.OS &&
           a.nphase == b.nphase && a.min_dy == b.min_dy && a.min_dx == b.min_dx && a.span_y == b.span_y &&
           a.span_x == b.span_x && a.act == b.act && !a.res1 == !b.res1 && a.r1cs == b.r1cs && !a.mul == !b.mul &&
           a.mcs == b.mcs && !a.res2 == !b.res2 && a.r2cs == b.r2cs && a.splitk == b.splitk && a.loaded == b.loaded &&
           a.ckbd == b.ckbd && !a.y2 == !b.y2 && a.y2cs == b.y2cs && a.subpix == b.subpix && !a.w2 == !b.w2 &&
           a.cout2_pad == b.cout2_pad && a.act_mid == b.act_mid && !a.w3 == !b.w3 && a.y3cs == b.y3cs &&
           a.cout3_pad == b.cout3_pad && memcmp(&a.taps, &b.taps, sizeof(TapTable)) == 0 && a.blocked == b.blocked &&
           a.bias_mode == b.bias_mode && a.tail_bias_init == b.tail_bias_init && a.exact_math == b.exact_math &&
           memcmp(a.blk_end, b.blk_end, sizeof(a.blk_end)) == 0 && memcmp(a.split_c16, b.split_c16, sizeof(a.split_c16)) == 0;
}

void rgbd_elic::conv_issue(ConvPlan& p, ConvPlan* q)
{
    if (dry()) {  // book the split-K scratch of this launch
        const size_t m0 = arena.top;
        (void)arena.take(p.partial_bytes + (q ? q->partial_bytes : 0));
        arena.top = m0;
        return;
    }
    if (rc || !p.ok || (q && !q->ok)) return;
    ConvArgs a = p.a;
    const size_t pmark = arena.top;
    if (p.partial_bytes) a.partial = (float*)arena.take(p.partial_bytes);
    if (q) {
        conv_args_group1(&a, q->a);
        if (q->partial_bytes) a.g1.partial = (float*)arena.take(q->partial_bytes);
    }
    hipEvent_t e1 = nullptr;
    if (profile && !prof_begin(&e1)) return;
    const int r = p.fused ? launch_conv_fused(a, s) : launch_conv(a, s);
    if (profile) {
        char key[200] = "";
        if (profile_keys)
            snprintf(key, sizeof(key), "|%d,%d,%d,%d,%d,%d,%d,%d,%d|%d", a.N * (a.groups == 2 ? 2 : 1), a.H, a.W, a.cin_pad, a.cout_pad,
                     a.ntaps_total, a.nphase > 1 ? a.OS : a.IS, a.nphase + 10 * a.ckbd + (a.blocked ? 100 : 0),
                     std::max(1, std::min(a.splitk, a.cin_pad / 16)), p.fused ? 1 : 0);
        prof_end(e1, p.name + key, p.flops + (q ? q->flops : 0.0), p.flops_exec + (q ? q->flops_exec : 0.0));
    }
    arena.top = pmark;  // stream order protects the scratch: later kernels of this stream run after the reducer
    if (r) {
        fprintf(stderr, "[rgbd_amd] conv launch failed at %s (%d)\n", p.name.c_str(), r);
        fail(r);
    }
}

bool rgbd_elic::conv_kpacked(const std::string& name, const Act& x, int stride, int pad, const Epi& ep, const Act* dst, Act* out)
{
    auto pcw = convs.find(name + ".weight");
    if (pcw == convs.end()) return false;
    const PackedConv* pc = &pcw->second;
    if (!(g_kpack && g_subpix && !pc->transposed && pc->k == 5 && stride == 2 && pad == 2 && x.c <= 3)) return false;
    auto kp = convs.find(name + ".kpack.weight");
    if (kp == convs.end()) return false;
    int OH, OW;
    conv_out_hw(x.h, x.w, 5, stride, pad, false, &OH, &OW);
    *out = dst ? *dst : alloc(x.n, OH, OW, pc->cout);
    const size_t mark = arena.top;
    Act xk = alloc(x.n, OH, OW, kp->second.cin_pad);
    if (!dry() && !rc) {
        const int r = launch_im2col5s2(x.p, x.n, x.h, x.w, x.cs, x.c, xk.p, OH, OW, xk.cs, s);
        if (r) fail(r);
    }
    conv(name + ".kpack", xk, 1, 0, ep, out);
    arena.top = mark;
    return true;
}

bool rgbd_elic::small_tensor_layer(const std::string& name, const Act& x) const
{
    if (!refnum || ref_batch != 1) return false;
    auto it = convs.find(name + ".weight");
    if (it == convs.end()) return false;
    const PackedConv& pc = it->second;
    return !pc.transposed && !pc.subpix && pc.k <= 3 && (long)pc.cin * x.h * x.w <= 20480;
}

Act rgbd_elic::conv_small(const std::string& name, const Act& x, int stride, int pad, const Epi& ep, const Act* dst)
{
    const PackedConv* pc = conv_of(name + ".weight");
    if (!pc) return Act();
    const int k = pc->k;
    int OH, OW;
    conv_out_hw(x.h, x.w, k, stride, pad, false, &OH, &OW);
    Act y = dst ? *dst : alloc(x.n, OH, OW, pc->cout);
    if (dry() || rc) return y;
    if (y.h != OH || y.w != OW || y.c != pc->cout || (ep.ckbd && stride != 1)) {
        fail(RGBD_EINVAL);
        return y;
    }
    SmallConvArgs a{};
    a.x = x.p;
    a.w = pc->w;
    a.bias = pc->bias;
    a.y = y.p;
    a.N = x.n;
    a.H = x.h;
    a.W = x.w;
    a.xcs = x.cs;
    a.C = pc->cin;
    a.cin_pad = pc->cin_pad;
    a.O = pc->cout;
    a.OH = OH;
    a.OW = OW;
    a.ycs = y.cs;
    a.K = k;
    a.stride = stride;
    a.pad = pad;
    a.act = ep.act;
    a.ckbd = ep.ckbd;
    if (ep.res1) a.res1 = ep.res1->p, a.r1cs = ep.res1->cs;
    if (ep.mul) a.mul = ep.mul->p, a.mcs = ep.mul->cs;
    if (ep.res2) a.res2 = ep.res2->p, a.r2cs = ep.res2->cs;
    if (ep.dup) a.y2 = ep.dup->p, a.y2cs = ep.dup->cs;
    const int Kt = pc->cin * k * k;
    const std::vector<int>* bl = ref_blocks(1, pc->cin, pc->cout, x.h, x.w, k * 100 + stride * 10 + pad);
    if (small_conv_set_kblocks(&a, bl && bl->size() <= 16 ? bl->data() : nullptr, bl ? (int)bl->size() : 0, Kt)) {
        fail(RGBD_EINVAL);
        return y;
    }
    const int r = launch_small_conv_ref(a, s);
    if (r) fail(r);
    return y;
}

bool rgbd_elic::sigmoid_scalar_tails(long numel) const
{
    long tasks = 1;
    if (numel >= 32768 && ref_threads > 1) tasks = std::min<long>(ref_threads, (numel + 32767) / 32768);
    const long chunk = (numel + tasks - 1) / tasks;
    return chunk % 32 != 0 || (numel - (tasks - 1) * chunk) % 32 != 0;
}

bool rgbd_elic::gate_needs_own_pass(const std::string& name, const Act& x, int stride, int pad, const Epi& ep)
{
    if (!refnum || ep.act != ACT_SIGMOID) return false;
    auto it = convs.find(name + ".weight");
    if (it == convs.end() || it->second.transposed) return false;
    const PackedConv& pc = it->second;
    int OH, OW;
    conv_out_hw(x.h, x.w, pc.k, stride, pad, false, &OH, &OW);
    return sigmoid_scalar_tails((long)(ref_batch == 1 ? 1 : x.n) * pc.cout * OH * OW);
}

Act rgbd_elic::conv_gated_ref(const std::string& name, const Act& x, int stride, int pad, const Epi& ep, const Act* dst)
{
    const PackedConv& pc = convs.find(name + ".weight")->second;
    int OH, OW;
    conv_out_hw(x.h, x.w, pc.k, stride, pad, false, &OH, &OW);
    Act out = dst ? *dst : alloc(x.n, OH, OW, pc.cout);
    const size_t mark = arena.top;
    Epi plain;
    plain.res1 = ep.res1;
    const Act t = conv(name, x, stride, pad, plain);
    if (!dry() && !rc) {
        const int r = launch_sigmoid_gate_ref(t.p, t.cs, ep.mul ? ep.mul->p : nullptr, ep.mul ? ep.mul->cs : 0,
                                              ep.res2 ? ep.res2->p : nullptr, ep.res2 ? ep.res2->cs : 0, out.p, out.cs, x.n,
                                              OH * OW, pc.cout, ref_batch == 1 ? 1 : 0, ref_threads, s);
        if (r) fail(r);
    }
    arena.top = mark;
    return out;
}

Act rgbd_elic::conv(const std::string& name, const Act& x, int stride, int pad, Epi ep, const Act* dst,
                    const std::string* fuse1x1, const std::string* lead1x1, const Act* lead_dst)
{
    Act out;
    if (!fuse1x1 && !ep.dup && !ep.ckbd && gate_needs_own_pass(name, x, stride, pad, ep)) return conv_gated_ref(name, x, stride, pad, ep, dst);
    if (!fuse1x1 && conv_kpacked(name, x, stride, pad, ep, dst, &out)) return out;
    if (!fuse1x1 && small_tensor_layer(name, x)) return conv_small(name, x, stride, pad, ep, dst);
    if (refnum && !fuse1x1 && !dst && stride == 2 && pad == 2 && !ep.res1 && !ep.mul && !ep.res2 && !ep.dup && !ep.ckbd) {
        Act o;  // a stride-2 transposed conv with a measured recipe (the hyper-synthesis stages)
        if (deconv_s2_ref(name, x, ep.act, &o)) return o;
    }
    ConvPlan cp = conv_plan(name, x, stride, pad, ep, dst, fuse1x1, lead1x1, lead_dst);
    conv_issue(cp);
    return cp.y;
}

int rgbd_elic::keep_taps(TapTable& t, int odd)
{
    int n = 0;
    for (int k = 0; k < t.n[0]; ++k) {
        if (((t.dy[0][k] + t.dx[0][k]) & 1) != odd) continue;
        t.dy[0][n] = t.dy[0][k];
        t.dx[0][n] = t.dx[0][k];
        t.wt[0][n] = t.wt[0][k];
        ++n;
    }
    for (int k = n; k < 25; ++k) t.dy[0][k] = t.dx[0][k] = t.wt[0][k] = 0;
    t.n[0] = (int8_t)n;
    return n;
}

void rgbd_elic::conv_anchor_in(const std::string& name, const Act& x, int pad, const Act& dst)
{
    static const bool off = getenv("RGBD_NO_ANCHOR_TAPS") != nullptr;
    ConvPlan cp = conv_plan(name, x, 1, pad, Epi(), &dst);
    if (off || g_force_ckbd || x.c < 128 || (!dry() && (!cp.ok || cp.a.nphase != 1 || cp.a.IS != 1 || cp.a.subpix))) {
        conv_issue(cp);
        return;
    }
    for (int par = 1; par <= 2; ++par) {
        ConvPlan h = cp;
        if (!dry()) {
            const int n = keep_taps(h.a.taps, par == 1 ? 0 : 1);  // anchor outputs (parity 1): dy + dx even
            h.a.ckbd = par;
            h.flops = cp.flops * 0.5;
            h.flops_exec = cp.flops * 0.5 * n / std::max(1, (int)cp.a.taps.n[0]);  // half the outputs, n of the taps
        }
        conv_issue(h);
    }
}

void rgbd_elic::conv2(int nm, const std::string n[2], const Act x[2], int stride, int pad, const Epi ep[2], const Act* const dst[2],
                      Act out[2], const std::string* const fuse1x1[2], const std::string* const lead1x1[2],
                      const Act* const lead_dst[2])
{
    if (nm == 1) {
        out[0] = conv(n[0], x[0], stride, pad, ep[0], dst ? dst[0] : nullptr, fuse1x1 ? fuse1x1[0] : nullptr,
                      lead1x1 ? lead1x1[0] : nullptr, lead_dst ? lead_dst[0] : nullptr);
        return;
    }
    if (!fuse1x1 && (gate_needs_own_pass(n[0], x[0], stride, pad, ep[0]) || gate_needs_own_pass(n[1], x[1], stride, pad, ep[1]))) {
        for (int m = 0; m < 2; ++m) out[m] = conv(n[m], x[m], stride, pad, ep[m], dst ? dst[m] : nullptr);
        return;
    }
    if (!fuse1x1) {
        Act o0;
        if (conv_kpacked(n[0], x[0], stride, pad, ep[0], dst ? dst[0] : nullptr, &o0)) {  // (the depth twin is of that kind too)
            out[0] = o0;
            out[1] = conv(n[1], x[1], stride, pad, ep[1], dst ? dst[1] : nullptr);
            return;
        }
    }
    if (!fuse1x1 && small_tensor_layer(n[0], x[0]) && small_tensor_layer(n[1], x[1])) {
        for (int m = 0; m < 2; ++m) out[m] = conv_small(n[m], x[m], stride, pad, ep[m], dst ? dst[m] : nullptr);
        return;
    }
    ConvPlan p[2];
    for (int m = 0; m < 2; ++m)
        p[m] = conv_plan(n[m], x[m], stride, pad, ep[m], dst ? dst[m] : nullptr, fuse1x1 ? fuse1x1[m] : nullptr,
                         lead1x1 ? lead1x1[m] : nullptr, lead_dst ? lead_dst[m] : nullptr);
    out[0] = p[0].y;
    out[1] = p[1].y;
    if (g_pair && (dry() || pairable(p[0], p[1]))) {
        conv_issue(p[0], &p[1]);
    } else {
        conv_issue(p[0]);
        conv_issue(p[1]);
    }
}

void rgbd_elic::copy_ch(const Act& src, const Act& dst)
{
    if (dry() || rc) return;
    const int r = launch_copy_channels(src.p, src.cs, dst.p, dst.cs, src.n * src.h * src.w, round_up(src.c, 4), s);
    if (r) fail(r);
}

bool rgbd_elic::fusable(const std::string& mid, const std::string& last, const Act& x, int groups)
{
    auto a = convs.find(mid + ".weight"), b = convs.find(last + ".weight");
    if (a == convs.end() || b == convs.end()) return false;
    const PackedConv &p3 = a->second, &p1 = b->second;
    if (p3.transposed || p1.transposed || p1.k != 1 || p3.k != 3 || p1.cin_pad != p3.cout_pad || p1.cout % 16) return false;
    if (refnum) {  // the fused tail runs its 1x1 as one chain: only when the reference's kernel has one reduce block there
        if (small_tensor_layer(mid, x) || small_tensor_layer(last, x)) return false;
        const std::vector<int>* bl = ref_blocks(0, p1.cin, p1.cout, x.h, x.w);
        if (bl && bl->size() > 1) return false;
    }
    return conv_fused_plan(p3.cout_pad, p1.cout_pad, p3.k * p3.k, x.n * groups, x.h, x.w, tile_mode) > 0;
}

bool rgbd_elic::lead_fusable(const std::string& last, const std::string& lead, const Act& x)
{
    static const bool off = getenv("RGBD_NO_FUSE_LEAD") != nullptr;
    if (off || g_fuse_lead_off || lead.empty()) return false;
    auto b = convs.find(last + ".weight"), c = convs.find(lead + ".weight");
    if (b == convs.end() || c == convs.end()) return false;
    const PackedConv &p1 = b->second, &p0 = c->second;
    if (refnum) {  // (as in fusable(): the leading 1x1 rides along only as a single reduce block)
        if (small_tensor_layer(lead, x)) return false;
        const std::vector<int>* bl = ref_blocks(0, p0.cin, p0.cout, x.h, x.w);
        if (bl && bl->size() > 1) return false;
    }
    return !p0.transposed && p0.k == 1 && p0.cin_pad == p1.cout_pad && p0.cout_pad == p1.cin_pad && p0.cout % 16 == 0 &&
           p1.cout_pad % 32 == 0;
}

void rgbd_elic::se_scale_to(const std::string& p, const Act& x, int mode, const Act& y, const float* means, int mstride)
{
    float* w0 = dense_of(p + ".fc.0.weight");
    float* w1 = dense_of(p + ".fc.2.weight");
    float* mean = means ? nullptr : (float*)arena.take((size_t)x.n * x.c * sizeof(float));
    float* sc = (float*)arena.take((size_t)x.n * x.c * sizeof(float));
    float* hid = (float*)arena.take((size_t)x.n * (x.c / 16 + 1) * sizeof(float));
    if (dry() || rc || !w0 || !w1) return;
    const int HW = x.h * x.w;
    int r = means ? RGBD_OK : (refnum ? launch_channel_mean_ref(x.p, x.n, HW, x.cs, x.c, mean, x.c, s)
                                      : launch_channel_mean(x.p, x.n, HW, x.cs, x.c, mean, s));
    const float* mu = means ? means : mean;
    if (!r && refnum)
        r = launch_se_fc_ref(mu, x.n, x.c, x.c / 16, w0, w1, cls_of(p + ".fc.0.weight"), cls_of(p + ".fc.2.weight"), hid, sc, s,
                             means ? mstride : 0, se_form());
    else if (!r) r = launch_se_fc(mu, x.n, x.c, x.c / 16, w0, w1, hid, sc, s, means ? mstride : 0, perm());
    if (!r) r = launch_channel_scale_to(x.p, x.n, HW, x.cs, x.c, sc, mode, y.p, y.cs, s);
    if (r) fail(r);
}

void rgbd_elic::se_cat_to(const std::string& p, const Act& own, const Act& other, const Act& f)
{
    const int C = own.c + other.c;
    float* w0 = dense_of(p + ".fc.0.weight");
    float* w1 = dense_of(p + ".fc.2.weight");
    float* mean = (float*)arena.take((size_t)own.n * C * sizeof(float));
    float* sc = (float*)arena.take((size_t)own.n * C * sizeof(float));
    float* hid = (float*)arena.take((size_t)own.n * (C / 16 + 1) * sizeof(float));
    if (C % 16 || own.c % 4) {
        fail(RGBD_EINVAL);
        return;
    }
    if (dry() || rc || !w0 || !w1) return;
    const int HW = own.h * own.w;
    int r = refnum ? launch_channel_mean_ref(own.p, own.n, HW, own.cs, own.c, mean, C, s)
                   : launch_channel_mean_strided(own.p, own.n, HW, own.cs, own.c, mean, C, s);
    if (!r)
        r = refnum ? launch_channel_mean_ref(other.p, other.n, HW, other.cs, other.c, mean + own.c, C, s)
                   : launch_channel_mean_strided(other.p, other.n, HW, other.cs, other.c, mean + own.c, C, s);
    if (!r && refnum)
        r = launch_se_fc_ref(mean, own.n, C, C / 16, w0, w1, cls_of(p + ".fc.0.weight"), cls_of(p + ".fc.2.weight"), hid, sc, s, 0, se_form());
    else if (!r) r = launch_se_fc(mean, own.n, C, C / 16, w0, w1, hid, sc, s, 0, perm());
    if (!r) r = launch_channel_scale_to_strided(own.p, own.n, HW, own.cs, own.c, sc, C, 0, f.p, f.cs, s);
    if (!r) r = launch_channel_scale_to_strided(other.p, other.n, HW, other.cs, other.c, sc + own.c, C, 0, f.p + own.c, f.cs, s);
    if (r) fail(r);
}

bool rgbd_elic::deconv_s2_ref(const std::string& name, const Act& x, int act, Act* out)
{
    if (!refnum) return false;
    const PackedConv* pc = conv_of(name + ".weight");
    if (!pc || !pc->transposed || pc->k != 5 || pc->subpix || x.cs != pc->cin_pad) return false;
    const std::vector<int>* rec = ref_blocks(3, pc->cin, pc->cout, x.h, x.w);
    if (!rec) return false;
    *out = alloc(x.n, 2 * x.h, 2 * x.w, pc->cout);
    ArenaScratch scratch{arena};
    const int r = deconv_s2_ref_run(*pc, rec->data(), rec->size(), x.p, x.n, x.h, x.w, act, out->p, out->cs, tile_mode,
                                    !dry() && !rc, s, scratch);
    if (r) fail(r);
    return true;
}
