// Host runtime of the gfx950 codec engine: the layer graph of MLIC++ (family 19, models/mlicpp.py; declared in engine.h) -- its
// residual blocks, the four transforms, and the slice loop.  Composition only: every launch below is one the other families or
// the module handles (families 7-9, 15-17) issue already, plus mlic_lrp_apply_kernel (mlic_loop.hip) once per coding part.
#include "engine.h"

Act rgbd_elic::ml_res_block(const std::string& p, const Act& x)
{
    Epi e1, e2;
    e1.act = e2.act = ACT_RELU;
    const Act t = conv(p + ".conv1", x, 1, 1, e1);
    const Act id = convs.count(p + ".skip.weight") ? conv(p + ".skip", x, 1, 0) : x;  // (in_ch != out_ch: g_s's first block when M != N)
    e2.res2 = &id;
    return conv(p + ".conv2", t, 1, 1, e2);
}

Act rgbd_elic::ml_res_block_stride(const std::string& p, const Act& x)
{
    Epi gelu;
    gelu.act = ACT_GELU;
    const Act t = conv(p + ".conv2", conv(p + ".conv1", x, 2, 1, gelu), 1, 1);
    const Act id = conv(p + ".skip", x, 2, 0);
    return gdn(p + ".gdn", t, false, &id);
}

Act rgbd_elic::ml_res_block_up(const std::string& p, const Act& x)
{
    const std::string n[2] = {p + ".subpel_conv.0", p + ".upsample.0"};
    const Act xin[2] = {x, x};
    Epi ep[2];
    ep[0].act = ACT_GELU;  // (pointwise: it rides in front of the shuffle)
    Act t[2];
    conv2(2, n, xin, 1, 1, ep, nullptr, t);
    const Act u = conv(p + ".conv", pixel_shuffle(t[0]), 1, 1);
    const Act id = pixel_shuffle(t[1]);
    return gdn(p + ".igdn", u, true, &id);
}

Act rgbd_elic::g_a_mlic(const Act& img)
{
    const std::string root = "g_a.analysis_transform.";
    Phase ph(this, "phase.transforms");
    Act x = img;
    for (int i = 0; i < 3; ++i) {
        const std::string a = root + std::to_string(2 * i), b = root + std::to_string(2 * i + 1);
        x = ck_stage(x, [&](const Act& t) { return ml_res_block(b, ml_res_block_stride(a, t)); }, x.h / 2, x.w / 2, N);
    }
    return conv(root + "6", x, 2, 1);
}

Act rgbd_elic::g_s_mlic(const Act& yhat)
{
    const std::string root = "g_s.synthesis_transform.";
    Phase ph(this, "phase.transforms");
    Act x = yhat;
    for (int i = 0; i < 3; ++i) {
        const std::string a = root + std::to_string(2 * i), b = root + std::to_string(2 * i + 1);
        x = ck_stage(x, [&](const Act& t) { return ml_res_block_up(b, ml_res_block(a, t)); }, 2 * x.h, 2 * x.w, N);
    }
    return pixel_shuffle(conv(root + "7.0", ml_res_block(root + "6", x), 1, 1));
}

Act rgbd_elic::h_a_mlic(const Act& y)
{
    static const int strides[5] = {1, 1, 2, 1, 2};
    Epi gelu;
    gelu.act = ACT_GELU;
    Phase ph(this, "phase.transforms");
    Act t = y;
    for (int k = 0; k < 5; ++k) t = conv("h_a.reduction." + std::to_string(2 * k), t, strides[k], 1, k < 4 ? gelu : Epi());
    return t;
}

void rgbd_elic::h_s_mlic(const Act& zhat, const Act& dst)
{
    Epi gelu;
    gelu.act = ACT_GELU;
    const size_t mark = arena.top;
    Phase ph(this, "phase.transforms");
    Act t = conv("h_s.increase.0", zhat, 1, 1, gelu);
    t = pixel_shuffle(conv("h_s.increase.2.0", t, 1, 1, gelu));
    t = conv("h_s.increase.4", t, 1, 1, gelu);
    t = pixel_shuffle(conv("h_s.increase.6.0", t, 1, 1, gelu));
    conv("h_s.increase.8", t, 1, 1, Epi(), &dst);
    arena.top = mark;
}

// Per slice i, in the reference's order (mlicpp.py:220-303): [inter and channel context over the decoded slices, i >= 1,] anchor
// parameters, anchor part, anchor LRP, [intra context, i >= 1,] local context, non-anchor parameters, non-anchor part, non-anchor
// LRP.  While the anchor half of slot i is the only decoded one, its other half reads zero: code_part's anchor pass writes the
// zeros with the values (ckbd_part_kernel), which is what mlic_slot_clear_kernel would do in a launch of its own, and the LRP,
// local and intra networks see them as the reference's do (`slice_anchor` is zero off the anchor positions).  The LRP correction
// is added at the part's own parity only (mlicpp.py:235, 257), in place; the non-anchor LRP therefore reads the corrected anchors.
void rgbd_elic::slice_loop_mlic(Coding& cd, const Act* y, const Act& hyper, const Act& state)
{
    const int C = MLIC_SLOT_CH, B = state.n, h = state.h, w = state.w, S = (int)slice_ch.size();
    yhat_base[0] = state.p + M;
    const int64_t part_syms = (int64_t)C * h * (w / 2);
    const Act params = alloc(B, h, w, 2 * C);  // (scales | means) of the current slice: each part fills its own half of the pixels
    auto lrp = [&](const std::string& p, int i, const Act& slot, int parity) {
        const size_t mark = arena.top;
        Phase ph(this, "phase.lrp");
        const Act r = lrp_mlic(view(state, 0, M + C * (i + 1)), p, false);
        if (!dry() && !rc) {
            const int q = launch_mlic_lrp_apply(slot.p, slot.cs, r.p, r.cs, C, B, h, w, parity, s);
            if (q) fail(q);
        }
        arena.top = mark;
    };
    for (int i = 0; i < S; ++i) {
        const size_t mark = arena.top;
        const std::string si = std::to_string(i) + ".";
        const Act slot = view(state, M + C * i, C);
        const Act ys = y ? view(*y, C * i, C) : Act();
        const int64_t part_off = 2 * part_syms * i;
        Act inter, chan;
        if (i) {
            Phase ph(this, "phase.contexts");
            const Act prev = view(state, M, C * i);  // cat(y_hat_slices)
            inter = linear_context(prev, prev, prev, 0, true, "global_inter_context." + si, i);
            chan = channel_context_mlic(prev, "channel_context." + si);
        }
        {
            Phase ph(this, "phase.params");
            const Act seg[3] = {i ? inter : hyper, chan, hyper};
            entropy_params_mlic(seg, i ? 3 : 1, 1, &params, "entropy_parameters_anchor." + si, 2 * C);
        }
        {
            Phase ph(this, "phase.coder");
            code_part(cd, 0, 1, params, ys, slot, part_off);
        }
        lrp("lrp_anchor." + si, i, slot, 0);
        Act intra, local;
        {
            Phase ph(this, "phase.contexts");
            if (i) {
                // y_hat_slices[-1], split into its checkerboard halves (context.py:191-192); launch_ckbd_split takes one
                // channel stride for all three tensors, so the slot is copied out of the state buffer first
                const Act last = alloc(B, h, w, C), xa = alloc(B, h, w, C), xn = alloc(B, h, w, C);
                copy_ch(view(state, M + C * (i - 1), C), last);
                if (!dry() && !rc) {
                    const int q = launch_ckbd_split(last.p, B, h, w, last.cs, xa.p, xn.p, s);
                    if (q) fail(q);
                }
                intra = linear_context(xa, xn, slot, 1, false, "global_intra_context." + si, 2);
            }
            local = local_context(slot, "local_context." + si, 2);
        }
        {
            Phase ph(this, "phase.params");
            const Act seg[5] = {local, i ? intra : hyper, inter, chan, hyper};
            entropy_params_mlic(seg, i ? 5 : 2, 2, &params, "entropy_parameters_nonanchor." + si, 2 * C);
        }
        {
            Phase ph(this, "phase.coder");
            code_part(cd, 0, 0, params, ys, slot, part_off + part_syms);
        }
        lrp("lrp_nonanchor." + si, i, slot, 1);
        arena.top = mark;
    }
}
