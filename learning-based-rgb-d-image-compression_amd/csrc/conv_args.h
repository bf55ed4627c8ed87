// The one place where the fields of a ConvArgs (common.h) are decided.  Plain host functions: no engine state, no HIP call,
// no allocation.  The engine's planner (engine_conv.hip: conv_plan / plan_refnum / conv_issue; engine.h: deconv_s2_ref_run) and the stand-alone
// entry points of the C ABI (hooks_abi.hip: rgbd_conv2d_nchw, rgbd_conv2d_ref_nchw, rgbd_conv_forms_nchw, rgbd_conv_bench) all
// build their launches from these pieces, so a test of one of them tests the rules of all.  What stays with a caller is
// policy -- which layer, which split factor, which scratch -- never how a decision becomes fields.
// A new ConvArgs field needs: the helper here that sets it, a term in rgbd_elic::pairable (engine_conv.hip) and, for a pointer with a
// twin in ConvPtrs, a line in conv_args_group1 and in conv_groups_ok (conv_mfma.hip).
#pragma once
#include <algorithm>
#include <cstring>

#include "common.h"

namespace rgbd_rt {

struct PackedConv {
    float* w = nullptr;  // [cout_pad][k*k][cin_pad]
    float* bias = nullptr;
    int cin = 0, cout = 0, cin_pad = 0, cout_pad = 0, k = 0;
    bool transposed = false;
    bool subpix = false;  // pack_subpix(): [16 = phase * 4 + cout][9 taps][cin_pad] of a k = 5, stride-2 transposed conv
};

// output extent of Conv2d / ConvTranspose2d (output_padding = stride - 1)
inline void conv_out_hw(int h, int w, int k, int stride, int pad, bool transposed, int* OH, int* OW)
{
    if (!transposed) {
        *OH = (h + 2 * pad - k) / stride + 1;
        *OW = (w + 2 * pad - k) / stride + 1;
    } else {
        *OH = (h - 1) * stride - 2 * pad + k + (stride - 1);
        *OW = (w - 1) * stride - 2 * pad + k + (stride - 1);
    }
}

inline void make_taps_subpix(ConvArgs* a)
{
    memset(&a->taps, 0, sizeof(a->taps));
    a->nphase = 1;
    a->IS = 1;
    a->OS = 2;
    a->subpix = 1;
    for (int u = 0; u < 9; ++u) {
        a->taps.dy[0][u] = (int8_t)(1 - u / 3);
        a->taps.dx[0][u] = (int8_t)(1 - u % 3);
        a->taps.wt[0][u] = (int8_t)u;
    }
    a->taps.n[0] = 9;
    a->min_dy = a->min_dx = -1;
    a->span_y = a->span_x = 3;
}

inline void make_taps(const PackedConv& pc, int stride, int pad, ConvArgs* a)
{
    const int k = pc.k;
    memset(&a->taps, 0, sizeof(a->taps));
    if (!pc.transposed) {
        a->nphase = 1;
        a->IS = stride;
        a->OS = 1;
        int n = 0;
        for (int ky = 0; ky < k; ++ky)
            for (int kx = 0; kx < k; ++kx) {
                a->taps.dy[0][n] = (int8_t)(ky - pad);
                a->taps.dx[0][n] = (int8_t)(kx - pad);
                a->taps.wt[0][n] = (int8_t)(ky * k + kx);
                ++n;
            }
        a->taps.n[0] = (int8_t)n;
        a->min_dy = a->min_dx = -pad;
        a->span_y = a->span_x = k;
        return;
    }
    // transposed: o = i*s - pad + k  =>  for o = s*t + r: i = t + (r + pad - k)/s for k == (r + pad) mod s
    a->nphase = stride * stride;
    a->IS = 1;
    a->OS = stride;
    int mn = 127, mx = -127;
    for (int ry = 0; ry < stride; ++ry)
        for (int rx = 0; rx < stride; ++rx) {
            const int ph = ry * stride + rx;
            int n = 0;
            for (int ky = 0; ky < k; ++ky) {
                if ((ry + pad - ky) % stride) continue;
                for (int kx = 0; kx < k; ++kx) {
                    if ((rx + pad - kx) % stride) continue;
                    const int dy = (ry + pad - ky) / stride, dx = (rx + pad - kx) / stride;
                    a->taps.dy[ph][n] = (int8_t)dy;
                    a->taps.dx[ph][n] = (int8_t)dx;
                    a->taps.wt[ph][n] = (int8_t)(ky * k + kx);
                    mn = std::min(mn, std::min(dy, dx));
                    mx = std::max(mx, std::max(dy, dx));
                    ++n;
                }
            }
            a->taps.n[ph] = (int8_t)n;
        }
    a->min_dy = a->min_dx = mn;
    a->span_y = a->span_x = mx - mn + 1;
}

// the layer and its two tensors: x [N][H][W][xcs] -> y [N][OH][OW][ycs] (both already offset to their first channel), the
// packed weights, the tap table of the form `pc` was packed for (per-phase, or sub-pixel: pack_subpix) and the tile grid
inline void conv_args_geometry(ConvArgs* a, const PackedConv& pc, const float* x, int N, int H, int W, int xcs, float* y, int ycs,
                               int OH, int OW, int stride, int pad)
{
    a->x = x;
    a->N = N;
    a->H = H;
    a->W = W;
    a->xcs = xcs;
    a->cin_pad = pc.cin_pad;
    a->w = pc.w;
    a->ntaps_total = pc.subpix ? 9 : pc.k * pc.k;
    a->bias = pc.bias;
    a->y = y;
    a->OH = OH;
    a->OW = OW;
    a->ycs = ycs;
    a->cout_pad = pc.cout_pad;
    if (pc.subpix) make_taps_subpix(a);
    else make_taps(pc, stride, pad, a);
    a->GH = pc.transposed ? H : OH;
    a->GW = pc.transposed ? W : OW;
}

// channels a launch stores for an output of c channels in a buffer of channel stride cs: a channel slice narrower than its
// 16-padded width inside a wider buffer (STF_united: 24 of 48) stops at the slice end; a buffer of its own gets its pad
// channels zeroed as usual
inline int conv_cout_store(int c, int cs) { return (c % 16 && cs != round_up(c, 16)) ? round_up(c, 4) : round_up(c, 16); }

// activation, checkerboard half and the optional operands (a null pointer leaves its stride at 0)
inline void conv_args_epilogue(ConvArgs* a, int act, int ckbd, const float* res1, int r1cs, const float* mul, int mcs,
                               const float* res2, int r2cs, float* y2, int y2cs)
{
    a->act = act;
    a->ckbd = ckbd;
    if (res1) a->res1 = res1, a->r1cs = r1cs;
    if (mul) a->mul = mul, a->mcs = mcs;
    if (res2) a->res2 = res2, a->r2cs = r2cs;
    if (y2) a->y2 = y2, a->y2cs = y2cs;
}

// fused trailing 1x1 (launch_conv_fused); in reference arithmetic its chains start at the bias
inline void conv_args_tail(ConvArgs* a, const PackedConv& pc2, int act_mid, bool refmode)
{
    a->w2 = pc2.w;
    a->bias2 = pc2.bias;
    a->cout2_pad = pc2.cout_pad;
    a->act_mid = act_mid;
    if (refmode) a->tail_bias_init = 1;
}

// ... and the leading 1x1 + ReLU of the block that follows, written to y3
inline void conv_args_lead(ConvArgs* a, const PackedConv& pc3, float* y3, int y3cs)
{
    a->w3 = pc3.w;
    a->bias3 = pc3.bias;
    a->y3 = y3;
    a->y3cs = y3cs;
    a->cout3_pad = pc3.cout_pad;
}

// blocked accumulation for a layer of a->cin_pad channels: block lengths in channels (multiples of 16 but for the last;
// nullptr = every 16-channel chunk is a block, the multi-tap kernels of the reference's CPU library) -> blk_end, blocked
inline int conv_set_blocks(ConvArgs* a, const int* blocks, int nblocks)
{
    memset(a->blk_end, 0, sizeof(a->blk_end));
    const int n16 = a->cin_pad / 16;
    if (n16 > 256) return RGBD_EINVAL;
    if (!blocks || nblocks <= 0) {
        for (int c = 0; c < n16; ++c) a->blk_end[c >> 5] |= 1u << (c & 31);
    } else {
        int pos = 0;
        for (int b = 0; b < nblocks; ++b) {
            if (blocks[b] <= 0 || (blocks[b] % 16 && b + 1 < nblocks)) return RGBD_EINVAL;
            pos += blocks[b];
            const int c = (pos + 15) / 16 - 1;
            if (c >= n16) return RGBD_EINVAL;
            a->blk_end[c >> 5] |= 1u << (c & 31);
        }
        if ((pos + 15) / 16 != n16) return RGBD_EINVAL;
    }
    a->blocked = 1;
    return RGBD_OK;
}

// the blocks (lengths in channels) as split-K ranges of the single-chain kernel: split b reduces block b, the ordered
// reducer adds the block sums -> splitk, split_c16.  At most 16 blocks (split_c16 has 18 entries), none empty, none past the
// layer's last chunk; anything stricter (multiples of 16, the sum) is the caller's.
inline int conv_set_split_ranges(ConvArgs* a, const int* blocks, int nblocks)
{
    const int n16 = a->cin_pad / 16;
    if (!blocks || nblocks < 1 || nblocks > 16 || n16 > 65535) return RGBD_EINVAL;
    int pos = 0;
    for (int b = 0; b < nblocks; ++b) {
        if (blocks[b] <= 0 || blocks[b] > 16 * n16 - pos) return RGBD_EINVAL;
        a->split_c16[b] = (uint16_t)(pos / 16);
        pos += blocks[b];
    }
    a->split_c16[nblocks] = (uint16_t)((pos + 15) / 16);
    a->splitk = nblocks;
    return RGBD_OK;
}

// taps of the longest phase: what the split-K rule (conv_splitk_for) calls taps per phase
inline int conv_max_taps(const ConvArgs& a)
{
    int mt = 1;
    for (int ph = 0; ph < a.nphase; ++ph) mt = std::max(mt, (int)a.taps.n[ph]);
    return mt;
}

// second operand set of a grouped launch: the pointers of b, a launch of the same shape (the caller has checked that:
// rgbd_elic::pairable).  The split-K planes of the two sets (partial, g1.partial) stay with the caller.
inline void conv_args_group1(ConvArgs* a, const ConvArgs& b)
{
    a->groups = 2;
    a->g1.x = b.x;
    a->g1.w = b.w;
    a->g1.bias = b.bias;
    a->g1.y = b.y;
    a->g1.res1 = b.res1;
    a->g1.mul = b.mul;
    a->g1.res2 = b.res2;
    a->g1.y2 = b.y2;
    a->g1.w2 = b.w2;
    a->g1.bias2 = b.bias2;
    a->g1.w3 = b.w3;
    a->g1.bias3 = b.bias3;
    a->g1.y3 = b.y3;
}

}  // namespace rgbd_rt
