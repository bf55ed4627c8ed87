// Host runtime of the gfx950 codec engine: weight packing (declared in engine.h).  A state-dict tensor becomes the operand of a
// conv kernel here -- the plain [cout_pad][taps][cin_pad] form, the sub-pixel form of the last transposed conv, the K-packed
// form of the first analysis conv -- as do SE_Block's transposed fc weight and the K blocks of the small-tensor route.
// Called by finalize (engine_abi.hip), the operator hooks (hooks_abi.hip) and conv_small (engine_conv.hip).
#include "engine.h"

namespace rgbd_rt {

int pack_conv(const HostTensor& w, const HostTensor* b, bool transposed, PackedConv* pc, DevGen* gen, int perm_in,
              int perm_out)
{
    if (w.shape.size() != 4 || w.shape[2] != w.shape[3]) return RGBD_EINVAL;
    const int k = (int)w.shape[2];
    const int cout = transposed ? (int)w.shape[1] : (int)w.shape[0];
    const int cin = transposed ? (int)w.shape[0] : (int)w.shape[1];
    pc->cin = cin;
    pc->cout = cout;
    pc->k = k;
    pc->transposed = transposed;
    pc->cin_pad = round_up(cin, 16);
    pc->cout_pad = round_up(cout, 16);
    const size_t n = (size_t)pc->cout_pad * k * k * pc->cin_pad;
    std::vector<float> h(n, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < k * k; ++t) {
                const size_t src = transposed ? (((size_t)ci * cout + co) * k * k + t) : (((size_t)co * cin + ci) * k * k + t);
                h[((size_t)rgbd_cperm(co, perm_out) * k * k + t) * pc->cin_pad + rgbd_cperm(ci, perm_in)] = w.v[src];
            }
    std::vector<float> hb(pc->cout_pad, 0.f);
    if (b) {
        if ((int)b->v.size() != cout) return RGBD_EINVAL;
        for (int co = 0; co < cout; ++co) hb[rgbd_cperm(co, perm_out)] = b->v[co];
    }
    HIP_TRY(hipMalloc((void**)&pc->w, n * sizeof(float)));
    if (gen) gen->p.push_back(pc->w);  // registered at once: a later failure leaves nothing behind
    HIP_TRY(hipMalloc((void**)&pc->bias, hb.size() * sizeof(float)));
    if (gen) gen->p.push_back(pc->bias);
    HIP_TRY(hipMemcpy(pc->w, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pc->bias, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice));
    return RGBD_OK;
}

void se_pack_fc2(const float* w1, size_t C, size_t Hd, float* w1t)
{
    for (size_t c = 0; c < C; ++c)
        for (size_t j = 0; j < Hd; ++j) w1t[j * C + c] = w1[c * Hd + j];
}

int pack_subpix(const HostTensor& w, const HostTensor* b, PackedConv* pc, DevGen* gen, int perm_in)
{
    if (w.shape.size() != 4 || w.shape[2] != 5 || w.shape[3] != 5 || w.shape[1] > 4) return RGBD_EINVAL;
    const int cin = (int)w.shape[0], cout = (int)w.shape[1];
    pc->cin = cin;
    pc->cout = cout;
    pc->k = 5;
    pc->transposed = true;
    pc->subpix = true;
    pc->cin_pad = round_up(cin, 16);
    pc->cout_pad = 16;
    std::vector<float> h((size_t)16 * 9 * pc->cin_pad, 0.f), hb(16, 0.f);
    for (int ry = 0; ry < 2; ++ry)
        for (int rx = 0; rx < 2; ++rx)
            for (int co = 0; co < cout; ++co) {
                const int row = (ry * 2 + rx) * 4 + co;
                if (b) hb[row] = b->v[co];
                for (int u = 0; u < 9; ++u) {
                    const int dy = 1 - u / 3, dx = 1 - u % 3;
                    const int ky = ry + 2 - 2 * dy, kx = rx + 2 - 2 * dx;
                    if (ky < 0 || ky > 4 || kx < 0 || kx > 4) continue;
                    for (int ci = 0; ci < cin; ++ci)
                        h[((size_t)row * 9 + u) * pc->cin_pad + rgbd_cperm(ci, perm_in)] = w.v[(((size_t)ci * cout + co) * 5 + ky) * 5 + kx];
                }
            }
    HIP_TRY(hipMalloc((void**)&pc->w, h.size() * sizeof(float)));
    if (gen) gen->p.push_back(pc->w);
    HIP_TRY(hipMalloc((void**)&pc->bias, hb.size() * sizeof(float)));
    if (gen) gen->p.push_back(pc->bias);
    HIP_TRY(hipMemcpy(pc->w, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pc->bias, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice));
    return RGBD_OK;
}

int pack_kpack(const HostTensor& w, const HostTensor* b, PackedConv* pc, DevGen* gen, int perm_out)
{
    if (w.shape.size() != 4 || w.shape[2] != 5 || w.shape[3] != 5 || w.shape[1] > 3) return RGBD_EINVAL;
    const int cout = (int)w.shape[0], cin = (int)w.shape[1], nterm = 25 * cin;
    HostTensor w1;
    const int KP = round_up(nterm, 16);
    w1.shape = {cout, KP, 1, 1};
    w1.v.assign((size_t)cout * KP, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int n = 0; n < nterm; ++n) {
            const int t = n / cin, c = n % cin, r = n % 16;
            w1.v[(size_t)co * KP + (n / 16) * 16 + (r % 4) * 4 + r / 4] = w.v[((size_t)co * cin + c) * 25 + t];
        }
    const int rc = pack_conv(w1, b, false, pc, gen, 0, perm_out);
    pc->cin = nterm;  // FLOP accounting: the real reduction length
    return rc;
}

int small_conv_set_kblocks(SmallConvArgs* a, const int* lens, int n, int Kt)
{
    a->nb = 1;
    a->kb[0] = 0;
    a->kb[1] = Kt;
    if (!lens) return RGBD_OK;
    if (n < 1 || n > 16) return RGBD_EINVAL;
    int pos = 0;
    a->nb = n;
    for (int b = 0; b < n; ++b) {
        if (lens[b] <= 0 || lens[b] > Kt - pos) return RGBD_EINVAL;
        pos += lens[b];
        a->kb[b + 1] = pos;
    }
    return pos == Kt ? RGBD_OK : RGBD_EINVAL;
}

}  // namespace rgbd_rt
