// Host runtime of the gfx950 codec engine: the engine's side of the C ABI of include/rgbd_amd.h -- the wait
// policy, engine life cycle (create / finalize / clone / destroy), the codec and module entry points and the per-engine
// debug readers.  The operator-level entry points, test hooks and debug switches live in hooks_abi.hip, the coder's
// stand-alone entry points in coder_abi.hip.
#include "engine.h"

namespace {

// Wait policy of the host threads: they sleep while they wait for the GPU instead of spinning (hipDeviceScheduleBlockingSync, a
// device flag of the process).  Work submitted under one policy and awaited under the other is what the two "hipFree never
// returns" records have in common (profiles/r03_hang_diagnosis.txt; round 4: an engine that had run under the spinning policy
// was garbage-collected -- rgbd_elic_destroy -> hipFree -> every stream of the device -- right after a CodecPool had switched
// the policy).  So the policy does not move while an engine exists: the FIRST engine created on a device switches that device
// to sleeping waits (what every pooled or pipelined user wants, and ~1 ms of a 190 ms call for a lone one) before it has
// launched anything, the device is drained under the OLD policy before the flag changes, rgbd_set_blocking_sync() refuses
// (RGBD_ESTATE) while any engine is alive, and the Python side collects garbage engines first (pool.py).  RGBD_SPIN_WAIT=1
// keeps the runtime's default (spinning) policy for the whole process.  (Measured and dropped: the spinning policy around
// every hipFree -- with a pool's other threads launching in that window it produced exactly such mixed waits: the suite hung.)
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

// ---- life cycle ---------------------------------------------------------------------------------------------------
// The one place a descriptor is filled, every field once (clone_shared comes here directly: its source's values were checked)
rgbd_elic* engine_make(Family f, int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, int32_t in_ch, int32_t out_ch,
                       int32_t heads)
{
    rgbd_elic* m = new rgbd_elic();
    m->family = f;
    m->N = N;
    m->M = M;
    m->slice_ch.assign(slice_ch, slice_ch + n_slices);
    m->in_ch = in_ch;
    m->out_ch = out_ch;
    m->ctx_heads = heads;
    if (!family_row(f).refnum) m->refnum = false;  // (nothing sets it later: perm() is 0 in this family's call paths)
    ++g_live_engines;
    return m;
}

// A new engine: what every family requires of N, M and the slices, the wait policy, then the descriptor
int engine_new(Family f, int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, int32_t in_ch, int32_t out_ch,
               int32_t heads, rgbd_elic** out)
{
    if (!out || !slice_ch || n_slices <= 0 || N % 16 || M % 16) return RGBD_EINVAL;
    int sum = 0;
    for (int i = 0; i < n_slices; ++i) {
        if (slice_ch[i] <= 0 || slice_ch[i] % 8) return RGBD_EINVAL;  // 16-byte channel views; STF_united has 24-wide slices
        sum += slice_ch[i];
    }
    if (sum != M) return RGBD_EINVAL;
    if (const int pr = ensure_wait_policy()) return pr;
    *out = engine_make(f, N, M, slice_ch, n_slices, in_ch, out_ch, heads);
    return RGBD_OK;
}

// A module alone: no codec, no tables.  N, M and the one slice are the aligner's embed_dim; the contexts read none of them.
int module_new(Family f, int32_t in_ch, int32_t out_ch, int32_t heads, rgbd_elic** out)
{
    const int32_t slice = 96;
    return engine_new(f, 96, 96, &slice, 1, in_ch, out_ch, heads, out);
}

int check_ready(const rgbd_elic* m)
{
    if (m && !m->row().codec) return RGBD_EINVAL;  // a Spatial_aligner or context handle has no codec calls
    if (!m || !m->finalized || !m->scale_table) return RGBD_ESTATE;
    for (int i = 0; i < 4; ++i)
        if (!m->tables[i].ready && !(m->single() && (i & 1))) return RGBD_ESTATE;  // single-modal: slots 0 and 2
    return RGBD_OK;
}

int module_ready(const rgbd_elic* m, Family f)
{
    if (!m || m->family != f) return RGBD_EINVAL;
    return m->finalized ? RGBD_OK : RGBD_ESTATE;
}

// ---- the call frame of every entry point that runs through the graph cache -------------------------------------------
// An entry point is its readiness check, its own argument predicate, the key of its call shape and a body; what follows
// the body differs between the directions, as it always has (kept as it is, not judged here):
struct Tail {
    bool wait;  // wait_stream() after a successful body
    enum { kNever, kAlways, kOnSuccess } profile;  // when profile_collect() runs (only with rgbd_elic_set_profile on)
};
// compress ends with a stream synchronise of its own (the streams are on the host), so there is nothing to wait for; the
// launches of a failed call are collected too
constexpr Tail kCompressTail = {false, Tail::kAlways};
// decompress returns when x_hat is there: the caller's wait happens here, on an event the host thread sleeps on (a pooled
// rank has 16 of them; the work may sit on the engine's own stream); a failed call collects nothing
constexpr Tail kDecompressTail = {true, Tail::kOnSuccess};
// forward and the module calls are asynchronous on the caller's stream and are not profiled
constexpr Tail kForwardTail = {false, Tail::kNever};

template <class... A>
std::string call_key(const char* fmt, A... a)  // the graph-cache key of a call shape
{
    char s[96];
    snprintf(s, sizeof(s), fmt, a...);
    return s;
}

template <class Body>
int run_call(rgbd_elic* m, void* stream, const std::string& key, Tail tail, Body&& body)
{
    if (const int ur = m->use_stream(stream)) return ur;
    int r = run_sized(m, key, body);
    if (tail.wait && !r) r = m->wait_stream();
    if (m->dec_err_pending) {  // a wide-coder decompress: its error flag arrived with the wait
        m->dec_err_pending = false;
        if (tail.wait && !r && m->res_pin[rgbd_elic::kResPinBytes / sizeof(int64_t) - 1]) r = RGBD_EINVAL;
    }
    if ((m->profile || m->profile_phases) && (tail.profile == Tail::kAlways || (tail.profile == Tail::kOnSuccess && !r))) m->profile_collect();
    return r;
}

inline bool hw64(int32_t B, int32_t H, int32_t W) { return B > 0 && H > 0 && W > 0 && !(H % 64) && !(W % 64); }
inline bool one_or_b(int32_t n_y, int32_t B) { return n_y == 1 || n_y == B; }
// MLIC++ runs 3x3 layers on the z grid (h_a, h_s): a z map of one row or one column is refused before any launch, as the 3x3
// modules refuse H < 2 or W < 2 -- image sides of at least 128
inline bool z_grid_ok(const rgbd_elic* m, int32_t zh, int32_t zw) { return m->family != Family::MLIC || (zh >= 2 && zw >= 2); }
// ELIC_master_latent: f [B,128,H,W] and f_hat [B,N,H,W] are full-resolution tensors of many channels; the layout kernels index
// them with 32 bits
inline bool master_ok(const rgbd_elic* m, int32_t B, int64_t H, int64_t W)
{
    return m->family == Family::ELIC_master_latent && (int64_t)B * std::max(m->in_ch, m->out_ch) * H * W <= 0x7fffffff;
}

// ---- finalize, first half: what a tensor of the state dict is ---------------------------------------------------------
bool ends_with(const std::string& s, const char* suf)
{
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

// Name, shape and family decide, nothing else (no HIP call, no engine state: rgbd_debug_tensor_kind asks on any machine).  The
// order of the tests is part of the rule: the 2x2 recovery deconv and the contexts' dense weights are 4-D `.weight` tensors too.
int tensor_kind(Family f, const std::string& name, const int64_t* shape, int ndim)
{
    const bool weight = ends_with(name, ".weight");
    // MLIC++ holds ten of each context and per-slice network under these prefixes (mlicpp.py:40-75); behind the prefix the names
    // are the module handles' and so are the kinds
    const bool mlic = f == Family::MLIC;
    // ELIC_master_latent reads none of ELIC_master's outer blocks (elic_master.py:104-107): a checkpoint's entries under these
    // prefixes are not this family's
    if (f == Family::ELIC_master_latent)
        for (const char* outer : {"aux_encoder.", "master_encoder.", "master_decoder.", "channel_aligner."})
            if (name.rfind(outer, 0) == 0) return RGBD_KIND_IGNORED;
    const bool mlic_local = mlic && name.rfind("local_context.", 0) == 0;
    const bool mlic_ctx = mlic_local || (mlic && (name.rfind("global_inter_context.", 0) == 0 || name.rfind("global_intra_context.", 0) == 0));
    if (ends_with(name, "recovery.weight") && ndim == 4 && shape[2] == 2 && shape[3] == 2) return RGBD_KIND_RECOVERY_DECONV;
    if (family_row(f).dense4d && weight && ndim == 4 && (mlic ? (mlic_local && ends_with(name, ".fusion.weight")) : name == "fusion.weight"))
        return RGBD_KIND_CONTEXT_DENSE;
    if (family_row(f).dense4d && weight && ndim == 4 && (!mlic || mlic_ctx) && shape[1] == 1 && shape[2] == 3 && shape[3] == 3)
        return RGBD_KIND_CONTEXT_DENSE;
    // EntropyParametersMLIC.fusion.{0,2,4,6}: packed twice, for the conv kernels and as the fragments of launch_pixel_mlp4
    if (f == Family::EntropyParametersMLIC && weight && ndim == 4 && shape[2] == 1 && shape[3] == 1 && name.rfind("fusion.", 0) == 0)
        return RGBD_KIND_PIXEL_MLP;
    if (mlic && weight && ndim == 4 && shape[2] == 1 && shape[3] == 1 && name.rfind("entropy_parameters_", 0) == 0 &&
        name.find(".fusion.") != std::string::npos)
        return RGBD_KIND_PIXEL_MLP;
    if (weight && ndim == 4) {
        // ConvTranspose2d layers: g_s stages 1/6/12/17 and the h_s deconvs (single-modal ELIC: g_s stages 1/5/10/14 and
        // h_s.increase.*; stage numbers that are not a bare "<stage>.weight" in the other model belong to blocks with
        // sub-names, so the union is unambiguous; ELIC_master_latent: "g_s.synthesis_transform.{1,5,10,14}.weight", the same rule)
        bool transposed = name.find(".deconv.") != std::string::npos || (!mlic && name.rfind("h_s.increase.", 0) == 0);
        if (!mlic && name.rfind("g_s.", 0) == 0)  // (MLIC++'s transforms hold no transposed convolution: sub-pixel convs throughout)
            for (const char* suf : {"_transform.1.weight", "_transform.6.weight", "_transform.12.weight", "_transform.17.weight",
                                    "_transform.5.weight", "_transform.10.weight", "_transform.14.weight"})
                transposed = transposed || ends_with(name, suf);
        // SynthesisTransformPlus names its stages without a "g_s." in front: the four bare "<stage>.weight" are its deconvs
        if (f == Family::SynthesisTransformPlus)
            for (const char* full : {"synthesis_transform.1.weight", "synthesis_transform.5.weight", "synthesis_transform.10.weight",
                                     "synthesis_transform.14.weight"})
                transposed = transposed || name == full;
        return transposed ? RGBD_KIND_CONV_TRANSPOSED : RGBD_KIND_CONV;
    }
    if (ends_with(name, ".gamma") && ndim == 2 && shape[0] == shape[1]) return RGBD_KIND_GDN_GAMMA;
    if (weight && ndim == 2) return RGBD_KIND_LINEAR;
    // Swin LayerNorm affine parameters and relative position bias tables; LocalContext names its own without a module prefix
    const bool local = f == Family::LocalContext;
    if ((ndim == 1 && (name.find(".norm") != std::string::npos || (local && name.rfind("norm", 0) == 0))) ||
        ends_with(name, "relative_position_bias_table") || (local && name == "relative_position_table") ||
        (mlic_local && ends_with(name, ".relative_position_table")))
        return RGBD_KIND_ARRAY;
    if (ends_with(name, "entropy_bottleneck.quantiles")) return RGBD_KIND_QUANTILES;
    return RGBD_KIND_IGNORED;
}

// ---- finalize, second half: one packer per kind, into the generation that finalize swaps in ----------------------------
struct Packer {
    const rgbd_elic* m;
    DevGen* gen;  // owner of everything packed here
    std::map<std::string, PackedConv> convs;
    std::map<std::string, float*> dense;

    const HostTensor* raw(const std::string& name) const
    {
        auto it = m->raw.find(name);
        return it == m->raw.end() ? nullptr : &it->second;
    }
    // "<layer>.weight" / "<layer>.gamma" -> "<layer>.<what>"
    static std::string sibling(const std::string& n, const char* suffix, const char* what) { return n.substr(0, n.size() - strlen(suffix)) + what; }
    int dev_copy(const float* src, size_t n, float** out)
    {
        float* d = nullptr;
        HIP_TRY(hipMalloc((void**)&d, n * sizeof(float)));
        gen->p.push_back(d);
        HIP_TRY(hipMemcpy(d, src, n * sizeof(float), hipMemcpyHostToDevice));
        *out = d;
        return RGBD_OK;
    }

    // Spatial_aligner.recovery = ConvTranspose2d(96, out, 2, 2) (spatialAligner.py:372-374): its taps do not overlap, so
    // it is a 1x1 convolution to output channel co * 4 + dy * 2 + dx followed by a pixel shuffle (spatial_aligner()).
    // Packed in plain channel order: the aligner runs the single-chain arithmetic.
    int pack_recovery_deconv(const std::string& name, const HostTensor& t)
    {
        const int ci_n = (int)t.shape[0], co_n = (int)t.shape[1];
        HostTensor w1, b1;
        w1.shape = {4 * co_n, ci_n, 1, 1};
        w1.v.resize((size_t)4 * co_n * ci_n);
        for (int ci = 0; ci < ci_n; ++ci)
            for (int co = 0; co < co_n; ++co)
                for (int tap = 0; tap < 4; ++tap) w1.v[(size_t)(co * 4 + tap) * ci_n + ci] = t.v[((size_t)ci * co_n + co) * 4 + tap];
        const HostTensor* bias = raw(sibling(name, "weight", "bias"));
        if (bias) {
            if ((int)bias->v.size() != co_n) return RGBD_EINVAL;
            b1.shape = {4 * co_n};
            b1.v.resize((size_t)4 * co_n);
            for (int i = 0; i < 4 * co_n; ++i) b1.v[i] = bias->v[i / 4];
        }
        PackedConv pc;
        if (const int r = pack_conv(w1, bias ? &b1 : nullptr, false, &pc, gen, 0, 0)) return r;
        convs[name] = pc;
        return RGBD_OK;
    }

    // the contexts of MLIC++: LocalContext.fusion (read by the attention launch in the reference's [2C][C][5][5] layout) and
    // the depthwise 3x3 layers ([C][1][3][3]) go to the device as they are, with their biases
    int pack_context_dense(const std::string& name, const HostTensor& t)
    {
        const std::string bname = sibling(name, "weight", "bias");
        const HostTensor* bias = raw(bname);
        if (!bias || (int64_t)bias->v.size() != t.shape[0]) return RGBD_EINVAL;
        float *dw = nullptr, *db = nullptr;
        if (const int r = dev_copy(t.v.data(), t.v.size(), &dw)) return r;
        if (const int r = dev_copy(bias->v.data(), bias->v.size(), &db)) return r;
        dense[name] = dw;
        dense[bname] = db;
        return RGBD_OK;
    }

    int pack_conv_layer(const std::string& name, const HostTensor& t, bool transposed)
    {
        const HostTensor* bias = raw(sibling(name, "weight", "bias"));
        const bool ckbd = m->family == Family::Cheng2020_ckbd;
        // refnum: activations store their channels permuted (rgbd_cperm) -- except the network's input (read channel by
        // channel by the K-packing gather) and its output images (<= 4 channels, converted straight to NCHW)
        const int pm = m->perm();
        const int k0 = (int)t.shape[2];
        const int cin0 = transposed ? (int)t.shape[0] : (int)t.shape[1], cout0 = transposed ? (int)t.shape[1] : (int)t.shape[0];
        const bool image_in = !transposed && cin0 <= 3 && k0 == 5, image_out = transposed && cout0 <= 4 && k0 == 5;
        const HostTensor* src = &t;
        HostTensor masked;
        if (ckbd && name == "context_prediction.weight") {
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
        PackedConv pc;
        if (const int r = pack_conv(*src, bias, transposed, &pc, gen, image_in ? 0 : pm, image_out ? 0 : pm)) return r;
        convs[name] = pc;
        if (ckbd && name == "entropy_parameters.0.weight") {
            // the anchor pass (Cheng2020withCKBD.py:122-123) feeds zeros into the context half of this layer's input
            // channels [ctx 2M | hyper 2M]: the same layer on the hyper half alone
            const int half = cin0 / 2;
            HostTensor hw;
            hw.shape = {cout0, half, 1, 1};
            hw.v.resize((size_t)cout0 * half);
            for (int co = 0; co < cout0; ++co)
                for (int ci = 0; ci < half; ++ci) hw.v[(size_t)co * half + ci] = t.v[(size_t)co * cin0 + half + ci];
            PackedConv ph;
            if (const int r = pack_conv(hw, bias, false, &ph, gen, 0, 0)) return r;
            convs["entropy_parameters.0.hyper.weight"] = ph;
        }
        if (!transposed && pc.cin <= 3 && pc.k == 5) {  // the image-consuming layer: also as a 1x1 over a K-packed input
            PackedConv pk;
            if (const int r = pack_kpack(t, bias, &pk, gen, pm)) return r;
            convs[sibling(name, "weight", "kpack.weight")] = pk;
        }
        if (transposed && pc.cout <= 4 && pc.k == 5) {  // the image-producing layer: also in its sub-pixel form
            PackedConv ps;
            if (const int r = pack_subpix(t, bias, &ps, gen, pm)) return r;
            convs[sibling(name, "weight", "subpix.weight")] = ps;
        }
        return RGBD_OK;
    }

    // a 1x1 layer of EntropyParametersMLIC: as every Conv2d (the four conv() launches of the unfused form; its bias is read
    // by both forms), and "<layer>.fragments" for launch_pixel_mlp4.  Channel counts that are no multiples of 16 are refused.
    int pack_pixel_mlp(const std::string& name, const HostTensor& t)
    {
        if (t.shape[0] % 16 || t.shape[1] % 16) return RGBD_EINVAL;
        if (const int r = pack_conv_layer(name, t, false)) return r;
        std::vector<float> frag(t.v.size());
        if (const int r = pixel_mlp4_pack(t.v.data(), (int)t.shape[0], (int)t.shape[1], frag.data())) return r;
        return dev_copy(frag.data(), frag.size(), &dense[sibling(name, "weight", "fragments")]);
    }

    // GDN / IGDN (layers/gdn.py): NonNegativeParametrizer.forward applied once here, in fp32; packed for gdn.hip
    int pack_gdn_gamma(const std::string& name, const HostTensor& t)
    {
        const std::string bname = sibling(name, "gamma", "beta");
        const HostTensor* beta = raw(bname);
        const int C = (int)t.shape[0];
        if (!beta || (int)beta->v.size() != C || C > 512) return RGBD_EINVAL;
        std::vector<float> hb, hg;
        gdn_pack(beta->v.data(), t.v.data(), C, &hb, &hg);
        float *db = nullptr, *dg = nullptr;
        if (const int r = dev_copy(hb.data(), hb.size(), &db)) return r;
        if (const int r = dev_copy(hg.data(), hg.size(), &dg)) return r;
        dense[bname] = db;
        dense[name] = dg;
        return RGBD_OK;
    }

    // SE_Block linears; fc.2 ([C][hidden]) is kept transposed so the gate kernel reads it coalesced
    int pack_linear(const std::string& name, const HostTensor& t)
    {
        std::vector<float> hv = t.v;
        const bool fc0 = ends_with(name, ".fc.0.weight"), fc2 = ends_with(name, ".fc.2.weight");
        if (m->refnum && (fc0 || fc2)) {
            // the reference's Linear on one vector: per-row accumulation class, measured per layer shape
            const int J = (int)t.shape[0], K = (int)t.shape[1];
            auto ct = m->ref_tab->blocks.find({2, K, J, 0, 0, 1});
            if (ct != m->ref_tab->blocks.end() && (int)ct->second.size() == J) {
                float* dcls = nullptr;
                if (const int r = dev_copy(reinterpret_cast<const float*>(ct->second.data()), (size_t)J, &dcls)) return r;
                dense[name + ".rowclass"] = dcls;
            }
        }
        if (fc2 && !m->refnum) se_pack_fc2(t.v.data(), (size_t)t.shape[0], (size_t)t.shape[1], hv.data());
        return dev_copy(hv.data(), hv.size(), &dense[name]);
    }

    // Swin LayerNorm affine parameters and relative position bias tables: plain device arrays
    int pack_array(const std::string& name, const HostTensor& t) { return dev_copy(t.v.data(), t.v.size(), &dense[name]); }

    // the factorised prior: medians = quantiles[:, 0, 1] (entropy_models.py:316-318), and softplus(matrix_i) / bias_i /
    // tanh(factor_i) per channel for the eval-mode likelihood (58 floats/channel) when the state dict holds all of them
    int pack_quantiles(const std::string& name, const HostTensor& t)
    {
        const int C = (int)t.shape[0];
        const std::string pre = name.substr(0, name.size() - 9);
        std::vector<float> med(C);
        for (int c = 0; c < C; ++c) med[c] = t.v[(size_t)c * 3 + 1];
        float* d = nullptr;
        if (const int r = dev_copy(med.data(), (size_t)C, &d)) return r;
        dense[pre + "medians"] = d;
        const int fi[6] = {1, 3, 3, 3, 3, 1};
        const float *mat[5] = {}, *bias[5] = {}, *fac[4] = {};
        for (int i = 0; i < 5; ++i) {
            const HostTensor* mi = raw(pre + "_matrix" + std::to_string(i));
            const HostTensor* bi = raw(pre + "_bias" + std::to_string(i));
            const HostTensor* fa = i < 4 ? raw(pre + "_factor" + std::to_string(i)) : nullptr;
            if (!mi || !bi || (i < 4 && !fa)) return RGBD_OK;  // (medians only)
            const size_t no = (size_t)fi[i + 1], ni = (size_t)fi[i];
            if (mi->v.size() != C * no * ni || bi->v.size() != C * no || (i < 4 && fa->v.size() != C * no)) return RGBD_EINVAL;
            mat[i] = mi->v.data();
            bias[i] = bi->v.data();
            if (i < 4) fac[i] = fa->v.data();
        }
        std::vector<float> prm((size_t)C * 58, 0.f);
        eb_pack_cumulative(mat, bias, fac, C, prm.data());
        float* dp = nullptr;
        if (const int r = dev_copy(prm.data(), prm.size(), &dp)) return r;
        dense[pre + "cumulative"] = dp;
        return RGBD_OK;
    }
};

}  // namespace

// ==== C ABI ========================================================================================================
extern "C" {

int rgbd_abi_version(void) { return RGBD_AMD_ABI_VERSION; }

int rgbd_get_blocking_sync(void)
{
    unsigned flags = 0;
    HIP_TRY(hipGetDeviceFlags(&flags));
    return (flags & hipDeviceScheduleMask) == hipDeviceScheduleBlockingSync ? 1 : 0;
}

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

// ---- codec: the create entry points check the limits of their own family, engine_new the common ones ------------------
int rgbd_elic_create(int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, rgbd_elic** out)
{
    return engine_new(Family::ELIC_united, N, M, slice_ch, n_slices, 3, 0, 0, out);
}

int rgbd_elic_create_r2d(int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, rgbd_elic** out)
{
    return engine_new(Family::ELIC_united_R2D, N, M, slice_ch, n_slices, 3, 0, 0, out);
}

int rgbd_elic_create_stf(int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, rgbd_elic** out)
{
    if (M != 384) return RGBD_EINVAL;  // embed_dim 48 * 8 (models/stf_united.py:640)
    return engine_new(Family::STF_united, N, M, slice_ch, n_slices, 3, 0, 0, out);
}

int rgbd_elic_create_single(int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, int32_t in_ch, rgbd_elic** out)
{
    if (in_ch < 1 || in_ch > 16) return RGBD_EINVAL;
    return engine_new(Family::ELIC, N, M, slice_ch, n_slices, in_ch, 0, 0, out);
}

int rgbd_elic_create_stf_single(int32_t in_ch, rgbd_elic** out)
{
    if (in_ch < 1 || in_ch > 16) return RGBD_EINVAL;
    int32_t slices[rgbd_elic::kStfSlices];
    for (int32_t& c : slices) c = rgbd_elic::kStfSliceCh;
    return engine_new(Family::STF, 192, rgbd_elic::kStfSlices * rgbd_elic::kStfSliceCh, slices, rgbd_elic::kStfSlices, in_ch, 0, 0,
                      out);  // stf.py:431,418
}

// Cheng2020AnchorwithCheckerboard (models/Cheng2020withCKBD.py:46-50): M = N, one slice of N channels
int rgbd_elic_create_ckbd(int32_t N, int32_t in_ch, rgbd_elic** out)
{
    if ((N != 128 && N != 192) || (in_ch != 3 && in_ch != 1)) return RGBD_EINVAL;
    const int32_t slice = N;
    return engine_new(Family::Cheng2020_ckbd, N, N, &slice, 1, in_ch, 0, 0, out);
}

// MLICPlusPlus (models/mlicpp.py:15-75): slice_num slices of M / slice_num channels.  LocalContext's kernel and the head counts
// slice_ch * i / 32 of the inter contexts are built for 32-channel slices; the widest parameter network reads 2M + 10 * 32
// channels, which launch_pixel_mlp4 takes up to 960.  Everything is checked before anything is allocated.
int rgbd_elic_create_mlic(int32_t N, int32_t M, int32_t slice_num, int32_t in_ch, rgbd_elic** out)
{
    if (!out || slice_num < 2 || slice_num > 10 || N < 16 || N > 512 || N % 16 || M != slice_num * MLIC_SLOT_CH || in_ch < 1 || in_ch > 16)
        return RGBD_EINVAL;
    int32_t slices[10];
    for (int i = 0; i < slice_num; ++i) slices[i] = MLIC_SLOT_CH;
    return engine_new(Family::MLIC, N, M, slices, slice_num, in_ch, 0, 0, out);
}

// The latent codec of ELIC_master (models/elic_master.py:67-98): g_a takes cat(fv, fv_bar) = 2 * 64 channels (:67, 113), g_s returns N
// (:68).  sp1..sp3 are Spatial_aligner() with the default 192 channels (synthesis.py:94-96), so N is 192, as for family 13.
int rgbd_master_latent_create(int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, rgbd_elic** out)
{
    if (!out || N != 192 || M < 16 || M > 1024) return RGBD_EINVAL;
    return engine_new(Family::ELIC_master_latent, N, M, slice_ch, n_slices, 128, N, 0, out);
}

// Spatial_aligner alone (modules/transform/spatialAligner.py:341-390): embed_dim 96, 3 heads, 4x4 windows
int rgbd_aligner_create(int32_t in_ch, int32_t out_ch, rgbd_elic** out)
{
    if (!out || in_ch < 1 || in_ch > 1024 || out_ch < 1 || out_ch > 1024) return RGBD_EINVAL;
    return module_new(Family::Spatial_aligner, in_ch, out_ch, 0, out);
}

// SynthesisTransformPlus alone (modules/transform/synthesis.py:74-110).  Its sp1..sp3 are Spatial_aligner() with the default
// 192 channels whatever N is (:94-96), so N is 192; out_ch is the `ch` of the last transposed convolution
int rgbd_synthesis_plus_create(int32_t N, int32_t M, int32_t out_ch, rgbd_elic** out)
{
    if (!out || N != 192 || M < 16 || M > 1024 || M % 16 || out_ch < 1 || out_ch > 1024) return RGBD_EINVAL;
    const int32_t slice = M;
    return engine_new(Family::SynthesisTransformPlus, N, M, &slice, 1, M, out_ch, 0, out);
}

// The attention contexts of MLIC++ alone (modules/transform/context.py)
int rgbd_local_context_create(int32_t dim, rgbd_elic** out)
{
    if (!out || dim != 32) return RGBD_EINVAL;  // window 5, 2 heads of 16: the one form MLIC++ builds (context_attn.hip)
    return module_new(Family::LocalContext, dim, 2 * dim, 2, out);
}

int rgbd_linear_inter_create(int32_t dim, int32_t out_dim, int32_t heads, rgbd_elic** out)
{
    if (!out || heads < 1 || dim < 1 || dim > 1024 || dim % heads || (dim / heads != 16 && dim / heads != 32) || out_dim < 32 ||
        out_dim > 1024 || out_dim % 32)
        return RGBD_EINVAL;
    return module_new(Family::LinearGlobalInterContext, dim, out_dim, heads, out);
}

int rgbd_linear_intra_create(int32_t dim, int32_t heads, rgbd_elic** out)
{
    if (!out || heads < 1 || dim < 1 || dim > 1024 || dim % heads || (dim / heads != 16 && dim / heads != 32)) return RGBD_EINVAL;
    return module_new(Family::LinearGlobalIntraContext, dim, 2 * dim, heads, out);
}

// The per-slice networks of MLIC++ alone.  EntropyParametersMLIC (modules/transform/entropy.py:31-53): what launch_pixel_mlp4 takes
int rgbd_entropy_params_mlic_create(int32_t in_dim, int32_t out_dim, rgbd_elic** out)
{
    if (!out || in_dim < 16 || in_dim > 960 || in_dim % 16 || out_dim < 16 || out_dim > 128 || out_dim % 16) return RGBD_EINVAL;
    return module_new(Family::EntropyParametersMLIC, in_dim, out_dim, 0, out);
}

// ChannelContext (modules/transform/context.py:140-160): in_dim -> 192 -> 128 -> 4 out_dim
int rgbd_channel_context_create(int32_t in_dim, int32_t out_dim, rgbd_elic** out)
{
    if (!out || in_dim < 1 || in_dim > 1024 || out_dim < 1 || out_dim > 256) return RGBD_EINVAL;
    return module_new(Family::ChannelContext, in_dim, 4 * out_dim, 0, out);
}

// LatentResidualPrediction (modules/transform/LRP.py:9-26): widths in - d / 4, in - d / 2, in - 3 d / 4, out with d = |out - in|
// in integer division, all of which must be positive
int rgbd_lrp_create(int32_t in_dim, int32_t out_dim, rgbd_elic** out)
{
    if (!out || in_dim < 1 || in_dim > 1024 || out_dim < 1 || out_dim > 1024) return RGBD_EINVAL;
    const int d = std::abs(out_dim - in_dim);
    if (in_dim - d * 3 / 4 < 1) return RGBD_EINVAL;
    return module_new(Family::LatentResidualPrediction, in_dim, out_dim, 0, out);
}

int rgbd_elic_clone_shared(const rgbd_elic* src, rgbd_elic** out)
{
    if (!src || !out || !src->finalized) return RGBD_EINVAL;
    rgbd_elic* m = engine_make(src->family, src->N, src->M, src->slice_ch.data(), (int32_t)src->slice_ch.size(), src->in_ch,
                               src->out_ch, src->ctx_heads);
    m->refnum = src->refnum;  // (what the shared weights were packed for)
    m->mlp_fused = src->mlp_fused;
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
    return RGBD_OK;
}

// ---- the single-modal codecs ---------------------------------------------------------------------------------------
int rgbd_elic_compress_single(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, int32_t per_image_streams,
                              void* stream)
{
    if (const int r = check_ready(m)) return r;
    if (!m->single() || !x_dev || !hw64(B, H, W) || !z_grid_ok(m, H / 64, W / 64)) return RGBD_EINVAL;
    if (m->family == Family::ELIC_master_latent && !master_ok(m, B, H, W)) return RGBD_EINVAL;
    const int per_image = (per_image_streams || B == 1) ? 1 : 0;
    return run_call(m, stream, call_key("c1|%d|%d|%d|%d", B, H, W, per_image), kCompressTail,
                    [&]() { return m->run_compress(1, {x_dev}, B, H, W, per_image); });
}

int rgbd_elic_forward_single(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, float* xhat_dev, float* lik_y,
                             float* lik_z, void* stream)
{
    if (const int r = check_ready(m)) return r;
    if (!m->single() || !x_dev || !xhat_dev || !lik_y || !lik_z || !hw64(B, H, W) || !z_grid_ok(m, H / 64, W / 64)) return RGBD_EINVAL;
    if (m->family == Family::ELIC_master_latent) return RGBD_EINVAL;  // (its g_s needs guides: rgbd_master_latent_forward)
    return run_call(m, stream, call_key("f1|%d|%d|%d", B, H, W), kForwardTail,
                    [&]() { return m->run_forward(1, {x_dev}, B, H, W, {xhat_dev}, {lik_y}, {lik_z}); });
}

int rgbd_elic_decompress_single(rgbd_elic* m, const uint8_t* const* y, const int64_t* y_len, int32_t n_y,
                                const uint8_t* const* z, const int64_t* z_len, int32_t B, int32_t zh, int32_t zw,
                                float* x_dev, void* stream)
{
    if (const int r = check_ready(m)) return r;
    if (!m->single() || !y || !y_len || !z || !z_len || !x_dev || B <= 0 || zh <= 0 || zw <= 0 || !one_or_b(n_y, B) || !z_grid_ok(m, zh, zw))
        return RGBD_EINVAL;
    if (m->family == Family::ELIC_master_latent) return RGBD_EINVAL;  // (its g_s needs guides: rgbd_master_latent_decompress)
    return run_call(m, stream, call_key("d1|%d|%d|%d|%d", B, zh, zw, n_y), kDecompressTail,
                    [&]() { return m->run_decompress(1, &y, &y_len, n_y, &z, &z_len, B, zh * 4, zw * 4, {x_dev}); });
}

// return_mid (models/elic.py:159-170, 318-329): the two calls above plus up1..up3; call shapes of their own in the graph cache
// (their bodies hold three more copies)
int rgbd_elic_forward_single_mid(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, float* xhat_dev, float* lik_y,
                                 float* lik_z, float* up1, float* up2, float* up3, void* stream)
{
    if (const int r = check_ready(m)) return r;
    if (m->family != Family::ELIC || !x_dev || !xhat_dev || !lik_y || !lik_z || !up1 || !up2 || !up3 || !hw64(B, H, W)) return RGBD_EINVAL;
    const rgbd_elic::Mid3 up = {up1, up2, up3};
    return run_call(m, stream, call_key("f1m|%d|%d|%d", B, H, W), kForwardTail,
                    [&]() { return m->run_forward(1, {x_dev}, B, H, W, {xhat_dev}, {lik_y}, {lik_z}, &up); });
}

int rgbd_elic_decompress_single_mid(rgbd_elic* m, const uint8_t* const* y, const int64_t* y_len, int32_t n_y,
                                    const uint8_t* const* z, const int64_t* z_len, int32_t B, int32_t zh, int32_t zw,
                                    float* x_dev, float* up1, float* up2, float* up3, void* stream)
{
    if (const int r = check_ready(m)) return r;
    if (m->family != Family::ELIC || !y || !y_len || !z || !z_len || !x_dev || !up1 || !up2 || !up3 || B <= 0 || zh <= 0 || zw <= 0 ||
        !one_or_b(n_y, B))
        return RGBD_EINVAL;
    const rgbd_elic::Mid3 up = {up1, up2, up3};
    return run_call(m, stream, call_key("d1m|%d|%d|%d|%d", B, zh, zw, n_y), kDecompressTail, [&]() {
        return m->run_decompress(1, &y, &y_len, n_y, &z, &z_len, B, zh * 4, zw * 4, {x_dev}, nullptr, &up);
    });
}

// The latent codec of ELIC_master: the two calls that run the guided g_s (compress is rgbd_elic_compress_single).  Call shapes of
// their own in the graph cache.
int rgbd_master_latent_forward(rgbd_elic* m, const float* f_dev, const float* up1_dev, const float* up2_dev, const float* up3_dev,
                               int32_t B, int32_t H, int32_t W, float* fhat_dev, float* lik_y, float* lik_z, void* stream)
{
    if (const int r = check_ready(m)) return r;
    if (!f_dev || !up1_dev || !up2_dev || !up3_dev || !fhat_dev || !lik_y || !lik_z || !hw64(B, H, W) || !master_ok(m, B, H, W))
        return RGBD_EINVAL;
    const rgbd_elic::Guide3 g = {up1_dev, up2_dev, up3_dev};
    return run_call(m, stream, call_key("fm|%d|%d|%d", B, H, W), kForwardTail,
                    [&]() { return m->run_forward(1, {f_dev}, B, H, W, {fhat_dev}, {lik_y}, {lik_z}, nullptr, &g); });
}

int rgbd_master_latent_decompress(rgbd_elic* m, const uint8_t* const* y, const int64_t* y_len, int32_t n_y, const uint8_t* const* z,
                                  const int64_t* z_len, int32_t B, int32_t zh, int32_t zw, const float* up1_dev, const float* up2_dev,
                                  const float* up3_dev, float* fhat_dev, void* stream)
{
    if (const int r = check_ready(m)) return r;
    if (!y || !y_len || !z || !z_len || !up1_dev || !up2_dev || !up3_dev || !fhat_dev || B <= 0 || zh <= 0 || zw <= 0 ||
        !one_or_b(n_y, B) || !master_ok(m, B, (int64_t)zh * 64, (int64_t)zw * 64))
        return RGBD_EINVAL;
    const rgbd_elic::Guide3 g = {up1_dev, up2_dev, up3_dev};
    return run_call(m, stream, call_key("dm|%d|%d|%d|%d", B, zh, zw, n_y), kDecompressTail, [&]() {
        return m->run_decompress(1, &y, &y_len, n_y, &z, &z_len, B, zh * 4, zw * 4, {fhat_dev}, nullptr, nullptr, &g);
    });
}

// ---- the modules alone ---------------------------------------------------------------------------------------------
int rgbd_aligner_forward(rgbd_elic* m, const float* x_dev, const float* guided_dev, int32_t B, int32_t H, int32_t W,
                         float* out_dev, void* stream)
{
    if (const int r = module_ready(m, Family::Spatial_aligner)) return r;
    if (!x_dev || !guided_dev || !out_dev || B <= 0 || H <= 0 || W <= 0 || H % 8 || W % 8) return RGBD_EINVAL;
    return run_call(m, stream, call_key("al|%d|%d|%d", B, H, W), kForwardTail,
                    [&]() { return m->run_aligner(x_dev, guided_dev, B, H, W, out_dev); });
}

int rgbd_synthesis_plus_forward(rgbd_elic* m, const float* yhat_dev, const float* up1_dev, const float* up2_dev,
                                const float* up3_dev, int32_t B, int32_t h, int32_t w, float* out_dev, void* stream)
{
    if (const int r = module_ready(m, Family::SynthesisTransformPlus)) return r;
    // the aligner behind up1 needs multiples of 8 at 2h x 2w; the output has B * out_ch * 256 h w elements
    if (!yhat_dev || !up1_dev || !up2_dev || !up3_dev || !out_dev || B <= 0 || h <= 0 || w <= 0 || h % 4 || w % 4 ||
        (int64_t)B * std::max(m->out_ch, m->N) * 256 * h * w > 0x7fffffff)
        return RGBD_EINVAL;
    const float* const up[3] = {up1_dev, up2_dev, up3_dev};
    return run_call(m, stream, call_key("sp|%d|%d|%d|%d", B, h, w, m->plus_guides ? 1 : 0), kForwardTail,
                    [&]() { return m->run_synthesis_plus(yhat_dev, up, B, h, w, out_dev); });
}

// A timing aid (tools/synplus_probe.py): 0 = the walk of a SynthesisTransformPlus handle without its three aligners (what
// SynthesisTransformEX computes from the same weights), 1 = the module.  A call shape of its own in the graph cache.
int rgbd_debug_synthesis_plus_guides(rgbd_elic* m, int32_t on)
{
    if (!m || m->family != Family::SynthesisTransformPlus) return RGBD_EINVAL;
    if (m->body_mode) return RGBD_ESTATE;  // a call of this engine is running
    m->plus_guides = on != 0;
    return RGBD_OK;
}

static int context_forward(rgbd_elic* m, Family f, const float* x1_dev, const float* x2_dev, int32_t B, int32_t H, int32_t W,
                           float* out_dev, void* stream)
{
    const bool intra = f == Family::LinearGlobalIntraContext;  // two inputs, the columns in pairs
    if (const int r = module_ready(m, f)) return r;
    if (!x1_dev || (intra && !x2_dev) || !out_dev || B <= 0 || H <= 0 || W <= 0 || (intra && (W & 1)) || (int64_t)B * H * W > 0x7fffffff)
        return RGBD_EINVAL;
    return run_call(m, stream, call_key("cx%d|%d|%d|%d", (int)f, B, H, W), kForwardTail,
                    [&]() { return m->run_context(x1_dev, x2_dev, B, H, W, out_dev); });
}

int rgbd_local_context_forward(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, float* out_dev, void* stream)
{
    return context_forward(m, Family::LocalContext, x_dev, nullptr, B, H, W, out_dev, stream);
}

int rgbd_linear_inter_forward(rgbd_elic* m, const float* x1_dev, int32_t B, int32_t H, int32_t W, float* out_dev, void* stream)
{
    return context_forward(m, Family::LinearGlobalInterContext, x1_dev, nullptr, B, H, W, out_dev, stream);
}

int rgbd_linear_intra_forward(rgbd_elic* m, const float* x1_dev, const float* x2_dev, int32_t B, int32_t H, int32_t W,
                              float* out_dev, void* stream)
{
    return context_forward(m, Family::LinearGlobalIntraContext, x1_dev, x2_dev, B, H, W, out_dev, stream);
}

int rgbd_entropy_params_mlic_forward(rgbd_elic* m, const float* const* seg_dev, const int32_t* seg_channels, int32_t n_seg, int32_t B,
                                     int32_t H, int32_t W, int32_t parity, float* out_dev, void* stream)
{
    if (const int r = module_ready(m, Family::EntropyParametersMLIC)) return r;
    if (!seg_dev || !seg_channels || n_seg < 1 || n_seg > PIXEL_MLP_MAX_SEGS || !out_dev || B <= 0 || H <= 0 || W <= 0 ||
        (int64_t)B * H * W * m->in_ch > 0x7fffffff || parity < -1 || parity > 1 || (parity >= 0 && (W & 1)))
        return RGBD_EINVAL;
    int sum = 0;
    std::string key = call_key("ep|%d|%d|%d|%d|%d", B, H, W, parity, m->mlp_fused ? 1 : 0);
    for (int i = 0; i < n_seg; ++i) {
        if (!seg_dev[i] || seg_channels[i] < 16 || seg_channels[i] % 16 || seg_channels[i] > m->in_ch - sum) return RGBD_EINVAL;
        sum += seg_channels[i];
        key += "|" + std::to_string(seg_channels[i]);
    }
    if (sum != m->in_ch) return RGBD_EINVAL;
    return run_call(m, stream, key, kForwardTail,
                    [&]() { return m->run_slice_net(seg_dev, seg_channels, n_seg, parity, B, H, W, out_dev); });
}

// 1 (default): the four layers as one launch_pixel_mlp4; 0: as four conv() launches (the yardstick and the probe's A/B).  Like
// the other switches it drops the cached graphs; refused with RGBD_ESTATE inside a running call of the engine.
int rgbd_entropy_params_mlic_set_fused(rgbd_elic* m, int32_t on)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);
    if (!m || m->family != Family::EntropyParametersMLIC || on < 0 || on > 1) return RGBD_EINVAL;
    if (m->body_mode) return RGBD_ESTATE;
    if (m->mlp_fused != (on != 0)) m->graphs_invalidate();
    m->mlp_fused = on != 0;
    return RGBD_OK;
}

// ChannelContext and LatentResidualPrediction: 3x3 layers.  Maps of one row or one column are refused here, before any launch
// (a 1 x 5 map through the MFMA 3x3 kernel once never returned, cause not found)
static int conv3_stack_forward(rgbd_elic* m, Family f, const float* x_dev, int32_t B, int32_t H, int32_t W, float* out_dev, void* stream)
{
    if (const int r = module_ready(m, f)) return r;
    if (!x_dev || !out_dev || B <= 0 || H < 2 || W < 2 || (int64_t)B * H * W * std::max(m->in_ch, m->out_ch) > 0x7fffffff) return RGBD_EINVAL;
    const float* const seg[1] = {x_dev};
    const int c[1] = {m->in_ch};
    return run_call(m, stream, call_key("sn%d|%d|%d|%d", (int)f, B, H, W), kForwardTail,
                    [&]() { return m->run_slice_net(seg, c, 1, -1, B, H, W, out_dev); });
}

int rgbd_channel_context_forward(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, float* out_dev, void* stream)
{
    return conv3_stack_forward(m, Family::ChannelContext, x_dev, B, H, W, out_dev, stream);
}

int rgbd_lrp_forward(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, float* out_dev, void* stream)
{
    return conv3_stack_forward(m, Family::LatentResidualPrediction, x_dev, B, H, W, out_dev, stream);
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

// Classify, then pack, in map order: tensor_kind says what a host tensor is, one Packer method per kind packs it into a fresh
// generation, swapped in at the end: a failure leaves the engine as it was, and the old generation lives on while a clone points into it.
int rgbd_elic_finalize(rgbd_elic* m)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);  // frees / synchronous copies: not while a stream captures
    if (!m) return RGBD_EINVAL;
    // a shared-weight clone has no host tensors of its own: re-finalising it would only drop the weights it borrows
    if (m->is_clone && m->raw.empty()) return RGBD_ESTATE;
    auto gen = std::make_shared<DevGen>();
    Packer p{m, gen.get()};
    for (const auto& kv : m->raw) {
        const std::string& name = kv.first;
        const HostTensor& t = kv.second;
        int r = RGBD_OK;
        switch (tensor_kind(m->family, name, t.shape.data(), (int)t.shape.size())) {
        case RGBD_KIND_RECOVERY_DECONV: r = p.pack_recovery_deconv(name, t); break;
        case RGBD_KIND_CONTEXT_DENSE: r = p.pack_context_dense(name, t); break;
        case RGBD_KIND_CONV: r = p.pack_conv_layer(name, t, false); break;
        case RGBD_KIND_CONV_TRANSPOSED: r = p.pack_conv_layer(name, t, true); break;
        case RGBD_KIND_GDN_GAMMA: r = p.pack_gdn_gamma(name, t); break;
        case RGBD_KIND_LINEAR: r = p.pack_linear(name, t); break;
        case RGBD_KIND_ARRAY: r = p.pack_array(name, t); break;
        case RGBD_KIND_QUANTILES: r = p.pack_quantiles(name, t); break;
        case RGBD_KIND_PIXEL_MLP: r = p.pack_pixel_mlp(name, t); break;
        default: break;  // RGBD_KIND_IGNORED: biases, betas, bottleneck matrices (read by the packer of their weight), buffers
        }
        if (r) return r;
    }
    m->convs.swap(p.convs);
    m->dense.swap(p.dense);
    m->gen_w = gen;
    m->graphs_invalidate();
    m->finalized = true;
    return RGBD_OK;
}

int rgbd_debug_tensor_kind(int32_t family, const char* name, const int64_t* shape, int32_t ndim)
{
    if (!family_ok(family) || !name || !shape || ndim < 1 || ndim > 4) return RGBD_EINVAL;
    for (int i = 0; i < ndim; ++i)
        if (shape[i] <= 0) return RGBD_EINVAL;
    return tensor_kind((Family)family, name, shape, ndim);
}

// ---- the two-modality codecs -----------------------------------------------------------------------------------------
int rgbd_elic_compress(rgbd_elic* m, const float* rgb_dev, const float* depth_dev, int32_t B, int32_t H, int32_t W,
                       int32_t per_image_streams, void* stream)
{
    if (const int r = check_ready(m)) return r;
    if (!rgb_dev || !depth_dev || !hw64(B, H, W)) return RGBD_EINVAL;
    const int per_image = (per_image_streams || B == 1) ? 1 : 0;
    return run_call(m, stream, call_key("c|%d|%d|%d|%d", B, H, W, per_image), kCompressTail,
                    [&]() { return m->run_compress(2, {rgb_dev, depth_dev}, B, H, W, per_image); });
}

int rgbd_elic_forward(rgbd_elic* m, const float* rgb_dev, const float* depth_dev, int32_t B, int32_t H, int32_t W,
                      float* xr_dev, float* xd_dev, float* lik_y_rgb, float* lik_y_depth, float* lik_z_rgb,
                      float* lik_z_depth, void* stream)
{
    if (const int r = check_ready(m)) return r;
    if (!rgb_dev || !depth_dev || !xr_dev || !xd_dev || !lik_y_rgb || !lik_y_depth || !lik_z_rgb || !lik_z_depth || !hw64(B, H, W))
        return RGBD_EINVAL;
    return run_call(m, stream, call_key("f|%d|%d|%d", B, H, W), kForwardTail, [&]() {
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
    if (const int r = check_ready(m)) return r;
    if (!y_rgb || !y_depth || !z_rgb || !z_depth || !xr_dev || !xd_dev || B <= 0 || zh <= 0 || zw <= 0 || !one_or_b(n_y, B))
        return RGBD_EINVAL;
    const uint8_t* const* ys[2] = {y_rgb, y_depth};
    const int64_t* yl[2] = {y_rgb_len, y_depth_len};
    const uint8_t* const* zs[2] = {z_rgb, z_depth};
    const int64_t* zl[2] = {z_rgb_len, z_depth_len};
    return run_call(m, stream, call_key("d|%d|%d|%d|%d", B, zh, zw, n_y), kDecompressTail,
                    [&]() { return m->run_decompress(2, ys, yl, n_y, zs, zl, B, zh * 4, zw * 4, {xr_dev, xd_dev}); });
}

// The Bi-CEE stage alone (rgbd_elic::Latents): latents and hyper tensors come from the caller, [B, ., h, w] on the latent grid
int rgbd_elic_compress_united(rgbd_elic* m, const float* y_rgb_dev, const float* hyper_rgb_dev, const float* y_depth_dev,
                              const float* hyper_depth_dev, int32_t B, int32_t h, int32_t w, int32_t per_image_streams,
                              void* stream)
{
    if (const int r = check_ready(m)) return r;
    if (!y_rgb_dev || !hyper_rgb_dev || !y_depth_dev || !hyper_depth_dev || B <= 0 || h <= 0 || w <= 0 || (w & 1))
        return RGBD_EINVAL;
    const int per_image = (per_image_streams || B == 1) ? 1 : 0;
    rgbd_elic::Latents lat = {{y_rgb_dev, y_depth_dev}, {hyper_rgb_dev, hyper_depth_dev}, {nullptr, nullptr}};
    return run_call(m, stream, call_key("cu|%d|%d|%d|%d", B, h, w, per_image), kCompressTail,
                    [&]() { return m->run_compress(2, {}, B, h * 16, w * 16, per_image, &lat); });
}

int rgbd_elic_decompress_united(rgbd_elic* m, const uint8_t* const* y_rgb, const int64_t* y_rgb_len, int32_t n_y,
                                const uint8_t* const* y_depth, const int64_t* y_depth_len, const float* hyper_rgb_dev,
                                const float* hyper_depth_dev, int32_t B, int32_t h, int32_t w, float* yhat_rgb_dev,
                                float* yhat_depth_dev, void* stream)
{
    if (const int r = check_ready(m)) return r;
    if (!y_rgb || !y_depth || !hyper_rgb_dev || !hyper_depth_dev || !yhat_rgb_dev || !yhat_depth_dev || B <= 0 || h <= 0 ||
        w <= 0 || (w & 1) || !one_or_b(n_y, B))
        return RGBD_EINVAL;
    const uint8_t* const* ys[2] = {y_rgb, y_depth};
    const int64_t* yl[2] = {y_rgb_len, y_depth_len};
    const uint8_t* const* zs[2] = {nullptr, nullptr};
    const int64_t* zl[2] = {nullptr, nullptr};
    rgbd_elic::Latents lat = {{nullptr, nullptr}, {hyper_rgb_dev, hyper_depth_dev}, {yhat_rgb_dev, yhat_depth_dev}};
    return run_call(m, stream, call_key("du|%d|%d|%d|%d", B, h, w, n_y), kDecompressTail,
                    [&]() { return m->run_decompress(2, ys, yl, n_y, zs, zl, B, h, w, {}, &lat); });
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
    m->profile = on != 0 && on != 3;
    m->profile_keys = on == 2;
    m->profile_phases = on == 3;  // (phases are bracketed in mlic_engine.hip only: another family records nothing)
    m->ev_used = 0;
    m->prof_flops = m->prof_flops_exec = m->prof_ms = 0.0;
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

// The y streams' format: 0 = the reference's (default), 1 = wide rANS with `lanes` interleaved states (rans_wide.hip).  Like the
// other switches it takes the capture lock and drops the cached graphs (the workspace layout and the launch list change); inside
// a running call of the engine it is refused with RGBD_ESTATE.
int rgbd_elic_set_coder(rgbd_elic* m, int32_t format, int32_t lanes)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);
    if (!m || format < 0 || format > 1) return RGBD_EINVAL;
    if (format == 1 && wide_lanes_log2(lanes) < 0) return RGBD_EINVAL;
    // the checkerboard slice loop of ELIC_united and ELIC is the wide coder's producer; the other families keep the reference
    // format and say so here, before anything is launched
    if (format == 1 && m->family != Family::ELIC_united && m->family != Family::ELIC) return RGBD_EINVAL;
    if (m->body_mode || m->dec_err_pending) return RGBD_ESTATE;  // a call of this engine is running
    const int want = format ? lanes : 0;
    if (m->coder_lanes != want) m->graphs_invalidate();
    m->coder_lanes = want;
    return RGBD_OK;
}

int rgbd_elic_set_forced_symbols(rgbd_elic* m, int32_t modality, const int32_t* y_sym, int64_t n_y, const int32_t* z_sym, int64_t n_z)
{
    std::unique_lock<std::shared_mutex> cap_lk(g_capture_mu);
    if (!m || modality < 0 || modality > 1 || n_y < 0 || n_z < 0 || (n_y && !y_sym) || (n_z && !z_sym)) return RGBD_EINVAL;
    // (the two-modality codecs, and modality 0 of the checkerboard Cheng2020 model, of MLIC++ and of ELIC_master_latent)
    if (m->single() && ((m->family != Family::Cheng2020_ckbd && m->family != Family::MLIC && m->family != Family::ELIC_master_latent) || modality != 0))
        return RGBD_EINVAL;
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
