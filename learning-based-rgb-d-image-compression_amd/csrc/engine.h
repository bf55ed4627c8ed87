// Host runtime of the gfx950 codec engine: the declaration.  The process-wide switches, the weight packers, the workspace
// arena, the family table and `struct rgbd_elic` -- its data, the descriptor types and tables of the families, accessors of a
// line or two, and a prototype for every other member: the methods that plan and issue HIP kernel launches on one stream.
// One source file per concern defines them:
//   engine_pack.hip   weight packing (pack_conv, pack_subpix, pack_kpack, ...)
//   engine_graph.hip  HangWatch, the stream, the per-call-shape HIP-graph cache, waits, pinned staging, workspace ends, profiler events
//   engine_conv.hip   the conv planner (tiles, split-K, reference arithmetic), issue, fusion decisions, SE gates
//   engine_elic.hip   the blocks of nm modalities, the ELIC-type transforms and the checkerboard slice loop
//   engine_swin.hip   Swin blocks, Spatial_aligner, the MLIC++ contexts and per-slice networks, the STF transforms and their slice loop
//   engine_ckbd.hip   the checkerboard Cheng2020 family
//   mlic_engine.hip   MLIC++: its transforms and the ten-slice loop over the contexts and per-slice networks of engine_swin.hip
//   engine.hip        the call paths (compress / decompress / forward: one per direction for one or two modalities; a family
//                     enters them through the four `*_family` hooks)
// engine_abi.hip and hooks_abi.hip are the C ABI (include/rgbd_amd.h): the engine's entry points, and the operator hooks and
// debug switches.  What stays defined here is `inline` (one instance for all of those translation units): the switches, which
// hooks_abi.hip writes, the templates, and the accessors.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include <atomic>
#include <condition_variable>  // (HangWatch's members; what its body needs is included by engine_graph.hip)
#include <thread>
#include <unistd.h>

#include "../../include/rgbd_amd.h"
#include "common.h"
#include "conv_args.h"
#include "engine_internal.h"


// (process-wide switches and the helpers below, inside a namespace of their own, so that the symbols they become cannot collide
// with a host application's globals; the switches are `inline`: one instance for every translation unit that includes this)
namespace rgbd_rt {


// ------------------------------------------------------------------------------------------------
// packed layers
// ------------------------------------------------------------------------------------------------
struct HostTensor {
    std::vector<float> v;
    std::vector<int64_t> shape;
};

// perm_in / perm_out: store the input / output channels at their permuted positions (rgbd_cperm)
int pack_conv(const HostTensor& w, const HostTensor* b, bool transposed, PackedConv* pc, DevGen* gen = nullptr, int perm_in = 0,
              int perm_out = 0);

// SE_Block's fc.2.weight ([C][hidden]) as launch_se_fc reads it: transposed to [hidden][C], so that the gate kernel's
// consecutive lanes read consecutive addresses.  w1t must not alias w1.
void se_pack_fc2(const float* w1, size_t C, size_t Hd, float* w1t);

// ConvTranspose2d(cin -> cout <= 4, k = 5, stride 2, pad 2, output_padding 1) as ONE stride-1 3x3 conv over the input grid
// with 16 output channels = 4 output phases x 4: the per-phase form pads the couts to 16 for each of its 25 taps, this one
// runs 9 taps for all phases together (2.8x fewer MFMAs).  Output phase (ry, rx) at input offset (dy, dx) uses kernel
// element ky = ry + 2 - 2 dy, kx = rx + 2 - 2 dx when that is inside the kernel, else a zero weight; the taps run dy, dx =
// 1, 0, -1, which keeps every phase's real taps in the order make_taps() gives them -- with fma(0, x, acc) == acc the
// value of every output is the same chain as in the per-phase form (tests/test_gpu_conv.py::test_subpixel_deconv).
int pack_subpix(const HostTensor& w, const HostTensor* b, PackedConv* pc, DevGen* gen, int perm_in = 0);

// Conv2d(cin <= 3 -> cout, k 5, stride 2, pad 2) as a 1x1 layer over the packed input of launch_im2col5s2: weight of
// term n = tap * cin + c at packed index (n / 16) * 16 + (n % 4) * 4 + (n % 16) / 4
int pack_kpack(const HostTensor& w, const HostTensor* b, PackedConv* pc, DevGen* gen, int perm_out = 0);


// ---- hang diagnostics (RGBD_DEBUG_DESTROY=1) -----------------------------------------------------------------------------
// A HangWatch around a runtime call that may wait for the device (hipFree = implicit device synchronise): if the call has
// not returned after `secs`, every thread of the process prints its host backtrace (SIGUSR2 handler; the runtime is
// stripped, but the exported entry points -- hipFree, hipGraphLaunch, hsa_signal_wait_*, pthread lock waits -- tell a
// host lock cycle from a wait for a GPU signal), then every engine stream is queried (hipStreamQuery does not block), which
// names the stream that still holds work.  This is how the round-2 "hipFree never returns" report was taken apart.
inline std::mutex g_live_mu;
inline std::map<const void*, hipStream_t> g_live_streams;  // engine -> the stream of its last call
inline const bool g_dbg_destroy = getenv("RGBD_DEBUG_DESTROY") != nullptr;

struct HangWatch {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    HangWatch(const char* what, int secs, bool always = false);
    ~HangWatch();
};

inline int g_cfg_epoch = 0;     // bumped by every debug switch that changes kernel choices: cached HIP graphs of older epochs are not reused
inline int g_force_splitk = 0;  // test hook (rgbd_debug_force_splitk)
inline int g_bench_streams = 1;  // rgbd_debug_bench_streams: rgbd_conv_bench issues every launch on this many streams at once
inline const bool g_kpack = !getenv("RGBD_NO_KPACK");  // A/B switch: first analysis conv over a K-packed input (1x1, K = 80 / 32)
inline int g_subpix = getenv("RGBD_NO_SUBPIX") ? 0 : 1;  // rgbd_debug_force_subpix: sub-pixel form of the last transposed conv
inline int g_fail_captures = 0;  // rgbd_debug_fail_captures: the next n graph captures count as lost (test hook)
inline int g_pair = getenv("RGBD_NO_PAIR") ? 0 : 1;  // rgbd_debug_force_pair: RGB / depth layer pairs as one grouped launch
inline int g_force_ckbd = 0;    // test hook (rgbd_debug_force_ckbd): checkerboard output mode of rgbd_conv2d_nchw / rgbd_conv_bench
inline int g_force_blocked = 0;  // rgbd_debug_force_blocked: rgbd_conv_bench launches the blocked-accumulation kernels (tile tuner)
inline const bool g_ckbd_conv = !getenv("RGBD_NO_CKBD_CONV");  // A/B switch: checkerboard-restricted entropy-parameter convs

// ------------------------------------------------------------------------------------------------
// the model
// ------------------------------------------------------------------------------------------------
// Workspace of one engine instance: a two-ended stack.  `top` is the fill of the ACTIVE end (the low end grows up from the
// base, the high end down from base + cap), `other` the fill of the other one.  Blocks allocate and release stack-style on
// the active end (`mark = top ... top = mark`); the stage loops of the big transforms alternate the ends (flip), so that a
// stage's output and temporaries go to the end that holds nothing live any more -- the input of the previous stage -- and
// the workspace holds two consecutive stages instead of the whole transform (round 4: 6.0 -> 2.9 GiB per c3 instance).
// Addresses are a function of the call shape and of cap; a re-allocation (new cap) drops the cached graphs.
struct Arena {
    unsigned char* base = nullptr;
    size_t cap = 0, top = 0, other = 0, peak = 0;
    bool hi = false;
    bool dry = false;
    void* take(size_t bytes)
    {
        bytes = (bytes + 255) & ~(size_t)255;
        void* p;
        if (dry) p = (void*)(uintptr_t)(0x1000 + top);
        else p = hi ? (void*)(base + cap - top - bytes) : (void*)(base + top);
        top += bytes;
        peak = std::max(peak, top + other);
        return p;
    }
    void reset()
    {
        top = other = 0;
        hi = false;
    }
    // make the other end the active one, emptied down to `floor` (what is below belongs to somebody who is still alive)
    void flip(size_t floor)
    {
        std::swap(top, other);
        hi = !hi;
        top = floor;
    }
};

struct Epi {
    int act = ACT_NONE;
    const Act* res1 = nullptr;
    const Act* mul = nullptr;
    const Act* res2 = nullptr;
    int ckbd = 0;  // ConvArgs::ckbd: compute / store only one checkerboard half of the output
    const Act* dup = nullptr;  // ConvArgs::y2: the output is also written here (same shape, own channel stride)
};


// ------------------------------------------------------------------------------------------------
// conv_transpose2d(k 5, stride 2, pad 2, output_padding 1) + activation in the reference's CPU arithmetic (oneDNN's
// brg_deconv: DESIGN.md 4a; oracle/cpu_arith.c orc_deconv_s2): the taps of an output pixel are accumulated tap by tap over
// all input channels, in chains whose membership depends on the layer shape and on the pixel's column block -- a measured
// recipe per (phase, column), refarith_tables.json kind 3.  Per phase and column class (columns with the same recipe) this
// is ONE GEMM whose K axis is (tap, channel): gathered input rows x gathered weight slabs, the chains as split-K ranges
// whose sums the ordered reducer adds (+ bias, activation), rows scattered to the phase's output positions.
// rec: the recipe's flat integers, 4 * w descriptors {n, n x (ky, kx, fresh)}.  x: NHWC with channel stride pc.cin_pad;
// out: [B][2h][2w][ocs].  Scratch: mark() / take(bytes) / release(mark), stack-style per column class -- the engine's arena
// (ArenaScratch) or device allocations of the stand-alone entry point.  launch = false: sizes only (the engine's dry pass).
struct ArenaScratch {
    Arena& a;
    size_t mark() const { return a.top; }
    float* take(size_t bytes) { return (float*)a.take(bytes); }
    void release(size_t m) { a.top = m; }
};
template <class Scratch>
inline int deconv_s2_ref_run(const PackedConv& pcv, const int* rec, size_t nrec, const float* x, int B, int h, int w, int act,
                             float* out, int ocs, int tile_mode, bool launch, hipStream_t s, Scratch& scratch)
{
    const PackedConv* pc = &pcv;
    // parse: 4 * w descriptors {n, n x (ky, kx, fresh)}
    std::vector<const int*> desc(4 * (size_t)w, nullptr);
    {
        size_t pos = 0;
        for (size_t i = 0; i < desc.size(); ++i) {
            if (pos >= nrec || rec[pos] < 0 || (size_t)rec[pos] > (nrec - pos - 1) / 3) return RGBD_EINVAL;
            desc[i] = rec + pos;
            pos += 1 + 3 * (size_t)rec[pos];
        }
        if (pos != nrec) return RGBD_EINVAL;
    }
    auto same = [](const int* a, const int* b) { return a[0] == b[0] && memcmp(a, b, sizeof(int) * (1 + 3 * (size_t)a[0])) == 0; };
    for (int ph = 0; ph < 4; ++ph) {
        const int py = ph >> 1, px = ph & 1;
        for (int j0 = 0; j0 < w;) {
            const int* d = desc[(size_t)ph * w + j0];
            int j1 = j0 + 1;
            while (j1 < w && same(d, desc[(size_t)ph * w + j1])) ++j1;
            const int jw = j1 - j0, nt = d[0];
            if (nt < 1 || nt > 16) return RGBD_EINVAL;
            int dy[16], dx[16], slab[16], chain[16], nch = 0;  // chain: channels of the GEMM's K axis each fma chain reduces
            for (int t = 0; t < nt; ++t) {
                const int ky = d[1 + 3 * t], kx = d[2 + 3 * t], fresh = d[3 + 3 * t];
                // (a tap of another phase -- (py + 2 - ky) or (px + 2 - kx) odd -- never meets this phase's pixels)
                if (ky < 0 || ky > 4 || kx < 0 || kx > 4 || ((py + ky) & 1) || ((px + kx) & 1) || (fresh != 0 && fresh != 1)) return RGBD_EINVAL;
                dy[t] = (py + 2 - ky) / 2;  // input row of output row 2 ty + py under tap ky: ty + (py + pad - ky) / 2
                dx[t] = (px + 2 - kx) / 2;
                slab[t] = ky * 5 + kx;
                if (fresh || t == 0) chain[nch++] = 0;
                chain[nch - 1] += pc->cin_pad;
            }
            const size_t mark = scratch.mark();
            const size_t npx = (size_t)B * h * jw;
            const int Kp = nt * pc->cin_pad;
            float* col = scratch.take(npx * Kp * sizeof(float));
            float* wsel = scratch.take((size_t)pc->cout_pad * Kp * sizeof(float));
            float* tmp = scratch.take(npx * pc->cout_pad * sizeof(float));
            float* part = nch > 1 ? scratch.take((size_t)nch * npx * pc->cout_pad * sizeof(float)) : nullptr;
            if (launch) {
                if (!col || !wsel || !tmp || (nch > 1 && !part)) return RGBD_ENOMEM;
                int r = launch_gather_taps(x, B, h, w, pc->cin_pad, j0, jw, nt, dy, dx, col, s);
                if (!r) r = launch_gather_wslabs(pc->w, pc->cout_pad, 25, pc->cin_pad, nt, slab, wsel, s);
                if (!r) {
                    PackedConv gemm;  // the 1x1 layer over the gathered columns
                    gemm.w = wsel;
                    gemm.bias = pc->bias;
                    gemm.cin_pad = Kp;
                    gemm.cout_pad = pc->cout_pad;
                    gemm.k = 1;
                    ConvArgs a{};
                    conv_args_geometry(&a, gemm, col, 1, B * h, jw, Kp, tmp, pc->cout_pad, B * h, jw, 1, 0);
                    a.cout_store = pc->cout_pad;
                    a.act = act;
                    a.loaded = tile_mode;
                    a.exact_math = 1;
                    a.splitk = 1;
                    if (nch > 1) {
                        a.partial = part;
                        r = conv_set_split_ranges(&a, chain, nch);
                    }
                    if (!r) r = launch_conv(a, s);
                }
                if (!r) r = launch_scatter_phase(tmp, B, h, jw, pc->cout_pad, j0, py, px, out, 2 * w, ocs, pc->cout_pad, s);
                if (r) return r;
            }
            scratch.release(mark);
            j0 = j1;
        }
    }
    return RGBD_OK;
}

// K blocks of the small-tensor route: block lengths in k = c * K * K + ky * K + kx -> SmallConvArgs::kb / nb (nullptr = one block)
int small_conv_set_kblocks(SmallConvArgs* a, const int* lens, int n, int Kt);

}  // namespace rgbd_rt
using namespace rgbd_rt;

// What an engine handle is: a codec (0-5, 19, 20) or one module alone (6-9, 13, 15-17: no codec calls, no tables, its own forward
// entry point).  DESIGN.md and the history name the families by these numbers, so the numbers stay; 10-12 are reserved for the
// held-back modules of ELIC_master and refused everywhere, and so are 14 and 18, which nothing has claimed
// (tests/test_synplus_kinds_cpu.py and tests/test_mlic_slice_kinds_cpu.py hold them refused): the table has holes, not a
// renumbering.
enum class Family : int {
    ELIC_united = 0,      // RGB + depth (models/elic_united.py)
    ELIC = 1,             // single-modal ELIC (models/elic.py)
    STF_united = 2,       // models/stf_united.py
    ELIC_united_R2D = 3,  // models/elic_united_R2D.py
    STF = 4,              // single-modal STF (models/stf.py)
    Cheng2020_ckbd = 5,   // checkerboard Cheng2020 (models/Cheng2020withCKBD.py)
    Spatial_aligner = 6,  // modules/transform/spatialAligner.py: rgbd_aligner_forward only
    LocalContext = 7,     // the contexts of MLIC++ (modules/transform/context.py): rgbd_local_context_forward /
    LinearGlobalInterContext = 8,  // rgbd_linear_inter_forward /
    LinearGlobalIntraContext = 9,  // rgbd_linear_intra_forward only
    SynthesisTransformPlus = 13,   // modules/transform/synthesis.py:74-110: rgbd_synthesis_plus_forward only
    EntropyParametersMLIC = 15,    // the per-slice networks of MLIC++: modules/transform/entropy.py:31-53, rgbd_entropy_params_mlic_forward /
    ChannelContext = 16,           // modules/transform/context.py:140-160, rgbd_channel_context_forward /
    LatentResidualPrediction = 17, // modules/transform/LRP.py:9-26, rgbd_lrp_forward only
    MLIC = 19,                     // MLIC++ (models/mlicpp.py): the codec over families 7-9 and 15-17
    ELIC_master_latent = 20,       // the latent codec of ELIC_master (models/elic_master.py:115-216, 228-304, 319-378): g_a on 128
                                   // channels, h_a, h_s, the checkerboard slice loop with EntropyParametersEX, the guided g_s
};
constexpr int kFamilies = 21;

struct FamilyRow {
    const char* name;
    int nm;        // modalities of a codec call; 0: a module handle
    bool codec;    // has compress / decompress / forward (check_ready refuses the others)
    bool refnum;   // default arithmetic: the reference's CPU arithmetic, unless RGBD_LEGACY_NUMERICS is set.  The
                   // Swin transforms (channel slices that are not 16-aligned), the checkerboard family and the float-only modules
                   // keep the single-chain arithmetic of rounds 1-4
    int clamp;     // decompress() clamps x_hat to [0, 1] (elic_united.py, stf.py:815; not elic.py:318-325 nor
                   // Cheng2020withCKBD.py:167-174); forward() and the Latents epilogue never clamp
    bool forward_names_z;  // forward() names z and z_hat too: the single-modal paths always did, the two-modality one never
                           // (it names y and y_hat only); kept so that the debug-tensor key sets stay what they were
    bool dense4d;  // finalize keeps `fusion.weight` and the depthwise [C][1][3][3] weights as plain device arrays
};
constexpr FamilyRow kFamilyTable[kFamilies] = {
    //  name                        nm codec  refnum clamp names_z dense4d
    {"ELIC_united",                 2, true,  true,  1, false, false},
    {"ELIC",                        1, true,  true,  0, true,  false},
    {"STF_united",                  2, true,  false, 1, false, false},
    {"ELIC_united_R2D",             2, true,  true,  1, false, false},
    {"STF",                         1, true,  false, 1, true,  false},
    {"Cheng2020_ckbd",              1, true,  false, 0, true,  false},
    {"Spatial_aligner",             0, false, false, 0, false, false},
    {"LocalContext",                0, false, false, 0, false, true},
    {"LinearGlobalInterContext",    0, false, false, 0, false, true},
    {"LinearGlobalIntraContext",    0, false, false, 0, false, true},
    {nullptr,                       0, false, false, 0, false, false},  // 10-12: reserved
    {nullptr,                       0, false, false, 0, false, false},
    {nullptr,                       0, false, false, 0, false, false},
    {"SynthesisTransformPlus",      0, false, false, 0, false, false},
    {nullptr,                       0, false, false, 0, false, false},  // 14: a hole
    {"EntropyParametersMLIC",       0, false, false, 0, false, false},
    {"ChannelContext",              0, false, false, 0, false, false},
    {"LatentResidualPrediction",    0, false, false, 0, false, false},
    {nullptr,                       0, false, false, 0, false, false},  // 18: a hole
    {"MLIC",                        1, true,  false, 0, true,  true},   // (mlicpp.py:406-413: x_hat is not clamped)
    {"ELIC_master_latent",          1, true,  false, 0, true,  false},  // (elic_master.py:378: g_s's output goes on to master_decoder)
};
constexpr bool family_ok(int f) { return f >= 0 && f < kFamilies && kFamilyTable[f].name; }
constexpr const FamilyRow& family_row(Family f) { return kFamilyTable[(int)f]; }

struct rgbd_elic {
    int N = 192, M = 320;
    int tile_mode = 0;  // rgbd_elic_set_tile_mode: 0 latency tiles (isolated launches), 1 throughput tiles (shared chip)
    Family family = Family::ELIC_united;
    const FamilyRow& row() const { return family_row(family); }
    bool single() const { return row().nm == 1; }
    int in_ch = 3;    // image channels of the single-modal codecs (Spatial_aligner: channels of x and guided; contexts: dim;
                      // SynthesisTransformPlus: M; the per-slice networks of MLIC++: in_dim; ELIC_master_latent: channels of f)
    int out_ch = 0;   // module handles: output channels; ELIC_master_latent: channels of f_hat (a codec with out_ch 0 returns in_ch)
    int ctx_heads = 0;  // contexts: num_heads
    // what the call paths (engine.hip) need to know about one versus two modalities; arrays are read at [0, nm)
    struct Modes {
        int nm;
        const char* sfx[2];  // suffix of the debug-tensor names: "y" / "y_r", "y_d"
        const char* eb[2];   // prefix of the entropy bottleneck's tensors
        int img_ch[2];       // image channels
        int out_ch[2];       // channels of x_hat (img_ch, but for ELIC_master_latent: f has 128 channels, f_hat N)
        int clamp;           // FamilyRow::clamp
        bool forward_names_z;  // FamilyRow::forward_names_z
    };
    Modes modes() const
    {
        const FamilyRow& f = row();
        const int oc = out_ch ? out_ch : in_ch;
        if (single()) return {1, {"", ""}, {"", ""}, {in_ch, in_ch}, {oc, oc}, f.clamp, f.forward_names_z};
        return {2, {"_r", "_d"}, {"rgb_", "depth_"}, {3, 1}, {3, 1}, f.clamp, f.forward_names_z};
    }
    std::vector<int> slice_ch;
    std::map<std::string, HostTensor> raw;
    std::map<std::string, PackedConv> convs;
    std::map<std::string, float*> dense;  // SE fc weights, EB medians (device)
    TableSet tables[4];
    float* scale_table = nullptr;
    std::shared_ptr<DevGen> gen_w;      // owner of every pointer in convs / dense
    std::shared_ptr<DevGen> gen_scale;  // owner of scale_table
    bool finalized = false;

    Arena arena;
    hipStream_t s = nullptr;
    int rc = 0;
    std::map<std::string, Act> named;  // intermediates of the last call (live in the arena)

    // last compress() results (host)
    std::vector<std::vector<uint8_t>> streams[2][2];
    // last compress() symbol buffers (device, inside the arena) for debug
    int32_t* dbg_sym = nullptr;
    int32_t* dbg_idx = nullptr;
    int64_t dbg_per_mod = 0;
    // rgbd_elic_set_debug_floats: the encoder also keeps, per symbol and in stream order, the value it rounded (y - mean)
    // and the scale it indexed -- what the parity bookkeeping compares with the reference's floats at a flipped symbol
    bool debug_floats = false;
    // rgbd_elic_set_coder: 0 = the reference's stream format, else the lanes of wide rANS for the y streams (rans_wide.hip)
    int coder_lanes = 0;
    WideSegs y_segs{};          // the parts of the call in stream order, recorded by code_part while compress runs
    int64_t y_seg_next = 0;     // where the next part must start (symbols of one stream)
    bool dec_err_pending = false;  // a wide decompress left its error flag in res_pin's last slot
    int y_state_words() const { return coder_lanes ? coder_lanes + 1 : 2; }  // 64-bit words of decoder state per y stream
    int64_t y_cap_words(int64_t n) const { return rgbd_enc_cap_words(n) + (coder_lanes ? 2 * (coder_lanes - 1) : 0); }
    float* dbg_x = nullptr;
    float* dbg_s = nullptr;

    // rgbd_elic_set_forced_symbols (teacher forcing, parity bookkeeping): the next compress() calls still take every decision
    // from their own floats (symbols / indexes / streams are the GPU's), but what later contexts see is rebuilt from THESE
    // symbols -- z_hat = forced z symbol + median after the z stage, y_hat = forced symbol + mean after every coding part --
    // so that the parts behind a first flip are evaluated under the reference's context (elic_united.py:265-348)
    std::vector<int32_t> force_y[2], force_z[2];

    bool is_clone = false;  // created by rgbd_elic_clone_shared: shares the parent's buffer generations (DevGen)

    // ---- reference arithmetic ----------------------------------------------------------------------
    // refnum: every float operation that feeds a coding decision is performed in the order and with the roundings of the CPU
    // kernels the reference runs on (torch CPU: oneDNN convolutions, Sleef sigmoid, ...): blocked accumulation in the
    // convolutions (conv_mfma_blk.hip), channels stored permuted inside their groups of 16 (rgbd_cperm) so that the MFMA
    // k order is ascending channels.  STF_united keeps the k-ordered single-chain arithmetic of rounds 1-4 (its channel
    // slices are not 16-aligned).  ref_blocks: the reduce blocks of the reference's 1x1 kernels per layer shape, measured on
    // the reference machine (tools/refarith/discover.py -> refarith_tables.json -> rgbd_elic_set_ref_blocks).
    bool refnum = getenv("RGBD_LEGACY_NUMERICS") == nullptr;
    int ref_batch = 1;  // the batch size of the reference call this call stands for (per-image streams: 1)
    int ref_threads = 8;  // CPU threads of the reference run the tables describe (refarith_tables.json "meta"; set_ref_blocks kind 4)
    struct RefTables {
        // kind 0 (1x1 reduce blocks): {0, cin, cout, h, w, batch} -> channels per block
        // kind 1 (small-tensor path, im2col + sgemm): {1, cin, cout, h, w, k * 100 + stride * 10 + pad} -> K-block lengths
        std::map<std::array<int, 6>, std::vector<int>> blocks;
        int misses = 0;
    };
    std::shared_ptr<RefTables> ref_tab = std::make_shared<RefTables>();
    int perm() const { return refnum ? 1 : 0; }
    const std::vector<int>* ref_blocks(int kind, int cin, int cout, int h, int w, int last = -1) const;

    // conv-kernel profiling (bench.py roofline): HIP event pairs around every conv launch on the launch stream
    bool profile = false;
    // rgbd_elic_set_profile(m, 3): event pairs around the PHASES of an MLIC++ call instead of its launches (tools/mlic_probe.py):
    // "phase.transforms", "phase.contexts", "phase.params", "phase.lrp", "phase.coder".  Pairs are never nested (profile_collect
    // names them in recording order), so the launches inside a phase record none of their own: `profile` stays off.
    bool profile_phases = false;
    struct Phase {
        rgbd_elic* m;
        const char* name;
        hipEvent_t e1 = nullptr;
        Phase(rgbd_elic* m_, const char* n) : m(m_), name(n)
        {
            if (m->profile_phases && !m->dry() && !m->rc && !m->prof_begin(&e1)) e1 = nullptr;
        }
        ~Phase()
        {
            if (e1) m->prof_end(e1, name, 0.0, 0.0);
        }
    };
    bool profile_keys = false;  // rgbd_elic_set_profile(m, 2): the recorded layer names carry the launch's shape key (tools/tune_insitu.py)
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    struct EvName {
        std::string first;  // layer name
        double second;      // algorithmic FLOPs of the launch (the reference's layer)
        double exec;        // FLOPs the launch executes (checkerboard-output / half-tap launches: less)
    };
    std::vector<EvName> ev_names;  // per recorded launch
    struct LayerAcc {
        double first = 0.0, second = 0.0, exec = 0.0;  // ms, algorithmic FLOPs, executed FLOPs
    };
    std::map<std::string, LayerAcc> prof_layers;
    std::map<std::string, int> prof_counts;
    double prof_flops = 0.0;   // algorithmic (unpadded) FLOPs of the recorded launches: the reference's layers
    double prof_flops_exec = 0.0;  // ... and what the launches execute of them (round-4 review: a checkerboard-output launch computes
                                   // one half of its layer's outputs, an anchor-input launch half of the taps as well)
    double prof_ms = 0.0;
    int64_t prof_launches = 0;

    // --- small helpers -------------------------------------------------------------------------
    bool dry() const { return arena.dry; }

    // ---- HIP graphs ---------------------------------------------------------------------------------------------
    // The launch sequence of a compress() / decompress() call (~750 dependent kernels for ELIC_united) depends only on
    // the call shape: workspace addresses are a deterministic function of (B, H, W, stream format), weights and tables
    // are fixed.  The second call of a shape therefore captures its "body" -- everything between the upload of the
    // inputs and the fetch of the results -- into a HIP graph, and later calls replay it with one hipGraphLaunch: no
    // per-launch host work (name lookups, tap tables, tile choice, argument marshalling), which is what the 16 host
    // threads of a pooled rank used to burn their cores on.  Anything that would stale a baked pointer or a baked
    // kernel choice drops the graphs: workspace re-allocation, new weights / tables, tile-mode and debug switches.
    struct GraphEntry {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        int seen = 0;                       // completed calls of this shape (the first one runs eagerly)
        int capture_fails = 0;              // failed capture attempts; kMaxCaptureFails of them retire the entry to eager launches
        uint64_t last_use = 0;              // graph_clock at the entry's last call (least-recently-used eviction)
        std::map<std::string, Act> named;   // debug tensors of the body (same workspace addresses on every replay)
        Act out[6];                         // body outputs the epilogue reads (x_hat / y_hat per modality; forward(): + likelihoods)
    };
    std::map<std::string, GraphEntry> graphs;
    static constexpr int kMaxCaptureFails = 3;
    static constexpr size_t kMaxGraphs = 24;  // instantiated graphs kept per engine instance (~750 nodes each)
    uint64_t graph_clock = 0;
    bool capture_failed = false;   // the call in progress lost its capture (body_end / a launch inside the capture failed)
    GraphEntry* cur_ge = nullptr;  // entry of the call in progress (nullptr: graphs off for this call)
    int body_mode = 0;             // 0 eager, 1 capturing, 2 replaying
    const bool use_graphs = getenv("RGBD_NO_GRAPH") == nullptr;
    const bool blocking_wait = getenv("RGBD_SPIN_WAIT") == nullptr;
    hipEvent_t done_ev = nullptr;  // blocking-sync event: the host thread sleeps instead of spinning on the stream
    // The legacy NULL stream cannot be captured: a caller that passes it runs the eager launch path (same results, no
    // graph).  Substituting an engine-owned stream for it was built in round 2 and taken out: with it, host waits inside
    // the runtime stopped returning once a pool had switched the device to blocking sync (DESIGN.md 3.5 and
    // profiles/r03_hang_diagnosis.txt have the analysis).  The switch that re-created that configuration is gone from the
    // product (round 4); throughput users drive their own streams (CodecPool), which do capture.
    int use_stream(void* stream);
    // pinned staging for the per-call uploads (stream bytes, offsets): truly asynchronous copies, no per-call pinning
    int64_t* res_pin = nullptr;  // pinned landing buffer of the per-call result sizes
    static constexpr size_t kResPinBytes = 64 * 1024;
    void* pin = nullptr;
    size_t pin_cap = 0;
    hipEvent_t pin_ev = nullptr;
    bool pin_busy = false;

    void graphs_invalidate();
    GraphEntry* graph_entry(const std::string& key);
    static void drop_entry(GraphEntry& ge);
    // Start of the capturable part of a call.  Returns true when the caller has to run the body code (eagerly, into a
    // capture, or as a sizing pass), false when a cached graph stands in for it.
    bool body_begin();
    int body_end();
    // an error return between body_begin() and body_end() must not leave the stream capturing
    void body_abort();
    // Is this engine's stream recording into a graph right now?  (Its own body, or -- when two users were handed the same
    // HIP stream, e.g. past torch's pool of 32 side streams -- somebody else's.)  The NULL stream never captures.
    bool capturing() const
    {
        if (!s) return false;
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &st) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        return st != hipStreamCaptureStatusNone;
    }
    int wait_stream();
    // pinned staging buffer of at least `bytes`; waits until the previous call's copies out of it have finished
    int pin_take(size_t bytes, void** out);
    int pin_release();
    void fail(int code);
    Act alloc(int n, int h, int w, int c);
    // ---- two-ended workspace (Arena): the stage loop of stages() ----------------------------------------------------
    // A stage reads tensors on one end and puts its output and temporaries on the other, which is emptied first: what it
    // held -- the previous stage's input -- is dead by then.  `cur_hi`: the end the stage's input lives on.  A fusion stage
    // (its inputs ARE its outputs: the concat buffers) only puts its temporaries there.
    struct Ends {
        size_t lo_floor = 0;  // low-end fill at the transform's entry: everything below belongs to the caller
        bool cur_hi = false;
    };
    Ends ends_begin();
    void ends_stage(Ends& e, bool output_moves);
    // back on the low end; the transform's results stay protected on whichever end they are until ends_release()
    void ends_finish(Ends& e);
    void ends_release() { arena.other = 0; }

    static Act view(const Act& a, int c0, int c)
    {
        Act v = a;
        v.p = a.p + c0;
        v.c = c;
        return v;
    }
    const PackedConv* conv_of(const std::string& name);
    // per-row dot-product classes of an SE_Block Linear layer (reference arithmetic; nullptr = every row "main")
    const int* cls_of(const std::string& wname);
    // the SE Linear layers of a reference call on a batch of two vectors take MKL's n = 2 form for every row (se_linear_ref_kernel
    // form 3; measured for batch 2 only: other batch sizes keep the "main" order and make no bit-level claim)
    int se_form() const { return ref_batch == 2 ? 3 : -1; }
    float* dense_of(const std::string& name);

    // --- operators -----------------------------------------------------------------------------
    // A convolution is planned (layer lookup, shapes, ConvArgs) and then issued.  Two plans of the same shape on independent
    // data -- the RGB and the depth branch of a transform stage -- are issued as ONE grouped launch (ConvArgs::groups = 2:
    // twice the workgroups, half the launches; every output keeps its fma chain, so the results are those of the two
    // launches bit for bit: tests/test_gpu_pairs.py).
    struct ConvPlan {
        ConvArgs a{};
        Act y;
        std::string name;
        double flops = 0.0;
        double flops_exec = 0.0;  // (see prof_flops_exec)
        size_t partial_bytes = 0;  // split-K / GELU partial planes of this layer
        bool fused = false;        // launch_conv_fused
        bool ok = false;           // a launch is wanted (not a dry run, no error so far)
    };

    // fuse1x1: name of a 1x1 layer applied to relu(conv(x)) inside the same launch (launch_conv_fused); ep / dst / the
    // returned tensor then describe that second layer's output.  Callers ask fusable() first.
    // lead1x1 / lead_dst (only with fuse1x1): a further 1x1 + ReLU applied to that output inside the same launch -- the
    // leading layer of the block that follows -- written to *lead_dst.
    ConvPlan conv_plan(const std::string& name, const Act& x, int stride, int pad, Epi ep = Epi(), const Act* dst = nullptr,
                       const std::string* fuse1x1 = nullptr, const std::string* lead1x1 = nullptr,
                       const Act* lead_dst = nullptr);

    // The accumulation structure of the reference's CPU kernel for this layer (oracle/cpu_arith.c is the C
    // restatement the GPU results are compared with, bit for bit):
    //   conv, k > 1 (oneDNN jit:avx512_core)      a block per 16 input channels; (S_0 + bias) + S_1 + ...
    //   conv, 1x1   (oneDNN jit_1x1:avx512_core)  the layer shape's reduce blocks (ref_blocks); the first chain starts at the bias
    //   conv_transpose2d, stride 1                a block per 16 input channels; bias last
    // Layers with no decision behind them that have a faster special form keep it (the image-producing sub-pixel layer);
    // stride-2 transposed convs: see deconv_s2_ref().
    void plan_refnum(ConvPlan& cp, const std::string& name, const PackedConv* pc, const PackedConv* pc2, bool subpix, const Act& x,
                     int stride, int OH, int OW);

    // can the two plans share a launch?  Same layer shape, strides and epilogue, operand by operand
    static bool pairable(const ConvPlan& p, const ConvPlan& q);

    // The profiler's event pair around one launch.  prof_begin() records the first event of the pool's next pair and hands
    // back the second (the pool grows by 256 events at a time; false: an event could not be created, the call has failed);
    // prof_end() records that one behind the launch and books the launch: name, algorithmic and executed FLOPs.
    bool prof_begin(hipEvent_t* e1);
    void prof_end(hipEvent_t e1, const std::string& name, double fl, double fx);

    // launch one plan, or two plans as one grouped launch (q != nullptr: the caller has checked pairable())
    void conv_issue(ConvPlan& p, ConvPlan* q = nullptr);

    // first analysis conv (3 / 1 -> N, k 5, stride 2): gather the 25 x C real inputs of every output pixel, then a 1x1 layer
    // with K = 80 / 32 (pack_kpack); returns false when the layer is not of that kind
    bool conv_kpacked(const std::string& name, const Act& x, int stride, int pad, const Epi& ep, const Act* dst, Act* out);

    // The reference's small-tensor route (torch ConvParams::use_mkldnn is false: batch 1, kernel <= 3, <= 20480 input
    // elements -> im2col + MKL sgemm): its own accumulation order, k = c -> ky -> kx in K blocks.
    bool small_tensor_layer(const std::string& name, const Act& x) const;  // (x: any tensor on the layer's input grid)
    Act conv_small(const std::string& name, const Act& x, int stride, int pad, const Epi& ep, const Act* dst);

    // torch.sigmoid on the CPU is not one function: the last len % 32 elements of every parallel chunk of the
    // tensor go through the scalar path (libm's expf instead of Sleef's vector exp).  A tensor that has such elements -- e.g.
    // the 320 x 16 x 16 attention map of a 256 x 256 image: three chunks of 27307 -- cannot take its gate in the conv epilogue,
    // which knows no flat index: the conv then writes its plain output and sigmoid_gate_ref_kernel applies a * sigmoid(b) + x.
    bool sigmoid_scalar_tails(long numel) const;
    bool gate_needs_own_pass(const std::string& name, const Act& x, int stride, int pad, const Epi& ep);
    Act conv_gated_ref(const std::string& name, const Act& x, int stride, int pad, const Epi& ep, const Act* dst);

    Act conv(const std::string& name, const Act& x, int stride, int pad, Epi ep = Epi(), const Act* dst = nullptr,
             const std::string* fuse1x1 = nullptr, const std::string* lead1x1 = nullptr, const Act* lead_dst = nullptr);

    // Keep the taps of a (one-phase) tap table whose dy + dx has parity `odd`, in their order; the rest of the table is
    // zeroed.  Returns the number kept.
    static int keep_taps(TapTable& t, int odd);

    // A stride-1 k x k conv whose INPUT is non-zero at the anchor positions only ((row + col) odd: the slice right after its
    // anchor pass, utils/ckbd.py:37-48 -- what the local-context convs read, elic_united.py:296,309).  An output pixel of
    // parity q then only meets non-zero inputs under the taps with (dy + dx) & 1 == 1 - q: the anchor outputs need the 13
    // taps with dy + dx even, the other outputs the 12 with dy + dx odd.  Two checkerboard-output launches (ConvArgs::ckbd
    // 1 / 2), each with its half of the tap table: half the MFMA work, and every output keeps its fma chain minus terms
    // that are exact zeros (round 4; RGBD_NO_ANCHOR_TAPS=1 runs the full conv).  Worth it for the 192-channel slice only
    // (368 -> 255 us at c3); at 64 channels two launches cost more than the taps they save (71 -> 86 us).
    void conv_anchor_in(const std::string& name, const Act& x, int pad, const Act& dst);

    // The same layer kind for nm modalities (names n[0] / n[1]: RGB / depth branch).  nm == 2: one grouped launch when the
    // two plans agree in every shape, otherwise (first / last image-facing layers: 3 vs 1 channels) two launches.
    // nm == 1: conv() of entry 0.  Every array argument is read at [0, nm) only.
    void conv2(int nm, const std::string n[2], const Act x[2], int stride, int pad, const Epi ep[2], const Act* const dst[2],
               Act out[2], const std::string* const fuse1x1[2] = nullptr, const std::string* const lead1x1[2] = nullptr,
               const Act* const lead_dst[2] = nullptr);

    // drain recorded event pairs into prof_ms (call after the stream has been synchronised)
    void profile_collect();

    void copy_ch(const Act& src, const Act& dst);

    // the pair (mid: 3x3 + ReLU, last: 1x1 + residual) as one launch?  (a speed decision: the results are bit-identical)
    bool fusable(const std::string& mid, const std::string& last, const Act& x, int groups = 1);

    // ... and can the leading 1x1 + ReLU of the block after it ride along?  (its input is this block's output)
    bool lead_fusable(const std::string& last, const std::string& lead, const Act& x);
    // outputs of leading layers that a previous block's launch has already produced, by layer name
    std::map<std::string, Act> pre_leads;

    // ---- blocks of nm modalities (p[0] / p[1]: the RGB / depth branch's layer names; arrays are read at [0, nm)) --------
    // With nm == 2 every layer pair is one grouped launch (conv2) and the fusion decisions are taken for the pair: a grouped
    // launch tiles like the layer at twice the batch.  nm == 1 is the block of one branch.
    void take_lead2(int nm, const std::string n[2], const Act x[2], Act t[2]);

    // modules/layers/res_blk.py:7-27.  next_lead[m]: the leading layer of the block that consumes this block's output
    // ("" = none)
    void bottleneck2(int nm, const std::string p[2], const Act x[2], const Act* const dst[2], const std::string next_lead[2],
                     Act out[2]);

    // CompressAI/compressai/layers/layers.py:177-196
    void res_unit2(int nm, const std::string p[2], const Act x[2], const std::string next_lead[2], Act out[2]);

    // layers.py:198-213
    void attention2(int nm, const std::string p[2], const Act x[2], const Act* const dst[2], Act out[2]);

    // modules/transform/attention.py:84-97: x[m] -> dst[m] = x[m] * sigmoid(...) (+ add[m]: STF_united adds the gated
    // features to the stream instead of concatenating them; add may be nullptr)
    void esa2(int nm, const std::string p[2], const Act x[2], const Act dst[2], const Act* const add[2]);

    // modules/transform/attention.py:35-48; rgb/depth: views of N channels; writes the gated features into
    // r_dst / d_dst (N channels each)
    void bi_spf(const std::string& p, const Act& rgb, const Act& depth, const Act& r_dst, const Act& d_dst,
                bool residual = false);

    // modules/transform/attention.py:63-67: y = x * g (mode 0) or x + x * g (mode 1), g = the per-(n,c) sigmoid weights of x
    // means / mstride: the channel means of x when somebody holds them already (Bi-CEE: SliceMeans), else they are computed.
    void se_scale_to(const std::string& p, const Act& x, int mode, const Act& y, const float* means = nullptr, int mstride = 0);

    // the SE of cat(own, other) written into the two halves of f (synthesis.py:345-362): means side by side, one gate
    void se_cat_to(const std::string& p, const Act& own, const Act& other, const Act& f);

    // ---- transforms -----------------------------------------------------------------------------
    // The ELIC-type analysis / synthesis transforms are lists of stages -- "conv" / "deconv" (k 5, stride 2), "rb"
    // (bottleneck2), "attn" (attention2), "spf" (cross-modal fusion) -- walked by stages().  What a family decides about the
    // walk is in its descriptor; ends and leads are on for ELIC_united only (open for the other families).
    // an "spf" stage: none, bi_spf (both branches widen), bi_spf_single (depth only)
    enum Fusion { kNoFusion, kBiSpf, kBiSpfDepth };
    struct Stages {
        const char* const* kinds;
        int n;
        int nm;
        const char* prefix[2];  // layer-name prefix per modality
        Fusion fusion;
        bool grouped;  // the branches of a stage go as one grouped launch (conv2(2, ...)), not one after the other
        bool ends;     // the stage loop alternates the workspace ends (ends_begin / ends_stage / ends_finish)
        bool leads;    // an "rb" stage hands the next block's .branch.0 to its fused tail (next_lead)
        const Act* mids = nullptr;  // kSyn15 with return_mid: buffers the outputs of stages 1, 5 and 10 (up1..up3,
                                    // synthesis.py:54-67) are copied into
        const Act* guides = nullptr;  // kSyn15 of SynthesisTransformPlus (synthesis.py:98-110): up1..up3 of the aux decoder; the
                                      // output of stages 1, 5 and 10 is replaced by spatial_aligner(sp_prefix + "spK", x, guides[K-1])
        const char* sp_prefix = "";   // name prefix of sp1, sp2, sp3
    };
    static constexpr const char* kAna18[18] = {"conv", "rb", "rb", "rb", "spf", "conv", "rb", "rb", "rb",
                                               "attn", "spf", "conv", "rb", "rb", "rb", "spf", "conv", "attn"};
    static constexpr const char* kSyn18[18] = {"attn", "deconv", "spf", "rb", "rb", "rb", "deconv", "attn", "spf",
                                               "rb", "rb", "rb", "deconv", "spf", "rb", "rb", "rb", "deconv"};
    static constexpr const char* kAna15[15] = {"conv", "rb", "rb", "rb", "conv", "rb", "rb", "rb",
                                               "attn", "conv", "rb", "rb", "rb", "conv", "attn"};
    static constexpr const char* kSyn15[15] = {"attn", "deconv", "rb", "rb", "rb", "deconv", "attn", "rb",
                                               "rb", "rb", "deconv", "rb", "rb", "rb", "deconv"};
    void stages(const Stages& sd, const Act in[2], Act out[2]);
    // ELIC_united: analysis.py:116-174 / synthesis.py:126-184
    void g_a(const Act x[2], Act y[2]);
    void g_s(const Act yhat[2], Act xhat[2]);

    // analysis.py:231-242
    void h_a(const Act& yr, const Act& yd, Act* zr, Act* zd);

    // conv_transpose2d(k 5, stride 2, pad 2, output_padding 1) + activation in the reference's CPU arithmetic: the layer's
    // measured recipe (refarith_tables.json kind 3) run by deconv_s2_ref_run(), scratch from the arena.
    // false = no recipe for this shape (the caller runs the sub-pixel-phase kernel).
    bool deconv_s2_ref(const std::string& name, const Act& x, int act, Act* out);

    // synthesis.py:345-362.  cat(own, other) -> SE -> deconv without materialising the unscaled concatenation: the channel
    // means of the two inputs land side by side (what the mean of the concatenation would be, channel by channel), the
    // gate is computed from them, and each input is scaled straight into its half of the deconv's input buffer.  The SE
    // gates stay per modality; with nm == 2 the two (transposed) convs are one grouped launch.
    void hs_block2(int nm, const std::string p[2], const Act own[2], const Act other[2], bool last, Act out[2]);

    // synthesis.py:316-323
    void h_s(const Act& zr, const Act& zd, Act* hr, Act* hd);

    // ---- the checkerboard slice loop (Bi-CEE, elic_united.py:265-348 / 454-541; elic_united_R2D.py:149-326; elic.py:180-251 /
    // 268-316) --------------------------------------------------------------------------------------------------------
    // y is coded slice by slice (slice_ch), every slice in two checkerboard parts per modality: anchor part of RGB, of depth,
    // non-anchor part of RGB, of depth.  The (scales, means) of a part come from a parameter net over everything known by then,
    // kept side by side in a context buffer per slice so that a net's input is a channel view of it, not a concatenation:
    // the hyper tensors (2M channels each), the channel contexts (a net over the slices coded so far, 2C channels, from the
    // second slice on) and the local contexts (a 5x5 conv over the slice's y_hat as decoded so far, 2C channels).  A net
    // reads its buffer from one segment to the end; the one input that is not such a suffix (the depth anchor net's: RGB's
    // local context, then hyper tensors and channel contexts, with depth's local-context slot in between) is gathered.
    // slice_loop_ckbd() is that loop for every family; what a family decides about it is in its SliceLoop descriptor.
    enum Seg : int8_t { kLocR, kLocD, kHypR, kHypD, kChR, kChD, kSegEnd = -1 };  // local ctx / hyper / channel ctx of RGB, depth
    struct CtxNet {
        int8_t buf;     // the context buffer the net reads ...
        Seg first;      // ... from this segment to the buffer's end
        bool gathered;  // buffer 0's kLocR slot in front of that suffix, copied together (they are not adjacent)
    };
    struct SliceLoop {
        Seg layout[2][7];       // segment order of each context buffer, kSegEnd-terminated (an unused buffer starts with it);
                                // the single-modal family's segments are the RGB ones
        CtxNet net[2][2];       // [anchor, non-anchor][modality]: input of each parameter net of a slice
        int8_t loc_buf[3];      // the buffer whose slot takes <m>local_context of RGB (kLocR), of depth (kLocD), and
                                // rgb_local_context_anchor_with_nonanchor (kLocR again)
        const char* prefix[2];  // layer-name prefix per modality
        // parameter-net form: SE rescale in front of the three layers (entropy.py:69-78) or not (entropy.py:7-29), and the
        // checkerboard half (Epi::ckbd) on all three layers (1x1: no layer mixes positions) or on the last one only
        bool se, ckbd_all;
        // Speed levers, on for ELIC_united / STF_united only (open for the other families).  mean_cache: the SE
        // gates' channel means are kept per segment (needs one buffer with the modalities' hyper segments, and their
        // channel contexts, side by side: one launch covers both); anchor_taps: conv_anchor_in() for the local contexts of the
        // anchor half; grouped_ch: the modalities' channel-context nets as grouped launches
        bool mean_cache, anchor_taps, grouped_ch;
    };
    static constexpr SliceLoop kLoopUnited = {{{kLocR, kLocD, kHypR, kHypD, kChR, kChD, kSegEnd}, {kSegEnd}},
                                              {{{0, kHypR, false}, {0, kHypR, true}}, {{0, kLocR, false}, {0, kLocR, false}}},
                                              {0, 0, 0}, {"rgb_", "depth_"}, true, false, true, true, true};
    // RGB's nets see no depth: their own buffer; depth's as in ELIC_united, its kLocR slot written by the second RGB conv only
    static constexpr SliceLoop kLoopR2D = {{{kLocR, kHypR, kChR, kSegEnd}, {kLocR, kLocD, kHypR, kHypD, kChR, kChD, kSegEnd}},
                                           {{{0, kHypR, false}, {1, kHypR, true}}, {{0, kLocR, false}, {1, kLocR, false}}},
                                           {0, 1, 1}, {"rgb_", "depth_"}, true, false, false, false, false};
    static constexpr SliceLoop kLoopSingle = {{{kLocR, kChR, kHypR, kSegEnd}, {kSegEnd}},
                                              {{{0, kChR, false}, {}}, {{0, kLocR, false}, {}}},
                                              {0, 0, 0}, {"", ""}, false, true, false, false, false};
    // ELIC_master's latent codec (elic_master.py:148,172,188): kLoopSingle's layout with EntropyParametersEX nets (SE rescale,
    // 1x1 / 3x3 / 5x5: entropy.py:56-78), whose 3x3 and 5x5 layers mix positions: only the last layer takes the checkerboard half
    static constexpr SliceLoop kLoopMaster = {{{kLocR, kChR, kHypR, kSegEnd}, {kSegEnd}},
                                              {{{0, kChR, false}, {}}, {{0, kLocR, false}, {}}},
                                              {0, 0, 0}, {"", ""}, true, false, false, false, false};
    const SliceLoop& slice_loop_family() const
    {
        return family == Family::ELIC                 ? kLoopSingle
               : family == Family::ELIC_master_latent ? kLoopMaster
               : family == Family::ELIC_united_R2D    ? kLoopR2D
                                                      : kLoopUnited;
    }

    // The parameter net of one part: [SE rescale,] three convs (1x1 / 3x3 / 5x5 or 1x1 x 3; padding k / 2) with ReLU between.
    // SE writes the rescaled copy the first conv reads (params + se(params), keeping the reference's association); `means`:
    // the input's channel means where the caller has them already.  `part` (1 anchor / 2 non-anchor): the caller only reads
    // that checkerboard half of (scales, means) (ckbd.py:83-125), so the last -- and largest -- conv computes just that half,
    // and so do the layers in front of it where none mixes positions; the values are those of the full convs.
    Act entropy_params(const SliceLoop& d, const std::string& p, const Act& ctx, int part, const Act* dst = nullptr,
                       const float* means = nullptr, int mstride = 0);

    // context.py:10-30 (slice i's two nets read only what earlier slices decoded: independent)
    void channel_context2(int nm, const std::string p[2], const Act x[2], const Act dst[2]);

    // what the coding loops (slice_loop_ckbd, slice_loop, two_pass_ckbd) hand to code_part()
    struct Coding {
        bool encode = true;
        bool estimate = false;      // eval-mode forward(): quantise + likelihood, no symbols
        Act lik[2];                 // likelihood tensors [B,h,w,M] per modality (estimate mode)
        int per_image = 1;
        int64_t per_image_total = 0;  // symbols per image per modality
        int32_t* sym = nullptr;       // [2][B*per_image_total]
        int32_t* idx = nullptr;
        const int64_t* stream_base = nullptr;  // device [B] symbol base of each stream inside a modality region
        const int32_t* force = nullptr;        // teacher forcing: [2][B*per_image_total] symbols later contexts are built from
        // decode side
        const uint32_t* words = nullptr;
        const int64_t* stream_off = nullptr;  // device [2][nstreams]
        const int64_t* stream_len = nullptr;
        uint64_t* state = nullptr;  // device [2][nstreams][2] ([lanes + 1] with the wide coder)
        int* err = nullptr;         // wide coder: the call's error flag
        int nstreams = 0;
        bool first[2] = {true, true};
    };

    void code_part(Coding& cd, int mod, int anchor, const Act& params, const Act& y_slice, const Act& yhat_slice,
                   int64_t part_off);

    float* yhat_base[2] = {nullptr, nullptr};

    // y, hyp, yhat: read at [0, nm); y is null when decoding
    void slice_loop_ckbd(Coding& cd, const SliceLoop& d, int nm, const Act* y, const Act hyp[2], const Act yhat[2]);

    // ---- STF_united (models/stf_united.py; BASELINE config 5): Swin transforms on [B,H,W,C] token maps -------------
    Act layernorm(const std::string& p, const Act& x);
    // stf_united.py:118-214: x + proj(attn(norm1(x))), then + mlp(norm2(.)); GELU and both adds are conv epilogues -- for both
    // modalities at once (round 4): the RGB and the depth stack of STF_united run the same layer shapes
    // on independent data between two fusions, so every Linear is one grouped conv launch (conv2) and every LayerNorm /
    // window attention one launch over both tensors -- half the launches of a model whose launches are too small to fill the
    // chip (35 us on average at one 512x512 pair).  Each output keeps its arithmetic: bit-identical to the one-by-one form.
    // nm == 1 (the single-modal STF, models/stf.py): the same blocks on one tensor; arrays are read at [0, nm) only.
    // A kernel with two operand sets (LayerNorm, window attention) over in[m] -> out[m] of nm modalities: one launch with
    // the second set when g_pair and the two modalities agree in shape and in both channel strides, else one launch each.
    // launch(m, pair): set m alone, or (pair) sets 0 and 1.
    template <class F>
    void pair_or_each(int nm, const Act in[2], const Act out[2], F launch)
    {
        const bool same = nm == 2 && g_pair && in[0].n == in[1].n && in[0].h == in[1].h && in[0].w == in[1].w &&
                          in[0].c == in[1].c && in[0].cs == in[1].cs && out[0].cs == out[1].cs;
        int r = launch(0, same);
        if (!r && nm == 2 && !same) r = launch(1, false);
        if (r) fail(r);
    }
    void layernorm2(int nm, const std::string p[2], const Act x[2], Act y[2]);
    // the Swin block after its attention: x + attn.proj(a), then + mlp(norm2(.)) into out (allocated by the caller, before
    // its arena mark); allocates x1, t2 and the hidden layer, in that order
    void swin_block_tail2(int nm, const std::string p[2], const Act x[2], const Act a[2], const Act out[2]);
    void swin_block2(int nm, const std::string p[2], const Act x[2], int shift, int heads, Act out[2]);
    // Spatial_aligner (modules/transform/spatialAligner.py:341-390): patch embeddings of x and guided, two Swin blocks whose
    // attention reads q from x and k, v from guided (:279-338; norm1 on both, guided itself never updated: :290-291, 383-384),
    // and the 2x2 stride-2 transposed convolution `recovery`, whose taps do not overlap: a 1x1 convolution to 4 * out channels
    // (repacked in finalize) and a pixel shuffle.  prefix: "" (the stand-alone variant) or the block's name, e.g. "g_s.sp1".
    Act spatial_aligner(const std::string& prefix, const Act& x, const Act& guided);
    // ---- the attention contexts of MLIC++ (modules/transform/context.py), each a block of its own (families 7-9) -------
    // nn.Conv2d(C, C, 3, 1, 1, groups = C) (+ nn.GELU()): weight [C][1][3][3] and bias as plain arrays (finalize)
    Act dwconv(const std::string& name, const Act& x, bool gelu);
    // LocalContext.forward (:82-137): norm1, qkv_proj, the 5x5 window attention with `fusion` (one launch), proj, and
    // x + mlp(norm2(x)); the Linear layers are 1x1 convolutions, GELU and the add their epilogues
    Act local_context(const Act& x, const std::string& p = "", int heads = -1);
    // LinearGlobalInterContext.forward (:243-262; xk = xq = xv = x1, mode 0, with `skip`) and LinearGlobalIntraContext.forward
    // (:189-213; xk = anchor half of x1, xq = the other half, xv = x2, mode 1, no `skip`): three 1x1 + depthwise branches, the
    // linear attention, the 5x5 reprojection, and skip(a) (or a) + mlp(a)
    Act linear_context(const Act& xk, const Act& xq, const Act& xv, int mode, bool skip, const std::string& p = "", int heads = -1);
    // stf_united.py:270-366 for both modalities; down: 0 none, 1 PatchMerging (:217-249), 2 PatchSplit (:252-267)
    void basic_layer2(int nm, const std::string p[2], const Act x_in[2], int depth, int heads, int down, Act out[2]);
    void stf_stack(const std::string& root, const char* kind, const Act& r_in, const Act& d_in, const int* depths,
                   const int* heads, int down, Act* r_out, Act* d_out);
    void g_a_stf(const Act& rgb, const Act& depth, Act* y_r, Act* y_d);
    void g_s_stf(const Act& yr, const Act& yd, Act* xr, Act* xd);

    // ---- ELIC_united_R2D (models/elic_united_R2D.py): RGB on its own, depth conditioned on RGB ------
    // attention.py:14-32: only the depth-side gated features exist
    void bi_spf_single(const std::string& p, const Act& rgb, const Act& depth, const Act& d_dst);
    // analysis.py:56-112 / synthesis.py:186-242: the same 18 stages as ELIC_united, one branch after the other; the fusion
    // stage only widens depth
    void g_a_r2d(const Act x[2], Act y[2]);
    void g_s_r2d(const Act yhat[2], Act xhat[2]);
    // synthesis.py:364-380
    Act hs_block_single(const std::string& p, const Act& x, bool last);
    // synthesis.py:336-343
    void h_s_r2d(const Act& zr, const Act& zd, Act* hr, Act* hd);
    // ---- single-modal ELIC (models/elic.py:15-57; BASELINE config 1) ------------------------------------------
    // analysis.py:29-52 / synthesis.py:32-70: the same blocks as above without the cross-modal fusion stages
    Act g_a1(const Act& x);
    Act g_s1(const Act& yhat);
    const Act* mid_dst = nullptr;  // set around g_s_family by a return_mid call (run_forward / run_decompress)
    // ELIC_master_latent (family 20): g_a = AnalysisTransformEX(N, M, ch = 128), the kAna15 walk on a 128-channel input, and
    // g_s = SynthesisTransformPlus(N, M, ch = N) under "g_s.", family 13's guided walk (elic_master.py:67-68)
    Act g_s_master(const Act& yhat);
    const Act* guide_src = nullptr;  // up1..up3 of the call in progress (NHWC, converted in the prologue): set by guides_begin
    int guides_begin(const float* const up_dev[3], int B, int H, int W, Act up[3]);
    // analysis.py:207-216
    Act h_a1(const Act& y);
    // synthesis.py:276-285
    Act h_s1(const Act& zhat, const Act* dst = nullptr);
    // ---- single-modal STF (models/stf.py:408-816): the Swin transforms without the cross-modal fusion, and the channel-slice
    // entropy model: 12 raster slices of 32 channels, two hyper-synthesis nets, per slice two parameter nets and latent
    // residual prediction (LRP) -------------------------------------------------------------------------------------
    static constexpr int kStfSlices = 12, kStfSliceCh = 32, kStfSupport = 6;  // num_slices, M / num_slices, max_support_slices
    Act swin_stack1(const std::string& root, const Act& x_in, const int* depths, const int* heads, int down);
    // stf.py:704-713
    Act g_a_stf1(const Act& img);
    // stf.py:809-815 (end_conv: 5x5 conv, PixelShuffle(2), 3x3 conv)
    Act g_s_stf1(const Act& yhat);
    // stf.py:507-517: five 3x3 convolutions (the third and the fifth with stride 2), GELU between them
    Act h_a_stf1(const Act& y);
    // stf.py:519-540: h_mean_s and h_scale_s have the same layer shapes on the same input: ONE grouped launch per layer.
    // subpel_conv3x3 = 3x3 conv to 4 C channels + PixelShuffle(2); the GELU behind it is pointwise, so it rides in the conv's
    // epilogue.  The last layers write the first 384 channels of the two context buffers.
    void h_s_stf1(const Act& zhat, const Act& means_dst, const Act& scales_dst);

    // ---- MLIC++ (models/mlicpp.py; mlic_engine.hip): residual blocks with GDN / IGDN as in the checkerboard Cheng2020 family but
    // with GELU (stride / up-sampling blocks) and ReLU (plain blocks), GELU hyper transforms, and a loop over slice_num slices of
    // 32 channels, each coded in two checkerboard parts under the attention contexts and per-slice networks above ---------------
    // res_blk.py:30-58: relu(conv2(relu(conv1 x))) + x, or + skip(x) (1x1) where the widths differ
    Act ml_res_block(const std::string& p, const Act& x);
    // res_blk.py:61-91: GDN(conv2(gelu(conv1 x, stride 2))) + skip(x) (1x1, stride 2)
    Act ml_res_block_stride(const std::string& p, const Act& x);
    // res_blk.py:94-119: IGDN(conv(gelu(subpel_conv x))) + upsample(x); the two sub-pixel convs as one grouped launch
    Act ml_res_block_up(const std::string& p, const Act& x);
    Act g_a_mlic(const Act& img);   // analysis.py:11-26
    Act g_s_mlic(const Act& yhat);  // synthesis.py:12-29
    Act h_a_mlic(const Act& y);     // analysis.py:180-204
    // synthesis.py:248-273, widths M, 3M/2, 2M; the last layer writes `dst` = hyper_params (scales | means)
    void h_s_mlic(const Act& zhat, const Act& dst);
    // mlicpp.py:220-303 / 331-404 / 105-182.  state [B,h,w,2M]: hyper_means in channels [0, M), y_hat slot i in
    // [M + 32 i, M + 32 i + 32).  Every concatenation the reference forms over decoded slices is a channel view of it: the LRP
    // input is the prefix [0, M + 32 (i + 1)), cat(y_hat_slices) is [M, M + 32 i), y_hat itself is [M, 2M).  hyper [B,h,w,2M]:
    // hyper_params, a segment of its own for the parameter networks.  y: null when decoding.
    void slice_loop_mlic(Coding& cd, const Act* y, const Act& hyper, const Act& state);

    ScaleTab scale_tab{};  // host copy of the Gaussian scale table: the slice kernels take it by value

    // one slice through the coder's side of the loop: symbols / indexes (encode), indexes + rANS + dequantise (decode) or
    // quantise + likelihood (forward); the pre-LRP y_hat lands in `slot`
    void code_slice(Coding& cd, int i, const Act& mu, const Act& sg, const Act& y_slice, const Act& slot);

    // stf.py:735-758 / 786-807 / 647-667.  ctxm = [latent_means 384 | 7 x 32], ctxs = [latent_scales 384 | 6 x 32 (+ 32 unused:
    // the two buffers share one channel stride so that the nets' first layers pair)]: slice i's pre-LRP y_hat goes to slot
    // min(i, 6) of ctxm, the LRP net reads the prefix up to and including that slot, the LRP update finalises slots 0..5 in
    // both buffers and slice i of yhat; the parameter nets of slice i read the prefix of min(i, 6) slots.  No concatenation.
    void slice_loop(Coding& cd, const Act* y, const Act& ctxm, const Act& ctxs, const Act& yhat);

    // ---- checkerboard Cheng2020 (models/Cheng2020withCKBD.py:40-174 on compressai/models/waseda.py:22-81): residual blocks of
    // 3x3 / 1x1 convolutions with GDN / IGDN, sub-pixel up-sampling, and a two-pass checkerboard entropy model on one slice of
    // M = N channels ----------------------------------------------------------------------------------------------------
    // GDN / IGDN (layers/gdn.py:52-67) + the block's `out += identity` (layers.py:97,125) as one launch (gdn.hip).  In the
    // profile it counts as the 1x1 convolution it contains (2 C^2 FLOPs per pixel).
    Act gdn(const std::string& name, const Act& x, bool inverse, const Act* res);
    Act pixel_shuffle(const Act& t);
    // layers.py:129-159: leaky(conv2(leaky(conv1 x))) + x
    Act ck_res_block(const std::string& p, const Act& x);
    // layers.py:67-98: GDN(conv2(leaky(conv1 x, stride 2))) + skip(x) (1x1, stride 2)
    Act ck_res_block_stride(const std::string& p, const Act& x);
    // layers.py:101-126: IGDN(conv(leaky(subpel_conv x))) + upsample(x); the two sub-pixel convs read the same tensor with
    // the same layer shape: one grouped launch.  LeakyReLU is pointwise, so it rides in front of the shuffle.
    Act ck_res_block_up(const std::string& p, const Act& x);
    // waseda.py:38-46.  Every stage's temporaries are released once its output has been copied down.
    Act ck_stage(const Act& x, const std::function<Act(const Act&)>& f, int oh, int ow, int oc);
    Act g_a_ckbd(const Act& img);
    // waseda.py:72-81
    Act g_s_ckbd(const Act& yhat);
    // waseda.py:48-58
    Act h_a_ckbd(const Act& y);
    // waseda.py:60-70; the last layer writes the hyper half of the entropy-parameter input [ctx 2M | hyper 2M]
    void h_s_ckbd(const Act& zhat, const Act& dst);
    // priors.py:403-409: three 1x1 convolutions.  part 1 (anchor, Cheng2020withCKBD.py:122-124): the context half of the
    // input is zero, so the first layer runs on the hyper half of its input channels only ("entropy_parameters.0.hyper": the
    // same chain without terms that are exact zeros); 1x1 layers do not mix positions, so each pass computes and stores its
    // own checkerboard half of `out` (part 0: the whole grid, forward()).
    void ck_entropy_params(const Act& cat, int part, const Act& out);
    // CheckerboardContext (Cheng2020withCKBD.py:12-37): the weight is masked when packed; only the 12 taps with (ky + kx) odd
    // are issued and only the non-anchor outputs computed (the anchor half of dst is left as it is: zeros)
    void ck_context(const Act& yhat, const Act& dst);
    // Cheng2020withCKBD.py:121-130 / 154-167: cat = [ctx 2M | hyper 2M] with the context half zeroed and the hyper half filled;
    // params = [scales M | means M]: the anchor pass leaves its half there, the non-anchor pass the other half
    void two_pass_ckbd(Coding& cd, const Act* y, const Act& cat, const Act& params, const Act& yhat);

    // ---- stream I/O of the call paths (engine.hip), for nm = 1 (the single-modal families) or 2 modalities -------------
    // workspace of a compress call: symbols, indexes and stream slots of every modality, and the stream geometry
    struct EncBufs {
        // meta: [0,B) y stream base inside a modality region (checkerboard kernels); [2B,3B) z bases; [3B,4B) z counts;
        //   [6B,6B+nm*B) z out_words; from 8B: y encoder bases [nm*ny] (absolute), counts [nm*ny], out_words [nm*ny]
        int64_t* meta = nullptr;
        int32_t *sym = nullptr, *idx = nullptr;    // [nm][B*T]
        int32_t *zsym = nullptr, *zidx = nullptr;  // [nm][B*Tz]
        uint32_t* ywords = nullptr;                // [nm][ny] slots of ycap words
        uint32_t* zwords = nullptr;                // [nm][B] slots of zcap words
        int* err = nullptr;
        int ny = 0;  // y streams per modality
        int64_t ycap = 0, zcap = 0;
        int64_t ycount = 0;  // symbols of one y stream
    };
    int enc_streams(int nm, int B, int64_t T, int64_t Tz, int per_image, EncBufs* e);
    int fetch_streams(int nm, int B, bool with_z, const EncBufs& e);
    // workspace of a decompress call with its streams uploaded
    struct DecBufs {
        uint32_t* words = nullptr;  // [y rgb | y depth | z rgb | z depth] slots of the size the encoder may produce
        uint64_t *state = nullptr, *zstate = nullptr;      // rANS states [nm][ns_y][2 (wide coder: lanes + 1)] / [nm][ns_z][2]
        int* err = nullptr;                                // wide coder only: the decoder's error flag
        int32_t *sym = nullptr, *idx = nullptr;            // [nm][B*T]
        int32_t *zsym = nullptr, *zidx = nullptr;          // [nm][B*Tz]
        const int64_t *yoff = nullptr, *ylen = nullptr;    // [nm][ns_y], in words
        const int64_t *zoff = nullptr, *zlen = nullptr;    // [nm][ns_z]
        const int64_t *ybase = nullptr, *zbase = nullptr;  // [B] symbol base of every image
    };
    int dec_streams(int nm, const uint8_t* const* ys[2], const int64_t* ylen[2], int ns_y, const uint8_t* const* zs[2],
                    const int64_t* zlen[2], int ns_z, int B, int64_t T, int64_t Tz, int per_image, DecBufs* d);

    // ---- the pieces every call path shares (engine.hip) ------------------------------------------------------------------
    void begin_call(int ref_batch_of_call, bool forward);  // resets the per-call state; the first thing a call path does
    int finish_body();                                     // body_end(), behind an error recorded inside the body
    int upload_forced(int nm, const std::vector<int32_t>* f, size_t n, int32_t** out);
    static Coding enc_coding(const EncBufs& e, int per_image, int64_t T, const int32_t* force);
    Coding dec_coding(const DecBufs& d, int per_image, int64_t T, int nstreams);
    // the z stage of modality m; pfx = "", "rgb_" or "depth_"
    void z_encode(int m, const char* pfx, const EncBufs& e, const Act& z, const Act& zhat, const int32_t* fz);
    void z_decode(int m, const char* pfx, const DecBufs& d, const Act& zhat);
    void z_estimate(const char* pfx, const Act& z, const Act& zhat, const Act& zlik);
    void y_encode(int nm, int B, const EncBufs& e);

    void name(const Modes& mo, const char* base, const Act a[2])  // a debug tensor per modality: "y" / "y_r", "y_d"
    {
        for (int m = 0; m < mo.nm; ++m) named[std::string(base) + mo.sfx[m]] = a[m];
    }

    // A family enters the call paths through these four hooks, which switch on `family`; Act arrays are read at
    // [0, nm).  latent_family owns everything between z_hat and y_hat: the family's buffers, its hyper synthesis (skipped when
    // the caller hands in `hyp`, the Latents path), its debug tensors and its coding loop.
    void g_a_family(const Act x[2], Act y[2]);
    void h_a_family(const Act y[2], Act z[2]);
    void g_s_family(const Act yhat[2], Act xhat[2]);
    void latent_family(Coding& cd, int B, int h, int w, const Act* y, const Act* zhat, const Act* hyp, Act yhat[2]);

    void analysis(const Act x[2], const Act y[2]);  // y = g_a(x), into the caller's buffers

    // lat != nullptr: the Bi-CEE stage alone (compress_united / decompress_united): latents and hyper parameters come
    // from the caller as NCHW device tensors, the transforms and the z path are skipped
    struct Latents {
        const float* y[2];    // [B,M,h,w]     (compress only)
        const float* hyp[2];  // [B,2M,h,w]
        float* yhat[2];       // [B,M,h,w]     (decompress only)
    };
    // the call paths: nm tensors per argument.  A model with another number of modalities is refused with RGBD_ESTATE, the
    // code such a call always ended with (a single-modal engine has none of the rgb_ / depth_ layers: conv_of)
    using In2 = std::array<const float*, 2>;
    using Out2 = std::array<float*, 2>;
    int run_compress(int nm, In2 x_dev, int B, int H, int W, int per_image, const Latents* lat = nullptr);
    // up: NULL, or (single-modal ELIC only) the three NCHW tensors of return_mid: [B,N,H/8,W/8], [B,N,H/4,W/4], [B,N,H/2,W/2]
    using Mid3 = std::array<float*, 3>;
    // guides: NULL, or (ELIC_master_latent only, where they are required for every call that runs g_s) the three NCHW tensors
    // up1..up3 of the aux decoder, shaped like Mid3
    using Guide3 = std::array<const float*, 3>;
    int run_forward(int nm, In2 x_dev, int B, int H, int W, Out2 xhat_dev, Out2 ly, Out2 lz, const Mid3* up = nullptr,
                    const Guide3* guides = nullptr);
    int run_decompress(int nm, const uint8_t* const* ys[2], const int64_t* ylen[2], int n_y, const uint8_t* const* zs[2],
                       const int64_t* zlen[2], int B, int h, int w, Out2 xhat_dev, const Latents* lat = nullptr,
                       const Mid3* up = nullptr, const Guide3* guides = nullptr);
    void mids_begin(int B, int H, int W, Act mid[3]);  // workspace of up1..up3; g_s1 fills it while mid_dst points at it
    int mids_out(const Act mid[3], int B, int H, int W, const Mid3& up);
    int run_aligner(const float* x_dev, const float* guided_dev, int B, int H, int W, float* out_dev);
    // SynthesisTransformPlus: yhat [B,M,h,w], up[k] [B,N,2h << k,2w << k] -> out [B,out_ch,16h,16w]
    bool plus_guides = true;  // rgbd_debug_synthesis_plus_guides(m, 0): the same walk without the three aligners (a timing aid)
    int run_synthesis_plus(const float* yhat_dev, const float* const up_dev[3], int B, int h, int w, float* out_dev);
    // the contexts: x1 (and, LinearGlobalIntraContext, x2) [B,in_ch,H,W] -> out [B,out_ch,H,W]
    int run_context(const float* x1_dev, const float* x2_dev, int B, int H, int W, float* out_dev);
    // ---- the per-slice networks of MLIC++, each a block of its own (families 15-17; engine_swin.hip) -------------------------
    // EntropyParametersMLIC.forward (entropy.py:43-53) on the concatenation of nseg tensors: ONE launch_pixel_mlp4 that reads the
    // segments where they are (mlp_fused), or the concatenation written out and four conv() launches with the GELU epilogue.
    // part: 0 the whole grid, 1 / 2 the anchor / non-anchor pixels only (Epi::ckbd); then dst holds the other pixels' values.
    bool mlp_fused = true;  // rgbd_entropy_params_mlic_set_fused
    Act entropy_params_mlic(const Act* seg, int nseg, int part, const Act* dst, const std::string& p = "", int out_dim = -1);
    // ChannelContext.forward (context.py:152-160): three 3x3 convolutions, GELU between them
    Act channel_context_mlic(const Act& x, const std::string& p = "");
    // LatentResidualPrediction.forward (LRP.py:22-26): four 3x3 convolutions, GELU between them, then 0.5 * tanh
    Act lrp_mlic(const Act& x, const std::string& p = "", bool tanh = true);
    // seg_dev[i] [B,seg_c[i],H,W] (one tensor of in_ch channels for the two 3x3 modules) -> out [B,out_ch,H,W]; parity -1 / 0 / 1
    // (EntropyParametersMLIC only): all pixels / the anchor pixels / the others, the rest of out keeps its values
    int run_slice_net(const float* const* seg_dev, const int* seg_c, int nseg, int parity, int B, int H, int W, float* out_dev);
    int ensure_arena(size_t bytes);
};

// One call through the graph cache: a dry run sizes the workspace of a new call shape, the second call of a shape captures
// its HIP graph, later ones replay it (used by every compress / decompress / forward entry point of the C ABI).
// One call = a sizing pass over the layer graph (workspace high-water mark; skipped when a cached HIP graph of this call
// shape exists, which implies the workspace already fits) and the real pass.
template <class F>
static int run_sized(rgbd_elic* m, const std::string& key, F&& run)
{
    rgbd_elic::GraphEntry* ge = m->graph_entry(key);
    if (!(ge && ge->exec)) {
        m->cur_ge = nullptr;
        m->arena.dry = true;
        m->arena.reset();
        m->arena.peak = 0;
        int r = run();
        m->arena.dry = false;
        if (r) return r;
        r = m->ensure_arena(m->arena.peak);  // a re-allocation drops every cached graph
        if (r) return r;
        ge = m->graph_entry(key);
    }
    m->cur_ge = ge;
    m->capture_failed = false;
    int r = run();
    if (r) m->body_abort();
    if (r && m->capture_failed) {
        // The capture of this call was lost before anything of its body ran.  Re-run it eagerly (the prologue is
        // idempotent); the entry tries again on its next call and retires to eager launches after kMaxCaptureFails.
        if (ge) ++ge->capture_fails;
        m->cur_ge = nullptr;
        m->capture_failed = false;
        r = run();
        if (r) m->body_abort();
        if (!r && ge) ++ge->seen;
    }
    m->cur_ge = nullptr;
    return r;
}

