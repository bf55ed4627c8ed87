// Host runtime of the gfx950 codec engine, part 1 of 4: weight packing, the workspace arena and `struct rgbd_elic` -- the
// layer graph of the six model variants (ELIC_united, single-modal ELIC, STF_united, ELIC_united_R2D, single-modal STF, checkerboard
// Cheng2020) as inline methods
// that plan and issue HIP kernel launches on one stream, the conv planner (tiles, split-K, reference arithmetic) and the
// per-call-shape HIP-graph cache.  engine.hip holds the call paths (compress / decompress / forward: one per direction for
// one or two modalities; a family enters them through the four `*_family` hooks), engine_abi.hip and hooks_abi.hip the C ABI
// (include/rgbd_amd.h): the engine's entry points, and the operator hooks and debug switches.  Everything shared between those
// translation units is `inline` here
// (one instance).
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
#include <chrono>
#include <condition_variable>
#include <dirent.h>
#include <execinfo.h>
#include <signal.h>
#include <sys/syscall.h>
#include <thread>
#include <unistd.h>

#include "../../include/rgbd_amd.h"
#include "common.h"
#include "conv_args.h"
#include "engine_internal.h"


// (process-wide switches and the helpers below: `inline` -- one instance for engine.hip, engine_abi.hip and hooks_abi.hip -- inside a namespace of
// their own, so that the weak symbols they become cannot collide with a host application's globals)
namespace rgbd_rt {


// ------------------------------------------------------------------------------------------------
// packed layers
// ------------------------------------------------------------------------------------------------
struct HostTensor {
    std::vector<float> v;
    std::vector<int64_t> shape;
};

// perm_in / perm_out: store the input / output channels at their permuted positions (rgbd_cperm)
inline int pack_conv(const HostTensor& w, const HostTensor* b, bool transposed, PackedConv* pc, DevGen* gen = nullptr, int perm_in = 0,
              int perm_out = 0)
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

// SE_Block's fc.2.weight ([C][hidden]) as launch_se_fc reads it: transposed to [hidden][C], so that the gate kernel's
// consecutive lanes read consecutive addresses.  w1t must not alias w1.
inline void se_pack_fc2(const float* w1, size_t C, size_t Hd, float* w1t)
{
    for (size_t c = 0; c < C; ++c)
        for (size_t j = 0; j < Hd; ++j) w1t[j * C + c] = w1[c * Hd + j];
}

// ConvTranspose2d(cin -> cout <= 4, k = 5, stride 2, pad 2, output_padding 1) as ONE stride-1 3x3 conv over the input grid
// with 16 output channels = 4 output phases x 4: the per-phase form pads the couts to 16 for each of its 25 taps, this one
// runs 9 taps for all phases together (2.8x fewer MFMAs).  Output phase (ry, rx) at input offset (dy, dx) uses kernel
// element ky = ry + 2 - 2 dy, kx = rx + 2 - 2 dx when that is inside the kernel, else a zero weight; the taps run dy, dx =
// 1, 0, -1, which keeps every phase's real taps in the order make_taps() gives them -- with fma(0, x, acc) == acc the
// value of every output is the same chain as in the per-phase form (tests/test_gpu_conv.py::test_subpixel_deconv).
inline int pack_subpix(const HostTensor& w, const HostTensor* b, PackedConv* pc, DevGen* gen, int perm_in = 0)
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

// Conv2d(cin <= 3 -> cout, k 5, stride 2, pad 2) as a 1x1 layer over the packed input of launch_im2col5s2: weight of
// term n = tap * cin + c at packed index (n / 16) * 16 + (n % 4) * 4 + (n % 16) / 4
inline int pack_kpack(const HostTensor& w, const HostTensor* b, PackedConv* pc, DevGen* gen, int perm_out = 0)
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


// ---- hang diagnostics (RGBD_DEBUG_DESTROY=1) -----------------------------------------------------------------------------
// A HangWatch around a runtime call that may wait for the device (hipFree = implicit device synchronise): if the call has
// not returned after `secs`, every thread of the process prints its host backtrace (SIGUSR2 handler; the runtime is
// stripped, but the exported entry points -- hipFree, hipGraphLaunch, hsa_signal_wait_*, pthread lock waits -- tell a
// host lock cycle from a wait for a GPU signal), then every engine stream is queried (hipStreamQuery does not block), which
// names the stream that still holds work.  This is how the round-2 "hipFree never returns" report was taken apart.
inline std::mutex g_live_mu;
inline std::map<const void*, hipStream_t> g_live_streams;  // engine -> the stream of its last call
inline const bool g_dbg_destroy = getenv("RGBD_DEBUG_DESTROY") != nullptr;

inline void bt_handler(int)
{
    void* fr[64];
    const int n = backtrace(fr, 64);
    char hdr[64];
    const int l = snprintf(hdr, sizeof(hdr), "[bt tid %ld]\n", (long)syscall(SYS_gettid));
    if (l > 0) (void)!write(2, hdr, (size_t)l);
    backtrace_symbols_fd(fr, n, 2);
}

struct HangWatch {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    HangWatch(const char* what, int secs, bool always = false)
    {
        if (!g_dbg_destroy && !always) return;
        th = std::thread([this, what, secs] {
            std::unique_lock<std::mutex> lk(mu);
            if (cv.wait_for(lk, std::chrono::seconds(secs), [this] { return done; })) return;
            lk.unlock();
            if (!g_dbg_destroy) {
                // production (always-armed) mode is PASSIVE: one line naming the call.  Signalling every thread of the host
                // application, replacing its SIGUSR2 handler and querying streams from here is for RGBD_DEBUG_DESTROY=1 only
                // (round-4 advisor finding): hipFree legitimately waits for the device, a caller's long kernels can be the cause.
                fprintf(stderr, "[rgbd_amd] %s has not returned after %d s (RGBD_DEBUG_DESTROY=1 prints host backtraces)\n", what, secs);
                return;
            }
            fprintf(stderr, "[watchdog] %s has not returned after %d s; host backtraces of every thread follow\n", what, secs);
            void* warm[4];
            (void)backtrace(warm, 4);  // loads libgcc outside the signal handler
            struct sigaction sa, old_sa;
            memset(&sa, 0, sizeof(sa));
            sa.sa_handler = bt_handler;
            sa.sa_flags = SA_RESTART;
            sigaction(SIGUSR2, &sa, &old_sa);
            const long self = (long)syscall(SYS_gettid);
            if (DIR* d = opendir("/proc/self/task")) {
                while (dirent* e = readdir(d)) {
                    const long tid = atol(e->d_name);
                    if (tid <= 0 || tid == self) continue;
                    syscall(SYS_tgkill, (long)getpid(), tid, SIGUSR2);
                    usleep(200 * 1000);
                }
                closedir(d);
            }
            std::map<const void*, hipStream_t> live;
            {
                std::lock_guard<std::mutex> g(g_live_mu);
                live = g_live_streams;
            }
            for (const auto& kv : live) {
                fprintf(stderr, "[watchdog] query stream %p of engine %p ...\n", (void*)kv.second, kv.first);
                fflush(stderr);
                const hipError_t e = hipStreamQuery(kv.second);
                fprintf(stderr, "[watchdog]   -> %s\n", hipGetErrorName(e));
            }
            fprintf(stderr, "[watchdog] query NULL stream ...\n");
            fflush(stderr);
            const hipError_t e0 = hipStreamQuery(nullptr);
            fprintf(stderr, "[watchdog]   -> %s\n", hipGetErrorName(e0));
            fflush(stderr);
            sigaction(SIGUSR2, &old_sa, nullptr);  // the host application's handler is back
            if (getenv("RGBD_DIAG_EXIT")) _exit(86);  // diagnostics runs end by themselves instead of at a time limit
        });
    }
    ~HangWatch()
    {
        if (!th.joinable()) return;
        {
            std::lock_guard<std::mutex> lk(mu);
            done = true;
        }
        cv.notify_all();
        th.join();
    }
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
inline int small_conv_set_kblocks(SmallConvArgs* a, const int* lens, int n, int Kt)
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
using namespace rgbd_rt;

// What an engine handle is: a codec (0-5) or one module alone (6-9, 13: no codec calls, no tables, its own forward entry point).
// DESIGN.md and the history name the families by these numbers, so the numbers stay; 10-12 are reserved for the held-back
// modules of ELIC_master and refused everywhere: the table has holes, not a renumbering.
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
};
constexpr int kFamilies = 14;

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
                      // SynthesisTransformPlus: M)
    int out_ch = 0;   // module handles: output channels
    int ctx_heads = 0;  // contexts: num_heads
    // what the call paths (engine.hip) need to know about one versus two modalities; arrays are read at [0, nm)
    struct Modes {
        int nm;
        const char* sfx[2];  // suffix of the debug-tensor names: "y" / "y_r", "y_d"
        const char* eb[2];   // prefix of the entropy bottleneck's tensors
        int img_ch[2];       // image channels
        int clamp;           // FamilyRow::clamp
        bool forward_names_z;  // FamilyRow::forward_names_z
    };
    Modes modes() const
    {
        const FamilyRow& f = row();
        if (single()) return {1, {"", ""}, {"", ""}, {in_ch, in_ch}, f.clamp, f.forward_names_z};
        return {2, {"_r", "_d"}, {"rgb_", "depth_"}, {3, 1}, f.clamp, f.forward_names_z};
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
    const std::vector<int>* ref_blocks(int kind, int cin, int cout, int h, int w, int last = -1) const
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

    // conv-kernel profiling (bench.py roofline): HIP event pairs around every conv launch on the launch stream
    bool profile = false;
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
    int use_stream(void* stream)
    {
        s = (hipStream_t)stream;
        if (g_dbg_destroy) {
            std::lock_guard<std::mutex> g(g_live_mu);
            g_live_streams[this] = s;
        }
        return RGBD_OK;
    }
    // pinned staging for the per-call uploads (stream bytes, offsets): truly asynchronous copies, no per-call pinning
    int64_t* res_pin = nullptr;  // pinned landing buffer of the per-call result sizes
    static constexpr size_t kResPinBytes = 64 * 1024;
    void* pin = nullptr;
    size_t pin_cap = 0;
    hipEvent_t pin_ev = nullptr;
    bool pin_busy = false;

    void graphs_invalidate()
    {
        for (auto& kv : graphs) drop_entry(kv.second);
        graphs.clear();
        cur_ge = nullptr;
    }
    GraphEntry* graph_entry(const std::string& key)
    {
        if (!use_graphs || profile || !s) return nullptr;  // (the NULL stream cannot be captured)
        // (the stream is part of the key: a graph is replayed on the stream it was captured on)
        char sk[32];
        snprintf(sk, sizeof(sk), "|%p", (void*)s);
        const std::string cfg = "|" + std::to_string(tile_mode) + "|" + std::to_string(g_cfg_epoch) + "|";
        const std::string full = key + cfg + (sk + 1);
        auto it = graphs.find(full);
        if (it == graphs.end()) {
            // A dataset with many image sizes must not grow this cache without bound: entries of other tile modes / debug
            // epochs can never be replayed again and go first, then the least recently used ones.
            for (auto e = graphs.begin(); e != graphs.end();) {
                // (an entry captured on ANOTHER stream is not stale: an engine used on two streams keeps both sets, the LRU
                //  limit below bounds them)
                const std::string& k = e->first;
                const size_t bar = k.rfind('|');
                const bool stale = bar == std::string::npos || bar + 1 < cfg.size() ||
                                   k.compare(bar + 1 - cfg.size(), cfg.size(), cfg) != 0;
                if (stale) {
                    drop_entry(e->second);
                    e = graphs.erase(e);
                } else {
                    ++e;
                }
            }
            while (graphs.size() >= kMaxGraphs) {
                auto lru = graphs.begin();
                for (auto e = graphs.begin(); e != graphs.end(); ++e)
                    if (e->second.last_use < lru->second.last_use) lru = e;
                drop_entry(lru->second);
                graphs.erase(lru);
            }
            it = graphs.emplace(full, GraphEntry()).first;
        }
        it->second.last_use = ++graph_clock;
        return &it->second;
    }
    static void drop_entry(GraphEntry& ge)
    {
        if (ge.exec) (void)hipGraphExecDestroy(ge.exec);
        if (ge.graph) (void)hipGraphDestroy(ge.graph);
        ge.exec = nullptr;
        ge.graph = nullptr;
    }
    // Start of the capturable part of a call.  Returns true when the caller has to run the body code (eagerly, into a
    // capture, or as a sizing pass), false when a cached graph stands in for it.
    bool body_begin()
    {
        body_mode = 0;
        if (dry() || !cur_ge) return true;
        if (cur_ge->exec) {
            body_mode = 2;
            return false;
        }
        if (cur_ge->seen < 1 || cur_ge->capture_fails >= kMaxCaptureFails) return true;  // first call / retired entry: eager
        // relaxed: other host threads (other engine instances) keep launching while this one captures; the operations
        // that must not overlap a capture are fenced off with g_capture_mu
        g_capture_mu.lock_shared();
        if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess) {
            g_capture_mu.unlock_shared();
            (void)hipGetLastError();
            return true;
        }
        body_mode = 1;
        return true;
    }
    int body_end()
    {
        const int mode = body_mode;
        body_mode = 0;
        if (dry()) return RGBD_OK;
        if (mode == 1) {
            hipGraph_t gr = nullptr;
            hipError_t e = hipStreamEndCapture(s, &gr);
            g_capture_mu.unlock_shared();
            if (g_fail_captures > 0) {  // test hook (rgbd_debug_fail_captures): this capture counts as lost
                --g_fail_captures;
                e = hipErrorStreamCaptureInvalidated;
            }
            if (e != hipSuccess || rc) {
                // Nothing of the body has run (it was being recorded, not executed): the caller re-runs the call eagerly
                // (run_sized).  A capture is lost when anything the runtime forbids during a capture happens on this
                // stream's behalf -- another library's device-wide call, an allocator trim -- not through any fault of
                // the call itself.
                if (gr) (void)hipGraphDestroy(gr);
                (void)hipGetLastError();
                capture_failed = true;
                return rc ? rc : RGBD_EHIP;
            }
            hipGraphExec_t ex = nullptr;
            if (hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0) != hipSuccess) {
                (void)hipGraphDestroy(gr);
                (void)hipGetLastError();
                capture_failed = true;
                return RGBD_EHIP;
            }
            cur_ge->graph = gr;
            cur_ge->exec = ex;
            cur_ge->named = named;
        }
        if (mode) {
            HIP_TRY(hipGraphLaunch(cur_ge->exec, s));
            if (mode == 2) named = cur_ge->named;
        }
        if (cur_ge && !rc) ++cur_ge->seen;
        return RGBD_OK;
    }
    // an error return between body_begin() and body_end() must not leave the stream capturing
    void body_abort()
    {
        if (body_mode == 1) {
            capture_failed = true;  // an error inside a capture: the eager re-run tells a lost capture from a real fault
            hipGraph_t gr = nullptr;
            (void)hipStreamEndCapture(s, &gr);
            g_capture_mu.unlock_shared();
            if (gr) (void)hipGraphDestroy(gr);
            (void)hipGetLastError();
        }
        body_mode = 0;
    }
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
    int wait_stream()
    {
        if (!blocking_wait) {
            HIP_TRY(hipStreamSynchronize(s));
            return RGBD_OK;
        }
        if (!done_ev) HIP_TRY(hipEventCreateWithFlags(&done_ev, hipEventBlockingSync | hipEventDisableTiming));
        if (capturing()) return RGBD_ESTATE;  // an event recorded inside a capture never signals: refuse by construction
        HIP_TRY(hipEventRecord(done_ev, s));
        HangWatch w("hipEventSynchronize(done_ev) in wait_stream", 30);
        HIP_TRY(hipEventSynchronize(done_ev));
        return RGBD_OK;
    }
    // pinned staging buffer of at least `bytes`; waits until the previous call's copies out of it have finished
    int pin_take(size_t bytes, void** out)
    {
        if (pin_busy) {
            HangWatch w("hipEventSynchronize(pin_ev) in pin_take", 30);
            HIP_TRY(hipEventSynchronize(pin_ev));
            pin_busy = false;
        }
        if (bytes > pin_cap) {
            std::unique_lock<std::shared_mutex> lk(g_capture_mu);
            if (pin) (void)hipHostFree(pin);
            pin = nullptr;
            pin_cap = 0;
            const size_t want = bytes + bytes / 4 + 4096;
            HIP_TRY(hipHostMalloc(&pin, want, hipHostMallocDefault));
            pin_cap = want;
        }
        *out = pin;
        return RGBD_OK;
    }
    int pin_release()
    {
        if (!pin_ev) HIP_TRY(hipEventCreateWithFlags(&pin_ev, hipEventBlockingSync | hipEventDisableTiming));
        if (capturing()) return RGBD_ESTATE;  // (see wait_stream)
        HIP_TRY(hipEventRecord(pin_ev, s));
        pin_busy = true;
        return RGBD_OK;
    }
    void fail(int code)
    {
        if (!rc) rc = code;
    }
    Act alloc(int n, int h, int w, int c)
    {
        Act a;
        a.n = n;
        a.h = h;
        a.w = w;
        a.c = c;
        a.cs = round_up(c, 16);
        a.p = (float*)arena.take(a.elems() * sizeof(float));
        return a;
    }
    // ---- two-ended workspace (Arena): the stage loop of stages() ----------------------------------------------------
    // A stage reads tensors on one end and puts its output and temporaries on the other, which is emptied first: what it
    // held -- the previous stage's input -- is dead by then.  `cur_hi`: the end the stage's input lives on.  A fusion stage
    // (its inputs ARE its outputs: the concat buffers) only puts its temporaries there.
    struct Ends {
        size_t lo_floor = 0;  // low-end fill at the transform's entry: everything below belongs to the caller
        bool cur_hi = false;
    };
    Ends ends_begin()
    {
        Ends e;
        if (arena.hi) arena.flip(arena.other);  // (never: transforms are entered on the low end)
        e.lo_floor = arena.top;
        return e;
    }
    void ends_stage(Ends& e, bool output_moves)
    {
        static const bool off = getenv("RGBD_NO_WS_REUSE") != nullptr;  // A/B switch: one-ended workspace as in rounds 1-3
        if (off) return;
        const bool want_hi = !e.cur_hi;
        if (arena.hi != want_hi) arena.flip(want_hi ? 0 : e.lo_floor);
        else arena.top = want_hi ? 0 : e.lo_floor;
        if (output_moves) e.cur_hi = want_hi;
    }
    // back on the low end; the transform's results stay protected on whichever end they are until ends_release()
    void ends_finish(Ends& e)
    {
        if (arena.hi) arena.flip(e.cur_hi ? e.lo_floor : arena.other);
    }
    void ends_release() { arena.other = 0; }

    static Act view(const Act& a, int c0, int c)
    {
        Act v = a;
        v.p = a.p + c0;
        v.c = c;
        return v;
    }
    const PackedConv* conv_of(const std::string& name)
    {
        auto it = convs.find(name);
        if (it == convs.end()) {
            fprintf(stderr, "[rgbd_amd] missing layer %s\n", name.c_str());
            fail(RGBD_ESTATE);
            return nullptr;
        }
        return &it->second;
    }
    // per-row dot-product classes of an SE_Block Linear layer (reference arithmetic; nullptr = every row "main")
    const int* cls_of(const std::string& wname)
    {
        auto it = dense.find(wname + ".rowclass");
        return (it == dense.end() || ref_batch != 1) ? nullptr : reinterpret_cast<const int*>(it->second);
    }
    // the SE Linear layers of a reference call on a batch of two vectors take MKL's n = 2 form for every row (se_linear_ref_kernel
    // form 3; measured for batch 2 only: other batch sizes keep the "main" order and make no bit-level claim)
    int se_form() const { return ref_batch == 2 ? 3 : -1; }
    float* dense_of(const std::string& name)
    {
        auto it = dense.find(name);
        if (it == dense.end()) {
            fprintf(stderr, "[rgbd_amd] missing tensor %s\n", name.c_str());
            fail(RGBD_ESTATE);
            return nullptr;
        }
        return it->second;
    }

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
                       const Act* lead_dst = nullptr)
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

    // The accumulation structure of the reference's CPU kernel for this layer (oracle/cpu_arith.c is the C
    // restatement the GPU results are compared with, bit for bit):
    //   conv, k > 1 (oneDNN jit:avx512_core)      a block per 16 input channels; (S_0 + bias) + S_1 + ...
    //   conv, 1x1   (oneDNN jit_1x1:avx512_core)  the layer shape's reduce blocks (ref_blocks); the first chain starts at the bias
    //   conv_transpose2d, stride 1                a block per 16 input channels; bias last
    // Layers with no decision behind them that have a faster special form keep it (the image-producing sub-pixel layer);
    // stride-2 transposed convs: see deconv_s2_ref().
    void plan_refnum(ConvPlan& cp, const std::string& name, const PackedConv* pc, const PackedConv* pc2, bool subpix, const Act& x,
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

    // can the two plans share a launch?  Same layer shape, strides and epilogue, operand by operand
    static bool pairable(const ConvPlan& p, const ConvPlan& q)
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

    // The profiler's event pair around one launch.  prof_begin() records the first event of the pool's next pair and hands
    // back the second (the pool grows by 256 events at a time; false: an event could not be created, the call has failed);
    // prof_end() records that one behind the launch and books the launch: name, algorithmic and executed FLOPs.
    bool prof_begin(hipEvent_t* e1)
    {
        if (ev_used + 2 > ev_pool.size()) {
            for (int i = 0; i < 256; ++i) {
                hipEvent_t e;
                if (hipEventCreate(&e) != hipSuccess) {
                    fail(RGBD_EHIP);
                    return false;
                }
                ev_pool.push_back(e);
            }
        }
        (void)hipEventRecord(ev_pool[ev_used++], s);
        *e1 = ev_pool[ev_used++];
        return true;
    }
    void prof_end(hipEvent_t e1, const std::string& name, double fl, double fx)
    {
        (void)hipEventRecord(e1, s);
        prof_flops += fl;
        prof_flops_exec += fx;
        ++prof_launches;
        ev_names.push_back({name, fl, fx});
    }

    // launch one plan, or two plans as one grouped launch (q != nullptr: the caller has checked pairable())
    void conv_issue(ConvPlan& p, ConvPlan* q = nullptr)
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

    // first analysis conv (3 / 1 -> N, k 5, stride 2): gather the 25 x C real inputs of every output pixel, then a 1x1 layer
    // with K = 80 / 32 (pack_kpack); returns false when the layer is not of that kind
    bool conv_kpacked(const std::string& name, const Act& x, int stride, int pad, const Epi& ep, const Act* dst, Act* out)
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

    // The reference's small-tensor route (torch ConvParams::use_mkldnn is false: batch 1, kernel <= 3, <= 20480 input
    // elements -> im2col + MKL sgemm): its own accumulation order, k = c -> ky -> kx in K blocks.
    bool small_tensor_layer(const std::string& name, const Act& x) const  // (x: any tensor on the layer's input grid)
    {
        if (!refnum || ref_batch != 1) return false;
        auto it = convs.find(name + ".weight");
        if (it == convs.end()) return false;
        const PackedConv& pc = it->second;
        return !pc.transposed && !pc.subpix && pc.k <= 3 && (long)pc.cin * x.h * x.w <= 20480;
    }
    Act conv_small(const std::string& name, const Act& x, int stride, int pad, const Epi& ep, const Act* dst)
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

    // torch.sigmoid on the CPU is not one function: the last len % 32 elements of every parallel chunk of the
    // tensor go through the scalar path (libm's expf instead of Sleef's vector exp).  A tensor that has such elements -- e.g.
    // the 320 x 16 x 16 attention map of a 256 x 256 image: three chunks of 27307 -- cannot take its gate in the conv epilogue,
    // which knows no flat index: the conv then writes its plain output and sigmoid_gate_ref_kernel applies a * sigmoid(b) + x.
    bool sigmoid_scalar_tails(long numel) const
    {
        long tasks = 1;
        if (numel >= 32768 && ref_threads > 1) tasks = std::min<long>(ref_threads, (numel + 32767) / 32768);
        const long chunk = (numel + tasks - 1) / tasks;
        return chunk % 32 != 0 || (numel - (tasks - 1) * chunk) % 32 != 0;
    }
    bool gate_needs_own_pass(const std::string& name, const Act& x, int stride, int pad, const Epi& ep)
    {
        if (!refnum || ep.act != ACT_SIGMOID) return false;
        auto it = convs.find(name + ".weight");
        if (it == convs.end() || it->second.transposed) return false;
        const PackedConv& pc = it->second;
        int OH, OW;
        conv_out_hw(x.h, x.w, pc.k, stride, pad, false, &OH, &OW);
        return sigmoid_scalar_tails((long)(ref_batch == 1 ? 1 : x.n) * pc.cout * OH * OW);
    }
    Act conv_gated_ref(const std::string& name, const Act& x, int stride, int pad, const Epi& ep, const Act* dst)
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

    Act conv(const std::string& name, const Act& x, int stride, int pad, Epi ep = Epi(), const Act* dst = nullptr,
             const std::string* fuse1x1 = nullptr, const std::string* lead1x1 = nullptr, const Act* lead_dst = nullptr)
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

    // Keep the taps of a (one-phase) tap table whose dy + dx has parity `odd`, in their order; the rest of the table is
    // zeroed.  Returns the number kept.
    static int keep_taps(TapTable& t, int odd)
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

    // A stride-1 k x k conv whose INPUT is non-zero at the anchor positions only ((row + col) odd: the slice right after its
    // anchor pass, utils/ckbd.py:37-48 -- what the local-context convs read, elic_united.py:296,309).  An output pixel of
    // parity q then only meets non-zero inputs under the taps with (dy + dx) & 1 == 1 - q: the anchor outputs need the 13
    // taps with dy + dx even, the other outputs the 12 with dy + dx odd.  Two checkerboard-output launches (ConvArgs::ckbd
    // 1 / 2), each with its half of the tap table: half the MFMA work, and every output keeps its fma chain minus terms
    // that are exact zeros (round 4; RGBD_NO_ANCHOR_TAPS=1 runs the full conv).  Worth it for the 192-channel slice only
    // (368 -> 255 us at c3); at 64 channels two launches cost more than the taps they save (71 -> 86 us).
    void conv_anchor_in(const std::string& name, const Act& x, int pad, const Act& dst)
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

    // The same layer kind for nm modalities (names n[0] / n[1]: RGB / depth branch).  nm == 2: one grouped launch when the
    // two plans agree in every shape, otherwise (first / last image-facing layers: 3 vs 1 channels) two launches.
    // nm == 1: conv() of entry 0.  Every array argument is read at [0, nm) only.
    void conv2(int nm, const std::string n[2], const Act x[2], int stride, int pad, const Epi ep[2], const Act* const dst[2],
               Act out[2], const std::string* const fuse1x1[2] = nullptr, const std::string* const lead1x1[2] = nullptr,
               const Act* const lead_dst[2] = nullptr)
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

    // drain recorded event pairs into prof_ms (call after the stream has been synchronised)
    void profile_collect()
    {
        for (size_t i = 0; i + 1 < ev_used; i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev_pool[i], ev_pool[i + 1]) == hipSuccess) {
                prof_ms += ms;
                if (i / 2 < ev_names.size()) {
                    auto& acc = prof_layers[ev_names[i / 2].first];
                    acc.first += ms;
                    acc.second += ev_names[i / 2].second;
                    acc.exec += ev_names[i / 2].exec;
                    ++prof_counts[ev_names[i / 2].first];
                }
            }
        }
        ev_used = 0;
        ev_names.clear();
    }

    void copy_ch(const Act& src, const Act& dst)
    {
        if (dry() || rc) return;
        const int r = launch_copy_channels(src.p, src.cs, dst.p, dst.cs, src.n * src.h * src.w, round_up(src.c, 4), s);
        if (r) fail(r);
    }

    // the pair (mid: 3x3 + ReLU, last: 1x1 + residual) as one launch?  (a speed decision: the results are bit-identical)
    bool fusable(const std::string& mid, const std::string& last, const Act& x, int groups = 1)
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

    // ... and can the leading 1x1 + ReLU of the block after it ride along?  (its input is this block's output)
    bool lead_fusable(const std::string& last, const std::string& lead, const Act& x)
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
    // outputs of leading layers that a previous block's launch has already produced, by layer name
    std::map<std::string, Act> pre_leads;

    // ---- blocks of nm modalities (p[0] / p[1]: the RGB / depth branch's layer names; arrays are read at [0, nm)) --------
    // With nm == 2 every layer pair is one grouped launch (conv2) and the fusion decisions are taken for the pair: a grouped
    // launch tiles like the layer at twice the batch.  nm == 1 is the block of one branch.
    void take_lead2(int nm, const std::string n[2], const Act x[2], Act t[2])
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

    // modules/layers/res_blk.py:7-27.  next_lead[m]: the leading layer of the block that consumes this block's output
    // ("" = none)
    void bottleneck2(int nm, const std::string p[2], const Act x[2], const Act* const dst[2], const std::string next_lead[2],
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

    // CompressAI/compressai/layers/layers.py:177-196
    void res_unit2(int nm, const std::string p[2], const Act x[2], const std::string next_lead[2], Act out[2])
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

    // layers.py:198-213
    void attention2(int nm, const std::string p[2], const Act x[2], const Act* const dst[2], Act out[2])
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

    // modules/transform/attention.py:84-97: x[m] -> dst[m] = x[m] * sigmoid(...) (+ add[m]: STF_united adds the gated
    // features to the stream instead of concatenating them; add may be nullptr)
    void esa2(int nm, const std::string p[2], const Act x[2], const Act dst[2], const Act* const add[2])
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

    // modules/transform/attention.py:35-48; rgb/depth: views of N channels; writes the gated features into
    // r_dst / d_dst (N channels each)
    void bi_spf(const std::string& p, const Act& rgb, const Act& depth, const Act& r_dst, const Act& d_dst,
                bool residual = false)
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

    // modules/transform/attention.py:63-67: y = x * g (mode 0) or x + x * g (mode 1), g = the per-(n,c) sigmoid weights of x
    // means / mstride: the channel means of x when somebody holds them already (Bi-CEE: SliceMeans), else they are computed.
    void se_scale_to(const std::string& p, const Act& x, int mode, const Act& y, const float* means = nullptr, int mstride = 0)
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

    // the SE of cat(own, other) written into the two halves of f (synthesis.py:345-362): means side by side, one gate
    void se_cat_to(const std::string& p, const Act& own, const Act& other, const Act& f)
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
    void stages(const Stages& sd, const Act in[2], Act out[2])
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
    // ELIC_united: analysis.py:116-174 / synthesis.py:126-184
    void g_a(const Act x[2], Act y[2])
    {
        const Stages sd = {kAna18, 18, 2, {"g_a.rgb_analysis_transform.", "g_a.depth_analysis_transform."},
                           kBiSpf, true, true, true};
        stages(sd, x, y);
    }
    void g_s(const Act yhat[2], Act xhat[2])
    {
        const Stages sd = {kSyn18, 18, 2, {"g_s.rgb_synthesis_transform.", "g_s.depth_synthesis_transform."},
                           kBiSpf, true, true, true};
        stages(sd, yhat, xhat);
    }

    // analysis.py:231-242
    void h_a(const Act& yr, const Act& yd, Act* zr, Act* zd)
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

    // conv_transpose2d(k 5, stride 2, pad 2, output_padding 1) + activation in the reference's CPU arithmetic: the layer's
    // measured recipe (refarith_tables.json kind 3) run by deconv_s2_ref_run(), scratch from the arena.
    // false = no recipe for this shape (the caller runs the sub-pixel-phase kernel).
    bool deconv_s2_ref(const std::string& name, const Act& x, int act, Act* out)
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

    // synthesis.py:345-362.  cat(own, other) -> SE -> deconv without materialising the unscaled concatenation: the channel
    // means of the two inputs land side by side (what the mean of the concatenation would be, channel by channel), the
    // gate is computed from them, and each input is scaled straight into its half of the deconv's input buffer.  The SE
    // gates stay per modality; with nm == 2 the two (transposed) convs are one grouped launch.
    void hs_block2(int nm, const std::string p[2], const Act own[2], const Act other[2], bool last, Act out[2])
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

    // synthesis.py:316-323
    void h_s(const Act& zr, const Act& zd, Act* hr, Act* hd)
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
    const SliceLoop& slice_loop_family() const
    {
        return family == Family::ELIC ? kLoopSingle : family == Family::ELIC_united_R2D ? kLoopR2D : kLoopUnited;
    }

    // The parameter net of one part: [SE rescale,] three convs (1x1 / 3x3 / 5x5 or 1x1 x 3; padding k / 2) with ReLU between.
    // SE writes the rescaled copy the first conv reads (params + se(params), keeping the reference's association); `means`:
    // the input's channel means where the caller has them already.  `part` (1 anchor / 2 non-anchor): the caller only reads
    // that checkerboard half of (scales, means) (ckbd.py:83-125), so the last -- and largest -- conv computes just that half,
    // and so do the layers in front of it where none mixes positions; the values are those of the full convs.
    Act entropy_params(const SliceLoop& d, const std::string& p, const Act& ctx, int part, const Act* dst = nullptr,
                       const float* means = nullptr, int mstride = 0)
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

    // context.py:10-30 (slice i's two nets read only what earlier slices decoded: independent)
    void channel_context2(int nm, const std::string p[2], const Act x[2], const Act dst[2])
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

    float* yhat_base[2] = {nullptr, nullptr};

    // y, hyp, yhat: read at [0, nm); y is null when decoding
    void slice_loop_ckbd(Coding& cd, const SliceLoop& d, int nm, const Act* y, const Act hyp[2], const Act yhat[2])
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

    // ---- STF_united (models/stf_united.py; BASELINE config 5): Swin transforms on [B,H,W,C] token maps -------------
    Act layernorm(const std::string& p, const Act& x)
    {
        Act y = alloc(x.n, x.h, x.w, x.c);
        float* w = dense_of(p + ".weight");
        float* b = dense_of(p + ".bias");
        if (dry() || rc || !w || !b) return y;
        const int r = launch_layernorm(x.p, (size_t)x.n * x.h * x.w, x.c, x.cs, w, b, y.p, y.cs, s);
        if (r) fail(r);
        return y;
    }
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
    void layernorm2(int nm, const std::string p[2], const Act x[2], Act y[2])
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
    // the Swin block after its attention: x + attn.proj(a), then + mlp(norm2(.)) into out (allocated by the caller, before
    // its arena mark); allocates x1, t2 and the hidden layer, in that order
    void swin_block_tail2(int nm, const std::string p[2], const Act x[2], const Act a[2], const Act out[2])
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
    void swin_block2(int nm, const std::string p[2], const Act x[2], int shift, int heads, Act out[2])
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
    // Spatial_aligner (modules/transform/spatialAligner.py:341-390): patch embeddings of x and guided, two Swin blocks whose
    // attention reads q from x and k, v from guided (:279-338; norm1 on both, guided itself never updated: :290-291, 383-384),
    // and the 2x2 stride-2 transposed convolution `recovery`, whose taps do not overlap: a 1x1 convolution to 4 * out channels
    // (repacked in finalize) and a pixel shuffle.  prefix: "" (the stand-alone variant) or the block's name, e.g. "g_s.sp1".
    Act spatial_aligner(const std::string& prefix, const Act& x, const Act& guided)
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
    // ---- the attention contexts of MLIC++ (modules/transform/context.py), each a block of its own (families 7-9) -------
    // nn.Conv2d(C, C, 3, 1, 1, groups = C) (+ nn.GELU()): weight [C][1][3][3] and bias as plain arrays (finalize)
    Act dwconv(const std::string& name, const Act& x, bool gelu)
    {
        const Act y = alloc(x.n, x.h, x.w, x.c);
        float* w = dense_of(name + ".weight");
        float* b = dense_of(name + ".bias");
        if (dry() || rc || !w || !b) return y;
        const int r = launch_dwconv3x3(x.p, x.n, x.h, x.w, x.c, x.cs, w, b, gelu ? 1 : 0, y.p, y.cs, s);
        if (r) fail(r);
        return y;
    }
    // LocalContext.forward (:82-137): norm1, qkv_proj, the 5x5 window attention with `fusion` (one launch), proj, and
    // x + mlp(norm2(x)); the Linear layers are 1x1 convolutions, GELU and the add their epilogues
    Act local_context(const Act& x)
    {
        const Act t = layernorm("norm1", x);
        const Act qkv = conv("qkv_proj", t, 1, 0);
        const Act a = alloc(x.n, x.h, x.w, 2 * x.c);
        float* tab = dense_of("relative_position_table");
        float* fw = dense_of("fusion.weight");
        float* fb = dense_of("fusion.bias");
        if (!dry() && !rc && tab && fw && fb) {
            const int r = launch_local_ckbd_attention(qkv.p, qkv.cs, x.n, x.h, x.w, x.c, ctx_heads, tab, fw, fb, a.p, a.cs, s);
            if (r) fail(r);
        }
        const Act x1 = conv("proj", a, 1, 0);
        const Act t2 = layernorm("norm2", x1);
        Epi g;
        g.act = ACT_GELU;
        const Act hdn = conv("mlp.fc1", t2, 1, 0, g);
        Epi e;
        e.res1 = &x1;
        return conv("mlp.fc2", hdn, 1, 0, e);
    }
    // LinearGlobalInterContext.forward (:243-262; xk = xq = xv = x1, mode 0, with `skip`) and LinearGlobalIntraContext.forward
    // (:189-213; xk = anchor half of x1, xq = the other half, xv = x2, mode 1, no `skip`): three 1x1 + depthwise branches, the
    // linear attention, the 5x5 reprojection, and skip(a) (or a) + mlp(a)
    Act linear_context(const Act& xk, const Act& xq, const Act& xv, int mode, bool skip)
    {
        const Act k = dwconv("keys.1", conv("keys.0", xk, 1, 0), false);
        const Act q = dwconv("queries.1", conv("queries.0", xq, 1, 0), false);
        const Act v = dwconv("values.1", conv("values.0", xv, 1, 0), false);
        const Act a = alloc(k.n, k.h, k.w, k.c);
        const int hd = k.c / ctx_heads;
        const int64_t wsf = linear_attention_ws_floats(k.n, k.h, k.w, ctx_heads, hd, mode);
        if (wsf <= 0) {
            fail(RGBD_EINVAL);
            return a;
        }
        float* ws = (float*)arena.take((size_t)wsf * sizeof(float));
        if (!dry() && !rc) {
            const int r = launch_linear_attention(k.p, k.cs, q.p, q.cs, v.p, v.cs, k.n, k.h, k.w, ctx_heads, hd, mode, a.p, a.cs, ws,
                                                  wsf, s);
            if (r) fail(r);
        }
        const Act att = conv("reprojection", a, 1, 2);
        Epi g;
        g.act = ACT_GELU;
        const Act h1 = conv("mlp.0", att, 1, 0, g);
        const Act h2 = dwconv("mlp.2", h1, true);
        const Act sk = skip ? conv("skip", att, 1, 0) : att;
        Epi e;
        e.res1 = &sk;
        return conv("mlp.4", h2, 1, 0, e);
    }
    // stf_united.py:270-366 for both modalities; down: 0 none, 1 PatchMerging (:217-249), 2 PatchSplit (:252-267)
    void basic_layer2(int nm, const std::string p[2], const Act x_in[2], int depth, int heads, int down, Act out[2])
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
    void stf_stack(const std::string& root, const char* kind, const Act& r_in, const Act& d_in, const int* depths,
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
    void g_a_stf(const Act& rgb, const Act& depth, Act* y_r, Act* y_d)
    {
        static const int depths[4] = {2, 2, 6, 2}, heads[4] = {3, 6, 12, 24};
        Act r = layernorm("g_a.rgb_patch_embed.norm", conv("g_a.rgb_patch_embed.proj", rgb, 2, 0));
        Act d = layernorm("g_a.depth_patch_embed.norm", conv("g_a.depth_patch_embed.proj", depth, 2, 0));
        stf_stack("g_a", "ana", r, d, depths, heads, 1, y_r, y_d);
    }
    void g_s_stf(const Act& yr, const Act& yd, Act* xr, Act* xd)
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

    // ---- ELIC_united_R2D (models/elic_united_R2D.py): RGB on its own, depth conditioned on RGB ------
    // attention.py:14-32: only the depth-side gated features exist
    void bi_spf_single(const std::string& p, const Act& rgb, const Act& depth, const Act& d_dst)
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
    // analysis.py:56-112 / synthesis.py:186-242: the same 18 stages as ELIC_united, one branch after the other; the fusion
    // stage only widens depth
    void g_a_r2d(const Act x[2], Act y[2])
    {
        const Stages sd = {kAna18, 18, 2, {"g_a.rgb_analysis_transform.", "g_a.depth_analysis_transform."},
                           kBiSpfDepth, false, false, false};
        stages(sd, x, y);
    }
    void g_s_r2d(const Act yhat[2], Act xhat[2])
    {
        const Stages sd = {kSyn18, 18, 2, {"g_s.rgb_synthesis_transform.", "g_s.depth_synthesis_transform."},
                           kBiSpfDepth, false, false, false};
        stages(sd, yhat, xhat);
    }
    // synthesis.py:364-380
    Act hs_block_single(const std::string& p, const Act& x, bool last)
    {
        Act f = alloc(x.n, x.h, x.w, x.c);
        se_scale_to(p + ".se", x, 0, f);
        Epi e;
        e.act = last ? ACT_NONE : ACT_LEAKY;
        Act o;
        if (!last && deconv_s2_ref(p + ".deconv", f, ACT_LEAKY, &o)) return o;
        return conv(p + ".deconv", f, last ? 1 : 2, last ? 1 : 2, e);
    }
    // synthesis.py:336-343
    void h_s_r2d(const Act& zr, const Act& zd, Act* hr, Act* hd)
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
    // ---- single-modal ELIC (models/elic.py:15-57; BASELINE config 1) ------------------------------------------
    // analysis.py:29-52 / synthesis.py:32-70: the same blocks as above without the cross-modal fusion stages
    Act g_a1(const Act& x)
    {
        Act y[2];
        stages({kAna15, 15, 1, {"g_a.analysis_transform.", ""}, kNoFusion, false, false, false}, &x, y);
        return y[0];
    }
    Act g_s1(const Act& yhat)
    {
        Act xhat[2];
        stages({kSyn15, 15, 1, {"g_s.synthesis_transform.", ""}, kNoFusion, false, false, false, mid_dst}, &yhat, xhat);
        return xhat[0];
    }
    const Act* mid_dst = nullptr;  // set around g_s_family by a return_mid call (run_forward / run_decompress)
    // analysis.py:207-216
    Act h_a1(const Act& y)
    {
        Epi relu;
        relu.act = ACT_RELU;
        Act t = conv("h_a.reduction.0", y, 1, 1, relu);
        t = conv("h_a.reduction.2", t, 2, 2, relu);
        return conv("h_a.reduction.4", t, 2, 2);
    }
    // synthesis.py:276-285
    Act h_s1(const Act& zhat, const Act* dst = nullptr)
    {
        Epi relu;
        relu.act = ACT_RELU;
        Act t = conv("h_s.increase.0", zhat, 2, 2, relu);
        t = conv("h_s.increase.2", t, 2, 2, relu);
        return conv("h_s.increase.4", t, 1, 1, Epi(), dst);
    }
    // ---- single-modal STF (models/stf.py:408-816): the Swin transforms without the cross-modal fusion, and the channel-slice
    // entropy model: 12 raster slices of 32 channels, two hyper-synthesis nets, per slice two parameter nets and latent
    // residual prediction (LRP) -------------------------------------------------------------------------------------
    static constexpr int kStfSlices = 12, kStfSliceCh = 32, kStfSupport = 6;  // num_slices, M / num_slices, max_support_slices
    Act swin_stack1(const std::string& root, const Act& x_in, const int* depths, const int* heads, int down)
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
    // stf.py:704-713
    Act g_a_stf1(const Act& img)
    {
        static const int depths[4] = {2, 2, 6, 2}, heads[4] = {3, 6, 12, 24};
        return swin_stack1("layers", layernorm("patch_embed.norm", conv("patch_embed.proj", img, 2, 0)), depths, heads, 1);
    }
    // stf.py:809-815 (end_conv: 5x5 conv, PixelShuffle(2), 3x3 conv)
    Act g_s_stf1(const Act& yhat)
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
    // stf.py:507-517: five 3x3 convolutions (the third and the fifth with stride 2), GELU between them
    Act h_a_stf1(const Act& y)
    {
        static const int strides[5] = {1, 1, 2, 1, 2};
        Epi gelu;
        gelu.act = ACT_GELU;
        Act t = y;
        for (int k = 0; k < 5; ++k) t = conv("h_a." + std::to_string(2 * k), t, strides[k], 1, k < 4 ? gelu : Epi());
        return t;
    }
    // stf.py:519-540: h_mean_s and h_scale_s have the same layer shapes on the same input: ONE grouped launch per layer.
    // subpel_conv3x3 = 3x3 conv to 4 C channels + PixelShuffle(2); the GELU behind it is pointwise, so it rides in the conv's
    // epilogue.  The last layers write the first 384 channels of the two context buffers.
    void h_s_stf1(const Act& zhat, const Act& means_dst, const Act& scales_dst)
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

    ScaleTab scale_tab{};  // host copy of the Gaussian scale table: the slice kernels take it by value

    // one slice through the coder's side of the loop: symbols / indexes (encode), indexes + rANS + dequantise (decode) or
    // quantise + likelihood (forward); the pre-LRP y_hat lands in `slot`
    void code_slice(Coding& cd, int i, const Act& mu, const Act& sg, const Act& y_slice, const Act& slot)
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

    // stf.py:735-758 / 786-807 / 647-667.  ctxm = [latent_means 384 | 7 x 32], ctxs = [latent_scales 384 | 6 x 32 (+ 32 unused:
    // the two buffers share one channel stride so that the nets' first layers pair)]: slice i's pre-LRP y_hat goes to slot
    // min(i, 6) of ctxm, the LRP net reads the prefix up to and including that slot, the LRP update finalises slots 0..5 in
    // both buffers and slice i of yhat; the parameter nets of slice i read the prefix of min(i, 6) slots.  No concatenation.
    void slice_loop(Coding& cd, const Act* y, const Act& ctxm, const Act& ctxs, const Act& yhat)
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

    // ---- checkerboard Cheng2020 (models/Cheng2020withCKBD.py:40-174 on compressai/models/waseda.py:22-81): residual blocks of
    // 3x3 / 1x1 convolutions with GDN / IGDN, sub-pixel up-sampling, and a two-pass checkerboard entropy model on one slice of
    // M = N channels ----------------------------------------------------------------------------------------------------
    // GDN / IGDN (layers/gdn.py:52-67) + the block's `out += identity` (layers.py:97,125) as one launch (gdn.hip).  In the
    // profile it counts as the 1x1 convolution it contains (2 C^2 FLOPs per pixel).
    Act gdn(const std::string& name, const Act& x, bool inverse, const Act* res)
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
    Act pixel_shuffle(const Act& t)
    {
        Act u = alloc(t.n, 2 * t.h, 2 * t.w, t.c / 4);
        if (!dry() && !rc) {
            const int q = launch_pixel_shuffle2(t.p, t.n, t.h, t.w, t.c / 4, t.cs, u.p, u.cs, s);
            if (q) fail(q);
        }
        return u;
    }
    // layers.py:129-159: leaky(conv2(leaky(conv1 x))) + x
    Act ck_res_block(const std::string& p, const Act& x)
    {
        Epi e1, e2;
        e1.act = e2.act = ACT_LEAKY;
        e2.res2 = &x;
        return conv(p + ".conv2", conv(p + ".conv1", x, 1, 1, e1), 1, 1, e2);
    }
    // layers.py:67-98: GDN(conv2(leaky(conv1 x, stride 2))) + skip(x) (1x1, stride 2)
    Act ck_res_block_stride(const std::string& p, const Act& x)
    {
        Epi leaky;
        leaky.act = ACT_LEAKY;
        const Act t = conv(p + ".conv2", conv(p + ".conv1", x, 2, 1, leaky), 1, 1);
        const Act id = conv(p + ".skip", x, 2, 0);
        return gdn(p + ".gdn", t, false, &id);
    }
    // layers.py:101-126: IGDN(conv(leaky(subpel_conv x))) + upsample(x); the two sub-pixel convs read the same tensor with
    // the same layer shape: one grouped launch.  LeakyReLU is pointwise, so it rides in front of the shuffle.
    Act ck_res_block_up(const std::string& p, const Act& x)
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
    // waseda.py:38-46.  Every stage's temporaries are released once its output has been copied down.
    Act ck_stage(const Act& x, const std::function<Act(const Act&)>& f, int oh, int ow, int oc)
    {
        Act out = alloc(x.n, oh, ow, oc);
        const size_t mark = arena.top;
        copy_ch(f(x), out);
        arena.top = mark;
        return out;
    }
    Act g_a_ckbd(const Act& img)
    {
        Act x = img;
        for (int i = 0; i < 3; ++i) {
            const std::string a = "g_a." + std::to_string(2 * i), b = "g_a." + std::to_string(2 * i + 1);
            x = ck_stage(x, [&](const Act& t) { return ck_res_block(b, ck_res_block_stride(a, t)); }, x.h / 2, x.w / 2, N);
        }
        return conv("g_a.6", x, 2, 1);
    }
    // waseda.py:72-81
    Act g_s_ckbd(const Act& yhat)
    {
        Act x = yhat;
        for (int i = 0; i < 3; ++i) {
            const std::string a = "g_s." + std::to_string(2 * i), b = "g_s." + std::to_string(2 * i + 1);
            x = ck_stage(x, [&](const Act& t) { return ck_res_block_up(b, ck_res_block(a, t)); }, 2 * x.h, 2 * x.w, N);
        }
        return pixel_shuffle(conv("g_s.7.0", ck_res_block("g_s.6", x), 1, 1));
    }
    // waseda.py:48-58
    Act h_a_ckbd(const Act& y)
    {
        static const int strides[5] = {1, 1, 2, 1, 2};
        Epi leaky;
        leaky.act = ACT_LEAKY;
        Act t = y;
        for (int k = 0; k < 5; ++k) t = conv("h_a." + std::to_string(2 * k), t, strides[k], 1, k < 4 ? leaky : Epi());
        return t;
    }
    // waseda.py:60-70; the last layer writes the hyper half of the entropy-parameter input [ctx 2M | hyper 2M]
    void h_s_ckbd(const Act& zhat, const Act& dst)
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
    // priors.py:403-409: three 1x1 convolutions.  part 1 (anchor, Cheng2020withCKBD.py:122-124): the context half of the
    // input is zero, so the first layer runs on the hyper half of its input channels only ("entropy_parameters.0.hyper": the
    // same chain without terms that are exact zeros); 1x1 layers do not mix positions, so each pass computes and stores its
    // own checkerboard half of `out` (part 0: the whole grid, forward()).
    void ck_entropy_params(const Act& cat, int part, const Act& out)
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
    // CheckerboardContext (Cheng2020withCKBD.py:12-37): the weight is masked when packed; only the 12 taps with (ky + kx) odd
    // are issued and only the non-anchor outputs computed (the anchor half of dst is left as it is: zeros)
    void ck_context(const Act& yhat, const Act& dst)
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
    // Cheng2020withCKBD.py:121-130 / 154-167: cat = [ctx 2M | hyper 2M] with the context half zeroed and the hyper half filled;
    // params = [scales M | means M]: the anchor pass leaves its half there, the non-anchor pass the other half
    void two_pass_ckbd(Coding& cd, const Act* y, const Act& cat, const Act& params, const Act& yhat)
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
    int run_forward(int nm, In2 x_dev, int B, int H, int W, Out2 xhat_dev, Out2 ly, Out2 lz, const Mid3* up = nullptr);
    int run_decompress(int nm, const uint8_t* const* ys[2], const int64_t* ylen[2], int n_y, const uint8_t* const* zs[2],
                       const int64_t* zlen[2], int B, int h, int w, Out2 xhat_dev, const Latents* lat = nullptr,
                       const Mid3* up = nullptr);
    void mids_begin(int B, int H, int W, Act mid[3]);  // workspace of up1..up3; g_s1 fills it while mid_dst points at it
    int mids_out(const Act mid[3], int B, int H, int W, const Mid3& up);
    int run_aligner(const float* x_dev, const float* guided_dev, int B, int H, int W, float* out_dev);
    // SynthesisTransformPlus: yhat [B,M,h,w], up[k] [B,N,2h << k,2w << k] -> out [B,out_ch,16h,16w]
    bool plus_guides = true;  // rgbd_debug_synthesis_plus_guides(m, 0): the same walk without the three aligners (a timing aid)
    int run_synthesis_plus(const float* yhat_dev, const float* const up_dev[3], int B, int h, int w, float* out_dev);
    // the contexts: x1 (and, LinearGlobalIntraContext, x2) [B,in_ch,H,W] -> out [B,out_ch,H,W]
    int run_context(const float* x1_dev, const float* x2_dev, int B, int H, int W, float* out_dev);
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

