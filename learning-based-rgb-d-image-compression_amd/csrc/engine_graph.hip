// Host runtime of the gfx950 codec engine: what a call runs on (declared in engine.h) -- the hang diagnostics (HangWatch),
// the engine's stream, the per-call-shape HIP-graph cache (graph_entry, body_begin / body_end / body_abort), the waits and
// the pinned staging buffer, error and workspace helpers (fail, alloc, the two-ended stage loop's ends_*) and the conv
// profiler's event pairs.
#include <chrono>
#include <dirent.h>
#include <execinfo.h>
#include <signal.h>
#include <sys/syscall.h>

#include "engine.h"

namespace rgbd_rt {

void bt_handler(int)
{
    void* fr[64];
    const int n = backtrace(fr, 64);
    char hdr[64];
    const int l = snprintf(hdr, sizeof(hdr), "[bt tid %ld]\n", (long)syscall(SYS_gettid));
    if (l > 0) (void)!write(2, hdr, (size_t)l);
    backtrace_symbols_fd(fr, n, 2);
}

HangWatch::HangWatch(const char* what, int secs, bool always)
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

HangWatch::~HangWatch()
{
    if (!th.joinable()) return;
    {
        std::lock_guard<std::mutex> lk(mu);
        done = true;
    }
    cv.notify_all();
    th.join();
}

}  // namespace rgbd_rt

int rgbd_elic::use_stream(void* stream)
{
    s = (hipStream_t)stream;
    if (g_dbg_destroy) {
        std::lock_guard<std::mutex> g(g_live_mu);
        g_live_streams[this] = s;
    }
    return RGBD_OK;
}

void rgbd_elic::graphs_invalidate()
{
    for (auto& kv : graphs) drop_entry(kv.second);
    graphs.clear();
    cur_ge = nullptr;
}

rgbd_elic::GraphEntry* rgbd_elic::graph_entry(const std::string& key)
{
    if (!use_graphs || profile || profile_phases || !s) return nullptr;  // (the NULL stream cannot be captured)
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

void rgbd_elic::drop_entry(GraphEntry& ge)
{
    if (ge.exec) (void)hipGraphExecDestroy(ge.exec);
    if (ge.graph) (void)hipGraphDestroy(ge.graph);
    ge.exec = nullptr;
    ge.graph = nullptr;
}

bool rgbd_elic::body_begin()
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

int rgbd_elic::body_end()
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

void rgbd_elic::body_abort()
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

int rgbd_elic::wait_stream()
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

int rgbd_elic::pin_take(size_t bytes, void** out)
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

int rgbd_elic::pin_release()
{
    if (!pin_ev) HIP_TRY(hipEventCreateWithFlags(&pin_ev, hipEventBlockingSync | hipEventDisableTiming));
    if (capturing()) return RGBD_ESTATE;  // (see wait_stream)
    HIP_TRY(hipEventRecord(pin_ev, s));
    pin_busy = true;
    return RGBD_OK;
}

void rgbd_elic::fail(int code)
{
    if (!rc) rc = code;
}

Act rgbd_elic::alloc(int n, int h, int w, int c)
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

rgbd_elic::Ends rgbd_elic::ends_begin()
{
    Ends e;
    if (arena.hi) arena.flip(arena.other);  // (never: transforms are entered on the low end)
    e.lo_floor = arena.top;
    return e;
}

void rgbd_elic::ends_stage(Ends& e, bool output_moves)
{
    static const bool off = getenv("RGBD_NO_WS_REUSE") != nullptr;  // A/B switch: one-ended workspace as in rounds 1-3
    if (off) return;
    const bool want_hi = !e.cur_hi;
    if (arena.hi != want_hi) arena.flip(want_hi ? 0 : e.lo_floor);
    else arena.top = want_hi ? 0 : e.lo_floor;
    if (output_moves) e.cur_hi = want_hi;
}

void rgbd_elic::ends_finish(Ends& e)
{
    if (arena.hi) arena.flip(e.cur_hi ? e.lo_floor : arena.other);
}

bool rgbd_elic::prof_begin(hipEvent_t* e1)
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

void rgbd_elic::prof_end(hipEvent_t e1, const std::string& name, double fl, double fx)
{
    (void)hipEventRecord(e1, s);
    prof_flops += fl;
    prof_flops_exec += fx;
    ++prof_launches;
    ev_names.push_back({name, fl, fx});
}

void rgbd_elic::profile_collect()
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
