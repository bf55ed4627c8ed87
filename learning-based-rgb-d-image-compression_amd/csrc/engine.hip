// Host runtime of the gfx950 codec engine: the call paths -- compress(), decompress() and the eval forward, once
// for every family of one or two modalities -- as sequences of kernel launches through the layer graphs that engine.h declares
// and engine_elic.hip, engine_swin.hip and engine_ckbd.hip define; the four `*_family` hooks choose among them
// (prologue: workspace of the call and stream geometry; body: captured into / replayed from a HIP graph; epilogue: fetch
// the finished streams).  Mirrors the call structure of the reference's models/elic_united.py:350-578 but keeps every
// tensor, symbol, index and bitstream resident in HBM; the only device->host traffic is the finished streams.
#include "engine.h"

std::shared_mutex g_capture_mu;
int64_t rgbd_enc_cap_words(int64_t n) { return ((5 * n + 32 + 704) + 63) & ~(int64_t)63; }

int rgbd_elic::ensure_arena(size_t bytes)
{
    if (bytes <= arena.cap) return RGBD_OK;
    graphs_invalidate();  // cached graphs have the old workspace addresses baked in
    dbg_sym = dbg_idx = nullptr;  // (they point into the workspace that is about to go)
    dbg_x = dbg_s = nullptr;
    std::unique_lock<std::shared_mutex> lk(g_capture_mu);  // hipFree synchronises the device: not while anyone captures
    if (arena.base) {
        HangWatch w("hipStreamSynchronize / hipFree in ensure_arena", 30);
        HIP_TRY(hipStreamSynchronize(s));  // only this instance's stream ever touches this workspace
        HIP_TRY(hipFree(arena.base));
        arena.base = nullptr;
        arena.cap = 0;
    }
    bytes += bytes / 16;
    bytes = (bytes + 255) & ~(size_t)255;  // (the high end of the two-ended stack allocates down from base + cap)
    HIP_TRY(hipMalloc((void**)&arena.base, bytes));
    arena.cap = bytes;

    return RGBD_OK;
}

// ---- stream I/O, for nm = 1 or 2 modalities ------------------------------------------------------------------------------
// workspace of a compress call (symbols, indexes, stream slots, error flag, debug copies) and the upload of its stream
// geometry (EncBufs::meta)
int rgbd_elic::enc_streams(int nm, int B, int64_t T, int64_t Tz, int per_image, EncBufs* e)
{
    const int ny = per_image ? B : 1;
    const int64_t ycount = per_image ? T : T * B;
    const size_t nmeta = (size_t)(8 + 3 * nm) * B + 64;
    e->ny = ny;
    e->ycap = y_cap_words(ycount);
    e->ycount = ycount;
    e->zcap = rgbd_enc_cap_words(Tz);
    e->meta = (int64_t*)arena.take(sizeof(int64_t) * nmeta);
    e->sym = (int32_t*)arena.take(sizeof(int32_t) * (size_t)(nm * B * T));
    e->idx = (int32_t*)arena.take(sizeof(int32_t) * (size_t)(nm * B * T));
    e->zsym = (int32_t*)arena.take(sizeof(int32_t) * (size_t)(nm * B * Tz));
    e->zidx = (int32_t*)arena.take(sizeof(int32_t) * (size_t)(nm * B * Tz));
    e->ywords = (uint32_t*)arena.take(sizeof(uint32_t) * (size_t)(nm * ny * e->ycap));
    e->zwords = (uint32_t*)arena.take(sizeof(uint32_t) * (size_t)(nm * B * e->zcap));
    e->err = (int*)arena.take(256);
    dbg_sym = e->sym;
    dbg_idx = e->idx;
    dbg_per_mod = (int64_t)B * T;
    dbg_x = dbg_s = nullptr;
    if (debug_floats) {
        dbg_x = (float*)arena.take(sizeof(float) * (size_t)(nm * B * T));
        dbg_s = (float*)arena.take(sizeof(float) * (size_t)(nm * B * T));
    }
    if (dry()) return RGBD_OK;
    void* pv = nullptr;
    if (const int r = pin_take(nmeta * sizeof(int64_t), &pv)) return r;
    int64_t* hmeta = (int64_t*)pv;
    memset(hmeta, 0, nmeta * sizeof(int64_t));
    for (int b = 0; b < B; ++b) {
        hmeta[b] = per_image ? (int64_t)b * T : 0;
        hmeta[2 * B + b] = (int64_t)b * Tz;
        hmeta[3 * B + b] = Tz;
    }
    for (int m = 0; m < nm; ++m)
        for (int i = 0; i < ny; ++i) {
            hmeta[(size_t)8 * B + (size_t)m * ny + i] = (int64_t)m * B * T + (per_image ? (int64_t)i * T : 0);
            hmeta[(size_t)8 * B + (size_t)nm * ny + (size_t)m * ny + i] = ycount;
        }
    HIP_TRY(hipMemcpyAsync(e->meta, hmeta, sizeof(int64_t) * nmeta, hipMemcpyHostToDevice, s));
    return pin_release();
}

// epilogue of a compress call: the finished streams into streams[m][0] (y) and streams[m][1] (z; with_z)
int rgbd_elic::fetch_streams(int nm, int B, bool with_z, const EncBufs& e)
{
    // stream sizes come back through a small pinned buffer: a device-to-host copy into pageable memory is synchronous in
    // HIP, i.e. the host thread would spin inside it for the whole call; with pinned memory the thread sleeps on an event
    if (!res_pin) HIP_TRY(hipHostMalloc((void**)&res_pin, kResPinBytes, hipHostMallocDefault));
    if ((size_t)(4 * B + 2) * sizeof(int64_t) > kResPinBytes) return RGBD_EINVAL;
    const int ny = e.ny;
    int64_t* ow = res_pin;  // [y rgb | y depth | z rgb | z depth], B slots each, then the error flag
    memset(ow, 0, (size_t)(4 * B + 2) * sizeof(int64_t));
    for (int m = 0; m < nm; ++m)
        HIP_TRY(hipMemcpyAsync(ow + (size_t)m * B, e.meta + 8 * B + (2 * nm + m) * ny, sizeof(int64_t) * ny, hipMemcpyDeviceToHost, s));
    if (with_z) HIP_TRY(hipMemcpyAsync(ow + 2 * B, e.meta + 6 * B, sizeof(int64_t) * nm * B, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(ow + 4 * B, e.err, sizeof(int), hipMemcpyDeviceToHost, s));
    if (const int r = wait_stream()) return r;
    if ((int)ow[4 * B]) return RGBD_ENOSPC;
    for (int m = 0; m < 2; ++m) {
        const int ns_y = m < nm ? ny : 0, ns_z = m < nm && with_z ? B : 0;
        streams[m][0].assign(ns_y, {});
        streams[m][1].assign(ns_z, {});
        for (int i = 0; i < ns_y; ++i) {
            const int64_t nw = ow[(size_t)m * B + i];
            if (nw < 0 || nw > e.ycap) return RGBD_EHIP;
            streams[m][0][i].resize((size_t)nw * 4);
            const uint32_t* src = e.ywords + ((size_t)m * ny + i) * e.ycap + (e.ycap - nw);
            HIP_TRY(hipMemcpyAsync(streams[m][0][i].data(), src, (size_t)nw * 4, hipMemcpyDeviceToHost, s));
        }
        for (int i = 0; i < ns_z; ++i) {
            const int64_t nw = ow[(size_t)2 * B + (size_t)m * B + i];
            if (nw < 0 || nw > e.zcap) return RGBD_EHIP;
            streams[m][1][i].resize((size_t)nw * 4);
            const uint32_t* src = e.zwords + ((size_t)m * B + i) * e.zcap + (e.zcap - nw);
            HIP_TRY(hipMemcpyAsync(streams[m][1][i].data(), src, (size_t)nw * 4, hipMemcpyDeviceToHost, s));
        }
    }
    return wait_stream();
}

// workspace of a decompress call and the upload of its streams: ns_y y streams and ns_z z streams per modality, every
// stream in a slot of the size the encoder may produce for this shape, so that the workspace layout (and with it a cached
// graph) does not depend on the stream lengths
int rgbd_elic::dec_streams(int nm, const uint8_t* const* ys[2], const int64_t* ylen[2], int ns_y, const uint8_t* const* zs[2],
                           const int64_t* zlen[2], int ns_z, int B, int64_t T, int64_t Tz, int per_image, DecBufs* d)
{
    const int64_t ycap = y_cap_words(per_image ? T : T * B), zcap = rgbd_enc_cap_words(Tz);
    const int64_t ymin = coder_lanes ? 8 * (int64_t)coder_lanes : 8;  // a stream holds at least its states
    // meta64: y off[nm][ns_y], y len[nm][ns_y], z off[nm][ns_z], z len[nm][ns_z], y base[B], z base[B]
    const size_t o_ylen = (size_t)nm * ns_y, o_zoff = 2 * o_ylen, o_zlen = o_zoff + (size_t)nm * ns_z;
    const size_t o_ybase = o_zlen + (size_t)nm * ns_z, nmeta = o_ybase + (size_t)2 * B;
    int64_t* meta64 = (int64_t*)arena.take(sizeof(int64_t) * nmeta);
    const size_t nwords_cap = (size_t)nm * ns_y * ycap + (size_t)nm * ns_z * zcap;
    d->words = (uint32_t*)arena.take(sizeof(uint32_t) * (nwords_cap + 4));
    d->state = (uint64_t*)arena.take(sizeof(uint64_t) * ((size_t)y_state_words() * nm * ns_y + (size_t)2 * nm * ns_z));
    d->zstate = d->state + (size_t)y_state_words() * nm * ns_y;
    d->err = coder_lanes ? (int*)arena.take(256) : nullptr;
    d->sym = (int32_t*)arena.take(sizeof(int32_t) * (size_t)(nm * B * T));
    d->idx = (int32_t*)arena.take(sizeof(int32_t) * (size_t)(nm * B * T));
    d->zsym = (int32_t*)arena.take(sizeof(int32_t) * (size_t)(nm * B * Tz));
    d->zidx = (int32_t*)arena.take(sizeof(int32_t) * (size_t)(nm * B * Tz));
    d->yoff = meta64;
    d->ylen = meta64 + o_ylen;
    d->zoff = meta64 + o_zoff;
    d->zlen = meta64 + o_zlen;
    d->ybase = meta64 + o_ybase;
    d->zbase = d->ybase + B;
    dbg_sym = d->sym;
    dbg_idx = d->idx;
    dbg_per_mod = (int64_t)B * T;
    dbg_x = dbg_s = nullptr;
    if (debug_floats) {
        dbg_x = (float*)arena.take(sizeof(float) * (size_t)(nm * B * T));
        dbg_s = (float*)arena.take(sizeof(float) * (size_t)(nm * B * T));
    }
    for (int m = 0; m < nm; ++m) {
        for (int i = 0; i < ns_y; ++i)
            if (!ys[m] || !ys[m][i] || ylen[m][i] < ymin || (ylen[m][i] & 3) || ylen[m][i] / 4 > ycap) return RGBD_EINVAL;
        for (int i = 0; i < ns_z; ++i)
            if (!zs[m] || !zs[m][i] || zlen[m][i] < 8 || (zlen[m][i] & 3) || zlen[m][i] / 4 > zcap) return RGBD_EINVAL;
    }
    if (dry()) return RGBD_OK;
    size_t total_words = 0;
    for (int m = 0; m < nm; ++m) {
        for (int i = 0; i < ns_y; ++i) total_words += (size_t)ylen[m][i] / 4;
        for (int i = 0; i < ns_z; ++i) total_words += (size_t)zlen[m][i] / 4;
    }
    void* pv = nullptr;
    if (const int r = pin_take(nmeta * sizeof(int64_t) + total_words * 4, &pv)) return r;
    int64_t* hmeta = (int64_t*)pv;
    uint32_t* hw = (uint32_t*)(hmeta + nmeta);
    size_t used = 0;
    auto put = [&](const uint8_t* src, int64_t len, size_t slot_off, size_t meta_off, size_t meta_len) -> int {
        memcpy(hw + used, src, (size_t)len);
        hmeta[meta_off] = (int64_t)slot_off;
        hmeta[meta_len] = len / 4;
        HIP_TRY(hipMemcpyAsync(d->words + slot_off, hw + used, (size_t)len, hipMemcpyHostToDevice, s));
        used += (size_t)len / 4;
        return RGBD_OK;
    };
    for (int m = 0; m < nm; ++m)
        for (int i = 0; i < ns_y; ++i) {
            const size_t k = (size_t)m * ns_y + i;
            if (const int r = put(ys[m][i], ylen[m][i], k * (size_t)ycap, k, o_ylen + k)) return r;
        }
    for (int m = 0; m < nm; ++m)
        for (int i = 0; i < ns_z; ++i) {
            const size_t k = (size_t)m * ns_z + i;
            if (const int r = put(zs[m][i], zlen[m][i], (size_t)nm * ns_y * ycap + k * (size_t)zcap, o_zoff + k, o_zlen + k)) return r;
        }
    for (int b = 0; b < B; ++b) {
        hmeta[o_ybase + b] = per_image ? (int64_t)b * T : 0;
        hmeta[o_ybase + B + b] = (int64_t)b * Tz;
    }
    HIP_TRY(hipMemcpyAsync(meta64, hmeta, sizeof(int64_t) * nmeta, hipMemcpyHostToDevice, s));
    return pin_release();
}

// ---- the pieces every call path shares -------------------------------------------------------------------------------------
void rgbd_elic::begin_call(int ref_batch_of_call, bool forward)
{
    ref_batch = ref_batch_of_call;
    named.clear();
    pre_leads.clear();
    arena.reset();
    rc = 0;
    y_segs.n = 0;
    y_seg_next = 0;
    if (forward) {
        dbg_sym = dbg_idx = nullptr;  // forward() keeps no symbols: the last compress()'s are gone with its workspace layout
        dbg_x = dbg_s = nullptr;
    }
}

// closes the body (ends the capture / launches the graph); an error recorded inside the body goes before body_end()'s own
int rgbd_elic::finish_body()
{
    const int r = body_end();
    return rc ? rc : r;
}

// teacher forcing (rgbd_elic_set_forced_symbols): the symbols of nm modalities, n each, into the workspace; *out stays null
// when none are set
int rgbd_elic::upload_forced(int nm, const std::vector<int32_t>* f, size_t n, int32_t** out)
{
    *out = nullptr;
    bool any = false;
    for (int m = 0; m < nm; ++m) any = any || !f[m].empty();
    if (!any) return RGBD_OK;
    for (int m = 0; m < nm; ++m)
        if (f[m].size() != n) return RGBD_EINVAL;
    *out = (int32_t*)arena.take(sizeof(int32_t) * nm * n);
    if (!dry())
        for (int m = 0; m < nm; ++m)
            HIP_TRY(hipMemcpyAsync(*out + m * n, f[m].data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    return RGBD_OK;
}

rgbd_elic::Coding rgbd_elic::enc_coding(const EncBufs& e, int per_image, int64_t T, const int32_t* force)
{
    Coding cd;
    cd.encode = true;
    cd.per_image = per_image;
    cd.per_image_total = T;
    cd.sym = e.sym;
    cd.idx = e.idx;
    cd.stream_base = e.meta;
    cd.force = force;
    return cd;
}

rgbd_elic::Coding rgbd_elic::dec_coding(const DecBufs& d, int per_image, int64_t T, int nstreams)
{
    Coding cd;
    cd.encode = false;
    cd.per_image = per_image;
    cd.per_image_total = T;
    cd.sym = d.sym;
    cd.idx = d.idx;
    cd.stream_base = d.ybase;
    cd.words = d.words;
    cd.stream_off = d.yoff;
    cd.stream_len = d.ylen;
    cd.state = d.state;
    cd.err = d.err;
    cd.nstreams = nstreams;
    return cd;
}

// The z stage of modality m; `pfx` ("", "rgb_", "depth_") names its entropy bottleneck.  A missing tensor ends the call with
// the error dense_of() records and launches nothing of the stage.
// compress: quantise, encode, dequantise (entropy_models.py:437-446); `fz`: forced symbols of all modalities, or null
void rgbd_elic::z_encode(int m, const char* pfx, const EncBufs& e, const Act& z, const Act& zhat, const int32_t* fz)
{
    if (dry() || rc) return;
    float* md = dense_of(std::string(pfx) + "entropy_bottleneck.medians");
    if (!md) return;
    const int B = zhat.n, zh = zhat.h, zw = zhat.w;
    const int64_t Tz = (int64_t)N * zh * zw;
    int32_t* zs = e.zsym + (size_t)m * B * Tz;
    int32_t* zi = e.zidx + (size_t)m * B * Tz;
    int r = launch_z_quant(z.p, z.cs, B, zh, zw, N, md, zs, zi, s, perm());
    if (!r)
        r = launch_rans_encode(zs, zi, e.meta + 2 * B, e.meta + 3 * B, B, B, tables[2 + m].d, tables[2 + m].d,
                               e.zwords + (size_t)m * B * e.zcap, e.zcap, e.meta + 6 * B + (size_t)m * B, e.err, s);
    if (!r) r = launch_z_dequant(fz ? fz + (size_t)m * B * Tz : zs, B, zh, zw, N, md, zhat.p, zhat.cs, s, perm());
    if (r) fail(r);
}

// decompress (entropy_models.py:442-446): one z stream per image
void rgbd_elic::z_decode(int m, const char* pfx, const DecBufs& d, const Act& zhat)
{
    if (dry() || rc) return;
    float* md = dense_of(std::string(pfx) + "entropy_bottleneck.medians");
    if (!md) return;
    const int B = zhat.n, zh = zhat.h, zw = zhat.w;
    const int64_t Tz = (int64_t)N * zh * zw;
    int32_t* zs = d.zsym + (size_t)m * B * Tz;
    int32_t* zi = d.zidx + (size_t)m * B * Tz;
    // indexes = channel id in (c, row, col) order: the quantiser's index writer on a zeroed tensor
    int r = launch_fill_zero(zhat.p, zhat.elems(), s);
    if (!r) r = launch_z_quant(zhat.p, zhat.cs, B, zh, zw, N, md, zs, zi, s, perm());
    if (!r)
        r = launch_rans_decode(d.words, d.zoff + (size_t)m * B, d.zlen + (size_t)m * B, B, d.zstate + (size_t)m * B * 2, 1, zi, zs,
                               d.zbase, 0, Tz, tables[2 + m].d, s);
    if (!r) r = launch_z_dequant(zs, B, zh, zw, N, md, zhat.p, zhat.cs, s, perm());
    if (r) fail(r);
}

// eval-mode forward: round and likelihood (entropy_models.py:391-428)
void rgbd_elic::z_estimate(const char* pfx, const Act& z, const Act& zhat, const Act& zlik)
{
    if (dry() || rc) return;
    float* md = dense_of(std::string(pfx) + "entropy_bottleneck.medians");
    float* prm = dense_of(std::string(pfx) + "entropy_bottleneck.cumulative");
    if (!md || !prm) return;
    const int r = launch_eb_forward(z.p, z.cs, zhat.n, zhat.h, zhat.w, N, md, prm, zhat.p, zlik.p, s, perm());
    if (r) fail(r);
}

// the y streams of all nm modalities in one launch, at the end of compress: streams [0, ny) are the first modality's,
// [ny, 2 ny) the second's; bases are relative to `sym`
void rgbd_elic::y_encode(int nm, int B, const EncBufs& e)
{
    if (dry() || rc) return;
    const int ny = e.ny, ns = nm * ny;
    if (coder_lanes) {  // wide rANS: the parts code_part recorded are the segments; they must tile the stream
        int r = y_segs.n > 0 && y_seg_next == e.ycount ? RGBD_OK : RGBD_ESTATE;
        if (!r)
            r = launch_rans_wide_encode(e.sym, e.idx, e.meta + 8 * B, y_segs, coder_lanes, ns, ny, tables[0].d, tables[nm - 1].d,
                                        e.ywords, e.ycap, e.meta + 8 * B + 2 * ns, e.err, s);
        if (r) fail(r);
        return;
    }
    const int r = launch_rans_encode(e.sym, e.idx, e.meta + 8 * B, e.meta + 8 * B + ns, ns, ny, tables[0].d, tables[nm - 1].d,
                                     e.ywords, e.ycap, e.meta + 8 * B + 2 * ns, e.err, s);
    if (r) fail(r);
}

// ---- the family hooks: ELIC_united (family 0, models/elic_united.py), ELIC (1, models/elic.py), STF_united (2,
// models/stf_united.py), ELIC_united_R2D (3, models/elic_united_R2D.py), STF (4, models/stf.py) and the checkerboard Cheng2020
// (5, models/Cheng2020withCKBD.py), MLIC++ (19, models/mlicpp.py) and the latent codec of ELIC_master (20, models/elic_master.py)
// share one call path per direction; a family enters through the four hooks below ----------
void rgbd_elic::g_a_family(const Act x[2], Act y[2])
{
    switch (family) {
    case Family::ELIC:
    case Family::ELIC_master_latent: y[0] = g_a1(x[0]); break;  // (AnalysisTransformEX with ch = 3 / 1 or 128: the same names)
    case Family::STF_united: g_a_stf(x[0], x[1], &y[0], &y[1]); break;
    case Family::ELIC_united_R2D: g_a_r2d(x, y); break;
    case Family::STF: y[0] = g_a_stf1(x[0]); break;
    case Family::Cheng2020_ckbd: y[0] = g_a_ckbd(x[0]); break;
    case Family::MLIC: y[0] = g_a_mlic(x[0]); break;
    default: g_a(x, y);
    }
}

void rgbd_elic::h_a_family(const Act y[2], Act z[2])
{
    switch (family) {
    case Family::ELIC:
    case Family::ELIC_master_latent: z[0] = h_a1(y[0]); break;
    case Family::STF: z[0] = h_a_stf1(y[0]); break;
    case Family::Cheng2020_ckbd: z[0] = h_a_ckbd(y[0]); break;
    case Family::MLIC: z[0] = h_a_mlic(y[0]); break;
    default: h_a(y[0], y[1], &z[0], &z[1]);
    }
}

void rgbd_elic::g_s_family(const Act yhat[2], Act xhat[2])
{
    switch (family) {
    case Family::ELIC: xhat[0] = g_s1(yhat[0]); break;
    case Family::STF_united: g_s_stf(yhat[0], yhat[1], &xhat[0], &xhat[1]); break;
    case Family::ELIC_united_R2D: g_s_r2d(yhat, xhat); break;
    case Family::STF: xhat[0] = g_s_stf1(yhat[0]); break;
    case Family::Cheng2020_ckbd: xhat[0] = g_s_ckbd(yhat[0]); break;
    case Family::MLIC: xhat[0] = g_s_mlic(yhat[0]); break;
    case Family::ELIC_master_latent: xhat[0] = g_s_master(yhat[0]); break;
    default: g_s(yhat, xhat);
    }
}

// The latent stage: everything between z_hat and y_hat -- the family's buffers, its hyper synthesis, its debug tensors and its
// coding loop (symbols when cd.encode, from the streams when not, likelihoods into cd.lik[m] when cd.estimate).  y: the
// latents (null when decoding); hyp: the hyper tensors when the caller has them already (the Latents path; zhat is null then).
//   ELIC: y_hat = round(y - mean) + mean slice by slice through the checkerboard slice loop (elic.py:180-251 / 268-316).
//   ELIC_master_latent: the same buffers and loop under kLoopMaster (elic_master.py:128-208 / 248-300 / 329-371).
//   STF: the y stream is ONE stream for all slices of all images of the call (per-image streams: one per image), coded after
//     the last slice; the decoder resumes its rANS state slice by slice.  A batch decompresses as the inverse of compress()
//     (the reference's decompress handles one image only, stf.py:799).
//   Checkerboard: both halves of all images of the call go into ONE y stream, anchor half first (per-image streams: one per
//     image, each with its own two halves); the decoder resumes its rANS state between the halves.
//   MLIC++: one state buffer [hyper_means M | y_hat M] that the loop's networks read as channel views (slice_loop_mlic); y_hat is
//     its upper half.  Streams as for ELIC: slice-major, anchor part then non-anchor part (mlicpp.py:220-305).
//   The two-modality codecs: hyper synthesis and the same slice loop over both modalities (Bi-CEE, elic_united.py:265-348).
void rgbd_elic::latent_family(Coding& cd, int B, int h, int w, const Act* y, const Act* zhat, const Act* hyp, Act yhat[2])
{
    const Modes mo = modes();
    switch (family) {
    case Family::ELIC:
    case Family::ELIC_master_latent: {
        Act hyper = h_s1(zhat[0]);
        named["hyper"] = hyper;
        yhat[0] = alloc(B, h, w, M);
        if (cd.estimate) cd.lik[0] = alloc(B, h, w, M);
        slice_loop_ckbd(cd, slice_loop_family(), 1, y, &hyper, yhat);
        break;
    }
    case Family::STF: {
        const int wide = M + (kStfSupport + 1) * kStfSliceCh;
        Act ctxm = alloc(B, h, w, wide), ctxs = alloc(B, h, w, wide);
        yhat[0] = alloc(B, h, w, M);
        {
            const size_t mark = arena.top;
            h_s_stf1(zhat[0], view(ctxm, 0, M), view(ctxs, 0, M));
            arena.top = mark;
        }
        named["latent_means"] = view(ctxm, 0, M);
        named["latent_scales"] = view(ctxs, 0, M);
        if (cd.estimate) cd.lik[0] = alloc(B, h, w, M);
        slice_loop(cd, y, ctxm, ctxs, yhat[0]);
        break;
    }
    case Family::Cheng2020_ckbd: {
        Act cat = alloc(B, h, w, 4 * M), params = alloc(B, h, w, 2 * M);
        yhat[0] = alloc(B, h, w, M);
        named["hyper"] = view(cat, 2 * M, 2 * M);
        named["ctx"] = view(cat, 0, 2 * M);
        named["scales"] = view(params, 0, M);
        named["means"] = view(params, M, M);
        if (!cd.estimate) {
            if (!dry() && !rc) {
                const int r = launch_fill_zero(cat.p, cat.elems(), s);
                if (r) fail(r);
            }
            h_s_ckbd(zhat[0], view(cat, 2 * M, 2 * M));
            two_pass_ckbd(cd, y, cat, params, yhat[0]);
            break;
        }
        // eval-mode forward (Cheng2020withCKBD.py:52-71): y_hat = round(y) (quantize "dequantize" without means, :61), the
        // context over the whole grid with its anchor outputs zeroed (:63-66), ONE parameter pass (:67-68), likelihoods of
        // round(y - mean) + mean (:69)
        Act scratch = alloc(B, h, w, M), lik = alloc(B, h, w, M);
        cd.lik[0] = lik;
        PartGeom g{};
        g.B = B;
        g.h = h;
        g.w = w;
        g.C = M;
        g.per_image = 1;
        g.perm = perm();
        if (!dry() && !rc) {
            int r = launch_fill_zero(cat.p, cat.elems(), s);
            if (!r) r = launch_fill_zero(params.p, params.elems(), s);
            // round(y): the quantiser of the parts with zero means (its likelihoods go to `lik`, overwritten below)
            for (int anchor = 1; anchor >= 0 && !r; --anchor) {
                g.anchor = anchor;
                r = launch_ckbd_estimate_part(y->p, y->cs, params.p, params.cs, yhat[0].p, yhat[0].cs, lik.p, lik.cs, g, s);
            }
            if (r) fail(r);
        }
        h_s_ckbd(zhat[0], view(cat, 2 * M, 2 * M));
        ck_context(yhat[0], view(cat, 0, 2 * M));
        ck_entropy_params(cat, 0, params);
        if (!dry() && !rc) {
            int r = 0;
            for (int anchor = 1; anchor >= 0 && !r; --anchor) {
                g.anchor = anchor;
                r = launch_ckbd_estimate_part(y->p, y->cs, params.p, params.cs, scratch.p, scratch.cs, lik.p, lik.cs, g, s);
            }
            if (r) fail(r);
        }
        break;
    }
    case Family::MLIC: {
        const Act state = alloc(B, h, w, 2 * M), hyper = alloc(B, h, w, 2 * M);
        h_s_mlic(zhat[0], hyper);
        copy_ch(view(hyper, M, M), view(state, 0, M));  // hyper_scales, hyper_means = hyper_params.chunk(2, 1)
        yhat[0] = view(state, M, M);
        named["hyper"] = hyper;
        if (cd.estimate) cd.lik[0] = alloc(B, h, w, M);
        slice_loop_mlic(cd, y, hyper, state);
        break;
    }
    default: {
        Act hy[2];
        if (hyp) {
            hy[0] = hyp[0];
            hy[1] = hyp[1];
        } else if (family == Family::ELIC_united_R2D) {
            h_s_r2d(zhat[0], zhat[1], &hy[0], &hy[1]);
        } else {
            h_s(zhat[0], zhat[1], &hy[0], &hy[1]);
        }
        if (!cd.estimate) name(mo, "hyper", hy);  // (deliberate: forward() of these codecs never named hyper_r / hyper_d; Modes)
        for (int m = 0; m < 2; ++m) yhat[m] = alloc(B, h, w, M);
        if (family == Family::STF_united && !dry()) {  // 24-wide slices: a 16-channel read chunk may straddle into a slice not coded yet
            int zr = launch_fill_zero(yhat[0].p, yhat[0].elems(), s);
            if (!zr) zr = launch_fill_zero(yhat[1].p, yhat[1].elems(), s);
            if (zr) fail(zr);
        }
        if (cd.estimate)
            for (int m = 0; m < 2; ++m) cd.lik[m] = alloc(B, h, w, M);
        slice_loop_ckbd(cd, slice_loop_family(), 2, y, hy, yhat);
    }
    }
    name(mo, "yhat", yhat);
}

// ---- the call paths, for nm = 1 or 2 modalities ---------------------------------------------------------------------------
// y = g_a(x) into buffers the caller keeps; the transform's own workspace goes back
void rgbd_elic::analysis(const Act x[2], const Act y[2])
{
    const size_t mark = arena.top;
    Act yt[2];
    g_a_family(x, yt);
    for (int m = 0; m < modes().nm; ++m) copy_ch(yt[m], y[m]);
    arena.top = mark;
    ends_release();
}

// compress: elic_united.py:350-460, elic.py:161-253, stf.py:703-764, Cheng2020withCKBD.py:101-136
int rgbd_elic::run_compress(int nm, In2 x_dev, int B, int H, int W, int per_image, const Latents* lat)
{
    const Modes mo = modes();
    if (nm != mo.nm) return RGBD_ESTATE;
    const int h = H / 16, w = W / 16, zh = lat ? 1 : H / 64, zw = lat ? 1 : W / 64;
    const int64_t T = (int64_t)M * h * w;  // y symbols per image per modality
    const int64_t Tz = (int64_t)N * zh * zw;
    begin_call(per_image ? 1 : B, false);  // per-image streams stand for the reference called image by image

    // ==== prologue (never captured): workspace of the call, upload of the stream geometry, input layout conversion ====
    EncBufs e;
    if (const int r = enc_streams(nm, B, T, Tz, per_image, &e)) return r;
    int32_t *fy = nullptr, *fz = nullptr;  // (of the single-modal families only the checkerboard one accepts forced symbols)
    if (const int r = upload_forced(nm, force_y, (size_t)(B * T), &fy)) return r;
    if (!lat)
        if (const int r = upload_forced(nm, force_z, (size_t)(B * Tz), &fz)) return r;

    Act y[2], hyp[2], x[2];
    for (int m = 0; m < nm; ++m) y[m] = alloc(B, h, w, M);
    if (lat) {
        for (int m = 0; m < nm; ++m) hyp[m] = alloc(B, h, w, 2 * M);
        int r = 0;
        for (int m = 0; m < nm && !r && !dry(); ++m)
            r = launch_nchw_to_nhwc16(lat->y[m], B, M, h, w, y[m].p, y[m].cs, s, perm());
        for (int m = 0; m < nm && !r && !dry(); ++m)
            r = launch_nchw_to_nhwc16(lat->hyp[m], B, 2 * M, h, w, hyp[m].p, hyp[m].cs, s, perm());
        if (r) return r;
    } else {
        for (int m = 0; m < nm; ++m) x[m] = alloc(B, H, W, mo.img_ch[m]);
        int r = 0;
        for (int m = 0; m < nm && !r && !dry(); ++m)
            r = launch_nchw_to_nhwc16(x_dev[m], B, mo.img_ch[m], H, W, x[m].p, x[m].cs, s);
        if (r) return r;
    }

    // ==== body: every kernel of the call, in stream order; captured into / replayed from a HIP graph per call shape ====
    if (body_begin()) {
        if (!dry()) {
            const int zr = launch_fill_zero((float*)e.err, 64, s);  // (a kernel, not a memset node: see launch_fill_zero)
            if (zr) fail(zr);
        }
        name(mo, "y", y);
        Act zhat[2], yhat[2];
        if (!lat) {
            analysis(x, y);
            Act z[2];
            h_a_family(y, z);
            name(mo, "z", z);
            for (int m = 0; m < nm; ++m) zhat[m] = alloc(B, zh, zw, N);
            for (int m = 0; m < nm; ++m) z_encode(m, mo.eb[m], e, z[m], zhat[m], fz);
            name(mo, "zhat", zhat);
        }
        Coding cd = enc_coding(e, per_image, T, fy);
        latent_family(cd, B, h, w, y, lat ? nullptr : zhat, lat ? hyp : nullptr, yhat);
        {
            Phase ph(this, "phase.coder");
            y_encode(nm, B, e);
        }
    }
    if (const int r = finish_body()) return r;
    if (dry()) return RGBD_OK;

    // ==== epilogue (never captured): fetch the streams ================================================================
    return fetch_streams(nm, B, !lat, e);
}

// eval-mode forward(): elic_united.py:234-263 with quant == "ste" (round in eval), elic.py:60-161, stf.py:618-678,
// Cheng2020withCKBD.py:52-71; likelihoods as in entropy_models.py:391-428 (factorised prior) and :534-558 (Gaussian
// conditional) instead of symbols
int rgbd_elic::run_forward(int nm, In2 x_dev, int B, int H, int W, Out2 xhat_dev, Out2 ly, Out2 lz, const Mid3* up, const Guide3* guides)
{
    const Modes mo = modes();
    if (nm != mo.nm) return RGBD_ESTATE;
    if (up && family != Family::ELIC) return RGBD_EINVAL;
    if ((guides != nullptr) != (family == Family::ELIC_master_latent)) return RGBD_EINVAL;
    const int h = H / 16, w = W / 16, zh = H / 64, zw = W / 64;
    begin_call(B, true);  // forward() is one reference call on the whole batch
    Act x[2];
    for (int m = 0; m < nm; ++m) x[m] = alloc(B, H, W, mo.img_ch[m]);
    if (!dry()) {
        int r = 0;
        for (int m = 0; m < nm && !r; ++m) r = launch_nchw_to_nhwc16(x_dev[m], B, mo.img_ch[m], H, W, x[m].p, x[m].cs, s);
        if (r) return r;
    }
    Act guide[3];
    if (guides)
        if (const int r = guides_begin(guides->data(), B, H, W, guide)) return r;
    // ==== body: captured into / replayed from a HIP graph per call shape (the prologue above reads the caller's pointers,
    // the epilogue below writes them) ====
    Act out[3][2];  // x_hat, likelihoods of y, likelihoods of z: cur_ge->out[2 * k + m]
    Act mid[3];     // return_mid (one modality): cur_ge->out[1], [3], [5]
    if (body_begin()) {
        Act y[2], z[2], zhat[2], yhat[2];
        for (int m = 0; m < nm; ++m) y[m] = alloc(B, h, w, M);
        analysis(x, y);
        h_a_family(y, z);
        for (int m = 0; m < nm; ++m) zhat[m] = alloc(B, zh, zw, N);
        for (int m = 0; m < nm; ++m) out[2][m] = alloc(B, zh, zw, N);
        for (int m = 0; m < nm; ++m) z_estimate(mo.eb[m], z[m], zhat[m], out[2][m]);
        name(mo, "y", y);
        if (mo.forward_names_z) {
            name(mo, "z", z);
            name(mo, "zhat", zhat);
        }
        Coding cd;
        cd.estimate = true;
        latent_family(cd, B, h, w, y, zhat, nullptr, yhat);
        if (up) mids_begin(B, H, W, mid);
        g_s_family(yhat, out[0]);
        mid_dst = nullptr;
        guide_src = nullptr;
        for (int m = 0; m < nm; ++m) out[1][m] = cd.lik[m];
        if (cur_ge && !dry()) {
            for (int k = 0; k < 3; ++k)
                for (int m = 0; m < nm; ++m) cur_ge->out[2 * k + m] = out[k][m];
            for (int k = 0; k < 3 && up; ++k) cur_ge->out[2 * k + 1] = mid[k];
        }
    } else {
        for (int k = 0; k < 3; ++k)
            for (int m = 0; m < nm; ++m) out[k][m] = cur_ge->out[2 * k + m];
        for (int k = 0; k < 3 && up; ++k) mid[k] = cur_ge->out[2 * k + 1];
    }
    guide_src = nullptr;  // (a replayed body never reads it)
    if (const int r = finish_body()) return r;
    if (dry()) return RGBD_OK;
    int r = 0;  // (not clamped: stf.py:677)
    for (int m = 0; m < nm && !r; ++m)
        r = launch_nhwc_to_nchw_clamp(out[0][m].p, B, mo.out_ch[m], H, W, out[0][m].cs, xhat_dev[m], 0, s);
    for (int m = 0; m < nm && !r; ++m) r = launch_nhwc_to_nchw_clamp(out[1][m].p, B, M, h, w, out[1][m].cs, ly[m], 0, s, perm());
    for (int m = 0; m < nm && !r; ++m) r = launch_nhwc_to_nchw_clamp(out[2][m].p, B, N, zh, zw, out[2][m].cs, lz[m], 0, s, perm());
    if (!r && up) r = mids_out(mid, B, H, W, *up);
    if (!r) r = wait_stream();
    return r;
}

// return_mid (models/elic.py:159-170, 318-329): up1..up3 are the outputs of g_s's first three transposed convolutions.  The body
// copies them into workspace of the call that lives until its end (the addresses a captured graph replays); like x_hat they go
// to the caller's NCHW tensors in the epilogue, which is never captured: a replay must not write to the tensors of the call
// that was captured.
// The guides of ELIC_master_latent (elic_master.py:213-216, 375-378): up1..up3 [B,N,H/8,W/8], [B,N,H/4,W/4], [B,N,H/2,W/2] of the aux
// decoder, converted to NHWC workspace of the call in the prologue, as run_synthesis_plus takes them: the body reads workspace
// addresses only, so a replayed graph sees the tensors of its own call.
int rgbd_elic::guides_begin(const float* const up_dev[3], int B, int H, int W, Act up[3])
{
    for (int k = 0; k < 3; ++k) up[k] = alloc(B, H >> (3 - k), W >> (3 - k), N);
    for (int k = 0; k < 3 && !dry(); ++k)
        if (const int r = launch_nchw_to_nhwc16(up_dev[k], B, N, up[k].h, up[k].w, up[k].p, up[k].cs, s)) return r;
    guide_src = up;
    return RGBD_OK;
}

void rgbd_elic::mids_begin(int B, int H, int W, Act mid[3])
{
    for (int k = 0; k < 3; ++k) mid[k] = alloc(B, H >> (3 - k), W >> (3 - k), N);
    mid_dst = mid;
}

int rgbd_elic::mids_out(const Act mid[3], int B, int H, int W, const Mid3& up)
{
    int r = 0;
    for (int k = 0; k < 3 && !r; ++k)
        r = launch_nhwc_to_nchw_clamp(mid[k].p, B, N, H >> (3 - k), W >> (3 - k), mid[k].cs, up[k], 0, s, perm());
    return r;
}

// Spatial_aligner alone (family 6): x, guided [B,in_ch,H,W] -> out [B,out_ch,H,W]
int rgbd_elic::run_aligner(const float* x_dev, const float* guided_dev, int B, int H, int W, float* out_dev)
{
    begin_call(B, true);
    const Act x = alloc(B, H, W, in_ch), g = alloc(B, H, W, in_ch);
    if (!dry()) {
        int r = launch_nchw_to_nhwc16(x_dev, B, in_ch, H, W, x.p, x.cs, s);
        if (!r) r = launch_nchw_to_nhwc16(guided_dev, B, in_ch, H, W, g.p, g.cs, s);
        if (r) return r;
    }
    // ==== body: captured into / replayed from a HIP graph per call shape ====
    Act out;
    if (body_begin()) {
        out = spatial_aligner("", x, g);
        if (cur_ge && !dry()) cur_ge->out[0] = out;
    } else {
        out = cur_ge->out[0];
    }
    if (const int r = finish_body()) return r;
    if (dry()) return RGBD_OK;
    int r = launch_nhwc_to_nchw_clamp(out.p, B, out_ch, H, W, out.cs, out_dev, 0, s);
    if (!r) r = wait_stream();
    return r;
}

// SynthesisTransformPlus alone (family 13; synthesis.py:74-110): the 15 g_s stages of the single-modal ELIC with
// Spatial_aligner(x, up_k) in place of x behind the first three transposed convolutions.  in_ch is M.
int rgbd_elic::run_synthesis_plus(const float* yhat_dev, const float* const up_dev[3], int B, int h, int w, float* out_dev)
{
    begin_call(B, true);
    const Act yhat = alloc(B, h, w, in_ch);
    Act up[3];
    for (int k = 0; k < 3; ++k) up[k] = alloc(B, (2 * h) << k, (2 * w) << k, N);
    if (!dry()) {
        int r = launch_nchw_to_nhwc16(yhat_dev, B, in_ch, h, w, yhat.p, yhat.cs, s);
        for (int k = 0; k < 3 && !r; ++k) r = launch_nchw_to_nhwc16(up_dev[k], B, N, up[k].h, up[k].w, up[k].p, up[k].cs, s);
        if (r) return r;
    }
    // ==== body: captured into / replayed from a HIP graph per call shape ====
    Act out;
    if (body_begin()) {
        Act xhat[2];
        stages({kSyn15, 15, 1, {"synthesis_transform.", ""}, kNoFusion, false, false, false, nullptr, plus_guides ? up : nullptr, ""},
               &yhat, xhat);
        out = xhat[0];
        if (cur_ge && !dry()) cur_ge->out[0] = out;
    } else {
        out = cur_ge->out[0];
    }
    if (const int r = finish_body()) return r;
    if (dry()) return RGBD_OK;
    int r = launch_nhwc_to_nchw_clamp(out.p, B, out_ch, 16 * h, 16 * w, out.cs, out_dev, 0, s);
    if (!r) r = wait_stream();
    return r;
}

// An attention context of MLIC++ alone (families 7-9): x1 (and x2 of LinearGlobalIntraContext) [B,in_ch,H,W] -> [B,out_ch,H,W]
int rgbd_elic::run_context(const float* x1_dev, const float* x2_dev, int B, int H, int W, float* out_dev)
{
    begin_call(B, true);
    const Act x1 = alloc(B, H, W, in_ch), x2 = family == Family::LinearGlobalIntraContext ? alloc(B, H, W, in_ch) : Act();
    if (!dry()) {
        int r = launch_nchw_to_nhwc16(x1_dev, B, in_ch, H, W, x1.p, x1.cs, s);
        if (!r && family == Family::LinearGlobalIntraContext) r = launch_nchw_to_nhwc16(x2_dev, B, in_ch, H, W, x2.p, x2.cs, s);
        if (r) return r;
    }
    // ==== body: captured into / replayed from a HIP graph per call shape ====
    Act out;
    if (body_begin()) {
        if (family == Family::LocalContext) {
            out = local_context(x1);
        } else if (family == Family::LinearGlobalInterContext) {
            out = linear_context(x1, x1, x1, 0, true);
        } else {
            const Act xa = alloc(B, H, W, in_ch), xn = alloc(B, H, W, in_ch);  // ckbd_anchor(x1), ckbd_nonanchor(x1): :191-192
            if (!dry() && !rc) {
                const int r = launch_ckbd_split(x1.p, B, H, W, x1.cs, xa.p, xn.p, s);
                if (r) fail(r);
            }
            out = linear_context(xa, xn, x2, 1, false);
        }
        if (cur_ge && !dry()) cur_ge->out[0] = out;
    } else {
        out = cur_ge->out[0];
    }
    if (const int r = finish_body()) return r;
    if (dry()) return RGBD_OK;
    int r = launch_nhwc_to_nchw_clamp(out.p, B, out_ch, H, W, out.cs, out_dev, 0, s);
    if (!r) r = wait_stream();
    return r;
}

// A per-slice network of MLIC++ alone (families 15-17).  EntropyParametersMLIC takes its input as nseg tensors, each converted
// to an NHWC tensor of its own: the fused launch reads them in place.  Under a parity the current content of out_dev is
// converted too, so that the pixels the launch leaves alone come back as they were.
int rgbd_elic::run_slice_net(const float* const* seg_dev, const int* seg_c, int nseg, int parity, int B, int H, int W, float* out_dev)
{
    begin_call(B, true);
    Act seg[PIXEL_MLP_MAX_SEGS];
    for (int i = 0; i < nseg; ++i) seg[i] = alloc(B, H, W, seg_c[i]);
    const Act kept = parity >= 0 ? alloc(B, H, W, out_ch) : Act();
    if (!dry()) {
        int r = 0;
        for (int i = 0; i < nseg && !r; ++i) r = launch_nchw_to_nhwc16(seg_dev[i], B, seg_c[i], H, W, seg[i].p, seg[i].cs, s);
        if (!r && parity >= 0) r = launch_nchw_to_nhwc16(out_dev, B, out_ch, H, W, kept.p, kept.cs, s);
        if (r) return r;
    }
    // ==== body: captured into / replayed from a HIP graph per call shape ====
    Act out;
    if (body_begin()) {
        if (family == Family::EntropyParametersMLIC) out = entropy_params_mlic(seg, nseg, parity + 1, parity >= 0 ? &kept : nullptr);
        else if (family == Family::ChannelContext) out = channel_context_mlic(seg[0]);
        else out = lrp_mlic(seg[0]);
        if (cur_ge && !dry()) cur_ge->out[0] = out;
    } else {
        out = cur_ge->out[0];
    }
    if (const int r = finish_body()) return r;
    if (dry()) return RGBD_OK;
    int r = launch_nhwc_to_nchw_clamp(out.p, B, out_ch, H, W, out.cs, out_dev, 0, s);
    if (!r) r = wait_stream();
    return r;
}

// decompress: elic_united.py:462-578, elic.py:255-325, stf.py:766-816, Cheng2020withCKBD.py:138-174; h x w: the latent grid
int rgbd_elic::run_decompress(int nm, const uint8_t* const* ys[2], const int64_t* ylen[2], int n_y, const uint8_t* const* zs[2],
                              const int64_t* zlen[2], int B, int h, int w, Out2 xhat_dev, const Latents* lat, const Mid3* up,
                              const Guide3* guides)
{
    const Modes mo = modes();
    if (nm != mo.nm) return RGBD_ESTATE;
    if (up && (family != Family::ELIC || lat)) return RGBD_EINVAL;
    if ((guides != nullptr) != (family == Family::ELIC_master_latent) || (guides && lat)) return RGBD_EINVAL;
    const int zh = lat ? 1 : h / 4, zw = lat ? 1 : w / 4, H = h * 16, W = w * 16;
    const int64_t T = (int64_t)M * h * w, Tz = (int64_t)N * zh * zw;
    const int per_image = (n_y == B && !(B == 1)) ? 1 : (n_y == 1 ? (B == 1 ? 1 : 0) : -1);
    if (per_image < 0) return RGBD_EINVAL;
    begin_call(per_image == 0 ? B : 1, false);

    // ==== prologue (never captured): upload the streams ================================================================
    const int ns_y = n_y, ns_z = lat ? 0 : B;
    DecBufs d;
    if (const int r = dec_streams(nm, ys, ylen, ns_y, zs, zlen, ns_z, B, T, Tz, per_image, &d)) return r;

    Act hyp[2];
    if (lat) {
        for (int m = 0; m < nm; ++m) hyp[m] = alloc(B, h, w, 2 * M);
        int r = 0;
        for (int m = 0; m < nm && !r && !dry(); ++m)
            r = launch_nchw_to_nhwc16(lat->hyp[m], B, 2 * M, h, w, hyp[m].p, hyp[m].cs, s, perm());
        if (r) return r;
    }
    Act guide[3];
    if (guides)
        if (const int r = guides_begin(guides->data(), B, H, W, guide)) return r;

    // ==== body: captured into / replayed from a HIP graph per call shape ================================================
    Act out[2];  // what the epilogue hands back: x_hat (or y_hat for decompress_united) per modality: cur_ge->out[m]
    Act mid[3];  // return_mid (one modality): cur_ge->out[1], [3], [5]
    if (body_begin()) {
        if (d.err && !dry()) {  // wide coder: the decoder's error flag
            const int zr = launch_fill_zero((float*)d.err, 64, s);
            if (zr) fail(zr);
        }
        Act zhat[2], yhat[2];
        if (!lat) {
            for (int m = 0; m < nm; ++m) zhat[m] = alloc(B, zh, zw, N);
            for (int m = 0; m < nm; ++m) z_decode(m, mo.eb[m], d, zhat[m]);
            name(mo, "zhat", zhat);
        }
        Coding cd = dec_coding(d, per_image, T, ns_y);
        latent_family(cd, B, h, w, nullptr, lat ? nullptr : zhat, lat ? hyp : nullptr, yhat);
        if (lat)  // decompress_united ends here: y_hat back to the caller
            for (int m = 0; m < nm; ++m) out[m] = yhat[m];
        else {
            if (up) mids_begin(B, H, W, mid);
            g_s_family(yhat, out);
            mid_dst = nullptr;
        }
        guide_src = nullptr;
        if (cur_ge && !dry()) {
            for (int m = 0; m < nm; ++m) cur_ge->out[m] = out[m];
            for (int k = 0; k < 3 && up; ++k) cur_ge->out[2 * k + 1] = mid[k];
        }
    } else {
        for (int m = 0; m < nm; ++m) out[m] = cur_ge->out[m];
        for (int k = 0; k < 3 && up; ++k) mid[k] = cur_ge->out[2 * k + 1];
    }
    guide_src = nullptr;  // (a replayed body never reads it)
    if (const int r = finish_body()) return r;
    if (dry()) return RGBD_OK;

    // ==== epilogue (never captured): results into the caller's NCHW tensors ==========================================
    int r = 0;
    for (int m = 0; m < nm && !r; ++m)
        r = lat ? launch_nhwc_to_nchw_clamp(out[m].p, B, M, h, w, out[m].cs, lat->yhat[m], 0, s, perm())
                : launch_nhwc_to_nchw_clamp(out[m].p, B, mo.out_ch[m], H, W, out[m].cs, xhat_dev[m], mo.clamp, s);
    if (!r && up) r = mids_out(mid, B, H, W, *up);
    if (!r && d.err) {  // the caller's wait (run_call) reads the flag: a damaged wide stream fails the call
        if (!res_pin) HIP_TRY(hipHostMalloc((void**)&res_pin, kResPinBytes, hipHostMallocDefault));
        int64_t* slot = res_pin + kResPinBytes / sizeof(int64_t) - 1;
        *slot = 0;
        HIP_TRY(hipMemcpyAsync(slot, d.err, sizeof(int), hipMemcpyDeviceToHost, s));
        dec_err_pending = true;
    }
    return r;
}
