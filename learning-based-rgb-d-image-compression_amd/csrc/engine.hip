// Host runtime of the gfx950 codec engine, part 2 of 3: the call paths -- compress(), decompress() and the eval forward of the
// two-modality codecs and, once for all of them, of the single-modal families -- as sequences of kernel launches through the
// layer graph of engine.h
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
    e->ycap = rgbd_enc_cap_words(ycount);
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
    const int64_t ycap = rgbd_enc_cap_words(per_image ? T : T * B), zcap = rgbd_enc_cap_words(Tz);
    // meta64: y off[nm][ns_y], y len[nm][ns_y], z off[nm][ns_z], z len[nm][ns_z], y base[B], z base[B]
    const size_t o_ylen = (size_t)nm * ns_y, o_zoff = 2 * o_ylen, o_zlen = o_zoff + (size_t)nm * ns_z;
    const size_t o_ybase = o_zlen + (size_t)nm * ns_z, nmeta = o_ybase + (size_t)2 * B;
    int64_t* meta64 = (int64_t*)arena.take(sizeof(int64_t) * nmeta);
    const size_t nwords_cap = (size_t)nm * ns_y * ycap + (size_t)nm * ns_z * zcap;
    d->words = (uint32_t*)arena.take(sizeof(uint32_t) * (nwords_cap + 4));
    d->state = (uint64_t*)arena.take(sizeof(uint64_t) * (size_t)(2 * nm * (ns_y + ns_z)));
    d->zstate = d->state + (size_t)2 * nm * ns_y;
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
            if (!ys[m] || !ys[m][i] || ylen[m][i] < 8 || (ylen[m][i] & 3) || ylen[m][i] / 4 > ycap) return RGBD_EINVAL;
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
    const int r = launch_rans_encode(e.sym, e.idx, e.meta + 8 * B, e.meta + 8 * B + ns, ns, ny, tables[0].d, tables[nm - 1].d,
                                     e.ywords, e.ycap, e.meta + 8 * B + 2 * ns, e.err, s);
    if (r) fail(r);
}

// ---- the two-modality codecs ---------------------------------------------------------------------------------------------
int rgbd_elic::run_compress(const float* rgb_dev, const float* depth_dev, int B, int H, int W, int per_image,
                            const Latents* lat)
{
    const int h = H / 16, w = W / 16, zh = lat ? 1 : H / 64, zw = lat ? 1 : W / 64;
    const int Ctot = M;
    const int64_t T = (int64_t)Ctot * h * w;  // y symbols per image per modality
    const int64_t Tz = (int64_t)N * zh * zw;
    begin_call(per_image ? 1 : B, false);  // per-image streams stand for the reference called image by image

    // ==== prologue (never captured): workspace of the call, upload of the stream geometry, input layout conversion ====
    EncBufs e;
    if (const int r = enc_streams(2, B, T, Tz, per_image, &e)) return r;
    int32_t *fy = nullptr, *fz = nullptr;
    if (const int r = upload_forced(2, force_y, (size_t)(B * T), &fy)) return r;
    if (!lat)
        if (const int r = upload_forced(2, force_z, (size_t)(B * Tz), &fz)) return r;

    Act y_r = alloc(B, h, w, M), y_d = alloc(B, h, w, M);
    Act hyp_r, hyp_d, rgb, depth;
    if (lat) {
        hyp_r = alloc(B, h, w, 2 * M);
        hyp_d = alloc(B, h, w, 2 * M);
        if (!dry()) {
            int r = launch_nchw_to_nhwc16(lat->y[0], B, M, h, w, y_r.p, y_r.cs, s, perm());
            if (!r) r = launch_nchw_to_nhwc16(lat->y[1], B, M, h, w, y_d.p, y_d.cs, s, perm());
            if (!r) r = launch_nchw_to_nhwc16(lat->hyp[0], B, 2 * M, h, w, hyp_r.p, hyp_r.cs, s, perm());
            if (!r) r = launch_nchw_to_nhwc16(lat->hyp[1], B, 2 * M, h, w, hyp_d.p, hyp_d.cs, s, perm());
            if (r) return r;
        }
    } else {
        rgb = alloc(B, H, W, 3);
        depth = alloc(B, H, W, 1);
        if (!dry()) {
            int r = launch_nchw_to_nhwc16(rgb_dev, B, 3, H, W, rgb.p, rgb.cs, s);
            if (!r) r = launch_nchw_to_nhwc16(depth_dev, B, 1, H, W, depth.p, depth.cs, s);
            if (r) return r;
        }
    }

    // ==== body: every kernel of the call, in stream order; captured into / replayed from a HIP graph per call shape ====
    if (body_begin()) {
        if (!dry()) {
            const int zr = launch_fill_zero((float*)e.err, 64, s);  // (a kernel, not a memset node: see launch_fill_zero)
            if (zr) fail(zr);
        }
        named["y_r"] = y_r;
        named["y_d"] = y_d;
        if (!lat) {
            // ---- analysis
            Act z_r, z_d;
            {
                const size_t mark = arena.top;
                Act yr_t, yd_t;
                if (variant == 2) g_a_stf(rgb, depth, &yr_t, &yd_t);
                else if (variant == 3) g_a_r2d(rgb, depth, &yr_t, &yd_t);
                else g_a(rgb, depth, &yr_t, &yd_t);
                copy_ch(yr_t, y_r);
                copy_ch(yd_t, y_d);
                arena.top = mark;
                ends_release();
            }
            h_a(y_r, y_d, &z_r, &z_d);
            named["z_r"] = z_r;
            named["z_d"] = z_d;

            Act zh_r = alloc(B, zh, zw, N), zh_d = alloc(B, zh, zw, N);
            z_encode(0, "rgb_", e, z_r, zh_r, fz);
            z_encode(1, "depth_", e, z_d, zh_d, fz);
            named["zhat_r"] = zh_r;
            named["zhat_d"] = zh_d;

            // ---- hyper synthesis
            if (variant == 3) h_s_r2d(zh_r, zh_d, &hyp_r, &hyp_d);
            else h_s(zh_r, zh_d, &hyp_r, &hyp_d);
        }
        named["hyper_r"] = hyp_r;
        named["hyper_d"] = hyp_d;
        Act yhat_r = alloc(B, h, w, M), yhat_d = alloc(B, h, w, M);
        if (variant == 2 && !dry()) {  // 24-wide slices: a 16-channel read chunk may straddle into a slice not coded yet
            int zr = launch_fill_zero(yhat_r.p, yhat_r.elems(), s);
            if (!zr) zr = launch_fill_zero(yhat_d.p, yhat_d.elems(), s);
            if (zr) fail(zr);
        }
        named["yhat_r"] = yhat_r;
        named["yhat_d"] = yhat_d;
        Coding cd = enc_coding(e, per_image, T, fy);
        if (variant == 3) bicee_r2d(cd, &y_r, &y_d, hyp_r, hyp_d, yhat_r, yhat_d);
        else bicee(cd, &y_r, &y_d, hyp_r, hyp_d, yhat_r, yhat_d);
        y_encode(2, B, e);
    }
    if (const int r = finish_body()) return r;
    if (dry()) return RGBD_OK;

    // ==== epilogue (never captured): fetch the streams ================================================================
    return fetch_streams(2, B, !lat, e);
}

// eval-mode forward(): models/elic_united.py:234-263 with quant == "ste" (round in eval), likelihoods as in
// entropy_models.py:391-428 (factorised prior) and :534-558 (Gaussian conditional)
int rgbd_elic::run_forward(const float* rgb_dev, const float* depth_dev, int B, int H, int W, float* xr_dev, float* xd_dev,
                           float* ly_r, float* ly_d, float* lz_r, float* lz_d)
{
    const int h = H / 16, w = W / 16, zh = H / 64, zw = W / 64;
    begin_call(B, true);  // forward() is one reference call on the whole batch
    Act rgb = alloc(B, H, W, 3), depth = alloc(B, H, W, 1);
    if (!dry()) {
        int r = launch_nchw_to_nhwc16(rgb_dev, B, 3, H, W, rgb.p, rgb.cs, s);
        if (!r) r = launch_nchw_to_nhwc16(depth_dev, B, 1, H, W, depth.p, depth.cs, s);
        if (r) return r;
    }
    // ==== body: captured into / replayed from a HIP graph per call shape (the prologue above reads the caller's pointers,
    // the epilogue below writes them) ====
    Act xr, xd, lik_r, lik_d, zl_r, zl_d;
    if (body_begin()) {
        Act y_r = alloc(B, h, w, M), y_d = alloc(B, h, w, M);
        Act z_r, z_d;
        {
            const size_t mark = arena.top;
            Act yr_t, yd_t;
            if (variant == 2) g_a_stf(rgb, depth, &yr_t, &yd_t);
            else if (variant == 3) g_a_r2d(rgb, depth, &yr_t, &yd_t);
            else g_a(rgb, depth, &yr_t, &yd_t);
            copy_ch(yr_t, y_r);
            copy_ch(yd_t, y_d);
            arena.top = mark;
            ends_release();
        }
        h_a(y_r, y_d, &z_r, &z_d);
        Act zh_r = alloc(B, zh, zw, N), zh_d = alloc(B, zh, zw, N);
        zl_r = alloc(B, zh, zw, N);
        zl_d = alloc(B, zh, zw, N);
        z_estimate("rgb_", z_r, zh_r, zl_r);
        z_estimate("depth_", z_d, zh_d, zl_d);
        Act hyp_r, hyp_d;
        if (variant == 3) h_s_r2d(zh_r, zh_d, &hyp_r, &hyp_d);
        else h_s(zh_r, zh_d, &hyp_r, &hyp_d);
        Act yhat_r = alloc(B, h, w, M), yhat_d = alloc(B, h, w, M);
        if (variant == 2 && !dry()) {  // 24-wide slices: a 16-channel read chunk may straddle into a slice not coded yet
            int zr = launch_fill_zero(yhat_r.p, yhat_r.elems(), s);
            if (!zr) zr = launch_fill_zero(yhat_d.p, yhat_d.elems(), s);
            if (zr) fail(zr);
        }
        Coding cd;
        cd.estimate = true;
        cd.lik[0] = alloc(B, h, w, M);
        cd.lik[1] = alloc(B, h, w, M);
        if (variant == 3) bicee_r2d(cd, &y_r, &y_d, hyp_r, hyp_d, yhat_r, yhat_d);
        else bicee(cd, &y_r, &y_d, hyp_r, hyp_d, yhat_r, yhat_d);
        named["y_r"] = y_r;
        named["y_d"] = y_d;
        named["yhat_r"] = yhat_r;
        named["yhat_d"] = yhat_d;
        if (variant == 2) g_s_stf(yhat_r, yhat_d, &xr, &xd);
        else if (variant == 3) g_s_r2d(yhat_r, yhat_d, &xr, &xd);
        else g_s(yhat_r, yhat_d, &xr, &xd);
        lik_r = cd.lik[0];
        lik_d = cd.lik[1];
        if (cur_ge && !dry()) {
            const Act o[6] = {xr, xd, lik_r, lik_d, zl_r, zl_d};
            for (int k = 0; k < 6; ++k) cur_ge->out[k] = o[k];
        }
    } else {
        xr = cur_ge->out[0];
        xd = cur_ge->out[1];
        lik_r = cur_ge->out[2];
        lik_d = cur_ge->out[3];
        zl_r = cur_ge->out[4];
        zl_d = cur_ge->out[5];
    }
    if (const int r = finish_body()) return r;
    if (dry()) return RGBD_OK;
    int r = launch_nhwc_to_nchw_clamp(xr.p, B, 3, H, W, xr.cs, xr_dev, 0, s);
    if (!r) r = launch_nhwc_to_nchw_clamp(xd.p, B, 1, H, W, xd.cs, xd_dev, 0, s);
    if (!r) r = launch_nhwc_to_nchw_clamp(lik_r.p, B, M, h, w, lik_r.cs, ly_r, 0, s, perm());
    if (!r) r = launch_nhwc_to_nchw_clamp(lik_d.p, B, M, h, w, lik_d.cs, ly_d, 0, s, perm());
    if (!r) r = launch_nhwc_to_nchw_clamp(zl_r.p, B, N, zh, zw, zl_r.cs, lz_r, 0, s, perm());
    if (!r) r = launch_nhwc_to_nchw_clamp(zl_d.p, B, N, zh, zw, zl_d.cs, lz_d, 0, s, perm());
    if (!r) r = wait_stream();
    return r;
}

int rgbd_elic::run_decompress(const uint8_t* const* ys[2], const int64_t* ylen[2], int n_y, const uint8_t* const* zs[2],
                              const int64_t* zlen[2], int B, int zh, int zw, float* xr_dev, float* xd_dev)
{
    return run_decompress_impl(ys, ylen, n_y, zs, zlen, B, zh * 4, zw * 4, xr_dev, xd_dev, nullptr);
}

int rgbd_elic::run_decompress_impl(const uint8_t* const* ys[2], const int64_t* ylen[2], int n_y,
                                   const uint8_t* const* zs[2], const int64_t* zlen[2], int B, int h, int w,
                                   float* xr_dev, float* xd_dev, const Latents* lat)
{
    const int zh = lat ? 1 : h / 4, zw = lat ? 1 : w / 4, H = h * 16, W = w * 16;
    const int64_t T = (int64_t)M * h * w, Tz = (int64_t)N * zh * zw;
    const int per_image = (n_y == B && !(B == 1)) ? 1 : (n_y == 1 ? (B == 1 ? 1 : 0) : -1);
    if (per_image < 0) return RGBD_EINVAL;
    begin_call(per_image == 0 ? B : 1, false);

    // ==== prologue (never captured): upload the streams ================================================================
    const int ns_y = n_y, ns_z = lat ? 0 : B;
    DecBufs d;
    if (const int r = dec_streams(2, ys, ylen, ns_y, zs, zlen, ns_z, B, T, Tz, per_image, &d)) return r;

    Act hyp_r, hyp_d;
    if (lat) {
        hyp_r = alloc(B, h, w, 2 * M);
        hyp_d = alloc(B, h, w, 2 * M);
        if (!dry()) {
            int r = launch_nchw_to_nhwc16(lat->hyp[0], B, 2 * M, h, w, hyp_r.p, hyp_r.cs, s, perm());
            if (!r) r = launch_nchw_to_nhwc16(lat->hyp[1], B, 2 * M, h, w, hyp_d.p, hyp_d.cs, s, perm());
            if (r) return r;
        }
    }

    // ==== body: captured into / replayed from a HIP graph per call shape ================================================
    Act out0, out1;  // what the epilogue hands back: x_hat (or y_hat for decompress_united) per modality
    if (body_begin()) {
        if (!lat) {
            Act zh_r = alloc(B, zh, zw, N), zh_d = alloc(B, zh, zw, N);
            z_decode(0, "rgb_", d, zh_r);
            z_decode(1, "depth_", d, zh_d);
            named["zhat_r"] = zh_r;
            named["zhat_d"] = zh_d;

            if (variant == 3) h_s_r2d(zh_r, zh_d, &hyp_r, &hyp_d);
            else h_s(zh_r, zh_d, &hyp_r, &hyp_d);
        }
        named["hyper_r"] = hyp_r;
        named["hyper_d"] = hyp_d;
        Act yhat_r = alloc(B, h, w, M), yhat_d = alloc(B, h, w, M);
        if (variant == 2 && !dry()) {  // 24-wide slices: a 16-channel read chunk may straddle into a slice not coded yet
            int zr = launch_fill_zero(yhat_r.p, yhat_r.elems(), s);
            if (!zr) zr = launch_fill_zero(yhat_d.p, yhat_d.elems(), s);
            if (zr) fail(zr);
        }
        named["yhat_r"] = yhat_r;
        named["yhat_d"] = yhat_d;
        Coding cd = dec_coding(d, per_image, T, ns_y);
        if (variant == 3) bicee_r2d(cd, nullptr, nullptr, hyp_r, hyp_d, yhat_r, yhat_d);
        else bicee(cd, nullptr, nullptr, hyp_r, hyp_d, yhat_r, yhat_d);
        if (lat) {  // decompress_united ends here: y_hat back to the caller
            out0 = yhat_r;
            out1 = yhat_d;
        } else {
            if (variant == 2) g_s_stf(yhat_r, yhat_d, &out0, &out1);
            else if (variant == 3) g_s_r2d(yhat_r, yhat_d, &out0, &out1);
            else g_s(yhat_r, yhat_d, &out0, &out1);
        }
        if (cur_ge && !dry()) {
            cur_ge->out[0] = out0;
            cur_ge->out[1] = out1;
        }
    } else {
        out0 = cur_ge->out[0];
        out1 = cur_ge->out[1];
    }
    if (const int r = finish_body()) return r;
    if (dry()) return RGBD_OK;

    // ==== epilogue (never captured): results into the caller's NCHW tensors ==========================================
    if (lat) {
        int r = launch_nhwc_to_nchw_clamp(out0.p, B, M, h, w, out0.cs, lat->yhat[0], 0, s, perm());
        if (!r) r = launch_nhwc_to_nchw_clamp(out1.p, B, M, h, w, out1.cs, lat->yhat[1], 0, s, perm());
        return r;
    }
    int r = launch_nhwc_to_nchw_clamp(out0.p, B, 3, H, W, out0.cs, xr_dev, 1, s);
    if (!r) r = launch_nhwc_to_nchw_clamp(out1.p, B, 1, H, W, out1.cs, xd_dev, 1, s);
    return r;
}

// ---- the single-modal families: ELIC (variant 1, models/elic.py), STF (4, models/stf.py) and the checkerboard Cheng2020
// (5, models/Cheng2020withCKBD.py) share one call path per direction; a family enters through the four hooks below ----------
Act rgbd_elic::g_a_single(const Act& x)
{
    switch (variant) {
    case 4: return g_a_stf1(x);
    case 5: return g_a_ckbd(x);
    default: return g_a1(x);
    }
}

Act rgbd_elic::h_a_single(const Act& y)
{
    switch (variant) {
    case 4: return h_a_stf1(y);
    case 5: return h_a_ckbd(y);
    default: return h_a1(y);
    }
}

Act rgbd_elic::g_s_single(const Act& yhat)
{
    switch (variant) {
    case 4: return g_s_stf1(yhat);
    case 5: return g_s_ckbd(yhat);
    default: return g_s1(yhat);
    }
}

// The latent stage: everything between z_hat and y_hat -- the family's buffers, its hyper synthesis, its debug tensors and its
// coding loop (symbols when cd.encode, from the streams when not, likelihoods into cd.lik[0] when cd.estimate).
//   ELIC: y_hat = round(y - mean) + mean slice by slice through the two-part checkerboard loop (elic.py:180-251 / 268-316).
//   STF: the y stream is ONE stream for all slices of all images of the call (per-image streams: one per image), coded after
//     the last slice; the decoder resumes its rANS state slice by slice.  A batch decompresses as the inverse of compress()
//     (the reference's decompress handles one image only, stf.py:799).
//   Checkerboard: both halves of all images of the call go into ONE y stream, anchor half first (per-image streams: one per
//     image, each with its own two halves); the decoder resumes its rANS state between the halves.
void rgbd_elic::latent_single(Coding& cd, const Act* y, const Act& zhat, Act* yhat)
{
    const int B = zhat.n, h = 4 * zhat.h, w = 4 * zhat.w;
    switch (variant) {
    case 4: {
        const int wide = M + (kStfSupport + 1) * kStfSliceCh;
        Act ctxm = alloc(B, h, w, wide), ctxs = alloc(B, h, w, wide);
        *yhat = alloc(B, h, w, M);
        {
            const size_t mark = arena.top;
            h_s_stf1(zhat, view(ctxm, 0, M), view(ctxs, 0, M));
            arena.top = mark;
        }
        named["latent_means"] = view(ctxm, 0, M);
        named["latent_scales"] = view(ctxs, 0, M);
        if (cd.estimate) cd.lik[0] = alloc(B, h, w, M);
        slice_loop(cd, y, ctxm, ctxs, *yhat);
        break;
    }
    case 5: {
        Act cat = alloc(B, h, w, 4 * M), params = alloc(B, h, w, 2 * M);
        *yhat = alloc(B, h, w, M);
        named["hyper"] = view(cat, 2 * M, 2 * M);
        named["ctx"] = view(cat, 0, 2 * M);
        named["scales"] = view(params, 0, M);
        named["means"] = view(params, M, M);
        if (!cd.estimate) {
            if (!dry() && !rc) {
                const int r = launch_fill_zero(cat.p, cat.elems(), s);
                if (r) fail(r);
            }
            h_s_ckbd(zhat, view(cat, 2 * M, 2 * M));
            two_pass_ckbd(cd, y, cat, params, *yhat);
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
                r = launch_ckbd_estimate_part(y->p, y->cs, params.p, params.cs, yhat->p, yhat->cs, lik.p, lik.cs, g, s);
            }
            if (r) fail(r);
        }
        h_s_ckbd(zhat, view(cat, 2 * M, 2 * M));
        ck_context(*yhat, view(cat, 0, 2 * M));
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
    default: {
        Act hyper = h_s1(zhat);
        named["hyper"] = hyper;
        *yhat = alloc(B, h, w, M);
        if (cd.estimate) cd.lik[0] = alloc(B, h, w, M);
        bicee1(cd, y, hyper, *yhat);
    }
    }
    named["yhat"] = *yhat;
}

// compress: elic.py:161-253, stf.py:703-764, Cheng2020withCKBD.py:101-136
int rgbd_elic::run_compress_single(const float* x_dev, int B, int H, int W, int per_image)
{
    const int h = H / 16, w = W / 16, zh = H / 64, zw = W / 64;
    const int64_t T = (int64_t)M * h * w, Tz = (int64_t)N * zh * zw;
    begin_call(per_image ? 1 : B, false);

    // ==== prologue (never captured): workspace of the call, upload of the stream geometry, input layout conversion ====
    EncBufs e;
    if (const int r = enc_streams(1, B, T, Tz, per_image, &e)) return r;
    int32_t *fy = nullptr, *fz = nullptr;  // (only the checkerboard family accepts forced symbols)
    if (const int r = upload_forced(1, force_y, (size_t)(B * T), &fy)) return r;
    if (const int r = upload_forced(1, force_z, (size_t)(B * Tz), &fz)) return r;
    Act x = alloc(B, H, W, in_ch);
    if (!dry()) {
        const int r = launch_nchw_to_nhwc16(x_dev, B, in_ch, H, W, x.p, x.cs, s);
        if (r) return r;
    }
    // ==== body: captured into / replayed from a HIP graph per call shape ================================================
    if (body_begin()) {
        if (!dry()) {
            const int zr = launch_fill_zero((float*)e.err, 64, s);  // (a kernel, not a memset node: DESIGN 3.5)
            if (zr) fail(zr);
        }
        Act y = alloc(B, h, w, M);
        {
            const size_t mark = arena.top;
            copy_ch(g_a_single(x), y);
            arena.top = mark;
        }
        Act z = h_a_single(y);
        named["y"] = y;
        named["z"] = z;
        Act zhat = alloc(B, zh, zw, N), yhat;
        z_encode(0, "", e, z, zhat, fz);
        named["zhat"] = zhat;
        Coding cd = enc_coding(e, per_image, T, fy);
        latent_single(cd, &y, zhat, &yhat);
        y_encode(1, B, e);
    }
    if (const int r = finish_body()) return r;
    if (dry()) return RGBD_OK;

    // ==== epilogue (never captured): fetch the streams ================================================================
    return fetch_streams(1, B, true, e);
}

// eval-mode forward(): elic.py:60-161 (quant = "ste"), stf.py:618-678, Cheng2020withCKBD.py:52-71; Gaussian / factorised
// likelihoods instead of symbols
int rgbd_elic::run_forward_single(const float* x_dev, int B, int H, int W, float* xhat_dev, float* ly, float* lz)
{
    const int h = H / 16, w = W / 16, zh = H / 64, zw = W / 64;
    begin_call(B, true);
    Act x = alloc(B, H, W, in_ch);
    if (!dry()) {
        const int r = launch_nchw_to_nhwc16(x_dev, B, in_ch, H, W, x.p, x.cs, s);
        if (r) return r;
    }
    Act xh, lik, zlik;
    if (body_begin()) {  // (captured / replayed per call shape like every other body)
        Act y = alloc(B, h, w, M);
        {
            const size_t mark = arena.top;
            copy_ch(g_a_single(x), y);
            arena.top = mark;
        }
        Act z = h_a_single(y);
        named["y"] = y;
        named["z"] = z;
        Act zhat = alloc(B, zh, zw, N), yhat;
        zlik = alloc(B, zh, zw, N);
        z_estimate("", z, zhat, zlik);
        named["zhat"] = zhat;
        Coding cd;
        cd.estimate = true;
        latent_single(cd, &y, zhat, &yhat);
        xh = g_s_single(yhat);
        lik = cd.lik[0];
        if (cur_ge && !dry()) {
            cur_ge->out[0] = xh;
            cur_ge->out[1] = lik;
            cur_ge->out[2] = zlik;
        }
    } else {
        xh = cur_ge->out[0];
        lik = cur_ge->out[1];
        zlik = cur_ge->out[2];
    }
    if (const int r = finish_body()) return r;
    if (dry()) return RGBD_OK;
    int r = launch_nhwc_to_nchw_clamp(xh.p, B, in_ch, H, W, xh.cs, xhat_dev, 0, s);  // (stf.py:677: not clamped)
    if (!r) r = launch_nhwc_to_nchw_clamp(lik.p, B, M, h, w, lik.cs, ly, 0, s, perm());
    if (!r) r = launch_nhwc_to_nchw_clamp(zlik.p, B, N, zh, zw, zlik.cs, lz, 0, s, perm());
    if (!r) r = wait_stream();
    return r;
}

// decompress: elic.py:255-325, stf.py:766-816, Cheng2020withCKBD.py:138-174
int rgbd_elic::run_decompress_single(const uint8_t* const* ys, const int64_t* ylen, int n_y, const uint8_t* const* zs,
                                     const int64_t* zlen, int B, int zh, int zw, float* x_out)
{
    const int h = zh * 4, w = zw * 4, H = zh * 64, W = zw * 64;
    const int64_t T = (int64_t)M * h * w, Tz = (int64_t)N * zh * zw;
    const int per_image = (n_y == B) ? 1 : 0;
    begin_call(per_image ? 1 : B, false);

    // ==== prologue (never captured): upload the streams ================================================================
    DecBufs d;
    if (const int r = dec_streams(1, &ys, &ylen, n_y, &zs, &zlen, B, B, T, Tz, per_image, &d)) return r;

    // ==== body: captured into / replayed from a HIP graph per call shape ================================================
    Act xh;
    if (body_begin()) {
        Act zhat = alloc(B, zh, zw, N), yhat;
        z_decode(0, "", d, zhat);
        named["zhat"] = zhat;
        Coding cd = dec_coding(d, per_image, T, n_y);
        latent_single(cd, nullptr, zhat, &yhat);
        xh = g_s_single(yhat);
        if (cur_ge && !dry()) cur_ge->out[0] = xh;
    } else {
        xh = cur_ge->out[0];
    }
    if (const int r = finish_body()) return r;
    if (dry()) return RGBD_OK;

    // ==== epilogue (never captured): x_hat into the caller's NCHW tensor; not clamped in elic.py:318-325 and
    // Cheng2020withCKBD.py:167-174, clamped to [0, 1] in stf.py:815
    return launch_nhwc_to_nchw_clamp(xh.p, B, in_ch, H, W, xh.cs, x_out, variant == 4 ? 1 : 0, s);
}
