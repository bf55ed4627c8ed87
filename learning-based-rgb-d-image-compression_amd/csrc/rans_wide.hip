// Wide rANS: the opt-in lane-interleaved stream format.  L Rans64 states (L = 1, 2, 4 ... 64), one lane of
// one wavefront per state, with the arithmetic of third_party/ryg_rans/rans64.h:59-142 and the escape coding of
// cpp_exts/rans/rans_interface.cpp:60-96,119-163 unchanged.  The format is fixed by its decoder:
//   * a stream codes a sequence of segments; inside a segment symbol i belongs to lane i mod L and row i div L;
//   * a symbol expands into items: item 0 is the table symbol, for the escape slot one count nibble and up to 8 payload
//     nibbles follow (int32 symbols need no more; a count above 8 is a damaged stream);
//   * start-up: lane l loads x_l = w[2l] | w[2l+1] << 32, pos = 2L;
//   * for every row and round j = 0, 1, ...: the lanes whose symbol has an item j decode it on their own state; those whose
//     state fell below 2^31 take one word each from pos upward in increasing lane order; the row ends with its last item.
// The encoder is the unique inverse (segments, rows and rounds backwards, words written downwards in decreasing lane order,
// lanes L-1 ... 0 flushed last).  With L = 1 and one segment this is the reference's stream byte for byte.
#include <mutex>

#include "common.h"

#define WR_LOW (1ull << 31)
#define WR_MAX_NIB 8  // payload nibbles of an int32 symbol

namespace {

__device__ __forceinline__ uint32_t wr_first(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// ---------------------------------------------------------------------------------------------
// Encoder: one wavefront per stream.  Rows are walked backwards over all segments; the operands of a row are fetched two
// rows ahead (symbol / index from HBM) and one row ahead (row geometry from LDS, gather of the reciprocal entry), so the
// state chain of the row being coded never waits for memory.
struct WRowIt {  // (segment, row) walking backwards; off = first symbol of the segment inside the stream
    int seg;
    int64_t row, off;
};

struct WRaw {
    int ti, sv;
    bool valid;
};

struct WItems {
    uint32_t mlo, mhi, w2, freq;  // DevTables::enc entry of the table symbol
    uint32_t raw;                 // escape payload
    int nitems;                   // 0: no symbol in this lane; 1: table symbol; 2 + nibbles: escape
    int nn;
};

__device__ __forceinline__ void wr_step(WRowIt& it, const int64_t* segc, int lgL)
{
    --it.row;
    while (it.row < 0 && it.seg >= 0) {
        --it.seg;
        if (it.seg < 0) break;
        const int64_t c = segc[it.seg];
        it.off -= c;
        it.row = ((c + ((int64_t)1 << lgL) - 1) >> lgL) - 1;
    }
}

__device__ __forceinline__ WRaw wr_load(const int32_t* __restrict__ sym, const int32_t* __restrict__ idx, int64_t base,
                                        const WRowIt& it, const int64_t* segc, int lane, int L, int lgL)
{
    WRaw r;
    r.ti = r.sv = 0;
    r.valid = false;
    if (it.seg >= 0 && lane < L) {
        const int64_t i = (it.row << lgL) + lane;
        if (i < segc[it.seg]) {
            r.valid = true;
            r.ti = idx[base + it.off + i];
            r.sv = sym[base + it.off + i];
        }
    }
    return r;
}

__device__ __forceinline__ WItems wr_finish(const DevTables& t, const int3* rowmeta, const WRaw& r)
{
    WItems b;
    b.mlo = b.mhi = ~0u;
    b.w2 = 65535u;
    b.freq = 1u;
    b.raw = 0;
    b.nitems = 0;
    b.nn = 0;
    if (r.valid) {
        const int3 rm = rowmeta[r.ti];  // {row_off, cdf_length, offset}
        const int top = rm.y - 2;
        int v = r.sv - rm.z;  // rans_interface.cpp:119-128
        uint32_t raw = 0;
        if (v < 0) {
            raw = (uint32_t)(-2 * v - 1);
            v = top;
        } else if (v >= top) {
            raw = (uint32_t)(2 * (v - top));
            v = top;
        }
        const uint4 e = reinterpret_cast<const uint4*>(t.enc)[rm.x + v];
        b.mlo = e.x;
        b.mhi = e.y;
        b.w2 = e.z;
        b.freq = e.w;
        b.raw = raw;
        b.nitems = 1;
        if (v == top) {  // rans_interface.cpp:139-162: the count, then the nibbles
            int nn = 0;
            while (nn < WR_MAX_NIB && (raw >> (nn * 4)) != 0) ++nn;
            b.nn = nn;
            b.nitems = 2 + nn;
        }
    }
    return b;
}

__global__ __launch_bounds__(64) void rans_wide_encode_kernel(const int32_t* __restrict__ sym, const int32_t* __restrict__ idx,
                                                              const int64_t* __restrict__ sym_base, int split, DevTables t0,
                                                              DevTables t1, WideSegs segs, int L, int lgL,
                                                              uint32_t* __restrict__ out, int64_t cap_words,
                                                              int64_t* __restrict__ out_words, int* __restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char wsm[];
    __shared__ int64_t segc[WIDE_MAX_SEGS];
    int3* rowmeta = reinterpret_cast<int3*>(wsm);
    const int s = blockIdx.x;
    const int lane = threadIdx.x;
    const DevTables& t = s < split ? t0 : t1;
    const int64_t base = sym_base[s];
    uint32_t* o = out + (size_t)s * cap_words;  // the stream's slot: every store below lands in o[0, cap_words)
    int w = (int)cap_words;                     // next free word is w - 1 (cap_words < 2^31: checked by the launcher)
    uint64_t x = WR_LOW;                        // Rans64EncInit
    bool bad = false;

    for (int i = lane; i < t.nrows; i += 64) rowmeta[i] = make_int3(t.row_off[i], t.sizes[i], t.offsets[i]);
    if (lane < WIDE_MAX_SEGS) segc[lane] = lane < segs.n ? segs.count[lane] : 0;
    __syncthreads();
    int64_t total = 0;
    for (int k = 0; k < segs.n; ++k) total += segc[k];

    // words of the lanes in `em`, highest lane first at the highest address (the decoder reads upwards in lane order)
    auto emit = [&](bool em) {
        const uint64_t bm = __ballot(em);
        if (!bm) return;
        const int cnt = __popcll(bm);
        if (cnt > w) {  // the slot is full: nothing is written outside it
            bad = true;
            return;
        }
        if (em) {
            const int above = __popcll((bm >> lane) >> 1);
            o[w - 1 - above] = (uint32_t)x;
            x >>= 32;
        }
        w -= cnt;
    };

    WRowIt it = {segs.n, -1, total};
    wr_step(it, segc, lgL);
    WItems cur = wr_finish(t, rowmeta, wr_load(sym, idx, base, it, segc, lane, L, lgL));
    bool more = it.seg >= 0;
    wr_step(it, segc, lgL);
    WRaw raw1 = wr_load(sym, idx, base, it, segc, lane, L, lgL);
    wr_step(it, segc, lgL);
    while (more && !bad) {
        const WItems nxt = wr_finish(t, rowmeta, raw1);  // the row before this one: its symbols arrived last round
        const bool more_nxt = __ballot(raw1.valid) != 0;
        raw1 = wr_load(sym, idx, base, it, segc, lane, L, lgL);  // two rows ahead: in flight during this round
        wr_step(it, segc, lgL);
        // rounds 9 ... 1: escape items, payload nibbles from the top down, then the count (Rans64EncPutBits with 4 bits)
        if (__ballot(cur.nitems > 1)) {
            for (int j = 1 + WR_MAX_NIB; j >= 1 && !bad; --j) {
                const bool act = cur.nitems > j;
                if (!__ballot(act)) continue;
                emit(act && x >= (1ull << 59));  // ((RANS64_L >> 16) << 32) << 12, rans_interface.cpp:67-69
                if (bad) break;
                const uint32_t val = j == 1 ? (uint32_t)cur.nn : ((cur.raw >> ((j - 2) * 4)) & 15u);
                if (act) x = (x << 4) | val;
            }
        }
        if (bad) break;
        // round 0: the table symbol (Rans64EncPut, rans64.h:77-94) with the reciprocal of DevTables::enc
        {
            const bool act = cur.nitems > 0;
            emit(act && (uint32_t)(x >> 47) >= cur.freq);
            if (bad) break;
            if (act) {
                const uint64_t m = (uint64_t)cur.mlo | ((uint64_t)cur.mhi << 32);
                const uint64_t q = __umul64hi(x, m) >> (cur.w2 >> 17);
                x = x + (cur.w2 & 0x1FFFFu) + q * (uint64_t)(65536u - cur.freq);
            }
        }
        cur = nxt;
        more = more_nxt;
    }
    // Rans64EncFlush of lanes L-1 ... 0 (rans64.h:96-103): lane 0's state heads the stream
    if (!bad && 2 * L > w) bad = true;
    if (bad) {
        if (lane == 0) {
            *err = 1;
            out_words[s] = 0;
        }
        return;
    }
    w -= 2 * L;
    if (lane < L) {
        o[w + 2 * lane] = (uint32_t)x;
        o[w + 2 * lane + 1] = (uint32_t)(x >> 32);
    }
    if (lane == 0) out_words[s] = cap_words - w;
}

// ---------------------------------------------------------------------------------------------
// Decoder: one wavefront per stream, four streams per workgroup sharing the tables in LDS (the bucket table DevTables::lut,
// the probe rows DevTables::cm and the row geometry).  A call decodes ONE segment of `count` symbols; the L states and the
// read position live in state[s * (L + 1) ...] between calls.
//   * the symbol search of a lane: the bucket entries of cum's bucket and of the next one bracket the answer, a binary
//     search over cm between them finds it -- at most log2(row size) steps, all inside the row;
//   * stream words come through a 128-word register window (two words per lane) that is refilled 64 words ahead, so a
//     round's reads are two lane permutes; every global read is clamped to the stream's length (a word past the end reads
//     as 0 and raises *err);
//   * a count nibble above 8 cannot come from the encoder: it raises *err and the symbol ends there.
__global__ __launch_bounds__(256) void rans_wide_decode_kernel(const uint32_t* __restrict__ streams,
                                                               const int64_t* __restrict__ stream_off,
                                                               const int64_t* __restrict__ stream_len,
                                                               uint64_t* __restrict__ state, int init,
                                                               const int32_t* __restrict__ idx, int32_t* __restrict__ sym,
                                                               const int64_t* __restrict__ sym_base, int64_t part_off,
                                                               int64_t count, DevTables t, int nstreams, int spw, int L, int lgL,
                                                               int* __restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char wdm[];
    const int lut_n = (1 << t.lut_bits) + 1;
    uint2* sl = reinterpret_cast<uint2*>(wdm);                                   // [nrows][lut_n] bucket table
    int4* rowinfo = reinterpret_cast<int4*>(sl + ((t.nrows * lut_n + 1) & ~1));  // [nrows] {row start in cm, escape slot, offset}
    uint16_t* cm = reinterpret_cast<uint16_t*>(rowinfo + t.nrows);               // [t.total + 64 * nrows]
    const int tid = threadIdx.x;
    const int s = blockIdx.x * spw + (tid >> 6);
    {
        const int ncm16 = ((t.total + 64 * t.nrows) * 2 + 15) / 16;  // (the image is padded to 16 bytes: build_tables)
        const uint4* gcm = reinterpret_cast<const uint4*>(t.cm);
        uint4* lcm = reinterpret_cast<uint4*>(cm);
        for (int i = tid; i < ncm16; i += 256) lcm[i] = gcm[i];
        const uint2* gl = reinterpret_cast<const uint2*>(t.lut);
        for (int i = tid; i < t.nrows * lut_n; i += 256) sl[i] = gl[i];
        for (int i = tid; i < t.nrows; i += 256) rowinfo[i] = make_int4(t.row_off[i] + 64 * i, t.sizes[i] - 2, t.offsets[i], 0);
    }
    __syncthreads();
    if ((tid >> 6) >= spw || s >= nstreams) return;
    const int lane = tid & 63;

    const uint32_t* st = streams + stream_off[s];
    const int64_t nwords = stream_len[s];
    auto rd = [&](int64_t p) -> uint32_t { return (p >= 0 && p < nwords) ? st[p] : 0u; };
    uint64_t* sp = state + (size_t)s * (L + 1);
    bool bad = false;
    uint64_t x = 0;
    int64_t pos;
    if (init) {  // Rans64DecInit of every lane (rans64.h:107-115)
        if (lane < L) x = (uint64_t)rd(2 * lane) | ((uint64_t)rd(2 * lane + 1) << 32);
        pos = 2 * L;
    } else {
        if (lane < L) x = sp[lane];
        pos = (int64_t)sp[L];
    }
    pos = (int64_t)((uint64_t)wr_first((uint32_t)pos) | ((uint64_t)wr_first((uint32_t)((uint64_t)pos >> 32)) << 32));
    if (pos < 2 * L) {  // (a state buffer nobody initialised)
        bad = true;
        pos = 2 * L;
    }
    const int64_t base = sym_base[s] + part_off;
    const int shift = 16 - t.lut_bits;

    // word window: lane k of wcur holds word wbase + k, wnext the 64 words behind them; wi (< 64) = next unread word
    int64_t wbase = pos;
    int wi = 0;
    uint32_t wcur = rd(wbase + lane), wnext = rd(wbase + 64 + lane);
    auto consume = [&](bool need) {  // the lanes in `need` renormalise: one word each, in increasing lane order
        const uint64_t bm = __ballot(need);
        if (!bm) return;
        const int k = wi + __popcll(bm & (((uint64_t)1 << lane) - 1));  // <= 63 + 63
        const uint32_t a = (uint32_t)__shfl((int)wcur, k & 63), b = (uint32_t)__shfl((int)wnext, k & 63);
        if (need) x = (x << 32) | (k < 64 ? a : b);
        wi += __popcll(bm);
        if (wi >= 64) {
            wi -= 64;
            wbase += 64;
            wcur = wnext;
            wnext = rd(wbase + 64 + lane);
        }
    };

    const int64_t rows = (count + ((int64_t)1 << lgL) - 1) >> lgL;
    int ti_n = (lane < L && lane < count) ? idx[base + lane] : 0;
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t i = (r << lgL) + lane;
        const bool valid = lane < L && i < count;
        int ti = ti_n;
        ti_n = (lane < L && i + L < count) ? idx[base + i + L] : 0;  // the next row's indexes: in flight during this one
        if (ti < 0 || ti >= t.nrows) {
            bad = true;
            ti = 0;
        }
        const int4 ri = rowinfo[ti];
        const int ro = ri.x, last = ri.y;
        // round 0: the table symbol (Rans64DecGet / Rans64DecAdvance, rans64.h:117-142)
        int v = 0;
        bool need = false;
        if (valid) {
            const uint32_t cum = (uint32_t)x & 0xFFFFu;
            const uint2* e = sl + ti * lut_n + (int)(cum >> shift);
            int lo = (int)(e[0].x & 0xFFFFu), hi = (int)(e[1].x & 0xFFFFu);
            hi = hi < last ? hi : last;
            while (lo < hi) {  // largest slot whose start is <= cum; cm holds start - 1
                const int mid = (lo + hi + 1) >> 1;
                if ((uint32_t)cm[ro + mid] < cum) lo = mid;
                else hi = mid - 1;
            }
            const uint32_t start = lo ? (uint32_t)cm[ro + lo] + 1u : 0u;
            const uint32_t freq = (uint32_t)cm[ro + lo + 1] + 1u - start;  // (the pad behind the row reads 65536 - 1)
            x = (uint64_t)freq * (x >> 16) + (cum - start);
            need = x < WR_LOW;
            v = lo;
        }
        consume(need);
        // rounds 1 ...: the escape items (rans_interface.cpp:323-345): one count nibble, then the payload
        const bool esc = valid && v == last;
        if (__ballot(esc)) {
            int nn = 0;
            uint32_t raw = 0;
            need = false;
            if (esc) {
                nn = (int)((uint32_t)x & 15u);
                x >>= 4;
                need = x < WR_LOW;
            }
            consume(need);
            if (nn > WR_MAX_NIB) {
                bad = true;
                nn = 0;
            }
            for (int k = 0; k < WR_MAX_NIB; ++k) {
                const bool act = esc && k < nn;
                if (!__ballot(act)) break;
                need = false;
                if (act) {
                    raw |= ((uint32_t)x & 15u) << (4 * k);
                    x >>= 4;
                    need = x < WR_LOW;
                }
                consume(need);
            }
            if (esc) {
                v = (int)(raw >> 1);
                v = (raw & 1u) ? -v - 1 : v + last;
            }
        }
        if (valid) sym[base + i] = v + ri.z;
    }
    pos = wbase + wi;
    if (pos > nwords) bad = true;  // words past the end were read as 0
    if (lane < L) sp[lane] = x;
    if (lane == 0) sp[L] = (uint64_t)pos;
    if (__ballot(bad) && lane == 0) *err = 1;
}

size_t wide_decode_lds_bytes(const DevTables& t)
{
    const size_t lut_n = ((size_t)1 << t.lut_bits) + 1;
    return (((size_t)t.nrows * lut_n + 1) & ~(size_t)1) * 8 + (size_t)t.nrows * 16 +
           ((((size_t)t.total + 64 * (size_t)t.nrows) * 2 + 15) & ~(size_t)15);
}

}  // namespace

int wide_lanes_log2(int lanes)
{
    for (int lg = 0; lg <= 6; ++lg)
        if (lanes == (1 << lg)) return lg;
    return -1;
}

int launch_rans_wide_encode(const int32_t* sym, const int32_t* idx, const int64_t* sym_base, const WideSegs& segs, int lanes,
                            int nstreams, int split, DevTables t0, DevTables t1, uint32_t* out, int64_t cap_words,
                            int64_t* out_words, int* err, hipStream_t s)
{
    const int lg = wide_lanes_log2(lanes);
    if (lg < 0 || segs.n < 1 || segs.n > WIDE_MAX_SEGS) return RGBD_EINVAL;
    for (int k = 0; k < segs.n; ++k)
        if (segs.count[k] < 0) return RGBD_EINVAL;
    if (nstreams <= 0) return RGBD_OK;
    if (cap_words < 2 * lanes || cap_words >= ((int64_t)1 << 31)) return RGBD_EINVAL;
    const size_t lds = sizeof(int3) * (size_t)(t0.nrows > t1.nrows ? t0.nrows : t1.nrows);
    if (lds > 60 * 1024) return RGBD_ENOSPC;
    hipLaunchKernelGGL(rans_wide_encode_kernel, dim3(nstreams), dim3(64), lds, s, sym, idx, sym_base, split, t0, t1, segs, lanes, lg,
                       out, cap_words, out_words, err);
    HIP_TRY(hipGetLastError());
    return RGBD_OK;
}

int launch_rans_wide_decode(const uint32_t* streams, const int64_t* stream_off_words, const int64_t* stream_len_words,
                            int nstreams, int lanes, uint64_t* state, int init, const int32_t* idx, int32_t* sym,
                            const int64_t* sym_base, int64_t part_off, int64_t count, DevTables t, int* err, hipStream_t s)
{
    const int lg = wide_lanes_log2(lanes);
    if (lg < 0 || count < 0) return RGBD_EINVAL;
    if (nstreams <= 0 || count == 0) return RGBD_OK;
    const size_t lds = wide_decode_lds_bytes(t);
    if (lds > 158 * 1024 || t.nrows * (((size_t)1 << t.lut_bits) + 1) > 65535 || t.total + 64 * t.nrows > 65535) return RGBD_ENOSPC;
    {   // the attribute is per device and this is called from several host threads (CodecPool)
        static std::mutex mu;
        static bool configured[64] = {false};
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(mu);
        if (dev < 0 || dev >= 64 || !configured[dev]) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(rans_wide_decode_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            if (dev >= 0 && dev < 64) configured[dev] = true;
        }
    }
    const int spw = nstreams <= 2 ? 1 : 4;
    hipLaunchKernelGGL(rans_wide_decode_kernel, dim3((nstreams + spw - 1) / spw), dim3(256), lds, s, streams, stream_off_words,
                       stream_len_words, state, init, idx, sym, sym_base, part_off, count, t, nstreams, spw, lanes, lg, err);
    HIP_TRY(hipGetLastError());
    return RGBD_OK;
}
