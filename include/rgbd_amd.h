/*
 * rgbd_amd.h -- C ABI of the MI355X-native ELIC_united encode/decode path.
 *
 * Shared library: learning-based-rgb-d-image-compression_amd/librgbd_amd.so (built by __graft_entry__.build()).
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative errno-style code
 * (-22 invalid argument, -12 out of memory, -28 buffer too small, -5 HIP runtime error, -1 wrong call order);
 * no exceptions cross the boundary; a handle may be used from one thread at a time.  "dev" pointers are HIP device
 * pointers (e.g. torch tensor .data_ptr() on ROCm); all others are host pointers.  `stream` is a hipStream_t passed
 * as void* (NULL = default stream).
 *
 * Each entry point names the reference interface it stands in for (paths relative to the reference repository).
 */
#ifndef RGBD_AMD_H
#define RGBD_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGBD_AMD_ABI_VERSION 1

int rgbd_abi_version(void);

/* Host-side wait policy of the current HIP device: 1 = host threads that wait for the GPU sleep (blocking sync) instead
 * of spinning.  No reference counterpart (the reference drives one image at a time from one thread); a pooled rank
 * keeps 16 host threads waiting on 16 streams, and 8 ranks share one host. */
int rgbd_set_blocking_sync(int32_t on);
/* The policy in force on the current device: 1 blocking sync, 0 anything else, negative on error (tests: CodecPool.close()
 * must give the device its default policy back). */
int rgbd_get_blocking_sync(void);

/* ---------------------------------------------------------------------------------------------------------------
 * Table construction (host, one-off).
 * Replaces compressai._CXX.pmf_to_quantized_cdf -- CompressAI/compressai/cpp_exts/ops/ops.cpp:24-81, bound at
 * ops.cpp:83-90 and called from entropy_models.py:60-63.   cdf_out receives n+1 entries.
 * ------------------------------------------------------------------------------------------------------------- */
int rgbd_pmf_to_quantized_cdf(const float* pmf, int32_t n, int32_t precision, uint32_t* cdf_out);

/* ---------------------------------------------------------------------------------------------------------------
 * Stand-alone rANS coder on the GPU (host buffers in / out).
 * Replaces compressai.ans.{RansEncoder,BufferedRansEncoder,RansDecoder} --
 * CompressAI/compressai/cpp_exts/rans/rans_interface.cpp:99-205 (encode_with_indexes + flush),
 * :207-276 (decode_with_indexes), :278-351 (set_stream / decode_stream), bound at :353-373.
 * cdf is row-major [n_cdf][cdf_stride] int32; cdf_sizes / offsets have n_cdf entries.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct rgbd_tables rgbd_tables; /* packed CDF rows + search accelerator resident in HBM */

int rgbd_tables_create(const int32_t* cdf, int32_t cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                       int32_t n_cdf, rgbd_tables** out);
void rgbd_tables_destroy(rgbd_tables* t);

/* Worst-case stream size in bytes for n symbols (escape-heavy input). */
int64_t rgbd_rans_max_bytes(int64_t n);

/* One stream from n (symbol, index) pairs.  out_len receives the byte count (multiple of 4, >= 8). */
int rgbd_rans_encode(const rgbd_tables* t, const int32_t* symbols, const int32_t* indexes, int64_t n, uint8_t* out,
                     int64_t cap, int64_t* out_len);

typedef struct rgbd_rans_decoder rgbd_rans_decoder;
int rgbd_rans_decoder_create(rgbd_rans_decoder** out);
int rgbd_rans_decoder_set_stream(rgbd_rans_decoder* d, const uint8_t* stream, int64_t nbytes);
/* Decodes n symbols for the given table indexes, continuing from the decoder's current state. */
int rgbd_rans_decoder_decode(rgbd_rans_decoder* d, const rgbd_tables* t, const int32_t* indexes, int64_t n,
                             int32_t* symbols_out);
void rgbd_rans_decoder_destroy(rgbd_rans_decoder* d);

/* The same coder with everything resident in HBM and many streams per launch -- what replaces a Python loop of
 * encode_with_indexes() / decode_stream() calls over images and modalities (elic_united.py:374-401, 543-578;
 * rans_interface.cpp:99-192, 286-351).  Every pointer is a DEVICE pointer; nothing is copied or allocated; the launch is
 * asynchronous on `stream` (a hipStream_t; NULL = the default stream).  Indexes must lie in [0, n_cdf): the codec's own
 * producer (rgbd_ckbd_quant_index) guarantees it, the kernels do not check.
 *   encode: stream s codes counts_dev[s] (symbol, index) pairs starting at element sym_base_dev[s] of symbols_dev / indexes_dev
 *           (both readable one element past the last pair).  out_dev holds nstreams slots of cap_words 32-bit words
 *           (cap_words a multiple of 64, >= rgbd_rans_max_bytes(max count) / 4); stream s is the LAST out_words_dev[s] words of
 *           slot s, byte for byte what RansEncoder.flush() returns.  *err_dev (zero it first) becomes non-zero if a slot
 *           overflowed.
 *   decode: stream s is stream_len_words_dev[s] words at word stream_off_words_dev[s] of streams_dev.  state_dev keeps two
 *           uint64 per stream between calls; init != 0 starts from the head of each stream (set_stream()), init == 0
 *           continues (the next decode_stream() on the same decoder).  Each call decodes `count` symbols per stream for the
 *           indexes at indexes_dev[sym_base_dev[s] + part_off ...) into symbols_dev at the same positions. */
int rgbd_rans_encode_batch_dev(const rgbd_tables* t, const int32_t* symbols_dev, const int32_t* indexes_dev,
                               const int64_t* sym_base_dev, const int64_t* counts_dev, int32_t nstreams, uint32_t* out_dev,
                               int64_t cap_words, int64_t* out_words_dev, int32_t* err_dev, void* stream);
int rgbd_rans_decode_batch_dev(const rgbd_tables* t, const uint32_t* streams_dev, const int64_t* stream_off_words_dev,
                               const int64_t* stream_len_words_dev, int32_t nstreams, uint64_t* state_dev, int32_t init,
                               const int32_t* indexes_dev, int32_t* symbols_dev, const int64_t* sym_base_dev, int64_t part_off,
                               int64_t count, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Wide rANS: an opt-in second stream format for callers who want low latency and do not need CompressAI-compatible
 * streams.  `lanes` (L = 1, 2, 4, ... 64) interleaved Rans64 states are coded by one wavefront, one lane per state, with
 * the reference's state arithmetic and escape coding unchanged.  A stream codes a list of at most 32 SEGMENTS; inside a
 * segment symbol i belongs to lane i mod L and row i div L, rows restart at every segment, and one decode call decodes one
 * segment.  The stream starts with the L states (lane 0 first, two words each); per row and item round, the lanes that
 * renormalise take one word each in increasing lane order.  With L = 1 and one segment the stream is the reference's,
 * byte for byte.  A wide stream is 8 * (L - 1) bytes longer than the serial one (504 bytes at L = 64) plus rounding.
 * Refused with RGBD_EINVAL before anything is launched: lanes not a power of two in 1 ... 64, nseg outside 1 ... 32, a
 * negative count, counts that do not sum to n, a stream shorter than 8 * L bytes, a NULL pointer; RGBD_ENOSPC: cap below
 * rgbd_rans_wide_max_bytes(n, lanes).  A decode that runs into a damaged stream (a read past its end, an escape of more
 * than 8 nibbles) reads zeros, stays inside its buffers and returns RGBD_EINVAL / raises *err_dev.
 * ------------------------------------------------------------------------------------------------------------- */
int64_t rgbd_rans_wide_max_bytes(int64_t n, int32_t lanes); /* RGBD_EINVAL for bad arguments */
int rgbd_rans_wide_encode(const rgbd_tables* t, const int32_t* symbols, const int32_t* indexes, int64_t n, int32_t lanes,
                          const int64_t* seg_counts, int32_t nseg, uint8_t* out, int64_t cap, int64_t* out_len);
typedef struct rgbd_rans_wide_decoder rgbd_rans_wide_decoder;
int rgbd_rans_wide_decoder_create(rgbd_rans_wide_decoder** out);
int rgbd_rans_wide_decoder_set_stream(rgbd_rans_wide_decoder* d, const uint8_t* stream, int64_t nbytes, int32_t lanes);
/* Decodes the next segment: n symbols for the given table indexes. */
int rgbd_rans_wide_decoder_decode(rgbd_rans_wide_decoder* d, const rgbd_tables* t, const int32_t* indexes, int64_t n,
                                  int32_t* symbols_out);
void rgbd_rans_wide_decoder_destroy(rgbd_rans_wide_decoder* d);
/* The device-resident pair, as rgbd_rans_{encode,decode}_batch_dev.  encode: every stream codes sum(seg_counts) symbols
 * from sym_base_dev[s] on; streams [0, split) use t0, the others t1; seg_counts is a HOST array, passed to the kernel by
 * value; cap_words >= 2 * lanes (the kernel checks every store: a slot smaller than rgbd_rans_wide_max_bytes / 4 that
 * overflows raises *err_dev and nothing is written outside it).  decode: one segment of `count` symbols per call; state_dev
 * keeps lanes + 1 uint64 per stream between calls; *err_dev (zero it first) is raised on a damaged stream. */
int rgbd_rans_wide_encode_batch_dev(const rgbd_tables* t0, const rgbd_tables* t1, int32_t split, const int32_t* symbols_dev,
                                    const int32_t* indexes_dev, const int64_t* sym_base_dev, int32_t nstreams, int32_t lanes,
                                    const int64_t* seg_counts, int32_t nseg, uint32_t* out_dev, int64_t cap_words,
                                    int64_t* out_words_dev, int32_t* err_dev, void* stream);
int rgbd_rans_wide_decode_batch_dev(const rgbd_tables* t, const uint32_t* streams_dev, const int64_t* stream_off_words_dev,
                                    const int64_t* stream_len_words_dev, int32_t nstreams, int32_t lanes, uint64_t* state_dev,
                                    int32_t init, const int32_t* indexes_dev, int32_t* symbols_dev, const int64_t* sym_base_dev,
                                    int64_t part_off, int64_t count, int32_t* err_dev, void* stream);

/* One checkerboard half of one channel slice on the encoder: utils/ckbd.py:83-105 (ckbd_anchor_sequeeze /
 * ckbd_nonanchor_sequeeze of y, means and scales), entropy_models.py:118-146 (quantize(y, "symbols", means)), :561-568
 * (build_indexes(scales)) and the scatter of y_hat = symbol + mean back onto the full grid (ckbd.py:107-125), as ONE pass.
 * y_dev / means_dev / scales_dev / yhat_dev: NCHW fp32 [n][c][h][w] on the device, w even.  anchor != 0: the positions with
 * (row + col) odd (ckbd.py:37-48), and the other half of yhat_dev is set to zero; anchor == 0: the positions with (row + col)
 * even, the other half of yhat_dev is left as it is.  scale_table: the 64 entries of get_scale_table() (host).
 * symbols_dev / indexes_dev: n * c * h * (w / 2) int32 each, in (n, c, h, w / 2) order -- the order the reference's
 * .reshape(-1).tolist() feeds its encoder.  One kernel, in place on the caller's tensors, asynchronous on `stream` (a hipStream_t;
 * NULL = the default stream) like the coder entry points above; 8-byte aligned tensors take the vectorised form.
 * rgbd_ckbd_dequant is the decoder's half of the same step (elic_united.py:497-506, 529-538): yhat = symbol + mean. */
int rgbd_ckbd_quant_index(const float* y_dev, const float* means_dev, const float* scales_dev, int32_t n, int32_t c, int32_t h,
                          int32_t w, int32_t anchor, const float* scale_table, int32_t* symbols_dev, int32_t* indexes_dev,
                          float* yhat_dev, void* stream);
int rgbd_ckbd_dequant(const int32_t* symbols_dev, const float* means_dev, int32_t n, int32_t c, int32_t h, int32_t w, int32_t anchor,
                      float* yhat_dev, void* stream);

/* One raster channel slice of the single-modal STF's entropy model (models/stf.py:746-751, 796-800): C channels of NHWC fp32
 * device tensors [B][h][w][channel stride], every pointer already offset to the slice's first channel; mean and scale come
 * from two tensors (two nets).  symbol = rint(y - mean) (half to even), index = build_indexes(scale) on the raw scale,
 * y_hat = symbol + mean written to yhat0_dev and, when not NULL, yhat1_dev.  Symbols / indexes land in stream order at
 * slice_off * B + ((b * C + c) * h + row) * w + col (per_image == 0: the reference's one stream per call, slice-major;
 * slice_off = symbols of one image's earlier slices) or at b * image_stride + slice_off + (c * h + row) * w + col
 * (per_image != 0: image b's own stream of image_stride symbols).  scale_table: the 64 entries of get_scale_table() (host).
 * rgbd_slice_dequant is the decoder's half (y_hat = symbol + mean).  Asynchronous on `stream`. */
int rgbd_slice_quant_index(const float* y_dev, int32_t ycs, const float* means_dev, int32_t mcs, const float* scales_dev, int32_t scs,
                           int32_t B, int32_t C, int32_t h, int32_t w, int32_t per_image, int64_t image_stride, int64_t slice_off,
                           const float* scale_table, int32_t* symbols_dev, int32_t* indexes_dev, float* yhat0_dev, int32_t cs0,
                           float* yhat1_dev, int32_t cs1, void* stream);
int rgbd_slice_dequant(const int32_t* symbols_dev, const float* means_dev, int32_t mcs, int32_t B, int32_t C, int32_t h, int32_t w,
                       int32_t per_image, int64_t image_stride, int64_t slice_off, float* yhat0_dev, int32_t cs0, float* yhat1_dev,
                       int32_t cs1, void* stream);
/* Latent residual prediction (stf.py:753-758): out = y_hat + 0.5 * tanh(lrp) for npix pixels of C channels (NHWC, channel
 * strides lcs / ycs / cs*), written to out0_dev and, when not NULL, out1_dev / out2_dev; a destination may be yhat_dev itself.
 * The sum is formed in double (tanh with explicit fused multiply-adds) and rounded once: within 0.5 ulp of the result,
 * the same floats on every call. */
int rgbd_lrp_update(const float* lrp_dev, int32_t lcs, const float* yhat_dev, int32_t ycs, int64_t npix, int32_t C, float* out0_dev,
                    int32_t cs0, float* out1_dev, int32_t cs1, float* out2_dev, int32_t cs2, void* stream);

/* The entropy stage's kernels on the engine's own layout, one launcher each (test hooks: tests/test_gpu_entropy.py).  Every
 * tensor is NHWC fp32 on the device, [B][h][w][channel stride], each with its own channel stride; with perm != 0 channel c of
 * a tensor sits at position (c & ~15) | (c & 3) << 2 | (c >> 2) & 3 (the conv kernels' order inside groups of 16), while
 * symbols, indexes, medians and parameters stay in logical channel order.  Each call checks its arguments on the host and
 * returns -22 before any launch on a NULL pointer, a non-positive extent, a channel stride smaller than the channels it has to
 * hold, odd w (checkerboard parts), perm with a channel count (z path: channel stride) that is no multiple of 16, or
 * B * channels * h * w >= 2^31.  Asynchronous on `stream` unless stated.
 *
 * rgbd_ckbd_estimate_part: eval-mode forward() of one checkerboard half of a slice (models/elic_united.py:234-263 on
 *   entropy_models.py:534-558): y_hat = rint(y - mean) + mean (half to even) and the Gaussian likelihood of the quantised
 *   value with scale >= 0.11, floored at 1e-9, at the half's positions ((row + col) odd for anchor != 0, else even).
 *   params_dev: [scale (C) | mean (C)] per pixel, pcs >= 2 * C.  The anchor pass also zeroes yhat_dev at the other half;
 *   lik_dev is written at the half's positions only.
 * rgbd_slice_estimate: the same for a raster channel slice (models/stf.py:657-660), mean / scale / y from three tensors,
 *   y_hat to yhat0_dev and, when not NULL, yhat1_dev.
 * rgbd_ckbd_part: the codec's integer step on the same layout.  mode 0: symbol = rint(y - mean), index =
 *   build_indexes(scale), y_hat = symbol + mean; mode 1: indexes only; mode 2: y_hat = symbol + mean from symbols_dev.
 *   Symbols / indexes land at stream_base_dev[b] + part_off + (c * h + row) * (w / 2) + k (per_image != 0: one stream per
 *   image, stream_base_dev has B entries) or at stream_base_dev[0] + part_off * B + ((b * C + c) * h + row) * (w / 2) + k
 *   (one stream for the batch); part_off >= 0 counts one image's earlier symbols.  scale_table_dev: the 64 entries of
 *   get_scale_table() on the device (modes 0 / 1).  Modes 0 / 2 zero the other half of yhat_dev in the anchor pass.
 * rgbd_z_quant / rgbd_z_dequant: the factorised prior's integer path (entropy_models.py:195-266, 431-446): symbol =
 *   rint(z - median_c), index = c, at (b * C + c) * h * w + row * w + col; z_hat = symbol + median_c, 0 in the channel
 *   positions that hold no channel (zcs > C).
 * rgbd_eb_forward: the factorised prior in eval mode (entropy_models.py:369-428): z_hat = rint(z - median) + median and
 *   |sigmoid(s * upper) - sigmoid(s * lower)|, s = -sign(lower + upper), floored at 1e-9; z_hat = lik = 0 in the positions
 *   that hold no channel.  z_dev / zhat_dev / lik_dev share the stride zcs.  matrices[5] / biases[5] / factors[4] / medians
 *   are HOST arrays of the raw parameters (_matrix{i} [C][f_{i+1}][f_i], _bias{i}, _factor{i} [C][f_{i+1}][1], filters
 *   1-3-3-3-3-1); they are packed by the function rgbd_elic_finalize packs them with.  Synchronous: returns when done. */
int rgbd_ckbd_estimate_part(const float* y_dev, int32_t ycs, const float* params_dev, int32_t pcs, float* yhat_dev, int32_t yhcs,
                            float* lik_dev, int32_t lcs, int32_t B, int32_t h, int32_t w, int32_t C, int32_t anchor, int32_t perm,
                            void* stream);
int rgbd_slice_estimate(const float* y_dev, int32_t ycs, const float* means_dev, int32_t mcs, const float* scales_dev, int32_t scs,
                        int32_t B, int32_t C, int32_t h, int32_t w, float* lik_dev, int32_t lcs, float* yhat0_dev, int32_t cs0,
                        float* yhat1_dev, int32_t cs1, void* stream);
int rgbd_ckbd_part(int32_t mode, const float* y_dev, int32_t ycs, const float* params_dev, int32_t pcs, float* yhat_dev, int32_t yhcs,
                   const float* scale_table_dev, int32_t B, int32_t h, int32_t w, int32_t C, int32_t anchor, int32_t per_image,
                   int32_t perm, int32_t* symbols_dev, int32_t* indexes_dev, const int64_t* stream_base_dev, int64_t part_off,
                   void* stream);
int rgbd_z_quant(const float* z_dev, int32_t zcs, int32_t B, int32_t h, int32_t w, int32_t C, const float* medians_dev,
                 int32_t* symbols_dev, int32_t* indexes_dev, int32_t perm, void* stream);
int rgbd_z_dequant(const int32_t* symbols_dev, int32_t B, int32_t h, int32_t w, int32_t C, const float* medians_dev, float* zhat_dev,
                   int32_t zcs, int32_t perm, void* stream);
int rgbd_eb_forward(const float* z_dev, int32_t zcs, int32_t B, int32_t h, int32_t w, int32_t C, const float* const* matrices,
                    const float* const* biases, const float* const* factors, const float* medians, float* zhat_dev, float* lik_dev,
                    int32_t perm, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Single operators on device tensors (NCHW fp32, contiguous) -- used by the parity tests of the conv kernels.
 * Replaces torch.nn.functional.conv2d / conv_transpose2d as used by modules/layers/conv.py:7-34.
 * weight: Conv2d layout (Cout,Cin,k,k) or ConvTranspose2d layout (Cin,Cout,k,k) when transposed != 0 (host ptr).
 * act: 0 none, 1 ReLU, 2 LeakyReLU(0.01), 3 sigmoid.  residual_dev (optional, output-shaped) is added before act.
 * ------------------------------------------------------------------------------------------------------------- */
int rgbd_conv2d_nchw(const float* x_dev, int32_t n, int32_t cin, int32_t h, int32_t w, const float* weight,
                     const float* bias, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t transposed,
                     int32_t act, const float* residual_dev, float* y_dev, void* stream);

/* The same operator in the arithmetic of the CPU kernels the reference's conv2d / conv_transpose2d calls end in (torch CPU ->
 * oneDNN 3.7.1 jit:avx512_core / jit_1x1:avx512_core, third-party to the reference): per output element a fresh
 * fp32 fma chain per block of input channels (tap-major inside a block, channels ascending), the block sums added in order.
 * blocks: channels per block (nblocks entries; NULL = one block per 16 channels, the multi-tap kernels' structure).
 * bias_mode: 0 = sum, then + bias; 1 = S_0 + bias, then the other block sums; 2 = the first chain starts from the bias.
 * flags bit 0: sigmoid (act 3) as torch's vectorised CPU kernel computes it; bit 1: run the blocks as split-K ranges. */
int rgbd_conv2d_ref_nchw(const float* x_dev, int32_t n, int32_t cin, int32_t h, int32_t w, const float* weight,
                         const float* bias, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t transposed,
                         int32_t act, const float* residual_dev, float* y_dev, void* stream, const int32_t* blocks,
                         int32_t nblocks, int32_t bias_mode, int32_t flags);

/* The conv launchers in every form the engine issues them in (a test hook: tests/test_gpu_convforms.py).  A superset of the
 * two operators above: it packs the host weights, converts the NCHW device tensors to the engine's layout, fills the
 * launch descriptor as the engine's conv planner does and calls the launcher the engine calls -- the fused one when cout2 > 0.
 *
 *   first layer   n, cin, h, w, cout, k <= 5, stride 1 / 2, pad, transposed, act; refmode != 0: the reference's CPU arithmetic
 *                 with blocks / nblocks / bias_mode / flags as in rgbd_conv2d_ref_nchw
 *   plain form    (cout2 == 0)  y = act(conv(x) + bias + res1) * mul + res2, every operand optional; y2: a second copy of y.
 *                 act 0 none, 1 ReLU, 2 LeakyReLU(0.01), 3 sigmoid, 4 GELU (erf form: 0.5 v (1 + erf(v / sqrt 2))).  GELU is
 *                 applied by the split-K reducer, as in the engine: the hook books one partial plane for it when the split
 *                 factor is 1, splitk * n * OH * OW * cout_pad floats in general (Engine::conv_plan's rule).
 *   fused tail    (cout2 > 0)   t = act_mid(conv(x) + bias), y = act(w2 * t + bias2 + res1); w2 [cout2][cout][1][1],
 *                 act_mid 0 / 1, act 0 / 1 / 2.  In refmode the chains of the 1x1 layers start from their bias.
 *   lead layer    (cout3 > 0, with a fused tail)  u = relu(w3 * y + bias3) -> y3; w3 [cout3][cout2][1][1]
 *   placement     the input is channels [x_off, x_off + cin) of x_dev [n, x_total, h, w] (x_off a multiple of 16); y is
 *                 channels [y_off, y_off + cy) of y_dev [n, y_total, OH, OW], cy = cout2 when fused, else cout (offsets
 *                 multiples of 4; of 16 in refmode); likewise y2 and y3 (cout3 channels) with their own off / total.  The
 *                 channels a launch stores follow the engine's rule: the slice rounded up to 4 when it is narrower than its
 *                 16-padded width inside a wider buffer, else the 16-padded width.  A destination whose stored channels
 *                 would run over a neighbouring slice is refused.  The caller fills y_dev / y2_dev / y3_dev beforehand; the
 *                 whole wide tensors come back, so what a launch did not write is visible.
 *   groups == 2   set[1] is a second operand set of the same shapes (a pointer is NULL there exactly when its twin in
 *                 set[0] is): both run as ONE grouped launch.  groups 0 / 1: set[0] alone.
 *   res1_dev / mul_dev / res2_dev are [n, cy, OH, OW].
 *
 * The debug switches apply: the forced tile, the forced split-K factor (plain form outside refmode), the forced checkerboard
 * half, and the forced fusing mode, whose value is the pixel-tile class of the fused forms (1 / 2 / 4 = 64 / 128 / 256
 * pixels).  With the fusing mode left at -1 the plan decides; it returns 0 on small maps, and the fused forms then return
 * -22 like the launcher itself.
 *
 * Every argument is checked on the host before anything is allocated or launched: a NULL required pointer, a bad size or any
 * combination the launchers refuse (fused with stride 2 / k = 5 / a first layer whose padded cout is not 96 / act 3, a lead
 * layer on a cout2 whose padded width is not a multiple of 32, y2 together with split-K, act 4 with a fused tail / in refmode /
 * with y2, act above 4, checkerboard output of a strided layer, a grouped call with a twin pointer missing, ...) returns -22.
 * A forced tile that cannot hold the layer returns -28.
 * Every destination, and the partial planes of a split-K / GELU launch, is followed on the device by a guard band of one output
 * row and one pixel; -1 = a launch wrote into it. */
typedef struct rgbd_conv_forms_ops {
    const float* x_dev;    /* [n, x_total, h, w] */
    const float* weight;   /* host: Conv2d layout, or ConvTranspose2d layout when transposed != 0 */
    const float* bias;     /* host [cout], optional */
    const float* w2;       /* host, fused tail */
    const float* bias2;    /* host [cout2], optional */
    const float* w3;       /* host, lead layer */
    const float* bias3;    /* host [cout3], optional */
    const float* res1_dev; /* optional */
    const float* mul_dev;  /* optional, plain form */
    const float* res2_dev; /* optional, plain form */
    float* y_dev;          /* [n, y_total, OH, OW], in / out */
    float* y2_dev;         /* [n, y2_total, OH, OW], in / out, optional, plain form */
    float* y3_dev;         /* [n, y3_total, OH, OW], in / out, lead layer */
} rgbd_conv_forms_ops;

typedef struct rgbd_conv_forms_desc {
    int32_t n, cin, h, w, cout, k, stride, pad, transposed, act;
    int32_t refmode, nblocks, bias_mode, flags;
    const int32_t* blocks;
    int32_t cout2, act_mid, cout3;
    int32_t x_off, x_total, y_off, y_total, y2_off, y2_total, y3_off, y3_total;
    int32_t groups;
    rgbd_conv_forms_ops set[2];
} rgbd_conv_forms_desc;

int rgbd_conv_forms_nchw(const rgbd_conv_forms_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The codec. Replaces models/elic_united.py: ELIC_united.__init__ :14-86, load_state_dict :588-620,
 * update :580-586, compress :403-427 (+ compress_united :350-401, compress_one_slice :265-348),
 * decompress :429-452 (+ decompress_united :543-578, decompress_one_slice :454-541).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct rgbd_elic rgbd_elic;

/* Reference arithmetic.  An engine created for ELIC_united / ELIC / ELIC_united_R2D computes every float that
 * feeds a coding decision in the accumulation order of the CPU kernels the reference runs on (torch CPU 2.10 -> oneDNN 3.7.1 /
 * MKL / Sleef; third-party to the reference).  Where that order depends on the layer shape -- the reduce blocks of oneDNN's 1x1
 * convolution kernel (kind 0) -- it is data measured on the reference machine and handed over here, per
 * (cin, cout, input h, w, batch of the reference call): blocks[0..nblocks) = channels per block.  Shapes without an entry
 * run as a single block.  rgbd_elic_get_refnum: 1 when the engine uses this arithmetic (STF_united: 0). */
int rgbd_elic_set_ref_blocks(rgbd_elic* m, int32_t kind, int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t batch,
                             const int32_t* blocks, int32_t nblocks);
int rgbd_elic_get_refnum(const rgbd_elic* m);
int rgbd_elic_ref_table_misses(const rgbd_elic* m);

/* A second instance that borrows `src`'s packed device weights and tables (own workspace, own stream): several
 * instances on one GPU then cost one weight copy.  `src` must outlive the clone. */
int rgbd_elic_clone_shared(const rgbd_elic* src, rgbd_elic** out);

/* config/config.py:5-10: N, M and the channel count of each latent slice. */
int rgbd_elic_create(int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, rgbd_elic** out);
void rgbd_elic_destroy(rgbd_elic* m);

/* One state_dict entry (float32, host, reference name and shape).  Call for every parameter, then finalize. */
int rgbd_elic_set_tensor(rgbd_elic* m, const char* name, const float* data, const int64_t* shape, int32_t ndim);
/* which: 0 rgb gaussian, 1 depth gaussian, 2 rgb bottleneck, 3 depth bottleneck (results of update()). */
int rgbd_elic_set_tables(rgbd_elic* m, int32_t which, const int32_t* cdf, int32_t cdf_stride, const int32_t* cdf_sizes,
                         const int32_t* offsets, int32_t n_cdf);
/* scale_table: 64 floats (utils/moduleFunc.py:11-12). */
int rgbd_elic_set_scale_table(rgbd_elic* m, const float* table, int32_t n);
/* Packs the weights for the MFMA kernels and uploads everything to the current device. */
int rgbd_elic_finalize(rgbd_elic* m);
/* What finalize takes a state-dict entry for, decided by the family, the name and the shape alone (test hook; host only, no
 * GPU needed).  family: 0 ELIC_united, 1 ELIC, 2 STF_united, 3 ELIC_united_R2D, 4 STF, 5 checkerboard Cheng2020,
 * 6 Spatial_aligner, 7 LocalContext, 8 LinearGlobalInterContext, 9 LinearGlobalIntraContext, 13 SynthesisTransformPlus,
 * 15 EntropyParametersMLIC, 16 ChannelContext, 17 LatentResidualPrediction, 19 MLIC++, 20 ELIC_master_latent (10 to 12 are
 * reserved, 14 and 18 unused).  Family 20 ignores ELIC_master's outer blocks (aux_encoder., master_encoder., master_decoder.,
 * channel_aligner.).  Returns one of
 * the kinds below, or RGBD_EINVAL for another family, a NULL pointer, ndim outside 1..4 or an extent < 1. */
enum {
    RGBD_KIND_IGNORED = 0,         /* read by no packer of its own: biases, betas, bottleneck matrices, buffers */
    RGBD_KIND_RECOVERY_DECONV = 1, /* Spatial_aligner.recovery, a 2x2 stride-2 deconv: packed as a 1x1 conv + pixel shuffle */
    RGBD_KIND_CONTEXT_DENSE = 2,   /* fusion.weight / depthwise [C][1][3][3] of the MLIC++ contexts: plain device arrays */
    RGBD_KIND_CONV = 3,            /* Conv2d layer, packed for the MFMA kernels */
    RGBD_KIND_CONV_TRANSPOSED = 4, /* ConvTranspose2d layer, likewise */
    RGBD_KIND_GDN_GAMMA = 5,       /* square .gamma, packed with its .beta */
    RGBD_KIND_LINEAR = 6,          /* 2-D .weight (SE_Block) */
    RGBD_KIND_ARRAY = 7,           /* LayerNorm parameters and relative position tables: plain device arrays */
    RGBD_KIND_QUANTILES = 8,       /* entropy_bottleneck.quantiles: medians and the cumulative's parameters */
    RGBD_KIND_PIXEL_MLP = 9        /* fusion.K.weight of EntropyParametersMLIC: as RGBD_KIND_CONV, and as the lane fragments of rgbd_pixel_mlp4 */
};
int rgbd_debug_tensor_kind(int32_t family, const char* name, const int64_t* shape, int32_t ndim);

/*
 * compress(): rgb_dev [B,3,H,W], depth_dev [B,1,H,W] fp32 on the device, H and W multiples of 64.
 * per_image_streams = 0 reproduces the reference's batched call (ONE y-stream per modality for the whole batch,
 * elic_united.py:392-400); 1 emits one y-stream per image (= what B separate reference calls produce).
 * z-streams are always per image.  Results are fetched with rgbd_elic_stream().
 */
int rgbd_elic_compress(rgbd_elic* m, const float* rgb_dev, const float* depth_dev, int32_t B, int32_t H, int32_t W,
                       int32_t per_image_streams, void* stream);
/* modality: 0 rgb, 1 depth; kind: 0 y, 1 z; index < count.  Pointer stays valid until the next compress(). */
int rgbd_elic_stream_count(const rgbd_elic* m, int32_t modality, int32_t kind);
int rgbd_elic_stream(const rgbd_elic* m, int32_t modality, int32_t kind, int32_t index, const uint8_t** data,
                     int64_t* nbytes);

/*
 * decompress(): streams as produced above (y: n_y = 1 or B per modality; z: B per modality), z-grid zh x zw
 * (= H/64, W/64).  Writes x_hat clamped to [0,1]: xr_dev [B,3,64*zh,64*zw], xd_dev [B,1,64*zh,64*zw].
 */
int rgbd_elic_decompress(rgbd_elic* m, const uint8_t* const* y_rgb, const int64_t* y_rgb_len, int32_t n_y,
                         const uint8_t* const* y_depth, const int64_t* y_depth_len, const uint8_t* const* z_rgb,
                         const int64_t* z_rgb_len, const uint8_t* const* z_depth, const int64_t* z_depth_len, int32_t B,
                         int32_t zh, int32_t zw, float* xr_dev, float* xd_dev, void* stream);

/*
 * The Bi-CEE entropy stage alone (BASELINE config 4): replaces ELIC_united.compress_united (models/elic_united.py:350-401,
 * with compress_one_slice :265-348) and decompress_united (:543-578, decompress_one_slice :454-541).  Latents y
 * [B,M,h,w] and hyper parameters [B,2M,h,w] are NCHW fp32 device tensors (w even); only y-streams are produced
 * (fetch them with rgbd_elic_stream(kind = 0)); decompress_united writes y_hat [B,M,h,w] per modality.
 */
int rgbd_elic_compress_united(rgbd_elic* m, const float* y_rgb_dev, const float* hyper_rgb_dev, const float* y_depth_dev,
                              const float* hyper_depth_dev, int32_t B, int32_t h, int32_t w, int32_t per_image_streams,
                              void* stream);
int rgbd_elic_decompress_united(rgbd_elic* m, const uint8_t* const* y_rgb, const int64_t* y_rgb_len, int32_t n_y,
                                const uint8_t* const* y_depth, const int64_t* y_depth_len, const float* hyper_rgb_dev,
                                const float* hyper_depth_dev, int32_t B, int32_t h, int32_t w, float* yhat_rgb_dev,
                                float* yhat_depth_dev, void* stream);

/*
 * Single-modal ELIC (BASELINE config 1): replaces models/elic.py: ELIC.__init__ :15-57, compress :161-253,
 * decompress :255-325 (x_hat is NOT clamped there).  Same life cycle as above (set_tensor with the reference's key names,
 * set_tables which = 0 gaussian / 2 bottleneck, set_scale_table, finalize); streams are fetched with
 * rgbd_elic_stream(modality = 0, kind, index).  x_dev: [B,in_ch,H,W] NCHW fp32, H and W multiples of 64.
 */
int rgbd_elic_create_single(int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, int32_t in_ch, rgbd_elic** out);
int rgbd_elic_compress_single(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, int32_t per_image_streams,
                              void* stream);
int rgbd_elic_decompress_single(rgbd_elic* m, const uint8_t* const* y, const int64_t* y_len, int32_t n_y,
                                const uint8_t* const* z, const int64_t* z_len, int32_t B, int32_t zh, int32_t zw,
                                float* x_dev, void* stream);
/* The single-modal STF (models/stf.py: SymmetricalTransFormer :408-816; N = 192, M = 384, 12 slices of 32 channels): Swin
 * analysis / synthesis transforms, two hyper-synthesis nets and the channel-slice entropy model with latent residual prediction.
 * Served by the three *_single entry points of this section: compress puts all slices of all images of a call into ONE y
 * stream (per_image_streams: one per image); decompress clamps x_hat to [0, 1] (stf.py:815) and, unlike the reference, is the
 * inverse of compress for a batch as well; forward's x_hat is not clamped.  Debug tensors: y, z, zhat, yhat, latent_means,
 * latent_scales. */
int rgbd_elic_create_stf_single(int32_t in_ch, rgbd_elic** out);
/* The checkerboard Cheng2020 model (models/Cheng2020withCKBD.py:40-174: Cheng2020AnchorwithCheckerboard, on CompressAI's
 * Cheng2020Anchor, compressai/models/waseda.py:22-81; N = 128 or 192, M = N, in_ch = 3 or 1): residual blocks of 3x3 / 1x1
 * convolutions with GDN / IGDN (one fused launch each, see rgbd_gdn_nchw), sub-pixel up-sampling, a hyper prior and a two-pass
 * checkerboard entropy model: entropy_parameters(cat(0, hyper)) codes the anchor half of y ((row + col) odd), the masked 5x5
 * context convolution over the decoded anchors (the mask of :28-35 is applied when the weights are packed) feeds
 * entropy_parameters(cat(ctx, hyper)) for the other half.  Served by the three *_single entry points of this section:
 * compress (:101-136) puts both halves of all images of a call into ONE y stream, anchor half first, each in (n, c, row, w/2)
 * order (per_image_streams: one stream per image); decompress (:138-174) does not clamp x_hat; forward is the eval forward()
 * (:52-71): y_hat = round(y), the context over the whole grid with its anchor outputs zeroed, one parameter pass.
 * rgbd_elic_get_refnum returns 0; rgbd_elic_set_forced_symbols works for modality 0.  Debug tensors: y, z, zhat, hyper, yhat,
 * ctx, means, scales. */
int rgbd_elic_create_ckbd(int32_t N, int32_t in_ch, rgbd_elic** out);
/* MLIC++ (models/mlicpp.py: MLICPlusPlus; N a multiple of 16, slice_num 2 ... 10 slices of 32 channels, M = 32 slice_num,
 * in_ch 1 ... 16; anything else is RGBD_EINVAL before any allocation): residual blocks of 3x3 / 1x1 convolutions with GDN / IGDN
 * and GELU, sub-pixel up-sampling, GELU hyper transforms, and per slice two checkerboard coding parts under the attention
 * contexts (LocalContext, LinearGlobalIntraContext, LinearGlobalInterContext), ChannelContext, EntropyParametersMLIC (one fused
 * launch per part) and LatentResidualPrediction, whose correction is added in place at the part's own pixels
 * (rgbd_mlic_lrp_apply).  State-dict names are the reference's: ten of each network under `local_context.{i}.` and so on.
 * Served by the three *_single entry points of this section, with image sides that are multiples of 64 and at least 128 (the
 * z grid runs 3x3 layers; a one-row or one-column z map is RGBD_EINVAL before any launch): compress (:199-312) puts all parts of
 * all images of a call into ONE y stream, slice-major, anchor part then non-anchor part, each in (n, c, row, w/2) order
 * (per_image_streams: one stream per image); decompress (:314-413) does not clamp x_hat; forward is the eval forward()
 * (:77-188).  rgbd_elic_get_refnum returns 0; rgbd_elic_set_coder(format 1) is refused; rgbd_elic_set_forced_symbols works for
 * modality 0.  Debug tensors: y, z, zhat, hyper, yhat. */
int rgbd_elic_create_mlic(int32_t N, int32_t M, int32_t slice_num, int32_t in_ch, rgbd_elic** out);
/* The latent codec of ELIC_master (models/elic_master.py; family 20): everything between the model's outer blocks -- g_a =
 * AnalysisTransformEX(N, M, ch = 128) on f = cat(fv, fv_bar) (:67, 113-115), h_a / h_s (:70-71), the checkerboard slice loop with
 * EntropyParametersEX nets over cat(local_ctx, channel_ctx, hyper_params) (:128-208; SE rescale, 1x1 / 3x3 / 5x5), and g_s =
 * SynthesisTransformPlus(N, M, ch = N) under the guides up1..up3 of the aux decoder (:68, 213-216).  Feature_encoder,
 * Feature_decoder and Channel_aligner are not part of it.  N must be 192 (sp1..sp3 are built with 192 channels whatever N is);
 * slice_ch as for rgbd_elic_create_single.  State-dict names are the reference's (g_a.*, g_s.synthesis_transform.*, g_s.sp1|2|3.*
 * with Linear weights as [out][in][1][1], h_a.*, h_s.*, local_context.*, channel_context.*, entropy_parameters_*.*,
 * entropy_bottleneck.*).  Single-chain float arithmetic (rgbd_elic_get_refnum returns 0); rgbd_elic_set_coder(format 1) is
 * refused; rgbd_elic_set_forced_symbols works for modality 0.  Debug tensors: y, z, zhat, hyper, yhat.
 *   compress (:228-304): rgbd_elic_compress_single with f [B,128,H,W] (NCHW fp32, H and W multiples of 64): one y stream per call
 *     (per_image_streams: per image), one z stream per image; g_s does not run and no guides are taken.
 *   rgbd_master_latent_decompress (:319-378): the streams and up1 [B,N,H/8,W/8], up2 [B,N,H/4,W/4], up3 [B,N,H/2,W/2] -> f_hat
 *     [B,N,H,W], the tensor of :378 before its cat with fv_bar; not clamped.
 *   rgbd_master_latent_forward (:115-216, eval mode with quant = "ste"): f and the guides -> f_hat, y_likelihoods [B,M,H/16,W/16],
 *     z_likelihoods [B,N,H/64,W/64].
 * RGBD_EINVAL before any write: a NULL pointer (a missing guide included), H or W not a multiple of 64 (zh, zw < 1), B < 1, a
 * tensor of 2^31 elements or more, a handle of another family; rgbd_elic_forward_single and rgbd_elic_decompress_single refuse a
 * handle of this family (they take no guides). */
int rgbd_master_latent_create(int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, rgbd_elic** out);
int rgbd_master_latent_forward(rgbd_elic* m, const float* f_dev, const float* up1_dev, const float* up2_dev, const float* up3_dev,
                               int32_t B, int32_t H, int32_t W, float* fhat_dev, float* lik_y, float* lik_z, void* stream);
int rgbd_master_latent_decompress(rgbd_elic* m, const uint8_t* const* y, const int64_t* y_len, int32_t n_y, const uint8_t* const* z,
                                  const int64_t* z_len, int32_t B, int32_t zh, int32_t zw, const float* up1_dev, const float* up2_dev,
                                  const float* up3_dev, float* fhat_dev, void* stream);
/* The two updates MLIC++'s slice loop makes to a 32-channel slot of its NHWC state buffer, alone (test hooks; asynchronous on
 * `stream`).  slot_dev [B][h][w][slot_cs] points at the slot's first channel inside a buffer of channel stride slot_cs;
 * parity 0: the pixels with (row + col) odd (the anchors), 1: the others.  Pixels of the other parity and channels outside the
 * slot are neither read nor written.
 *   rgbd_mlic_lrp_apply: slot += 0.5 * tanh(r) -- the value of rgbd_pw_half_tanh followed by one fp32 add; r_dev [B][h][w][r_cs].
 *   rgbd_mlic_slot_clear: slot = 0.
 * RGBD_EINVAL before any launch: channels other than 32, a stride below 32 or not a multiple of 4, a pointer that is NULL or
 * not 16-byte aligned, B, h or w below 1, a parity other than 0 / 1, 2^31 elements or more, r_dev == slot_dev. */
int rgbd_mlic_lrp_apply(float* slot_dev, int32_t slot_cs, const float* r_dev, int32_t r_cs, int32_t channels, int32_t B, int32_t h,
                        int32_t w, int32_t parity, void* stream);
int rgbd_mlic_slot_clear(float* slot_dev, int32_t slot_cs, int32_t channels, int32_t B, int32_t h, int32_t w, int32_t parity,
                         void* stream);
/* Eval-mode forward() of the single-modal model (models/elic.py:60-161 with config quant = "ste"): x_hat [B,in_ch,H,W]
 * (not clamped), likelihoods of y [B,M,H/16,W/16] and of z [B,N,H/64,W/64] ("y_likelihoods" / "z_likelihoods"). */
int rgbd_elic_forward_single(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, float* xhat_dev, float* lik_y,
                             float* lik_z, void* stream);
/* ELIC(return_mid=True) (models/elic.py:159-170 forward, :318-329 decompress; modules/transform/synthesis.py:54-67): the two
 * calls above for a handle of rgbd_elic_create_single, which also hand back the outputs of the first three transposed
 * convolutions of g_s: up1 [B,N,H/8,W/8], up2 [B,N,H/4,W/4], up3 [B,N,H/2,W/2], NCHW fp32, none NULL.  x_hat and the
 * likelihoods are those of the calls above, bit for bit. */
int rgbd_elic_decompress_single_mid(rgbd_elic* m, const uint8_t* const* y, const int64_t* y_len, int32_t n_y,
                                    const uint8_t* const* z, const int64_t* z_len, int32_t B, int32_t zh, int32_t zw,
                                    float* x_dev, float* up1, float* up2, float* up3, void* stream);
int rgbd_elic_forward_single_mid(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, float* xhat_dev, float* lik_y,
                                 float* lik_z, float* up1, float* up2, float* up3, void* stream);
/* Spatial_aligner alone (modules/transform/spatialAligner.py:341-390; the block SynthesisTransformPlus inserts behind up1..up3,
 * synthesis.py:74-110): two 2x2 stride-2 patch embeddings to 96 channels, two Swin blocks whose attention takes the query from
 * x and key / value from guided (rgbd_guided_window_attention; shift 0, then 2), a 2x2 stride-2 transposed convolution to
 * out_ch.  Life cycle of the codec handles: set_tensor with the reference's names (patch_embeding1/2, blocks.K.*, recovery;
 * Linear weights as [out][in][1][1]), finalize, clone_shared, destroy; no tables.  x, guided: [B,in_ch,H,W] NCHW fp32; out:
 * [B,out_ch,H,W]; H % 8 == 0, W % 8 == 0.  The codec calls on an aligner handle, and rgbd_aligner_forward on a handle of
 * another family, return RGBD_EINVAL. */
int rgbd_aligner_create(int32_t in_ch, int32_t out_ch, rgbd_elic** out);
int rgbd_aligner_forward(rgbd_elic* m, const float* x_dev, const float* guided_dev, int32_t B, int32_t H, int32_t W,
                         float* out_dev, void* stream);
/* SynthesisTransformPlus alone (modules/transform/synthesis.py:74-110; the g_s of ELIC_master, models/elic_master.py): the 15
 * g_s stages of the single-modal ELIC, with x replaced by Spatial_aligner(x, up_k) behind each of the first three transposed
 * convolutions (stages 1, 5, 10: in front of the bottlenecks of 2, 7, 11 and of the AttentionBlock of 6).  up1..up3 are what
 * rgbd_elic_decompress_single_mid hands back for the aux image.  A handle of the aligner's kind (set_tensor, finalize,
 * clone_shared, destroy; no tables; family 13 of rgbd_debug_tensor_kind) under the reference's names: synthesis_transform.K.*
 * and sp1|sp2|sp3.* (Linear weights as [out][in][1][1]).  N must be 192 (the reference builds sp1..sp3 with 192 channels whatever
 * N is); out_ch is `ch`: 1 ... 1024.  yhat [B,M,h,w], up1 [B,N,2h,2w], up2 [B,N,4h,4w], up3 [B,N,8h,8w] -> out
 * [B,out_ch,16h,16w] (not clamped), NCHW fp32; h % 4 == 0, w % 4 == 0.  Single-chain float arithmetic, weights in plain channel
 * order.  A bad argument, a handle of another family, the codec calls, rgbd_aligner_forward and rgbd_elic_set_coder(m, 1, .)
 * on this handle return RGBD_EINVAL before any launch. */
int rgbd_synthesis_plus_create(int32_t N, int32_t M, int32_t out_ch, rgbd_elic** out);
int rgbd_synthesis_plus_forward(rgbd_elic* m, const float* yhat_dev, const float* up1_dev, const float* up2_dev,
                                const float* up3_dev, int32_t B, int32_t h, int32_t w, float* out_dev, void* stream);
/* Timing aid for the call above: on = 0 runs the walk without the three aligners (the guides are converted and not read),
 * 1 (default) the module.  RGBD_EINVAL on a handle of another family. */
int rgbd_debug_synthesis_plus_guides(rgbd_elic* m, int32_t on);
/* The three attention contexts of MLIC++ alone (modules/transform/context.py; MLICPlusPlus builds them with slice_ch 32,
 * config/config.py:15-18).  Handles of the aligner's kind: set_tensor under the reference's state-dict names (Linear weights
 * as [out][in][1][1], depthwise weights as [C][1][3][3]), finalize, clone_shared, destroy; no tables; the codec calls on such
 * a handle, and a forward call on a handle of another family, return RGBD_EINVAL.  All tensors NCHW fp32 on the device.
 * rgbd_local_context_*: LocalContext(dim) (:33-137): norm1, qkv_proj, rgbd_local_ckbd_attention (5x5 window, 2 heads of 16,
 *   with `fusion`), proj, x + mlp(norm2(x)).  dim must be 32.  x [B,dim,H,W] -> out [B,2 dim,H,W], any H, W >= 1.
 * rgbd_linear_inter_*: LinearGlobalInterContext(dim, out_dim, heads) (:216-262): keys / queries / values = 1x1 + depthwise 3x3
 *   of x1, rgbd_linear_attention mode 0, 5x5 reprojection to 3/2 out_dim, skip(a) + mlp(a).  dim / heads in {16, 32},
 *   out_dim % 32 == 0.  x1 [B,dim,H,W] -> out [B,out_dim,H,W].
 * rgbd_linear_intra_*: LinearGlobalIntraContext(dim, heads) (:163-213): keys from the anchor half of x1 ((row + col) odd,
 *   utils/ckbd.py:37-48), queries from the other half, values from x2, rgbd_linear_attention mode 1, 5x5 reprojection to
 *   2 dim, a + mlp(a).  dim / heads in {16, 32}, W even.  x1, x2 [B,dim,H,W] -> out [B,2 dim,H,W]. */
int rgbd_local_context_create(int32_t dim, rgbd_elic** out);
int rgbd_local_context_forward(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, float* out_dev, void* stream);
int rgbd_linear_inter_create(int32_t dim, int32_t out_dim, int32_t heads, rgbd_elic** out);
int rgbd_linear_inter_forward(rgbd_elic* m, const float* x1_dev, int32_t B, int32_t H, int32_t W, float* out_dev, void* stream);
int rgbd_linear_intra_create(int32_t dim, int32_t heads, rgbd_elic** out);
int rgbd_linear_intra_forward(rgbd_elic* m, const float* x1_dev, const float* x2_dev, int32_t B, int32_t H, int32_t W,
                              float* out_dev, void* stream);
/* The three networks MLIC++ runs inside its slice loop, alone (MLICPlusPlus builds them per 32-channel slice, models/mlicpp.py).
 * Handles of the contexts' kind: set_tensor under the reference's state-dict names, finalize, clone_shared, destroy; no tables;
 * the codec calls and rgbd_elic_set_coder(m, 1, .) on such a handle, and a forward call on a handle of another family, return
 * RGBD_EINVAL.  All tensors NCHW fp32 on the device.
 * rgbd_entropy_params_mlic_*: EntropyParametersMLIC(in_dim, out_dim) (modules/transform/entropy.py:31-53): four 1x1
 *   convolutions in_dim -> 320 -> 256 -> 128 -> out_dim with nn.GELU() (erf form) between them, names fusion.{0,2,4,6}.  in_dim
 *   16 ... 960, out_dim 16 ... 128, multiples of 16.  The input is the concatenation of n_seg (1 ... 6) tensors
 *   [B,seg_channels[i],H,W], each a multiple of 16 channels wide and summing to in_dim, which is never formed (the codec's
 *   torch.cat([...], dim=1)): a layout pass per tensor, then one rgbd_pixel_mlp4 launch.  parity -1: out [B,out_dim,H,W] is
 *   written; 0 / 1: only its anchor ((row + col) odd) / other pixels are, the rest keeps its values (W even).
 *   rgbd_entropy_params_mlic_set_fused(m, 0) runs the same layers as four launches of the conv kernels over the written-out
 *   concatenation instead (the yardstick; default 1); it drops the cached graphs.
 * rgbd_channel_context_*: ChannelContext(in_dim, out_dim) (modules/transform/context.py:140-160): three 3x3 convolutions
 *   in_dim -> 192 -> 128 -> 4 out_dim, GELU between them, names fushion.{0,2,4} (the reference's spelling).
 *   x [B,in_dim,H,W] -> out [B,4 out_dim,H,W].
 * rgbd_lrp_*: LatentResidualPrediction(in_dim, out_dim) (modules/transform/LRP.py:9-26): four 3x3 convolutions of widths
 *   in - d / 4, in - d / 2, in - 3 d / 4, out (d = |out - in|, integer division), GELU between them, then 0.5 * tanh; names
 *   lrp_transform.{0,2,4,6}.  Widths that are no multiples of 16 are padded with zero weights.  x [B,in_dim,H,W] -> out
 *   [B,out_dim,H,W].
 * The two 3x3 modules refuse H < 2 or W < 2 with RGBD_EINVAL before any launch. */
int rgbd_entropy_params_mlic_create(int32_t in_dim, int32_t out_dim, rgbd_elic** out);
int rgbd_entropy_params_mlic_forward(rgbd_elic* m, const float* const* seg_dev, const int32_t* seg_channels, int32_t n_seg, int32_t B,
                                     int32_t H, int32_t W, int32_t parity, float* out_dev, void* stream);
int rgbd_entropy_params_mlic_set_fused(rgbd_elic* m, int32_t on);
int rgbd_channel_context_create(int32_t in_dim, int32_t out_dim, rgbd_elic** out);
int rgbd_channel_context_forward(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, float* out_dev, void* stream);
int rgbd_lrp_create(int32_t in_dim, int32_t out_dim, rgbd_elic** out);
int rgbd_lrp_forward(rgbd_elic* m, const float* x_dev, int32_t B, int32_t H, int32_t W, float* out_dev, void* stream);
/* The 1x1 stack of EntropyParametersMLIC as ONE launch on NHWC device tensors (csrc/pixel_mlp.hip; replaces the four
 * nn.Conv2d / three nn.GELU calls of entropy.py:35-41 and the torch.cat in front of them): a workgroup stages 16 pixels of the
 * input in LDS, the three intermediates stay there, only weights stream.  seg_dev[i]: [B][H][W][seg_stride[i]], of which the
 * first seg_channels[i] channels are read; n_seg 1 ... 6; every channel count a multiple of 16, their sum 16 ... 960; strides
 * multiples of 4, pointers 16-byte aligned.  w_dev[k]: layer k's weight [cout][cin] after rgbd_pixel_mlp4_pack (a host-side
 * reordering into MFMA lane fragments, cout * cin floats), bias_dev[k]: [cout]; the hidden widths are 320, 256 and 128,
 * out_dim 16 ... 128.  out_dev: [B][H][W][out_stride].  parity -1: every pixel; 0: the anchor pixels ((row + col) odd); 1: the
 * others; what is not selected is neither computed nor written (W even).  Every output is one fp32 chain that starts from the
 * bias and takes k in increasing order: a pixel's bits depend on nothing but its own input -- not on B, H, W, parity or on how
 * the channels are cut into segments.  Any other shape: RGBD_EINVAL before anything is launched. */
int rgbd_pixel_mlp4_pack(const float* w, int32_t cout, int32_t cin, float* out);
int rgbd_pixel_mlp4(const float* const* seg_dev, const int32_t* seg_channels, const int32_t* seg_stride, int32_t n_seg,
                    const float* const* w_dev, const float* const* bias_dev, int32_t out_dim, int32_t B, int32_t H, int32_t W,
                    int32_t parity, float* out_dev, int32_t out_stride, void* stream);

/*
 * STF_united (BASELINE config 5): replaces models/stf_united.py: SymmetricalTransFormerUnited :605-678 with
 * AnalysisTransformSTFunited :403-502 / SynthesisTransformSTFunited :505-602 (Swin blocks :118-214, PatchMerging :217-249,
 * PatchSplit :252-267, BasicLayer :270-366, PatchEmbed :369-400).  Everything behind the transforms is ELIC_united's (same
 * compress / decompress / forward entry points above); nn.Linear weights are passed as (out, in, 1, 1).
 */
int rgbd_elic_create_stf(int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, rgbd_elic** out);
/* ELIC_united_R2D: replaces models/elic_united_R2D.py:9-326 (AnalysisTransformEXSingle analysis.py:56-112,
 * SynthesisTransformEXSingle synthesis.py:186-242, HyperSynthesisEXSingle synthesis.py:325-343, the one-directional context
 * wiring of compress_one_slice / decompress_one_slice).  Same entry points as ELIC_united otherwise. */
int rgbd_elic_create_r2d(int32_t N, int32_t M, const int32_t* slice_ch, int32_t n_slices, rgbd_elic** out);

/*
 * Eval-mode forward(): replaces ELIC_united.forward / entropy_estimate_united / codeOnePart (models/elic_united.py:94-263)
 * and the likelihood halves of EntropyBottleneck.forward / GaussianConditional.forward (entropy_models.py:391-428,
 * 534-558).  x_hat is NOT clamped (as in the reference); likelihoods are lower-bounded at 1e-9.
 * Outputs (device, NCHW fp32): xr [B,3,H,W], xd [B,1,H,W], lik_y_* [B,M,H/16,W/16], lik_z_* [B,N,H/64,W/64].
 */
int rgbd_elic_forward(rgbd_elic* m, const float* rgb_dev, const float* depth_dev, int32_t B, int32_t H, int32_t W,
                      float* xr_dev, float* xd_dev, float* lik_y_rgb, float* lik_y_depth, float* lik_z_rgb,
                      float* lik_z_depth, void* stream);

/* Intermediate of the last compress()/decompress() as NCHW fp32 on the host (parity tests).  Names: y_r y_d z_r z_d
 * zhat_r zhat_d hyper_r hyper_d yhat_r yhat_d.  shape_out receives 4 ints; data may be NULL to query the shape. */
int rgbd_elic_debug_tensor(rgbd_elic* m, const char* name, float* data, int64_t cap_floats, int32_t* shape_out);
/* Symbols / indexes of the last compress() in stream order (modality 0/1), total count in *n. */
int rgbd_elic_debug_symbols(rgbd_elic* m, int32_t modality, int32_t* symbols, int32_t* indexes, int64_t cap, int64_t* n);
/* Parity bookkeeping: with set_debug_floats(1) the next compress() also keeps, per symbol and in stream order, the value
 * it rounded (y - mean: the argument of quantize(), entropy_models.py:131-137) and the scale it indexed (build_indexes(),
 * entropy_models.py:561-568); debug_floats copies them out.  Lets a test put the GPU's floats next to the reference's at
 * the first symbol where the two streams part (tests/test_gpu_parity_pinned.py). */
int rgbd_elic_set_debug_floats(rgbd_elic* m, int32_t on);
int rgbd_elic_debug_floats(rgbd_elic* m, int32_t modality, float* x, float* scale, int64_t cap, int64_t* n);
/* Teacher forcing (parity bookkeeping; tests/test_gpu_parity_pinned.py::test_teacher_forced_*): the following compress() /
 * compress_united() calls still take every decision from their own floats -- debug_symbols / debug_floats / the streams
 * are the GPU's -- but the context later parts see is rebuilt from the symbols given here, in stream order (what
 * models/elic_united.py:265-348 would have fed forward had it taken exactly these decisions): z_hat = z_sym + median
 * after the z stage (entropy_models.py:437-446), y_hat = y_sym + mean after each of the 20 coding parts.  With the
 * reference's symbols (tests/golden/margins_*.npz) every part BEHIND a first flip is compared under the reference's
 * context.  n_y = B * M * h * w per modality (n_z = B * N * zh * zw; 0 = this stage is not forced); n_y = n_z = 0 clears. */
int rgbd_elic_set_forced_symbols(rgbd_elic* m, int32_t modality, const int32_t* y_sym, int64_t n_y, const int32_t* z_sym,
                                 int64_t n_z);

/* The format of the y streams: format 0 = the reference's (default; `lanes` ignored), 1 = wide rANS with `lanes`
 * interleaved states (1, 2, 4 ... 64; see rgbd_rans_wide_encode above), one segment per checkerboard half of a slice.  The z
 * streams keep the reference format.  compress() then returns bare wide y streams and decompress() expects them (the
 * Python models add and check a 4-byte tag); a damaged wide stream fails decompress() with RGBD_EINVAL.  Drops the cached
 * graphs.  RGBD_EINVAL: NULL engine, format outside 0 ... 1, bad lanes, or format 1 on a family other than ELIC_united and
 * ELIC (STF_united, ELIC_united_R2D, STF and the checkerboard Cheng2020 keep the reference format and refuse here, before
 * anything is launched).  RGBD_ESTATE inside a running call of the engine. */
int rgbd_elic_set_coder(rgbd_elic* m, int32_t format, int32_t lanes);

/* Test hooks: force a split-K factor for rgbd_conv2d_nchw / the codec's entropy-model layers (0 = automatic) and
 * kernel-only timing of one convolution shape on NHWC scratch buffers (tools/conv_sweep.py). */
int rgbd_debug_force_splitk(int32_t s);
/* ResidualBottleneck / ResidualUnit tails (3x3 + ReLU -> 1x1 + residual; res_blk.py:7-27, layers.py:177-196) run as one
 * launch where that is faster, together with the leading 1x1 + ReLU of the block that follows.  -1 = automatic (default),
 * 0 = never, 1 / 2 / 4 = always, with 64 / 128 / 256-pixel tiles; + 16 (15, 17, 18, 20) = the same without the following
 * block's leading layer.  Results are bit-identical in every mode. */
int rgbd_debug_force_fuse(int32_t mode);
/* The image-producing ConvTranspose2d (N -> 3 / 1, k 5, stride 2; synthesis.py:147,168) runs as one 9-tap sub-pixel conv
 * over the input grid (16 channels = 4 output phases x 4) instead of four phases with the couts padded to 16 each:
 * 0 = per-phase form, 1 = sub-pixel form inside the codec (default), 2 = also in rgbd_conv2d_nchw.  Same bits.
 * Mode 0 also returns the image-consuming first conv (3 / 1 -> N, k 5, stride 2; analysis.py:125,150) from its K-packed
 * 1x1 form (25 taps x C real inputs gathered into 80 / 32 channels) to the tap-by-tap form. */
int rgbd_debug_force_subpix(int32_t mode);
/* ELIC_united's RGB and depth branches run the same layer shapes on independent data (analysis.py:116-174,
 * synthesis.py:126-184,305-323, the per-slice channel-context nets of elic_united.py:288-333): 1 (default) issues each such
 * layer pair as ONE grouped launch (twice the workgroups, half the launches), 0 issues two launches.  Same bits either way. */
int rgbd_debug_force_pair(int32_t mode);
/* Convolution tile tables: mode 0 (default) = the winners of isolated launches (lowest latency of one compress / decompress),
 * mode 1 = the winners with the chip shared between several engine instances (highest job throughput; CodecPool sets it).
 * Results are bit-identical in both modes -- tile choice never changes an output. */
int rgbd_elic_set_tile_mode(rgbd_elic* m, int32_t mode);
int rgbd_debug_bench_streams(int32_t n); /* rgbd_conv_bench: issue every launch on n streams at once (1 = isolated) and
                                            report the time per launch -- the cost of a launch on a shared chip */
int rgbd_debug_force_blocked(int32_t on); /* rgbd_conv_bench: time the blocked-accumulation kernels (tools/tune_tiles.py --blocked) */
int rgbd_debug_force_ckbd(int32_t part); /* rgbd_conv2d_nchw / rgbd_conv_bench: 0 = all outputs, 1 = anchor positions only
                                           ((row + col) odd, utils/ckbd.py:37-48), 2 = non-anchor only; the rest reads 0 */
int rgbd_debug_conv_log(int32_t on);                      /* record the shape of every conv launch (tools/tune_tiles.py) */
int64_t rgbd_debug_conv_log_read(char* buf, int64_t cap); /* CSV text of the recorded shapes; returns the size needed */
int rgbd_debug_force_tile(const char* cfg); /* "wm,mt,nt,kc,dma" or "" = automatic (tools/tile_sweep.py) */
/* every (wm,mt,nt,kc,dma) the conv dispatch can reach, one "wm,mt,nt,kc,dma\n" line each; blocked 0 / 1.
 * Returns the bytes needed (like rgbd_debug_conv_log's reader); touches no device. */
long rgbd_debug_tile_list(int32_t blocked, char* buf, long cap);
/* In-situ tuning (tools/tune_insitu.py): tile / staging form per layer-shape key, lines of
 * "N,H,W,cin_pad,cout_pad,ntaps,stride,nphase,splitk,wm,mt,nt,kc,dma"; "" clears.  rgbd_elic_set_profile(m, 2) makes the profile's
 * layer names carry the shape key of every launch, so one codec call times every layer under its candidate. */
int rgbd_debug_tile_override(const char* csv);

/* The pointwise operators of Bi-SPF / ESA / SE_Block alone (test hook; NCHW device tensors in and out, host weights):
 * op 0 = F.max_pool2d(kernel 7, stride 3) (attention.py:87), 1 = F.interpolate(bilinear, align_corners=False) to (oh, ow)
 * (attention.py:91), 2 = SE_Block x * gate (attention.py:52-67; w0 = fc.0.weight [c/16][c], w1 = fc.2.weight [c][c/16]),
 * 3 = x + x * gate as the entropy-parameter nets use it (entropy.py:75).
 * Every operator runs in its reference-arithmetic form with permuted channels, and stages its tensors through the layout
 * kernels.  The single-chain forms (STF_united, the single-modal STF, the checkerboard Cheng2020 model, the aligner) and the
 * layout kernels themselves are reached through the rgbd_pw_* hooks below. */
int rgbd_pointwise_nchw(int32_t op, const float* x_dev, int32_t n, int32_t c, int32_t h, int32_t w, int32_t oh, int32_t ow,
                        const float* w0, const float* w1, float* y_dev, void* stream);

/* The single-chain pointwise kernels and the two layout kernels alone, on the engine's own layout (test hooks:
 * tests/test_gpu_pointwise_forms.py).  Tensors are NHWC fp32 on the device, [N][pixels][channel stride], with the caller's
 * channel strides; nothing is staged or converted, so pad channels and neighbouring memory stay visible to the caller.  Each
 * call checks its arguments on the host and returns -22 before any launch on a NULL required pointer, a non-positive extent,
 * N > 65535, a channel stride smaller than the channels it has to hold or no multiple of 4, a vector stride (mstride, sstride)
 * smaller than C or no multiple of 4, a pointer its kernel reads or writes in 16-byte vectors that is not 16-byte aligned, one
 * half of an operand pair (x1 without y1), perm / mode / clamp01 outside {0, 1}, or N * stride * pixels >= 2^31 for any
 * tensor; then it calls the launcher the engine calls.  Asynchronous on `stream` unless stated.
 *
 * rgbd_pw_channel_mean: mean_dev[n * mstride + c] = mean over the HW pixels of channel c < C (SE_Block's x.mean((2, 3)),
 *   attention.py:63).  Fixed order: chain r = 0..3 adds pixels r, r + 4, ... one after the other from 0; the total is
 *   (chain0 + chain1) + (chain2 + chain3), divided by float(HW).  Only those N x C floats are written.
 * rgbd_pw_se_gate: gate_dev[n * C + pos] = sigmoid(fc.2 . relu(fc.0 . mean)) (attention.py:64-66); w0 = fc.0.weight
 *   [C/16][C], w1 = fc.2.weight [C][C/16] (HOST; w1 is transposed as rgbd_elic_finalize does it), mean_dev[n * mstride + pos].
 *   perm != 0: channel c sits at position (c & ~15) | (c & 3) << 2 | (c >> 2) & 3 of the mean and gate vectors, and the
 *   sigmoid is the reference-arithmetic one; perm == 0: pos = c, 1 / (1 + expf(-s)).  C % 16 == 0.  Synchronous.
 * rgbd_pw_bilinear: F.interpolate(bilinear, align_corners=False) from (h, w) to (H, W) over all cs channel positions
 *   (attention.py:91).  ref_channels == 0: the single-chain form (source index = scale * (dst + 0.5) - 0.5 as a multiply
 *   and a subtract, taps combined as ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11), every step rounded);
 *   ref_channels = C > 0: the reference-arithmetic form for a tensor of C permuted channels.  x1_dev / y1_dev: NULL, or a
 *   second operand pair of the same shape in the same launch.
 * rgbd_pw_maxpool7s3: F.max_pool2d(kernel 7, stride 3) (attention.py:87) over all cs channel positions, H, W >= 7,
 *   y [N][(H - 7) / 3 + 1][(W - 7) / 3 + 1][cs]; x1_dev / y1_dev as above.
 * rgbd_pw_channel_scale: y[n][p][c] = x * s (mode 0) or x + x * s (mode 1; two roundings), s = scale_dev[n * sstride + c],
 *   c < C, C % 4 == 0; x / y with strides xcs / ycs.  scale_dev and y_dev may point into wider buffers (the gate and the
 *   destination of one half of a concatenation); channels C .. ycs - 1 of y are not written.
 * rgbd_pw_copy_channels: dst[p][c] = src[p][c], c < C, C % 4 == 0, npix pixels with strides scs / dcs.
 * rgbd_pw_im2col5s2: the packed input of the image-consuming Conv2d(C <= 3, k 5, stride 2, pad 2): y [N][(H + 1) / 2]
 *   [(W + 1) / 2][KP]; term = tap * C + c (tap = ky * 5 + kx) = j * 16 + e * 4 + q sits at packed index j * 16 + q * 4 + e;
 *   taps outside the image and the terms 25 C .. KP - 1 are 0.  KP % 16 == 0, 25 C <= KP, C <= cs.
 * rgbd_pw_fill_zero: n floats at p_dev become 0.
 * rgbd_pw_nchw_to_nhwc: src [N][C][H][W] -> dst [N][H][W][cs]; position p holds channel p (perm 0) or the channel whose
 *   permuted position is p (perm 1, cs % 16 == 0); positions that hold no channel < C are written as 0.
 * rgbd_pw_nhwc_to_nchw: the inverse, dst [N][C][H][W]; clamp01: fminf(fmaxf(v, 0), 1) on the way. */
int rgbd_pw_channel_mean(const float* x_dev, int32_t N, int32_t HW, int32_t cs, int32_t C, float* mean_dev, int32_t mstride,
                         void* stream);
int rgbd_pw_se_gate(const float* mean_dev, int32_t N, int32_t C, const float* w0, const float* w1, int32_t mstride, int32_t perm,
                    float* gate_dev, void* stream);
int rgbd_pw_bilinear(const float* x_dev, int32_t N, int32_t h, int32_t w, int32_t cs, float* y_dev, int32_t H, int32_t W,
                     const float* x1_dev, float* y1_dev, int32_t ref_channels, void* stream);
int rgbd_pw_maxpool7s3(const float* x_dev, int32_t N, int32_t H, int32_t W, int32_t cs, float* y_dev, const float* x1_dev,
                       float* y1_dev, void* stream);
int rgbd_pw_channel_scale(const float* x_dev, int32_t N, int32_t HW, int32_t xcs, int32_t C, const float* scale_dev, int32_t sstride,
                          int32_t mode, float* y_dev, int32_t ycs, void* stream);
int rgbd_pw_copy_channels(const float* src_dev, int32_t scs, float* dst_dev, int32_t dcs, int32_t npix, int32_t C, void* stream);
int rgbd_pw_im2col5s2(const float* x_dev, int32_t N, int32_t H, int32_t W, int32_t cs, int32_t C, float* y_dev, int32_t KP,
                      void* stream);
int rgbd_pw_fill_zero(float* p_dev, int64_t n, void* stream);
/* y = 0.5 * tanh(x) over the first C channels (a multiple of 4) of npix NHWC pixels with channel strides xcs / ycs (multiples of
 * 4, 16-byte aligned pointers); x_dev == y_dev is allowed.  LatentResidualPrediction's tail (modules/transform/LRP.py:24-25). */
int rgbd_pw_half_tanh(const float* x_dev, int32_t xcs, float* y_dev, int32_t ycs, int64_t npix, int32_t C, void* stream);
int rgbd_pw_nchw_to_nhwc(const float* src_dev, int32_t N, int32_t C, int32_t H, int32_t W, float* dst_dev, int32_t cs, int32_t perm,
                         void* stream);
int rgbd_pw_nhwc_to_nchw(const float* src_dev, int32_t N, int32_t C, int32_t H, int32_t W, int32_t cs, float* dst_dev,
                         int32_t clamp01, int32_t perm, void* stream);

/* The reference-arithmetic pointwise kernels alone (test hooks; tests/test_gpu_refpointwise.py compares each with
 * oracle/cpu_arith.c bit for bit).  Device tensors are logical NCHW fp32 / vectors in logical channel order, weights and
 * tables are host pointers; the engine's channel permutation stays inside.  Every argument is checked on the host before
 * anything is launched: RGBD_EINVAL (-22) for a null pointer, a non-positive size or anything named below.
 *
 * rgbd_ref_channel_mean: mean over H x W per (image, channel) as ATen's cascade sum forms it (replaces x.mean((2, 3)) of
 *   attention.py:63): mean_dev[image * mstride + channel]; only those n x c floats are written.  c % 16 == 0, mstride >= c.
 * rgbd_ref_linear: y[n][J] = act(x[n][K] . weight[J][K]^T), nn.Linear(bias=False) of SE_Block (attention.py:56-60) in MKL's
 *   summation orders.  row_class: per output row 0 / 1 / 2 (NULL = all 0), used when form == -1; form 3 = the batch-of-two
 *   order for every row.  act 0 / 1 / 3.  stage 0 = fc.0 (the input vector is the engine's mean vector: K % 16 == 0),
 *   stage 1 = fc.2 (the output vector is the engine's gate vector: J % 16 == 0).
 * rgbd_ref_sigmoid_gate: y = sigmoid(t) [* mul] [+ res], each step one fp32 rounding; the sigmoid of element i of the
 *   contiguous [n or 1, c, h, w] tensor is the form torch's CPU kernel run by `threads` threads applies there (vector body or
 *   scalar tail).  per_image 1: every image is a tensor of its own.  mul_dev / res_dev may be NULL.
 * rgbd_ref_small_conv_nchw: conv2d (k <= 3, stride 1 / 2) on ATen's small-tensor route (im2col + sgemm): kblocks = lengths of the
 *   K blocks in k = c * k * k + ky * k + kx (at most 16, summing to cin * k * k; NULL = one block); then + res1, act (0..3),
 *   * mul, + res2.  ckbd 1 / 2 (stride 1 only): only the positions with (row + col) odd / even are computed, the others read 0.
 *   y2_dev (optional): a second copy of the output.  weight [cout][cin][k][k], bias [cout] or NULL (zeros).
 * rgbd_ref_deconv_s2_nchw: conv_transpose2d(k 5, stride 2, pad 2, output_padding 1) in oneDNN brg_deconv's order: recipe = 4 * w
 *   descriptors {ntaps, ntaps x (ky, kx, fresh)} for (phase py * 2 + px, input column), at most 16 taps and 16 chains each,
 *   every tap of its phase's parity.  weight [cin][cout][5][5]; act 0 / 1 / 2. */
int rgbd_ref_channel_mean(const float* x_dev, int32_t n, int32_t c, int32_t h, int32_t w, float* mean_dev, int32_t mstride,
                          void* stream);
int rgbd_ref_linear(const float* weight, const float* x_dev, int32_t n, int32_t K, int32_t J, const int32_t* row_class, int32_t form,
                    int32_t act, int32_t stage, float* y_dev, void* stream);
int rgbd_ref_sigmoid_gate(const float* t_dev, const float* mul_dev, const float* res_dev, int32_t n, int32_t c, int32_t h, int32_t w,
                          int32_t per_image, int32_t threads, float* y_dev, void* stream);
int rgbd_ref_small_conv_nchw(const float* x_dev, int32_t n, int32_t cin, int32_t h, int32_t w, const float* weight, const float* bias,
                             int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t act, int32_t ckbd, const int32_t* kblocks,
                             int32_t nkblocks, const float* res1_dev, const float* mul_dev, const float* res2_dev, float* y_dev,
                             float* y2_dev, void* stream);
int rgbd_ref_deconv_s2_nchw(const float* x_dev, int32_t n, int32_t cin, int32_t h, int32_t w, const float* weight, const float* bias,
                            int32_t cout, int32_t act, const int32_t* recipe, int32_t nrecipe, float* y_dev, void* stream);

/* Kernel-only timing of one convolution shape on NHWC scratch buffers (tools/conv_sweep.py, tools/tune_tiles.py): iters launches,
 * *ms_out = milliseconds per launch. */
int rgbd_conv_bench(int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t k, int32_t stride, int32_t pad,
                    int32_t transposed, int32_t with_residual, int32_t iters, float* ms_out);
int rgbd_elic_profile_dump(rgbd_elic* m, const char* path);

/* Measurement hook (bench.py): when on, every convolution launch is bracketed by HIP events on the launch stream.
 * profile_read returns the summed kernel time (ms), the launch count and the algorithmic FLOPs (2*MACs, unpadded)
 * accumulated since set_profile(). */
/* ---------------------------------------------------------------------------------------------------------------
 * Harness metric: MS-SSIM statistics on the GPU.
 * Replaces the pytorch_msssim.ms_ssim call of utils/metrics.py:8-14 (testing/tester_united.py:92-96) -- 11-tap Gaussian
 * (sigma 1.5) "valid" filtering, SSIM and contrast-structure maps, five dyadic scales with 2x2 average pooling.
 * x, y: device [P][H][W] fp32 planes (P = N * C, contiguous); out: device [P][5][2] = mean SSIM / mean CS per plane and
 * scale, combined by the caller (relu, the five weights, product over scales, mean over channels: rgbd_amd/metrics.py).
 * taps11: the 11 filter taps (host); clamp01: clamp both inputs to [0, 1] first (metrics.py:9-10).  min(H, W) > 160.
 * workspace: device scratch of at least rgbd_msssim_workspace_bytes(P, H, W) bytes.  Deterministic (no atomics).
 * ------------------------------------------------------------------------------------------------------------- */
int64_t rgbd_msssim_workspace_bytes(int32_t P, int32_t H, int32_t W);
int rgbd_msssim_stats(const float* x, const float* y, int32_t P, int32_t H, int32_t W, const float* taps11, float data_range,
                      int32_t clamp01, float* out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * STF_united operator: nn.LayerNorm(C, eps = 1e-5) over the channels of a token (models/stf_united.py:143,155,225,263,
 * 387-391).  x: device [ntok][xcs] fp32 (the first C of xcs channels are the token), w / b: device [C], y: device
 * [ntok][ycs] (channels C .. ycs - 1 are zeroed).  Biased variance, two passes, fixed summation tree.
 * rgbd_debug_force_layernorm_form: -1 by shape (default), 0 one wavefront per token, 1 sixteen lanes per token (C % 4 == 0)
 * -- the two forms are bit-identical (tests).
 * ------------------------------------------------------------------------------------------------------------- */
int rgbd_layernorm(const float* x, int64_t ntok, int32_t C, int32_t xcs, const float* w, const float* b, float* y, int32_t ycs,
                   void* stream);
void rgbd_debug_force_layernorm_form(int32_t form);
/* The same LayerNorm over two operand sets in one launch (the engine's RGB / depth pair): set 1 is x1 / w1 / b1 / y1, of the
 * same ntok / C / xcs / ycs.  Pad channels C .. ycs - 1 of both outputs are zeroed. */
int rgbd_layernorm2(const float* x, int64_t ntok, int32_t C, int32_t xcs, const float* w, const float* b, float* y, int32_t ycs,
                    const float* x1, const float* w1, const float* b1, float* y1, void* stream);

/* STF_united test hooks: the Swin kernels the engine launches, each behind its own operator boundary.  All tensors are NHWC
 * fp32 on the device with a channel stride (xcs / ycs / qcs / ocs floats per pixel).  Each returns RGBD_EINVAL (-22) without
 * launching when an argument breaks what its kernel assumes.
 *
 * rgbd_window_attention: WindowAttention of a 4x4 window with head_dim 16 and the cyclic shift around it
 * (models/stf_united.py:48-114, 162-203).  qkv: [B][H][W][qcs], channel which * C + head * 16 + d (which = q, k, v);
 * rpb: [49][heads] relative position bias table; out: [B][H][W][ocs].  Requires H % 4 == 0, W % 4 == 0, C == 16 * heads,
 * 0 <= shift < 4 (shift > 0: roll by -shift, the -100 mask between the regions of the rolled frame, roll back),
 * qcs >= 3 C, qcs % 4 == 0, ocs >= C, qkv 16-byte aligned, B * (H/4) * (W/4) * heads <= 0x7fffffff - 16.  qkv1 / rpb1 /
 * out1: all NULL, or a second operand set of the same shape run in the same launch.  Pad channels C .. ocs - 1 of out are
 * not written.  (The same kernel as rgbd_guided_window_attention, csrc/swin.hip: window_attention_kernel<head_dim>, behind
 * the same checks.)
 *
 * rgbd_patch_merge_gather: PatchMerging's 2x2 gather (stf_united.py:240-245), y[b][h][w] = cat(x[2h][2w], x[2h+1][2w],
 * x[2h][2w+1], x[2h+1][2w+1]) over the first C channels; x: [B][H][W][xcs], y: [B][H/2][W/2][ycs].  H, W even, C % 4 == 0,
 * xcs % 4 == 0, ycs >= 4 C, ycs % 4 == 0, both 16-byte aligned.  Pad channels 4C .. ycs - 1 of y are not written.
 *
 * rgbd_pixel_shuffle2: nn.PixelShuffle(2) on NHWC, y[b][2h+i][2w+j][c] = x[b][h][w][4c + 2i + j]; x: [B][H][W][xcs] with
 * xcs >= 4 Co, y: [B][2H][2W][ycs] with ycs >= Co.  Pad channels Co .. ycs - 1 of y are zeroed.
 * ------------------------------------------------------------------------------------------------------------- */
int rgbd_window_attention(const float* qkv, int32_t B, int32_t H, int32_t W, int32_t C, int32_t qcs, int32_t heads, int32_t shift,
                          const float* rpb, float* out, int32_t ocs, const float* qkv1, const float* rpb1, float* out1,
                          void* stream);
/* rgbd_guided_window_attention: the cross attention of Spatial_aligner's Swin blocks (modules/transform/spatialAligner.py:
 * WindowAttention.forward :138-170 with the partition / roll / mask of SwinTransformerBlock.forward :279-331 and create_mask
 * :249-277): 4x4 windows, head_dim 32, softmax((q * 32^-0.5) k^T + bias + mask) v.  q: [B][H][W][qcs], channel head * 32 + d
 * (qkv1, :130,147); kv: [B][H][W][kvcs], channel which * C + head * 32 + d, which 0 = k, 1 = v (qkv2, :131,148-149); rpb:
 * [49][heads]; out: [B][H][W][ocs], channels C .. ocs - 1 untouched.  H and W are those of the token grid.  Returns RGBD_EINVAL
 * and writes nothing unless H % 4 == 0, W % 4 == 0, C == 32 * heads, 0 <= shift < 4, qcs >= C, kvcs >= 2 C, ocs >= C,
 * qcs % 4 == 0, kvcs % 4 == 0, q and kv 16-byte aligned, B * (H/4) * (W/4) * heads <= 0x7fffffff - 16, no pointer NULL. */
int rgbd_guided_window_attention(const float* q, int32_t qcs, const float* kv, int32_t kvcs, int32_t B, int32_t H, int32_t W,
                                 int32_t C, int32_t heads, int32_t shift, const float* rpb, float* out, int32_t ocs, void* stream);
/* The kernels of MLIC++'s attention contexts alone (csrc/context_attn.hip; modules/transform/context.py).  fp32, single-chain
 * sums in a fixed order: the same bits on every call, and image b of a batch as it is alone.  Each returns RGBD_EINVAL and
 * writes nothing when a condition below fails or a pointer is NULL.  Inputs and outputs must not overlap.
 * rgbd_local_ckbd_attention: LocalContext.forward :93-133.  qkv: [B][H][W][qcs], channel which * C + c, which 0 / 1 / 2 =
 *   q / k / v, c = d * heads + h (head fast, :102-110); table: relative_position_table [81][heads]; fusion_w: [2C][C][5][5],
 *   fusion_b: [2C]; out: [B][H][W][ocs], channels 0 .. 2C - 1 written (input channel of fusion: h * 16 + d, :127-132),
 *   channels 2C .. ocs - 1 untouched.  Around every position a 5x5 window (zeros outside the map, which still take part in
 *   the softmax); per head softmax_j((q_i / 4) k_j + table[(iy - jy + 4) * 9 + ix - jx + 4][h] + mask[i][j]) v_j with
 *   mask 0 where window positions i and j are both inside the map with (row + col) odd and -100 (a finite addend)
 *   otherwise (:67-78); then fusion over the 25 * C values.  Conditions: C == 32, heads == 2, qcs >= 3C, qcs % 4 == 0,
 *   ocs >= 2C, qkv and fusion_w 16-byte aligned, B <= 65535, H <= 131070, B * H * W <= 0x7fffffff.
 * rgbd_linear_attention: :198-208 (mode 1) and :250-259 (mode 0).  k, q, v, out: [B][H][W][kcs / qcs / vcs / ocs], channel
 *   head * head_dim + d; out channels 0 .. heads * head_dim - 1 written, the others untouched.  Per image and head:
 *   Ks = softmax over the tokens of each key channel, Qs = softmax over the head's channels at each token,
 *   ctx[d1][d2] = sum_n Ks[d1][n] v[d2][n], out[d2][n] = sum_d1 ctx[d1][d2] Qs[d1][n].  mode 0: every position is a token of
 *   all three.  mode 1: the tokens of k and v are the anchor positions ((row + col) odd), those of q the others; out is
 *   written at the query positions and is 0.0f at the anchor positions.  ws: scratch of ws_floats floats, at least
 *   rgbd_linear_attention_ws_floats(...) (which returns RGBD_EINVAL for a shape the kernel refuses).  Conditions: head_dim
 *   16 or 32, mode 0 or 1, W even in mode 1, strides >= heads * head_dim and % 4 == 0, k, q, v, out 16-byte aligned,
 *   B, heads <= 65535, B * H * W <= 0x7fffffff.
 * rgbd_dwconv3x3: nn.Conv2d(C, C, 3, 1, 1, groups = C) (+ nn.GELU(), erf form, when gelu == 1).  x: [B][H][W][xcs],
 *   w: [C][1][3][3], bias: [C], y: [B][H][W][ycs], channels C .. ycs - 1 untouched.  Conditions: xcs >= C, ycs >= C,
 *   gelu 0 or 1, x != y, B * H * W <= 0x7fffffff. */
int rgbd_local_ckbd_attention(const float* qkv, int32_t qcs, int32_t B, int32_t H, int32_t W, int32_t C, int32_t heads,
                              const float* table, const float* fusion_w, const float* fusion_b, float* out, int32_t ocs,
                              void* stream);
int64_t rgbd_linear_attention_ws_floats(int32_t B, int32_t H, int32_t W, int32_t heads, int32_t head_dim, int32_t mode);
int rgbd_linear_attention(const float* k, int32_t kcs, const float* q, int32_t qcs, const float* v, int32_t vcs, int32_t B,
                          int32_t H, int32_t W, int32_t heads, int32_t head_dim, int32_t mode, float* out, int32_t ocs, float* ws,
                          int64_t ws_floats, void* stream);
int rgbd_dwconv3x3(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t xcs, const float* w, const float* bias,
                   int32_t gelu, float* y, int32_t ycs, void* stream);
/* The pooled head of Channel_aligner alone (csrc/pooled_head.hip): AdaptiveAvgPool2d(1) of nn.Conv2d(Cin, Cout, 3, 1, 1),
 * replacing modules/transform/channelAligner.py:30-31 and :35-36 without forming the convolution's output.
 *   out[b][o] = bias[o] + (1 / (H W)) * sum_c sum_(di,dj) w[o][c][di][dj] * S_c(di, dj),
 *   S_c(di, dj) = T_c - (di == 0: last row's sum, di == 2: first row's) - (dj == 0: last column's, dj == 2: first column's)
 *                 + (the corner both took out),
 * which is the mean over all output positions exactly, H = 1 and W = 1 included.  x: [B][H][W][cs] fp32, channels Cin ..
 * cs - 1 never read; w: [Cout][Cin][3][3] and bias: [Cout] as the state dict holds them; out: [B][Cout]; ws: scratch of
 * rgbd_pooled_conv3x3_ws_floats(B, H, W, Cin) floats (which returns RGBD_EINVAL for a shape the kernel refuses).  The map is
 * read once in chunks of pixels whose size depends on H * W only; partial sums (fp32 runs of at most 1024 terms) go through
 * ws and are combined in fp64 in a fixed order, no atomics: the same bits on every call, and image b of a batch as it is
 * alone.  Returns RGBD_EINVAL and writes nothing unless: no pointer NULL; B, H, W >= 1; Cin % 4 == 0, 4 <= Cin <= 1024;
 * 1 <= Cout <= 65535; cs >= Cin, cs % 4 == 0; x and ws 16-byte aligned; B <= 65535; H * W <= 2^30. */
int64_t rgbd_pooled_conv3x3_ws_floats(int32_t B, int32_t H, int32_t W, int32_t Cin);
int rgbd_pooled_conv3x3(const float* x, int32_t cs, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w,
                        const float* bias, int32_t Cout, float* out, float* ws, void* stream);
/* The two thin 3x3 layers of Feature_encoder / Feature_decoder (csrc/thin_conv.hip; models/elic_master.py:18,41; DESIGN.md
 * 5.6): stride 1, zero padding 1, no activation, plain fp32 FMA in a fixed order, no workspace.  w: [Cout][Cin][3][3] on the
 * device, bias: [Cout] on the device or NULL.  The same bits on every call, and image b of a batch as it is alone.
 * rgbd_conv3x3_thin_in: x [B][Cin][H][W] planes, Cin in 1..4 -> y [B][H][W][ycs]; Cout % 4 == 0, 4 <= Cout <= 64; ycs >= Cout,
 * ycs % 4 == 0, y 16-byte aligned; channels Cout .. ycs - 1 of y are not written.
 * rgbd_conv3x3_thin_out: x [B][H][W][xcs], Cin % 4 == 0, 4 <= Cin <= 64, xcs >= Cin, xcs % 4 == 0, x 16-byte aligned, channels
 * Cin .. xcs - 1 never loaded -> y [B][Cout][H][W] planes, Cout in 1..4.  w in convolution orientation: for a
 * ConvTranspose2d(Cin, Cout, 3, 1, 1) weight t [Cin][Cout][3][3] that is w[o][c][ky][kx] = t[c][o][2 - ky][2 - kx].
 * Both return RGBD_EINVAL and write nothing unless the above holds, x, w, y are not NULL, B, H, W >= 1, B <= 65535 and
 * H * W <= 2^30. */
int rgbd_conv3x3_thin_in(const float* x_nchw, int32_t B, int32_t Cin, int32_t H, int32_t W, const float* w, const float* bias,
                         int32_t Cout, float* y_nhwc, int32_t ycs, void* stream);
int rgbd_conv3x3_thin_out(const float* x_nhwc, int32_t xcs, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w,
                          const float* bias, int32_t Cout, float* y_nchw, void* stream);
int rgbd_patch_merge_gather(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t xcs, float* y, int32_t ycs,
                            void* stream);
int rgbd_pixel_shuffle2(const float* x, int32_t B, int32_t H, int32_t W, int32_t Co, int32_t xcs, float* y, int32_t ycs,
                        void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * GDN / IGDN (CompressAI/compressai/layers/gdn.py:22-67), the normalisation of Cheng2020's ResidualBlockWithStride /
 * ResidualBlockUpsample (layers.py:67-126), as ONE launch on the fp32 MFMA:
 *     y[n][i][p] = x[n][i][p] * f(beta'[i] + sum_j gamma'[i][j] * x[n][j][p]^2)  (+ res[n][i][p]),
 * f = 1 / sqrt (inverse = 0) or sqrt (inverse = 1).  It replaces gdn.py:52-67 (parametrizers, x ** 2, F.conv2d, rsqrt / sqrt,
 * multiply) and the `out += identity` of layers.py:97,125.  x_dev / res_dev (optional, may be NULL) / y_dev: device tensors,
 * NCHW fp32, contiguous; beta [c] and gamma [c][c] are the RAW parameters of the state_dict on the host: beta' / gamma' =
 * NonNegativeParametrizer.forward (ops/parametrizers.py:42-45) applied here in fp32, bit for bit torch's values.  Every
 * element is one fp32 chain from beta' over j, a correctly rounded sqrt, an IEEE divide (inverse = 0), the multiply and the
 * add; the bits do not depend on the batch or on the pixel tile.  c in [1, 512], not necessarily a multiple of 16.
 * Returns RGBD_EINVAL (-22) before anything is launched or written on a NULL x / beta / gamma / y, c <= 0, c > 512, a
 * non-positive extent or inverse outside {0, 1}.  Synchronous on return.
 * rgbd_gdn_parametrize: the parameter map alone (host only; is_beta selects the lower bound: 1 = beta, 0 = gamma).
 * rgbd_debug_force_gdn_tile: pixels per workgroup, 64 / 32 (one wave per 16 pixels) or 16 (the output channels spread over
 * four waves: small grids), 0 = automatic (default).  Same bits for every tile.
 * rgbd_gdn_bench: kernel-only time of one launch on NHWC scratch buffers, as rgbd_conv_bench (tools/gdn_probe.py).
 * rgbd_gdn_pack (host only): the raw beta [c] / gamma [c][c] as the kernel's operands, exactly what the engine's finalize
 * uploads: cs = c rounded up to 16; beta_out [cs] = beta', pad channels 1; gamma_out [cs / 16][cs / 16][64][4] = MFMA A
 * fragments, [it][g][lane][e] = gamma'[16 it + lane % 16][16 g + 4 (lane / 16) + e], pad 0.  -22 on a NULL or c outside [1, 512].
 * rgbd_gdn_nhwc: the launch itself on the engine's NHWC device tensors -- the boundary the engine uses: no copies, no layout
 * passes, no synchronisation (asynchronous on `stream`).  x [npix][xcs], y [npix][ycs], res [npix][rcs] (optional, NULL: rcs
 * is ignored); channels [0, cs) are computed, cs a multiple of 16 up to 512 with x's pad channels zero; channels past cs of
 * any tensor are neither read nor written; beta_dev / gamma_dev: rgbd_gdn_pack's output on the device.  inverse: 0 = GDN,
 * otherwise IGDN.  -22 before anything is launched on a NULL x / y / beta / gamma, npix outside [1, 2^30], cs <= 0, cs % 16,
 * cs > 512, a stride below cs or no multiple of 4, or a pointer that is not 16-byte aligned.
 * ------------------------------------------------------------------------------------------------------------- */
int rgbd_gdn_nchw(const float* x_dev, int32_t n, int32_t c, int32_t h, int32_t w, const float* beta, const float* gamma,
                  int32_t inverse, const float* res_dev, float* y_dev, void* stream);
int rgbd_gdn_parametrize(const float* raw, int64_t n, int32_t is_beta, float* out);
int rgbd_debug_force_gdn_tile(int32_t pixels);
int rgbd_gdn_pack(const float* beta_raw, const float* gamma_raw, int32_t c, float* beta_out, float* gamma_out);
int rgbd_gdn_nhwc(const float* x, int32_t xcs, int64_t npix, int32_t cs, const float* beta_dev, const float* gamma_dev,
                  int32_t inverse, const float* res, int32_t rcs, float* y, int32_t ycs, void* stream);
int rgbd_gdn_bench(int32_t n, int32_t c, int32_t h, int32_t w, int32_t inverse, int32_t with_residual, int32_t iters, float* ms_out);

/* Bytes of HBM workspace this engine instance holds (grows with the largest call shape seen, never shrinks); the packed
 * weights, shared by all instances of a pool, are not included.  bench.py reports it as config.hbm_workspace_gib. */
int64_t rgbd_elic_workspace_bytes(const rgbd_elic* m);

/* Number of call shapes whose kernel sequence is currently cached as a HIP graph (tests / diagnostics). */
int rgbd_elic_graph_count(const rgbd_elic* m);
/* Test hook: the next n graph captures are treated as lost (as if another library's device-wide call had invalidated
 * them).  The affected calls must still return correct results (they re-run eagerly); an entry that loses three captures
 * keeps launching eagerly. */
int rgbd_debug_fail_captures(int32_t n);
/* on = 1: event pairs around every conv / GDN launch (graphs off while it is set); 2: the layer names carry the launch's shape key;
 * 3 (MLIC++ handles): pairs around the PHASES of a call instead -- rows "phase.transforms", "phase.contexts", "phase.params",
 * "phase.lrp", "phase.coder" of rgbd_elic_profile_dump -- and none around the launches inside them; 0: off. */
int rgbd_elic_set_profile(rgbd_elic* m, int32_t on);
int rgbd_elic_profile_read(rgbd_elic* m, double* conv_ms, int64_t* launches, double* flops);
/* `flops` above are ALGORITHMIC: the FLOPs of the reference's layers (what bench.py's roofline divides by time).  A launch that
 * computes one checkerboard half of a layer's outputs (the entropy-parameter nets' last layer, utils/ckbd.py:83-125) or meets
 * only half of the taps with non-zero inputs (local-context convs on an anchor-only slice) EXECUTES fewer: this is their sum,
 * so that executed FLOP/s -- what the MFMA-busy counter sees -- can be reported beside the algorithmic figure. */
int rgbd_elic_profile_read_executed(rgbd_elic* m, double* flops_executed);

#ifdef __cplusplus
}
#endif
#endif /* RGBD_AMD_H */
