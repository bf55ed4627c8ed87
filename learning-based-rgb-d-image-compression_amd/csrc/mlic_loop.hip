// MLIC++'s slice loop on gfx950 (models/mlicpp.py:220-303): the two things a coding part does to its slot of the state buffer
// besides running networks.  The loop keeps hyper_means and the ten decoded slices side by side in one NHWC buffer
// [B][h][w][2M] (mlic_engine.hip), so "slice_anchor + ckbd_anchor(lrp)" (mlicpp.py:235, 257) is an update in place of one
// checkerboard half of 32 channels: one launch per part instead of 0.5 * tanh, a masked add and a copy -- twenty parts sit on a
// serial chain.  Plain fp32 vector code: a thread owns 16 bytes of a pixel's 32-channel run; the grid is cut by pixel of the
// part's parity ((row + col) odd is the anchor, as ckbd_part_kernel has it), so the other half is neither read nor written.
#include "common.h"

typedef float mlic_f4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kQuads = MLIC_SLOT_CH / 4;  // 16-byte pieces of a slot's channel run

// pixel-of-parity index t -> pixel (b, row, col), or false past the row's end (odd w: the rows' halves differ by one)
__device__ __forceinline__ bool parity_pixel(size_t t, int h, int w, int parity, size_t* pix)
{
    const int w2 = (w + 1) / 2;
    const int k = (int)(t % w2);
    const size_t br = t / w2;  // b * h + row
    const int row = (int)(br % h);
    const int col = 2 * k + (parity == 0 ? 1 - (row & 1) : (row & 1));
    *pix = br * w + col;
    return col < w;
}

__global__ void mlic_lrp_apply_kernel(float* __restrict__ slot, int scs, const float* __restrict__ r, int rcs, int h, int w, int parity,
                                      size_t total)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(i % kQuads);
        size_t pix;
        if (!parity_pixel(i / kQuads, h, w, parity, &pix)) continue;
        const mlic_f4 x = *(const mlic_f4*)(r + pix * rcs + 4 * q);
        mlic_f4 v = *(const mlic_f4*)(slot + pix * scs + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(v[e], half_tanh_of(x[e]));  // half_tanh_kernel's value, then one fp32 add
        *(mlic_f4*)(slot + pix * scs + 4 * q) = v;
    }
}

__global__ void mlic_slot_clear_kernel(float* __restrict__ slot, int scs, int h, int w, int parity, size_t total)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(i % kQuads);
        size_t pix;
        if (!parity_pixel(i / kQuads, h, w, parity, &pix)) continue;
        *(mlic_f4*)(slot + pix * scs + 4 * q) = (mlic_f4){0.f, 0.f, 0.f, 0.f};
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// what both launchers require of a slot-shaped operand
inline bool slot_ok(const float* p, int cs, int C, int B, int h, int w, int parity)
{
    return p && aligned16(p) && C == MLIC_SLOT_CH && cs >= C && cs % 4 == 0 && B > 0 && h > 0 && w > 0 && (parity == 0 || parity == 1) &&
           (int64_t)B * h * w * cs <= 0x7fffffff;
}

inline size_t work_of(int B, int h, int w) { return (size_t)B * h * ((w + 1) / 2) * kQuads; }

inline unsigned grid_of(size_t work)
{
    const size_t n = (work + 255) / 256;
    return (unsigned)(n < 1 ? 1 : (n > 2048 ? 2048 : n));
}

}  // namespace

int launch_mlic_lrp_apply(float* slot, int scs, const float* r, int rcs, int C, int B, int h, int w, int parity, hipStream_t s)
{
    if (!slot_ok(slot, scs, C, B, h, w, parity) || !slot_ok(r, rcs, C, B, h, w, parity) || slot == r) return RGBD_EINVAL;
    const size_t total = work_of(B, h, w);
    hipLaunchKernelGGL(mlic_lrp_apply_kernel, dim3(grid_of(total)), dim3(256), 0, s, slot, scs, r, rcs, h, w, parity, total);
    HIP_TRY(hipGetLastError());
    return RGBD_OK;
}

int launch_mlic_slot_clear(float* slot, int scs, int C, int B, int h, int w, int parity, hipStream_t s)
{
    if (!slot_ok(slot, scs, C, B, h, w, parity)) return RGBD_EINVAL;
    const size_t total = work_of(B, h, w);
    hipLaunchKernelGGL(mlic_slot_clear_kernel, dim3(grid_of(total)), dim3(256), 0, s, slot, scs, h, w, parity, total);
    HIP_TRY(hipGetLastError());
    return RGBD_OK;
}

// ---- C ABI (include/rgbd_amd.h): the two kernels alone, on device pointers the caller owns ----
extern "C" int rgbd_mlic_lrp_apply(float* slot_dev, int32_t slot_cs, const float* r_dev, int32_t r_cs, int32_t channels, int32_t B,
                                   int32_t h, int32_t w, int32_t parity, void* stream)
{
    return launch_mlic_lrp_apply(slot_dev, slot_cs, r_dev, r_cs, channels, B, h, w, parity, (hipStream_t)stream);
}

extern "C" int rgbd_mlic_slot_clear(float* slot_dev, int32_t slot_cs, int32_t channels, int32_t B, int32_t h, int32_t w,
                                    int32_t parity, void* stream)
{
    return launch_mlic_slot_clear(slot_dev, slot_cs, channels, B, h, w, parity, (hipStream_t)stream);
}
