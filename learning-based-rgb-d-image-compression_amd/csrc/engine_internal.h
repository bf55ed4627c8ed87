// Shared between the translation units of the host runtime (engine.h and the engine*.hip files that define what it declares,
// engine_abi.hip, hooks_abi.hip: the codec; coder_abi.hip: the stand-alone coder and checkerboard operators of the C ABI;
// gdn.hip: the GDN packers).  Not part of the ABI.
#pragma once
#include <algorithm>
#include <memory>
#include <shared_mutex>
#include <vector>

#include "common.h"

// One generation of device buffers: freed when the last engine instance that still points into it lets go.  A parent
// engine and its rgbd_elic_clone_shared() clones share generations, so re-uploading weights or tables on one of them
// (finalize / set_tables / set_scale_table build a NEW generation) can never free memory another one still reads.
struct DevGen {
    std::vector<void*> p;
    ~DevGen()
    {
        for (void* q : p) (void)hipFree(q);
    }
};

// Device scratch of a stand-alone entry point of the C ABI (operator-level calls, test hooks, the bench entry points): one
// allocation per get() (nullptr = out of memory), all released when the call returns, on every way out.
struct DevBufs {
    std::vector<void*> v;
    float* get(size_t floats)
    {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(floats, 1) * sizeof(float)) != hipSuccess) return nullptr;
        v.push_back(p);
        return (float*)p;
    }
    ~DevBufs()
    {
        for (void* p : v) (void)hipFree(p);
    }
};

struct TableSet {
    DevTables d{};
    void* blob = nullptr;
    bool ready = false;
    int stride_src = 0;
    std::shared_ptr<DevGen> hold;  // owner of blob (engine table slots); rgbd_tables frees its blob itself
};

// packs the reference's CDF rows (entropy_models.py:196-204 via ops.cpp:24-81) with the coder's search / division tables
int build_tables(const int32_t* cdf, int stride, const int32_t* sizes, const int32_t* offsets, int nrows, TableSet* ts);

struct rgbd_tables {
    TableSet ts;
};

// Stream capture vs device-wide operations: a hipFree / hipDeviceSynchronize / synchronous hipMemcpy issued by ANY host
// thread while another thread's stream is capturing fails ("operation not permitted when stream is capturing") and
// poisons that capture.  Captures hold this lock shared (several engine instances may capture at once); everything that
// frees or synchronises device-wide takes it exclusively.
extern std::shared_mutex g_capture_mu;

int64_t rgbd_enc_cap_words(int64_t n);  // worst-case words of one stream of n symbols (rgbd_rans_max_bytes / 4)

// GDN parameters (gdn.hip): NonNegativeParametrizer.forward in fp32 on the host, and the packing of one layer's raw beta [c] /
// gamma [c][c] into the operands of GdnArgs
void gdn_parametrize(const float* raw, int64_t n, int is_beta, float* out);
void gdn_pack(const float* beta_raw, const float* gamma_raw, int c, std::vector<float>* beta, std::vector<float>* gamma);

// Factorised prior (entropy.hip: eb_forward_kernel): the raw per-channel parameters of the 1-3-3-3-3-1 cumulative network
// (entropy_models.py:290-312: _matrix{i} [C][f_{i+1}][f_i], _bias{i} [C][f_{i+1}][1], _factor{i} [C][f_{i+1}][1]) as the
// 58 floats per channel the kernel reads: softplus(matrix_i) / bias_i / tanh(factor_i) in layer order, fp32 on the host
void eb_pack_cumulative(const float* const matrix[5], const float* const bias[5], const float* const factor[4], int C, float* prm);
