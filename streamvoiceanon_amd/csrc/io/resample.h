// The two kernels of the I/O adaptor (sva_io_*): a streaming polyphase resampler in each direction, arithmetic and readiness rule as io_plan.h
// states them.  Sample counters live on the host (IoPlan) and arrive as launch arguments, so the launches stay outside every captured graph.
#pragma once
#include <hip/hip_runtime.h>

#include "io_plan.h"

namespace sva {

constexpr int kIoFmtF32 = 0, kIoFmtI16 = 1;
constexpr int kIoTile = 256;               // outputs of one workgroup, one per lane

// one direction's table on the device
struct ResampleDev {
    const float* k = nullptr;              // [support][new]
    const int* lo = nullptr;               // [new] first tap of the phase
    const int* cnt = nullptr;              // [new] taps of the phase
    int orig = 1, new_ = 1, width = 0, taps = 1, identity = 1;
    int hist = 1;                          // history samples per slot
    int lds_floats = 0;                    // input span one tile stages in LDS
};
int resample_upload(const ResampleTable& t, ResampleDev* out);        // hipMalloc; resample_free releases
void resample_free(ResampleDev* d);

// what both kernels share: outputs [j0, j1) of every slot from the history (inputs [n0 - hist, n0)) and the block (inputs [n0, n0 + n)); the
// history of the next call is written to hist_new (the two buffers alternate, so no workgroup reads what another one writes)
struct ResampleCall {
    long long n0 = 0, j0 = 0, j1 = 0;
    int n = 0;
    const float* hist_old = nullptr;       // [B][hist]
    float* hist_new = nullptr;
    const int* slot_flag = nullptr;
};

// caller block [B][n] (fmt) -> chunk staging: sample j of slot s at stage[((j / chunk) % nbuf * B + s) * chunk + j % chunk].  A kSlotInputMuted
// slot's block is not read: zeros are staged and its history becomes zeros.
int launch_io_resample_in(const ResampleDev& d, const ResampleCall& c, int B, const void* block, int fmt, float* stage, int chunk, int nbuf,
                          hipStream_t st);
// step output [B] rows of n floats, row stride block_bstride -> output FIFO (fmt): sample j of slot s at fifo[s * fifo_cap + (j + fifo_off) % fifo_cap]
int launch_io_resample_out(const ResampleDev& d, const ResampleCall& c, int B, const float* block, long block_bstride, void* fifo, int fmt,
                           int fifo_cap, long long fifo_off, hipStream_t st);

}  // namespace sva
