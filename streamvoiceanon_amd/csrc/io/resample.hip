// Streaming polyphase resampler of the I/O adaptor, both directions (resample.h).  One output sample per lane, one workgroup per tile of
// consecutive outputs of one slot; the tile's contiguous input span is staged in LDS, the phase rows are read through L1 / L2 from a table
// stored tap-major, so adjacent lanes -- adjacent phases -- read adjacent floats.  Every output is one serial fmaf chain over its phase's taps,
// first tap upward, in its own lane: the bits do not depend on how the caller cut the signal into blocks.
#include "resample.h"

#include "../kernels.h"
#include "../sva_common.h"

namespace sva {

// round to nearest even of y * 32768, saturated
__device__ inline short to_i16(float y) { return (short)fminf(fmaxf(rintf(y * 32768.f), -32768.f), 32767.f); }

struct StoreStage {
    float* stage; int chunk, nbuf, B;
    __device__ void operator()(int slot, long long j, float v) const {
        const long long c = j / chunk;
        stage[((c % nbuf) * B + slot) * (long long)chunk + (j - c * chunk)] = v;
    }
};
struct StoreFifo {
    void* fifo; int fmt, cap; long long off;
    __device__ void operator()(int slot, long long j, float v) const {
        const long long at = (long long)slot * cap + (j + off) % cap;
        if (fmt == kIoFmtI16) ((short*)fifo)[at] = to_i16(v);
        else ((float*)fifo)[at] = v;
    }
};

namespace {

struct LoadF32 {
    const float* p; long bstride;
    __device__ float operator()(int slot, int i) const { return p[(long)slot * bstride + i]; }
};
struct LoadI16 {
    const short* p; long bstride;
    __device__ float operator()(int slot, int i) const { return (float)p[(long)slot * bstride + i] / 32768.f; }
};
// input sample `idx` (absolute) of `slot`: history below n0, the block from n0 on; zero where neither holds it (no ready output reads there)
template <class Load>
__device__ inline float input_at(const ResampleDev& d, const ResampleCall& c, const Load& load, int slot, long long idx) {
    if (idx < c.n0) {
        const long long h = idx - (c.n0 - d.hist);
        return h >= 0 ? c.hist_old[(long)slot * d.hist + h] : 0.f;
    }
    return idx >= c.n0 + c.n ? 0.f : load(slot, (int)(idx - c.n0));
}

// grid (tiles + history blocks, B).  Blocks 0 .. n_tiles - 1 compute outputs, the rest write the next call's history.
template <class Load, class Store>
__device__ inline void resample_block(const ResampleDev& d, const ResampleCall& c, const Load& load, const Store& store, bool mute_input, float* xs) {
    const int slot = blockIdx.y, tid = threadIdx.x;
    const bool muted = mute_input && c.slot_flag && (c.slot_flag[slot] & kSlotInputMuted);
    const int n_tiles = (int)((c.j1 - c.j0 + kIoTile - 1) / kIoTile);
    if ((int)blockIdx.x >= n_tiles) {
        const int q = ((int)blockIdx.x - n_tiles) * kIoTile + tid;
        if (q < d.hist) c.hist_new[(long)slot * d.hist + q] = muted ? 0.f : input_at(d, c, load, slot, c.n0 + c.n - d.hist + q);
        return;
    }
    const long long jt0 = c.j0 + (long long)blockIdx.x * kIoTile;
    const int nj = (int)(c.j1 - jt0 < kIoTile ? c.j1 - jt0 : kIoTile);
    if (muted) {
        if (tid < nj) store(slot, jt0 + tid, 0.f);
        return;
    }
    const long long i0 = jt0 / d.new_;
    const int p0 = (int)(jt0 - i0 * d.new_);
    const long long s0 = i0 * d.orig - d.width;
    const int span = ((p0 + nj - 1) / d.new_) * d.orig + d.taps;          // <= d.lds_floats
    for (int k = tid; k < span; k += kIoTile) xs[k] = input_at(d, c, load, slot, s0 + k);
    __syncthreads();
    if (tid >= nj) return;
    const int jl = p0 + tid, ir = jl / d.new_, p = jl - ir * d.new_;
    const int base = ir * d.orig + d.lo[p];
    float acc;
    if (d.identity) {
        acc = xs[base];
    } else {
        acc = 0.f;
        const int nt = d.cnt[p];
        const float* kp = d.k + p;
        for (int s = 0; s < nt; ++s) acc = fmaf(kp[(long)s * d.new_], xs[base + s], acc);
    }
    store(slot, jt0 + tid, acc);
}

}  // namespace

__global__ __launch_bounds__(kIoTile) void io_resample_in_kernel(ResampleDev d, ResampleCall c, const void* block, int fmt, StoreStage store) {
    extern __shared__ __align__(16) float io_xs[];
    if (fmt == kIoFmtI16) resample_block(d, c, LoadI16{(const short*)block, c.n}, store, true, io_xs);
    else resample_block(d, c, LoadF32{(const float*)block, c.n}, store, true, io_xs);
}

__global__ __launch_bounds__(kIoTile) void io_resample_out_kernel(ResampleDev d, ResampleCall c, const float* block, long block_bstride, StoreFifo store) {
    extern __shared__ __align__(16) float io_xs[];
    resample_block(d, c, LoadF32{block, block_bstride}, store, false, io_xs);
}

int resample_upload(const ResampleTable& t, ResampleDev* out) {
    ResampleDev d;
    d.orig = t.orig; d.new_ = t.new_; d.width = t.width; d.taps = t.taps; d.identity = t.identity ? 1 : 0;
    d.hist = t.history();
    d.lds_floats = ((kIoTile - 1) / t.new_ + 1) * t.orig + t.taps;
    std::vector<int> cnt(t.new_);
    for (int p = 0; p < t.new_; ++p) cnt[p] = t.hi[p] - t.lo[p] + 1;
    float* k = nullptr; int *lo = nullptr, *cn = nullptr;
    SVA_HIP(hipMalloc((void**)&k, sizeof(float) * t.k.size()));
    d.k = k;
    SVA_HIP(hipMalloc((void**)&lo, sizeof(int) * t.new_));
    d.lo = lo;
    SVA_HIP(hipMalloc((void**)&cn, sizeof(int) * t.new_));
    d.cnt = cn;
    *out = d;
    SVA_HIP(hipMemcpy(k, t.k.data(), sizeof(float) * t.k.size(), hipMemcpyHostToDevice));
    SVA_HIP(hipMemcpy(lo, t.lo.data(), sizeof(int) * t.new_, hipMemcpyHostToDevice));
    SVA_HIP(hipMemcpy(cn, cnt.data(), sizeof(int) * t.new_, hipMemcpyHostToDevice));
    return 0;
}
void resample_free(ResampleDev* d) {
    if (d->k) (void)hipFree((void*)d->k);
    if (d->lo) (void)hipFree((void*)d->lo);
    if (d->cnt) (void)hipFree((void*)d->cnt);
    *d = ResampleDev();
}

static int check_call(const ResampleDev& d, const ResampleCall& c, int B) {
    SVA_CHECK(B >= 1 && c.n >= 1 && c.j1 >= c.j0 && c.n0 >= 0 && c.hist_old && c.hist_new && c.hist_old != c.hist_new, "io resample: bad call");
    SVA_CHECK(d.k && d.lo && d.cnt && (size_t)d.lds_floats * sizeof(float) <= 64 * 1024, "io resample: table not uploaded");
    return 0;
}
static dim3 call_grid(const ResampleDev& d, const ResampleCall& c, int B) {
    return dim3((unsigned)((c.j1 - c.j0 + kIoTile - 1) / kIoTile + (d.hist + kIoTile - 1) / kIoTile), B);
}

int launch_io_resample_in(const ResampleDev& d, const ResampleCall& c, int B, const void* block, int fmt, float* stage, int chunk, int nbuf,
                          hipStream_t st) {
    if (const int rc = check_call(d, c, B)) return rc;
    SVA_CHECK(block && stage && (fmt == kIoFmtF32 || fmt == kIoFmtI16) && chunk >= 1 && nbuf >= 1, "io_resample_in: bad argument");
    SVA_CHECK(c.j1 - c.j0 <= (long long)(nbuf - 1) * chunk + 1, "io_resample_in: more outputs than the staging buffers hold");
    hipLaunchKernelGGL(io_resample_in_kernel, call_grid(d, c, B), dim3(kIoTile), sizeof(float) * d.lds_floats, st, d, c, block, fmt,
                       StoreStage{stage, chunk, nbuf, B});
    SVA_HIP(hipGetLastError());
    return 0;
}

int launch_io_resample_out(const ResampleDev& d, const ResampleCall& c, int B, const float* block, long block_bstride, void* fifo, int fmt,
                           int fifo_cap, long long fifo_off, hipStream_t st) {
    if (const int rc = check_call(d, c, B)) return rc;
    SVA_CHECK(block && fifo && (fmt == kIoFmtF32 || fmt == kIoFmtI16) && block_bstride >= c.n && fifo_off >= 0, "io_resample_out: bad argument");
    SVA_CHECK(c.j1 - c.j0 <= fifo_cap, "io_resample_out: more outputs than the FIFO holds");
    hipLaunchKernelGGL(io_resample_out_kernel, call_grid(d, c, B), dim3(kIoTile), sizeof(float) * d.lds_floats, st, d, c, block, block_bstride,
                       StoreFifo{fifo, fmt, fifo_cap, fifo_off});
    SVA_HIP(hipGetLastError());
    return 0;
}

}  // namespace sva
