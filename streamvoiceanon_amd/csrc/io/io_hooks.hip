// Test hooks of the I/O adaptor (include/sva.h): the planner without a GPU, and either kernel over host arrays without a batch.
#include "../../../include/sva.h"
#include "../sva_common.h"
#include "resample.h"

#include <string.h>

#include <string>
#include <vector>

using namespace sva;

extern "C" int sva_test_io_plan(int io_rate, int chunk_frames, const int* blocks, int n_blocks, int* out, int out_cap) {
    SVA_CHECK(out && (blocks || n_blocks == 0) && n_blocks >= 0 && chunk_frames >= 1 && chunk_frames <= 64, "sva_test_io_plan: bad arguments");
    SVA_CHECK(io_rate_supported(io_rate), std::string("sva_test_io_plan: unsupported io_rate ") + std::to_string(io_rate) + ": " + kIoRateRule);
    SVA_CHECK(out_cap >= 12 + 5 * n_blocks, "sva_test_io_plan: out is too short");
    int max_block = 1;
    for (int i = 0; i < n_blocks; ++i) {
        SVA_CHECK(blocks[i] >= 1 && blocks[i] <= (1 << 20), "sva_test_io_plan: block length outside 1 .. 2^20");
        max_block = std::max(max_block, blocks[i]);
    }
    IoPlan pl;
    SVA_CHECK(pl.open(io_rate, chunk_frames, max_block), "sva_test_io_plan: the planner refused this rate");
    const int head[12] = {pl.L, pl.L_filter, pl.nbuf, pl.hist_in, pl.hist_out, pl.fifo_cap, (int)pl.period, pl.in.orig, pl.in.new_, pl.in.width,
                          pl.out.width, max_block};
    for (int i = 0; i < 12; ++i) out[i] = head[i];
    for (int i = 0; i < n_blocks; ++i) {
        const IoCall c = pl.push(blocks[i]);
        int* o = out + 12 + 5 * i;
        o[0] = (int)(c.m1 - c.m0); o[1] = c.steps; o[2] = (int)(c.r1 - c.r0); o[3] = c.in_fill; o[4] = c.out_fill;
    }
    return 12 + 5 * n_blocks;
}

namespace {
struct Dev {
    void* p = nullptr;
    Dev() = default;
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { if (p) (void)hipFree(p); }
    int zalloc(size_t bytes) {
        SVA_HIP(hipMalloc(&p, bytes ? bytes : 4));
        SVA_HIP(hipMemset(p, 0, bytes ? bytes : 4));
        return 0;
    }
};
struct Table {
    ResampleDev d;
    ~Table() { resample_free(&d); }
};
// block boundaries 0 = e[0] < e[1] < ... = n from the split points
int block_edges(const int* splits, int n_splits, long n, std::vector<long>* e) {
    e->assign(1, 0);
    for (int i = 0; i < n_splits; ++i) {
        SVA_CHECK(splits[i] >= e->back() && splits[i] <= n, "sva_test_resample: splits must ascend inside 0 .. n");
        if (splits[i] > e->back() && splits[i] < n) e->push_back(splits[i]);
    }
    e->push_back(n);
    return 0;
}
// one direction over x [B][n] on the host -> every ready output, y [B][count]
int run_direction(bool in_kernel, int from_rate, int to_rate, int fmt_in, int fmt_out, int B, const void* x, long n, const std::vector<long>& edges,
                  std::vector<char>* y, long* count) {
    ResampleTable t;
    t.build(from_rate, to_rate);
    SVA_CHECK(t.monotone(), "sva_test_resample: readiness is not monotone for this pair");
    Table tab;
    if (const int rc = resample_upload(t, &tab.d)) return rc;
    const size_t es_in = fmt_in == kIoFmtI16 ? 2 : 4, es_out = fmt_out == kIoFmtI16 ? 2 : 4;
    const long long M = t.ready(n);
    const int C = 2048, nbuf = (int)(M / C) + 2;
    const int cap = (int)M + 1;
    Dev hist[2], dst;
    for (Dev& h : hist) if (const int rc = h.zalloc(sizeof(float) * (size_t)B * t.history())) return rc;
    if (const int rc = dst.zalloc(in_kernel ? sizeof(float) * (size_t)nbuf * B * C : es_out * (size_t)B * cap)) return rc;
    int par = 0;
    for (size_t i = 0; i + 1 < edges.size(); ++i) {
        const long a = edges[i], len = edges[i + 1] - a;
        Dev blk_;
        if (const int rc = blk_.zalloc(es_in * (size_t)B * len)) return rc;
        SVA_HIP(hipMemcpy2D(blk_.p, es_in * len, (const char*)x + es_in * a, es_in * n, es_in * len, B, hipMemcpyHostToDevice));
        ResampleCall c;
        c.n0 = a; c.j0 = t.ready(a); c.j1 = t.ready(a + len); c.n = (int)len;
        c.hist_old = (const float*)hist[par].p; c.hist_new = (float*)hist[par ^ 1].p;
        par ^= 1;
        const int rc = in_kernel ? launch_io_resample_in(tab.d, c, B, blk_.p, fmt_in, (float*)dst.p, C, nbuf, 0)
                                 : launch_io_resample_out(tab.d, c, B, (const float*)blk_.p, len, dst.p, fmt_out, cap, 0, 0);
        if (rc) return rc;
        SVA_HIP(hipDeviceSynchronize());
    }
    y->assign(es_out * (size_t)B * M, 0);
    if (in_kernel) {
        std::vector<float> st((size_t)nbuf * B * C);
        SVA_HIP(hipMemcpy(st.data(), dst.p, sizeof(float) * st.size(), hipMemcpyDeviceToHost));
        float* o = (float*)y->data();
        for (int s = 0; s < B; ++s)
            for (long long j = 0; j < M; ++j) o[(size_t)s * M + j] = st[((size_t)((j / C) % nbuf) * B + s) * C + j % C];
    } else if (M > 0) {
        SVA_HIP(hipMemcpy2D(y->data(), es_out * M, dst.p, es_out * cap, es_out * M, B, hipMemcpyDeviceToHost));
    }
    *count = (long)M;
    return 0;
}
}  // namespace

extern "C" int sva_test_resample(int device, int from_rate, int to_rate, int fmt_in, int fmt_out, int B, const void* x, long n, const int* splits,
                                 int n_splits, void* y, long y_cap, long* n_out) {
    SVA_CHECK(x && y && n_out && (splits || n_splits == 0) && n_splits >= 0, "sva_test_resample: null argument");
    SVA_CHECK(B >= 1 && B <= 64 && n >= 1 && n <= (1 << 24) && y_cap >= 0, "sva_test_resample: bad sizes");
    const bool run_in = to_rate == kIoModelRate, run_out = from_rate == kIoModelRate;
    SVA_CHECK(run_in || run_out, "sva_test_resample: one of the two rates is 44100");
    SVA_CHECK(io_rate_supported(run_in ? from_rate : to_rate), std::string("sva_test_resample: unsupported rate: ") + kIoRateRule);
    SVA_CHECK((fmt_in == kIoFmtF32 || (fmt_in == kIoFmtI16 && run_in)) && (fmt_out == kIoFmtF32 || (fmt_out == kIoFmtI16 && run_out)),
              "sva_test_resample: int16 is the input format of the in kernel and the output format of the out kernel");
    SVA_HIP(hipSetDevice(device));
    std::vector<long> edges;
    if (const int rc = block_edges(splits, n_splits, n, &edges)) return rc;
    std::vector<char> res;
    long count = n;
    if (run_in)
        if (const int rc = run_direction(true, from_rate, kIoModelRate, fmt_in, kIoFmtF32, B, x, n, edges, &res, &count)) return rc;
    if (run_out) {       // (behind the in kernel only for 44100 -> 44100, where it received every sample: the same cuts apply)
        SVA_CHECK(count == n, "sva_test_resample: the pass-through keeps the length");
        std::vector<char> mid;
        mid.swap(res);
        if (const int rc = run_direction(false, kIoModelRate, to_rate, kIoFmtF32, fmt_out, B, run_in ? (const void*)mid.data() : x, n, edges, &res, &count))
            return rc;
    }
    SVA_CHECK(count <= y_cap, "sva_test_resample: y is too short");
    const size_t es = fmt_out == kIoFmtI16 ? 2 : 4;
    for (int s = 0; s < B; ++s) memcpy((char*)y + es * (size_t)s * y_cap, res.data() + es * (size_t)s * count, es * (size_t)count);
    *n_out = count;
    return 0;
}
