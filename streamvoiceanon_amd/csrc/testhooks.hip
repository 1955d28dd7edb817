// Kernel unit-test hooks exported through the C ABI (include/sva.h: sva_test_*).
#include "../../include/sva.h"
#include "kernels.h"
#include "engine.h"
#include "engine_kernels.h"
#include "stream_overlap.h"
#include "ar_device.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

using namespace sva;

#define SVA_TRY(expr)            \
    do {                         \
        const int _rc = (expr);  \
        if (_rc) return _rc;     \
    } while (0)

static int test_gemm_impl(int device, int M, int N, int K, const float* A, const float* W, const float* bias, float* C, const int* choice);
// The kind numbers of sva_test_gemm_choice (include/sva.h) as plans.  The planes kernel's variants 0 .. 7 / 9 .. 14 are two families (GemmFamily).
static GemmPlan test_choice_plan(int kind, int a, int b, int c) {
    static const GemmFamily fam[8] = {GemmFamily::SmallM, GemmFamily::Tiled, GemmFamily::SmallM, GemmFamily::Ring, GemmFamily::Split, GemmFamily::SmallM,
                                      GemmFamily::Planes, GemmFamily::Stream};
    if (kind < 0 || kind > 7 || kind == 5) return GemmPlan{GemmFamily::SmallM, -1, 0, 0, 1};      // (no plan takes a = -1: refused)
    if (kind == 2) return GemmPlan{GemmFamily::SmallM, a, b, c & 15, c >> 4};
    return GemmPlan{kind == 6 && a >= 8 ? GemmFamily::PlanesDma : fam[kind], a, b, c, 1};
}
extern "C" int sva_test_gemm(int device, int M, int N, int K, const float* A, const float* W, const float* bias, float* C) {
    return test_gemm_impl(device, M, N, K, A, W, bias, C, nullptr);
}
extern "C" int sva_test_gemm_choice(int device, int M, int N, int K, const float* A, const float* W, const float* bias, float* C, int kind,
                                    int a, int b, int c) {
    const int ch[4] = {kind, a, b, c};
    return test_gemm_impl(device, M, N, K, A, W, bias, C, ch);
}
static int test_gemm_impl(int device, int M, int N, int K, const float* A, const float* W, const float* bias, float* C, const int* choice) {
    SVA_HIP(hipSetDevice(device));
    float *dA, *dW, *dB = nullptr, *dC;
    SVA_HIP(hipMalloc(&dA, sizeof(float) * (size_t)M * K));
    SVA_HIP(hipMalloc(&dW, sizeof(float) * (size_t)N * K));
    SVA_HIP(hipMalloc(&dC, sizeof(float) * (size_t)M * N));
    SVA_HIP(hipMemcpy(dA, A, sizeof(float) * (size_t)M * K, hipMemcpyHostToDevice));
    SVA_HIP(hipMemcpy(dW, W, sizeof(float) * (size_t)N * K, hipMemcpyHostToDevice));
    if (bias) {
        SVA_HIP(hipMalloc(&dB, sizeof(float) * N));
        SVA_HIP(hipMemcpy(dB, bias, sizeof(float) * N, hipMemcpyHostToDevice));
    }
    ConvGemm g;
    g.A = dA; g.a_bstride = (long)M * K; g.lda = K; g.T = M; g.M = M; g.Cin = K; g.taps = 1;
    g.W = dW; g.N = N; g.bias = dB; g.C = dC; g.c_bstride = (long)M * N; g.ldc = N;
    const GemmPlan p = choice ? test_choice_plan(choice[0], choice[1], choice[2], choice[3]) : GemmPlan();
    int rc = !choice ? launch_conv_gemm(g, 0) : launch_conv_gemm_plan(g, p, 0);
    if (!rc && choice && p.z > 1) rc = launch_conv_gemm_plan(g, p, 0);   // a grid-level K split twice: the counters re-arm
    if (rc) return rc;
    SVA_HIP(hipDeviceSynchronize());
    SVA_HIP(hipMemcpy(C, dC, sizeof(float) * (size_t)M * N, hipMemcpyDeviceToHost));
    (void)hipFree(dA); (void)hipFree(dW); (void)hipFree(dC); if (dB) (void)hipFree(dB);
    return 0;
}

// fp16-weight GEMM of the batched fp16 AR (gemm_f16w.hip): W is rounded to fp16 here; mode bits: 1 = RMSNorm prologue (rms_w [K]),
// 2 = residual add (res [M][N]), 4 = SwiGLU over 16-row interleaved (gate, up) weights (C is [M][N/2]).  iters > 0 also times it.
extern "C" int sva_test_gemm_f16w(int device, int M, int N, int K, const float* A, const float* W, const float* bias, const float* rms_w,
                                  const float* res, int mode, float* C, int iters, float* out_us) {
    SVA_HIP(hipSetDevice(device));
    const int NC = (mode & 4) ? N / 2 : N;
    float *dA, *dC, *dB = nullptr, *dN = nullptr, *dR = nullptr;
    uint16_t* dW;
    std::vector<uint16_t> hb((size_t)N * K);
    for (size_t i = 0; i < hb.size(); ++i) { const _Float16 h = (_Float16)W[i]; memcpy(&hb[i], &h, 2); }
    SVA_HIP(hipMalloc(&dA, sizeof(float) * (size_t)M * K));
    SVA_HIP(hipMalloc(&dW, 2 * (size_t)N * K));
    SVA_HIP(hipMalloc(&dC, sizeof(float) * (size_t)M * NC));
    SVA_HIP(hipMemcpy(dA, A, sizeof(float) * (size_t)M * K, hipMemcpyHostToDevice));
    SVA_HIP(hipMemcpy(dW, hb.data(), 2 * (size_t)N * K, hipMemcpyHostToDevice));
    if (bias) { SVA_HIP(hipMalloc(&dB, sizeof(float) * N)); SVA_HIP(hipMemcpy(dB, bias, sizeof(float) * N, hipMemcpyHostToDevice)); }
    if (mode & 1) { SVA_HIP(hipMalloc(&dN, sizeof(float) * K)); SVA_HIP(hipMemcpy(dN, rms_w, sizeof(float) * K, hipMemcpyHostToDevice)); }
    if (mode & 2) { SVA_HIP(hipMalloc(&dR, sizeof(float) * (size_t)M * N)); SVA_HIP(hipMemcpy(dR, res, sizeof(float) * (size_t)M * N, hipMemcpyHostToDevice)); }
    ConvGemm g;
    g.A = dA; g.a_bstride = (long)M * K; g.lda = K; g.T = M; g.M = M; g.Cin = K; g.taps = 1;
    g.Wh = dW; g.N = N; g.bias = dB; g.C = dC; g.c_bstride = (long)M * NC; g.ldc = NC;
    g.rms_w = dN; g.res = dR; g.r_bstride = (long)M * N; g.ldr = N; g.w13 = (mode & 4) ? 1 : 0;
    SVA_CHECK(f16w_gemm_supported(g), "sva_test_gemm_f16w: unsupported shape");
    { const int rc = launch_f16w_gemm(g, 0); if (rc) return rc; }
    SVA_HIP(hipDeviceSynchronize());
    SVA_HIP(hipMemcpy(C, dC, sizeof(float) * (size_t)M * NC, hipMemcpyDeviceToHost));
    if (iters > 0 && out_us) {
        hipEvent_t e0, e1;
        SVA_HIP(hipEventCreate(&e0)); SVA_HIP(hipEventCreate(&e1));
        SVA_HIP(hipEventRecord(e0, 0));
        for (int i = 0; i < iters; ++i) if (launch_f16w_gemm(g, 0)) return -1;
        SVA_HIP(hipEventRecord(e1, 0));
        SVA_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        SVA_HIP(hipEventElapsedTime(&ms, e0, e1));
        *out_us = ms * 1000.f / iters;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    (void)hipFree(dA); (void)hipFree(dW); (void)hipFree(dC);
    if (dB) (void)hipFree(dB); if (dN) (void)hipFree(dN); if (dR) (void)hipFree(dR);
    return 0;
}

// Device buffer of a test hook: freed when the hook returns, on every path
namespace {
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) { SVA_HIP(hipMalloc(&p, bytes ? bytes : 4)); return 0; }
    int put(const void* host, size_t bytes) {
        SVA_TRY(alloc(bytes));
        if (bytes) SVA_HIP(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
        return 0;
    }
    int get(void* host, size_t bytes) const {
        if (bytes) SVA_HIP(hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost));
        return 0;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};
std::vector<uint16_t> to_half_bits(const float* v, size_t n) {
    std::vector<uint16_t> h(n);
    for (size_t i = 0; i < n; ++i) { const _Float16 hv = (_Float16)v[i]; memcpy(&h[i], &hv, 2); }
    return h;
}
}  // namespace

// Prefill / pair attention hooks: M query rows at positions pos0 .. pos0 + M - 1 of slot 0 against a cache holding `keys` [pos0 + M][H*64] /
// `vals` (fp32, or rounded to fp16 when half_kv): out_ref = the per-row kernel (ar_attention_kernel), out_b = kernel B -- the flash-style MFMA
// kernel (ar_prefill_attention_kernel, pairs == 0) or the decode frame's PAIRED kernel (rows 2 i, 2 i + 1 = consecutive positions; M even);
// us[0], us[1] = their average launch times over `iters`.
static int test_attention_vs_per_row(int device, bool pairs, int M, int H, int pos0, int S, const float* q, const float* keys, const float* vals,
                                     int half_kv, float* out_ref, float* out_b, int iters, float* us) {
    SVA_HIP(hipSetDevice(device));
    const int D = H * 64, L = pos0 + M;
    SVA_CHECK(L <= S, "attention test hook: pos0 + M must fit the cache");
    std::vector<float> qkv((size_t)M * 3 * D, 0.f);
    for (int m = 0; m < M; ++m) memcpy(&qkv[(size_t)m * 3 * D], q + (size_t)m * D, sizeof(float) * D);
    const size_t cache_elems = (size_t)2 * H * S * 64;
    std::vector<float> cf(cache_elems, 0.f);
    for (int j = 0; j < L; ++j)
        for (int h = 0; h < H; ++h)
            for (int dd = 0; dd < 64; ++dd) {
                cf[((size_t)h * S + j) * 64 + dd] = keys[(size_t)j * D + h * 64 + dd];
                cf[(size_t)H * S * 64 + ((size_t)h * S + j) * 64 + dd] = vals[(size_t)j * D + h * 64 + dd];
            }
    std::vector<int> slot(M, 0), pos(M);
    for (int m = 0; m < M; ++m) pos[m] = pos0 + m;
    DevBuf bq, bc, bo1, bo2, bs, bp, bch;
    SVA_TRY(bq.put(qkv.data(), sizeof(float) * qkv.size()));
    SVA_TRY(bc.put(cf.data(), sizeof(float) * cache_elems));
    SVA_TRY(bo1.alloc(sizeof(float) * (size_t)M * D));
    SVA_TRY(bo2.alloc(sizeof(float) * (size_t)M * D));
    SVA_TRY(bs.put(slot.data(), sizeof(int) * M));
    SVA_TRY(bp.put(pos.data(), sizeof(int) * M));
    if (half_kv) {
        const std::vector<uint16_t> ch = to_half_bits(cf.data(), cache_elems);
        SVA_TRY(bch.put(ch.data(), 2 * cache_elems));
    }
    float *dq = bq.as<float>(), *dc = bc.as<float>(), *do1 = bo1.as<float>(), *do2 = bo2.as<float>();
    const int *ds = bs.as<int>(), *dp = bp.as<int>();
    const __half* c16 = bch.as<__half>();
    const long slot_stride = (long)cache_elems;
    auto run = [&](int which) -> int {
        if (half_kv) {
            if (!which) return launch_ar_attention<__half>(dq, M, H, 64, ds, dp, c16, slot_stride, S, do1, 0);
            return pairs ? launch_ar_attention_pairs<__half>(dq, M, H, 64, ds, dp, c16, slot_stride, S, do2, 0)
                         : launch_ar_prefill_attention<__half>(dq, M, H, 64, 0, pos0, c16, slot_stride, S, do2, 0);
        }
        if (!which) return launch_ar_attention<float>(dq, M, H, 64, ds, dp, dc, slot_stride, S, do1, 0);
        return pairs ? launch_ar_attention_pairs<float>(dq, M, H, 64, ds, dp, dc, slot_stride, S, do2, 0)
                     : launch_ar_prefill_attention<float>(dq, M, H, 64, 0, pos0, dc, slot_stride, S, do2, 0);
    };
    for (int which = 0; which < 2; ++which) {
        if (run(which)) return -1;
        SVA_HIP(hipDeviceSynchronize());
        if (iters > 0 && us) {
            hipEvent_t e0, e1;
            SVA_HIP(hipEventCreate(&e0)); SVA_HIP(hipEventCreate(&e1));
            SVA_HIP(hipEventRecord(e0, 0));
            for (int i = 0; i < iters; ++i) if (run(which)) return -1;
            SVA_HIP(hipEventRecord(e1, 0));
            SVA_HIP(hipEventSynchronize(e1));
            float ms = 0.f;
            SVA_HIP(hipEventElapsedTime(&ms, e0, e1));
            us[which] = ms * 1000.f / iters;
            (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        }
    }
    SVA_TRY(bo1.get(out_ref, sizeof(float) * (size_t)M * D));
    SVA_TRY(bo2.get(out_b, sizeof(float) * (size_t)M * D));
    return 0;
}
extern "C" int sva_test_prefill_attention(int device, int M, int H, int pos0, int S, const float* q, const float* keys, const float* vals,
                                          int half_kv, float* out_ref, float* out_mfma, int iters, float* us) {
    return test_attention_vs_per_row(device, false, M, H, pos0, S, q, keys, vals, half_kv, out_ref, out_mfma, iters, us);
}
extern "C" int sva_test_prefill_attention_runs(int device, int n_runs, const int* runs, int total_rows, int H, int S, int n_slots, int half_kv, const float* q,
                                               const float* cache, float* out, float* single_out) {
    SVA_CHECK(runs && q && cache && out && n_runs >= 0 && total_rows >= 1 && H >= 1 && S >= 1 && n_slots >= 1, "sva_test_prefill_attention_runs: bad arguments");
    SVA_HIP(hipSetDevice(device));
    const int D = H * 64;
    const size_t slot_elems = (size_t)2 * H * S * 64, cache_elems = slot_elems * n_slots, out_elems = (size_t)total_rows * D;
    std::vector<float> qkv((size_t)total_rows * 3 * D, 0.f);
    for (int m = 0; m < total_rows; ++m) memcpy(&qkv[(size_t)m * 3 * D], q + (size_t)m * D, sizeof(float) * D);
    DevBuf bq, bc, bo, bo1, bt;
    SVA_TRY(bq.put(qkv.data(), sizeof(float) * qkv.size()));
    if (half_kv) {
        const std::vector<uint16_t> ch = to_half_bits(cache, cache_elems);
        SVA_TRY(bc.put(ch.data(), 2 * cache_elems));
    } else {
        SVA_TRY(bc.put(cache, sizeof(float) * cache_elems));
    }
    SVA_TRY(bo.put(out, sizeof(float) * out_elems));
    PrefillTiles tt;
    tt.max_runs = (size_t)std::max(n_runs, 1); tt.max_tiles = (size_t)total_rows / 16 + tt.max_runs;
    SVA_TRY(bt.alloc(sizeof(int) * (4 * tt.max_runs + 2 * tt.max_tiles)));
    tt.dev = bt.as<int>();
    const int rc = half_kv ? launch_ar_prefill_attention_runs<__half>(bq.as<float>(), runs, n_runs, total_rows, H, 64, bc.as<__half>(), (long)slot_elems, n_slots, S,
                                                                      bo.as<float>(), tt, 0)
                           : launch_ar_prefill_attention_runs<float>(bq.as<float>(), runs, n_runs, total_rows, H, 64, bc.as<float>(), (long)slot_elems, n_slots, S,
                                                                     bo.as<float>(), tt, 0);
    if (rc) return 1;                                 // refused: nothing was launched, the caller's arrays are as they were
    SVA_HIP(hipDeviceSynchronize());
    SVA_TRY(bo.get(out, sizeof(float) * out_elems));
    if (single_out) {
        SVA_TRY(bo1.put(single_out, sizeof(float) * out_elems));
        for (int r = 0; r < n_runs; ++r) {
            const int slot = runs[4 * r], pos0 = runs[4 * r + 1], M = runs[4 * r + 2], row0 = runs[4 * r + 3];
            const float* qr = bq.as<float>() + (size_t)row0 * 3 * D;
            float* orow = bo1.as<float>() + (size_t)row0 * D;
            if (half_kv) SVA_TRY(launch_ar_prefill_attention<__half>(qr, M, H, 64, slot, pos0, bc.as<__half>(), (long)slot_elems, S, orow, 0));
            else SVA_TRY(launch_ar_prefill_attention<float>(qr, M, H, 64, slot, pos0, bc.as<float>(), (long)slot_elems, S, orow, 0));
        }
        SVA_HIP(hipDeviceSynchronize());
        SVA_TRY(bo1.get(single_out, sizeof(float) * out_elems));
    }
    return 0;
}
extern "C" int sva_test_prefill_pack(const int* M, int n, int Mmax, int* out, int out_cap) {
    SVA_CHECK(M && out && n >= 1 && Mmax >= 1, "sva_test_prefill_pack: bad arguments");
    std::vector<int> pass_of, row0_of;
    const int n_pass = prefill_pack(M, n, Mmax, pass_of, row0_of);
    SVA_CHECK(n_pass >= 1, "sva_test_prefill_pack: a slot's rows do not fit one pass (M outside 1 .. Mmax)");
    std::vector<int> o;
    for (int i = 0; i < n; ++i) { o.push_back(pass_of[i]); o.push_back(row0_of[i]); }
    for (int i0 = 0; i0 < n;) {
        std::vector<int> runs, tiles;
        int i1 = i0;
        for (; i1 < n && pass_of[i1] == pass_of[i0]; ++i1) runs.insert(runs.end(), {i1, 0, M[i1], row0_of[i1]});
        const int nt = prefill_tile_table(runs.data(), (int)runs.size() / 4, tiles);
        o.push_back(nt);
        o.insert(o.end(), tiles.begin(), tiles.end());
        i0 = i1;
    }
    SVA_CHECK((int)o.size() <= out_cap, "sva_test_prefill_pack: out is too short");
    memcpy(out, o.data(), sizeof(int) * o.size());
    return n_pass;
}
extern "C" int sva_test_pair_attention(int device, int M, int H, int pos0, int S, const float* q, const float* keys, const float* vals,
                                       int half_kv, float* out_ref, float* out_mfma, int iters, float* us) {
    SVA_CHECK(M % 2 == 0, "sva_test_pair_attention: an even number of rows");
    return test_attention_vs_per_row(device, true, M, H, pos0, S, q, keys, vals, half_kv, out_ref, out_mfma, iters, us);
}


// microbenchmark of the conv-GEMM dispatcher on device-resident random data:
//   out_us[0] = average microseconds per launch over `iters` back-to-back launches (hipEvents)
// mode bits: 1 = GELU epilogue, 2 = residual + gamma, 4 = silu-on-load, 8 = w13
extern "C" int sva_bench_gemm(int device, int B, int T, int N, int Cin, int taps, int dil, int mode, int iters, float* out_us) {
    SVA_HIP(hipSetDevice(device));
    const int H = (taps - 1) * dil;
    const long rows = H + T;
    float *dA, *dW, *dB, *dC, *dR;
    const long K = (long)taps * Cin;
    const int Nout = (mode & 8) ? N / 2 : N;
    SVA_HIP(hipMalloc(&dA, sizeof(float) * (size_t)B * rows * Cin));
    SVA_HIP(hipMalloc(&dW, sizeof(float) * (size_t)N * K));
    SVA_HIP(hipMalloc(&dB, sizeof(float) * N));
    SVA_HIP(hipMalloc(&dC, sizeof(float) * (size_t)B * T * Nout));
    SVA_HIP(hipMalloc(&dR, sizeof(float) * (size_t)B * T * Nout));
    std::vector<float> h((size_t)std::max<long>((long)B * rows * Cin, (long)N * K));
    unsigned s = 12345;
    for (auto& v : h) { s = s * 1664525u + 1013904223u; v = ((s >> 8) & 0xFFFF) / 32768.0f - 1.0f; }
    SVA_HIP(hipMemcpy(dA, h.data(), sizeof(float) * (size_t)B * rows * Cin, hipMemcpyHostToDevice));
    SVA_HIP(hipMemcpy(dW, h.data(), sizeof(float) * (size_t)N * K, hipMemcpyHostToDevice));
    SVA_HIP(hipMemset(dB, 0, sizeof(float) * N));
    SVA_HIP(hipMemset(dR, 0, sizeof(float) * (size_t)B * T * Nout));
    ConvGemm g;
    g.A = dA; g.a_bstride = rows * Cin; g.a_off = 0; g.lda = Cin; g.T = T; g.M = B * T; g.Cin = Cin; g.taps = taps; g.dil = dil;
    g.W = dW; g.N = N; g.bias = (mode & 8) ? nullptr : dB; g.C = dC; g.c_bstride = (long)T * Nout; g.ldc = Nout;
    if (mode & 1) g.act = ACT_GELU;
    if (mode & 2) { g.res = dR; g.r_bstride = (long)T * Nout; g.ldr = Nout; g.gamma = dB; }
    if (mode & 4) g.a_silu = 1;
    if (mode & 8) g.w13 = 1;
    hipStream_t st;
    SVA_HIP(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    SVA_HIP(hipEventCreate(&e0));
    SVA_HIP(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) { int rc = launch_conv_gemm(g, st); if (rc) return rc; }
    SVA_HIP(hipStreamSynchronize(st));
    SVA_HIP(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) { int rc = launch_conv_gemm(g, st); if (rc) return rc; }
    SVA_HIP(hipEventRecord(e1, st));
    SVA_HIP(hipStreamSynchronize(st));
    float ms = 0;
    SVA_HIP(hipEventElapsedTime(&ms, e0, e1));
    out_us[0] = ms * 1e3f / iters;
    (void)hipFree(dA); (void)hipFree(dW); (void)hipFree(dB); (void)hipFree(dC); (void)hipFree(dR);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(st);
    return 0;
}

// W [N][K] -> the fragment-major packing gemm_stream.hip reads (ConvGemm::Wk): [N / 16][K / 16][lane = (n & 15) + 16 * (k4)][4], zero rows past N
static void pack_fragment_major(const float* W, int N, long K, std::vector<float>& out) {
    const long nkb = K / 16, nt16 = (N + 15) / 16;
    out.assign((size_t)nt16 * nkb * 256, 0.f);
    for (long t = 0; t < nt16; ++t)
        for (long kb = 0; kb < nkb; ++kb)
            for (int l = 0; l < 64; ++l) {
                const long n = t * 16 + (l & 15);
                if (n >= N) continue;
                for (int e = 0; e < 4; ++e) out[((t * nkb + kb) * 64 + l) * 4 + e] = W[(size_t)n * K + kb * 16 + 4 * (l >> 4) + e];
            }
}

// One dispatch choice of the conv-GEMM family timed on device-resident random data, `nrot` weight copies rotated launch by launch (large nrot:
// every launch streams its weights from HBM, as inside a step that touches 0.8 GB of weights; 1: the weights stay in L2 / MALL).
//   kind -1 = the dispatcher; 0 / 1 / 2 / 4 = GemmFamily SmallM (c = column tiles + 16 * grid-level K split) / Tiled / Ring / Split with its parameters
//   (sva_common.h); 6 = the weight-streaming kernel launched directly (gemm_stream.hip: a = mt + 16 * nt, b = kw, c = wmode + 16 * probe)
//   mode bits: 1 GELU, 2 residual + gamma, 4 SiLU on load, 8 SwiGLU (w13), 16 fused RMSNorm of the rows
//   out[0] = microseconds per launch, eager back-to-back; out[1] = the same launches replayed as one hipGraph; out[2] = max |C - C_dispatcher|;
//   out[3] = max |C_dispatcher|
// its kind numbers are the tuned table's (kind 6, the weight-streaming kernel with its weight mode and probes, is launched directly below)
static GemmPlan bench_choice_plan(int kind, int a, int b, int c) {
    GemmPlan p;
    if (kind == 7) return GemmPlan{GemmFamily::Stream, a, b, c & 15, 1};       // (row-major weights, through the plan check)
    if (kind == 6 || !plan_from_table_kind(kind, a, b, c & 15, kind == 0 && (c >> 4) > 1 ? c >> 4 : 1, &p)) p.a = -1;      // (no plan takes a = -1: refused)
    return p;
}
extern "C" int sva_bench_gemm_choice(int device, int B, int T, int N, int Cin, int taps, int dil, int mode, int kind, int a, int b, int c, int nrot,
                                     int iters, float* out) {
    SVA_HIP(hipSetDevice(device));
    SVA_CHECK(nrot >= 1 && iters >= 1 && out, "bench_gemm_choice: arguments");
    const int H = (taps - 1) * dil;
    const long rows = H + T;
    const long K = (long)taps * Cin;
    const int Nout = (mode & 8) ? N / 2 : N;
    const bool packed = kind == 6 && ((c & 15) & 2);
    float *dA, *dB, *dC, *dC2, *dR, *dG;
    std::vector<float*> dW(nrot, nullptr), dWp(nrot, nullptr);
    SVA_HIP(hipMalloc(&dA, sizeof(float) * (size_t)B * rows * Cin));
    SVA_HIP(hipMalloc(&dB, sizeof(float) * N));
    SVA_HIP(hipMalloc(&dG, sizeof(float) * Cin));
    SVA_HIP(hipMalloc(&dC, sizeof(float) * (size_t)B * T * Nout));
    SVA_HIP(hipMalloc(&dC2, sizeof(float) * (size_t)B * T * Nout));
    SVA_HIP(hipMalloc(&dR, sizeof(float) * (size_t)B * T * Nout));
    std::vector<float> hA((size_t)B * rows * Cin), hW((size_t)N * K), hB(N), hG(Cin), hR((size_t)B * T * Nout);
    unsigned s = 12345;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xFFFF) / 32768.0f - 1.0f; };
    for (auto& v : hA) v = rnd();
    for (auto& v : hW) v = rnd() * 0.05f;
    for (auto& v : hB) v = rnd() * 0.1f;
    for (auto& v : hG) v = 1.f + 0.1f * rnd();
    for (auto& v : hR) v = rnd();
    SVA_HIP(hipMemcpy(dA, hA.data(), sizeof(float) * hA.size(), hipMemcpyHostToDevice));
    SVA_HIP(hipMemcpy(dB, hB.data(), sizeof(float) * N, hipMemcpyHostToDevice));
    SVA_HIP(hipMemcpy(dG, hG.data(), sizeof(float) * Cin, hipMemcpyHostToDevice));
    SVA_HIP(hipMemcpy(dR, hR.data(), sizeof(float) * hR.size(), hipMemcpyHostToDevice));
    std::vector<float> hWp;
    if (packed) pack_fragment_major(hW.data(), N, K, hWp);
    for (int r = 0; r < nrot; ++r) {
        SVA_HIP(hipMalloc(&dW[r], sizeof(float) * hW.size()));
        SVA_HIP(hipMemcpy(dW[r], hW.data(), sizeof(float) * hW.size(), hipMemcpyHostToDevice));
        if (packed) {
            SVA_HIP(hipMalloc(&dWp[r], sizeof(float) * hWp.size()));
            SVA_HIP(hipMemcpy(dWp[r], hWp.data(), sizeof(float) * hWp.size(), hipMemcpyHostToDevice));
        }
    }
    ConvGemm g;
    g.A = dA; g.a_bstride = rows * Cin; g.a_off = 0; g.lda = Cin; g.T = T; g.M = B * T; g.Cin = Cin; g.taps = taps; g.dil = dil;
    g.W = dW[0]; g.N = N; g.bias = (mode & 8) ? nullptr : dB; g.C = dC; g.c_bstride = (long)T * Nout; g.ldc = Nout;
    if (mode & 1) g.act = ACT_GELU;
    if (mode & 2) { g.res = dR; g.r_bstride = (long)T * Nout; g.ldr = Nout; g.gamma = dB; }
    if (mode & 4) g.a_silu = 1;
    if (mode & 8) g.w13 = 1;
    if (mode & 16) g.rms_w = dG;
    hipStream_t st;
    SVA_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    SVA_TRY(conv_gemm_prepare_stream(st));
    auto run = [&](int r) -> int {
        ConvGemm q = g;
        q.W = dW[r];
        if (kind < 0) return launch_conv_gemm(q, st);
        if (kind == 6) return launch_stream_gemm(q, packed ? dWp[r] : dW[r], a & 15, a >> 4, b, c & 15, c >> 4, st);
        return launch_conv_gemm_plan(q, bench_choice_plan(kind, a, b, c), st);
    };
    // reference result: the dispatcher's own choice
    {
        ConvGemm q = g;
        q.C = dC2;
        SVA_TRY(launch_conv_gemm(q, st));
    }
    for (int i = 0; i < 3; ++i) SVA_TRY(run(i % nrot));
    SVA_HIP(hipStreamSynchronize(st));
    {
        std::vector<float> c1((size_t)B * T * Nout), c2(c1.size());
        SVA_HIP(hipMemcpy(c1.data(), dC, sizeof(float) * c1.size(), hipMemcpyDeviceToHost));
        SVA_HIP(hipMemcpy(c2.data(), dC2, sizeof(float) * c2.size(), hipMemcpyDeviceToHost));
        float md = 0.f, mx = 0.f;
        for (size_t i = 0; i < c1.size(); ++i) { md = std::max(md, std::fabs(c1[i] - c2[i])); mx = std::max(mx, std::fabs(c2[i])); }
        out[2] = md; out[3] = mx;
    }
    hipEvent_t e0, e1;
    SVA_HIP(hipEventCreate(&e0));
    SVA_HIP(hipEventCreate(&e1));
    float best = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {
        SVA_HIP(hipEventRecord(e0, st));
        for (int i = 0; i < iters; ++i) SVA_TRY(run(i % nrot));
        SVA_HIP(hipEventRecord(e1, st));
        SVA_HIP(hipStreamSynchronize(st));
        float ms = 0;
        SVA_HIP(hipEventElapsedTime(&ms, e0, e1));
        best = std::min(best, ms);
    }
    out[0] = best * 1e3f / iters;
    // the same chain as one graph
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    SVA_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    int rc = 0;
    for (int i = 0; i < iters && !rc; ++i) rc = run(i % nrot);
    SVA_HIP(hipStreamEndCapture(st, &graph));
    if (rc) return rc;
    SVA_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    SVA_HIP(hipGraphLaunch(exec, st));
    SVA_HIP(hipStreamSynchronize(st));
    best = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {
        SVA_HIP(hipEventRecord(e0, st));
        SVA_HIP(hipGraphLaunch(exec, st));
        SVA_HIP(hipEventRecord(e1, st));
        SVA_HIP(hipStreamSynchronize(st));
        float ms = 0;
        SVA_HIP(hipEventElapsedTime(&ms, e0, e1));
        best = std::min(best, ms);
    }
    out[1] = best * 1e3f / iters;
    (void)hipGraphExecDestroy(exec); (void)hipGraphDestroy(graph);
    for (int r = 0; r < nrot; ++r) { (void)hipFree(dW[r]); if (dWp[r]) (void)hipFree(dWp[r]); }
    (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dG); (void)hipFree(dC); (void)hipFree(dC2); (void)hipFree(dR);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(st);
    return 0;
}

// A5 sampler through one explicit implementation (see launch_sampler_variant); noise = the Exp(1) draws [rows, V].
// us_out (optional) = average microseconds per launch over `iters` back-to-back launches.
extern "C" int sva_test_sampler(int device, int variant, int rows, int V, const float* logits, const float* noise, float temperature,
                                float top_p, int* tok_out, int iters, float* us_out) {
    SVA_HIP(hipSetDevice(device));
    float *dL, *dN;
    int* dT;
    const size_t n = (size_t)rows * V;
    SVA_HIP(hipMalloc(&dL, sizeof(float) * n));
    SVA_HIP(hipMalloc(&dN, sizeof(float) * n));
    SVA_HIP(hipMalloc(&dT, sizeof(int) * rows));
    SVA_HIP(hipMemcpy(dL, logits, sizeof(float) * n, hipMemcpyHostToDevice));
    SVA_HIP(hipMemcpy(dN, noise, sizeof(float) * n, hipMemcpyHostToDevice));
    int rc = launch_sampler_variant(variant, dL, rows, V, V, dN, V, nullptr, nullptr, temperature, top_p, dT, 0);
    if (!rc) {
        SVA_HIP(hipDeviceSynchronize());
        SVA_HIP(hipMemcpy(tok_out, dT, sizeof(int) * rows, hipMemcpyDeviceToHost));
        if (us_out && iters > 0) {
            hipEvent_t e0, e1;
            SVA_HIP(hipEventCreate(&e0));
            SVA_HIP(hipEventCreate(&e1));
            SVA_HIP(hipEventRecord(e0, 0));
            for (int i = 0; i < iters && !rc; ++i) rc = launch_sampler_variant(variant, dL, rows, V, V, dN, V, nullptr, nullptr, temperature, top_p, dT, 0);
            SVA_HIP(hipEventRecord(e1, 0));
            SVA_HIP(hipEventSynchronize(e1));
            float ms = 0.f;
            SVA_HIP(hipEventElapsedTime(&ms, e0, e1));
            us_out[0] = ms * 1000.f / iters;
            (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        }
    }
    (void)hipFree(dL); (void)hipFree(dN); (void)hipFree(dT);
    return rc;
}

// Host cost of enqueueing one kernel from the calling thread (microseconds), measured with `iters` launches of a one-element
// kernel into an otherwise idle stream.  A single-stream step is ~430 launches, so the launch rate of the enqueueing thread
// bounds the step rate, and on a two-socket host it depends on which core the thread runs on (measured 3.7 vs 4.8 us);
// engine.py pin_enqueue_thread() uses this to place the thread.
extern "C" int sva_host_launch_cost(int device, int iters, float* us_per_launch) {
    SVA_CHECK(iters > 0 && us_per_launch, "host_launch_cost: iters > 0 and an output pointer");
    SVA_HIP(hipSetDevice(device));
    static std::mutex mu;
    static std::map<int, std::pair<hipStream_t, int*>> res;
    std::lock_guard<std::mutex> lk(mu);
    auto& r = res[device];
    if (!r.first) {
        SVA_HIP(hipStreamCreateWithFlags(&r.first, hipStreamNonBlocking));
        SVA_HIP(hipMalloc((void**)&r.second, 64 * sizeof(int)));
    }
    for (int i = 0; i < 32; ++i) if (int rc = launch_fill_i32(r.second, 1, i, r.first)) return rc;
    SVA_HIP(hipStreamSynchronize(r.first));
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < iters; ++i) if (int rc = launch_fill_i32(r.second, 1, i, r.first)) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    SVA_HIP(hipStreamSynchronize(r.first));
    *us_per_launch = (float)(std::chrono::duration<double, std::micro>(t1 - t0).count() / iters);
    return 0;
}

// The planes GEMM (gemm_planes.hip) on one problem: weights split on the device as the engine does at finalize.  mode = PlanesMode,
// variant = tile variant; flags: 1 = the A operand as planes (to_planes pass first), 2 = the result leaves as planes only (summed back
// to fp32 here), 4 = GELU epilogue, 8 = SiLU on load (fp32 A only).  iters > 0 also times it (out_us[0] = microseconds per launch).
extern "C" int sva_test_gemm_planes(int device, int M, int N, int K, const float* A, const float* W, const float* bias, float* C, int mode,
                                    int variant, int flags, int iters, float* out_us) {
    SVA_HIP(hipSetDevice(device));
    SVA_CHECK((mode == PLANES_H3 || mode == PLANES_H1) && K % 32 == 0 && N % 4 == 0, "test_gemm_planes: bad arguments");
    const int npl = planes_count(mode);
    float *dA, *dW, *dB = nullptr, *dC;
    unsigned short *dWp, *dAp = nullptr, *dCp = nullptr;
    SVA_HIP(hipMalloc(&dA, sizeof(float) * (size_t)M * K));
    SVA_HIP(hipMalloc(&dW, sizeof(float) * (size_t)N * K));
    SVA_HIP(hipMalloc(&dC, sizeof(float) * (size_t)M * N));
    SVA_HIP(hipMalloc(&dWp, 2 * (size_t)npl * N * K));
    SVA_HIP(hipMemcpy(dA, A, sizeof(float) * (size_t)M * K, hipMemcpyHostToDevice));
    SVA_HIP(hipMemcpy(dW, W, sizeof(float) * (size_t)N * K, hipMemcpyHostToDevice));
    if (bias) {
        SVA_HIP(hipMalloc(&dB, sizeof(float) * N));
        SVA_HIP(hipMemcpy(dB, bias, sizeof(float) * N, hipMemcpyHostToDevice));
    }
    float mx = 0.f;
    for (size_t i = 0; i < (size_t)N * K; ++i) mx = std::max(mx, fabsf(W[i]));
    ConvGemm g;
    g.A = dA; g.a_bstride = (long)M * K; g.lda = K; g.T = M; g.M = M; g.Cin = K; g.taps = 1;
    g.W = dW; g.N = N; g.bias = dB; g.C = dC; g.c_bstride = (long)M * N; g.ldc = N;
    g.Wp = dWp; g.wp_pstride = (long)N * K; g.pmode = mode;
    SVA_TRY(make_weight_planes(dW, N, K, mx, mode, dWp, &g.wp_inv, 0));
    if (flags & 1) {
        SVA_HIP(hipMalloc(&dAp, 2 * (size_t)npl * M * K));
        SVA_TRY(launch_to_planes(dA, M, K, K, dAp, (long)M * K, mode, 1.f, 0, 0));
        g.Ap = dAp; g.ap_pstride = (long)M * K; g.ap_rows = M; g.A = nullptr;
    }
    if (flags & 2) {
        SVA_HIP(hipMalloc(&dCp, 2 * (size_t)npl * M * N));
        g.Cp = dCp; g.cp_pstride = (long)M * N; g.cp_rows = M; g.C = nullptr;
    }
    if (flags & 4) g.act = ACT_GELU;
    if ((flags & 8) && !(flags & 1)) g.a_silu = 1;
    // flags 32: SwiGLU (W rows interleave w1 | w3 in groups of 16; C is [M][N / 2]); 64: gamma (= bias vector reversed) and a residual (= a
    // deterministic pattern) in front of the store; 128: rows t in [T / 3, T / 3 + 6) of every batch item of T = 170 rows are not stored
    // (M % 170 == 0), C is pre-filled with a marker there
    const int Nout = (flags & 32) ? N / 2 : N;
    float *dG = nullptr, *dR = nullptr;
    if (flags & 32) {
        g.w13 = 1; g.ldc = Nout; g.c_bstride = (long)M * Nout; g.cp_pstride = (long)M * Nout;
    }
    if (flags & 64) {
        std::vector<float> hg(N), hr((size_t)M * N);
        for (int i = 0; i < N; ++i) hg[i] = 0.5f + 0.001f * (float)((i * 37) % 101);
        for (size_t i = 0; i < hr.size(); ++i) hr[i] = 0.01f * (float)((i * 13) % 257) - 1.f;
        SVA_HIP(hipMalloc(&dG, sizeof(float) * N));
        SVA_HIP(hipMalloc(&dR, sizeof(float) * (size_t)M * N));
        SVA_HIP(hipMemcpy(dG, hg.data(), sizeof(float) * N, hipMemcpyHostToDevice));
        SVA_HIP(hipMemcpy(dR, hr.data(), sizeof(float) * hr.size(), hipMemcpyHostToDevice));
        g.gamma = dG; g.res = dR; g.r_bstride = (long)M * N; g.ldr = N;
    }
    if (flags & 128) {
        SVA_CHECK(M % 170 == 0 && !(flags & 2), "test_gemm_planes: the skip-rows case takes M = 170 b and an fp32 C");
        g.T = 170; g.a_bstride = (long)170 * K; g.c_bstride = (long)170 * Nout; g.r_bstride = (long)170 * N; g.skip_lo = 56; g.skip_hi = 62;
        std::vector<float> mark((size_t)M * Nout, -77.f);
        SVA_HIP(hipMemcpy(dC, mark.data(), sizeof(float) * mark.size(), hipMemcpyHostToDevice));
    }
    int* h_ovf = nullptr;
    if (flags & 16) {       // the range check of the fp16 formats: a non-finite output is an error of the call
        SVA_HIP(hipHostMalloc((void**)&h_ovf, sizeof(int), hipHostMallocMapped));
        *h_ovf = 0;
        SVA_HIP(hipHostGetDevicePointer((void**)&g.ovf, h_ovf, 0));
    }
    SVA_TRY(launch_conv_gemm_plan(g, test_choice_plan(6, variant, 0, 0), 0));
    SVA_HIP(hipDeviceSynchronize());
    if (h_ovf) {
        const int o = *reinterpret_cast<volatile int*>(h_ovf);
        (void)hipHostFree(h_ovf);
        g.ovf = nullptr;
        if (o) { set_error("planes GEMM: non-finite output (an operand outside the fp16 range)"); return -3; }
    }
    if (flags & 2) {
        std::vector<uint16_t> hp((size_t)npl * M * N);
        SVA_HIP(hipMemcpy(hp.data(), dCp, hp.size() * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < (size_t)M * Nout; ++i) {
            float s = 0.f;
            const size_t row = i / Nout, col = i % Nout;
            const size_t bo = ((col >> 5) * (size_t)M + row) * 32 + (col & 31);          // K-blocked (planes_split.h)
            for (int p = npl - 1; p >= 0; --p) {
                const uint16_t bits = hp[(size_t)p * M * Nout + bo];
                _Float16 h; memcpy(&h, &bits, 2); s += (float)h;
            }
            C[i] = s;
        }
    } else {
        SVA_HIP(hipMemcpy(C, dC, sizeof(float) * (size_t)M * Nout, hipMemcpyDeviceToHost));
    }
    if (iters > 0 && out_us) {
        hipEvent_t e0, e1;
        SVA_HIP(hipEventCreate(&e0));
        SVA_HIP(hipEventCreate(&e1));
        SVA_HIP(hipEventRecord(e0, 0));
        for (int i = 0; i < iters; ++i) SVA_TRY(launch_conv_gemm_plan(g, test_choice_plan(6, variant, 0, 0), 0));
        SVA_HIP(hipEventRecord(e1, 0));
        SVA_HIP(hipDeviceSynchronize());
        float ms = 0;
        SVA_HIP(hipEventElapsedTime(&ms, e0, e1));
        out_us[0] = ms * 1e3f / iters;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    (void)hipFree(dA); (void)hipFree(dW); (void)hipFree(dC); (void)hipFree(dWp);
    if (dB) (void)hipFree(dB);
    if (dAp) (void)hipFree(dAp);
    if (dCp) (void)hipFree(dCp);
    if (dG) (void)hipFree(dG);
    if (dR) (void)hipFree(dR);
    return 0;
}

// The fp16-operand weight-streaming conv-GEMM (gemm_stream_h.hip) through its production launcher: the caller's tile configuration (mt = 0:
// the heuristic's), weights packed as sva_engine_finalize packs them.  Host arrays, all dense: A [B][(T - 1) stride + (taps - 1) dil + 1][Cin],
// W [N][taps * Cin], bias [N] or null, gamma [N] and res [B][T][N] (mode bit 2), C [B][T][N or N / 2] -- uploaded first, so what the caller
// pre-filled survives where the kernel stores nothing.  mode bits: 1 = GELU, 2 = gamma + residual, 4 = rows t in [T / 4, T / 2) of every item are
// computed but not stored (skip_lo / skip_hi), 8 = SwiGLU over 16-row interleaved (gate, up) weights, 16 = on the device the items sit at padded
// strides behind non-zero offsets (the padding is checked to come back untouched), 32 = range check (a non-finite output fails the call).
// Every index the launch will touch is checked against the device arrays' lengths before the launch.  iters > 0 also times it.
extern "C" int sva_test_gemm_h16(int device, int B, int T, int N, int Cin, int taps, int dil, int stride, const float* A, const float* W,
                                 const float* bias, const float* gamma, const float* res, int mode, int mt, int nt, int kw, float* C, int iters,
                                 float* out_us) {
    SVA_HIP(hipSetDevice(device));
    SVA_CHECK(B >= 1 && T >= 1 && N >= 1 && Cin >= 32 && Cin % 32 == 0 && taps >= 1 && dil >= 1 && stride >= 1 && A && W && C, "test_gemm_h16: bad arguments");
    SVA_CHECK(!(mode & 2) || (gamma && res), "test_gemm_h16: mode bit 2 needs gamma and res");
    SVA_CHECK(!(mode & 8) || (N % 32 == 0 && !(mode & 3) && !bias), "test_gemm_h16: SwiGLU takes N % 32 == 0 and no other epilogue");
    const long K = (long)taps * Cin, rows_in = (long)(T - 1) * stride + (long)(taps - 1) * dil + 1;
    const int Nout = (mode & 8) ? N / 2 : N;
    const bool pad = (mode & 16) != 0;
    const long a_bs = rows_in * Cin + (pad ? 8 : 0), a_off = pad ? 4 : 0;
    const long c_bs = (long)T * Nout + (pad ? 5 : 0), c_off = pad ? 3 : 0;
    const long r_bs = (long)T * N + (pad ? 7 : 0), r_off = pad ? 1 : 0;
    const size_t lenA = (size_t)B * a_bs + a_off, lenC = (size_t)B * c_bs + c_off, lenR = (size_t)B * r_bs + r_off;
    const float marker = -12345.f;
    std::vector<float> hA(lenA, 0.f), hC(lenC, marker), hR;
    for (int b = 0; b < B; ++b) {
        memcpy(&hA[(size_t)b * a_bs + a_off], A + (size_t)b * rows_in * Cin, sizeof(float) * rows_in * Cin);
        memcpy(&hC[(size_t)b * c_bs + c_off], C + (size_t)b * T * Nout, sizeof(float) * (size_t)T * Nout);
    }
    std::vector<uint16_t> hW;
    stream_h_pack_weights(W, N, (int)K, hW);
    DevBuf dA, dW, dB, dG, dR, dC;
    SVA_TRY(dA.put(hA.data(), sizeof(float) * lenA));
    SVA_TRY(dW.put(hW.data(), 2 * hW.size()));
    SVA_TRY(dC.put(hC.data(), sizeof(float) * lenC));
    if (bias) SVA_TRY(dB.put(bias, sizeof(float) * N));
    ConvGemm g;
    g.A = dA.as<float>(); g.a_bstride = a_bs; g.a_off = a_off; g.lda = Cin; g.T = T; g.M = B * T; g.stride = stride; g.dil = dil; g.taps = taps; g.Cin = Cin;
    g.Wkh = dW.p; g.N = N; g.bias = bias ? dB.as<float>() : nullptr;
    g.C = dC.as<float>(); g.c_bstride = c_bs; g.c_off = c_off; g.ldc = Nout;
    if (mode & 1) g.act = ACT_GELU;
    if (mode & 2) {
        hR.assign(lenR, 0.f);
        for (int b = 0; b < B; ++b) memcpy(&hR[(size_t)b * r_bs + r_off], res + (size_t)b * T * N, sizeof(float) * (size_t)T * N);
        SVA_TRY(dG.put(gamma, sizeof(float) * N));
        SVA_TRY(dR.put(hR.data(), sizeof(float) * lenR));
        g.gamma = dG.as<float>(); g.res = dR.as<float>(); g.r_bstride = r_bs; g.r_off = r_off; g.ldr = N;
    }
    if (mode & 4) { g.skip_lo = T / 4; g.skip_hi = T / 2; }
    if (mode & 8) g.w13 = 1;
    // the largest index of every array the launch touches
    SVA_CHECK((size_t)((long)(B - 1) * g.a_bstride + g.a_off + ((long)(T - 1) * stride + (long)(taps - 1) * dil) * g.lda + Cin - 1) < lenA, "test_gemm_h16: A index out of range");
    SVA_CHECK((size_t)((long)(B - 1) * g.c_bstride + g.c_off + (long)(T - 1) * g.ldc + Nout - 1) < lenC, "test_gemm_h16: C index out of range");
    SVA_CHECK(!g.res || (size_t)((long)(B - 1) * g.r_bstride + g.r_off + (long)(T - 1) * g.ldr + N - 1) < lenR, "test_gemm_h16: res index out of range");
    SVA_CHECK((size_t)((N + 15) / 16) * (K / 32) * 512 == hW.size(), "test_gemm_h16: weight packing size");
    SVA_CHECK(stream_h_gemm_supported(g), "test_gemm_h16: unsupported problem");
    if (mt == 0) stream_h_config(g, &mt, &nt, &kw);
    SVA_CHECK((mt == 1 || mt == 2 || mt == 4) && (nt == 1 || nt == 2) && (kw == 4 || kw == 8 || (kw == 16 && mt * nt <= 2)) && !(g.w13 && nt != 2),
              "test_gemm_h16: bad tile configuration");
    int* h_ovf = nullptr;
    if (mode & 32) {
        SVA_HIP(hipHostMalloc((void**)&h_ovf, sizeof(int), hipHostMallocMapped));
        *h_ovf = 0;
        SVA_HIP(hipHostGetDevicePointer((void**)&g.ovf, h_ovf, 0));
    }
    int rc = launch_stream_h_gemm(g, mt, nt, kw, 0);
    if (!rc && hipGetLastError() != hipSuccess) { set_error("test_gemm_h16: launch failed"); rc = -2; }
    const hipError_t se = hipDeviceSynchronize();
    if (h_ovf) {
        const int o = *reinterpret_cast<volatile int*>(h_ovf);
        (void)hipHostFree(h_ovf);
        g.ovf = nullptr;
        if (!rc && se == hipSuccess && o) {
            set_error("fp16-operand GEMM: non-finite output (an operand outside the fp16 range); sva_config.enc_dtype = 0 keeps the encoder on the fp32-grade kernels");
            return -3;
        }
    }
    if (rc) return rc;
    SVA_HIP(se);
    SVA_TRY(dC.get(hC.data(), sizeof(float) * lenC));
    for (int b = 0; b < B; ++b) memcpy(C + (size_t)b * T * Nout, &hC[(size_t)b * c_bs + c_off], sizeof(float) * (size_t)T * Nout);
    if (pad) {
        bool clean = true;
        for (long i = 0; i < c_off; ++i) clean = clean && hC[i] == marker;
        for (int b = 0; b < B; ++b)
            for (long i = (long)T * Nout; i < c_bs; ++i) clean = clean && hC[(size_t)b * c_bs + c_off + i] == marker;
        SVA_CHECK(clean, "test_gemm_h16: the kernel stored between the items");
    }
    if (iters > 0 && out_us) {
        hipEvent_t e0, e1;
        SVA_HIP(hipEventCreate(&e0));
        SVA_HIP(hipEventCreate(&e1));
        SVA_HIP(hipEventRecord(e0, 0));
        for (int i = 0; i < iters; ++i) SVA_TRY(launch_stream_h_gemm(g, mt, nt, kw, 0));
        SVA_HIP(hipEventRecord(e1, 0));
        SVA_HIP(hipDeviceSynchronize());
        float ms = 0;
        SVA_HIP(hipEventElapsedTime(&ms, e0, e1));
        out_us[0] = ms * 1e3f / iters;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Per-kernel hooks of the non-GEMM launchers (tests/test_gpu_kernels.py): each uploads the caller's arrays, calls the launcher the engine
// calls with the caller's arguments, synchronises and downloads.  Output arrays are uploaded first, so whatever the caller pre-filled them
// with (a sentinel) survives where the kernel writes nothing.  Every index the launch will touch is checked against the array lengths here.
// ------------------------------------------------------------------------------------------------------------------------------------
extern "C" int sva_test_decode_attention(int device, int variant, int M, int H, int S, int n_slots, const int* slot, const int* pos, int half_kv,
                                         float* qkv, float* cache, const float* rope, int n_pos, const float* x, const float* W, const float* norm_w,
                                         float* out) {
    SVA_HIP(hipSetDevice(device));
    SVA_CHECK(variant >= 0 && variant <= 6 && M >= 1 && H >= 1 && S >= 1 && n_slots >= 1, "sva_test_decode_attention: bad arguments");
    SVA_CHECK(!half_kv || variant == 0 || variant == 2 || variant == 5, "sva_test_decode_attention: fp16 cache only for the per-row, pair and rope_kvwrite kernels");
    const bool needs_rope = variant == 3 || variant == 5 || variant == 6;
    for (int m = 0; m < M; ++m) {
        SVA_CHECK(slot[m] >= 0 && slot[m] < n_slots && pos[m] >= 0 && pos[m] < S, "sva_test_decode_attention: slot / pos outside the cache");
        SVA_CHECK(!needs_rope || pos[m] < n_pos, "sva_test_decode_attention: pos outside the RoPE table");
    }
    if (variant == 2) {
        SVA_CHECK(M % 2 == 0, "sva_test_decode_attention: pairs need an even number of rows");
        for (int m = 0; m < M; m += 2)
            SVA_CHECK(slot[m + 1] == slot[m] && pos[m + 1] == pos[m] + 1, "sva_test_decode_attention: pair rows are positions (p, p + 1) of one slot");
    }
    SVA_CHECK(!needs_rope || rope, "sva_test_decode_attention: RoPE table missing");
    SVA_CHECK((variant != 1 && variant != 4 && variant != 6) || (W && M <= 2), "sva_test_decode_attention: GEMV variants need W and M <= 2");
    SVA_CHECK(variant != 6 || (x && norm_w), "sva_test_decode_attention: mode 2 needs x and norm_w");
    const int D = H * 64, splits = 8;
    const size_t slot_elems = (size_t)2 * H * S * 64, cache_elems = slot_elems * n_slots;
    DevBuf bq, bc, bs, bp, br, bx, bw, bn, bo, bpart;
    SVA_TRY(bq.put(qkv, sizeof(float) * (size_t)M * 3 * D));
    if (half_kv) {
        const std::vector<uint16_t> ch = to_half_bits(cache, cache_elems);
        SVA_TRY(bc.put(ch.data(), 2 * cache_elems));
    } else {
        SVA_TRY(bc.put(cache, sizeof(float) * cache_elems));
    }
    SVA_TRY(bs.put(slot, sizeof(int) * M));
    SVA_TRY(bp.put(pos, sizeof(int) * M));
    if (rope) SVA_TRY(br.put(rope, sizeof(float) * (size_t)n_pos * 64));
    if (x) SVA_TRY(bx.put(x, sizeof(float) * (size_t)M * D));
    if (W) SVA_TRY(bw.put(W, sizeof(float) * (size_t)(variant == 6 ? 3 * D : D) * D));
    if (norm_w) SVA_TRY(bn.put(norm_w, sizeof(float) * D));
    SVA_TRY(bo.put(out, sizeof(float) * (size_t)M * D));
    float *dq = bq.as<float>(), *dc = bc.as<float>(), *dout = bo.as<float>();
    __half* dch = bc.as<__half>();
    const int *ds = bs.as<int>(), *dp = bp.as<int>();
    const long ss = (long)slot_elems;
    Gemv g;
    g.M = M; g.W = bw.as<float>(); g.K = D; g.slot = ds; g.pos = dp; g.H = H;
    switch (variant) {
        case 0:
            SVA_TRY(half_kv ? launch_ar_attention<__half>(dq, M, H, 64, ds, dp, dch, ss, S, dout, 0) : launch_ar_attention<float>(dq, M, H, 64, ds, dp, dc, ss, S, dout, 0));
            break;
        case 1:         // slow AR at B <= 2: split-key attention, merged by the wo GEMV (+ residual)
            SVA_TRY(bpart.alloc(sizeof(float) * (size_t)M * H * splits * 68));
            SVA_TRY(launch_ar_attention<float>(dq, M, H, 64, ds, dp, dc, ss, S, nullptr, 0, bpart.as<float>(), splits));
            g.X = bpart.as<float>(); g.ldx = 0; g.mode = 4; g.S = splits; g.N = D; g.res = bx.as<float>(); g.ldr = D; g.Y = dout; g.ldy = D;
            SVA_TRY(launch_gemv(g, 0));
            break;
        case 2:
            SVA_TRY(half_kv ? launch_ar_attention_pairs<__half>(dq, M, H, 64, ds, dp, dch, ss, S, dout, 0) : launch_ar_attention_pairs<float>(dq, M, H, 64, ds, dp, dc, ss, S, dout, 0));
            break;
        case 3:
            SVA_TRY(launch_ar_fast_attention(dq, M, H, ds, dp, br.as<float>(), dc, ss, S, dout, 0));
            break;
        case 4:         // fast AR at B <= 2: attention over <= 8 cached keys inside the wo GEMV (+ residual)
            g.X = dq; g.ldx = 3 * D; g.mode = 3; g.kv = dc; g.kv_slot_stride = ss; g.S = S; g.N = D; g.res = bx.as<float>(); g.ldr = D; g.Y = dout; g.ldy = D;
            SVA_TRY(launch_gemv(g, 0));
            break;
        case 5:
            SVA_TRY(half_kv ? launch_rope_kvwrite<__half>(dq, M, H, 64, ds, dp, br.as<float>(), dch, ss, S, 0) : launch_rope_kvwrite<float>(dq, M, H, 64, ds, dp, br.as<float>(), dc, ss, S, 0));
            break;
        default:        // 6: QKV GEMV with the RMSNorm prologue and the RoPE + KV-write epilogue
            g.X = bx.as<float>(); g.ldx = D; g.N = 3 * D; g.norm_w = bn.as<float>(); g.eps = 1e-5f; g.Y = dq; g.ldy = 3 * D; g.mode = 2; g.rope = br.as<float>();
            g.kv = dc; g.kv_slot_stride = ss; g.S = S;
            SVA_TRY(launch_gemv(g, 0));
            break;
    }
    SVA_HIP(hipDeviceSynchronize());
    SVA_TRY(bq.get(qkv, sizeof(float) * (size_t)M * 3 * D));
    SVA_TRY(bo.get(out, sizeof(float) * (size_t)M * D));
    if (half_kv) {
        std::vector<uint16_t> ch(cache_elems);
        SVA_TRY(bc.get(ch.data(), 2 * cache_elems));
        for (size_t i = 0; i < cache_elems; ++i) { _Float16 hv; memcpy(&hv, &ch[i], 2); cache[i] = (float)hv; }
    } else {
        SVA_TRY(bc.get(cache, sizeof(float) * cache_elems));
    }
    return 0;
}

// planes: uint16 [n_planes][rows * K] in the tensor's own index space (blocked == 0) or K-blocked over `rows` rows (planes_split.h)
extern "C" int sva_test_enc_attention(int device, int B, int T, int H, int row0, const float* qkv, const float* rope, int n_planes, int blocked,
                                      float* out, unsigned short* planes) {
    SVA_HIP(hipSetDevice(device));
    SVA_CHECK(B >= 1 && T >= 1 && H >= 1 && row0 >= 0 && row0 < T && n_planes >= 0 && n_planes <= 2, "sva_test_enc_attention: bad arguments");
    const int D = H * 64;
    const size_t n = (size_t)B * T * D;
    DevBuf bq, br, bo, bpl;
    SVA_TRY(bq.put(qkv, sizeof(float) * n * 3));
    SVA_TRY(br.put(rope, sizeof(float) * (size_t)T * 64));
    SVA_TRY(bo.put(out, sizeof(float) * n));
    if (n_planes) SVA_TRY(bpl.put(planes, 2 * n * 2));
    SVA_TRY(launch_enc_attention(bq.as<float>(), br.as<float>(), B, T, H, 64, bo.as<float>(), row0, 0, n_planes ? bpl.as<unsigned short>() : nullptr, (long)n,
                                 n_planes, blocked ? (long)B * T : 0));
    SVA_HIP(hipDeviceSynchronize());
    SVA_TRY(bo.get(out, sizeof(float) * n));
    if (n_planes) SVA_TRY(bpl.get(planes, 2 * n * 2));
    return 0;
}

// kind 0: launch_dwconv7_ln (p0 = wT [7][C], p1 = bias, p2 = ln_w, p3 = ln_b; ldx = ldo = C), 1: launch_layernorm_rows (p0 = w, p1 = b),
// 2: launch_rmsnorm_rows (p0 = w).  x [x_len], out [o_len] and planes uint16 [2][p_len] are whole arrays with the strides / offsets applied inside.
extern "C" int sva_test_rowop(int device, int kind, int B, int T, int C, const float* x, long x_len, long x_bstride, long x_off, int ldx, const float* p0,
                              const float* p1, const float* p2, const float* p3, float eps, float* out, long o_len, long o_bstride, long o_off, int ldo,
                              int skip_lo, int skip_hi, int n_planes, int blocked, unsigned short* planes, long p_len) {
    SVA_HIP(hipSetDevice(device));
    SVA_CHECK(kind >= 0 && kind <= 2 && B >= 1 && T >= 1 && C >= 1 && n_planes >= 0 && n_planes <= 2, "sva_test_rowop: bad arguments");
    if (kind == 0) SVA_CHECK(ldx == C && ldo == C && o_off == 0, "sva_test_rowop: dwconv7_ln rows are dense");
    SVA_CHECK(kind != 1 || n_planes == 0, "sva_test_rowop: LayerNorm rows have no planes output");
    const int in_rows = kind == 0 ? T + 6 : T;
    SVA_CHECK(x_bstride >= 0 && x_off >= 0 && ldx >= C && (long)(B - 1) * x_bstride + x_off + (long)(in_rows - 1) * ldx + C <= x_len, "sva_test_rowop: input range outside x");
    SVA_CHECK(o_bstride >= 0 && o_off >= 0 && ldo >= C && (long)(B - 1) * o_bstride + o_off + (long)(T - 1) * ldo + C <= o_len, "sva_test_rowop: output range outside out");
    if (n_planes) {
        if (blocked) SVA_CHECK(C % 32 == 0 && ldo == C && o_off == 0 && o_bstride == (long)T * C && (long)B * T * C <= p_len, "sva_test_rowop: K-blocked planes cover B * T dense rows");
        else SVA_CHECK(o_len <= p_len, "sva_test_rowop: planes share the output's index space");
    }
    DevBuf bx, b0, b1, b2, b3, bo, bpl;
    SVA_TRY(bx.put(x, sizeof(float) * (size_t)x_len));
    SVA_TRY(b0.put(p0, sizeof(float) * (size_t)(kind == 0 ? 7 * C : C)));
    if (p1) SVA_TRY(b1.put(p1, sizeof(float) * C));
    if (p2) SVA_TRY(b2.put(p2, sizeof(float) * C));
    if (p3) SVA_TRY(b3.put(p3, sizeof(float) * C));
    SVA_CHECK(kind == 2 || p1, "sva_test_rowop: bias missing");
    SVA_CHECK(kind != 0 || (p2 && p3), "sva_test_rowop: LayerNorm parameters missing");
    SVA_TRY(bo.put(out, sizeof(float) * (size_t)o_len));
    if (n_planes) SVA_TRY(bpl.put(planes, 2 * (size_t)p_len * 2));
    unsigned short* dpl = n_planes ? bpl.as<unsigned short>() : nullptr;
    const long op_rows = blocked ? (long)B * T : 0;
    if (kind == 0)
        SVA_TRY(launch_dwconv7_ln(bx.as<float>(), x_bstride, x_off, B, T, C, b0.as<float>(), b1.as<float>(), b2.as<float>(), b3.as<float>(), eps, bo.as<float>(), o_bstride, 0,
                                  dpl, p_len, n_planes, op_rows));
    else if (kind == 1)
        SVA_TRY(launch_layernorm_rows(bx.as<float>(), x_bstride, x_off, ldx, B, T, C, b0.as<float>(), b1.as<float>(), eps, bo.as<float>(), o_bstride, o_off, ldo, 0, skip_lo, skip_hi));
    else
        SVA_TRY(launch_rmsnorm_rows(bx.as<float>(), x_bstride, x_off, ldx, B, T, C, b0.as<float>(), eps, bo.as<float>(), o_bstride, o_off, ldo, 0, dpl, p_len, n_planes, op_rows));
    SVA_HIP(hipDeviceSynchronize());
    SVA_TRY(bo.get(out, sizeof(float) * (size_t)o_len));
    if (n_planes) SVA_TRY(bpl.get(planes, 2 * (size_t)p_len * 2));
    return 0;
}

// launch_bsq: z [z_len] (rows b * z_bstride + z_off + t * ldz), zn_out (null or [z_len], same layout), idx_out int64 [idx_len] at b * idx_bstride + idx_off + t,
// u_out (null or [idx_len][nbits])
extern "C" int sva_test_bsq(int device, int B, int T, int C, const float* z, long z_len, long z_bstride, long z_off, int ldz, const float* norm_w, float eps,
                            float* zn_out, const float* W, const float* bias, int nbits, long long* idx_out, long idx_len, int idx_bstride, int idx_off, float* u_out) {
    SVA_HIP(hipSetDevice(device));
    SVA_CHECK(B >= 1 && T >= 1 && C >= 1 && nbits >= 1 && nbits <= 62, "sva_test_bsq: bad arguments");
    SVA_CHECK(z_bstride >= 0 && z_off >= 0 && ldz >= C && (long)(B - 1) * z_bstride + z_off + (long)(T - 1) * ldz + C <= z_len, "sva_test_bsq: input range outside z");
    SVA_CHECK(idx_bstride >= 0 && idx_off >= 0 && (long)(B - 1) * idx_bstride + idx_off + T <= idx_len, "sva_test_bsq: index range outside idx_out");
    DevBuf bz, bn, bzn, bw, bb, bi, bu;
    SVA_TRY(bz.put(z, sizeof(float) * (size_t)z_len));
    if (norm_w) SVA_TRY(bn.put(norm_w, sizeof(float) * C));
    if (zn_out) SVA_TRY(bzn.put(zn_out, sizeof(float) * (size_t)z_len));
    SVA_TRY(bw.put(W, sizeof(float) * (size_t)nbits * C));
    SVA_TRY(bb.put(bias, sizeof(float) * nbits));
    SVA_TRY(bi.put(idx_out, sizeof(long long) * (size_t)idx_len));
    if (u_out) SVA_TRY(bu.put(u_out, sizeof(float) * (size_t)idx_len * nbits));
    SVA_TRY(launch_bsq(bz.as<float>(), z_bstride, z_off, ldz, B, T, C, norm_w ? bn.as<float>() : nullptr, eps, zn_out ? bzn.as<float>() : nullptr, bw.as<float>(), bb.as<float>(),
                       nbits, bi.as<long long>(), idx_bstride, idx_off, u_out ? bu.as<float>() : nullptr, 0));
    SVA_HIP(hipDeviceSynchronize());
    if (zn_out) SVA_TRY(bzn.get(zn_out, sizeof(float) * (size_t)z_len));
    SVA_TRY(bi.get(idx_out, sizeof(long long) * (size_t)idx_len));
    if (u_out) SVA_TRY(bu.get(u_out, sizeof(float) * (size_t)idx_len * nbits));
    return 0;
}

// ring [B][N]; step == null -> the launcher's nullptr; two != 0: launch_stft_mag_ring2.  mag [B][mag_rows][ldm] (batch stride mag_rows * ldm).
// The twiddle and window tables are the engine's (packer.hip).
extern "C" int sva_test_stft_ring(int device, int B, int N, const float* ring, const int* step, int n_chunk, int add, int m0, int nfr, int two, int m0b, int nfrb,
                                  int row_b0, float* mag, int mag_rows, int ldm) {
    SVA_HIP(hipSetDevice(device));
    SVA_CHECK(B >= 1 && N >= 512 && nfr >= 1 && nfr <= mag_rows && n_chunk >= 0, "sva_test_stft_ring: bad arguments");
    SVA_CHECK(!step || (long)*step + add >= 0, "sva_test_stft_ring: negative ring origin");
    SVA_CHECK(!two || (nfrb >= 1 && row_b0 >= nfr && row_b0 + nfrb <= mag_rows), "sva_test_stft_ring: second range outside mag");
    std::vector<float> hann(2048), tw(2048);
    for (int i = 0; i < 2048; ++i) hann[i] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * i / 2048.0));
    for (int k = 0; k < 1024; ++k) {
        tw[2 * k] = (float)cos(2.0 * M_PI * k / 2048.0);
        tw[2 * k + 1] = (float)(-sin(2.0 * M_PI * k / 2048.0));
    }
    const size_t mag_n = (size_t)B * mag_rows * ldm;
    DevBuf br, bs, bh, bt, bm;
    SVA_TRY(br.put(ring, sizeof(float) * (size_t)B * N));
    if (step) SVA_TRY(bs.put(step, sizeof(int)));
    SVA_TRY(bh.put(hann.data(), sizeof(float) * 2048));
    SVA_TRY(bt.put(tw.data(), sizeof(float) * 2048));
    SVA_TRY(bm.put(mag, sizeof(float) * mag_n));
    const int* dstep = step ? bs.as<int>() : nullptr;
    if (two)
        SVA_TRY(launch_stft_mag_ring2(br.as<float>(), dstep, n_chunk, add, B, N, bt.as<float2>(), bh.as<float>(), bm.as<float>(), ldm, (long)mag_rows * ldm, m0, nfr, m0b, nfrb,
                                      row_b0, 0));
    else
        SVA_TRY(launch_stft_mag_ring(br.as<float>(), dstep, n_chunk, add, B, N, bt.as<float2>(), bh.as<float>(), bm.as<float>(), ldm, (long)mag_rows * ldm, m0, nfr, 0));
    SVA_HIP(hipDeviceSynchronize());
    SVA_TRY(bm.get(mag, sizeof(float) * mag_n));
    return 0;
}

// encode != 0: launch_fsq_encode (lat = x in, Wt = Win [G][4][gdim], bs = bin [G][4], codes out); else launch_fsq_decode (codes in, Wt = Wout [G][gdim][4],
// bs = bout [G][gdim], lat = out).  lat element (b, t, c) at b * l_bstride + l_off + t * ld + c; codes element (b, g, t) at b * c_bstride + g * c_gstride + t.
extern "C" int sva_test_fsq(int device, int encode, int B, int T, int G, int gdim, float* lat, long l_len, long l_bstride, long l_off, int ld, const float* Wt,
                            const float* bs, int* codes, long c_len, long c_bstride, long c_gstride) {
    SVA_HIP(hipSetDevice(device));
    SVA_CHECK(B >= 1 && T >= 1 && G >= 1 && gdim >= 1, "sva_test_fsq: bad arguments");
    SVA_CHECK(l_bstride >= 0 && l_off >= 0 && ld >= G * gdim && (long)(B - 1) * l_bstride + l_off + (long)(T - 1) * ld + (long)G * gdim <= l_len, "sva_test_fsq: latent range outside lat");
    SVA_CHECK(c_bstride >= 0 && c_gstride >= 0 && (long)(B - 1) * c_bstride + (long)(G - 1) * c_gstride + T <= c_len, "sva_test_fsq: code range outside codes");
    DevBuf bl, bw, bb, bc;
    SVA_TRY(bl.put(lat, sizeof(float) * (size_t)l_len));
    SVA_TRY(bw.put(Wt, sizeof(float) * (size_t)G * gdim * 4));
    SVA_TRY(bb.put(bs, sizeof(float) * (size_t)(encode ? G * 4 : G * gdim)));
    SVA_TRY(bc.put(codes, sizeof(int) * (size_t)c_len));
    if (encode) SVA_TRY(launch_fsq_encode(bl.as<float>(), l_bstride, l_off, ld, B, T, G, gdim, bw.as<float>(), bb.as<float>(), bc.as<int>(), c_bstride, c_gstride, 0));
    else SVA_TRY(launch_fsq_decode(bc.as<int>(), c_bstride, c_gstride, B, T, G, gdim, bw.as<float>(), bb.as<float>(), bl.as<float>(), l_bstride, l_off, ld, 0));
    SVA_HIP(hipDeviceSynchronize());
    SVA_TRY(bl.get(lat, sizeof(float) * (size_t)l_len));
    SVA_TRY(bc.get(codes, sizeof(int) * (size_t)c_len));
    return 0;
}

// launch_conv_post_tanh: x element (b, r, c) at b * x_bstride + x_off + r * C + c (rows 0 .. T + k - 2), pcm (b, t) at b * p_bstride + p_off + t
extern "C" int sva_test_conv_post(int device, int B, int T, int C, int k, const float* x, long x_len, long x_bstride, long x_off, const float* w, const float* bias,
                                  float* pcm, long p_len, long p_bstride, long p_off, const int* slot_flag) {
    SVA_HIP(hipSetDevice(device));
    SVA_CHECK(B >= 1 && T >= 1 && C >= 1 && k >= 1, "sva_test_conv_post: bad arguments");
    SVA_CHECK(x_bstride >= 0 && x_off >= 0 && (long)(B - 1) * x_bstride + x_off + (long)(T + k - 1) * C <= x_len, "sva_test_conv_post: input range outside x");
    SVA_CHECK(p_bstride >= 0 && p_off >= 0 && (long)(B - 1) * p_bstride + p_off + T <= p_len, "sva_test_conv_post: output range outside pcm");
    DevBuf bx, bw, bb, bp, bf;
    SVA_TRY(bx.put(x, sizeof(float) * (size_t)x_len));
    SVA_TRY(bw.put(w, sizeof(float) * (size_t)k * C));
    SVA_TRY(bb.put(bias, sizeof(float)));
    SVA_TRY(bp.put(pcm, sizeof(float) * (size_t)p_len));
    if (slot_flag) SVA_TRY(bf.put(slot_flag, sizeof(int) * B));
    SVA_TRY(launch_conv_post_tanh(bx.as<float>(), x_bstride, x_off, B, T, C, k, bw.as<float>(), bb.as<float>(), bp.as<float>(), p_bstride, p_off, 0,
                                  slot_flag ? bf.as<int>() : nullptr));
    SVA_HIP(hipDeviceSynchronize());
    SVA_TRY(bp.get(pcm, sizeof(float) * (size_t)p_len));
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The tail of the AR decode (tests/test_gpu_decode_tail.py): the production samplers, the device helpers of the persistent kernels
// (ar_device.h), launch_gemv in its plain and SwiGLU modes, the token and history kernels.  Same convention as above; arguments arrive
// as desc (integers), fpar (floats) and ptrs (host arrays, NULL = absent) in the order include/sva.h lists.  Return codes: 0 ran,
// 1 REFUSED by the launcher's own check (nothing was launched; sva_last_error has its message), -2 a HIP error, -4 arguments the hook
// itself declines (an index outside an array).
// ------------------------------------------------------------------------------------------------------------------------------------
#define SVA_HOOK_CHECK(cond, msg)                                             \
    do {                                                                      \
        if (!(cond)) {                                                        \
            set_error(std::string(msg) + " [" #cond "]");                    \
            return -4;                                                        \
        }                                                                     \
    } while (0)

// a launcher's SVA_CHECK (-1) is a refusal, anything else non-zero an error
#define SVA_LAUNCH_OR_REFUSED(expr) \
    do {                            \
        const int _rc = (expr);     \
        if (_rc == -1) return 1;    \
        if (_rc) return _rc;        \
    } while (0)

namespace {
struct EditArgs { int on, W, prev_cap, prev_len, n_sup, sup_len; };
// the logit edits in front of a sampler, on the same device rows (stages.hip): every index checked, params = {W, n_suppress, penalty bits}
int run_logit_edits(float* d_rows, int rows, int V, int ldl, const EditArgs& e, float penalty, const int* prev, const int* suppress, DevBuf& bprev, DevBuf& bsup,
                    DevBuf& bpar, int* refused) {
    SVA_HOOK_CHECK(e.prev_cap >= 0 && e.prev_len >= 0 && e.n_sup >= 0 && e.sup_len >= e.n_sup, "logit edits hook: list lengths");
    SVA_HOOK_CHECK((long)std::min(std::max(e.W, 0), e.prev_cap) <= (long)e.prev_len, "logit edits hook: prev shorter than min(W, prev_cap)");
    SVA_HOOK_CHECK((e.prev_len == 0 || prev) && (e.sup_len == 0 || suppress), "logit edits hook: list missing");
    int pbits;
    memcpy(&pbits, &penalty, 4);
    const int params[4] = {e.W, e.n_sup, pbits, 0};
    SVA_TRY(bprev.put(prev, sizeof(int) * (size_t)e.prev_len));
    SVA_TRY(bsup.put(suppress, sizeof(int) * (size_t)e.sup_len));
    SVA_TRY(bpar.put(params, sizeof(params)));
    const int rc = launch_logit_edits(d_rows, rows, V, ldl, bprev.as<int>(), e.prev_cap, bsup.as<int>(), bpar.as<int>(), 0);
    if (rc == -1) { *refused = 1; return 0; }
    return rc;
}
// the production sampler launchers on host operands; samp != null: n_pairs {inv_temp, top_p} pairs, row r reads pair row_slot[r] (null: r)
int sampler_launch_impl(int device, const long long* d, const float* fpar, void* const* ptrs, const float* samp, int n_pairs, const int* row_slot) {
    SVA_HIP(hipSetDevice(device));
    const int small = (int)d[0], rows = (int)d[1], V = (int)d[2], ldl = (int)d[3], ldn = (int)d[6], kind = (int)d[9], noise_elem_off = (int)d[10];
    const int tok_stride = (int)d[11], forced_stride = (int)d[14], use_forced = (int)d[17], emb_rows = (int)d[18], D = (int)d[19], ldo = (int)d[20];
    const long col_off = d[4], l_len = d[5], noise_off = d[7], n_len = d[8], tok_off = d[12], t_len = d[13], forced_off = d[15], f_len = d[16], e_len = d[21];
    const EditArgs ed = {(int)d[22], (int)d[23], (int)d[24], (int)d[25], (int)d[26], (int)d[27]};
    float* logits = (float*)ptrs[0];
    const float* noise = (const float*)ptrs[1];
    const unsigned long long* seed = (const unsigned long long*)ptrs[2];
    const int* frame = (const int*)ptrs[3];
    int *tok_raw = (int*)ptrs[4], *tok = (int*)ptrs[5];
    const int* forced = (const int*)ptrs[6];
    const float* emb_table = (const float*)ptrs[7];
    float* emb_out = (float*)ptrs[8];
    SVA_HOOK_CHECK(rows >= 1 && V >= 1 && ldl >= V && col_off >= 0 && logits && col_off + (long)(rows - 1) * ldl + V <= l_len, "sampler hook: logits range");
    SVA_HOOK_CHECK(!noise || (ldn >= 0 && noise_off >= 0 && noise_off + (long)(rows - 1) * ldn + V <= n_len), "sampler hook: noise range");
    SVA_HOOK_CHECK(noise || (seed && frame && noise_elem_off >= 0), "sampler hook: seed / frame missing");
    SVA_HOOK_CHECK(tok_raw && tok_stride >= 1 && tok_off >= 0 && tok_off + (long)(rows - 1) * tok_stride < t_len, "sampler hook: token range");
    SVA_HOOK_CHECK(small || (!tok && !forced && !emb_table && !emb_out), "sampler hook: only the V <= 1024 entry point fuses forcing and the gather");
    if (forced) {
        SVA_HOOK_CHECK(tok && use_forced >= 0 && forced_stride >= 0 && forced_off >= 0 && forced_off + (long)(rows - 1) * forced_stride < f_len, "sampler hook: forced range");
        for (long i = 0; i < f_len; ++i) SVA_HOOK_CHECK(!emb_table || (forced[i] >= 0 && forced[i] < emb_rows), "sampler hook: forced code outside the table");
    }
    if (emb_table) SVA_HOOK_CHECK(tok && emb_out && emb_rows >= V && D >= 1 && ldo >= D && (long)(rows - 1) * ldo + D <= e_len, "sampler hook: embedding range");
    SVA_HOOK_CHECK(samp || !row_slot, "sampler hook: row_slot without pairs");
    if (samp) {
        SVA_HOOK_CHECK(n_pairs >= 1 && (row_slot || n_pairs >= rows), "sampler hook: fewer pairs than rows");
        for (int r = 0; row_slot && r < rows; ++r) SVA_HOOK_CHECK(row_slot[r] >= 0 && row_slot[r] < n_pairs, "sampler hook: row_slot outside the pairs");
    }
    DevBuf bl, bn, bs, bf, btr, bt, bfo, buf, bet, beo, bprev, bsup, bpar, bsamp, brs;
    if (samp) SVA_TRY(bsamp.put(samp, sizeof(float) * 2 * (size_t)n_pairs));
    if (row_slot) SVA_TRY(brs.put(row_slot, sizeof(int) * (size_t)rows));
    const float* dsamp = samp ? bsamp.as<float>() : nullptr;
    const int* drs = row_slot ? brs.as<int>() : nullptr;
    SVA_TRY(btr.put(tok_raw, sizeof(int) * (size_t)t_len));
    if (tok) SVA_TRY(bt.put(tok, sizeof(int) * (size_t)t_len));
    if (emb_out) SVA_TRY(beo.put(emb_out, sizeof(float) * (size_t)e_len));          // (uploaded and handed over without a table too: nothing may be written then)
    SVA_TRY(bl.put(logits, sizeof(float) * (size_t)l_len));
    if (noise) SVA_TRY(bn.put(noise, sizeof(float) * (size_t)n_len));
    if (seed) SVA_TRY(bs.put(seed, sizeof(unsigned long long) * rows));
    if (frame) SVA_TRY(bf.put(frame, sizeof(int) * rows));
    if (forced) SVA_TRY(bfo.put(forced, sizeof(int) * (size_t)f_len));
    if (use_forced >= 0) SVA_TRY(buf.put(&use_forced, sizeof(int)));
    if (emb_table) SVA_TRY(bet.put(emb_table, sizeof(float) * (size_t)emb_rows * D));
    float* dl = bl.as<float>() + col_off;
    int refused = 0;
    if (ed.on) SVA_TRY(run_logit_edits(dl, rows, V, ldl, ed, fpar[2], (const int*)ptrs[9], (const int*)ptrs[10], bprev, bsup, bpar, &refused));
    if (refused) return 1;
    const float* dn = noise ? bn.as<float>() + noise_off : nullptr;
    int rc;
    if (small)
        rc = launch_sampler_small(dl, rows, V, ldl, dn, ldn, seed ? bs.as<unsigned long long>() : nullptr, frame ? bf.as<int>() : nullptr, kind, noise_elem_off, fpar[0], fpar[1],
                                  btr.as<int>() + tok_off, tok ? bt.as<int>() + tok_off : nullptr, tok_stride, forced ? bfo.as<int>() + forced_off : nullptr, forced_stride,
                                  use_forced >= 0 ? buf.as<int>() : nullptr, emb_table ? bet.as<float>() : nullptr, D, emb_out ? beo.as<float>() : nullptr, ldo, 0, dsamp, drs);
    else
        rc = launch_sampler(dl, rows, V, ldl, dn, ldn, seed ? bs.as<unsigned long long>() : nullptr, frame ? bf.as<int>() : nullptr, kind, noise_elem_off, fpar[0], fpar[1],
                            btr.as<int>() + tok_off, tok_stride, 0, dsamp, drs);
    SVA_LAUNCH_OR_REFUSED(rc);
    SVA_HIP(hipDeviceSynchronize());
    SVA_TRY(bl.get(logits, sizeof(float) * (size_t)l_len));
    SVA_TRY(btr.get(tok_raw, sizeof(int) * (size_t)t_len));
    if (tok) SVA_TRY(bt.get(tok, sizeof(int) * (size_t)t_len));
    if (emb_out) SVA_TRY(beo.get(emb_out, sizeof(float) * (size_t)e_len));
    return 0;
}
}  // namespace

extern "C" int sva_test_sampler_launch(int device, const long long* d, const float* fpar, void* const* ptrs) {
    return sampler_launch_impl(device, d, fpar, ptrs, nullptr, 0, nullptr);
}
// the operands of sva_test_sampler_launch + per-row sampling pairs: samp [n_pairs][2] = {inv_temp, top_p} (null: the scalars of fpar),
// row_slot [rows] or null
extern "C" int sva_test_sampler_rows(int device, const long long* d, const float* fpar, void* const* ptrs, const float* samp, int n_pairs,
                                     const int* row_slot) {
    return sampler_launch_impl(device, d, fpar, ptrs, samp, n_pairs, row_slot);
}

// ---- ar_device.h: nucleus_sample and gemv exactly as ar_decode.hip / ar_batch.hip instantiate them ----
namespace {
// One workgroup per row (NW == 1: one WAVE per row, red = nullptr, as the fast head of ar_batch.hip).  PER == 16 (ar_batch.hip) loads through a clamped
// index and selects, the others (ar_decode.hip) under the predicate.  tok[row] = thread 0's (lane 0's) return value, same[row] = 1 when every
// participating thread returned it.
template <int NW, int PER, int NTH>
__global__ __launch_bounds__(NTH) void test_nucleus_kernel(const float* __restrict__ logits, int rows, int V, int ldl, const float* __restrict__ noise, int ldn,
                                                           const unsigned long long* __restrict__ seed, const int* __restrict__ frame, int kind, int noise_elem_off,
                                                           float inv_temp, float top_p, int* __restrict__ tok, int* __restrict__ same) {
    __shared__ double red[64];
    __shared__ int first_tok, mismatch;
    const int tid = threadIdx.x, lane = tid & 63;
    const int row = NW == 1 ? (int)blockIdx.x * (NTH / 64) + (tid >> 6) : (int)blockIdx.x;
    const int e0 = NW == 1 ? lane : tid;
    if (NW == 1 && row >= rows) return;             // (wave-uniform; the one-wave form has no barrier)
    const float* lg = logits + (long)row * ldl;
    float l[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int e = e0 + NW * 64 * r;
        if constexpr (PER == 16) {
            const float v = lg[e < V ? e : V - 1];
            l[r] = e < V ? v : -INFINITY;
        } else {
            l[r] = e < V ? lg[e] : -INFINITY;
        }
    }
    const float* nz = noise ? noise + (long)row * ldn : nullptr;
    const unsigned long long sd = seed ? seed[row] : 0ull;
    const int fr = frame ? frame[row] : 0;
    const int t = ardev::nucleus_sample<NW, PER>(l, V, e0, nz, sd, fr, kind, noise_elem_off, inv_temp, top_p, NW == 1 ? nullptr : red);
    if constexpr (NW == 1) {
        const int t0 = __builtin_amdgcn_readfirstlane(t);
        const bool ok = __all(t == t0);
        if (lane == 0) { tok[row] = t0; same[row] = ok ? 1 : 0; }
    } else {
        if (tid == 0) { first_tok = t; mismatch = 0; }
        __syncthreads();
        if (t != first_tok) atomicOr(&mismatch, 1);
        __syncthreads();
        if (tid == 0) { tok[row] = t; same[row] = mismatch ? 0 : 1; }
    }
}

// One wave per group of ROWS consecutive weight rows (row0 + group * ROWS ...): out[m][group * ROWS + r] from lane 0, same[group] = 1 when all 64 lanes
// hold bit-identical values.
template <typename WT, int K, int ROWS, int M, bool NORM>
__global__ __launch_bounds__(64) void test_ardev_gemv_kernel(const void* __restrict__ W, long row0, const float* __restrict__ x, int ldx, const float* __restrict__ nw,
                                                             float eps, float* __restrict__ out, int ldo, int* __restrict__ same) {
    const int lane = threadIdx.x;
    ardev::WFrag<WT, K> w[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) w[r].load(W, row0 + (long)blockIdx.x * ROWS + r, lane);
    float o[M][ROWS];
    ardev::gemv<WT, K, ROWS, M, NORM>(w, x, ldx, nw, eps, lane, o);
    bool ok = true;
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int bits = __builtin_bit_cast(int, o[m][r]);
            ok = ok && bits == __builtin_amdgcn_readfirstlane(bits);
        }
    ok = __all(ok);
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int r = 0; r < ROWS; ++r) out[(long)m * ldo + (long)blockIdx.x * ROWS + r] = o[m][r];
        same[blockIdx.x] = ok ? 1 : 0;
    }
}

struct ArdevGemvInst { int K, ROWS, M, norm; };
// the ten instantiations of ar_decode.hip (M = 2 rows of a frame) and ar_batch.hip (M = 1)
constexpr ArdevGemvInst kArdevGemv[10] = {{768, 6, 2, 1},  {768, 2, 2, 0}, {768, 12, 2, 1}, {2304, 2, 2, 0}, {768, 11, 1, 1},
                                          {768, 6, 1, 1},  {768, 2, 1, 0}, {768, 12, 1, 1}, {2304, 2, 1, 0}, {768, 3, 1, 1}};
template <int I>
int launch_test_ardev_gemv(bool half, int groups, const void* W, long row0, const float* x, int ldx, const float* nw, float eps, float* out, int ldo, int* same) {
    constexpr ArdevGemvInst c = kArdevGemv[I];
    if (half) hipLaunchKernelGGL((test_ardev_gemv_kernel<__half, c.K, c.ROWS, c.M, c.norm != 0>), dim3(groups), dim3(64), 0, 0, W, row0, x, ldx, nw, eps, out, ldo, same);
    else hipLaunchKernelGGL((test_ardev_gemv_kernel<float, c.K, c.ROWS, c.M, c.norm != 0>), dim3(groups), dim3(64), 0, 0, W, row0, x, ldx, nw, eps, out, ldo, same);
    SVA_HIP(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" int sva_test_ar_device(int device, int op, const long long* d, const float* fpar, void* const* ptrs) {
    SVA_HIP(hipSetDevice(device));
    if (op == 0) {
        const int inst = (int)d[0], rows = (int)d[1], V = (int)d[2], ldl = (int)d[3], ldn = (int)d[5], kind = (int)d[7], noise_elem_off = (int)d[8];
        const long l_len = d[4], n_len = d[6];
        const float* logits = (const float*)ptrs[0];
        const float* noise = (const float*)ptrs[1];
        const unsigned long long* seed = (const unsigned long long*)ptrs[2];
        const int* frame = (const int*)ptrs[3];
        int *tok = (int*)ptrs[4], *same = (int*)ptrs[5];
        SVA_HOOK_CHECK(inst >= 0 && inst <= 3 && rows >= 1 && V >= 1 && V <= ((inst == 0 || inst == 3) ? 1024 : 8192), "ar_device sampler hook: instantiation / V");
        SVA_HOOK_CHECK(logits && tok && same && ldl >= V && (long)(rows - 1) * ldl + V <= l_len, "ar_device sampler hook: logits range");
        SVA_HOOK_CHECK(!noise || (ldn >= 0 && (long)(rows - 1) * ldn + V <= n_len), "ar_device sampler hook: noise range");
        SVA_HOOK_CHECK(noise || (seed && frame && noise_elem_off >= 0), "ar_device sampler hook: seed / frame missing");
        DevBuf bt, bsm, bl, bn, bs, bf;
        SVA_TRY(bt.put(tok, sizeof(int) * rows));
        SVA_TRY(bsm.put(same, sizeof(int) * rows));
        SVA_TRY(bl.put(logits, sizeof(float) * (size_t)l_len));
        if (noise) SVA_TRY(bn.put(noise, sizeof(float) * (size_t)n_len));
        if (seed) SVA_TRY(bs.put(seed, sizeof(unsigned long long) * rows));
        if (frame) SVA_TRY(bf.put(frame, sizeof(int) * rows));
        const float tclamp = fpar[0] > 1e-5f ? fpar[0] : 1e-5f;
#define SVA_NS_ARGS bl.as<float>(), rows, V, ldl, noise ? bn.as<float>() : nullptr, ldn, seed ? bs.as<unsigned long long>() : nullptr, frame ? bf.as<int>() : nullptr, \
                    kind, noise_elem_off, 1.0f / tclamp, fpar[1], bt.as<int>(), bsm.as<int>()
        if (inst == 0) hipLaunchKernelGGL((test_nucleus_kernel<4, 4, 256>), dim3(rows), dim3(256), 0, 0, SVA_NS_ARGS);
        else if (inst == 1) hipLaunchKernelGGL((test_nucleus_kernel<4, 32, 256>), dim3(rows), dim3(256), 0, 0, SVA_NS_ARGS);
        else if (inst == 2) hipLaunchKernelGGL((test_nucleus_kernel<8, 16, 512>), dim3(rows), dim3(512), 0, 0, SVA_NS_ARGS);
        else hipLaunchKernelGGL((test_nucleus_kernel<1, 16, 512>), dim3((rows + 7) / 8), dim3(512), 0, 0, SVA_NS_ARGS);
#undef SVA_NS_ARGS
        SVA_HIP(hipGetLastError());
        SVA_HIP(hipDeviceSynchronize());
        SVA_TRY(bt.get(tok, sizeof(int) * rows));
        SVA_TRY(bsm.get(same, sizeof(int) * rows));
        return 0;
    }
    SVA_HOOK_CHECK(op == 1, "ar_device hook: op 0 (nucleus_sample) or 1 (gemv)");
    const int inst = (int)d[0], half = (int)d[1], groups = (int)d[2], ldx = (int)d[4], ldo = (int)d[6];
    const long row0 = d[3], x_len = d[5], o_len = d[7];
    SVA_HOOK_CHECK(inst >= 0 && inst < 10 && groups >= 1 && row0 >= 0, "ar_device gemv hook: instantiation / groups");
    const ArdevGemvInst c = kArdevGemv[inst];
    const float *W = (const float*)ptrs[0], *x = (const float*)ptrs[1], *nw = (const float*)ptrs[2];
    float* out = (float*)ptrs[3];
    int* same = (int*)ptrs[4];
    const long n_rows = (long)groups * c.ROWS;
    SVA_HOOK_CHECK(W && x && out && same && (!c.norm || nw), "ar_device gemv hook: array missing");
    SVA_HOOK_CHECK(ldx >= c.K && ldx % 4 == 0 && (long)(c.M - 1) * ldx + c.K <= x_len, "ar_device gemv hook: x range (rows are read as float4)");
    SVA_HOOK_CHECK(ldo >= n_rows && (long)(c.M - 1) * ldo + n_rows <= o_len, "ar_device gemv hook: out range");
    // the weight array holds rows [0, row0 + n_rows); only the caller's rows [row0, ...) are uploaded, the ones in front are never read
    const size_t esz = half ? 2 : 4, w_elems = (size_t)(row0 + n_rows) * c.K;
    DevBuf bo, bsm, bw, bx, bnw;
    SVA_TRY(bo.put(out, sizeof(float) * (size_t)o_len));
    SVA_TRY(bsm.put(same, sizeof(int) * groups));
    SVA_TRY(bw.alloc(w_elems * esz));
    if (half) {
        const std::vector<uint16_t> hb = to_half_bits(W, (size_t)n_rows * c.K);
        SVA_HIP(hipMemcpy(bw.as<char>() + (size_t)row0 * c.K * esz, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
    } else {
        SVA_HIP(hipMemcpy(bw.as<char>() + (size_t)row0 * c.K * esz, W, (size_t)n_rows * c.K * 4, hipMemcpyHostToDevice));
    }
    SVA_TRY(bx.put(x, sizeof(float) * (size_t)x_len));
    if (c.norm) SVA_TRY(bnw.put(nw, sizeof(float) * c.K));
    const float* dnw = c.norm ? bnw.as<float>() : nullptr;
    int rc = 0;
    switch (inst) {
#define SVA_AG(I_) case I_: rc = launch_test_ardev_gemv<I_>(half != 0, groups, bw.p, row0, bx.as<float>(), ldx, dnw, fpar[0], bo.as<float>(), ldo, bsm.as<int>()); break;
        SVA_AG(0) SVA_AG(1) SVA_AG(2) SVA_AG(3) SVA_AG(4) SVA_AG(5) SVA_AG(6) SVA_AG(7) SVA_AG(8) SVA_AG(9)
#undef SVA_AG
    }
    if (rc) return rc;
    SVA_HIP(hipDeviceSynchronize());
    SVA_TRY(bo.get(out, sizeof(float) * (size_t)o_len));
    SVA_TRY(bsm.get(same, sizeof(int) * groups));
    return 0;
}

// launch_gemv, modes 0 (plain) and 1 (SwiGLU), a whole Gemv from host arrays; modes 3 / 4 only to reach the launcher's refusals (operands of the
// right size, all zero).  Only array lengths are checked here: what the launcher accepts is the launcher's business.
extern "C" int sva_test_gemv(int device, const long long* d, const float* fpar, void* const* ptrs) {
    SVA_HIP(hipSetDevice(device));
    const int M = (int)d[0], N = (int)d[1], K = (int)d[2], ldx = (int)d[3], ldy = (int)d[6], ldr = (int)d[9], mode = (int)d[11], alias = (int)d[12], S = (int)d[13], H = (int)d[14];
    const long x_len = d[4], w_rows = d[5], y_off = d[7], y_len = d[8], r_len = d[10];
    const float *X = (const float*)ptrs[0], *W = (const float*)ptrs[1], *norm_w = (const float*)ptrs[2], *bias = (const float*)ptrs[3], *res = (const float*)ptrs[4];
    float* Y = (float*)ptrs[5];
    SVA_HOOK_CHECK(mode == 0 || mode == 1 || mode == 3 || mode == 4, "gemv hook: modes 0, 1 (and 3, 4 for their refusals)");
    SVA_HOOK_CHECK(M >= 0 && M <= 64 && N >= 1 && K >= 1 && ldx >= 0 && ldy >= 0 && ldr >= 0 && y_off >= 0 && W && Y, "gemv hook: bad arguments");
    const int Mr = M < 1 ? 1 : M;                                   // (the kernel reads row 0 in place of rows >= M)
    const int n_units = mode == 1 ? N / 4 : N / 2, n_out = mode == 1 ? N / 2 : N;
    long w_top = 0;                                                 // one past the highest weight row a wave reads
    for (int u = 0; u < n_units; ++u)
        for (int q = 0; q < 2; ++q) {
            const int f = 2 * u + q;
            w_top = std::max<long>(w_top, mode == 1 ? (long)(f >> 4) * 32 + (f & 15) + 16 + 1 : (long)f + 1);
        }
    SVA_HOOK_CHECK(w_top <= w_rows, "gemv hook: weight rows outside W");
    SVA_HOOK_CHECK(y_off + (long)(Mr - 1) * ldy + n_out <= y_len, "gemv hook: output range outside Y");
    SVA_HOOK_CHECK(!alias || (!res && ldr == ldy), "gemv hook: the aliased residual is Y itself");
    SVA_HOOK_CHECK(!res || (long)(Mr - 1) * ldr + N <= r_len, "gemv hook: residual range outside res");
    DevBuf by, bx, bw, bn, bb, br, bsl, bkv;
    SVA_TRY(by.put(Y, sizeof(float) * (size_t)y_len));
    SVA_TRY(bw.put(W, sizeof(float) * (size_t)w_rows * K));
    if (norm_w) SVA_TRY(bn.put(norm_w, sizeof(float) * K));
    if (bias) SVA_TRY(bb.put(bias, sizeof(float) * N));
    if (res) SVA_TRY(br.put(res, sizeof(float) * (size_t)r_len));
    Gemv g;
    g.M = M; g.W = bw.as<float>(); g.N = N; g.K = K; g.norm_w = norm_w ? bn.as<float>() : nullptr; g.eps = fpar[0];
    g.bias = bias ? bb.as<float>() : nullptr; g.Y = by.as<float>() + y_off; g.ldy = ldy; g.mode = mode; g.ldx = ldx;
    if (alias) { g.res = g.Y; g.ldr = ldy; }
    else if (res) { g.res = br.as<float>(); g.ldr = ldr; }
    if (mode <= 1) {
        SVA_HOOK_CHECK(X && (long)(Mr - 1) * ldx + K <= x_len, "gemv hook: input range outside X");
        SVA_TRY(bx.put(X, sizeof(float) * (size_t)x_len));
        g.X = bx.as<float>();
    } else {
        SVA_HOOK_CHECK(H == 12 && K == 768 && S >= 1 && S <= 64, "gemv hook: the attention modes are sized for K = 12 x 64");
        std::vector<int> zi(Mr, 0);
        SVA_TRY(bsl.put(zi.data(), sizeof(int) * Mr));
        g.slot = bsl.as<int>(); g.pos = bsl.as<int>(); g.H = H; g.S = S;
        if (mode == 3) {                                            // X = qkv rows [M][3 K], kv = one slot [2][H][S][64]
            std::vector<float> z((size_t)std::max((long)Mr * 3 * K, (long)2 * H * S * 64), 0.f);
            SVA_TRY(bx.put(z.data(), sizeof(float) * (size_t)Mr * 3 * K));
            SVA_TRY(bkv.put(z.data(), sizeof(float) * (size_t)2 * H * S * 64));
            g.X = bx.as<float>(); g.ldx = 3 * K; g.kv = bkv.as<float>(); g.kv_slot_stride = (long)2 * H * S * 64;
        } else {                                                    // X = partials [M][H][S][68]
            std::vector<float> z((size_t)Mr * H * S * 68, 0.f);
            SVA_TRY(bx.put(z.data(), sizeof(float) * z.size()));
            g.X = bx.as<float>(); g.ldx = 0;
        }
    }
    SVA_LAUNCH_OR_REFUSED(launch_gemv(g, 0));
    SVA_HIP(hipDeviceSynchronize());
    SVA_TRY(by.get(Y, sizeof(float) * (size_t)y_len));
    return 0;
}

// kind 0 launch_logit_edits, 1 launch_gather_rows, 2 launch_audio_embed, 3 launch_shift_history (descriptors built on the device), 4 launch_ring_write
extern "C" int sva_test_token_ops(int device, int kind, const long long* d, const float* fpar, void* const* ptrs) {
    SVA_HIP(hipSetDevice(device));
    if (kind == 0) {
        const int rows = (int)d[0], V = (int)d[1], ldl = (int)d[2];
        const long l_len = d[3];
        const EditArgs ed = {1, (int)d[4], (int)d[5], (int)d[6], (int)d[7], (int)d[8]};
        float* logits = (float*)ptrs[0];
        SVA_HOOK_CHECK(rows >= 1 && V >= 1 && ldl >= V && logits && (long)(rows - 1) * ldl + V <= l_len, "logit edits hook: logits range");
        DevBuf bl, bprev, bsup, bpar;
        SVA_TRY(bl.put(logits, sizeof(float) * (size_t)l_len));
        int refused = 0;
        SVA_TRY(run_logit_edits(bl.as<float>(), rows, V, ldl, ed, fpar[0], (const int*)ptrs[1], (const int*)ptrs[2], bprev, bsup, bpar, &refused));
        if (refused) return 1;
        SVA_HIP(hipDeviceSynchronize());
        SVA_TRY(bl.get(logits, sizeof(float) * (size_t)l_len));
        return 0;
    }
    if (kind == 1 || kind == 2) {
        // d: rows, D, ldo, o_len, t_rows, idx_len, (1) idx_stride, idx_offset | (2) code_stride, cb_stride, ncb, codebook_size
        const int rows = (int)d[0], D = (int)d[1], ldo = (int)d[2], s0 = (int)d[6], s1 = (int)d[7], ncb = kind == 2 ? (int)d[8] : 1, cbs = kind == 2 ? (int)d[9] : 0;
        const long o_len = d[3], t_rows = d[4], i_len = d[5];
        const float* table = (const float*)ptrs[0];
        const int* idx = (const int*)ptrs[1];
        float* out = (float*)ptrs[2];
        SVA_HOOK_CHECK(rows >= 1 && D >= 1 && ldo >= D && table && idx && out && (long)(rows - 1) * ldo + D <= o_len && ncb >= 1 && s0 >= 0 && cbs >= 0, "token ops hook: bad arguments");
        for (int r = 0; r < rows; ++r)
            for (int i = 0; i < ncb; ++i) {
                const long at = kind == 1 ? (long)r * s0 : (long)r * s0 + (long)i * s1;
                SVA_HOOK_CHECK(at >= 0 && at < i_len, "token ops hook: index position outside idx");
                const long row = kind == 1 ? (long)idx[at] + s1 : (long)idx[at] + (long)i * cbs;
                SVA_HOOK_CHECK(row >= 0 && row < t_rows, "token ops hook: table row outside the table");
            }
        DevBuf bo, bt, bi;
        SVA_TRY(bo.put(out, sizeof(float) * (size_t)o_len));
        SVA_TRY(bt.put(table, sizeof(float) * (size_t)t_rows * D));
        SVA_TRY(bi.put(idx, sizeof(int) * (size_t)i_len));
        if (kind == 1) SVA_LAUNCH_OR_REFUSED(launch_gather_rows(bt.as<float>(), bi.as<int>(), s0, s1, rows, D, bo.as<float>(), ldo, 0));
        else SVA_LAUNCH_OR_REFUSED(launch_audio_embed(bt.as<float>(), bi.as<int>(), s0, s1, rows, ncb, cbs, D, bo.as<float>(), ldo, 0));
        SVA_HIP(hipDeviceSynchronize());
        SVA_TRY(bo.get(out, sizeof(float) * (size_t)o_len));
        return 0;
    }
    if (kind == 3) {
        // d: n_desc, B, col_slices, has_counter, counter_add, buf_len, then per descriptor: offset, bstride, H, T, C
        const int n_desc = (int)d[0], B = (int)d[1], zs = (int)d[2], has_counter = (int)d[3], counter_add = (int)d[4];
        const long b_len = d[5];
        float* buf = (float*)ptrs[0];
        int* counter = (int*)ptrs[1];
        SVA_HOOK_CHECK(n_desc >= 0 && n_desc <= 64 && B >= 1 && B <= 65535 && zs >= 1 && zs <= 64 && buf && (!has_counter || counter), "shift_history hook: bad arguments");
        DevBuf bb, bc, bd;
        SVA_TRY(bb.put(buf, sizeof(float) * (size_t)b_len));
        if (has_counter) SVA_TRY(bc.put(counter, sizeof(int)));
        std::vector<ShiftDesc> hd(n_desc);
        for (int i = 0; i < n_desc; ++i) {
            const long off = d[6 + 5 * i], bs = d[7 + 5 * i], Hh = d[8 + 5 * i], T = d[9 + 5 * i], Cc = d[10 + 5 * i];
            SVA_HOOK_CHECK(off >= 0 && bs >= 0 && Hh >= 0 && T >= 0 && Cc >= 1 && Hh < (1 << 20) && T < (1 << 20) && Cc < (1 << 20) &&
                           off + (long)(B - 1) * bs + (Hh + T) * Cc <= b_len, "shift_history hook: tensor outside the buffer");
            hd[i].ptr = bb.as<float>() + off; hd[i].bstride = bs; hd[i].H = (int)Hh; hd[i].T = (int)T; hd[i].C = (int)Cc; hd[i].pad = 0;
        }
        SVA_TRY(bd.put(hd.data(), sizeof(ShiftDesc) * (size_t)n_desc));
        SVA_LAUNCH_OR_REFUSED(launch_shift_history(bd.as<ShiftDesc>(), n_desc, B, 0, zs, has_counter ? bc.as<int>() : nullptr, counter_add));
        SVA_HIP(hipDeviceSynchronize());
        SVA_TRY(bb.get(buf, sizeof(float) * (size_t)b_len));
        if (has_counter) SVA_TRY(bc.get(counter, sizeof(int)));
        return 0;
    }
    SVA_HOOK_CHECK(kind == 4, "token ops hook: kind 0 .. 4");
    // d: B, N, n, has_step, step; ptrs: ring [B][N] (in / out), chunk [B][n], slot_flag [B] or NULL
    const int B = (int)d[0], N = (int)d[1], n = (int)d[2], has_step = (int)d[3], step = (int)d[4];
    float* ring = (float*)ptrs[0];
    const float* chunk = (const float*)ptrs[1];
    const int* flag = (const int*)ptrs[2];
    SVA_HOOK_CHECK(B >= 1 && N >= 1 && n >= 1 && n <= N && step >= 0 && ring && chunk, "ring_write hook: bad arguments (n <= N, step >= 0)");
    DevBuf br, bc, bs, bf;
    SVA_TRY(br.put(ring, sizeof(float) * (size_t)B * N));
    SVA_TRY(bc.put(chunk, sizeof(float) * (size_t)B * n));
    if (has_step) SVA_TRY(bs.put(&step, sizeof(int)));
    if (flag) SVA_TRY(bf.put(flag, sizeof(int) * B));
    SVA_LAUNCH_OR_REFUSED(launch_ring_write(br.as<float>(), has_step ? bs.as<int>() : nullptr, B, N, bc.as<float>(), n, 0, flag ? bf.as<int>() : nullptr));
    SVA_HIP(hipDeviceSynchronize());
    SVA_TRY(br.get(ring, sizeof(float) * (size_t)B * N));
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The bookkeeping kernels of the chunk step through their launchers (engine_kernels.h; include/sva.h: sva_test_step_ops; tests/test_gpu_step_ops.py).
// Whole host arrays in (outputs first carry the caller's sentinels), the launcher, every array the kernel may write back.  Everything a launch
// would index with -- codes, slots, counters' capacities, row counts -- is checked against the array lengths of the descriptor first: a failed
// check returns 1 (refused) or -4 (arguments the hook cannot lay out) and nothing is launched.
// ------------------------------------------------------------------------------------------------------------------------------------
#define SVA_HOOK_REFUSE(cond, msg)                                  \
    do {                                                            \
        if (!(cond)) {                                              \
            set_error(std::string(msg) + " [" #cond "]");          \
            return 1;                                               \
        }                                                           \
    } while (0)
namespace {
struct StepBufs {
    DevBuf b[13];
    void* const* ptrs;
    int up(int i, size_t bytes) {
        SVA_HOOK_CHECK(ptrs[i], "step ops hook: a required array is missing");
        return b[i].put(ptrs[i], bytes);
    }
    int down(int i, size_t bytes) { return b[i].get(ptrs[i], bytes); }
    template <typename T> T* at(int i) const { return b[i].as<T>(); }
};
bool all_in(const int* v, size_t n, long lo, long hi) {
    for (size_t i = 0; i < n; ++i)
        if (v[i] < lo || v[i] >= hi) return false;
    return true;
}
bool all_in64(const long long* v, size_t n, long lo, long hi) {
    for (size_t i = 0; i < n; ++i)
        if (v[i] < lo || v[i] >= hi) return false;
    return true;
}
bool is_pow2(long v) { return v >= 1 && (v & (v - 1)) == 0; }
const long kStepMax = 1L << 26;          // elements of any one array of the hook
}  // namespace

extern "C" int sva_test_step_ops(int device, int kind, const long long* d, const float* fpar, void* const* ptrs) {
    (void)fpar;
    SVA_CHECK(d && ptrs, "sva_test_step_ops: null argument");
    SVA_HIP(hipSetDevice(device));
    StepBufs s;
    s.ptrs = ptrs;
    const size_t F = sizeof(float), I = sizeof(int), L = sizeof(long long);
    if (kind == 0) {          // ar_prepare_step
        const long B = d[0], T2 = d[1], code_off = d[2], D = d[3], chunk = d[4], ci = d[5], n_rows = d[6];
        SVA_HOOK_CHECK(B >= 1 && B <= 4096 && T2 >= 1 && T2 <= 4096 && D >= 1 && D <= 8192 && chunk >= 1 && chunk <= 64 && n_rows >= 1 && n_rows * D <= kStepMax, "ar_prepare_step hook: sizes");
        SVA_HOOK_REFUSE(code_off >= 0 && code_off < T2 && ci >= 0 && ci < chunk, "ar_prepare_step hook: code_off / ci outside their arrays");
        SVA_HOOK_CHECK(ptrs[2], "ar_prepare_step hook: codes");
        SVA_HOOK_REFUSE(all_in64((const long long*)ptrs[2], (size_t)(B * T2), 0, n_rows), "ar_prepare_step hook: a code outside the content table");
        SVA_TRY(s.up(4, F * 2 * B * D)); SVA_TRY(s.up(5, I * 2 * B)); SVA_TRY(s.up(6, I * 2 * B)); SVA_TRY(s.up(7, I * B * chunk));
        SVA_TRY(s.up(0, F * B * D)); SVA_TRY(s.up(1, F * n_rows * D)); SVA_TRY(s.up(2, L * B * T2)); SVA_TRY(s.up(3, I * B));
        SVA_LAUNCH_OR_REFUSED(launch_ar_prepare_step(s.at<float>(0), s.at<float>(1), s.at<long long>(2), (int)T2, (int)code_off, s.at<int>(3), (int)D, s.at<float>(4),
                                                     s.at<int>(5), s.at<int>(6), s.at<int>(7), (int)chunk, (int)ci, (int)B, 0));
        SVA_HIP(hipDeviceSynchronize());
        SVA_TRY(s.down(4, F * 2 * B * D)); SVA_TRY(s.down(5, I * 2 * B)); SVA_TRY(s.down(6, I * 2 * B)); SVA_TRY(s.down(7, I * B * chunk));
        return 0;
    }
    if (kind == 1) {          // apply_forced
        const long B = d[0], ncb = d[1], cb = d[2], chunk = d[3], ci = d[4], use = d[5];
        SVA_HOOK_CHECK(B >= 1 && B <= 4096 && chunk >= 1 && chunk <= 64 && ncb >= 1, "apply_forced hook: sizes");
        SVA_HOOK_REFUSE(ncb <= 8 && cb >= 0 && cb < ncb && ci >= 0 && ci < chunk, "apply_forced hook: ncb <= 8, cb < ncb, ci < chunk");
        const int use_i = use ? 1 : 0;
        SVA_TRY(s.up(2, I * B * ncb)); SVA_TRY(s.up(0, I * B * ncb)); SVA_TRY(s.up(1, I * B * ncb * chunk)); SVA_TRY(s.b[3].put(&use_i, I));
        SVA_LAUNCH_OR_REFUSED(launch_apply_forced(s.at<int>(0), s.at<int>(1), s.at<int>(3), (int)chunk, (int)ci, (int)cb, (int)ncb, s.at<int>(2), (int)B, 0));
        SVA_HIP(hipDeviceSynchronize());
        return s.down(2, I * B * ncb);
    }
    if (kind == 2) {          // ar_finish_frame
        const long B = d[0], ncb = d[1], cap = d[2], chunk = d[3], ci = d[4], inc = d[5];
        SVA_HOOK_CHECK(B >= 1 && B <= 4096 && chunk >= 1 && chunk <= 64 && ncb >= 1 && cap >= 1 && cap <= 65536, "ar_finish_frame hook: sizes");
        SVA_HOOK_REFUSE(ncb <= 8 && is_pow2(cap) && ci >= 0 && ci < chunk, "ar_finish_frame hook: ncb <= 8, a power-of-two capacity, ci < chunk");
        SVA_TRY(s.up(1, I * B)); SVA_TRY(s.up(2, I * B)); SVA_TRY(s.up(3, I * B * ncb * cap)); SVA_TRY(s.up(4, I * B * ncb * chunk)); SVA_TRY(s.up(0, I * B * ncb));
        SVA_LAUNCH_OR_REFUSED(launch_ar_finish_frame(s.at<int>(0), (int)ncb, s.at<int>(1), s.at<int>(2), s.at<int>(3), (int)cap, s.at<int>(4), (int)chunk, (int)ci, (int)B,
                                                     (int)inc, 0));
        SVA_HIP(hipDeviceSynchronize());
        SVA_TRY(s.down(1, I * B)); SVA_TRY(s.down(2, I * B)); SVA_TRY(s.down(3, I * B * ncb * cap)); SVA_TRY(s.down(4, I * B * ncb * chunk));
        return 0;
    }
    if (kind == 3 || kind == 4) {          // append_content (d: B, T2, chunk, cap, counter given) / put_codes (d: B, T2, n_per, cap)
        const long B = d[0], T2 = d[1], n = d[2], cap = d[3], has_counter = kind == 3 ? d[4] : 0;
        SVA_HOOK_CHECK(B >= 1 && B <= 4096 && T2 >= 1 && T2 <= 4096 && n >= 1 && cap >= 1 && cap <= 65536, "content ring hook: sizes");
        SVA_HOOK_REFUSE(is_pow2(cap) && n <= T2 && n <= cap, "content ring hook: a power-of-two capacity, n <= T2, n <= capacity");
        if (kind == 3) {
            SVA_TRY(s.up(1, I * B * cap)); SVA_TRY(s.up(2, I * B)); SVA_TRY(s.up(3, I * B * n)); SVA_TRY(s.up(0, L * B * T2));
            if (has_counter) SVA_TRY(s.up(4, I));
            SVA_LAUNCH_OR_REFUSED(launch_append_content(s.at<long long>(0), (int)T2, (int)n, s.at<int>(1), (int)cap, s.at<int>(2), s.at<int>(3), (int)B,
                                                        has_counter ? s.at<int>(4) : nullptr, 0));
            SVA_HIP(hipDeviceSynchronize());
            SVA_TRY(s.down(1, I * B * cap)); SVA_TRY(s.down(2, I * B)); SVA_TRY(s.down(3, I * B * n));
            if (has_counter) SVA_TRY(s.down(4, I));
            return 0;
        }
        SVA_TRY(s.up(1, L * B * T2)); SVA_TRY(s.up(2, I * B * cap)); SVA_TRY(s.up(3, I * B)); SVA_TRY(s.up(0, L * B * n));
        SVA_LAUNCH_OR_REFUSED(launch_put_codes(s.at<long long>(0), (int)n, s.at<long long>(1), (int)T2, s.at<int>(2), (int)cap, s.at<int>(3), (int)B, 0));
        SVA_HIP(hipDeviceSynchronize());
        SVA_TRY(s.down(1, L * B * T2)); SVA_TRY(s.down(2, I * B * cap)); SVA_TRY(s.down(3, I * B));
        return 0;
    }
    if (kind == 5) {          // build_prompt
        const long nspk = d[0], R = d[1], dl = d[2], ncb = d[3], cbs = d[4], D = d[5], Pmax = d[6], n_rows = d[7], md = d[8], rows = d[9];
        SVA_HOOK_CHECK(nspk >= 0 && nspk <= 64 && R >= 1 && R <= 4096 && dl >= 1 && ncb >= 1 && cbs >= 1 && D >= 1 && D <= 8192 && Pmax >= 1 && Pmax <= 8192 && n_rows >= 1 &&
                       md >= 1 && md <= 64 && rows >= 1 && n_rows * D <= kStepMax && ncb * cbs * D <= kStepMax, "build_prompt hook: sizes");
        SVA_HOOK_REFUSE(ncb <= 8 && dl <= md && R <= Pmax && rows <= nspk + 2 * R, "build_prompt hook: ncb <= 8, d <= max_delay, R <= Pmax, rows <= nspk + 2 R");
        SVA_HOOK_CHECK(ptrs[4] && ptrs[5], "build_prompt hook: codes");
        SVA_HOOK_REFUSE(all_in((const int*)ptrs[4], (size_t)R, 0, n_rows), "build_prompt hook: a content code outside the table");
        for (long q = 0; q < ncb; ++q)
            SVA_HOOK_REFUSE(all_in((const int*)ptrs[5] + q * Pmax, (size_t)R, 0, cbs), "build_prompt hook: an audio code outside its codebook");
        SVA_TRY(s.up(6, F * rows * D));
        SVA_TRY(s.up(0, F * std::max(nspk, 1L) * D)); SVA_TRY(s.up(1, F * n_rows * D)); SVA_TRY(s.up(2, F * ncb * cbs * D)); SVA_TRY(s.up(3, F * md * D));
        SVA_TRY(s.up(4, I * R)); SVA_TRY(s.up(5, I * ncb * Pmax));
        SVA_LAUNCH_OR_REFUSED(launch_build_prompt(s.at<float>(0), (int)nspk, s.at<float>(1), s.at<float>(2), s.at<float>(3), s.at<int>(4), s.at<int>(5), (int)Pmax, (int)R,
                                                  (int)dl, (int)ncb, (int)cbs, (int)D, s.at<float>(6), (int)rows, 0));
        SVA_HIP(hipDeviceSynchronize());
        return s.down(6, F * rows * D);
    }
    if (kind == 6) {          // build_delayfill
        const long B = d[0], n = d[1], dl = d[2], D = d[3], cap = d[4], md = d[5], n_rows = d[6], rows = 2 * dl - 1;
        SVA_HOOK_CHECK(B >= 1 && B <= 4096 && n >= 1 && n <= B && dl >= 1 && D >= 1 && D <= 8192 && cap >= 1 && cap <= 65536 && md >= 1 && md <= 64 && n_rows >= 1 &&
                       n_rows * D <= kStepMax && B * md * D <= kStepMax, "build_delayfill hook: sizes");
        SVA_HOOK_REFUSE(is_pow2(cap) && dl <= md && dl <= cap, "build_delayfill hook: a power-of-two capacity, d <= max_delay, d <= capacity");
        SVA_HOOK_CHECK(ptrs[1] && ptrs[5], "build_delayfill hook: history / slot list");
        SVA_HOOK_REFUSE(all_in((const int*)ptrs[5], (size_t)n, 0, B), "build_delayfill hook: a listed slot outside the batch");
        SVA_HOOK_REFUSE(all_in((const int*)ptrs[1], (size_t)(B * cap), 0, n_rows), "build_delayfill hook: a content code outside the table");
        SVA_TRY(s.up(6, F * n * rows * D)); SVA_TRY(s.up(7, I * n * rows)); SVA_TRY(s.up(8, I * n * rows)); SVA_TRY(s.up(9, F * B * D));
        SVA_TRY(s.up(0, F * n_rows * D)); SVA_TRY(s.up(1, I * B * cap)); SVA_TRY(s.up(2, I * B)); SVA_TRY(s.up(3, F * B * md * D)); SVA_TRY(s.up(4, I * B)); SVA_TRY(s.up(5, I * n));
        SVA_LAUNCH_OR_REFUSED(launch_build_delayfill(s.at<float>(0), s.at<int>(1), (int)cap, s.at<int>(2), s.at<float>(3), (int)md, s.at<int>(4), (int)dl, (int)D, s.at<float>(6),
                                                     s.at<int>(7), s.at<int>(8), s.at<float>(9), s.at<int>(5), (int)n, 0));
        SVA_HIP(hipDeviceSynchronize());
        SVA_TRY(s.down(6, F * n * rows * D)); SVA_TRY(s.down(7, I * n * rows)); SVA_TRY(s.down(8, I * n * rows)); SVA_TRY(s.down(9, F * B * D));
        return 0;
    }
    if (kind == 7 || kind == 8) {          // build_reprefill / finish_reprefill
        const long B = d[0], n = d[1], dl = d[2], ncb = d[3], cbs = d[4], D = d[5], nspk = d[6], cap = d[7], md = d[8], n_rows = d[9];
        SVA_HOOK_CHECK(B >= 1 && B <= 4096 && n >= 1 && dl >= 1 && ncb >= 1 && cbs >= 1 && D >= 1 && D <= 8192 && nspk >= 0 && cap >= 1 && cap <= 65536 && md >= 1 && md <= 64 &&
                       n_rows >= 1 && n_rows * D <= kStepMax && ncb * cbs * D <= kStepMax && B * md * D <= kStepMax, "re-prefill hook: sizes");
        SVA_HOOK_REFUSE(n <= 128 && ncb <= 8 && is_pow2(cap) && dl <= md, "re-prefill hook: n <= 128, ncb <= 8, a power-of-two capacity, d <= max_delay");
        for (int i = 0; i < 5; ++i) SVA_HOOK_CHECK(ptrs[i], "re-prefill hook: per-slot arrays");
        const int *hs = (const int*)ptrs[0], *hRt = (const int*)ptrs[1], *hnf = (const int*)ptrs[2], *hna = (const int*)ptrs[3], *hnc = (const int*)ptrs[4];
        SVA_HOOK_REFUSE(all_in(hs, (size_t)n, 0, B), "re-prefill hook: a slot outside the batch");
        ReprefillArgs a;
        a.n = (int)n;
        a.row_off[0] = 0;
        for (long i = 0; i < n; ++i) {
            SVA_HOOK_REFUSE(hna[i] >= 0 && hna[i] <= cap && hRt[i] >= 0 && hRt[i] <= 65536, "re-prefill hook: na / Rt out of range");
            a.slot[i] = hs[i]; a.Rt[i] = hRt[i]; a.nf[i] = hnf[i]; a.na[i] = hna[i]; a.ncon[i] = hnc[i];
            a.row_off[i + 1] = a.row_off[i] + 2 * hna[i];
        }
        const long M = std::max(a.row_off[n], 1);
        const int ic = kind == 7 ? 7 : -1, ip = kind == 7 ? 8 : 6, it = kind == 7 ? 9 : 7;       // content_hist, pred_hist, ref_tail
        SVA_HOOK_CHECK(ptrs[ip] && ptrs[it] && (ic < 0 || ptrs[ic]), "re-prefill hook: histories");
        if (ic >= 0) SVA_HOOK_REFUSE(all_in((const int*)ptrs[ic], (size_t)(B * cap), 0, n_rows), "re-prefill hook: a content code outside the table");
        SVA_HOOK_REFUSE(all_in((const int*)ptrs[ip], (size_t)(B * ncb * cap), 0, cbs), "re-prefill hook: a predicted code outside its codebook");
        SVA_HOOK_REFUSE(all_in((const int*)ptrs[it], (size_t)(B * ncb * md), 0, cbs), "re-prefill hook: a reference code outside its codebook");
        if (kind == 7) {
            SVA_TRY(s.up(10, F * M * D)); SVA_TRY(s.up(11, I * M)); SVA_TRY(s.up(12, I * M));
            SVA_TRY(s.up(5, F * n_rows * D)); SVA_TRY(s.up(6, F * ncb * cbs * D)); SVA_TRY(s.up(7, I * B * cap)); SVA_TRY(s.up(8, I * B * ncb * cap)); SVA_TRY(s.up(9, I * B * ncb * md));
            SVA_LAUNCH_OR_REFUSED(launch_build_reprefill(a, s.at<float>(5), s.at<float>(6), s.at<int>(7), s.at<int>(8), (int)cap, s.at<int>(9), (int)md, (int)dl, (int)ncb, (int)cbs,
                                                         (int)D, (int)nspk, s.at<float>(10), s.at<int>(11), s.at<int>(12), 0));
            SVA_HIP(hipDeviceSynchronize());
            SVA_TRY(s.down(10, F * M * D)); SVA_TRY(s.down(11, I * M)); SVA_TRY(s.down(12, I * M));
            return 0;
        }
        SVA_TRY(s.up(8, F * B * md * D)); SVA_TRY(s.up(9, I * B));
        SVA_TRY(s.up(5, F * ncb * cbs * D)); SVA_TRY(s.up(6, I * B * ncb * cap)); SVA_TRY(s.up(7, I * B * ncb * md));
        SVA_LAUNCH_OR_REFUSED(launch_finish_reprefill(a, s.at<float>(5), s.at<int>(6), (int)cap, s.at<int>(7), (int)md, (int)dl, (int)ncb, (int)cbs, (int)D, (int)nspk,
                                                      s.at<float>(8), s.at<int>(9), 0));
        SVA_HIP(hipDeviceSynchronize());
        SVA_TRY(s.down(8, F * B * md * D)); SVA_TRY(s.down(9, I * B));
        return 0;
    }
    if (kind == 9 || kind == 10) {          // copy_rows / copy_rows2
        const long rows = d[0], D = d[1], stride = d[2], off = d[3], s_len = d[4];
        SVA_HOOK_CHECK(rows >= 1 && rows <= 4096 && D >= 1 && D <= 8192 && s_len >= 1 && s_len <= kStepMax, "copy_rows hook: sizes");
        SVA_HOOK_REFUSE(stride >= 0 && off >= 0 && off + (rows - 1) * stride + D <= s_len, "copy_rows hook: source rows outside src");
        SVA_TRY(s.up(1, F * rows * D));
        if (kind == 10) SVA_TRY(s.up(2, F * rows * D));
        SVA_TRY(s.up(0, F * s_len));
        if (kind == 9) SVA_LAUNCH_OR_REFUSED(launch_copy_rows(s.at<float>(0), stride, off, s.at<float>(1), (int)D, (int)rows, 0));
        else SVA_LAUNCH_OR_REFUSED(launch_copy_rows2(s.at<float>(0), stride, off, s.at<float>(1), s.at<float>(2), (int)D, (int)rows, 0));
        SVA_HIP(hipDeviceSynchronize());
        SVA_TRY(s.down(1, F * rows * D));
        if (kind == 10) SVA_TRY(s.down(2, F * rows * D));
        return 0;
    }
    if (kind == 11 || kind == 12) {          // broadcast_row (d: B, bstride, C, len, src_row, lo, hi) / fill_rows (d: B, bstride, C, len, rows)
        const long B = d[0], bs = d[1], C = d[2], len = d[3];
        SVA_HOOK_CHECK(B >= 1 && B <= 4096 && C >= 1 && C <= 8192 && len >= 1 && len <= kStepMax && bs >= 0, "row fill hook: sizes");
        if (kind == 11) {
            const long src_row = d[4], lo = d[5], hi = d[6];
            SVA_HOOK_REFUSE(src_row >= 0 && lo >= 0 && hi > lo && hi <= 65535 && (B - 1) * bs + std::max(hi, src_row + 1) * C <= len, "broadcast_row hook: rows outside the buffer");
            SVA_TRY(s.up(0, F * len));
            SVA_LAUNCH_OR_REFUSED(launch_broadcast_row(s.at<float>(0), bs, (int)src_row, (int)lo, (int)hi, (int)C, (int)B, 0));
        } else {
            const long rows = d[4];
            SVA_HOOK_REFUSE(rows >= 0 && rows <= 65535 && (B - 1) * bs + rows * C <= len, "fill_rows hook: rows outside the buffer");
            SVA_TRY(s.up(0, F * len)); SVA_TRY(s.up(1, F * C));
            SVA_LAUNCH_OR_REFUSED(launch_fill_rows(s.at<float>(0), bs, (int)C, s.at<float>(1), (int)rows, (int)B, 0));
        }
        SVA_HIP(hipDeviceSynchronize());
        return s.down(0, F * len);
    }
    if (kind >= 13 && kind <= 16) {          // inc (d: len, v) / add_list (d: len, v, n) / add_vec (d: len, v, n) / set_slot_i32 (d: len, v, slot)
        const long len = d[0], v = d[1], x = kind == 13 ? 0 : d[2];
        SVA_HOOK_CHECK(len >= 1 && len <= kStepMax, "counter hook: sizes");
        SVA_TRY(s.up(0, I * len));
        if (kind == 13) SVA_LAUNCH_OR_REFUSED(launch_inc(s.at<int>(0), (int)v, 0));
        else if (kind == 14) {
            SVA_HOOK_CHECK(x >= 1 && x <= kStepMax && ptrs[1], "add_list hook: list");
            SVA_HOOK_REFUSE(all_in((const int*)ptrs[1], (size_t)x, 0, len), "add_list hook: a listed index outside the array");
            SVA_TRY(s.up(1, I * x));
            SVA_LAUNCH_OR_REFUSED(launch_add_list(s.at<int>(0), s.at<int>(1), (int)x, (int)v, 0));
        } else if (kind == 15) {
            SVA_HOOK_REFUSE(x >= 1 && x <= len, "add_vec hook: n outside the array");
            SVA_LAUNCH_OR_REFUSED(launch_add_vec(s.at<int>(0), (int)x, (int)v, 0));
        } else {
            SVA_HOOK_REFUSE(x >= 0 && x < len, "set_slot_i32 hook: slot outside the array");
            SVA_LAUNCH_OR_REFUSED(launch_set_slot_i32(s.at<int>(0), (int)x, (int)v, 0));
        }
        SVA_HIP(hipDeviceSynchronize());
        return s.down(0, I * len);
    }
    if (kind == 17) {          // history_rows_copy: d n_desc, n_slots, slot_lo, to_live, len(buf), len(save), save_bstride, then (offset, bstride, H, C, save offset) per descriptor
        const long nd = d[0], ns = d[1], slot_lo = d[2], to_live = d[3], b_len = d[4], s_len = d[5], sbs = d[6];
        SVA_HOOK_CHECK(nd >= 0 && nd <= 64 && ns >= 1 && ns <= 4096 && slot_lo >= 0 && slot_lo <= 4096 && b_len >= 1 && b_len <= kStepMax && s_len >= 1 && s_len <= kStepMax && sbs >= 0,
                       "history_rows_copy hook: sizes");
        SVA_TRY(s.up(0, F * b_len)); SVA_TRY(s.up(1, F * s_len));
        std::vector<ShiftDesc> hd(nd);
        std::vector<long> offs(nd);
        const long top = slot_lo + ns - 1;
        for (long i = 0; i < nd; ++i) {
            const long off = d[7 + 5 * i], bs = d[8 + 5 * i], H = d[9 + 5 * i], C = d[10 + 5 * i], so = d[11 + 5 * i];
            SVA_HOOK_REFUSE(off >= 0 && bs >= 0 && H >= 0 && C >= 1 && H < (1 << 20) && C < (1 << 20) && so >= 0 && off + top * bs + H * C <= b_len && top * sbs + so + H * C <= s_len,
                            "history_rows_copy hook: rows outside the buffers");
            hd[i].ptr = s.at<float>(0) + off; hd[i].bstride = bs; hd[i].H = (int)H; hd[i].T = 0; hd[i].C = (int)C; hd[i].pad = 0;
            offs[i] = so;
        }
        SVA_TRY(s.b[2].put(hd.data(), sizeof(ShiftDesc) * (size_t)nd)); SVA_TRY(s.b[3].put(offs.data(), sizeof(long) * (size_t)nd));
        SVA_LAUNCH_OR_REFUSED(launch_history_rows_copy(s.at<ShiftDesc>(2), (int)nd, s.at<long>(3), s.at<float>(1), sbs, (int)slot_lo, (int)ns, (int)to_live, 0));
        SVA_HIP(hipDeviceSynchronize());
        SVA_TRY(s.down(0, F * b_len));
        return s.down(1, F * s_len);
    }
    if (kind == 18) {          // history_rows_move: d n_desc, slot, len(src), len(dst), then (source offset, destination offset, destination bstride, H, C) per descriptor
        const long nd = d[0], slot = d[1], s_len = d[2], t_len = d[3];
        SVA_HOOK_CHECK(nd >= 0 && nd <= 64 && slot >= 0 && slot <= 4096 && s_len >= 1 && s_len <= kStepMax && t_len >= 1 && t_len <= kStepMax, "history_rows_move hook: sizes");
        SVA_TRY(s.up(1, F * t_len)); SVA_TRY(s.up(0, F * s_len));
        std::vector<ShiftDesc> sd(nd), dd(nd);
        for (long i = 0; i < nd; ++i) {
            const long so = d[4 + 5 * i], to = d[5 + 5 * i], bs = d[6 + 5 * i], H = d[7 + 5 * i], C = d[8 + 5 * i];
            SVA_HOOK_REFUSE(so >= 0 && to >= 0 && bs >= 0 && H >= 0 && C >= 1 && H < (1 << 20) && C < (1 << 20) && so + H * C <= s_len && to + slot * bs + H * C <= t_len,
                            "history_rows_move hook: rows outside the buffers");
            sd[i].ptr = s.at<float>(0) + so; sd[i].bstride = 0; sd[i].H = (int)H; sd[i].T = 0; sd[i].C = (int)C; sd[i].pad = 0;
            dd[i].ptr = s.at<float>(1) + to; dd[i].bstride = bs; dd[i].H = (int)H; dd[i].T = 0; dd[i].C = (int)C; dd[i].pad = 0;
        }
        SVA_TRY(s.b[2].put(sd.data(), sizeof(ShiftDesc) * (size_t)nd)); SVA_TRY(s.b[3].put(dd.data(), sizeof(ShiftDesc) * (size_t)nd));
        SVA_LAUNCH_OR_REFUSED(launch_history_rows_move(s.at<ShiftDesc>(2), s.at<ShiftDesc>(3), (int)nd, (int)slot, 0));
        SVA_HIP(hipDeviceSynchronize());
        return s.down(1, F * t_len);
    }
    if (kind == 19) {          // put_row
        const long n_rows = d[0], code = d[1], D = d[2];
        SVA_HOOK_CHECK(n_rows >= 1 && D >= 1 && D <= 8192 && n_rows * D <= kStepMax, "put_row hook: sizes");
        SVA_HOOK_REFUSE(code >= 0 && code < n_rows, "put_row hook: the code outside the table");
        SVA_TRY(s.up(1, F * D)); SVA_TRY(s.up(0, F * n_rows * D));
        SVA_LAUNCH_OR_REFUSED(launch_put_row(s.at<float>(0), code, (int)D, s.at<float>(1), 0));
        SVA_HIP(hipDeviceSynchronize());
        return s.down(1, F * D);
    }
    if (kind == 20) {          // mean3
        const long B = d[0], ybs = d[1], y_len = d[2], obs = d[3], o_off = d[4], o_len = d[5], n4 = d[6];
        SVA_HOOK_CHECK(B >= 1 && B <= 4096 && y_len >= 1 && y_len <= kStepMax && o_len >= 1 && o_len <= kStepMax, "mean3 hook: sizes");
        SVA_HOOK_REFUSE(n4 >= 1 && ybs >= 0 && obs >= 0 && o_off >= 0 && (B - 1) * ybs + 4 * n4 <= y_len && (B - 1) * obs + o_off + 4 * n4 <= o_len, "mean3 hook: lanes outside the arrays");
        SVA_TRY(s.up(3, F * o_len)); SVA_TRY(s.up(0, F * y_len)); SVA_TRY(s.up(1, F * y_len)); SVA_TRY(s.up(2, F * y_len));
        SVA_LAUNCH_OR_REFUSED(launch_mean3(s.at<float>(0), s.at<float>(1), s.at<float>(2), ybs, s.at<float>(3), obs, o_off, n4, (int)B, 0));
        SVA_HIP(hipDeviceSynchronize());
        return s.down(3, F * o_len);
    }
    SVA_HOOK_CHECK(kind == 21, "step ops hook: kind 0 .. 21");          // copy_tokens
    const long B = d[0], Ht = d[1], gap = d[2], c = d[3], T2 = d[4], D = d[5], tbs = d[6], t_len = d[7], dbs = d[8], d_len = d[9];
    SVA_HOOK_CHECK(B >= 1 && B <= 4096 && D >= 1 && D <= 8192 && t_len >= 1 && t_len <= kStepMax && d_len >= 1 && d_len <= kStepMax, "copy_tokens hook: sizes");
    SVA_HOOK_REFUSE(Ht >= 0 && gap >= 0 && c >= 1 && T2 >= Ht + c && Ht + c <= 65535 && tbs >= 0 && dbs >= 0 && (B - 1) * tbs + (Ht + gap + c) * D <= t_len && (B - 1) * dbs + T2 * D <= d_len,
                    "copy_tokens hook: rows outside the arrays");
    SVA_TRY(s.up(1, F * d_len)); SVA_TRY(s.up(0, F * t_len));
    SVA_LAUNCH_OR_REFUSED(launch_copy_tokens(s.at<float>(0), tbs, (int)Ht, (int)gap, (int)c, s.at<float>(1), dbs, (int)T2, (int)D, (int)B, 0));
    SVA_HIP(hipDeviceSynchronize());
    return s.down(1, F * d_len);
}

// launch_voc_level (voc_fused.hip) from host arrays.  d: C, B, Tl, xH, x_bstride, len(X), y_bstride, len(Y), dil0, dil1, dil2, rows_per_frame, frames_done;
// ptrs: 0 X, 1 .. 3 the branch outputs Y3[br] (in / out, len(Y) each), 4 W: the 18 weights back to back in (branch, conv) order, [C][k C] each, k = 3 / 7 / 11,
// 5 bias [18][C], 6 int [1] (out): the tile height TR the launcher chose.  Returns 1 when the launcher refuses.
extern "C" int sva_test_voc_level(int device, const long long* d, const float* fpar, void* const* ptrs) {
    (void)fpar;
    SVA_CHECK(d && ptrs, "sva_test_voc_level: null argument");
    SVA_HIP(hipSetDevice(device));
    const long C = d[0], B = d[1], Tl = d[2], xH = d[3], xbs = d[4], x_len = d[5], ybs = d[6], y_len = d[7], rpf = d[11], fd = d[12];
    const int dil[3] = {(int)d[8], (int)d[9], (int)d[10]};
    SVA_HOOK_CHECK(C >= 1 && C <= 64 && B >= 1 && B <= 64 && Tl >= 1 && Tl <= (1 << 16) && xH >= 0 && xH <= 4096 && xbs >= 0 && ybs >= 0 && x_len >= 1 && x_len <= kStepMax &&
                   y_len >= 1 && y_len <= kStepMax && rpf >= 0 && fd >= 0, "voc_level hook: sizes");
    for (int j = 0; j < 3; ++j) SVA_HOOK_CHECK(dil[j] >= 1 && dil[j] <= 8, "voc_level hook: dilations 1 .. 8");
    SVA_HOOK_CHECK((B - 1) * xbs + (xH + Tl) * C <= x_len && (B - 1) * ybs + Tl * C <= y_len, "voc_level hook: rows outside X / Y");
    SVA_HOOK_CHECK((xbs * 4) % 16 == 0 && (ybs * 4) % 16 == 0, "voc_level hook: 16-byte rows");
    for (int i = 0; i < 7; ++i) SVA_HOOK_CHECK(ptrs[i], "voc_level hook: a required array is missing");
    static const int ks[3] = {3, 7, 11};
    const long w_total = 6 * (3 + 7 + 11) * C * C;
    DevBuf bx, by[3], bw, bb, bf;
    for (int br = 0; br < 3; ++br) SVA_TRY(by[br].put(ptrs[1 + br], sizeof(float) * (size_t)y_len));
    SVA_TRY(bx.put(ptrs[0], sizeof(float) * (size_t)x_len));
    SVA_TRY(bw.put(ptrs[4], sizeof(float) * (size_t)w_total));
    SVA_TRY(bb.put(ptrs[5], sizeof(float) * (size_t)(18 * C)));
    const int fdi = (int)fd;
    SVA_TRY(bf.put(&fdi, sizeof(int)));
    const float* W[3][6];
    const float* bias[3][6];
    float* y3[3];
    long wo = 0;
    for (int br = 0; br < 3; ++br) {
        for (int q = 0; q < 6; ++q) { W[br][q] = bw.as<float>() + wo; wo += (long)ks[br] * C * C; bias[br][q] = bb.as<float>() + (long)(br * 6 + q) * C; }
        y3[br] = by[br].as<float>();
    }
    SVA_LAUNCH_OR_REFUSED(launch_voc_level(bx.as<float>(), xbs, (int)xH, (int)C, (int)B, (int)Tl, W, bias, dil, y3, ybs, bf.as<int>(), (int)rpf, 0, (int*)ptrs[6]));
    SVA_HIP(hipDeviceSynchronize());
    for (int br = 0; br < 3; ++br) SVA_TRY(by[br].get(ptrs[1 + br], sizeof(float) * (size_t)y_len));
    return 0;
}

// launch_voc_conv (gemm_planes.hip: voc_conv_kernel -- one conv stage of 1..3 ResBlock branches of a narrow HiFiGAN level) from host arrays, the
// operands made the way the engine makes them: input planes by the row-major arm of launch_to_planes_act over caller-given rows of caller-filled
// planes (or handed in ready: one launch's Cp as the next one's Ap), weight planes by make_weight_planes (C = 32) / make_weight_planes_padded
// (C = 16).  Descriptor and array order: include/sva.h.  Every row the launch may touch is checked against the arrays first -- a failed check
// returns 1 and nothing is launched; what launch_voc_conv itself refuses returns 1 as well.  After a refusal no array is written back.
namespace {
enum { VC_C, VC_MODE, VC_B, VC_T, VC_N, VC_CU_LIMIT, VC_REPEAT, VC_NH = 8 };
enum { VM_TAPS, VM_DIL, VM_A_ROWS_B, VM_A_ROW0, VM_C_BSTRIDE, VM_C_OFF, VM_F_LEN, VM_R_BSTRIDE, VM_R_OFF, VM_R_LEN, VM_C_ROWS_B, VM_C_ROW0, VM_CONV, VM_CONV_ROW0,
       VM_CONV_T, VM_DROP, VM_ND = 16 };
enum { VP_A, VP_AP, VP_W, VP_WP, VP_BIAS, VP_RES, VP_CF, VP_CP, VP_NP = 8 };
struct VocMember {
    DevBuf A, Ap, W, Wp, bias, res, Cf, Cp;
    size_t ap_elems = 0, wp_elems = 0, f_len = 0, r_len = 0, cp_elems = 0;
    std::vector<float> cf0;             // Cf as the caller handed it in
    std::vector<uint16_t> cp0;          // Cp likewise
};
}  // namespace

extern "C" int sva_test_voc_conv(int device, const long long* d, const float* fpar, void* const* ptrs) {
    (void)fpar;
    SVA_CHECK(d && ptrs, "sva_test_voc_conv: null argument");
    const long C = d[VC_C], B = d[VC_B], T = d[VC_T], n = d[VC_N], cu_limit = d[VC_CU_LIMIT];
    const int mode = (int)d[VC_MODE];
    const bool repeat = d[VC_REPEAT] != 0;
    SVA_HOOK_CHECK((C == 16 || C == 32 || C == 64) && B >= 1 && B <= 64 && T >= 1 && T <= (1 << 16) && n >= 0 && n <= 4 && cu_limit >= 0 && cu_limit <= 1024 &&
                   d[VC_MODE] >= 0 && d[VC_MODE] <= 2, "voc_conv hook: sizes");
    SVA_HOOK_CHECK(!repeat || ptrs[1], "voc_conv hook: a repeated launch needs the verdict word");
    const bool fp16 = mode == PLANES_H3 || mode == PLANES_H1;          // (another format reaches the launcher with operands nobody made: it refuses)
    const int npl = planes_count(mode), nm = (int)std::min(n, 3L);     // (n = 4 reaches the launcher with three members built: it refuses)
    // ---- every member's geometry against its arrays, before anything is uploaded ----
    for (int i = 0; i < nm; ++i) {
        const long long* m = d + VC_NH + VM_ND * i;
        void* const* pp = ptrs + 2 + VP_NP * i;
        const long taps = m[VM_TAPS], dil = m[VM_DIL], a_rows_b = m[VM_A_ROWS_B], a_row0 = m[VM_A_ROW0], c_bs = m[VM_C_BSTRIDE], c_off = m[VM_C_OFF], f_len = m[VM_F_LEN],
                   r_bs = m[VM_R_BSTRIDE], r_off = m[VM_R_OFF], r_len = m[VM_R_LEN], c_rows_b = m[VM_C_ROWS_B], c_row0 = m[VM_C_ROW0], conv = m[VM_CONV],
                   conv_row0 = m[VM_CONV_ROW0], conv_T = m[VM_CONV_T];
        SVA_HOOK_CHECK(taps >= 1 && taps <= 64 && dil >= 1 && dil <= 64 && a_rows_b >= 1 && a_rows_b <= (1 << 20) && c_rows_b >= 0 && c_rows_b <= (1 << 20) && f_len >= 0 &&
                       f_len <= kStepMax && r_len >= 0 && r_len <= kStepMax && conv >= 0 && conv <= 2 && m[VM_DROP] >= 0 && m[VM_DROP] <= 3, "voc_conv hook: member sizes");
        SVA_HOOK_CHECK(pp[VP_AP] && pp[VP_W] && pp[VP_WP] && (!conv || pp[VP_A]), "voc_conv hook: Ap, W and Wp are required, A with a conversion");
        SVA_HOOK_CHECK((!pp[VP_CF] || f_len >= 1) && (!pp[VP_RES] || r_len >= 1) && (!pp[VP_CP] || c_rows_b >= 1), "voc_conv hook: an output array without its length");
        SVA_HOOK_REFUSE(a_row0 >= 0 && a_row0 + T + (taps - 1) * dil <= a_rows_b, "voc_conv hook: input rows outside the planes");
        SVA_HOOK_REFUSE(!conv || (conv_row0 >= 0 && conv_T >= 1 && conv_row0 + conv_T <= a_rows_b), "voc_conv hook: converted rows outside the planes");
        SVA_HOOK_REFUSE(!pp[VP_CF] || (c_off >= 0 && c_bs >= 0 && c_off % 4 == 0 && c_bs % 4 == 0 && (B - 1) * c_bs + c_off + T * C <= f_len), "voc_conv hook: Cf rows outside the array");
        SVA_HOOK_REFUSE(!pp[VP_RES] || (r_off >= 0 && r_bs >= 0 && r_off % 4 == 0 && r_bs % 4 == 0 && (B - 1) * r_bs + r_off + T * C <= r_len), "voc_conv hook: res rows outside the array");
        SVA_HOOK_REFUSE(!pp[VP_CP] || (c_row0 >= 0 && c_row0 + T <= c_rows_b), "voc_conv hook: Cp rows outside the planes");
    }
    SVA_HIP(hipSetDevice(device));
    VocConvGroup gg;
    gg.n = (int)n; gg.B = (int)B; gg.T = (int)T;
    VocMember mem[3];
    DevBuf bovf;
    if (ptrs[0]) { SVA_TRY(bovf.put(ptrs[0], sizeof(int))); gg.ovf = bovf.as<int>(); }
    for (int i = 0; i < nm; ++i) {
        const long long* m = d + VC_NH + VM_ND * i;
        void* const* pp = ptrs + 2 + VP_NP * i;
        VocMember& M = mem[i];
        VocConv& g = gg.g[i];
        const long taps = m[VM_TAPS], a_rows_b = m[VM_A_ROWS_B], K = taps * C, Kp = C == 16 ? padded_weight_k((int)K) : K;
        const long a_rows = B * a_rows_b;
        M.ap_elems = (size_t)npl * a_rows * C;
        SVA_TRY(M.Ap.put(pp[VP_AP], 2 * M.ap_elems));
        if (m[VM_CONV] && fp16) {
            SVA_TRY(M.A.put(pp[VP_A], sizeof(float) * a_rows * C));
            SVA_LAUNCH_OR_REFUSED(launch_to_planes_act(M.A.as<float>(), (int)B, a_rows_b, m[VM_CONV_ROW0], (int)m[VM_CONV_T], (int)C, M.Ap.as<unsigned short>(), a_rows * C, mode,
                                                       m[VM_CONV] == 2 ? 1 : 0, 0, 0));
        }
        SVA_TRY(M.W.put(pp[VP_W], sizeof(float) * C * K));
        M.wp_elems = (size_t)npl * C * Kp;
        SVA_TRY(M.Wp.alloc(2 * M.wp_elems));
        SVA_HIP(hipMemset(M.Wp.p, 0, 2 * M.wp_elems));
        if (fp16 && C == 16) {              // weight planes as sva_engine_finalize makes them
            SVA_TRY(make_weight_planes_padded(M.W.as<float>(), (int)C, (int)K, mode, M.Wp.as<unsigned short>(), &g.wp_inv));
        } else if (fp16) {
            const float* W = (const float*)pp[VP_W];
            float mx = 0.f;
            for (long k = 0; k < C * K; ++k) mx = std::max(mx, fabsf(W[k]));
            SVA_TRY(make_weight_planes(M.W.as<float>(), (int)C, (int)K, mx, mode, M.Wp.as<unsigned short>(), &g.wp_inv, 0));
        }
        g.Ap = (m[VM_DROP] & 1) ? nullptr : M.Ap.as<unsigned short>();
        g.ap_pstride = a_rows * C; g.a_rows_b = a_rows_b; g.a_row0 = m[VM_A_ROW0]; g.a_rows_total = a_rows;
        g.Wp = (m[VM_DROP] & 2) ? nullptr : M.Wp.as<unsigned short>();
        g.wp_pstride = C * Kp;
        g.taps = (int)taps; g.dil = (int)m[VM_DIL];
        if (pp[VP_BIAS]) { SVA_TRY(M.bias.put(pp[VP_BIAS], sizeof(float) * C)); g.bias = M.bias.as<float>(); }
        if (pp[VP_RES]) {
            M.r_len = (size_t)m[VM_R_LEN];
            SVA_TRY(M.res.put(pp[VP_RES], sizeof(float) * M.r_len));
            g.res = M.res.as<float>(); g.r_bstride = m[VM_R_BSTRIDE]; g.r_off = m[VM_R_OFF];
        }
        if (pp[VP_CF]) {
            M.f_len = (size_t)m[VM_F_LEN];
            M.cf0.assign((const float*)pp[VP_CF], (const float*)pp[VP_CF] + M.f_len);
            SVA_TRY(M.Cf.put(M.cf0.data(), sizeof(float) * M.f_len));
            g.Cf = M.Cf.as<float>(); g.c_bstride = m[VM_C_BSTRIDE]; g.c_off = m[VM_C_OFF];
        }
        if (pp[VP_CP]) {
            M.cp_elems = (size_t)npl * B * m[VM_C_ROWS_B] * C;
            M.cp0.assign((const uint16_t*)pp[VP_CP], (const uint16_t*)pp[VP_CP] + M.cp_elems);
            SVA_TRY(M.Cp.put(M.cp0.data(), 2 * M.cp_elems));
            g.Cp = M.Cp.as<unsigned short>(); g.cp_pstride = B * m[VM_C_ROWS_B] * C; g.c_rows_b = m[VM_C_ROWS_B]; g.c_row0 = m[VM_C_ROW0];
        }
    }
    SVA_HIP(hipDeviceSynchronize());
    auto run = [&]() -> int {
        SVA_LAUNCH_OR_REFUSED(launch_voc_conv(gg, (int)C, mode, (int)cu_limit, 0));
        SVA_HIP(hipDeviceSynchronize());
        return 0;
    };
    SVA_TRY(run());             // (refused: 1, and the caller's arrays stay as they are)
    for (int i = 0; i < nm; ++i) {
        void* const* pp = ptrs + 2 + VP_NP * i;
        VocMember& M = mem[i];
        SVA_TRY(M.Ap.get(pp[VP_AP], 2 * M.ap_elems));
        SVA_TRY(M.Wp.get(pp[VP_WP], 2 * M.wp_elems));
        if (pp[VP_RES]) SVA_TRY(M.res.get(pp[VP_RES], sizeof(float) * M.r_len));
        if (pp[VP_CF]) SVA_TRY(M.Cf.get(pp[VP_CF], sizeof(float) * M.f_len));
        if (pp[VP_CP]) SVA_TRY(M.Cp.get(pp[VP_CP], 2 * M.cp_elems));
    }
    if (ptrs[0]) SVA_TRY(bovf.get(ptrs[0], sizeof(int)));
    if (repeat) {               // the same launch again from the same initial Cf / Cp: the tile walk has no order that may change a bit
        for (int i = 0; i < nm; ++i) {
            if (mem[i].f_len) SVA_HIP(hipMemcpy(mem[i].Cf.p, mem[i].cf0.data(), sizeof(float) * mem[i].f_len, hipMemcpyHostToDevice));
            if (mem[i].cp_elems) SVA_HIP(hipMemcpy(mem[i].Cp.p, mem[i].cp0.data(), 2 * mem[i].cp_elems, hipMemcpyHostToDevice));
        }
        SVA_TRY(run());
        bool same = true;
        for (int i = 0; i < nm; ++i) {
            void* const* pp = ptrs + 2 + VP_NP * i;
            if (mem[i].f_len) {
                std::vector<float> c2(mem[i].f_len);
                SVA_TRY(mem[i].Cf.get(c2.data(), sizeof(float) * mem[i].f_len));
                same = same && memcmp(c2.data(), pp[VP_CF], sizeof(float) * mem[i].f_len) == 0;
            }
            if (mem[i].cp_elems) {
                std::vector<uint16_t> p2(mem[i].cp_elems);
                SVA_TRY(mem[i].Cp.get(p2.data(), 2 * mem[i].cp_elems));
                same = same && memcmp(p2.data(), pp[VP_CP], 2 * mem[i].cp_elems) == 0;
            }
        }
        *(int*)ptrs[1] = same ? 1 : 0;
    }
    return 0;
}

// Do the four chain streams of a pipelined batch (main, encoder side stream, AR, vocoder) each have a hardware queue of their own?  For
// every unordered pair (X, Y), in the order (main, aux0) (main, sa) (main, sv) (aux0, sa) (aux0, sv) (sa, sv): a bounded waiter kernel on
// X and, enqueued after it, a setter kernel on Y (stream_overlap.h); pair_ok[k] = 1 when the waiter saw the setter's store, 0 when it ran
// into its 2 ms limit -- the two streams share a hardware queue.  Synchronises the device; the batch's own state is not touched.
extern "C" int sva_test_stream_overlap(sva_batch* b, int* pair_ok) {
    SVA_CHECK(b && pair_ok, "sva_test_stream_overlap: a batch and an output array of 6 ints");
    SVA_CHECK(b->main_stream && b->aux0 && b->sa && b->sv, "sva_test_stream_overlap: the batch is not pipelined (no AR / vocoder streams)");
    SVA_HIP(hipSetDevice(b->e->device));
    DevBuf words;
    SVA_TRY(words.alloc(2 * sizeof(int)));
    const hipStream_t st[4] = {b->main_stream, b->aux0, b->sa, b->sv};
    SVA_HIP(sva_overlap::pairs_of_four(st, words.as<int>(), pair_ok));
    return 0;
}

// The dispatcher's decision for a described problem, without a GPU (include/sva.h).  Pointers are fabricated: nothing dereferences them.
static void plan_hook_problem(const int* d, ConvGemm* g) {
    alignas(16) static float mem[4];                                    // a 16-byte aligned address that stands for every operand
    float* const P = mem;
    const int B = d[0], T = d[1], N = d[2], Cin = d[3], taps = d[4], stride = d[5], dil = d[6], fl = d[7], op = d[8], mis = d[10];
    const int Nout = (fl & 32) ? N / 2 : N;
    const long H = (long)(taps - 1) * dil, rows = H + (long)T * stride;
    g->A = P; g->lda = Cin; g->a_bstride = rows * Cin; g->a_off = (mis & 1) ? 2 : 0;
    g->T = T; g->M = B * T; g->stride = stride; g->dil = dil; g->taps = taps; g->Cin = Cin;
    g->W = P; g->N = N;
    g->C = P; g->ldc = Nout + ((mis & 2) ? 1 : 0); g->c_bstride = (long)T * g->ldc; g->c_off = 0;
    if (fl & 1) g->bias = P;
    if (fl & 2) g->gamma = P;
    if (fl & 4) { g->res = P; g->ldr = Nout + ((mis & 4) ? 1 : 0); g->r_bstride = (long)T * g->ldr; g->r_off = 0; }
    if (fl & 8) g->act = ACT_GELU;
    g->a_silu = (fl >> 4) & 1; g->w13 = (fl >> 5) & 1; g->accumulate = (fl >> 6) & 1;
    if (fl & 128) g->rms_w = P;
    if (fl & 256) { g->dw_wT = P; g->dw_b = P; g->ln_w = P; g->ln_b = P; }
    g->cp_silu = (fl >> 9) & 1;
    if (op & 1) g->Wk = P;
    if (op & 2) g->Wh = P;
    if (op & 4) g->Wkh = P;
    if (op & 8) { g->Wp = reinterpret_cast<const unsigned short*>(P); g->wp_pstride = (long)N * taps * Cin; }
    g->pmode = d[9];
    if (op & 16) {          // A as planes over the dense rows of the tensor: (b, t) -> b * rows + t
        g->Ap = reinterpret_cast<const unsigned short*>(P); g->A = nullptr;
        g->ap_rows = (long)B * rows; g->ap_pstride = g->ap_rows * Cin;
    }
    if (op & 32) {
        g->Cp = reinterpret_cast<unsigned short*>(P); g->C = nullptr;
        g->cp_rows = (long)B * T; g->cp_pstride = g->cp_rows * Nout;
    }
}
extern "C" int sva_test_gemm_plan(const int* desc, int n, int* out) {
    SVA_CHECK(desc && out && n >= 1 && n <= 3, "test_gemm_plan: 1..3 members");
    ConvGemm gs[3];
    for (int i = 0; i < n; ++i) plan_hook_problem(desc + 12 * i, &gs[i]);
    ConvGemmGroup gg;
    int lead = 0;
    GemmPlan p;
    SVA_TRY(conv_gemm_group_of(gs, n, &gg, &lead));
    SVA_TRY(plan_conv_gemm(gg, lead, &p));
    out[0] = (int)p.family; out[1] = p.a; out[2] = p.b; out[3] = p.c; out[4] = p.z; out[5] = plan_report_kind(p, gg.g[lead].pmode);
    return 0;
}

// The slot book's transitions, scripted without a device (include/sva.h).  A `step` drives the book the way step_body does: the warm-up or steady
// step, the re-prefills it plans and their delay fills, then the activations that are due (prefill, delay fill, activated).
extern "C" int sva_test_slot_book(const int* cfg, const int* ops, int n_ops, int* trace) {
    SVA_CHECK(cfg && ops && trace && n_ops >= 0, "sva_test_slot_book: null argument");
    const int B = cfg[0], chunk = cfg[1], delay = cfg[2], max_seq_frames = cfg[3], buffer_frames = cfg[4], window = cfg[5], nspk = cfg[6];
    SVA_CHECK(B >= 1 && B <= 64 && chunk >= 1 && delay >= 1 && max_seq_frames >= 1 && buffer_frames >= 0 && window >= 1 && nspk >= 1, "sva_test_slot_book: bad config");
    const int W = 8 * B + 6;
    SlotBook book;
    book.reset(B);
    bool begun = false;
    int adopt_pos = -1, adopt_frames = -1;
    auto prefill = [&](int slot, int R) {          // one codebook of zeros stands for the prompt: only its length matters here
        const std::vector<int64_t> cc((size_t)R, 0);
        const std::vector<int32_t> ac((size_t)R, 0);
        book.prefilled(slot, nspk, R, R, 1, cc.data(), ac.data());
    };
    for (int k = 0; k < n_ops; ++k) {
        const int op = ops[3 * k], slot = ops[3 * k + 1], R = ops[3 * k + 2];
        int* row = trace + (size_t)k * W;
        std::fill(row, row + W, -1);
        StepPlan plan;
        std::vector<int> acts;
        int one_pass = -1, prime = -1;
        if (op == 1 || op == 3 || op == 4 || op == 5) SVA_CHECK(slot >= 0 && slot < B, "sva_test_slot_book: slot out of range");
        if (op == 1 || op == 3) SVA_CHECK(R > delay, "sva_test_slot_book: the prompt must be longer than the delay");
        if (op >= 2 && op != 5) SVA_CHECK(begun, "sva_test_slot_book: step / restart / retire before begin");
        if (op == 0) {
            SVA_CHECK(book.all_prefilled(), "sva_test_slot_book: begin before every slot was prefilled");
            book.begin();
            begun = true;
            prime = book.priming_frames(0, window, chunk);
            for (int i = 1; i < B; ++i) prime = std::min(prime, book.priming_frames(i, window, chunk));
        } else if (op == 1) {
            prefill(slot, R);
        } else if (op == 2) {
            if (!book.delay_filled) {
                if (book.warmup_step(chunk, delay)) {
                    std::vector<int> all(B);
                    for (int i = 0; i < B; ++i) all[i] = i;
                    book.delay_filled_for(all, delay);
                }
            } else {
                plan = book.steady_step(chunk, max_seq_frames, nspk);
                if (!plan.redo.empty()) one_pass = book.one_pass_ok(plan.redo, buffer_frames, delay) ? 1 : 0;
                for (int s_ : plan.redo) book.reprefilled(s_, book.reprefill_end(s_, nspk, buffer_frames));
                book.delay_filled_for(plan.redo, delay);
            }
            acts = book.due_activations(delay);
            for (int s_ : acts) {
                prefill(s_, book.s[s_].pending.R);
                book.delay_filled_for(std::vector<int>{s_}, delay);
                if (prime < 0) prime = book.priming_frames(s_, window, chunk);
                book.activated(s_);
            }
        } else if (op == 3) {
            PendingPrompt p;
            p.R = R;
            book.restart(slot, std::move(p), nspk, kSlotOutputMuted);
        } else if (op == 4) {
            book.retire(slot, kSlotInputMuted | kSlotOutputMuted);
        } else if (op == 5) {          // a prompt of delay + 1 + R frames whose stored copy is truncated to R frames (max_prompt_frames = R)
            SVA_CHECK(R >= 1, "sva_test_slot_book: a stored prompt has at least one frame");
            const std::vector<int64_t> cc((size_t)(delay + 1 + R), 0);
            const std::vector<int32_t> ac((size_t)(delay + 1 + R), 0);
            book.prefilled(slot, nspk, delay + 1 + R, R, 1, cc.data(), ac.data());
        } else if (op == 6) {          // stage the counters of the next adopt: last_pos = slot field, nframes = R field (ncontent = nframes + delay)
            adopt_pos = slot; adopt_frames = R;
        } else if (op == 7) {          // SlotBook::adopt (sva_stream_load): a decoding stream with a stored prompt of R frames and the staged counters
            SVA_CHECK(slot >= 0 && slot < B && R >= 1 && adopt_pos >= 0 && adopt_frames >= 0, "sva_test_slot_book: adopt needs a slot, a stored prompt and staged counters (op 6)");
            book.adopt(slot, adopt_pos, adopt_frames, adopt_frames + delay, std::vector<int64_t>((size_t)R, 0), std::vector<int32_t>((size_t)R, 0), 0.7f, 1.0f / 0.7f, 0.7f);
        } else {
            SVA_CHECK(false, "sva_test_slot_book: unknown op");
        }
        for (int i = 0; i < B; ++i) {
            const SlotHost& h = book.s[i];
            row[4 * i] = h.phase; row[4 * i + 1] = h.last_pos; row[4 * i + 2] = h.nframes; row[4 * i + 3] = h.ncontent;
        }
        row[4 * B] = book.delay_filled ? 1 : 0;
        row[4 * B + 1] = one_pass;
        row[4 * B + 2] = (int)plan.redo.size();
        for (size_t i = 0; i < plan.redo.size(); ++i) row[4 * B + 3 + i] = plan.redo[i];
        row[5 * B + 3] = (int)plan.rewind.size();
        for (size_t i = 0; i < plan.rewind.size(); ++i) { row[5 * B + 4 + 2 * i] = plan.rewind[i].first; row[5 * B + 5 + 2 * i] = plan.rewind[i].second; }
        row[7 * B + 4] = (int)acts.size();
        for (size_t i = 0; i < acts.size(); ++i) row[7 * B + 5 + i] = acts[i];
        row[8 * B + 5] = prime;
    }
    return 0;
}

// The stored prompt and its tail, without a device (include/sva.h): a prompt of R frames with content code i at frame i and audio code
// 1000 q + i in codebook q, stored truncated to Rt frames; out [ncb][n] = frames [first, first + n) of the last P stored frames.
extern "C" int sva_test_slot_prompt_tail(int R, int Rt, int ncb, int P, int first, int n, int* out, int* stored) {
    SVA_CHECK(out && stored && R >= 1 && Rt >= 1 && Rt <= R && ncb >= 1, "sva_test_slot_prompt_tail: bad prompt");
    SVA_CHECK(P >= 0 && P <= Rt && first >= 0 && n >= 0 && first + n <= P, "sva_test_slot_prompt_tail: frames outside the stored prompt's tail");
    std::vector<int64_t> cc((size_t)R);
    std::vector<int32_t> ac((size_t)ncb * R);
    for (int i = 0; i < R; ++i) cc[i] = i;
    for (int q = 0; q < ncb; ++q)
        for (int i = 0; i < R; ++i) ac[(size_t)q * R + i] = 1000 * q + i;
    SlotBook book;
    book.reset(1);
    book.prefilled(0, 33, R, Rt, ncb, cc.data(), ac.data());
    const SlotHost& h = book.s[0];
    stored[0] = h.ref_len; stored[1] = (int)h.ref_content.size(); stored[2] = (int)h.ref_audio.size(); stored[3] = (int)h.ref_content.back();
    book.prompt_tail(0, ncb, P, first, n, out);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The conv-GEMM in its conv and epilogue forms (include/sva.h: sva_test_conv_gemm; tests/test_gpu_conv_gemm.py): 1..3 members as whole host
// arrays with the caller's strides and offsets, a full ConvGemm per member, the dispatcher or one given plan, whole arrays back.
// Return codes: 0 ran, 1 REFUSED (the dispatcher, plan_accepts or a launcher's own check declined the problem: nothing was launched), -2 a HIP
// error, -4 arguments the hook itself declines (an index outside an array, an operand it cannot build).
// ------------------------------------------------------------------------------------------------------------------------------------
#define SVA_HOOK_ARG(cond, msg)                                                         \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            ::sva::set_error(std::string("sva_test_conv_gemm: ") + msg + " [" #cond "]"); \
            return -4;                                                                  \
        }                                                                               \
    } while (0)
namespace {
enum { CG_B, CG_T, CG_N, CG_CIN, CG_TAPS, CG_STRIDE, CG_DIL, CG_LDA, CG_A_OFF, CG_A_BSTRIDE, CG_A_LEN, CG_LDC, CG_C_OFF, CG_C_BSTRIDE, CG_C_LEN, CG_LDR,
       CG_R_OFF, CG_R_BSTRIDE, CG_R_LEN, CG_ACT, CG_ACCUMULATE, CG_A_SILU, CG_W13, CG_SKIP_LO, CG_SKIP_HI, CG_USE_WK, CG_PMODE, CG_A_PLANES, CG_C_PLANES,
       CG_CP_SILU, CG_ND = 32 };
enum { CP_A, CP_W, CP_BIAS, CP_GAMMA, CP_RES, CP_RMS_W, CP_DW_WT, CP_DW_B, CP_LN_W, CP_LN_B, CP_C, CP_CP, CP_AP, CP_NP = 16 };
struct ConvMember {
    DevBuf A, W, Wk, bias, gamma, res, rms, dww, dwb, lnw, lnb, C, Wp, Ap, Cp;
    std::vector<float> c0;              // C as the caller handed it in
    std::vector<uint16_t> cp0;          // Cp likewise
    size_t c_len = 0, cp_elems = 0, ap_elems = 0;
    float* c_host = nullptr;
    uint16_t *cp_host = nullptr, *ap_host = nullptr;
};
// one member: arguments checked, every index of the launch inside its array, operands uploaded / built
int conv_member_build(const long long* d, const float* fp, void* const* pp, ConvMember& m, ConvGemm& g) {
    const long B = d[CG_B], T = d[CG_T], N = d[CG_N], Cin = d[CG_CIN], taps = d[CG_TAPS], stride = d[CG_STRIDE], dil = d[CG_DIL];
    SVA_HOOK_ARG(B >= 1 && T >= 1 && N >= 1 && Cin >= 1 && taps >= 1 && stride >= 1 && dil >= 1 && B * T < (1 << 24) && N < (1 << 20) && taps * Cin < (1 << 20), "shape");
    const long K = taps * Cin, Nout = d[CG_W13] ? N / 2 : N;
    const float *A = (const float*)pp[CP_A], *W = (const float*)pp[CP_W], *bias = (const float*)pp[CP_BIAS], *gamma = (const float*)pp[CP_GAMMA],
                *res = (const float*)pp[CP_RES], *rms_w = (const float*)pp[CP_RMS_W], *dw_wT = (const float*)pp[CP_DW_WT];
    SVA_HOOK_ARG(A && W && pp[CP_C], "A, W and C are required");
    SVA_HOOK_ARG(!dw_wT || (pp[CP_DW_B] && pp[CP_LN_W] && pp[CP_LN_B]), "the ConvNeXt prologue takes dw_wT, dw_b, ln_w and ln_b");
    // the largest index of every array the launch touches
    const long lda = d[CG_LDA], a_off = d[CG_A_OFF], a_bs = d[CG_A_BSTRIDE], a_len = d[CG_A_LEN];
    const long in_rows = (T - 1) * stride + (taps - 1) * dil + 1 + (dw_wT ? 6 : 0);
    SVA_HOOK_ARG(lda >= Cin && a_off >= 0 && a_bs >= 0 && (B - 1) * a_bs + a_off + (in_rows - 1) * lda + Cin <= a_len, "A index out of range");
    const long ldc = d[CG_LDC], c_off = d[CG_C_OFF], c_bs = d[CG_C_BSTRIDE], c_len = d[CG_C_LEN];
    SVA_HOOK_ARG(ldc >= Nout && c_off >= 0 && c_bs >= 0 && (B - 1) * c_bs + c_off + (T - 1) * ldc + Nout <= c_len, "C index out of range");
    const long ldr = d[CG_LDR], r_off = d[CG_R_OFF], r_bs = d[CG_R_BSTRIDE], r_len = d[CG_R_LEN];
    SVA_HOOK_ARG(!res || (ldr >= Nout && r_off >= 0 && r_bs >= 0 && (B - 1) * r_bs + r_off + (T - 1) * ldr + Nout <= r_len), "res index out of range");
    SVA_HOOK_ARG(d[CG_SKIP_LO] >= 0 && d[CG_SKIP_HI] <= T, "skip rows");
    SVA_TRY(m.A.put(A, sizeof(float) * a_len));
    SVA_TRY(m.W.put(W, sizeof(float) * N * K));
    m.c_host = (float*)pp[CP_C];
    m.c_len = (size_t)c_len;
    m.c0.assign(m.c_host, m.c_host + c_len);
    SVA_TRY(m.C.put(m.c0.data(), sizeof(float) * c_len));
    g.A = m.A.as<float>(); g.a_bstride = a_bs; g.a_off = a_off; g.lda = (int)lda; g.T = (int)T; g.M = (int)(B * T);
    g.stride = (int)stride; g.dil = (int)dil; g.taps = (int)taps; g.Cin = (int)Cin;
    g.W = m.W.as<float>(); g.N = (int)N;
    g.C = m.C.as<float>(); g.c_bstride = c_bs; g.c_off = c_off; g.ldc = (int)ldc;
    if (bias) { SVA_TRY(m.bias.put(bias, sizeof(float) * N)); g.bias = m.bias.as<float>(); }
    if (gamma) { SVA_TRY(m.gamma.put(gamma, sizeof(float) * N)); g.gamma = m.gamma.as<float>(); }
    if (res) { SVA_TRY(m.res.put(res, sizeof(float) * r_len)); g.res = m.res.as<float>(); g.r_bstride = r_bs; g.r_off = r_off; g.ldr = (int)ldr; }
    if (rms_w) { SVA_TRY(m.rms.put(rms_w, sizeof(float) * Cin)); g.rms_w = m.rms.as<float>(); g.rms_eps = fp[2]; }
    if (dw_wT) {
        SVA_TRY(m.dww.put(dw_wT, sizeof(float) * 7 * Cin));
        SVA_TRY(m.dwb.put(pp[CP_DW_B], sizeof(float) * Cin));
        SVA_TRY(m.lnw.put(pp[CP_LN_W], sizeof(float) * Cin));
        SVA_TRY(m.lnb.put(pp[CP_LN_B], sizeof(float) * Cin));
        g.dw_wT = m.dww.as<float>(); g.dw_b = m.dwb.as<float>(); g.ln_w = m.lnw.as<float>(); g.ln_b = m.lnb.as<float>(); g.ln_eps = fp[1];
    }
    g.scale = fp[0]; g.act = (int)d[CG_ACT]; g.accumulate = d[CG_ACCUMULATE] != 0; g.a_silu = d[CG_A_SILU] != 0; g.w13 = d[CG_W13] != 0;
    g.skip_lo = (int)d[CG_SKIP_LO]; g.skip_hi = (int)d[CG_SKIP_HI];
    if (d[CG_USE_WK]) {
        SVA_HOOK_ARG(K % 16 == 0, "packed weights take whole 16-k blocks");
        std::vector<float> wk;
        pack_fragment_major(W, (int)N, K, wk);
        SVA_TRY(m.Wk.put(wk.data(), sizeof(float) * wk.size()));
        g.Wk = m.Wk.as<float>();
    }
    const int pmode = (int)d[CG_PMODE];
    if (pmode >= 0) {           // weight planes as the engine makes them at finalize
        SVA_HOOK_ARG((pmode == PLANES_H3 || pmode == PLANES_H1) && Cin % 32 == 0, "planes: H3 or H1, whole 32-k blocks per tap");
        const int npl = planes_count(pmode);
        float mx = 0.f;
        for (long i = 0; i < N * K; ++i) mx = std::max(mx, fabsf(W[i]));
        SVA_TRY(m.Wp.alloc(2 * (size_t)npl * N * K));
        g.Wp = m.Wp.as<unsigned short>(); g.wp_pstride = N * K; g.pmode = pmode;
        SVA_TRY(make_weight_planes(g.W, (int)N, (int)K, mx, pmode, m.Wp.as<unsigned short>(), &g.wp_inv, 0));
    }
    if (d[CG_A_PLANES]) {       // the whole A array as planes over its dense rows (every pad row included), by the activation pass of the engine
        SVA_HOOK_ARG(pmode >= 0 && lda == Cin && a_len % lda == 0 && a_off % lda == 0 && a_bs % lda == 0 && stride == 1 && !d[CG_A_SILU] && !dw_wT && !rms_w,
                     "A as planes: dense rows of Cin values, stride 1, SiLU belongs to the producer");
        const long ap_rows = a_len / lda;
        const int npl = planes_count(pmode);
        SVA_HOOK_ARG(ap_rows < (1 << 24) && (B - 1) * (a_bs / lda) + a_off / lda + in_rows <= ap_rows, "A planes row out of range");
        m.ap_elems = (size_t)npl * ap_rows * Cin;
        SVA_TRY(m.Ap.alloc(2 * m.ap_elems));
        SVA_TRY(launch_to_planes_act(g.A, 1, ap_rows, 0, (int)ap_rows, (int)Cin, m.Ap.as<unsigned short>(), ap_rows * Cin, pmode, d[CG_A_PLANES] == 2 ? 1 : 0, 0));
        g.Ap = m.Ap.as<unsigned short>(); g.ap_pstride = ap_rows * Cin; g.ap_rows = ap_rows; g.A = nullptr;
        m.ap_host = (uint16_t*)pp[CP_AP];
    }
    if (d[CG_C_PLANES]) {       // C (also) as planes over the dense rows of the C array; uploaded first like C
        SVA_HOOK_ARG(pmode >= 0 && pp[CP_CP] && ldc == Nout && Nout % 32 == 0 && c_len % ldc == 0 && c_off % ldc == 0 && c_bs % ldc == 0,
                     "C as planes: dense rows of whole 32-column blocks");
        const long cp_rows = c_len / ldc;
        const int npl = planes_count(pmode);
        SVA_HOOK_ARG((B - 1) * (c_bs / ldc) + c_off / ldc + T <= cp_rows, "C planes row out of range");
        m.cp_elems = (size_t)npl * cp_rows * Nout;
        m.cp_host = (uint16_t*)pp[CP_CP];
        m.cp0.assign(m.cp_host, m.cp_host + m.cp_elems);
        SVA_TRY(m.Cp.put(m.cp0.data(), 2 * m.cp_elems));
        g.Cp = m.Cp.as<unsigned short>(); g.cp_pstride = cp_rows * Nout; g.cp_rows = cp_rows; g.cp_silu = d[CG_CP_SILU] != 0;
        if (d[CG_C_PLANES] == 2) g.C = nullptr;
    } else {
        SVA_HOOK_ARG(!d[CG_CP_SILU], "cp_silu needs C as planes");
    }
    return 0;
}
}  // namespace

extern "C" int sva_test_conv_gemm(int device, int n, const long long* desc, const float* fpar, void* const* ptrs, const int* plan, int repeat, int* out) {
    SVA_HOOK_ARG(n >= 1 && n <= 3 && desc && fpar && ptrs && plan && out, "1..3 members");
    SVA_HOOK_ARG(plan[0] >= -1 && plan[0] <= (int)GemmFamily::StreamH, "plan: -1 (the dispatcher) or a GemmFamily");
    out[0] = -1; out[1] = -1;
    SVA_HIP(hipSetDevice(device));
    ConvGemm gs[3];
    ConvMember mem[3];
    for (int i = 0; i < n; ++i) SVA_TRY(conv_member_build(desc + (size_t)CG_ND * i, fpar + 4 * i, ptrs + (size_t)CP_NP * i, mem[i], gs[i]));
    SVA_HIP(hipDeviceSynchronize());
    const GemmPlan p{(GemmFamily)(plan[0] < 0 ? 0 : plan[0]), plan[1], plan[2], plan[3], plan[4]};
    int kind_out = -1;
    auto run = [&]() -> int {
        const int rc = plan[0] < 0 ? launch_conv_gemm_group(gs, n, 0, &kind_out) : launch_conv_gemm_group_plan(gs, n, p, 0);
        if (rc == -1) return 1;         // an SVA_CHECK of the dispatcher / plan_accepts / a launcher: refused before any launch
        if (rc) return rc;
        SVA_HIP(hipDeviceSynchronize());
        return 0;
    };
    const int rc = run();
    if (rc != 0 && rc != 1) return rc;
    if (!rc) out[0] = plan[0] >= 0 ? plan_report_kind(p, gs[0].pmode) : kind_out;
    for (int i = 0; i < n; ++i) {       // (after a refusal too: the arrays come back as the device holds them, i.e. as they went in)
        SVA_TRY(mem[i].C.get(mem[i].c_host, sizeof(float) * mem[i].c_len));
        if (mem[i].cp_host) SVA_TRY(mem[i].Cp.get(mem[i].cp_host, 2 * mem[i].cp_elems));
        if (mem[i].ap_host) SVA_TRY(mem[i].Ap.get(mem[i].ap_host, 2 * mem[i].ap_elems));
    }
    if (rc == 1) return 1;
    if (repeat) {               // the same launch again from the same initial C: a K split's counters re-armed, the same summation order
        for (int i = 0; i < n; ++i) {
            SVA_HIP(hipMemcpy(mem[i].C.p, mem[i].c0.data(), sizeof(float) * mem[i].c_len, hipMemcpyHostToDevice));
            if (mem[i].cp_host) SVA_HIP(hipMemcpy(mem[i].Cp.p, mem[i].cp0.data(), 2 * mem[i].cp_elems, hipMemcpyHostToDevice));
        }
        SVA_TRY(run());
        bool same = true;
        for (int i = 0; i < n; ++i) {
            std::vector<float> c2(mem[i].c_len);
            SVA_TRY(mem[i].C.get(c2.data(), sizeof(float) * mem[i].c_len));
            same = same && memcmp(c2.data(), mem[i].c_host, sizeof(float) * mem[i].c_len) == 0;
            if (mem[i].cp_host) {
                std::vector<uint16_t> p2(mem[i].cp_elems);
                SVA_TRY(mem[i].Cp.get(p2.data(), 2 * mem[i].cp_elems));
                same = same && memcmp(p2.data(), mem[i].cp_host, 2 * mem[i].cp_elems) == 0;
            }
        }
        out[1] = same ? 1 : 0;
    }
    return 0;
}

// Read-only seam of the fast-path tests (include/sva.h): rows of the engine's fast-layer-0 table.  No kernel: one copy.
extern "C" int sva_test_fast_qkv0(sva_engine* e, int row0, int n, float* out) {
    SVA_CHECK(e && out, "sva_test_fast_qkv0: null argument");
    SVA_CHECK(e->fast_qkv0, "sva_test_fast_qkv0: this engine has no table (sizes the persistent decode kernel is not built for)");
    const sva_config& c = e->cfg;
    SVA_CHECK(n >= 1 && row0 >= 0 && n <= c.codebook_size && row0 <= c.codebook_size - n, "sva_test_fast_qkv0: rows outside the table");
    SVA_HIP(hipSetDevice(e->device));
    SVA_HIP(hipDeviceSynchronize());
    const size_t ld = (size_t)3 * c.ar_dim;
    SVA_HIP(hipMemcpy(out, e->fast_qkv0 + (size_t)row0 * ld, sizeof(float) * ld * n, hipMemcpyDeviceToHost));
    return 0;
}

// Read-only seam of the whole-frame tests (include/sva.h): rows pos0 .. pos0 + n - 1 of one slot's slow KV cache, every layer, as float
// out[layers][2 (k, v)][H][n][64].  An fp16 cache (ar_dtype = 1) is widened on the host, exactly.  No kernel: one strided copy per layer.
extern "C" int sva_test_kv_rows(sva_batch* b, int slot, int pos0, int n, float* out) {
    SVA_CHECK(b && out && b->kv_slow, "sva_test_kv_rows: null argument");
    const sva_config& c = b->e->cfg;
    const int S = c.max_seq_len, H = c.ar_heads;
    SVA_CHECK(slot >= 0 && slot < b->B, "sva_test_kv_rows: slot outside the batch");
    SVA_CHECK(n >= 1 && n <= S && pos0 >= 0 && pos0 <= S - n, "sva_test_kv_rows: rows outside the KV cache");
    SVA_HIP(hipSetDevice(b->e->device));
    std::vector<int> lp((size_t)b->B);
    if (sva_get_tap(b, "last_pos", lp.data(), (long)(sizeof(int) * lp.size())) < 0) return -2;      // drains the batch's streams
    const size_t esz = b->kv_half ? 2 : 4, per_layer = (size_t)2 * H * n * 64;
    std::vector<uint16_t> hb(b->kv_half ? per_layer : 0);
    for (int l = 0; l < c.ar_layers; ++l) {
        const size_t off = (size_t)l * b->kv_slow_layer + (size_t)slot * b->kv_slow_slot + (size_t)pos0 * 64;       // (k, v) x head = 2 H planes of S rows
        float* dst = out + (size_t)l * per_layer;
        SVA_HIP(hipMemcpy2D(b->kv_half ? (void*)hb.data() : (void*)dst, (size_t)n * 64 * esz, (const char*)b->kv_slow + off * esz, (size_t)S * 64 * esz,
                            (size_t)n * 64 * esz, (size_t)2 * H, hipMemcpyDeviceToHost));
        if (b->kv_half)
            for (size_t i = 0; i < per_layer; ++i) { _Float16 h; memcpy(&h, &hb[i], 2); dst[i] = (float)h; }
    }
    return 0;
}
