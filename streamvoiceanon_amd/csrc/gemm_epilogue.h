// The conv-GEMM epilogue contract (ConvGemm, sva_common.h) as device code, written once for every GEMM family:
//     value = (act(acc + bias) * gamma + residual) * scale (+ old C);  SwiGLU: C[., n / 2] = silu(w1 column) * (w3 column);
//     output rows t of a batch item in [skip_lo, skip_hi) are computed but not stored.
// A kernel supplies its accumulators, how it gets at its operands (loaded at the point of use or requested earlier) and how it stores;
// the order of the stages, the activations and the row addressing live here.  Everything is __forceinline__ and the functors handed in
// are lambdas: the library holds no device-function call (two-build audit).
// (ar_device.h has a silu_f of its own on expf for the persistent decode kernels: another function, hence the namespace.)
#pragma once
#include "sva_common.h"

namespace sva {
namespace epi {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float silu(float x) { return x / (1.f + __expf(-x)); }
__device__ __forceinline__ float gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float logclamp(float x) { return __logf(fmaxf(x, 1e-5f)); }

// f applied to a scalar, or to the four components of a float4 / f32x4
template <class F>
__device__ __forceinline__ float map(F f, float v) { return f(v); }
template <class F, class V4>
__device__ __forceinline__ V4 map(F f, V4 v) {
    v.x = f(v.x); v.y = f(v.y); v.z = f(v.z); v.w = f(v.w);
    return v;
}
template <class T>
__device__ __forceinline__ T silu_of(T v) { return map([](float x) { return silu(x); }, v); }
// the activation switch (ActKind)
template <class T>
__device__ __forceinline__ T act(int kind, T v) {
    if (kind == ACT_GELU) v = map([](float x) { return gelu(x); }, v);
    else if (kind == ACT_LOGCLAMP) v = map([](float x) { return logclamp(x); }, v);
    return v;
}
template <class T>
__device__ __forceinline__ T swiglu(T gate, T up) { return silu_of(gate) * up; }

// The stages after the accumulator, over operand VALUES: each operand is a flag and a functor that yields it, so a kernel either loads
// it where it is used (flag = the pointer is set) or hands over what it requested before its K loop (flag = true, neutral defaults:
// bias 0, gamma 1 -- the two choices differ in the sign of a zero and stay each kernel's own).
// STRICT: no implicit contraction, for the weight-streaming kernels (`#pragma clang fp contract(off)` is lexical: it does not reach
// code inlined from here, and the other kernels must keep the contraction they are compiled with) -- hence one text, two bodies.
#define SVA_EPI_STAGES                \
    if (has_bias) v += bias();        \
    v = act(act_kind, v);             \
    if (has_gamma) v *= gamma();      \
    if (has_res) v += res();          \
    v *= scale;                       \
    if (accumulate) v += old();
template <bool STRICT, class T, class FB, class FG, class FR, class FC>
__device__ __forceinline__ T value(T v, int act_kind, float scale, bool has_bias, FB bias, bool has_gamma, FG gamma, bool has_res, FR res,
                                   bool accumulate, FC old) {
    if constexpr (STRICT) {
#pragma clang fp contract(off)
        SVA_EPI_STAGES
    } else {
        SVA_EPI_STAGES
    }
    return v;
}
#undef SVA_EPI_STAGES

// Row addressing.  G: ConvGemm or a kernel's slim copy of it.  m -> (b, t); false for a row that is not stored
template <class G>
__device__ __forceinline__ bool stored_row(const G& g, int b, int t) { return !(t >= g.skip_lo && t < g.skip_hi); }
template <class G>
__device__ __forceinline__ bool out_row(const G& g, int m, int& b, int& t) {
    if (m >= g.M) return false;
    b = m / g.T; t = m - b * g.T;
    return stored_row(g, b, t);
}
// the same from the (b0, t0) of a tile's first row, without a division per row (a tile rarely spans more than two batch items)
template <class G>
__device__ __forceinline__ bool out_row_from(const G& g, int b0, int t0, int row, int m, int& b, int& t) {
    if (m >= g.M) return false;
    b = b0; t = t0 + row;
    if (t >= g.T) { t -= g.T; ++b; if (t >= g.T) { b += t / g.T; t %= g.T; } }
    return stored_row(g, b, t);
}
// element offset of column 0 of row (b, t) in C / in the residual
template <class G>
__device__ __forceinline__ long c_row(const G& g, int b, int t) { return (long)b * g.c_bstride + g.c_off + (long)t * g.ldc; }
template <class G>
__device__ __forceinline__ long r_row(const G& g, int b, int t) { return (long)b * g.r_bstride + g.r_off + (long)t * g.ldr; }

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// ---- the LDS-staged epilogue of a BM x BN workgroup tile (NTH threads) ----
// The accumulators (C/D layout of the 16x16 MFMA: col = lane & 15, row = (lane >> 4) * 4 + reg) are staged through LDS so that bias /
// residual reads and the C stores are whole 16-byte, row-contiguous accesses (a lane-per-element epilogue touches a 64-byte segment per
// row per instruction and costs up to 30 % of a K = 512 GEMM).  The caller's K loop ended with a barrier: its buffers are free.
//   Cs          [BM][BN + 4] floats
//   stages      this wave holds accumulators (false: the producer waves of a wave-specialised kernel); its tile starts at (wrow0, wcol0)
//   pre(x)      applied to an accumulator element on its way to LDS (the planes kernels' 2^-e)
//   row_scale(row)  factor of a tile row, read after the barrier (the ring kernel's fused RMSNorm; [](int) { return 1.f; } folds away)
//   store(v, idx, b, t, n)  four consecutive outputs of row (b, t) from column n, idx = their element offset in C
struct Store16 {
    float* C;
    __device__ __forceinline__ void operator()(const f32x4& v, long idx, int, int, int) const { *reinterpret_cast<f32x4*>(C + idx) = v; }
};
template <int BM, int BN, int NTH, int MI, int NI, class Pre, class RowScale, class Store>
__device__ __forceinline__ void tile_epilogue(const ConvGemm& g, float* Cs, const f32x4 (&acc)[MI][NI], bool stages, int wrow0, int wcol0,
                                              int bm0, int bn0, Pre pre, RowScale row_scale, Store store) {
    constexpr int CS = BN + 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int col = lane & 15, rq = (lane >> 4) * 4;
    if (stages) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) Cs[(wrow0 + i * 16 + rq + r) * CS + wcol0 + j * 16 + col] = pre(acc[i][j][r]);
    }
    __syncthreads();
    const int b0 = bm0 / g.T, t0 = bm0 - b0 * g.T;              // one division per workgroup
    if (g.w13) {
        // SwiGLU: tile columns alternate 16 x w1 | 16 x w3; output column (n0 >> 1) + c
        constexpr int OC4 = BN / 8;                // float4 chunks of output per row
        for (int idx = tid; idx < BM * OC4; idx += NTH) {
            const int row = idx / OC4, q = idx - row * OC4;
            const int grp = q >> 2, c4 = (q & 3) * 4;       // 16-wide group, offset inside it
            const int n = bn0 + grp * 32 + c4;              // w1 column
            int b, t;
            if (n >= g.N || !out_row_from(g, b0, t0, row, bm0 + row, b, t)) continue;
            const float inv = row_scale(row);
            const f32x4 o = swiglu(ld4(&Cs[row * CS + grp * 32 + c4]) * inv, ld4(&Cs[row * CS + grp * 32 + 16 + c4]) * inv);
            const int nc = ((bn0 + grp * 32) >> 1) + c4;
            store(o, c_row(g, b, t) + nc, b, t, nc);
        }
        return;
    }
    constexpr int C4 = BN / 4;
    for (int idx = tid; idx < BM * C4; idx += NTH) {
        const int row = idx / C4, c4 = (idx - row * C4) * 4;
        const int n = bn0 + c4;
        int b, t;
        if (n >= g.N || !out_row_from(g, b0, t0, row, bm0 + row, b, t)) continue;
        const long ci = c_row(g, b, t) + n;
        const f32x4 v = value<false>(ld4(&Cs[row * CS + c4]) * row_scale(row), g.act, g.scale,
                                     g.bias != nullptr, [&] { return ld4(g.bias + n); }, g.gamma != nullptr, [&] { return ld4(g.gamma + n); },
                                     g.res != nullptr, [&] { return ld4(g.res + r_row(g, b, t) + n); }, g.accumulate != 0, [&] { return ld4(g.C + ci); });
        store(v, ci, b, t, n);
    }
}

}  // namespace epi
}  // namespace sva
