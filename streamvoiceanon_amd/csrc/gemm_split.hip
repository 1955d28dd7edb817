// fp32 conv-GEMM on the bf16 matrix pipes: every fp32 operand element is split into three bf16 parts (x = hi + mid + lo exactly:
// 3 x 8 significand bits) when its tile is staged in LDS, and each 16 x 16 x 32 block is the sum of the six part products whose
// weight is >= 2^-16 of the leading one (hi.hi, hi.mid, mid.hi, hi.lo, mid.mid, lo.hi) accumulated in fp32 by
// v_mfma_f32_16x16x32_bf16.  The three dropped products are below 2^-24 relative -- one fp32 rounding -- so the result is
// fp32-grade (measured on the encoder: max |du| 1.1e-6 against the exact fp32 formulation, BSQ indices identical;
// tools/bf16split_feasibility.py), while six 16-cycle MFMAs replace eight 32-cycle v_mfma_f32_16x16x4_f32 per 32 k: 2.7x less
// matrix-pipe time.  The ConvGemm contract (taps, SiLU prologue, groups; epilogue: gemm_epilogue.h).
//
// LDS: one buffer of 3 planes per operand, [rows][32 bf16] with a 96-byte row stride (16-byte fragment reads, the lanes of every
// ds_read_b128 lane group on distinct banks); global -> registers prefetch of the next K tile runs under the MFMAs; two workgroups per CU.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "sva_common.h"
#include "gemm_epilogue.h"

namespace sva {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// two fp32 -> packed (hi, mid, lo) bf16 pairs; RNE conversions (v_cvt_pk_bf16_f32), residuals exact in fp32
__device__ __forceinline__ void split2(float a, float b, unsigned& hi, unsigned& mid, unsigned& lo) {
    const f32x2 v = {a, b};
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    const f32x2 r1 = {a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u)};
    mid = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, bf16x2));
    const f32x2 r2 = {r1.x - __uint_as_float(mid << 16), r1.y - __uint_as_float(mid & 0xffff0000u)};
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2));
}

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void split_gemm_kernel(const ConvGemmGroup gg) {
    constexpr int NTH = 256, BK = 32;
    static_assert(WM * WN == 4, "4 waves");
    const ConvGemm& g = gg.g[blockIdx.z];
    constexpr int TM = BM / WM, TN = BN / WN;
    constexpr int MI = TM / 16, NI = TN / 16;
    constexpr int RS = 48;                        // row stride in bf16 elements (96 bytes = 24 dwords: the 16 lanes of every ds_read_b128
                                                  // lane group -- rows {0-3,12-15} with k offset 0 and rows 4-11 with k offset 8, etc. -- land on 64 distinct banks)
    constexpr int F4R = BK / 4;                   // float4 per tile row (8)
    constexpr int RPP = NTH / F4R;                // rows covered per pass (32)
    constexpr int A_LD = BM / RPP, B_LD = BN / RPP;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned short* Ap = reinterpret_cast<unsigned short*>(smem);                  // [3][BM][RS]
    unsigned short* Bp = Ap + 3 * BM * RS;                                         // [3][BN][RS]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    int tbx = blockIdx.x, tby = blockIdx.y;
    xcd_tile(gg.xcd_swz, gridDim.x, gridDim.y, tbx, tby);
    const int bm0 = tby * BM, bn0 = tbx * BN;
    const int kq = tid % F4R;
    const int lrow = tid / F4R;

    const float* a_ptr[A_LD];
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
        int m = bm0 + lrow + i * RPP;
        if (m > g.M - 1) m = g.M - 1;
        const int b = m / g.T, t = m - b * g.T;
        a_ptr[i] = g.A + (long)b * g.a_bstride + g.a_off + (long)t * g.stride * g.lda + kq * 4;
    }
    const float* b_ptr[B_LD];
    const long Kt = (long)g.taps * g.Cin;
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
        int n = bn0 + lrow + i * RPP;
        if (n > g.N - 1) n = g.N - 1;
        b_ptr[i] = g.W + (long)n * Kt + kq * 4;
    }

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int kc_tiles = g.Cin / BK;
    const int nk = g.taps * kc_tiles;
    f32x4 ra[A_LD], rb[B_LD];

    auto gload = [&](int kt) {
        const int tap = kt / kc_tiles;
        const int kc = (kt - tap * kc_tiles) * BK;
        const long aoff = (long)tap * g.dil * g.lda + kc;
        const long boff = (long)tap * g.Cin + kc;
#pragma unroll
        for (int i = 0; i < A_LD; ++i) ra[i] = *reinterpret_cast<const f32x4*>(a_ptr[i] + aoff);
#pragma unroll
        for (int i = 0; i < B_LD; ++i) rb[i] = *reinterpret_cast<const f32x4*>(b_ptr[i] + boff);
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            f32x4 v = ra[i];
            if (g.a_silu) v = epi::silu_of(v);
            unsigned h0, m0, l0, h1, m1, l1;
            split2(v.x, v.y, h0, m0, l0);
            split2(v.z, v.w, h1, m1, l1);
            unsigned short* d = Ap + (lrow + i * RPP) * RS + kq * 4;
            *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
            *reinterpret_cast<uint2*>(d + BM * RS) = make_uint2(m0, m1);
            *reinterpret_cast<uint2*>(d + 2 * BM * RS) = make_uint2(l0, l1);
        }
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            const f32x4 v = rb[i];
            unsigned h0, m0, l0, h1, m1, l1;
            split2(v.x, v.y, h0, m0, l0);
            split2(v.z, v.w, h1, m1, l1);
            unsigned short* d = Bp + (lrow + i * RPP) * RS + kq * 4;
            *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
            *reinterpret_cast<uint2*>(d + BN * RS) = make_uint2(m0, m1);
            *reinterpret_cast<uint2*>(d + 2 * BN * RS) = make_uint2(l0, l1);
        }
    };

    gload(0);
    const int fr = lane & 15, fk = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        lstore();
        __syncthreads();
        if (kt + 1 < nk) gload(kt + 1);            // in flight under the MFMAs of this tile
        // lane (fr, fk) supplies k = 8 fk .. 8 fk + 7 of row fr: the same rule on both operands
        const unsigned short* Ab = Ap + (wm * TM + fr) * RS + fk * 8;
        const unsigned short* Bb = Bp + (wn * TN + fr) * RS + fk * 8;
        bf16x8 ah[MI], am[MI], al[MI];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            ah[i] = *reinterpret_cast<const bf16x8*>(Ab + i * 16 * RS);
            am[i] = *reinterpret_cast<const bf16x8*>(Ab + i * 16 * RS + BM * RS);
            al[i] = *reinterpret_cast<const bf16x8*>(Ab + i * 16 * RS + 2 * BM * RS);
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const bf16x8 bh = *reinterpret_cast<const bf16x8*>(Bb + j * 16 * RS);
            const bf16x8 bm = *reinterpret_cast<const bf16x8*>(Bb + j * 16 * RS + BN * RS);
            const bf16x8 bl = *reinterpret_cast<const bf16x8*>(Bb + j * 16 * RS + 2 * BN * RS);
            // small products first
#pragma unroll
            for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[i], bm, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[i], bh, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bm, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh, acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // ---- epilogue: staged through LDS (gemm_epilogue.h); the last loop iteration ended with a barrier, so the A/B buffers are free to reuse ----
    epi::tile_epilogue<BM, BN, NTH>(g, smem, acc, true, wm * TM, wn * TN, bm0, bn0, [](float x) { return x; }, [](int) { return 1.f; }, epi::Store16{g.C});
}

// Wave-specialised form (512 threads): waves 0..3 are CONSUMERS (fragment reads + MFMAs, 64 x 64 each of a 128 x 128 tile), waves
// 4..7 are PRODUCERS (global loads, the hi/mid/lo split on the VALU, LDS stores into the other buffer).  One producer and one
// consumer wave share each SIMD, so the split arithmetic and the LDS writes run under the matrix pipe without relying on
// instruction scheduling inside one wave; LDS is double-buffered, one barrier per K tile.
template <int BM, int BN>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void split_ws_kernel(const ConvGemmGroup gg) {
    constexpr int NTH = 512, BK = 32, WM = 2, WN = 2;
    const ConvGemm& g = gg.g[blockIdx.z];
    constexpr int TM = BM / WM, TN = BN / WN;
    constexpr int MI = TM / 16, NI = TN / 16;
    constexpr int RS = 48;
    constexpr int F4R = BK / 4;
    constexpr int RPP = 256 / F4R;                // rows covered per pass of the 256 producer threads
    constexpr int A_LD = BM / RPP, B_LD = BN / RPP;
    constexpr int PLANE_A = BM * RS, PLANE_B = BN * RS, BUF = 3 * (PLANE_A + PLANE_B);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned short* lds = reinterpret_cast<unsigned short*>(smem);                 // [2][ A: 3 planes | B: 3 planes ]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const bool producer = wave >= 4;
    const int cw = wave & 3;
    const int wm = cw / WN, wn = cw % WN;
    int tbx = blockIdx.x, tby = blockIdx.y;
    xcd_tile(gg.xcd_swz, gridDim.x, gridDim.y, tbx, tby);
    const int bm0 = tby * BM, bn0 = tbx * BN;
    const int ptid = tid & 255;
    const int kq = ptid % F4R;
    const int lrow = ptid / F4R;
    const int kc_tiles = g.Cin / BK;
    const int nk = g.taps * kc_tiles;

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (producer) {
        const float* a_ptr[A_LD];
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            int m = bm0 + lrow + i * RPP;
            if (m > g.M - 1) m = g.M - 1;
            const int b = m / g.T, t = m - b * g.T;
            a_ptr[i] = g.A + (long)b * g.a_bstride + g.a_off + (long)t * g.stride * g.lda + kq * 4;
        }
        const float* b_ptr[B_LD];
        const long Kt = (long)g.taps * g.Cin;
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            int n = bn0 + lrow + i * RPP;
            if (n > g.N - 1) n = g.N - 1;
            b_ptr[i] = g.W + (long)n * Kt + kq * 4;
        }
        // two register sets: the tile stored in iteration kt was requested two iterations earlier (the A operand streams from HBM:
        // one K tile of MFMAs is shorter than its latency under load)
        f32x4 ra[2][A_LD], rb[2][B_LD];
        auto gload = [&](int kt, f32x4 (&xa)[A_LD], f32x4 (&xb)[B_LD]) {
            const int tap = kt / kc_tiles;
            const int kc = (kt - tap * kc_tiles) * BK;
            const long aoff = (long)tap * g.dil * g.lda + kc;
            const long boff = (long)tap * g.Cin + kc;
#pragma unroll
            for (int i = 0; i < A_LD; ++i) xa[i] = *reinterpret_cast<const f32x4*>(a_ptr[i] + aoff);
#pragma unroll
            for (int i = 0; i < B_LD; ++i) xb[i] = *reinterpret_cast<const f32x4*>(b_ptr[i] + boff);
        };
        auto lstore = [&](int buf, const f32x4 (&xa)[A_LD], const f32x4 (&xb)[B_LD]) {
            unsigned short* Ap = lds + buf * BUF;
            unsigned short* Bp = Ap + 3 * PLANE_A;
#pragma unroll
            for (int i = 0; i < A_LD; ++i) {
                f32x4 v = xa[i];
                if (g.a_silu) v = epi::silu_of(v);
                unsigned h0, m0, l0, h1, m1, l1;
                split2(v.x, v.y, h0, m0, l0);
                split2(v.z, v.w, h1, m1, l1);
                unsigned short* d = Ap + (lrow + i * RPP) * RS + kq * 4;
                *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
                *reinterpret_cast<uint2*>(d + PLANE_A) = make_uint2(m0, m1);
                *reinterpret_cast<uint2*>(d + 2 * PLANE_A) = make_uint2(l0, l1);
            }
#pragma unroll
            for (int i = 0; i < B_LD; ++i) {
                const f32x4 v = xb[i];
                unsigned h0, m0, l0, h1, m1, l1;
                split2(v.x, v.y, h0, m0, l0);
                split2(v.z, v.w, h1, m1, l1);
                unsigned short* d = Bp + (lrow + i * RPP) * RS + kq * 4;
                *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
                *reinterpret_cast<uint2*>(d + PLANE_B) = make_uint2(m0, m1);
                *reinterpret_cast<uint2*>(d + 2 * PLANE_B) = make_uint2(l0, l1);
            }
        };
        gload(0, ra[0], rb[0]);
        if (nk > 1) gload(1, ra[1], rb[1]);
        lstore(0, ra[0], rb[0]);
        if (nk > 2) gload(2, ra[0], rb[0]);
        __syncthreads();
        // iteration kt stores tile kt + 1 (set (kt + 1) & 1) and requests tile kt + 3 into the set it just freed
        for (int kt = 0; kt < nk; kt += 2) {
            if (kt + 1 < nk) {
                lstore(1, ra[1], rb[1]);
                if (kt + 3 < nk) gload(kt + 3, ra[1], rb[1]);
            }
            __syncthreads();
            if (kt + 1 < nk) {
                if (kt + 2 < nk) {
                    lstore(0, ra[0], rb[0]);
                    if (kt + 4 < nk) gload(kt + 4, ra[0], rb[0]);
                }
                __syncthreads();
            }
        }
    } else {
        const int fr = lane & 15, fk = lane >> 4;
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const unsigned short* Ap = lds + (kt & 1) * BUF;
            const unsigned short* Bp = Ap + 3 * PLANE_A;
            const unsigned short* Ab = Ap + (wm * TM + fr) * RS + fk * 8;
            const unsigned short* Bb = Bp + (wn * TN + fr) * RS + fk * 8;
            bf16x8 ah[MI], am[MI], al[MI], bh[NI], bm[NI], bl[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                ah[i] = *reinterpret_cast<const bf16x8*>(Ab + i * 16 * RS);
                am[i] = *reinterpret_cast<const bf16x8*>(Ab + i * 16 * RS + PLANE_A);
                al[i] = *reinterpret_cast<const bf16x8*>(Ab + i * 16 * RS + 2 * PLANE_A);
            }
#pragma unroll
            for (int j = 0; j < NI; ++j) {       // every fragment of the K tile is requested before the first MFMA (256 VGPRs per wave)
                bh[j] = *reinterpret_cast<const bf16x8*>(Bb + j * 16 * RS);
                bm[j] = *reinterpret_cast<const bf16x8*>(Bb + j * 16 * RS + PLANE_B);
                bl[j] = *reinterpret_cast<const bf16x8*>(Bb + j * 16 * RS + 2 * PLANE_B);
            }
#pragma unroll
            for (int j = 0; j < NI; ++j) {
#pragma unroll
                for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[i], bm[j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bm[j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
            }
            __syncthreads();
        }
    }

    // ---- epilogue: the consumer waves stage their accumulators, all 512 threads store (gemm_epilogue.h) ----
    epi::tile_epilogue<BM, BN, NTH>(g, smem, acc, !producer, wm * TM, wn * TN, bm0, bn0, [](float x) { return x; }, [](int) { return 1.f; }, epi::Store16{g.C});
}

template <int BM, int BN>
int launch_split_ws(const ConvGemmGroup& gg_in, hipStream_t st) {
    ConvGemmGroup gg = gg_in;
    const ConvGemm& g = gg.g[0];
    constexpr size_t smem_ab = (size_t)2 * 3 * (BM + BN) * 48 * sizeof(unsigned short);
    constexpr size_t smem_c = (size_t)BM * (BN + 4) * sizeof(float);
    constexpr size_t smem = smem_ab > smem_c ? smem_ab : smem_c;
    static DeviceOnce attr_set;
    SVA_TRY_RC(attr_set.max_dynamic_lds((const void*)split_ws_kernel<BM, BN>, smem));
    dim3 grid((g.N + BN - 1) / BN, (g.M + BM - 1) / BM, gg.n);
    gg.xcd_swz = xcd_swizzle_for(grid.x, grid.y);
    hipLaunchKernelGGL((split_ws_kernel<BM, BN>), grid, dim3(512), smem, st, gg);
    return 0;
}

template <int BM, int BN, int WM, int WN>
int launch_split_t(const ConvGemmGroup& gg_in, hipStream_t st) {
    ConvGemmGroup gg = gg_in;
    const ConvGemm& g = gg.g[0];
    constexpr size_t smem_ab = (size_t)3 * (BM + BN) * 48 * sizeof(unsigned short);
    constexpr size_t smem_c = (size_t)BM * (BN + 4) * sizeof(float);
    constexpr size_t smem = smem_ab > smem_c ? smem_ab : smem_c;
    static DeviceOnce attr_set;
    if (smem > 48 * 1024) SVA_TRY_RC(attr_set.max_dynamic_lds((const void*)split_gemm_kernel<BM, BN, WM, WN>, smem));
    dim3 grid((g.N + BN - 1) / BN, (g.M + BM - 1) / BM, gg.n);
    gg.xcd_swz = xcd_swizzle_for(grid.x, grid.y);
    hipLaunchKernelGGL((split_gemm_kernel<BM, BN, WM, WN>), grid, dim3(256), smem, st, gg);
    return 0;
}

}  // namespace

// the tiled epilogue's conditions (16-byte aligned C rows) are the caller's; here: channels in whole 32-wide K tiles
bool split_gemm_supported(const ConvGemm& g) { return g.Cin % 32 == 0 && g.stride >= 1 && !g.rms_w && !g.dw_wT; }

// variant: 0 = 128x128, 1 = 128x64, 2 = 64x128, 3 = 64x64 (one wave group does everything, two workgroups per CU);
// 4 = 128x128 wave-specialised (producer / consumer waves, 512 threads, double-buffered LDS)
int launch_split_gemm(const ConvGemmGroup& gg, int variant, hipStream_t st) {
    SVA_CHECK(split_gemm_supported(gg.g[0]), "split_gemm: unsupported problem");
    switch (variant) {
        case 4: return launch_split_ws<128, 128>(gg, st);
        case 0: return launch_split_t<128, 128, 2, 2>(gg, st);
        case 1: return launch_split_t<128, 64, 2, 2>(gg, st);
        case 2: return launch_split_t<64, 128, 2, 2>(gg, st);
        case 3: return launch_split_t<64, 64, 2, 2>(gg, st);
    }
    set_error("split_gemm: bad variant");
    return -1;
}

}  // namespace sva
