// f32 MFMA conv-GEMM for gfx950 (v_mfma_f32_16x16x4_f32: exact f32, 32-cycle issue).
//
// Why f32 MFMA: BSQ content codes must be bit-exact against the fp32 reference
// (SURVEY.md §7 hard part 2), so the encoder cannot use fp16/bf16 matrix cores; the f32-input
// MFMA is bitwise an fmaf chain at the f32 vector peak (157 TF) with one VGPR per operand.
//
// Tiling: 256 threads = 4 waves in a WM x WN grid, block tile BM x BN, BK = 16.  A and W tiles
// are staged global -> registers -> LDS (k-major, row stride +16 floats so the two k-rows a
// 32-lane ds_read_b32 group touches fall on disjoint bank halves) and double-buffered: the
// next tile's global loads are issued before the current tile's MFMAs and written to the other
// LDS buffer after them (one barrier per K tile).
#include "sva_common.h"
#include "gemm_epilogue.h"
#include "gemm_stream_common.h"
#include <mutex>
#include <unordered_map>

namespace sva {

constexpr int KS_ERR_WORD = (1 << 16) - 1;      // last word of a stream's split-K arrival counters: set when a partial never arrived

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int BM, int BN, int WM, int WN, int BK>
__global__ __launch_bounds__(64 * WM * WN) void conv_gemm_kernel(const ConvGemmGroup gg) {
    constexpr int NTH = 64 * WM * WN;             // 4 or 8 waves
    const ConvGemm& g = gg.g[blockIdx.z];
    constexpr int TM = BM / WM, TN = BN / WN;     // wave tile
    constexpr int MI = TM / 16, NI = TN / 16;
    constexpr int LS = BK + 4;                    // LDS row stride: 16-byte aligned rows; row*LS mod 64 banks is a permutation of
                                                  // the multiples of 4 over 16 rows, so the ds_read_b128 fragments are conflict-free
    constexpr int F4R = BK / 4;                   // float4 per tile row
    constexpr int RPP = NTH / F4R;                // rows covered per pass of the workgroup's threads
    constexpr int A_LD = (BM + RPP - 1) / RPP;
    constexpr int B_LD = (BN + RPP - 1) / RPP;
    static_assert(WM * WN == 4 || WM * WN == 8, "4 or 8 waves");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                             // [2][BM][LS]
    float* Bs = smem + 2 * BM * LS;               // [2][BN][LS]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    int tbx = blockIdx.x, tby = blockIdx.y;
    xcd_tile(gg.xcd_swz, gridDim.x, gridDim.y, tbx, tby);
    const int bm0 = tby * BM, bn0 = tbx * BN;
    const int kq = tid % F4R;                     // which float4 of the BK-wide k tile
    const int lrow = tid / F4R;

    const float* a_ptr[A_LD];
    bool a_on[A_LD];
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
        int r = lrow + i * RPP;
        a_on[i] = r < BM;
        int m = bm0 + r;
        if (m > g.M - 1) m = g.M - 1;
        int b = m / g.T, t = m - b * g.T;
        a_ptr[i] = g.A + (long)b * g.a_bstride + g.a_off + (long)t * g.stride * g.lda + kq * 4;
    }
    const float* b_ptr[B_LD];
    bool b_on[B_LD];
    const long Kt = (long)g.taps * g.Cin;
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
        int r = lrow + i * RPP;
        b_on[i] = r < BN;
        int n = bn0 + r;
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
    float4 ra[A_LD], rb[B_LD];

    auto gload = [&](int kt) {
        int tap = kt / kc_tiles;
        int kc = (kt - tap * kc_tiles) * BK;
        long aoff = (long)tap * g.dil * g.lda + kc;
        long boff = (long)tap * g.Cin + kc;
#pragma unroll
        for (int i = 0; i < A_LD; ++i)
            if (a_on[i]) ra[i] = *reinterpret_cast<const float4*>(a_ptr[i] + aoff);
#pragma unroll
        for (int i = 0; i < B_LD; ++i)
            if (b_on[i]) rb[i] = *reinterpret_cast<const float4*>(b_ptr[i] + boff);
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_LD; ++i)
            if (a_on[i]) {
                float4 v = ra[i];
                if (g.a_silu) v = epi::silu_of(v);
                *reinterpret_cast<float4*>(As + ((buf * BM + lrow + i * RPP) * LS + kq * 4)) = v;
            }
#pragma unroll
        for (int i = 0; i < B_LD; ++i)
            if (b_on[i]) {
                float4 v = rb[i];
                *reinterpret_cast<float4*>(Bs + ((buf * BN + lrow + i * RPP) * LS + kq * 4)) = v;
            }
    };

    gload(0);
    lstore(0);
    __syncthreads();
    const int fr = lane & 15, fk = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) gload(kt + 1);
        // One ds_read_b128 per fragment and 16 k: lane (fr, fk) supplies k = 16*blk + 4*fk + j to MFMA step j of the block --
        // a permutation of k inside the block, identical on both operands (same trick as the small-M kernel).
        const float* Ab = As + (buf * BM + wm * TM + fr) * LS + fk * 4;
        const float* Bb = Bs + (buf * BN + wn * TN + fr) * LS + fk * 4;
#pragma unroll
        for (int ks = 0; ks < BK; ks += 16) {
            float4 af[MI], bf[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) af[i] = *reinterpret_cast<const float4*>(Ab + i * 16 * LS + ks);
#pragma unroll
            for (int j = 0; j < NI; ++j) bf[j] = *reinterpret_cast<const float4*>(Bb + j * 16 * LS + ks);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) lstore(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue: staged through LDS (gemm_epilogue.h); the last loop iteration ended with a barrier, so the A/B buffers are free to reuse ----
    epi::tile_epilogue<BM, BN, NTH>(g, smem, acc, true, wm * TM, wn * TN, bm0, bn0, [](float x) { return x; }, [](int) { return 1.f; }, epi::Store16{g.C});
}

// ------------------------------------------------------------------------------------------
// small-M ("skinny") path: M <= 64 rows -- the AR decode GEMMs (M = 2B / B tokens) and the streaming
// vocoder's first levels.  These are weight-streaming problems: the tiled kernel above would run a
// handful of workgroups through a long serial K loop (one 16-wide tile in flight per barrier) and sit on
// HBM/L2 latency.  Here a workgroup owns 16*NT output columns and ALL rows; its KW waves split the K axis
// (interleaved 16-wide blocks), every lane streams one float4 of W and one float4 of A per block straight
// from global memory into the MFMA operands (no LDS, no barrier in the loop, loads software-pipelined by
// unrolling), and the KW partial accumulators are reduced through LDS once at the end.
// Operand mapping: lane l supplies, for MFMA step j of a block, W[n0 + (l&15)][k0 + 4*(l>>4) + j] and
// A[m0 + (l&15)][k0 + 4*(l>>4) + j] -- a permutation of k inside the block, identical on both operands.
// ------------------------------------------------------------------------------------------
// AOP: what happens to A on load -- 0 nothing, 1 SiLU (HiFiGAN), 2 RMSNorm of the row (weight folded into the operand,
// row statistics accumulated on the fly and applied to the accumulators in the epilogue).
template <int MT, int NT, int KW, int D, int AOP>
__global__ __launch_bounds__(64 * KW) void skinny_gemm_kernel(const ConvGemmGroup gg) {
    // blockIdx.z: member of a group, or (single problem) the K split this workgroup owns
    const ConvGemm& g = gg.g[gg.n > 1 ? blockIdx.z : 0];
    const int Z = gg.n > 1 ? 1 : g.ksplit, ks = gg.n > 1 ? 0 : (int)blockIdx.z;
    constexpr bool SILU = AOP == 1, RMS = AOP == 2, DWLN = AOP == 3;
    extern __shared__ __attribute__((aligned(16))) float red[];      // [KW][MT*NT][64][4] (+ [KW][MT][16] row sums of squares)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * (16 * NT);
    const int m_base = blockIdx.y * (16 * MT);
    const int fr = lane & 15, fg = lane >> 4;
    const long Kt = (long)g.taps * g.Cin;
    const float* wp[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        int n = n0 + j * 16 + fr;
        if (n > g.N - 1) n = g.N - 1;
        wp[j] = g.W + (long)n * Kt + 4 * fg;
    }
    const float* ap[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        int m = m_base + i * 16 + fr;
        if (m > g.M - 1) m = g.M - 1;
        const int b = m / g.T, t = m - b * g.T;
        ap[i] = g.A + (long)b * g.a_bstride + g.a_off + (long)t * g.stride * g.lda + 4 * fg;
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // AOP 3: ConvNeXt prologue -- rows of this tile = LayerNorm(depthwise k7 conv) of x, one wave per row, kept in LDS with a
    // padded row stride (the K loop then reads its A fragments from there instead of from global memory)
    const int a_ld = g.Cin + 4;
    float* a_s = red + KW * MT * NT * 256;                 // [16*MT][Cin + 4]
    if constexpr (DWLN) {
        const int C = g.Cin;
        for (int r = wave; r < 16 * MT; r += KW) {
            const int m = m_base + r;
            float* dst = a_s + r * a_ld;
            if (m >= g.M) {
                for (int c = lane; c < C; c += 64) dst[c] = 0.f;
                continue;
            }
            const int b = m / g.T, t = m - b * g.T;
            const float* xr = g.A + (long)b * g.a_bstride + g.a_off + (long)t * g.lda;      // tap 0 row
            float v[8], sum = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = lane + 64 * i;
                float acc = 0.f;
                if (c < C) {
                    acc = g.dw_b[c];
#pragma unroll
                    for (int j = 0; j < 7; ++j) acc = fmaf(g.dw_wT[j * C + c], xr[(long)j * g.lda + c], acc);
                    sum += acc;
                }
                v[i] = acc;
            }
            sum += __shfl_xor(sum, 1, 64); sum += __shfl_xor(sum, 2, 64); sum += __shfl_xor(sum, 4, 64);
            sum += __shfl_xor(sum, 8, 64); sum += __shfl_xor(sum, 16, 64); sum += __shfl_xor(sum, 32, 64);
            const float mean = sum / (float)C;
            float q = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (lane + 64 * i < C) { const float d = v[i] - mean; q = fmaf(d, d, q); }
            q += __shfl_xor(q, 1, 64); q += __shfl_xor(q, 2, 64); q += __shfl_xor(q, 4, 64);
            q += __shfl_xor(q, 8, 64); q += __shfl_xor(q, 16, 64); q += __shfl_xor(q, 32, 64);
            const float inv = 1.f / sqrtf(q / (float)C + g.ln_eps);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = lane + 64 * i;
                if (c < C) dst[c] = (v[i] - mean) * inv * g.ln_w[c] + g.ln_b[c];
            }
        }
        __syncthreads();
    }
    const int kc_tiles = g.Cin / 16;
    const int nk = g.taps * kc_tiles;
    // software pipeline, D K-blocks in flight per wave.  No branch around any load (a conditional load makes
    // hipcc drain vmcnt(0) at the join): out-of-range blocks re-load the wave's last valid block and are masked.
    // this workgroup's share of the K blocks (grid-level split), interleaved over its waves
    const int kb_lo = (int)((long)ks * nk / Z), kb_hi = (int)((long)(ks + 1) * nk / Z);
    int my_n, last_kb;                                                           // K blocks owned by this wave
    wstream::wave_blocks<KW>(kb_lo, kb_hi, wave, my_n, last_kb);
    auto kbq = [&](int q) { return kb_lo + wave + q * KW; };
    float4 wv[D][NT], av[D][MT], nv[D];
    float ssq[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) ssq[i] = 0.f;
    auto issue = [&](float4 (&w)[NT], float4 (&a)[MT], float4& nw, int kb) {
        kb = kb < kb_hi ? kb : last_kb;
        const int tap = kb / kc_tiles;
        const int kc = (kb - tap * kc_tiles) * 16;
        const long aoff = (long)tap * g.dil * g.lda + kc;
        const long woff = (long)tap * g.Cin + kc;
#pragma unroll
        for (int j = 0; j < NT; ++j) w[j] = *reinterpret_cast<const float4*>(wp[j] + woff);
        if constexpr (DWLN) {            // A fragments come from the LDS tile written by the prologue (no latency to hide)
#pragma unroll
            for (int i = 0; i < MT; ++i) a[i] = *reinterpret_cast<const float4*>(a_s + (i * 16 + fr) * a_ld + kc + 4 * fg);
        } else {
#pragma unroll
            for (int i = 0; i < MT; ++i) a[i] = *reinterpret_cast<const float4*>(ap[i] + aoff);
        }
        if (RMS) nw = *reinterpret_cast<const float4*>(g.rms_w + kc + 4 * fg);
    };
#pragma unroll
    for (int d = 0; d < D; ++d) issue(wv[d], av[d], nv[d], kbq(d));
    for (int it = 0; it < my_n; it += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int kb = kbq(it + d);
            const float keep = kb < kb_hi ? 1.f : 0.f;
            float4 w[NT], a[MT];
#pragma unroll
            for (int j = 0; j < NT; ++j) w[j] = wv[d][j];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                a[i] = av[d][i];
                if (SILU) a[i] = epi::silu_of(a[i]);
                a[i].x *= keep; a[i].y *= keep; a[i].z *= keep; a[i].w *= keep;
                if (RMS) {
                    // explicit sequential fmas: under -ffp-contract the pairwise form was fused differently per unrolled row tile (gemm_stream.hip), so a row's statistic depended on its position
                    ssq[i] = __builtin_fmaf(a[i].x, a[i].x, ssq[i]);
                    ssq[i] = __builtin_fmaf(a[i].y, a[i].y, ssq[i]);
                    ssq[i] = __builtin_fmaf(a[i].z, a[i].z, ssq[i]);
                    ssq[i] = __builtin_fmaf(a[i].w, a[i].w, ssq[i]);
                    a[i].x *= nv[d].x; a[i].y *= nv[d].y; a[i].z *= nv[d].z; a[i].w *= nv[d].w;
                }
            }
            issue(wv[d], av[d], nv[d], kbq(it + d + D));
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, w[j].x, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, w[j].y, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, w[j].z, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, w[j].w, acc[i][j], 0, 0, 0);
        }
    }
    // cross-wave reduction of the K slices
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
            *reinterpret_cast<f32x4*>(&red[((wave * (MT * NT) + i * NT + j) * 64 + lane) * 4]) = acc[i][j];
    float* redss = red + KW * MT * NT * 256;                          // [KW][MT][16]
    if (RMS) {
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            float v = ssq[i];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (fg == 0) redss[(wave * MT + i) * 16 + fr] = v;
        }
    }
    __syncthreads();
    // tail: the MT row tiles are spread over the waves (each sums the KW partials of its tiles straight from LDS and runs
    // the epilogue for them) instead of leaving all of it to wave 0
    const int col = lane & 15, rq = (lane >> 4) * 4;
    auto epilogue = [&](int i, f32x4 (&t)[NT]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int b, tt;
            if (!epi::out_row(g, m_base + i * 16 + rq + r, b, tt)) continue;
            float* crow = g.C + epi::c_row(g, b, tt);
            const float* rrow = g.res ? g.res + epi::r_row(g, b, tt) : nullptr;
            if (g.w13) {
                if constexpr (NT % 2 == 0) {          // column tiles come in (gate, up) pairs
#pragma unroll
                    for (int jp = 0; jp < NT / 2; ++jp) {
                        const int n = n0 + jp * 32 + col;
                        if (n < g.N) crow[(n0 >> 1) + jp * 16 + col] = epi::swiglu(t[2 * jp][r], t[2 * jp + 1][r]);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const int n = n0 + j * 16 + col;
                    if (n >= g.N) continue;
                    crow[n] = epi::value<false>(t[j][r], g.act, g.scale, g.bias != nullptr, [&] { return g.bias[n]; }, g.gamma != nullptr, [&] { return g.gamma[n]; },
                                                rrow != nullptr, [&] { return rrow[n]; }, g.accumulate != 0, [&] { return crow[n]; });
                }
            }
        }
    };
    const int tile = blockIdx.y * gridDim.x + blockIdx.x, n_tiles = gridDim.x * gridDim.y;
    for (int i = wave; i < MT; i += KW) {
        f32x4 t[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            t[j] = wstream::tile_sum<MT, NT, KW, KW>(red, i, j, lane);
        }
        if (RMS) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float tot = 0.f;
#pragma unroll
                for (int w = 0; w < KW; ++w) tot += redss[(w * MT + i) * 16 + rq + r];
                const float inv = 1.f / sqrtf(tot / (float)Kt + g.rms_eps);
#pragma unroll
                for (int j = 0; j < NT; ++j) t[j][r] *= inv;
            }
        }
        if (Z == 1) {
            epilogue(i, t);
        } else {          // raw partial tile of this K split as self-validating granules {tag = 1, value} (register layout)
            unsigned long long* gw = reinterpret_cast<unsigned long long*>(g.ks_ws);
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    __hip_atomic_store(gw + ((((long)ks * n_tiles + tile) * MT + i) * NT + j) * 256 + e * 64 + lane,
                                       (1ull << 32) | (unsigned long long)__float_as_uint(t[j][e]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (Z == 1) return;
    // The last workgroup to arrive for this output tile sums the Z partials in split order (deterministic) and runs the epilogue.
    // Hand-off without fences (guide G16, form R2 -- as in ar_decode.hip): every datum is an 8-byte granule {tag, value} written
    // with one relaxed agent-scope atomic store, the reader polls each granule until its tag is set.  The arrival counter only
    // ELECTS the reader, it carries no visibility promise: a writer's granules may land after its counter increment, the poll
    // covers that.  The reader clears the tags it consumed (the next launch on this stream starts behind a kernel boundary).
    // An agent-scope release per writer -- what a counter-validated hand-off needs across XCDs -- cost more than the split won.
    __syncthreads();
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(g.ks_cnt + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == (unsigned)(Z - 1)) __hip_atomic_store(g.ks_cnt + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // re-armed for the next launch
        reinterpret_cast<unsigned*>(red)[0] = old;
    }
    __syncthreads();
    if (reinterpret_cast<const unsigned*>(red)[0] != (unsigned)(Z - 1)) return;
    unsigned long long* gw = reinterpret_cast<unsigned long long*>(g.ks_ws);
    for (int i = wave; i < MT; i += KW) {
        f32x4 t[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) t[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int z = 0; z < Z; ++z) {
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                unsigned long long* gp = gw + ((((long)z * n_tiles + tile) * MT + i) * NT + j) * 256 + lane;
                unsigned long long x[4];
                unsigned pending = 0xfu;
                for (int spin = 0; pending && spin < (1 << 20); ++spin) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (pending & (1u << e)) {
                            x[e] = __hip_atomic_load(gp + e * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if ((unsigned)(x[e] >> 32) == 1u) pending &= ~(1u << e);
                        }
                }
                // (every writer finished its stores before it took its arrival ticket, so the poll only bridges their flight time;
                // a partial that never shows up is a hardware / protocol fault: flag it -- sva_sync reports it -- and leave its tag alone)
                if (pending) __hip_atomic_store(g.ks_cnt + KS_ERR_WORD, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (pending & (1u << e)) continue;
                    t[j][e] += __uint_as_float((unsigned)x[e]);
                    __hip_atomic_store(gp + e * 64, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        epilogue(i, t);
    }
}

// split-K scratch (partial tiles + arrival counters), one per stream: launches on one stream are ordered, so they can
// share it; concurrent streams must not
struct KsScratch { float* ws = nullptr; unsigned* cnt = nullptr; };
static std::mutex g_ks_mu;
static std::unordered_map<hipStream_t, KsScratch> g_ks;
constexpr size_t KS_WS_FLOATS = (size_t)4 << 20;      // granules of partial tiles (8 bytes each: 32 MiB)
constexpr int KS_CNT = 1 << 16;
static_assert(KS_ERR_WORD == KS_CNT - 1, "error word = last counter");
// sva_sync: has any split-K reader on any stream of this process flagged a missing partial?
int conv_gemm_check_errors() {
    std::lock_guard<std::mutex> lk(g_ks_mu);
    for (auto& kv : g_ks) {
        if (!kv.second.cnt) continue;
        unsigned v = 0;
        SVA_HIP(hipMemcpy(&v, kv.second.cnt + KS_ERR_WORD, sizeof(unsigned), hipMemcpyDeviceToHost));
        if (v != 0) {
            // reported once (the word used to stay set, so every later sva_sync of every batch failed): the fault word and the
            // whole hand-off scratch of that stream are cleared -- a partial that arrives late must not be consumed as a stale tile
            SVA_HIP(hipDeviceSynchronize());
            SVA_HIP(hipMemset(kv.second.ws, 0, KS_WS_FLOATS * 8));
            SVA_HIP(hipMemset(kv.second.cnt, 0, KS_CNT * sizeof(unsigned)));
            SVA_CHECK(false, "split-K GEMM: a partial tile never arrived (hand-off fault); the results of the steps since the last sva_sync are invalid");
        }
    }
    return 0;
}
static int ks_scratch(hipStream_t st, KsScratch* out) {
    std::lock_guard<std::mutex> lk(g_ks_mu);
    auto it = g_ks.find(st);
    if (it != g_ks.end()) { *out = it->second; return 0; }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { *out = KsScratch(); return 0; }   // no allocation inside a capture
    KsScratch k;
    // UNCACHED device memory: partial tiles and counters bypass the (per-XCD, mutually incoherent) L2s, so the hand-off
    // needs no agent-scope fence -- an agent-scope release / acquire per workgroup writes back / invalidates the whole
    // L2 and serialises (measured: + 0.37 us per workgroup)
    SVA_HIP(hipExtMallocWithFlags((void**)&k.ws, KS_WS_FLOATS * 8, hipDeviceMallocUncached));
    SVA_HIP(hipMemset(k.ws, 0, KS_WS_FLOATS * 8));
    SVA_HIP(hipExtMallocWithFlags((void**)&k.cnt, KS_CNT * sizeof(unsigned), hipDeviceMallocUncached));
    SVA_HIP(hipMemset(k.cnt, 0, KS_CNT * sizeof(unsigned)));
    g_ks[st] = k;
    *out = k;
    return 0;
}

// split-K scratch of a stream, allocated ahead of time: a launch inside a stream capture cannot allocate and would silently fall
// back to an unsplit launch -- a different summation order from the eager launch of the same shape
int conv_gemm_prepare_stream(hipStream_t st) {
    KsScratch k;
    SVA_TRY_RC(ks_scratch(st, &k));
    return 0;
}

template <int MT, int NT, int KW, int D, int AOP>
static int launch_skinny_op(const ConvGemmGroup& gin, int z, hipStream_t st) {
    const ConvGemm& g = gin.g[0];
    const size_t smem = ((size_t)KW * MT * NT * 256 + (AOP == 2 ? KW * MT * 16 : 0) + (AOP == 3 ? (size_t)16 * MT * (g.Cin + 4) : 0)) * sizeof(float);
    ConvGemmGroup gg = gin;
    dim3 grid((g.N + 16 * NT - 1) / (16 * NT), (g.M + 16 * MT - 1) / (16 * MT), gg.n);
    if (gg.n == 1) {
        int Z = AOP == 2 ? 1 : z;                         // grid-level K split of the plan (the fused RMSNorm needs the whole row in one workgroup)
        const long nkb = (long)g.taps * g.Cin / 16;
        if (Z > nkb) Z = (int)nkb;
        const size_t tiles = (size_t)grid.x * grid.y;
        KsScratch k;
        if (Z > 1 && (tiles >= (size_t)KS_ERR_WORD || (size_t)Z * tiles * MT * NT * 256 > KS_WS_FLOATS)) Z = 1;
        if (Z > 1) { SVA_TRY_RC(ks_scratch(st, &k)); if (!k.ws) Z = 1; }
        gg.g[0].ksplit = Z; gg.g[0].ks_ws = k.ws; gg.g[0].ks_cnt = k.cnt;
        grid.z = Z;
    }
    static DeviceOnce attr;
    if (smem > 48 * 1024) SVA_TRY_RC(attr.max_dynamic_lds((const void*)skinny_gemm_kernel<MT, NT, KW, D, AOP>, 132 * 1024));
    hipLaunchKernelGGL((skinny_gemm_kernel<MT, NT, KW, D, AOP>), grid, dim3(64 * KW), smem, st, gg);
    return 0;
}
template <int MT, int NT, int KW, int D>
static int launch_skinny(const ConvGemmGroup& gg, int z, hipStream_t st) {
    const ConvGemm& g = gg.g[0];
    if (g.dw_wT) {
        if constexpr (MT == 1 && NT == 1) return launch_skinny_op<MT, NT, KW, D, 3>(gg, z, st);
        else { set_error("conv_gemm: the fused ConvNeXt prologue runs on one 16-row tile"); return -1; }
    }
    if (g.rms_w) return launch_skinny_op<MT, NT, KW, D, 2>(gg, z, st);
    if (g.a_silu) return launch_skinny_op<MT, NT, KW, D, 1>(gg, z, st);
    return launch_skinny_op<MT, NT, KW, D, 0>(gg, z, st);
}

#ifndef SVA_D18
#define SVA_D116 4
#define SVA_D18 6
#define SVA_D14 8
#define SVA_D28 4
#define SVA_D24 6
#define SVA_D48 3
#define SVA_D44 4
#endif
template <int NT>
static int launch_cfg(const ConvGemmGroup& gg, int mt, int kw, int z, hipStream_t st) {
    if constexpr (NT == 4) {      // 64-column workgroups: rows x K-split waves in {16, 32, 64} x {4, 8}
        switch (mt) {
            case 1: return kw == 8 ? launch_skinny<1, 4, 8, 4>(gg, z, st) : launch_skinny<1, 4, 4, 4>(gg, z, st);
            case 2: return kw == 8 ? launch_skinny<2, 4, 8, 3>(gg, z, st) : launch_skinny<2, 4, 4, 3>(gg, z, st);
            default: return kw == 8 ? launch_skinny<4, 4, 8, 2>(gg, z, st) : launch_skinny<4, 4, 4, 2>(gg, z, st);
        }
    }
    switch (mt) {
        case 1:
            if (kw == 16) return launch_skinny<1, NT, 16, SVA_D116>(gg, z, st);
            if (kw == 8) return launch_skinny<1, NT, 8, SVA_D18>(gg, z, st);
            return launch_skinny<1, NT, 4, SVA_D14>(gg, z, st);
        case 2:
            if (kw == 8) return launch_skinny<2, NT, 8, SVA_D28>(gg, z, st);
            return launch_skinny<2, NT, 4, SVA_D24>(gg, z, st);
        case 3:
            if (kw == 8) return launch_skinny<3, NT, 8, SVA_D28>(gg, z, st);
            return launch_skinny<3, NT, 4, SVA_D44>(gg, z, st);
        default:
            if (kw == 8) return launch_skinny<4, NT, 8, SVA_D48>(gg, z, st);
            return launch_skinny<4, NT, 4, SVA_D44>(gg, z, st);
    }
}

template <int BM, int BN, int WM, int WN, int BK>
static int launch_t(const ConvGemmGroup& gin, hipStream_t st) {
    const ConvGemm& g = gin.g[0];
    constexpr size_t smem_ab = (size_t)2 * (BM + BN) * (BK + 4) * sizeof(float);
    constexpr size_t smem_c = (size_t)BM * (BN + 4) * sizeof(float);          // epilogue staging tile reuses the buffers
    constexpr size_t smem = smem_ab > smem_c ? smem_ab : smem_c;
    static DeviceOnce attr_set;
    if (smem > 48 * 1024) SVA_TRY_RC(attr_set.max_dynamic_lds((const void*)conv_gemm_kernel<BM, BN, WM, WN, BK>, 160 * 1024));
    ConvGemmGroup gg = gin;
    dim3 grid((g.N + BN - 1) / BN, (g.M + BM - 1) / BM, gg.n);
    gg.xcd_swz = xcd_swizzle_for(grid.x, grid.y);
    hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, WM, WN, BK>), grid, dim3(64 * WM * WN), smem, st, gg);
    return 0;
}

// The two entry points of this file for the dispatcher (gemm_dispatch.hip); a single problem is a group of one.
// small-M kernel: mt = rows / 16 per workgroup, kw = K-split waves, nt = 16-column tiles per wave, z = grid-level K split
int launch_small_m_gemm(const ConvGemmGroup& gg, int mt, int kw, int nt, int z, hipStream_t st) {
    return nt == 4 ? launch_cfg<4>(gg, mt, kw, z, st) : nt == 2 ? launch_cfg<2>(gg, mt, kw, z, st) : launch_cfg<1>(gg, mt, kw, z, st);
}
// LDS-tiled kernel: variant 0 = 64x64, 1 = 128x128, 2 = 128x32, 3 = 256x16, 4 = 128x64, 5 = 64x128, 6 = 256x64, 7 = 256x128 on 8 waves (4..7 are
// reached through the autotuner only); the K tile is as deep as Cin allows
int launch_tiled_gemm(const ConvGemmGroup& gg, int variant, hipStream_t st) {
    const int Cin = gg.g[0].Cin;
    const int bk = Cin % 64 == 0 ? 64 : (Cin % 32 == 0 ? 32 : 16);
    switch (variant) {
        case 3: return launch_t<256, 16, 4, 1, 16>(gg, st);
        case 2: return bk >= 32 ? launch_t<128, 32, 4, 1, 32>(gg, st) : launch_t<128, 32, 4, 1, 16>(gg, st);
        case 1: return bk >= 32 ? launch_t<128, 128, 2, 2, 32>(gg, st) : launch_t<128, 128, 2, 2, 16>(gg, st);
        case 4: return bk >= 32 ? launch_t<128, 64, 2, 2, 32>(gg, st) : launch_t<128, 64, 2, 2, 16>(gg, st);
        case 5: return bk >= 32 ? launch_t<64, 128, 2, 2, 32>(gg, st) : launch_t<64, 128, 2, 2, 16>(gg, st);
        case 6: return bk >= 32 ? launch_t<256, 64, 4, 1, 32>(gg, st) : launch_t<256, 64, 4, 1, 16>(gg, st);
        case 7: return bk >= 32 ? launch_t<256, 128, 4, 2, 32>(gg, st) : launch_t<256, 128, 4, 2, 16>(gg, st);       // 8 waves, 64x64 per wave
        default:
            if (bk == 64) return launch_t<64, 64, 2, 2, 64>(gg, st);
            if (bk == 32) return launch_t<64, 64, 2, 2, 32>(gg, st);
            return launch_t<64, 64, 2, 2, 16>(gg, st);
    }
}

}  // namespace sva
