// Weight-streaming fp16-MFMA conv-GEMM for few rows: the content encoder's GEMMs of 1-9 streams when sva_config.enc_dtype = 1.  The
// skeleton of gemm_stream.hip on fp16 operands; what the two share is gemm_stream_common.h (tile numbering, the waves' K-block schedule,
// the early request of the epilogue operands, the meeting in LDS summed in the fixed order wave 0 .. KW - 1, the unit-per-thread tail),
// KB blocks = (4 NT + 8 MT) KB registers in flight per lane.
// What is this kernel's own:
//   * the product is v_mfma_f32_16x16x32_f16: BOTH operands rounded once, to nearest even, to fp16; products exact, accumulation fp32.  Lane l
//     supplies k = 8 (l >> 4) + j, j < 8, of row / column l & 15 of a 32-k block on both operands; the accumulator holds column l & 15, rows
//     4 (l >> 4) + reg;
//   * the weights are read ONLY from the fp16 fragment-major packing made at finalize ([N / 16][K / 32][64 lanes][8 halves]: one
//     wave-instruction = one contiguous KiB, half the bytes of gemm_stream.hip's fp32 packing; stream_h_pack_weights below);
//   * the activations are read as fp32 and converted in registers, element by element (v_cvt_f16_f32, round to nearest even -- never the
//     round-towards-zero pack).  The A operand is the activation exactly as its producer stored it: no SiLU / RMSNorm / ConvNeXt prologue here
//     (a fused RMSNorm would round x * w before the row statistic is applied -- another number than fp16(RMSNorm(x) w));
//   * epilogues: bias, GELU, gamma + residual, SwiGLU over the w13 pairing, skipped history rows; nothing else (stream_h_gemm_supported);
//   * an output that is not finite (an operand beyond fp16's +-65504) raises the host-mapped flag g.ovf from the lanes that see it.
// The mode is NOT parity-preserving by construction: content codes may differ from the fp32 fixtures where a pre-sign value is near zero
// ("enc_dtype = 1").  Conversion and epilogue arithmetic are scalar per element and nothing is contracted: a row's result does
// not depend on the tile or slot it sits in.
#include "sva_common.h"
#include "device_util.h"
#include "gemm_stream_common.h"

#include <cstring>
#include <vector>

namespace sva {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

struct StreamHArgs {
    const float* A; long a_bstride, a_off; int lda, T, M, stride, dil, taps, Cin;
    const _Float16* W; int N; int nkb;           // nkb = taps * Cin / 32
    const float* bias; const float* gamma; const float* res; long r_bstride, r_off; int ldr;
    float* C; long c_bstride, c_off; int ldc;
    int skip_lo, skip_hi, act, w13;
    int* ovf;
    int m_tiles, n_tiles;                        // workgroup tiles
};

// one element, round to nearest even (the cast is v_cvt_f16_f32 under the default rounding mode)
__device__ __forceinline__ f16x8 to_f16x8(const f32x4& lo, const f32x4& hi) {
    f16x8 h;
    h[0] = (_Float16)lo.x; h[1] = (_Float16)lo.y; h[2] = (_Float16)lo.z; h[3] = (_Float16)lo.w;
    h[4] = (_Float16)hi.x; h[5] = (_Float16)hi.y; h[6] = (_Float16)hi.z; h[7] = (_Float16)hi.w;
    return h;
}

// KB: blocks a wave holds in registers = the smallest instantiated count that covers its share of K (a block beyond the share is a clamped
//     re-load whose MFMAs are skipped by a wave-uniform branch -- a branch around arithmetic only, the loads stay unconditional)
// LOOP: some wave holds more than KB blocks (a consumed block's registers are re-requested at once, clamped indices instead of a branch)
template <int MT, int NT, int KW, int KB, bool LOOP>
__global__ __launch_bounds__(64 * KW) void stream_h_gemm_kernel(const StreamHArgs g) {
    // no implicit contraction in this kernel: every row tile's arithmetic must round the same way (a row's result must not depend on its position)
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float red[];      // [KW][MT*NT][64] f32x4
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n0, m_base;
    wstream::tile_origin<MT, NT>(g, n0, m_base);
    const int fr = lane & 15, fg = lane >> 4;
    const int kc_tiles = g.Cin >> 5;
    const _Float16* wp[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        int t16 = (n0 >> 4) + j;
        const int last = (g.N - 1) >> 4;
        if (t16 > last) t16 = last;
        wp[j] = g.W + ((long)t16 * g.nkb * 64 + lane) * 8;
    }
    const float* ap[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        int m = m_base + i * 16 + fr;
        if (m > g.M - 1) m = g.M - 1;
        const int b = m / g.T, t = m - b * g.T;
        ap[i] = g.A + (long)b * g.a_bstride + g.a_off + (long)t * g.stride * g.lda + 8 * fg;
    }
    int my_n, last_kb;                           // blocks of this wave: wave, wave + KW, ...
    wstream::wave_blocks<KW>(0, g.nkb, wave, my_n, last_kb);

    f16x8 wv[KB][NT];
    f32x4 av[KB][MT][2];
    auto issue_w = [&](f16x8 (&w)[NT], int kb) {
        kb = kb < g.nkb ? kb : last_kb;
#pragma unroll
        for (int j = 0; j < NT; ++j) w[j] = *reinterpret_cast<const f16x8*>(wp[j] + (long)kb * 512);
    };
    auto issue_a = [&](f32x4 (&a)[MT][2], int kb) {
        kb = kb < g.nkb ? kb : last_kb;
        const int tap = kb / kc_tiles;                       // Cin % 32 == 0: a block never straddles two taps
        const int kc = (kb - tap * kc_tiles) * 32;
        const long aoff = (long)tap * g.dil * g.lda + kc;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            a[i][0] = *reinterpret_cast<const f32x4*>(ap[i] + aoff);
            a[i][1] = *reinterpret_cast<const f32x4*>(ap[i] + aoff + 4);
        }
    };
    // epilogue operands of this thread's output units, requested first
    wstream::EpiOperands<MT, NT, KW> e;
    e.request(g, tid, n0, m_base);
    // everything this wave needs (or its first KB blocks) is requested here, weights first
#pragma unroll
    for (int d = 0; d < KB; ++d) issue_w(wv[d], wave + d * KW);
#pragma unroll
    for (int d = 0; d < KB; ++d) issue_a(av[d], wave + d * KW);
    __builtin_amdgcn_sched_barrier(0);          // hipcc's scheduler otherwise sinks the requests next to their uses (a queue two blocks deep)

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int it = 0; it < (LOOP ? my_n : 1); it += KB) {
#pragma unroll
        for (int d = 0; d < KB; ++d) {
            f16x8 w[NT], a[MT];
#pragma unroll
            for (int j = 0; j < NT; ++j) w[j] = wv[d][j];
#pragma unroll
            for (int i = 0; i < MT; ++i) a[i] = to_f16x8(av[d][i][0], av[d][i][1]);
            if constexpr (LOOP) {
                issue_w(wv[d], wave + (it + d + KB) * KW);
                issue_a(av[d], wave + (it + d + KB) * KW);
            }
            if (it + d < my_n) {                     // wave-uniform; no load inside
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], w[j], acc[i][j], 0, 0, 0);
            }
        }
    }
    // the KW partial tiles meet in LDS (a store of the kernel's own: handed to a shared function it cost registers and an occupancy step in some
    // instances); every thread sums and stores its share (no scale, no accumulate: stream_h_gemm_supported)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
            *reinterpret_cast<f32x4*>(&red[((wave * (MT * NT) + i * NT + j) * 64 + lane) * 4]) = acc[i][j];
    __syncthreads();
    bool bad = false;
    wstream::unit_tail<MT, NT, KW>(g, red, tid, n0, m_base, e, 1.f, false, [](int, int) { return (f32x4){1.f, 1.f, 1.f, 1.f}; },
                                   [&](float v) { bad = bad || !(fabsf(v) < INFINITY); });
    // range report: an ordinary store from the lanes that saw a non-finite output
    if (bad && g.ovf) *reinterpret_cast<volatile int*>(g.ovf) = 1;
}

template <int MT, int NT, int KW, int KB, bool LOOP>
int launch_stream_h_kl(const ConvGemm& g, hipStream_t st) {
    StreamHArgs a;
    wstream::fill_front(a, g, 32, MT, NT);
    a.W = reinterpret_cast<const _Float16*>(g.Wkh); a.ovf = g.ovf;
    static DeviceOnce attr;
    return wstream::launch_tiles(stream_h_gemm_kernel<MT, NT, KW, KB, LOOP>, a, KW, (size_t)KW * MT * NT * 256 * sizeof(float), attr, st);
}

// registers in flight: (4 NT + 8 MT) KB per lane (weights as 8 halves, activations as 8 floats)
template <int MT, int NT, int KW>
int launch_stream_h_k(const ConvGemm& g, hipStream_t st) {
    const int nkb = g.taps * g.Cin / 32, need = (nkb + KW - 1) / KW;
    constexpr int PER = 4 * NT + 8 * MT;
    constexpr int KB0 = wstream::kb_for<PER, KW, false, 16>(), KB1 = wstream::kb_for<PER, KW, true, 16>();
    int rc = 0;
    if (wstream::kb_ladder<KB0>(need, rc, [&](auto kb) { return launch_stream_h_kl<MT, NT, KW, decltype(kb)::value, false>(g, st); })) return rc;
    return launch_stream_h_kl<MT, NT, KW, KB1, true>(g, st);
}

}  // namespace

// fp16 fragment-major packing of a host [N][K] matrix (K % 32 == 0): tile t of 16 rows, block kb of 32 k, lane l = (row & 15) + 16 * (k / 8):
// eight consecutive k, each rounded once to nearest even -- what lane l feeds to the MFMA of the block; rows beyond N are zeros
void stream_h_pack_weights(const float* W, int N, int K, std::vector<uint16_t>& out) {
    const long nkb = K / 32, nt16 = (N + 15) / 16;
    out.assign((size_t)nt16 * nkb * 512, 0);
    for (long t = 0; t < nt16; ++t)
        for (long kb = 0; kb < nkb; ++kb)
            for (int ln = 0; ln < 64; ++ln) {
                const long n = t * 16 + (ln & 15);
                if (n >= N) continue;
                const float* src = W + (size_t)n * K + kb * 32 + 8 * (ln >> 4);
                uint16_t* dst = &out[((t * nkb + kb) * 64 + ln) * 8];
                for (int j = 0; j < 8; ++j) {
                    const _Float16 h = (_Float16)src[j];
                    memcpy(&dst[j], &h, 2);
                }
            }
}

// exactly the prologues / epilogues the encoder's calls use; everything else is refused
bool stream_h_gemm_supported(const ConvGemm& g) {
    return g.Wkh && g.A && g.C && !g.Ap && !g.Cp && g.Cin > 0 && g.Cin % 32 == 0 && g.taps >= 1 && g.stride >= 1 && g.dil >= 1 && g.M > 0 && g.T > 0 && g.N >= 1 &&
           g.lda % 4 == 0 && g.a_off % 4 == 0 && g.a_bstride % 4 == 0 && !g.dw_wT && !g.rms_w && !g.a_silu && !g.accumulate && g.scale == 1.f &&
           g.ksplit <= 1 && (g.act == ACT_NONE || g.act == ACT_GELU) &&
           (!g.w13 || (g.N % 32 == 0 && !g.bias && !g.gamma && !g.res && g.act == ACT_NONE)) &&
           (long)((g.M + 15) / 16) * ((g.N + 15) / 16) < (1L << 30);
}

// (MT, NT, KW) for a shape, modelled on what the tuned table gives gemm_stream.hip for the encoder's shapes (tune_table.inc, kind 6; a 32-k
// block is two of its 16-k blocks): one row tile up to 16 rows, two to 64, four beyond; column-tile pairs for SwiGLU and for wide outputs;
// 4 K-split waves up to 512 k, 8 up to 2048 k, 16 beyond when the tile is small enough for 16 waves' registers
void stream_h_config(const ConvGemm& g, int* mt, int* nt, int* kw) {
    const int nkb = g.taps * g.Cin / 32;
    *nt = (g.w13 || (g.N % 32 == 0 && g.N >= 2048)) ? 2 : 1;
    *mt = g.M <= 16 ? 1 : g.M <= 64 ? 2 : 4;
    *kw = nkb <= 16 ? 4 : (nkb <= 64 || *mt * *nt > 2) ? 8 : 16;
}

// mt in {1, 2, 4}, nt in {1, 2}, kw in {4, 8, 16 (mt * nt <= 2)}; mt = 0: the heuristic's
int launch_stream_h_gemm(const ConvGemm& g, int mt, int nt, int kw, hipStream_t st) {
    SVA_CHECK(stream_h_gemm_supported(g), "stream_h_gemm: unsupported problem");
    if (mt == 0) stream_h_config(g, &mt, &nt, &kw);
    SVA_CHECK(!(g.w13 && nt != 2), "stream_h_gemm: SwiGLU needs column-tile pairs (nt = 2)");
    int rc = 0;
    if (wstream::config_ladder(mt, nt, kw, rc, [&](auto MTc, auto NTc, auto KWc) {
            return launch_stream_h_k<decltype(MTc)::value, decltype(NTc)::value, decltype(KWc)::value>(g, st);
        })) return rc;
    set_error("stream_h_gemm: bad configuration");
    return -1;
}

}  // namespace sva
