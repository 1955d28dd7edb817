// What the two weight-streaming kernels (gemm_stream.hip: f32 MFMA, gemm_stream_h.hip: fp16 MFMA) share: everything that does not depend
// on the operand format.  A workgroup owns a (16 MT) x (16 NT) output tile for the whole K axis; its KW waves take the K blocks round-robin
// (wave_blocks), request the epilogue's operands first (EpiOperands) and then every operand fragment (the kernels' own issue_w / issue_a);
// the KW partial tiles meet in LDS once (each kernel stores its own; tile_sum sums them, also for the small-M kernel of gemm.hip) and every thread sums and
// stores its share of the tile (unit_tail).  A kernel keeps its fragment types, issue_w / issue_a, its prologue and its MFMA.
// (The f32 kernel also keeps its own text of EpiOperands::request and unit_tail -- see there; the fp16 kernel calls them.)
// Device code here that does arithmetic carries `#pragma clang fp contract(off)` itself: the pragma of the kernels is lexical and does
// not reach code inlined into them, and a row's rounding must not depend on its tile position.
#pragma once
#include <utility>

#include "gemm_epilogue.h"
#include "sva_common.h"

namespace sva {
namespace wstream {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Both kernels' argument structs are slim copies of a ConvGemm (the kernarg segment stays small, and the fields a kernel needs first --
// W, then A -- sit in front: a struct with W behind the common fields measured 2-7 % slower per launch).  They share the NAMES of their
// common fields, which the templates below (G) rely on; this fills those.  nkb = K blocks of kblk k
template <class G>
void fill_front(G& a, const ConvGemm& g, int kblk, int mt, int nt) {
    a.A = g.A; a.a_bstride = g.a_bstride; a.a_off = g.a_off; a.lda = g.lda; a.T = g.T; a.M = g.M; a.stride = g.stride; a.dil = g.dil;
    a.taps = g.taps; a.Cin = g.Cin; a.N = g.N; a.nkb = g.taps * g.Cin / kblk;
    a.bias = g.bias; a.gamma = g.gamma; a.res = g.res; a.r_bstride = g.r_bstride; a.r_off = g.r_off; a.ldr = g.ldr;
    a.C = g.C; a.c_bstride = g.c_bstride; a.c_off = g.c_off; a.ldc = g.ldc; a.skip_lo = g.skip_lo; a.skip_hi = g.skip_hi;
    a.act = g.act; a.w13 = g.w13;
    a.m_tiles = (g.M + 16 * mt - 1) / (16 * mt); a.n_tiles = (g.N + 16 * nt - 1) / (16 * nt);
}

// tile of workgroup blockIdx.x: XCD x owns the x-th contiguous eighth of the tile sequence (row tiles fastest), so a weight panel is
// fetched from the fabric by one L2
template <int MT, int NT, class G>
__device__ __forceinline__ void tile_origin(const G& g, int& n0, int& m_base) {
    const int V = xcd_band_index(blockIdx.x, g.m_tiles * g.n_tiles);
    const int tn = V / g.m_tiles, tm = V - tn * g.m_tiles;
    n0 = tn * (16 * NT); m_base = tm * (16 * MT);
}

// K blocks [kb_lo, kb_hi) over KW waves: wave w takes kb_lo + w, kb_lo + w + KW, ...; my_n of them, the last one last_kb (what a
// request beyond the share re-loads: no load under a branch)
template <int KW>
__device__ __forceinline__ void wave_blocks(int kb_lo, int kb_hi, int wave, int& my_n, int& last_kb) {
    const int n = kb_hi - kb_lo;
    my_n = n > wave ? (n - wave + KW - 1) / KW : 0;
    last_kb = my_n > 0 ? kb_lo + wave + (my_n - 1) * KW : kb_lo;
}

// Epilogue operands of a thread's output units (unit u = tid + k 64 KW = (row tile i, column tile j, lane slot l): see unit_tail),
// requested before anything else so that the tail is arithmetic and stores only.  Neutral defaults where an operand is absent.
template <int MT, int NT, int KW>
struct EpiOperands {
    static constexpr int UNITS = (MT * NT + KW - 1) / KW;
    float bias[UNITS], gamma[UNITS], res[UNITS][4];
    template <class G>
    __device__ __forceinline__ void request(const G& g, int tid, int n0, int m_base) {
#pragma unroll
        for (int k = 0; k < UNITS; ++k) {
            bias[k] = 0.f; gamma[k] = 1.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) res[k][r] = 0.f;
        }
        if (g.w13) return;
#pragma unroll
        for (int k = 0; k < UNITS; ++k) {
            int u = tid + k * 64 * KW;
            if (u > MT * NT * 64 - 1) u = MT * NT * 64 - 1;
            const int l = u & 63, ij = u >> 6, i = ij / NT, jj = ij - i * NT;
            int n = n0 + jj * 16 + (l & 15);
            if (n > g.N - 1) n = g.N - 1;
            if (g.bias) bias[k] = g.bias[n];
            if (g.gamma) gamma[k] = g.gamma[n];
            if (g.res) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    int m = m_base + i * 16 + (l >> 4) * 4 + r;
                    if (m > g.M - 1) m = g.M - 1;
                    const int b = m / g.T, tt = m - b * g.T;
                    res[k][r] = g.res[epi::r_row(g, b, tt) + n];
                }
            }
        }
    }
};

// the KW partial tiles met in LDS as red[KW][MT * NT][64 lanes] f32x4: their sum in the fixed order wave 0 .. KW - 1 (UNR: unroll of that sum)
template <int MT, int NT, int KW, int UNR>
__device__ __forceinline__ f32x4 tile_sum(const float* red, int i, int j, int l) {
#pragma clang fp contract(off)
    f32x4 s = *reinterpret_cast<const f32x4*>(&red[((i * NT + j) * 64 + l) * 4]);
#pragma unroll UNR
    for (int w = 1; w < KW; ++w) s += *reinterpret_cast<const f32x4*>(&red[((w * (MT * NT) + i * NT + j) * 64 + l) * 4]);
    return s;
}

// Every thread sums and stores its share of the tile: unit u = (row tile i, column tile j [pair for SwiGLU], lane slot l).
//   row_factor(i, rq)  f32x4 factor of rows rq .. rq + 3 of row tile i (the fused RMSNorm; ones otherwise: folds away)
//   report(v)          sees every stored value (the fp16 kernel's range report)
template <int MT, int NT, int KW, class G, class RowFactor, class Report>
__device__ __forceinline__ void unit_tail(const G& g, const float* red, int tid, int n0, int m_base, const EpiOperands<MT, NT, KW>& e,
                                          float scale, bool accumulate, RowFactor row_factor, Report report) {
#pragma clang fp contract(off)
    const bool w13 = g.w13 != 0;
    const int jt = w13 ? NT / 2 : NT;
    const int units = MT * jt * 64;
#pragma unroll
    for (int k = 0; k < EpiOperands<MT, NT, KW>::UNITS; ++k) {
        const int u = tid + k * 64 * KW;
        if (u >= units) break;
        const int l = u & 63, ij = u >> 6;
        const int i = ij / jt, jj = ij - i * jt;
        const int col = l & 15, rq = (l >> 4) * 4;
        const f32x4 inv4 = row_factor(i, rq);
        if (w13) {
            const f32x4 ga = tile_sum<MT, NT, KW, 4>(red, i, 2 * jj, l) * inv4, up = tile_sum<MT, NT, KW, 4>(red, i, 2 * jj + 1, l) * inv4;
            const int n = n0 + jj * 32 + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int b, tt;
                if (n >= g.N || !epi::out_row(g, m_base + i * 16 + rq + r, b, tt)) continue;
                const float v = epi::swiglu(ga[r], up[r]);
                report(v);
                g.C[epi::c_row(g, b, tt) + (n0 >> 1) + jj * 16 + col] = v;
            }
            continue;
        }
        const f32x4 s = tile_sum<MT, NT, KW, 4>(red, i, jj, l) * inv4;
        const int n = n0 + jj * 16 + col;
        if (n >= g.N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int b, tt;
            if (!epi::out_row(g, m_base + i * 16 + rq + r, b, tt)) continue;
            float* cp = g.C + epi::c_row(g, b, tt) + n;
            const float v = epi::value<true>(s[r], g.act, scale, true, [&] { return e.bias[k]; }, true, [&] { return e.gamma[k]; }, true, [&] { return e.res[k][r]; },
                                             accumulate, [&] { return *cp; });
            report(v);
            *cp = v;
        }
    }
}

// ---- host side ----
// K blocks a wave holds in registers: `per` registers per block and lane against a budget of ~200 load registers per wave (a 16-wave
// workgroup's waves own 128 registers; the looping form keeps a second copy of the block it is consuming), at most `cap`
template <int PER, int KW, bool LOOP, int CAP>
constexpr int kb_for() {
    constexpr int budget = KW == 16 ? (LOOP ? 44 : 64) : (LOOP ? 136 : 200);
    return budget / PER > CAP ? CAP : (budget / PER < 2 ? 2 : budget / PER);
}
// the smallest instantiated KB <= KB0 that covers `need` blocks per wave: rc = launch(integral_constant<int, KB>); false: none does
template <int KB0, int KBv, class F>
bool try_kb(int need, int& rc, F& launch) {
    if constexpr (KBv <= KB0) {
        if (need <= KBv) { rc = launch(std::integral_constant<int, KBv>{}); return true; }
    }
    return false;
}
template <int KB0, class F>
bool kb_ladder(int need, int& rc, F launch) {
    return try_kb<KB0, 1>(need, rc, launch) || try_kb<KB0, 2>(need, rc, launch) || try_kb<KB0, 3>(need, rc, launch) || try_kb<KB0, 4>(need, rc, launch) ||
           try_kb<KB0, 6>(need, rc, launch) || try_kb<KB0, 8>(need, rc, launch) || try_kb<KB0, 12>(need, rc, launch) || try_kb<KB0, 16>(need, rc, launch) ||
           try_kb<KB0, 24>(need, rc, launch);
}
// the instantiated (MT, NT, KW): mt in {1, 2, 4}, nt in {1, 2}, kw in {4, 8, 16 (mt * nt <= 2)}; false: not one of them
template <class F>
bool config_ladder(int mt, int nt, int kw, int& rc, F launch) {
#define SVA_SG(MTv, NTv, KWv) \
    if (mt == MTv && nt == NTv && kw == KWv) { rc = launch(std::integral_constant<int, MTv>{}, std::integral_constant<int, NTv>{}, std::integral_constant<int, KWv>{}); return true; }
    SVA_SG(1, 1, 4) SVA_SG(1, 1, 8) SVA_SG(1, 1, 16)
    SVA_SG(2, 1, 4) SVA_SG(2, 1, 8) SVA_SG(2, 1, 16)
    SVA_SG(4, 1, 4) SVA_SG(4, 1, 8)
    SVA_SG(1, 2, 4) SVA_SG(1, 2, 8) SVA_SG(1, 2, 16)
    SVA_SG(2, 2, 4) SVA_SG(2, 2, 8)
    SVA_SG(4, 2, 4) SVA_SG(4, 2, 8)
#undef SVA_SG
    return false;
}
// one workgroup of KW waves per tile
template <class Args>
int launch_tiles(void (*kernel)(Args), const Args& a, int kw, size_t smem, DeviceOnce& attr, hipStream_t st) {
    if (smem > 48 * 1024) SVA_TRY_RC(attr.max_dynamic_lds((const void*)kernel, smem));
    hipLaunchKernelGGL(kernel, dim3(a.m_tiles * a.n_tiles), dim3(64 * kw), smem, st, a);
    SVA_HIP(hipGetLastError());
    return 0;
}

}  // namespace wstream
}  // namespace sva
