// Conv-GEMM dispatch (host only): which kernel family runs a problem, in which configuration.
//   plan_conv_gemm     the decision, a pure function of the problem (+ debug_options() and the compiled-in tables): no HIP call, no stream
//   run_plan           a switch over the family onto the launchers of gemm*.hip
//   plan_report_kind   the one numbering of the families that leaves this file (profiling tables, tune_table.inc, tune log / dump)
//   tune_conv_gemm     SVA_DEBUG=autotune=1: the timed search (tools/make_tune_table.py), outside the planner
#include "sva_common.h"
#include <array>
#include <map>
#include <mutex>
#include <vector>
#include <stdlib.h>
#include <stdio.h>

namespace sva {

// Kernel family of a plan as the profiling table reports it (stages.hip: prof_shapes; bench.py reads it; profiles/*gemm_table*.csv hold it).
// The numbers are frozen.  The five families of the timed search carry the same number in tune_table.inc, the tune log and the tune dump.
int plan_report_kind(const GemmPlan& p, int pmode) {
    //                         SmallM Tiled Ring Split F16W Stream Planes PlanesDma StreamH      (Planes / PlanesDma: + pmode = 7 / 8 in H3 / H1, 9 / 10)
    // (Planes' base equals Stream's: harmless, because table_kind / plan_from_table_kind below only ever see the five families of the timed search)
    static const int base[] = {0,     1,    2,   4,    5,   6,     6,     8,        11};
    const bool planes = p.family == GemmFamily::Planes || p.family == GemmFamily::PlanesDma;
    return base[(int)p.family] + (planes ? pmode : 0);
}
static int table_kind(const GemmPlan& p) { return plan_report_kind(p, 0); }
bool plan_from_table_kind(int kind, int a, int b, int c, int z, GemmPlan* out) {
    for (GemmFamily f : {GemmFamily::SmallM, GemmFamily::Tiled, GemmFamily::Ring, GemmFamily::Split, GemmFamily::Stream}) {
        *out = GemmPlan{f, a, b, c, z};
        if (table_kind(*out) == kind) return true;
    }
    return false;
}

using ShapeKey = std::array<int, 6>;      // (M, N, K, taps, epilogue / prologue flags, stride)
// the tiled / ring / split / planes epilogues store whole 16-byte pieces of C rows (and read the residual the same way)
static bool c_rows_vectorised(const ConvGemm& g) {
    return g.N % 4 == 0 && g.ldc % 4 == 0 && g.c_off % 4 == 0 && g.c_bstride % 4 == 0 && (!g.res || (g.ldr % 4 == 0 && g.r_off % 4 == 0 && g.r_bstride % 4 == 0));
}
static ShapeKey shape_key(const ConvGemm& g, int group_n) {
    const int flags = (g.a_silu ? 1 : 0) | (g.rms_w ? 2 : 0) | (g.w13 ? 4 : 0) | (c_rows_vectorised(g) ? 8 : 0) | (g.accumulate ? 16 : 0) | (group_n > 1 ? 32 : 0) | (g.dw_wT ? 64 : 0);
    return {g.M, g.N, g.taps * g.Cin, g.taps, flags, g.stride};
}
// compiled-in per-shape choices: the outcome of an offline tuning run (tools/make_tune_table.py -> tune_table.inc), so the
// default dispatch is a pure function of the problem shape
struct TuneRow { int key[6]; int kind, a, b, c, z; };
static const TuneRow kTuneTable[] = {
#include "tune_table.inc"
    {{0, 0, 0, 0, 0, 0}, -1, 0, 0, 0, 1}};
static const std::map<ShapeKey, GemmPlan>& static_table() {
    static const std::map<ShapeKey, GemmPlan> m = [] {
        std::map<ShapeKey, GemmPlan> t;
        if (!debug_options().tune_table) return t;
        for (const TuneRow& r : kTuneTable) {
            GemmPlan p;
            if (r.kind < 0 || !((debug_options().tune_kinds >> r.kind) & 1) || !plan_from_table_kind(r.kind, r.a, r.b, r.c, r.z, &p)) continue;
            t[{r.key[0], r.key[1], r.key[2], r.key[3], r.key[4], r.key[5]}] = p;
        }
        return t;
    }();
    return m;
}
// A decode-sized row count between two tabulated ones (40 or 44 streams: the table holds 36 and 48) takes the choice of the next larger one within
// 1.5 x -- every kernel handles partial row tiles, and the heuristic's pick there measured 20 % slower (AR stage 4.7 ms at 40 / 44 streams, 3.8 at 48).
// The scan is memoised per shape (an untabulated shape paid up to M / 2 map look-ups on every launch).
static const GemmPlan* table_row(const ShapeKey& key) {
    const auto& tab = static_table();
    auto it = tab.find(key);
    const int M = key[0];
    if (it == tab.end() && M >= 8 && M <= 512) {
        static std::mutex memo_mu;
        static std::map<ShapeKey, int> memo;            // shape -> the tabulated row count it borrows (0: none)
        int borrowed = -1;
        {
            std::lock_guard<std::mutex> lk(memo_mu);
            auto mi = memo.find(key);
            if (mi != memo.end()) borrowed = mi->second;
        }
        ShapeKey k = key;
        if (borrowed < 0) {
            borrowed = 0;
            for (int m = M + 1; m <= M + M / 2; ++m) {
                k[0] = m;
                if (tab.find(k) != tab.end()) { borrowed = m; break; }
            }
            std::lock_guard<std::mutex> lk(memo_mu);
            memo[key] = borrowed;
        }
        k[0] = borrowed;
        if (borrowed > 0) it = tab.find(k);
    }
    return it == tab.end() ? nullptr : &it->second;
}
// SVA_DEBUG=autotune=1: what the timed search of this process picked, per shape
static std::mutex g_tune_mu;
static std::map<ShapeKey, GemmPlan> g_tune;
static bool tuned_plan(const ShapeKey& key, GemmPlan* out) {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    auto it = g_tune.find(key);
    if (it != g_tune.end()) *out = it->second;
    return it != g_tune.end();
}

// Tile variant of the planes kernel (gemm_planes.hip) for a problem.  The candidates that ever win on the encoder's / vocoder's shapes
// (tools/planes_bench.py, profiles/r04_planes_bench.txt) are 128 x 128 (two workgroups per CU) and 256 x 128 (eight waves, one per CU,
// two thirds of the operand traffic); which one is a matter of how the tile count quantises over the 256 CUs.  In units of the time
// T a CU needs for one 128 x 128 tile's worth of work when it is full: a round of 512 small tiles costs 2 T, a last round of <= 256
// of them (one per CU) 1.3 T, a round of 256 large tiles 1.7 T.  The rule reproduces the measured winner of the two on all ten shapes.
struct PlanesRow { int M, N, K, variant; };
static const PlanesRow g_planes_table[] = {
#include "planes_table.inc"
};
static int planes_variant(const ConvGemmGroup& gg, int lead) {
    const ConvGemm& g = gg.g[lead];
    const int group_n = gg.n;
    // conv taps over A planes (the HiFiGAN levels' ResBlock convs, three branches per launch): only the LDS-DMA form reads them; its tile by
    // the output width and by whether 128 x 128 tiles would fill the chip
    if (g.Ap && (g.taps > 1 || group_n > 1 || g.cp_silu) && debug_options().planes_dma != 0) {
        bool ok = true;
        for (int i = 0; i < gg.n; ++i) ok = ok && planes_dma_conv_supported(gg.g[i]);
        if (ok) {
            const int dv = debug_options().voc_dma_variant;
            if (g.N % 128 == 0 && (long)((g.M + 127) / 128) * (g.N / 128) * group_n >= 192) return dv >= 9 && dv <= 14 && dv != 12 ? dv : 11;       // (its loader-wave form: 66 / 61 -> 60 / 55 us per launch at C = 128, 64 streams)
            return g.N == 64 && g.M * (long)group_n >= 3 * 8192 ? 13 : 14;
        }
    }
    bool dma_ok = planes_dma_gemm_supported(g) && debug_options().planes_dma != 0;
    if (group_n > 1) dma_ok = false;
    // measured winners for the encoder's shapes (tools/planes_tune.py -> planes_table.inc; every variant computes the same accumulation per
    // output, so the table is a speed choice only): the row with this (N, K) whose M is nearest, if within a quarter of it
    if (group_n == 1 && g.taps == 1) {
        const PlanesRow* best = nullptr;
        for (const PlanesRow& r : g_planes_table)
            if (r.N == g.N && r.K == g.Cin && (r.variant < 8 || dma_ok) &&
                (!best || std::abs(r.M - g.M) < std::abs(best->M - g.M))) best = &r;
        if (best && std::abs(best->M - g.M) * 4 <= g.M && (best->variant != 6 || g.M >= 256) &&
            (g.M >= 128 || best->variant == 2 || best->variant == 3 || best->variant >= 9))
            return best->variant >= 11 && debug_options().planes_lw == 0 ? 10 : best->variant;       // (A/B: the loader-wave forms off)
    }
    // both operands as planes, whole 128-column tiles, a shape outside the table: the persistent LDS-DMA form with 128 x 128 tiles and TWO
    // workgroups per CU (variant 10: one workgroup's epilogue runs under the other's K steps) -- it wins or ties on every encoder shape at 64
    // streams with the real epilogues (profiles/r05_planes_dma_bench.txt); 256 x 128 (8) never wins.  (Table vs this rule for the shapes
    // the table holds: encoder stage 4.41 / 5.13 / 8.50 ms against 4.67 / 5.28 / 8.68 at 48 / 64 / 128 streams, pipelined frames/s equal.)
    if (dma_ok && (long)((g.M + 127) / 128) * (g.N / 128) >= 64) return 10;
    if (g.N < 128) return g.M >= 128 ? 1 : 3;
    if (g.M < 128) return 2;
    const long wg0 = (long)((g.M + 127) / 128) * ((g.N + 127) / 128) * group_n, wg6 = (long)((g.M + 255) / 256) * ((g.N + 127) / 128) * group_n;
    if (wg0 < 224) return 3;                // too few 128 x 128 tiles for the chip: 64 x 64 (the mid-size shapes of profiles/r04_planes_bench_small.txt)
    if (g.M < 256) return 0;
    const long rem = wg0 % 512;
    const double t0 = (double)(wg0 / 512) * 2.0 + (rem == 0 ? 0.0 : rem <= 256 ? 1.3 : 2.0);
    const double t6 = (double)((wg6 + 255) / 256) * 1.7;
    if (t6 < t0) return 6;
    return wg0 <= 768 ? 7 : 0;              // up to a round and a half of tiles: the 8-wave form of the same tile (four waves per SIMD overlap its phases better)
}
static GemmPlan planes_plan(const ConvGemmGroup& gg, int lead) {
    const int v = planes_variant(gg, lead);
    return GemmPlan{v >= 8 ? GemmFamily::PlanesDma : GemmFamily::Planes, v, 0, 0, 1};
}
// Operands that only exist as planes have no other kernel; fp16 x 1 weight planes (H1: a voc_dtype = 1 vocoder, an enc_dtype = 1 encoder) cost one
// product per block instead of the six or eight of any fp32-grade kernel -- every problem with enough rows to fill the planes kernel's tiles
static bool wants_planes_h1(const ConvGemm& g) { return g.Ap || g.Cp || (g.pmode == PLANES_H1 && g.M >= 1024 && g.N >= 32); }

// tile variant of the ring kernel for an under-filled grid: the largest tile that still gives every CU of a partition work
static int pipe_variant(const ConvGemm& g) {
    auto tiles = [&](int bm, int bn) { return (long)((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn); };
    if (tiles(128, 64) >= 192) return 2;
    if (tiles(64, 64) >= 160) return 1;
    if (tiles(32, 64) >= 96 || g.N % 64 == 0) return 0;
    return 6;
}

// Heuristic choice of (rows per workgroup = 16*MT, K-split waves KW) for the small-M kernel.
static void skinny_heuristic(const ConvGemm& g, int NT, int* mt_out, int* kw_out) {
    const int mt_total = (g.M + 15) / 16;
    const long nk = (long)g.taps * g.Cin / 16;
    const long cols = (g.N + 16 * NT - 1) / (16 * NT);
    int mt = mt_total < 4 ? mt_total : 4;
    auto blocks = [&](int m) { return cols * ((mt_total + m - 1) / m); };
    // Every row tile of a column block re-reads that block's weights.  Weight-heavy problems (AR layers at M = 64..128:
    // the panel comes from HBM) keep the tallest workgroup; light ones (encoder at M = 128..160: the panel sits in L2)
    // trade re-reads for >= ~1.5 workgroups per CU.  Tuned with tools/gemm_sweep4.py.
    const bool heavy = (long)g.N * g.taps * g.Cin * 4 > (8L << 20);
    if (heavy) { while (mt > 1 && blocks(mt) * 4 < 512) mt = mt > 2 ? 2 : 1; }
    else       { while (mt > 1 && blocks(mt) < 384) mt = mt > 2 ? 2 : 1; }
    int kw = 4;
    while (kw < 8 && blocks(mt) * kw < 2048 && nk / (2 * kw) >= 2) kw *= 2;
    if (kw == 8 && blocks(mt) * 8 < 512 && nk / 32 >= 2 && mt == 1) kw = 16;     // a handful of column blocks: split K deeper
    *mt_out = mt; *kw_out = kw;
}

// under-filled grids (fewer than ~1 tiled workgroup per CU): the barrier-free K-split kernel keeps far more
// loads in flight per CU than the LDS-staged one and pays for it with extra L2 reads, which are cheap there
static bool small_m_shape(int M, int N) {
    const long tiles64 = (long)((M + 63) / 64) * ((N + 63) / 64);
    return M <= 64 || (tiles64 < 256 && N >= 64);
}
bool conv_gemm_can_fuse_rms(int M, int N) { return small_m_shape(M, N); }

static GemmPlan heuristic_plan(const ConvGemm& g, bool c_vec) {
    // MFMA-bound problems outside the tuned table (batch sizes the tuning runs did not visit): the split-bf16 kernel, tile shape by
    // the rule the table shows -- wave-specialised 128x128 for narrow outputs with a long K, plain 128x128 otherwise, 64x64 for N < 128
    if (c_vec && split_gemm_supported(g) && g.M >= 2048 && g.N >= 64) {
        if (g.N < 128) return GemmPlan{GemmFamily::Split, 3, 0, 0, 1};
        const long K = (long)g.taps * g.Cin;
        return GemmPlan{GemmFamily::Split, (g.N <= 512 && K >= 1024) ? 4 : 0, 0, 0, 1};
    }
    const long tiles64 = (long)((g.M + 63) / 64) * ((g.N + 63) / 64);
    if (c_vec && pipe_gemm_supported(g) && g.M >= 32 && g.N >= 32 && tiles64 < 1024) return GemmPlan{GemmFamily::Ring, pipe_variant(g), 0, 0, 1};
    if (small_m_shape(g.M, g.N) || !c_vec) {      // (the tiled epilogue needs 16-byte aligned C rows)
        // two 16-column tiles per wave halve the A re-reads; worth it once the A panel dominates the L2 traffic
        const bool nt2 = g.w13 || (g.N % 32 == 0 && g.M >= 512 && (long)g.M * g.N >= 256L * 1024);
        GemmPlan p{GemmFamily::SmallM, 1, 4, nt2 ? 2 : 1, 1};
        skinny_heuristic(g, p.c, &p.a, &p.b);
        // A workgroup ingests 16*(MT + NT) rows of K floats and a CU sustains only ~40 GB/s of loads (tools/gemm_kscale.py:
        // time grows with K alone), so when the tiles do not cover the 256 CUs the K axis is split over more workgroups
        const long wgs = (long)((g.N + 16 * p.c - 1) / (16 * p.c)) * (((g.M + 15) / 16 + p.a - 1) / p.a);
        const long nkb = (long)g.taps * g.Cin / 16;
        while (p.z < 8 && wgs * p.z * 2 <= 256 && nkb / (2L * p.z * p.b) >= 2) p.z *= 2;
        return p;
    }
    if (g.N <= 16 && !g.w13) return GemmPlan{GemmFamily::Tiled, 3, 0, 0, 1};
    if (g.N <= 32) return GemmPlan{GemmFamily::Tiled, 2, 0, 0, 1};
    // 128x128 tiles only when they still fill the 256 CUs and their last (partial) round over them does not cost more than the lower
    // operand reuse of 64x64 tiles (e.g. 320 big tiles = 2 rounds for 1.25 rounds of work)
    const long big = (long)((g.M + 127) / 128) * ((g.N + 127) / 128);
    if (big >= 256 && ((big + 255) / 256) * 4.0 <= ((tiles64 + 255) / 256) * 1.25) return GemmPlan{GemmFamily::Tiled, 1, 0, 0, 1};
    return GemmPlan{GemmFamily::Tiled, 0, 0, 0, 1};
}

// Does the plan's family take THIS problem, with parameters its launcher knows?  The filter of the tuned table (keyed by shape only: a seam
// such as sva_op_conv can present a tuned shape with other strides), of a pick of the timed search, and the check of a plan that comes from
// outside (test / bench hooks).  Stricter than the table filter it replaces where no committed row is affected (tests/test_gemm_plan_cpu.py
// shows that every row passes): parameter ranges, no operand planes on the split kernel, and 16-byte C rows for EVERY tiled variant -- a
// future 64 x 64 tiled row keyed without the c_vec flag would be dropped, and should be: its float4 epilogue writes past a ragged row end.
// (The planes-DMA predicates include planes_gemm_supported; which of the variants 9 .. 12 a conv-form problem takes is the launcher's check.)
// A field a family's kernel never reads is refused here, not dropped: the tiled kernel has no RMSNorm / ConvNeXt prologue, the small-M kernel's
// prologues are one-of (tests/test_gpu_conv_gemm.py runs every refusal).
static bool plan_accepts(const ConvGemmGroup& gg, int lead, const GemmPlan& p) {
    const ConvGemm& g = gg.g[lead];
    const bool c_vec = c_rows_vectorised(g);
    const int a = p.a, b = p.b, c = p.c;
    // the fp32 families (and the fp16-weight kernel) read A and store C as fp32 arrays: operands that exist only as planes are the planes kernel's
    bool f32_ops = true;
    for (int i = 0; i < gg.n; ++i) f32_ops = f32_ops && gg.g[i].A && gg.g[i].C && !gg.g[i].Ap && !gg.g[i].Cp;
    switch (p.family) {
        case GemmFamily::SmallM:
            if (!f32_ops) return false;
            // (SwiGLU pairs two column tiles of one wave: with c == 1 the kernel stores nothing.  The fused RMSNorm form of the launcher takes no
            // SiLU and sums the squares of ONE row of Cin values; the ConvNeXt prologue is instantiated for one 16 x 16 tile only, reads seven
            // consecutive rows whatever the stride, holds at most 512 channels per wave and ignores taps / SiLU / RMSNorm.)
            if (g.w13 && c == 1) return false;
            if (g.rms_w && (g.taps != 1 || g.a_silu || gg.n > 1)) return false;
            if (g.dw_wT && !(a == 1 && c == 1 && g.taps == 1 && g.stride == 1 && g.M <= 16 && g.Cin <= 512 && !g.a_silu && !g.rms_w && !g.w13 && gg.n == 1 &&
                             g.dw_b && g.ln_w && g.ln_b)) return false;
            return (a >= 1 && a <= 4) && (b == 4 || b == 8 || (b == 16 && a == 1)) &&
                   (c == 1 || (c == 2 && g.N % 32 == 0) || (c == 4 && g.N % 64 == 0 && a != 3 && b != 16)) && p.z >= 1 && p.z <= 8 && (gg.n == 1 || p.z == 1);
        // (the tiled kernel has no prologue but SiLU: it never reads rms_w / dw_wT; its 256 x 16 tile cannot hold a SwiGLU column pair)
        case GemmFamily::Tiled: return f32_ops && a >= 0 && a <= 7 && c_vec && !g.rms_w && !g.dw_wT && !(g.w13 && a == 3);
        case GemmFamily::Ring: return f32_ops && a >= 0 && a <= 6 && c_vec && pipe_gemm_supported(g);
        case GemmFamily::Split: return f32_ops && a >= 0 && a <= 4 && c_vec && split_gemm_supported(g);
        case GemmFamily::F16W: return f32_ops && gg.n == 1 && f16w_gemm_supported(g);
        case GemmFamily::Stream:
            return f32_ops && gg.n == 1 && stream_gemm_supported(g) && (a == 1 || a == 2 || a == 4) && (c == 1 || c == 2) && (b == 4 || b == 8 || (b == 16 && a * c <= 2)) &&
                   !(g.w13 && c != 2) && (g.M + 16 * a - 1) / (16 * a) * (long)((g.N + 16 * c - 1) / (16 * c)) < 65536;
        case GemmFamily::Planes: return a >= 0 && a <= 7 && c_vec && planes_gemm_supported(g);
        case GemmFamily::PlanesDma: return a >= 9 && a <= 14 && c_vec && ((a <= 12 && planes_dma_gemm_supported(g)) || (a != 12 && planes_dma_conv_supported(g)));
        case GemmFamily::StreamH: return gg.n == 1 && stream_h_gemm_supported(g);
    }
    return false;
}

int conv_gemm_group_of(const ConvGemm* gs, int n, ConvGemmGroup* gg, int* lead) {
    SVA_CHECK(n >= 1 && n <= 3, "conv_gemm_group: 1..3 members");
    gg->n = n;
    *lead = 0;
    for (int i = 0; i < n; ++i) {
        const ConvGemm& a = gs[i];
        const ConvGemm& r = gs[0];
        if (n > 1) {
            SVA_CHECK(a.M == r.M && a.T == r.T && a.N == r.N && a.Cin == r.Cin && a.stride == r.stride && a.a_silu == r.a_silu && a.w13 == r.w13 &&
                      a.act == r.act && a.accumulate == r.accumulate && !a.rms_w && !a.dw_wT && a.ldc % 4 == r.ldc % 4 && (a.res != nullptr) == (r.res != nullptr) &&
                      (a.gamma != nullptr) == (r.gamma != nullptr) && (a.bias != nullptr) == (r.bias != nullptr),
                      "conv_gemm_group: members must share shape and epilogue");
            SVA_CHECK(a.lda % 4 == 0 && a.a_off % 4 == 0 && a.a_bstride % 4 == 0 && a.c_off % 4 == r.c_off % 4 && a.c_bstride % 4 == r.c_bstride % 4 &&
                      (!a.res || (a.ldr % 4 == r.ldr % 4 && a.r_off % 4 == r.r_off % 4 && a.r_bstride % 4 == r.r_bstride % 4)),
                      "conv_gemm_group: alignment classes must match");
        }
        gg->g[i] = a;
        if (a.taps > gs[*lead].taps) *lead = i;        // the decision is taken for (and timed on) the member with the longest K
    }
    return 0;
}

// Deterministic by default: the kernel / configuration of a problem shape comes from the compiled-in table (tune_table.inc, generated offline
// from a logged tuning run) or the heuristic -- never from wall-clock measurements of this process, so two processes, ranks or runs sum in the
// same order.  (SVA_DEBUG=autotune=1: a shape the timed search of this process has visited takes its pick instead of the table's.)
int plan_conv_gemm(const ConvGemmGroup& gg, int lead, GemmPlan* out) {
    const ConvGemm& g = gg.g[lead];
    const int group_n = gg.n;
    SVA_CHECK(g.Cin % 16 == 0 && g.Cin > 0, "conv_gemm: Cin must be a multiple of 16");
    // decode-sized linear layers of an fp16-weight AR: stream the fp16 weights (half the bytes of the fp32 copy) through the f16 pipes
    if (g.Wh && group_n == 1 && g.M <= 256 && debug_options().f16_weights && (f16w_gemm_validated_compiler() || debug_options().f16_weights == 2) &&
        f16w_gemm_supported(g)) {
        *out = GemmPlan{GemmFamily::F16W, 0, 0, 0, 1};
        return 0;
    }
    SVA_CHECK(g.lda % 4 == 0 && (g.a_off % 4) == 0 && (g.a_bstride % 4) == 0, "conv_gemm: A must be float4-aligned");
    const bool c_vec = c_rows_vectorised(g);
    SVA_CHECK(g.M > 0 && g.N > 0 && g.T > 0, "conv_gemm: empty problem");
    if (g.w13) SVA_CHECK(g.N % 32 == 0, "conv_gemm: w13 needs N % 32 == 0");
    if (g.rms_w) SVA_CHECK(g.taps == 1 && !g.a_silu && conv_gemm_can_fuse_rms(g.M, g.N), "conv_gemm: fused RMSNorm needs taps == 1 on the small-M path");
    if (g.dw_wT) SVA_CHECK(g.taps == 1 && g.stride == 1 && g.M <= 16 && g.Cin <= 512 && !g.a_silu && !g.rms_w && !g.w13 && group_n == 1 && g.dw_b && g.ln_w && g.ln_b,
                           "conv_gemm: the fused ConvNeXt prologue needs taps == 1, M <= 16, Cin <= 512");
    bool planes_ok = c_vec;
    for (int i = 0; i < gg.n; ++i) planes_ok = planes_ok && planes_gemm_supported(gg.g[i]);
    // A layer that carries the fp16 fragment-major packing (the content encoder of an enc_dtype = 1 engine) runs on fp16 operands only: the planes
    // kernel in H1 under its rule, the fp16 weight-streaming kernel otherwise -- never an fp32 family; no table, no timed search
    if (g.Wkh) {
        SVA_CHECK(group_n == 1, "conv_gemm: fp16-operand layers take single problems");
        if (wants_planes_h1(g) && planes_ok && g.pmode == PLANES_H1) {
            *out = planes_plan(gg, lead);
            return 0;
        }
        SVA_CHECK(!g.Ap && !g.Cp, "conv_gemm: operand planes handed to a problem the planes kernel does not take");
        SVA_CHECK(stream_h_gemm_supported(g), "conv_gemm: an fp16-operand layer that neither the planes kernel nor the fp16 weight-streaming kernel takes");
        *out = GemmPlan{GemmFamily::StreamH, 0, 0, 0, 1};
        return 0;
    }
    GemmPlan p = heuristic_plan(g, c_vec);
    const ShapeKey key = shape_key(g, group_n);
    const GemmPlan* row = table_row(key);
    if (row && plan_accepts(gg, lead, *row)) p = *row;
    GemmPlan tuned;
    if (debug_options().autotune && tuned_plan(key, &tuned) && plan_accepts(gg, lead, tuned)) p = tuned;      // (the key holds the shape, not the strides)
    // Weights that carry pre-split planes (gemm_planes.hip): H1 by the rule above.  fp32-grade planes (H3: fp16 x 2): where the split kernels are the
    // choice anyway and the batch is large enough for the 128-row tiles to fill the chip (measured: with its tile variant from the measured table it
    // beats the tuned in-loop split kernels on 38 of 40 mid-size shapes, by 5-60 %: profiles/r04_old_vs_planes.txt (full chip); from 3072 rows = 24
    // streams -- below that the pipelined mode runs the encoder on a CU partition the old table was tuned for: 16 streams -2.6 %, 24 / 32 / 48 streams
    // +1 / +1 / +8 %), and the few 2048+-row problems of a 64-stream batch that the table gives to the f32-MFMA kernels: the C = 256 HiFiGAN level's
    // grouped convs -- 5.6 GFLOP per launch at ~60 TF/s there.
    const double gflop = 2e-9 * g.M * (double)g.N * g.taps * g.Cin * group_n;
    const bool want = wants_planes_h1(g) || (g.pmode != PLANES_H1 && g.N >= 64 &&
                                             (p.family == GemmFamily::Split ? g.M >= 3072 : g.M >= 2048 && g.N >= 128 && gflop >= 2.0));
    if (planes_ok && want) p = planes_plan(gg, lead);
    else SVA_CHECK(!g.Ap && !g.Cp, "conv_gemm: operand planes handed to a problem the planes kernel does not take");
    *out = p;
    return 0;
}

static int run_plan(const ConvGemmGroup& gg, const GemmPlan& p, hipStream_t st) {
    const ConvGemm& g = gg.g[0];
    switch (p.family) {
        case GemmFamily::SmallM: return launch_small_m_gemm(gg, p.a, p.b, p.c, p.z, st);
        case GemmFamily::Tiled: return launch_tiled_gemm(gg, p.a, st);
        case GemmFamily::Ring: return launch_pipe_gemm(gg, p.a, st);
        case GemmFamily::Split: return launch_split_gemm(gg, p.a, st);
        case GemmFamily::F16W: return launch_f16w_gemm(g, st);
        case GemmFamily::Stream: return launch_stream_gemm(g, g.Wk ? g.Wk : g.W, p.a, p.c, p.b, g.Wk ? 2 : 0, 0, st);       // (reads the fragment-major weight copy when the problem carries one)
        case GemmFamily::Planes:
        case GemmFamily::PlanesDma: return launch_planes_gemm(gg, p.a, st);
        case GemmFamily::StreamH: return launch_stream_h_gemm(g, 0, 0, 0, st);
    }
    return -1;
}

// SVA_DEBUG=tune_dump=<file>: the shapes tuned by this process are appended as table rows when the library unloads
static void dump_tune_table() {
    if (debug_options().tune_dump.empty()) return;
    FILE* f = fopen(debug_options().tune_dump.c_str(), "a");
    if (!f) return;
    for (const auto& kv : g_tune)
        fprintf(f, "{{%d, %d, %d, %d, %d, %d}, %d, %d, %d, %d, %d},\n", kv.first[0], kv.first[1], kv.first[2], kv.first[3], kv.first[4], kv.first[5],
                table_kind(kv.second), kv.second.a, kv.second.b, kv.second.c, kv.second.z);
    fclose(f);
}
static const int g_tune_dump_registered = (atexit(dump_tune_table), 0);
static float* g_tune_c = nullptr;
static size_t g_tune_elems = 0;

static std::vector<GemmPlan> tune_candidates(const ConvGemmGroup& gg, int lead) {
    const ConvGemm& g = gg.g[lead];
    const int group_n = gg.n;
    const bool c_vec = c_rows_vectorised(g);
    std::vector<GemmPlan> cand;
    const long tiles64 = (long)((g.M + 63) / 64) * ((g.N + 63) / 64);
    const bool must_skinny = g.rms_w || g.dw_wT || !c_vec;
    const int mt_total = (g.M + 15) / 16;
    if (must_skinny || tiles64 < 1024) {
        const long nk = (long)g.taps * g.Cin / 16;
        for (int nt = 1; nt <= 4; nt *= 2) {
            if (g.w13 && nt == 1) continue;
            if (nt == 2 && (g.N % 32 != 0 || g.dw_wT)) continue;
            if (nt == 4 && (g.N % 64 != 0 || g.dw_wT || g.M < 32)) continue;       // 64-column workgroups: a third of the operand reads per output
            const int mts[3] = {1, 2, 4}, kws[3] = {4, 8, 16};
            for (int a = 0; a < 3; ++a)
                for (int b2 = 0; b2 < 3; ++b2) {
                    if (mts[a] > mt_total || (mts[a] >= 2 && kws[b2] == 16) || nk / kws[b2] < 1) continue;
                    if (nt == 4 && kws[b2] == 16) continue;
                    cand.push_back(GemmPlan{GemmFamily::SmallM, mts[a], kws[b2], nt, 1});
                    if (g.rms_w || group_n > 1) continue;
                    const long wgs = (long)((g.N + 16 * nt - 1) / (16 * nt)) * ((mt_total + mts[a] - 1) / mts[a]);
                    for (int z = 2; z <= 8; z *= 2)
                        if (wgs * z <= 512 && nk / ((long)z * kws[b2]) >= 1) cand.push_back(GemmPlan{GemmFamily::SmallM, mts[a], kws[b2], nt, z});
                }
        }
    }
    if (!must_skinny) {
        if (g.N > 32) cand.push_back(GemmPlan{GemmFamily::Tiled, 0, 0, 0, 1});
        if (g.M >= 128 && g.N >= 128) cand.push_back(GemmPlan{GemmFamily::Tiled, 1, 0, 0, 1});
        if (g.M >= 128 && g.N >= 64) cand.push_back(GemmPlan{GemmFamily::Tiled, 4, 0, 0, 1});
        if (g.M >= 64 && g.N >= 128) cand.push_back(GemmPlan{GemmFamily::Tiled, 5, 0, 0, 1});
        if (g.M >= 256 && g.N >= 64) cand.push_back(GemmPlan{GemmFamily::Tiled, 6, 0, 0, 1});
        if (g.M >= 256 && g.N >= 128) cand.push_back(GemmPlan{GemmFamily::Tiled, 7, 0, 0, 1});
        if (g.N <= 64) cand.push_back(GemmPlan{GemmFamily::Tiled, 2, 0, 0, 1});
        if (g.N <= 16 && !g.w13) cand.push_back(GemmPlan{GemmFamily::Tiled, 3, 0, 0, 1});
    }
    if (group_n == 1 && stream_gemm_supported(g) && g.M <= 512 && !g.dw_wT && g.N >= 16) {
        // weight-streaming kernel: (row tiles, column tiles, K-split waves) per workgroup
        const int cfgs[15][3] = {{1, 1, 4}, {1, 1, 8}, {1, 1, 16}, {2, 1, 4}, {2, 1, 8}, {2, 1, 16}, {4, 1, 4}, {4, 1, 8},
                                 {1, 2, 4}, {1, 2, 8}, {1, 2, 16}, {2, 2, 4}, {2, 2, 8}, {4, 2, 4}, {4, 2, 8}};
        for (const auto& cf : cfgs) {
            if (cf[0] > mt_total || (g.w13 && cf[1] != 2) || (cf[1] == 2 && g.N % 32 != 0)) continue;
            cand.push_back(GemmPlan{GemmFamily::Stream, cf[0], cf[2], cf[1], 1});
        }
    }
    if (c_vec && pipe_gemm_supported(g) && g.M >= 32 && g.N >= 32)
        for (int v = 0; v <= 6; ++v) {
            if (v == 4 && (g.M < 128 || g.N < 128)) continue;
            if ((v == 2 && g.M < 128) || ((v == 3 || v == 5) && g.N < 128)) continue;
            cand.push_back(GemmPlan{GemmFamily::Ring, v, 0, 0, 1});
        }
    if (c_vec && split_gemm_supported(g) && g.M >= 64 && g.N >= 64)
        for (int v = 0; v <= 4; ++v) {
            if ((v == 0 || v == 1 || v == 4) && g.M < 128) continue;
            if ((v == 0 || v == 2 || v == 4) && g.N < 128) continue;
            cand.push_back(GemmPlan{GemmFamily::Split, v, 0, 0, 1});
        }
    return cand;
}

// Shape-keyed: the first eager launch of a problem shape times the candidate kernels / configurations on the real operands with the output
// redirected to scratch, and keeps a candidate only if it beats the planner's choice among the fp32 families by > 7 %.  Launches inside a stream
// capture (and shapes first seen there) keep the planner's choice.  The planes rule of the planner applies on top of the pick.
static int tune_conv_gemm(const ConvGemmGroup& gg, int lead, hipStream_t st) {
    const ConvGemm& g = gg.g[lead];
    const ShapeKey key = shape_key(g, gg.n);
    GemmPlan ch;
    if (tuned_plan(key, &ch)) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return 0;
    // the baseline: the planner's choice for the problem without its weight planes (table or heuristic)
    ConvGemmGroup tg = gg;
    for (int i = 0; i < tg.n; ++i) tg.g[i].Wp = nullptr;
    SVA_TRY_RC(plan_conv_gemm(tg, lead, &ch));
    std::lock_guard<std::mutex> lk(g_tune_mu);
    if (g_tune.count(key)) return 0;
    const int ldc = g.w13 ? g.N / 2 : g.N;
    const size_t need = (size_t)g.M * ldc * (size_t)gg.n;
    if (need > g_tune_elems) {
        if (g_tune_c) (void)hipFree(g_tune_c);
        SVA_HIP(hipMalloc((void**)&g_tune_c, need * sizeof(float)));
        g_tune_elems = need;
    }
    // a group is timed as a group, every member's output redirected to its own scratch slab
    tg = gg;
    for (int i = 0; i < tg.n; ++i) {
        tg.g[i].C = g_tune_c + (size_t)i * g.M * ldc; tg.g[i].c_bstride = (long)g.T * ldc; tg.g[i].c_off = 0; tg.g[i].ldc = ldc;
    }
    hipEvent_t e0, e1;
    SVA_HIP(hipEventCreate(&e0)); SVA_HIP(hipEventCreate(&e1));
    // measured alone on the device (other streams drained first) and as the better of two batches: the pick should
    // not depend on what happened to run beside the probe
    SVA_HIP(hipDeviceSynchronize());
    auto time_plan = [&](const GemmPlan& c, float* ms) -> int {
        SVA_TRY_RC(run_plan(tg, c, st));
        float best_ms = 1e30f;
        for (int rep = 0; rep < 2; ++rep) {
            SVA_HIP(hipEventRecord(e0, st));
            for (int r = 0; r < 5; ++r) SVA_TRY_RC(run_plan(tg, c, st));
            SVA_HIP(hipEventRecord(e1, st));
            SVA_HIP(hipEventSynchronize(e1));
            float m = 0.f;
            SVA_HIP(hipEventElapsedTime(&m, e0, e1));
            if (m < best_ms) best_ms = m;
        }
        *ms = best_ms;
        return 0;
    };
    float base = 0.f;
    SVA_TRY_RC(time_plan(ch, &base));
    float best = base * 0.93f;
    for (const GemmPlan& c : tune_candidates(gg, lead)) {
        if (c.family == ch.family && c.a == ch.a && c.b == ch.b && c.c == ch.c && c.z == ch.z) continue;
        float ms = 0.f;
        SVA_TRY_RC(time_plan(c, &ms));
        if (ms < best) { best = ms; ch = c; }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (debug_options().tune_log)
        fprintf(stderr, "[sva tune] M=%d N=%d K=%d taps=%d flags=%llu: heuristic %.1f us -> kind %d (%d,%d,%d) z%d %.1f us\n", g.M, g.N,
                g.taps * g.Cin, g.taps, (unsigned long long)key[4], base * 200.f, table_kind(ch), ch.a, ch.b, ch.c, ch.z, (best < base * 0.93f ? best : base) * 200.f);
    g_tune[key] = ch;
    return 0;
}

int launch_conv_gemm_group(const ConvGemm* gs, int n, hipStream_t st, int* kind_out) {
    ConvGemmGroup gg;
    int lead = 0;
    SVA_TRY_RC(conv_gemm_group_of(gs, n, &gg, &lead));
    const ConvGemm& g = gg.g[lead];
    GemmPlan p;
    SVA_TRY_RC(plan_conv_gemm(gg, lead, &p));
    static const bool tune = debug_options().autotune != 0;
    // (a problem with one family -- fp16 weights, fp16 operands, operands as planes -- is not searched: its variant comes from its own rule)
    if (tune && p.family != GemmFamily::F16W && !g.Wkh && !g.Ap && !g.Cp) {
        SVA_TRY_RC(tune_conv_gemm(gg, lead, st));
        SVA_TRY_RC(plan_conv_gemm(gg, lead, &p));
    }
    SVA_TRY_RC(run_plan(gg, p, st));
    if (kind_out) *kind_out = plan_report_kind(p, g.pmode);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_conv_gemm(const ConvGemm& g, hipStream_t st, int* kind_out) { return launch_conv_gemm_group(&g, 1, st, kind_out); }

// test / bench hooks: run one given plan on a problem or a group, under the planner's own preconditions and plan_accepts
int launch_conv_gemm_group_plan(const ConvGemm* gs, int n, const GemmPlan& p, hipStream_t st) {
    ConvGemmGroup gg;
    int lead = 0;
    SVA_TRY_RC(conv_gemm_group_of(gs, n, &gg, &lead));
    const ConvGemm& g = gg.g[lead];
    SVA_CHECK(g.Cin > 0 && g.Cin % 16 == 0 && g.M > 0 && g.N > 0 && g.T > 0 && g.lda % 4 == 0 && g.a_off % 4 == 0 && g.a_bstride % 4 == 0 &&
              (!g.w13 || g.N % 32 == 0) && plan_accepts(gg, lead, p),
              "conv_gemm_plan: the kernel family does not take this problem in this configuration");
    SVA_TRY_RC(run_plan(gg, p, st));
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_conv_gemm_plan(const ConvGemm& g, const GemmPlan& p, hipStream_t st) { return launch_conv_gemm_group_plan(&g, 1, p, st); }

}  // namespace sva
