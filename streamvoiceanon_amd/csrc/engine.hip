// sva engine: per-batch state, stream / graph orchestration and the per-chunk step of the streaming
// voice-conversion hot path (content encoder -> dual AR -> Firefly vocoder) on MI355X.
//
// Host-side control flow mirrors evaluations/infer_arvc.py InferenceWrapper.{prefill_prompt,
// setup_stream_caches, process_one_chunk} (:443-596) and modules/dual_ar_stream.py
// DualARWrapper.{prefill_prompt, prefill_src_condition4delay, decode_one} (:764-837); the
// arithmetic runs in the HIP kernels of gemm.hip / kernels.hip.
#include "engine_internal.h"
#include "engine_kernels.h"
#include "io/resample.h"
#include "snapshot/slot_pack.h"
#include "snapshot/snapshot_format.h"
#include <map>
#include <mutex>

#include <math.h>
#include <cmath>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>

namespace sva {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

}  // namespace sva

using namespace sva;

// joins the AR / vocoder streams of the pipelined mode back into the main stream (no-op when nothing is in flight there)
namespace sva {
static void parse_debug(DebugOptions& o, const char* env) {
    if (!env) return;
    std::string all(env);
    size_t pos = 0;
    while (pos <= all.size()) {
        const size_t end = std::min(all.find(',', pos), all.size());
        const std::string kv = all.substr(pos, end - pos);
        const size_t eq = kv.find('=');
        if (eq != std::string::npos) {
            const std::string k = kv.substr(0, eq), v = kv.substr(eq + 1);
            if (k == "ar_timing") o.ar_timing = atoi(v.c_str());
            else if (k == "pipe_trace") o.pipe_trace = atoi(v.c_str());
            else if (k == "concurrency") o.concurrency = atoi(v.c_str());
            else if (k == "ar_persistent") o.ar_persistent = atoi(v.c_str());
            else if (k == "ar_batch") o.ar_batch = atoi(v.c_str());
            else if (k == "ar_batch_wgs") o.ar_batch_wgs = atoi(v.c_str());
            else if (k == "planes_dbg") o.planes_dbg = atoi(v.c_str());
            else if (k == "reprefill") o.reprefill = atoi(v.c_str());
            else if (k == "planes_dma") o.planes_dma = atoi(v.c_str());
            else if (k == "voc_dma") o.voc_dma = atoi(v.c_str());
            else if (k == "voc_dma_variant") o.voc_dma_variant = atoi(v.c_str());
            else if (k == "planes_lw") o.planes_lw = atoi(v.c_str());
            else if (k == "planes_min_streams") o.planes_min_streams = atoi(v.c_str());
            else if (k == "ar_graph") o.ar_graph = atoi(v.c_str());
            else if (k == "ar_pairs") o.ar_pairs = atoi(v.c_str());
            else if (k == "head_fuse") o.head_fuse = atoi(v.c_str());
            else if (k == "voc_fused_mask") o.voc_fused_mask = atoi(v.c_str());
            else if (k == "hist_cap") o.hist_cap = atoi(v.c_str());
            else if (k == "autotune") o.autotune = atoi(v.c_str());
            else if (k == "tune_log") o.tune_log = atoi(v.c_str());
            else if (k == "tune_table") o.tune_table = atoi(v.c_str());
            else if (k == "tune_kinds") o.tune_kinds = atoi(v.c_str());
            else if (k == "f16_weights") o.f16_weights = atoi(v.c_str());
            else if (k == "cu_partition") o.cu_partition = atoi(v.c_str());
            else if (k == "cu_ar") o.cu_ar = atoi(v.c_str());
            else if (k == "stream_queues") o.stream_queues = atoi(v.c_str());
            else if (k == "pipe_skip") o.pipe_skip = atoi(v.c_str());
            else if (k == "tune_dump") o.tune_dump = v;
            else fprintf(stderr, "[sva] debug option '%s' unknown, ignored\n", k.c_str());
        }
        pos = end + 1;
    }
}
static DebugOptions& debug_options_mut() {
    // never destroyed: the tuning dump (an atexit handler registered before this object exists) reads it during process teardown
    static DebugOptions& opt = *new DebugOptions([] { DebugOptions o; parse_debug(o, getenv("SVA_DEBUG")); return o; }());
    return opt;
}
const DebugOptions& debug_options() { return debug_options_mut(); }
}  // namespace sva

namespace { int quiesce(sva_batch* b); }

// Recovery from a persistent-kernel timeout (called by sva_prefill_prompt / sva_streams_begin): clear the device flag, leave the
// persistent kernel for the multi-launch decode (whatever kept its workgroups from being co-resident may still be there), drop the
// graphs that captured its launches, and require fresh prompts: the KV caches and positions of the failed frames are garbage.
static int recover_ar_failure(sva_batch* b) {
    if (!b->ar_failed) return 0;
    SVA_HIP(hipDeviceSynchronize());
    SVA_HIP(hipMemset(b->d_ar_fail, 0, sizeof(int)));
    if (b->h_ar_fail) *b->h_ar_fail = 0;
    b->use_mega = false;
    b->use_abatch = false;
    for (auto& ge : b->pipe_graph_a) if (ge) { (void)hipGraphExecDestroy(ge); ge = nullptr; }
    if (b->graph_exec) { (void)hipGraphExecDestroy(b->graph_exec); b->graph_exec = nullptr; }
    b->slots.forget_prompts();
    b->begun = false;
    b->ar_failed = false;
    return 0;
}

// ============================================================================================
// config defaults
// ============================================================================================
extern "C" const char* sva_last_error(void) { return g_err.c_str(); }


// ============================================================================================
// batch
// ============================================================================================

namespace {
struct StreamSet { hipStream_t main = nullptr, aux0 = nullptr, sa = nullptr, sv = nullptr; };
std::mutex g_streams_mu;
std::map<int, StreamSet> g_streams;          // per device, process lifetime
// `partitioned`: the AR stream and the encoder / vocoder streams get disjoint compute-unit masks (hipExtStreamCreateWithCUMask;
// mask bit i -> XCD i % 8, so every range is spread over all XCDs).  With few streams the three stage chains are strings of
// short dependent kernels that each leave most of the chip idle, yet when they share CUs the AR chain's kernels queue behind
// the encoder's and vocoder's workgroups.  The gain shrinks with the batch (and wants a smaller AR share as it grows) and turns
// into a loss beyond 32 streams, where the GEMMs want the whole chip.  SVA_DEBUG=cu_partition=0|1[,cu_ar=N] overrides for A/B runs.
//
// Hardware queues.  The runtime multiplexes plain streams onto a pool of hardware queues (4 unless the process environment said
// otherwise before the runtime started -- which a library loaded into a host application cannot count on), the host application's
// streams included, and two streams on one hardware queue serialise.  The four chains of the pipelined step must not: with a pool
// of 4 and four plain streams the single-stream step ran at 630 frames/s against 1070 with a pool of 8, 64 streams at 7880 against
// 8580 (profiles/hw_queues_report.txt).  So the unpartitioned set (variant 0) is provisioned by construction:
//   SQ_PRIO  (the default) the AR and the vocoder stream at the highest stream priority, main and the encoder side stream at normal
//            priority, all hipStreamNonBlocking.  The runtime keeps one pool PER priority level and hands a new stream the entry with
//            the fewest users, so the two pairs cannot meet and two streams of a pair share an entry only when the host application
//            itself keeps more than pool - 2 streams at that level.  Measured at a pool of 4 under torch: all six pairs concurrent
//            (tests/test_gpu_stream_queues.py), 1065-1074 frames/s at one stream, 8550-8720 at 64.
//   SQ_MASK  CU-masked streams with every CU enabled: a queue each outside the pool (what the partitioned variants get anyway).  Same
//            throughput (1070 / 8690), but the runtime creates a CU-masked stream with the DEFAULT flags: it synchronises with the
//            legacy null stream, i.e. with a host application's torch work, and costs four more hardware queues.  Not the default.
//   SQ_PLAIN four plain non-blocking streams (the behaviour before; each stream's fallback when the chosen call fails).
// SVA_DEBUG=stream_queues=0|1|2 picks plain / mask / prio for A/B runs (tools/hwq_ab.sh; tools/micro/stream_queues.hip is the
// stand-alone probe of the three).  ops_stream and the test hooks' streams stay plain.
// Hardware queues a process can end up with: the pools (4 entries per priority level in use: normal + highest = 8, shared with the
// host application) + 4 dedicated ones per LIVE partitioned variant (the policy uses the 1-stream split and 64 / 96 / 128 AR CUs: 16
// if one process ever creates all four, 4 in a process that serves one partitioned batch size) = 8 to 12 as a rule, 24 at the very
// most, under the 32 the runtime allows a process; SQ_MASK would add 4.
enum { SQ_PLAIN = 0, SQ_MASK = 1, SQ_PRIO = 2 };
constexpr int kStreamQueues = SQ_PRIO;
int get_streams(int device, int n_streams_if_pipelined, StreamSet* out, int ar_cus = 96) {
    std::lock_guard<std::mutex> lk(g_streams_mu);
    // variant 1 (one stream): AR 96 CUs | encoder 128 | vocoder 32 (12 / 16 / 4 per XCD) -- 2.11 -> 1.75 ms per step, 1.60 with the
    // encoder split; 96/136/24 measures the same but leaves the vocoder no slack (96/138/22 and 92/140/24 lose the whole gain:
    // the AR GEMV grids are multiples of 96 workgroups, the vocoder is throughput-bound on its share).  Two streams and more: AR
    // `ar_cus` CUs | encoder and vocoder share the rest (the three-way split is worse there); the caller picks ar_cus by batch size.
    bool partitioned = n_streams_if_pipelined >= 1;
    int variant = !partitioned ? 0 : n_streams_if_pipelined == 1 ? 1 : ar_cus;      // (a stream set per split, created on first use)
    int part[6] = {0, 96, 96, 160, 96, 160};
    if (variant == 1) { part[3] = 128; part[4] = 224; part[5] = 32; }
    if (variant > 1) {
        const int n = std::min(std::max(ar_cus & ~7, 32), 224);
        part[1] = n; part[2] = part[4] = n; part[3] = part[5] = 256 - n;
        variant = n;
    }
    int cus = 0;
    SVA_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    if (partitioned && cus != 256) partitioned = false;         // the ranges are sized for the 256 CUs of an MI355X
    if (!partitioned) variant = 0;
    StreamSet& s = g_streams[device * 256 + variant];
    if (!s.main) {
        const int sq = debug_options().stream_queues >= 0 ? debug_options().stream_queues : kStreamQueues;
        int prio_least = 0, prio_greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) { (void)hipGetLastError(); prio_least = prio_greatest = 0; }
        // a failed call of either kind: clear the error, plain non-blocking stream (no partition / the shared pool)
        auto make = [&](hipStream_t* st, int lo, int n, bool high) -> int {
            *st = nullptr;
            if (!partitioned && sq == SQ_PRIO && prio_greatest < prio_least) {
                if (hipStreamCreateWithPriority(st, hipStreamNonBlocking, high ? prio_greatest : 0) == hipSuccess) return 0;
                (void)hipGetLastError();
                *st = nullptr;
            }
            if (!partitioned && sq == SQ_MASK) { lo = 0; n = cus; }        // every CU: only the queue of its own is wanted
            if ((partitioned && n > 0 && n < 256) || (!partitioned && sq == SQ_MASK && n > 0 && n <= 256)) {
                uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (int i = lo; i < lo + n && i < 256; ++i) mask[i >> 5] |= 1u << (i & 31);
                if (hipExtStreamCreateWithCUMask(st, partitioned ? 8 : (uint32_t)((n + 31) / 32), mask) == hipSuccess) return 0;
                (void)hipGetLastError();
                *st = nullptr;
            }
            SVA_HIP(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
            return 0;
        };
        SVA_TRY(make(&s.main, part[2], part[3], false));
        SVA_TRY(make(&s.aux0, part[2], part[3], false));
        SVA_TRY(make(&s.sa, part[0], part[1], true));
        SVA_TRY(make(&s.sv, part[4], part[5], true));
    }
    *out = s;
    return 0;
}
}  // namespace

// batch sizes the batched persistent decode kernel (ar_batch.hip) serves: where it beats both the two-streams-per-launch kernel
// (ar_decode.hip, below) and the multi-launch decode (above).  Pipelined (throughput) mode, fp32 AR: 4-24 streams (4: 1681 vs 1632
// frames/s, 5: 2064 vs 1654, 6: 2421 vs 1914, 8: 2949 vs 2508, 16: 4439 vs 4133, 32: 5288 vs 5419); fp16 AR: 3-11 (3: 1624 vs 1487, 4: 2071
// vs 1914, 8: 3440 vs 3197, 12: 4059 vs 4110); with several frames per step (chunk > 1) the decode is the step's longest stage and the
// kernel serves up to 32 streams (32 x chunk 4: 7763 vs 6341 frames/s).  A caller that synchronises every chunk sees the kernel's
// ~2.1-2.3 ms frame against 1.75 ms for two launches of the two-stream kernel: there it starts at 5 streams
// (profiles/r04_small_batch_ab.txt, r04_abatch_sweep in the comments above).  SVA_DEBUG ar_batch=0 never, ar_batch=2 every size it can run
// (a GROUP form of the persistent kernel -- 2-4 streams sharing each phase's weight registers and hand-offs on one set of 96 workgroups --
// was built in round 4, measured slower than this policy at every size and removed in round 5: profiles/r04_group_ab.txt, git history)
// The PIPELINED-mode policy -- which decode serves a batch of B streams (the batched persistent kernel or the multi-launch chain) and how many
// CUs the AR chain's stream owns when it is the chain -- is a GENERATED table: tools/make_policy.py sweeps the candidates on the GPU
// (frames/s of bench.py per stream count x decode x CU partition; log under profiles/) and emits policy_table.inc, so a kernel change
// re-derives every threshold with one command instead of hand-edited constants.  A batch takes the row of the largest
// measured stream count <= its own (same AR precision, same chunk class).
struct PolicyRow { int ar_dtype, chunk_gt1, B, decode, cu_ar; };       // decode: 0 multi-launch chain, 2 batched persistent kernel; cu_ar: 0 = no partition
static const PolicyRow kPolicy[] = {
#include "policy_table.inc"
};
static const PolicyRow* policy_row(int B, int ar_dtype, int chunk) {
    const PolicyRow *below = nullptr, *smallest = nullptr;
    for (const PolicyRow& r : kPolicy) {
        if (r.ar_dtype != ar_dtype || r.chunk_gt1 != (chunk > 1 ? 1 : 0)) continue;
        if (r.B <= B && (!below || r.B > below->B)) below = &r;
        if (!smallest || r.B < smallest->B) smallest = &r;
    }
    return below ? below : smallest;          // (fewer streams than any measured row: the smallest one)
}
// smallest pipelined stream count the batched kernel serves = one more than what the per-stream persistent kernel (ar_decode.hip) takes
static int abatch_lo(int ar_dtype, bool pipelined) { return pipelined ? (ar_dtype == 1 ? 3 : 4) : 5; }
static bool abatch_serves(int B, int ar_dtype, bool pipelined, int chunk) {
    const int mode = debug_options().ar_batch;
    if (mode == 0 || B > AR_BATCH_MAX_STREAMS) return false;
    if (mode == 2) return true;
    if (B < abatch_lo(ar_dtype, pipelined)) return false;
    if (!pipelined) return B <= 32;           // a caller that synchronises every chunk: one launch per frame from 5 streams (profiles/r04_small_batch_ab.txt)
    const PolicyRow* r = policy_row(B, ar_dtype, chunk);
    return r ? r->decode == 2 : B <= 32;
}

// The form of HiFiGAN level `level` (C = ch, rpf rows per code frame) of a batch of B streams and Tv code frames per call.
// Fused (voc_fused.hip): measured on MI355X (profiles/r02_voc_fused.txt), the C = 16 level takes 27-33 us fused against 7 launches / ~70 us at
// one stream and breaks even around 4-8 streams; from there on, and for C = 32 at any batch, the tap-split GEMM formulation is faster (the fused
// kernel recomputes an 18 (k - 1)-row halo per tile and runs one workgroup per CU), so the default fuses C = 16 for <= 4 streams.
// SVA_DEBUG=voc_fused_mask=M (bit 0: C = 16, bit 1: C = 32) / sva_debug_configure override it for the parity tests.
// Planes: every other level of a batch with enough rows per step runs its 18 ResBlock convs on operand planes, three branches per launch, the
// activations between them as planes (history included).  From 10 code frames per step over the batch (streams x voc_max_frames): +4.7 / +5.7 /
// +6.7 / +5.2 / +3.9 % frames/s at 16 / 24 / 32 / 48 / 128 streams, +2 % and a 6 % shorter synchronous step at 10 / 12, even at 8
// (profiles/r05_voc_dma_sweep.txt).  C = 16 / 32: row-major planes + voc_conv_kernel (the input rows of a tile and the branch's whole weight
// resident in LDS); wider: K-blocked planes + the LDS-DMA GEMM's conv form.  A level whose weights lack the planes of its form stays on fp32 rows.
static int voc_planes_mode(const sva_config& c) { return c.voc_dtype == 1 ? PLANES_H1 : (c.mm_mode == 1 ? PLANES_H3 : -1); }
static VocForm voc_level_form(const sva_engine* e, int level, int ch, int rpf, int B, int Tv) {
    const DebugOptions& o = debug_options();
    if (voc_level_supported(ch) && (o.voc_fused_mask >= 0 ? (o.voc_fused_mask & (ch == 16 ? 1 : 2)) != 0 : ch == 16 && B <= 4)) return VocForm::Fused;
    const int pm = voc_planes_mode(e->cfg);
    if (!(ch % 16 == 0 && pm >= 0 && o.planes_dma != 0 && o.voc_dma != 0 && (o.voc_dma == 1 || (long)B * Tv >= 10))) return VocForm::Rows;
    const bool halo = ch <= 32 && voc_conv_supported(ch, rpf, pm);
    for (const auto& branch : e->res[level])
        for (const ResConv& rcv : branch)
            if (halo ? !(rcv.q1 && rcv.q2) : !(ch % 64 == 0 && rcv.c1.Wp && rcv.c2.Wp && rcv.c1.pmode == pm && rcv.c2.pmode == pm)) return VocForm::Rows;
    return halo ? VocForm::PlanesHalo : VocForm::PlanesDma;
}

// The vocoder workspace of batch b: activations with their history rows, operand planes, the ShiftDesc table, code and PCM buffers for up to
// Tv code frames per call.  Every level's form is derived from the batch (owner == nullptr), or taken over from the workspace `owner` of the
// batch that owns b as its priming workspace: the history rows of the two must be the same rows in the same layout, whatever B = 1 and its Tv
// would have chosen.
static int alloc_vocoder(sva_batch* b, int Tv, const VocWorkspace* owner) {
    sva_engine* e = b->e;
    const sva_config& c = e->cfg;
    auto& A = b->allocs;
    VocWorkspace& v = b->voc;
    const int B = b->B, V = c.voc_dim, ncb = c.num_codebooks;
    v.Tv = Tv;
    SVA_TRY(dev_alloc(A, &v.d_frames, 1));
    SVA_TRY(alloc_act(A, v.zq, B, 0, Tv, V));
    SVA_TRY(alloc_act(A, v.u0, B, 6, 2L * Tv, V));
    SVA_TRY(alloc_act(A, v.v0, B, 0, 2L * Tv, V));
    SVA_TRY(alloc_act(A, v.u1, B, 6, 4L * Tv, V));
    SVA_TRY(alloc_act(A, v.pin, B, e->pre_k - 1, 4L * Tv, V));
    SVA_TRY(dev_alloc(A, &v.vh1, (size_t)B * 4 * Tv * V));
    SVA_TRY(dev_alloc(A, &v.vh2, (size_t)B * 4 * Tv * 4 * V));
    SVA_TRY(alloc_act(A, v.S[0], B, 1, 4L * Tv, V));
    long rows = 4L * Tv;
    int rpf = 4;
    int ch = V;
    for (int i = 0; i < 5; ++i) {
        VocLevel& l = v.lv[i];
        rows *= e->ups_s[i];
        rpf *= e->ups_s[i];
        ch /= 2;
        l.rpf = rpf;
        l.form = owner ? owner->lv[i].form : voc_level_form(e, i, ch, rpf, B, Tv);
        if (voc_form_planes(l.form)) v.pmode = voc_planes_mode(c);
        // every streaming tensor of the level, in a planes form followed by its operand planes.  The allocation keeps a loop of its own beside
        // for_each_voc_state: the stateless tensors (zq, v0, y3, the scratch) lie between the streaming ones, and the order in the arena is part
        // of the measured behaviour (all streaming tensors first: -0.3 % frames/s at one stream, profiles/voc_workspace_refactor_ab.txt)
        auto alloc = [&](Act& a, unsigned short*& P, int H) -> int {
            SVA_TRY(alloc_act(A, a, B, H, rows, ch));
            return voc_form_planes(l.form) ? dev_alloc(A, &P, (size_t)planes_count(v.pmode) * B * a.bstride) : 0;
        };
        // fused levels keep the receptive field of the whole six-conv chain as input history (their only streaming state)
        SVA_TRY(alloc(l.X, l.XP, l.form == VocForm::Fused ? (kResK[2] - 1) * 2 * (kResD[0] + kResD[1] + kResD[2]) : (kResK[2] - 1) * kResD[0]));
        for (int br = 0; br < 3; ++br)
            for (int j = 0; j < 3; ++j) {
                SVA_TRY(alloc(l.tb[br][j], l.tbP[br][j], (kResK[br] - 1) * kResD[j]));
                if (j < 2) SVA_TRY(alloc(l.yb[br][j], l.ybP[br][j], (kResK[br] - 1) * kResD[j + 1]));
            }
        for (int br = 0; br < 3; ++br) SVA_TRY(alloc_act(A, l.y3[br], B, 0, rows, ch));
        SVA_TRY(alloc_act(A, v.S[i + 1], B, i < 4 ? 1 : e->post_k - 1, rows, ch));
    }
    // the ShiftDesc table: the fp32 rows themselves, or in a planes form the tensor's operand planes
    SVA_TRY(for_each_voc_state(v, [&](Act& a, unsigned short*& P, int rpf, VocForm form) -> int {
        if (!voc_form_planes(form)) return register_shift(b, a, rpf);
        for (int p = 0; p < planes_count(v.pmode) && a.H > 0; ++p) {
            ShiftDesc d;
            d.H = a.H; d.T = 0; d.pad = rpf;
            if (form == VocForm::PlanesHalo) {       // row-major plane: a [B][rows][C / 2 floats] tensor
                d.ptr = reinterpret_cast<float*>(P + (size_t)p * B * a.bstride);
                d.bstride = a.rows * (a.C / 2); d.C = a.C / 2;
                v.shift_host.push_back(d);
                continue;
            }
            // K-blocked: the history rows of every (plane, 32-channel block) shift like a [B][rows][16 floats] tensor of its own
            for (int kb = 0; kb < a.C / 32; ++kb) {
                d.ptr = reinterpret_cast<float*>(P + (size_t)p * B * a.bstride + (size_t)kb * B * a.rows * 32);
                d.bstride = a.rows * 16; d.C = 16;
                v.shift_host.push_back(d);
            }
        }
        return 0;
    }));
    SVA_TRY(dev_alloc(A, &v.d_pcm, (size_t)B * 2048 * Tv));
    SVA_TRY(dev_alloc(A, &v.d_vcodes, (size_t)B * ncb * Tv));
    SVA_TRY(dev_alloc(A, &v.d_shift, v.shift_host.size()));
    return 0;
}

// Slot-local activation (sva_stream_params.slot_priming): the one-stream vocoder a restarted slot's state is primed in.  An internal sva_batch
// = a launch context (the owner's stream, CU limit and fp16-range overflow flag, B = 1) + a vocoder workspace in the owner's forms.  Allocated
// with the owner so that no activating step allocates; freed by sva_batch_destroy(owner).
static int create_priming_workspace(sva_batch* b) {
    const int chunk = b->p.chunk_frames;
    const int Tv = ((b->p.decode_window_frames - 1) / chunk) * chunk;
    SVA_CHECK(b->p.slot_priming == 1, "slot_priming must be 0 or 1");
    SVA_CHECK(Tv >= 1, "slot_priming: decode_window_frames - 1 holds no whole chunk to prime with");
    sva_batch* w = new sva_batch();
    for (auto& ev : w->evpool) ev = nullptr;
    for (auto& ev : w->ev) ev = nullptr;
    b->prime_ws = w;                        // (owned from here on: a failure below is cleaned up with the owner)
    w->e = b->e;
    w->p = b->p;
    w->p.n_streams = 1; w->p.slot_priming = 0; w->p.voc_max_frames = Tv; w->p.pipeline = 0; w->p.use_graph = 0;
    w->B = 1;
    w->stream = w->main_stream = w->out_stream = b->main_stream;
    w->aux0 = b->aux0;
    w->concurrency = b->concurrency;
    w->enc_cus = b->enc_cus;
    w->d_mm_ovf = b->d_mm_ovf;              // (h_mm_ovf stays null here: the owner polls and frees the flag)
    for (int i = 0; i < 64; ++i) SVA_HIP(hipEventCreateWithFlags(&w->evpool[i], hipEventDisableTiming));
    SVA_TRY(alloc_vocoder(w, Tv, &b->voc));
    // the move kernel walks the two ShiftDesc tables in parallel: refuse anything but the same state in the same form here, not in an activating step
    auto state = [](VocWorkspace& v) {
        std::vector<std::array<int, 5>> s;
        for_each_voc_state(v, [&](Act& a, unsigned short*& P, int rpf, VocForm form) -> int {
            s.push_back({a.H, a.C, rpf, (int)form, P != nullptr});
            return 0;
        });
        return s;
    };
    SVA_CHECK(state(w->voc) == state(b->voc) && w->voc.pmode == b->voc.pmode && w->voc.shift_host.size() == b->voc.shift_host.size(),
              "slot_priming: the priming workspace's vocoder state is not in the form of the batch's (history descriptors differ)");
    SVA_HIP(hipMemcpy(w->voc.d_shift, w->voc.shift_host.data(), sizeof(ShiftDesc) * w->voc.shift_host.size(), hipMemcpyHostToDevice));
    return 0;
}

static int batch_create_impl(sva_engine* e, const sva_stream_params* p, sva_batch* b);

extern "C" int sva_batch_create(sva_engine* e, const sva_stream_params* p, sva_batch** out) {
    SVA_CHECK(e && p && out && e->finalized, "engine not finalized");
    SVA_HIP(hipSetDevice(e->device));
    (void)hipGetLastError();
    sva_batch* b = new sva_batch();
    for (auto& ev : b->evpool) ev = nullptr;
    for (auto& ev : b->ev) ev = nullptr;
    b->e = e;
    const int rc = batch_create_impl(e, p, b);
    if (rc) {                      // nothing of a half-built batch survives (events, arena chunks, pinned buffers)
        const std::string msg = sva_last_error();
        sva_batch_destroy(b);
        set_error(msg);
        return rc;
    }
    *out = b;
    return 0;
}

static int batch_create_impl(sva_engine* e, const sva_stream_params* p, sva_batch* b) {
    const sva_config& c = e->cfg;
    b->p = *p;
    const int B = b->B = p->n_streams;
    SVA_CHECK(B >= 1 && p->chunk_frames >= 1 && p->delay >= 1 && p->delay <= c.max_delay, "bad stream params (delay 0 is broken upstream too)");
    // a re-prefill rebuilds [speaker prefix | 2 x (truncated prompt + buffer_frames)] + the delay fill in one slot's cache (infer_arvc.py:547-564)
    SVA_CHECK(c.timbre_tokens + 1 + 2 * (p->max_prompt_frames + p->buffer_frames) + 2 * p->delay <= c.max_seq_len,
              "max_prompt_frames + buffer_frames do not fit the KV cache: a re-prefill would overrun the slot");
    SVA_CHECK(p->encode_window_frames % 1 == 0 && p->encode_window_frames >= p->chunk_frames, "bad encode window");
    if (b->p.voc_max_frames < p->chunk_frames) b->p.voc_max_frames = p->chunk_frames;
    // Streams come from a process-wide set per device, created once in a fixed order (main, encoder side stream, AR,
    // vocoder) and shared by every batch: the runtime multiplexes streams onto a few hardware queues (4 by default),
    // two streams on one hardware queue serialise (a stream stuck behind another one's event wait blocks
    // its queue mates), and streams created after others were destroyed land on unlucky queues -- measured: the pipelined
    // mode gains 16 % at 64 streams in a fresh process and nothing after one create / destroy cycle.  Batches that are
    // alive at the same time therefore share the streams (in-order, so still correct), and get_streams keeps the four
    // chains on four hardware queues whatever the size of that pool.
    {
        StreamSet ss;
        // one stream with the persistent AR decode kernel: no CU partition -- that kernel is a single launch of 96 workgroups that
        // mostly wait on hand-offs, so the AR chain no longer queues behind the other stages' workgroups, and the encoder /
        // vocoder GEMMs want the whole chip (measured 1.41 ms per step with the 96 | 128 | 32 split, 1.13 without)
        // (fp16 AR: the batched decode on the f16 pipes overtakes the persistent kernel at 5 streams -- 2191 vs 1645 frames/s, 6: 2562 vs
        // 2064, 4: 1420 vs 1919; fp32: the persistent kernel wins up to 6 -- the round-3 partition A/B scripts, git history)
        int mega_max = debug_options().ar_batch == 0 ? (c.ar_dtype == 1 ? std::min(4, AR_PERSISTENT_MAX_STREAMS) : AR_PERSISTENT_MAX_STREAMS)
                                                     : std::min(abatch_lo(c.ar_dtype, b->p.pipeline != 0) - 1, AR_PERSISTENT_MAX_STREAMS);
        const bool will_mega = B <= mega_max && e->mega_ok && debug_options().ar_persistent != 0 && debug_options().ar_batch != 2;
        b->mega_max = mega_max;
        // multi-launch decode (more than 6 streams): its ~265 small launches per frame are a latency chain that the encoder's and
        // vocoder's chip-filling GEMMs would otherwise queue in front of -- disjoint CU masks (AR n | encoder + vocoder 256 - n)
        // win up to 32 streams, with a smaller AR share as the batch grows (the round-3 partition A/B scripts, git history, round-3 A/B;
        // profiles/r03_partition_ab.txt -- fp32 AR: 8 streams 1873 unpartitioned / 2206 with 96 CUs / 2497 with 128; 12: 2683 / 3422
        // with 96; 24: 3960 / 4312 with 64; 32: 5008 / 5322 with 64; 48: 5725 / 5628.  fp16 AR: 12: 3053 / 3989 with 64; 16: 3682 /
        // 4234; 24: 4415 / 4884; 32: 5337 / 5421).  Round 2 partitioned 7-8 streams only, always 96 | 160.
        // batched persistent decode kernel (ar_batch.hip; the range it serves: batch_create_impl): no CU partition either -- its 72
        // workgroups of 8 waves x 256 registers fill 72 CUs by themselves and leave the other 184 to the encoder and the vocoder
        // (pipelined, fp32 AR, unpartitioned vs the multi-launch decode on its best partition: 8 streams 3066-3169 vs 2538 frames/s,
        // 12: 3761-3795 vs 3463, 16: 4465 vs 4166, 24: 4839 vs 4223, 32: 5288 vs 5419; on 64 / 96 / 128-CU partitions it loses 3-20 %;
        // fp16 AR: 6 streams 2989 vs 2664, 8: 3440 vs 3197, 12: 4059 vs 4110 -- profiles/r04_abatch_sweep.txt)
        const bool will_abatch = !will_mega && abatch_serves(B, c.ar_dtype, b->p.pipeline != 0, p->chunk_frames) && e->mega_ok && debug_options().ar_persistent != 0;
        int ar_cus = 96, part_streams = 0;
        if (b->p.pipeline && !will_mega && !will_abatch && B <= (p->chunk_frames > 1 ? 16 : 32)) {      // (chunk 4: 16 streams +11 %, 32 streams -15 %: the round-3 partition A/B scripts, git history)
            part_streams = B;
            if (B >= 2) ar_cus = c.ar_dtype == 1 ? (B <= 8 ? 96 : 64) : (B <= 8 ? 128 : B <= 20 ? 96 : 64);
        }
        if (b->p.pipeline && !will_mega && !will_abatch && debug_options().ar_batch == 1) {      // the measured table, when it has a row for this batch
            if (const PolicyRow* r = policy_row(B, c.ar_dtype, p->chunk_frames)) {
                if (r->decode == 0) { part_streams = r->cu_ar > 0 ? B : 0; if (r->cu_ar > 0) ar_cus = r->cu_ar; }
            }
        }
        if (debug_options().cu_partition == 0) part_streams = 0;
        else if (debug_options().cu_partition == 1 && b->p.pipeline) { part_streams = B; if (debug_options().cu_ar > 0) ar_cus = debug_options().cu_ar; }
        SVA_TRY(get_streams(e->device, part_streams, &ss, ar_cus));
        b->ar_cus = part_streams >= 1 ? ar_cus : 0;
        b->ar_partitioned = part_streams >= 1;
        if (b->ar_partitioned) {
            int cus = 0;
            SVA_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
            b->enc_cus = std::max(8, cus - ar_cus);
        }
        b->stream = b->main_stream = ss.main;
        b->aux0 = ss.aux0;
        if (b->p.pipeline) { b->sa = ss.sa; b->sv = ss.sv; }
        // split-K scratch per stream, now: a launch inside a stream capture must not allocate (and must not fall back to an
        // unsplit launch, which sums in a different order than the eager launch of the same shape)
        for (hipStream_t s_ : {ss.main, ss.aux0, ss.sa, ss.sv})
            if (s_) SVA_TRY(conv_gemm_prepare_stream(s_));
    }
    b->out_stream = b->stream;
    for (int i = 0; i < 64; ++i) SVA_HIP(hipEventCreateWithFlags(&b->evpool[i], hipEventDisableTiming));
    if (debug_options().pipe_trace > 0) {
        b->trace_n = debug_options().pipe_trace;
        b->trace_ev.resize((size_t)b->trace_n * 9);
        for (auto& t : b->trace_ev) SVA_HIP(hipEventCreate(&t));
    }
    // a whole-step graph is captured from ONE stream: a capture that forks to the side stream replays at 14 ms per step on this
    // runtime, the single-stream one at 3.8 (eager multi-stream: 3.6)
    if (b->p.use_graph) b->concurrency = false;
    if (!debug_options().concurrency) b->concurrency = false;      // single stream (PMC profiling)
    auto& A = b->allocs;
    const int chunk = p->chunk_frames;
    // control block
    SVA_TRY(dev_alloc(A, &b->d_step, 1));
    SVA_TRY(dev_alloc(A, &b->d_step_x, 1));
    SVA_TRY(dev_alloc(A, &b->d_last_pos, B));
    SVA_TRY(dev_alloc(A, &b->d_nframes, B));
    SVA_TRY(dev_alloc(A, &b->d_ncontent, B));
    SVA_TRY(dev_alloc(A, &b->d_seed, B));
    SVA_TRY(dev_alloc(A, &b->d_samp, (size_t)B * 2));
    SVA_TRY(dev_alloc(A, &b->d_use_forced, 1));
    SVA_TRY(dev_alloc(A, &b->d_slot_flag, B));
    // encoder
    b->We = p->encode_window_frames;
    b->N = b->We * 2048;
    b->T0 = b->N / 512;
    b->T2 = b->T0 / 4;
    SVA_CHECK(b->T2 % 4 == 0 && b->T2 <= 2048, "encode_window_frames must be a multiple of 4 and <= 2048 (the RoPE table of the tokenizer's transformer)");
    const int T0 = b->T0;
    SVA_TRY(dev_alloc(A, &b->ring, (size_t)B * b->N));
    SVA_TRY(dev_alloc(A, &b->d_chunk, (size_t)B * 2048 * chunk));
    SVA_TRY(dev_alloc(A, &b->mag, (size_t)B * T0 * 1088));
    SVA_TRY(alloc_act(A, b->mel, B, 6, T0, c.n_mels));
    for (int i = 0; i < 4; ++i) SVA_TRY(alloc_act(A, b->xs[i], B, 6, T0, c.enc_dims[i]));
    const int Dm = c.tr_dim;
    SVA_TRY(dev_alloc(A, &b->h1, (size_t)B * T0 * Dm));
    SVA_TRY(dev_alloc(A, &b->h2, (size_t)B * T0 * 4 * Dm));
    SVA_TRY(alloc_act(A, b->feat, B, 0, T0, Dm));
    SVA_TRY(alloc_act(A, b->d1, B, 6, T0 / 2, Dm));
    SVA_TRY(alloc_act(A, b->d2, B, 6, T0 / 4, Dm));
    const int T2 = b->T2;
    SVA_TRY(dev_alloc(A, &b->tr_hn, (size_t)B * T2 * Dm));
    SVA_TRY(dev_alloc(A, &b->tr_qkv, (size_t)B * T2 * 3 * Dm));
    SVA_TRY(dev_alloc(A, &b->tr_att, (size_t)B * T2 * Dm));
    SVA_TRY(dev_alloc(A, &b->tr_g, (size_t)B * T2 * c.tr_inter));
    SVA_TRY(dev_alloc(A, &b->tr_z, (size_t)B * T2 * Dm));
    SVA_TRY(dev_alloc(A, &b->tr_x, (size_t)B * T2 * Dm));
    SVA_TRY(alloc_act(A, b->d2c, B, 0, T2, Dm));
    b->Ht = 40;
    b->enc_incremental = T2 > b->Ht + p->chunk_frames;
    {   // steady token cache of the exact-incremental encoder: rows [Ht + c, T2) slide to [Ht, T2 - c) every step
        ShiftDesc dc;
        dc.ptr = b->d2c.p + (long)b->Ht * Dm; dc.bstride = b->d2c.bstride; dc.H = std::max(0, T2 - b->Ht - chunk); dc.T = chunk; dc.C = Dm; dc.pad = 0;
        SVA_TRY(dev_alloc(A, &b->d_shift_d2c, 1));
        SVA_HIP(hipMemcpy(b->d_shift_d2c, &dc, sizeof(ShiftDesc), hipMemcpyHostToDevice));
    }
    if (b->enc_incremental) {
        EncMerged& M = b->em;
        M.Hh = 4 * b->Ht; M.nm = 4 * chunk;
        const int Hh = M.Hh, nm = M.nm, R0 = Hh + 6 + nm, R1 = Hh / 2 + 6 + nm / 2, R2 = Hh / 4 + 6 + nm / 4;
        std::vector<ShiftDesc> sd;
        auto reg = [&](Act& a, int head_rows, int new_rows) {      // history rows sit right behind the head rows
            ShiftDesc d;
            d.ptr = a.p + (long)(a.H + head_rows) * a.C; d.bstride = a.bstride; d.H = 6; d.T = new_rows; d.C = a.C; d.pad = 0;
            sd.push_back(d);
        };
        SVA_TRY(dev_alloc(A, &M.mag, (size_t)B * R0 * 1088));
        SVA_TRY(alloc_act(A, M.mel, B, 6, R0, c.n_mels));
        reg(M.mel, Hh, nm);
        SVA_TRY(dev_alloc(A, &M.stem, (size_t)B * R0 * c.enc_dims[0]));
        M.x.resize(4);
        for (int i = 0; i < 4; ++i) {
            M.x[i].resize(c.enc_depths[i]);
            for (int j = 0; j < c.enc_depths[i]; ++j) {
                SVA_TRY(alloc_act(A, M.x[i][j], B, 6, R0, c.enc_dims[i]));
                reg(M.x[i][j], Hh, nm);
            }
            SVA_TRY(alloc_act(A, M.xout[i], B, 0, R0, c.enc_dims[i]));
        }
        SVA_TRY(alloc_act(A, M.feat, B, 0, R0, Dm));
        SVA_TRY(alloc_act(A, M.feat2, B, 0, R0, Dm));
        SVA_TRY(dev_alloc(A, &M.h1b, (size_t)B * R1 * Dm));
        SVA_TRY(dev_alloc(A, &M.h2b, (size_t)B * R1 * 4 * Dm));
        SVA_TRY(alloc_act(A, M.d1, B, 6, R1, Dm));
        reg(M.d1, Hh / 2, nm / 2);
        SVA_TRY(alloc_act(A, M.d1o, B, 0, R1, Dm));
        SVA_TRY(alloc_act(A, M.d2, B, 6, R2, Dm));
        reg(M.d2, Hh / 4, nm / 4);
        SVA_TRY(alloc_act(A, M.tok, B, 0, R2, Dm));
        SVA_TRY(dev_alloc(A, &M.h1, (size_t)B * R0 * Dm));
        SVA_TRY(dev_alloc(A, &M.h2, (size_t)B * R0 * 4 * Dm));
        M.n_shift = (int)sd.size();
        M.shift_host = sd;
        SVA_TRY(dev_alloc(A, &M.d_shift, sd.size()));
        SVA_HIP(hipMemcpy(M.d_shift, sd.data(), sizeof(ShiftDesc) * sd.size(), hipMemcpyHostToDevice));
    }
    SVA_TRY(dev_alloc(A, &b->aatt_part, (size_t)4 * c.ar_heads * 8 * 68));
    SVA_TRY(dev_alloc(A, &b->d_codes_buf[0], (size_t)B * T2));
    SVA_TRY(dev_alloc(A, &b->d_codes_buf[1], (size_t)B * T2));
    b->d_codes = b->d_codes_buf[0];
    SVA_TRY(dev_alloc(A, &b->d_fsq_codes, (size_t)B * c.num_codebooks * T2));
    SVA_TRY(dev_alloc(A, &b->d_u, (size_t)B * T2 * c.bsq_bits));
    // AR
    const int D = c.ar_dim, S = c.max_seq_len, H = c.ar_heads, ncb = c.num_codebooks;
    b->Mmax = std::max(std::max(std::max(2 * B, B * (2 * c.max_delay - 1)), S), std::min(B, 128) * 2 * p->buffer_frames);    // (last: a whole batch re-prefilling at once)
    SVA_TRY(dev_alloc(A, &b->ax, (size_t)b->Mmax * D));
    SVA_TRY(dev_alloc(A, &b->ahn, (size_t)b->Mmax * D));
    SVA_TRY(dev_alloc(A, &b->aqkv, (size_t)b->Mmax * 3 * D));
    SVA_TRY(dev_alloc(A, &b->aatt, (size_t)b->Mmax * D));
    SVA_TRY(dev_alloc(A, &b->ag, (size_t)b->Mmax * c.ar_inter));
    SVA_TRY(dev_alloc(A, &b->xf, (size_t)B * D));
    SVA_TRY(dev_alloc(A, &b->hidden, (size_t)B * D));
    SVA_TRY(dev_alloc(A, &b->slow_logits, (size_t)B * c.ar_vocab));
    SVA_TRY(dev_alloc(A, &b->fast_logits, (size_t)B * ncb * c.codebook_size));
    SVA_TRY(dev_alloc(A, &b->d_slot, b->Mmax));
    SVA_TRY(dev_alloc(A, &b->d_pos, b->Mmax));
    SVA_TRY(dev_alloc(A, &b->d_fast_slot, B));
    SVA_TRY(dev_alloc(A, &b->d_fast_pos, ncb * B));
    {
        std::vector<int> fs(B), fp((size_t)ncb * B);
        for (int i = 0; i < B; ++i) fs[i] = i;
        for (int cb = 0; cb < ncb; ++cb)
            for (int i = 0; i < B; ++i) fp[(size_t)cb * B + i] = cb;
        SVA_HIP(hipMemcpy(b->d_fast_slot, fs.data(), sizeof(int) * B, hipMemcpyHostToDevice));
        SVA_HIP(hipMemcpy(b->d_fast_pos, fp.data(), sizeof(int) * fp.size(), hipMemcpyHostToDevice));
    }
    b->kv_slow_slot = 2L * H * S * 64;
    b->kv_slow_layer = b->kv_slow_slot * B;
    b->kv_fast_slot = 2L * H * ncb * 64;
    b->kv_fast_layer = b->kv_fast_slot * B;
    b->kv_half = c.ar_dtype == 1;              // slow KV cache in fp16 (75.5 MB per stream instead of 151), as the reference's (infer_arvc.py:55-59)
    {
        float* p2;
        if (b->kv_half) { uint16_t* ph; SVA_TRY(dev_alloc(A, &ph, (size_t)c.ar_layers * b->kv_slow_layer)); b->kv_slow = ph; }
        else { float* p1; SVA_TRY(dev_alloc(A, &p1, (size_t)c.ar_layers * b->kv_slow_layer)); b->kv_slow = p1; }
        SVA_TRY(dev_alloc(A, &p2, (size_t)c.ar_fast_layers * b->kv_fast_layer));
        b->kv_fast = p2;
    }
    // persistent batch-1 decode kernel (ar_decode.hip): granule buffers, tag epoch, timeout word, fast K/V scratch
    // up to mega_max_b streams decode in ONE launch of it (96 workgroups per stream, each stream's group talks only to itself); the
    // multi-launch chain of the batched path (~200 dependent launches, 2.4-3.3 ms per frame at 2-8 streams) takes over above that
    b->use_mega = B <= b->mega_max && e->mega_ok && debug_options().ar_persistent != 0 && debug_options().ar_batch != 2;
    if (b->use_mega) {
        // every workgroup of a persistent launch must be resident at once: check the launch geometry against the occupancy query and
        // the CUs the AR stream may use, never assume it.  One workgroup per CU is what the kernel is sized for (256 registers, 4 waves);
        // the query's answer beyond 1 is not relied on (it over-reports by one on SGPR-heavy kernels, MI355X_MICROARCH.md).
        int per_cu = 0, cus = 0;
        SVA_TRY(ar_decode_occupancy(c.ar_dtype == 1, b->kv_half, &per_cu));
        SVA_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
        const int avail = b->ar_partitioned ? std::min(cus, b->ar_cus > 0 ? b->ar_cus : 96) : cus;       // the AR stream's CU mask (get_streams) is CUs 0 .. ar_cus - 1
        const int wgs = AR_WGS;
        b->mega_per_launch = (avail >= 2 * wgs && !b->ar_partitioned) ? 2 : 1;
        if (per_cu < 1 || avail < wgs) b->use_mega = false;                // fall back to the multi-launch decode
    }
    if (b->use_mega) {
        SVA_TRY(dev_alloc(A, &b->d_gran, ar_decode_granule_words() * B));
        SVA_TRY(dev_alloc(A, &b->d_epoch, B));
        SVA_TRY(dev_alloc(A, &b->d_ar_fail, 1));
        SVA_TRY(dev_alloc(A, &b->kv_fast_mega, (size_t)B * AR_FAST_LAYERS * 8 * 2 * D));
        if (debug_options().ar_timing) SVA_TRY(dev_alloc(A, &b->d_ar_dbg, 1024));
    }
    // batched persistent decode kernel (ar_batch.hip): every stream of the batch in one launch per frame.  Takes the batches the
    // two-streams-per-launch kernel above does not serve; its workgroups must all be resident (same check as above).
    b->use_abatch = !b->use_mega && e->mega_ok && debug_options().ar_persistent != 0 && abatch_serves(B, c.ar_dtype, b->p.pipeline != 0, b->p.chunk_frames) && c.ar_vocab <= 8192 &&
                    c.codebook_size <= 1024;
    if (b->use_abatch) {
        int per_cu = 0, cus = 0;
        SVA_TRY(ar_batch_occupancy(c.ar_dtype == 1, B, &per_cu));
        SVA_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
        const int avail = b->ar_partitioned ? std::min(cus, b->ar_cus > 0 ? b->ar_cus : 96) : cus;
        const int cap = std::min(per_cu, 1) * avail;             // 8 waves with up to 256 registers each: one workgroup per CU (the occupancy query's answer beyond 1 is not relied on)
        int G = ar_batch_wanted_workgroups(B);
        if (debug_options().ar_batch_wgs > 0) G = debug_options().ar_batch_wgs;
        G = std::min(G, cap);
        if (G < 48) b->use_abatch = false;
        b->abatch_G = G;
    }
    if (b->use_abatch) {
        static_assert(AR_BATCH_NBUF == 11, "ab_offs");
        const size_t words = ar_batch_granule_words(B, b->ab_offs);
        SVA_TRY(dev_alloc(A, &b->d_ab_gran, words));             // zeroed: tag 0 is never a live epoch (the counter starts at 1)
        SVA_TRY(dev_alloc(A, &b->d_ab_epoch, 2));
        if (!b->d_ar_fail) SVA_TRY(dev_alloc(A, &b->d_ar_fail, 1));
        if (debug_options().ar_timing && !b->d_ar_dbg) SVA_TRY(dev_alloc(A, &b->d_ar_dbg, 1024));
    }
    if (c.mm_mode == 1 || c.voc_dtype == 1 || c.enc_dtype == 1) {       // fp16 operands: their range check reports here (checked by sva_sync)
        SVA_HIP(hipHostMalloc((void**)&b->h_mm_ovf, sizeof(int), hipHostMallocMapped));
        *b->h_mm_ovf = 0;
        SVA_HIP(hipHostGetDevicePointer((void**)&b->d_mm_ovf, b->h_mm_ovf, 0));
    }
    if (b->d_ar_fail) {     // host-visible mirror of the timeout flag (the stream-ordered API never synchronises, so nothing read d_ar_fail)
        SVA_HIP(hipHostMalloc((void**)&b->h_ar_fail, sizeof(int), hipHostMallocMapped));
        *b->h_ar_fail = 0;
        SVA_HIP(hipHostGetDevicePointer((void**)&b->d_ar_fail_host, b->h_ar_fail, 0));
    }
    SVA_TRY(dev_alloc(A, &b->cached_audio_emb, (size_t)B * D));
    SVA_TRY(dev_alloc(A, &b->cached_ref_emb, (size_t)B * c.max_delay * D));
    SVA_TRY(dev_alloc(A, &b->d_ref_tail, (size_t)B * c.num_codebooks * c.max_delay));
    SVA_TRY(dev_alloc(A, &b->spk, (size_t)(c.timbre_tokens + 1) * D));
    SVA_TRY(dev_alloc(A, &b->d_style, (size_t)B * c.style_dim));
    SVA_TRY(dev_alloc(A, &b->d_timbre, (size_t)B * c.timbre_tokens * c.timbre_dim));
    SVA_TRY(dev_alloc(A, &b->d_sem, B));
    SVA_TRY(dev_alloc(A, &b->d_tok, B * ncb));
    SVA_TRY(dev_alloc(A, &b->d_tok_raw, B * ncb));
    SVA_TRY(dev_alloc(A, &b->d_forced, (size_t)B * ncb * chunk));
    SVA_TRY(dev_alloc(A, &b->d_noise, (size_t)B * chunk * (c.ar_vocab + ncb * c.codebook_size)));
    b->hist_cap = debug_options().hist_cap;   // 4096 unless SVA_DEBUG hist_cap=N (the ring-wrap tests); power of two (ring indexing); > buffer_frames + delay + chunk
    SVA_CHECK(b->hist_cap >= 1 && (b->hist_cap & (b->hist_cap - 1)) == 0, "hist_cap must be a power of two");
    SVA_CHECK(p->buffer_frames + p->delay + chunk < b->hist_cap, "buffer_frames too large for the history rings (buffer_frames + delay + chunk < hist_cap)");
    SVA_TRY(dev_alloc(A, &b->d_slot_list, B));
    SVA_TRY(dev_alloc(A, &b->d_content_hist, (size_t)B * b->hist_cap));
    SVA_TRY(dev_alloc(A, &b->d_pred_hist, (size_t)B * ncb * b->hist_cap));
    SVA_TRY(dev_alloc(A, &b->d_step_content, (size_t)B * chunk));
    SVA_TRY(dev_alloc(A, &b->d_step_audio_buf[0], (size_t)B * ncb * chunk));
    SVA_TRY(dev_alloc(A, &b->d_step_audio_buf[1], (size_t)B * ncb * chunk));
    b->d_step_audio = b->d_step_audio_buf[0];
    b->Pmax = S;
    SVA_TRY(dev_alloc(A, &b->d_prompt_cc, b->Pmax));
    SVA_TRY(dev_alloc(A, &b->d_prompt_ac, (size_t)ncb * b->Pmax));
    b->slots.reset(B);
    b->slots.sampling_defaults(p->temperature, p->top_p);
    for (int i = 0; i < B; ++i)
        SVA_HIP(hipMemcpyAsync(b->d_samp + 2 * i, b->slots.s[i].samp, sizeof(float) * 2, hipMemcpyHostToDevice, b->stream));
    SVA_HIP(hipStreamSynchronize(b->stream));
    // vocoder
    SVA_TRY(alloc_vocoder(b, b->p.voc_max_frames, nullptr));
    if (b->p.slot_priming) SVA_TRY(create_priming_workspace(b));
    SVA_HIP(hipHostMalloc((void**)&b->hp_in, sizeof(float) * (size_t)B * 2048 * chunk));
    SVA_HIP(hipHostMalloc((void**)&b->hp_out, sizeof(float) * (size_t)B * 2048 * chunk));
    for (int i = 0; i < 5; ++i) SVA_HIP(hipEventCreate(&b->ev[i]));
    b->ev_ok = true;
    if (b->use_mega || b->use_abatch) {        // counted BEFORE the synchronisation below: launches another batch enqueued without a chain record are complete behind it
        std::lock_guard<std::mutex> lk(e->mega_mu);
        e->persistent_batches += 1;
        b->counted_persistent = true;
    }
    SVA_HIP(hipDeviceSynchronize());
    return 0;
}

extern "C" void sva_batch_destroy(sva_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->e->device);
    if (b->io) sva_io_close(b->io);
    (void)quiesce(b);
    {   // (a later batch may be allocated at this address: the chain's "same batch, no wait" test must not match it)
        std::lock_guard<std::mutex> lk(b->e->mega_mu);
        if (b->e->mega_last == b) b->e->mega_last = nullptr;
        if (b->counted_persistent) { b->e->persistent_batches -= 1; b->counted_persistent = false; }
    }
    if (b->main_stream) (void)hipStreamSynchronize(b->main_stream);
    if (b->aux0) (void)hipStreamSynchronize(b->aux0);
    if (b->sa) (void)hipStreamSynchronize(b->sa);
    if (b->sv) (void)hipStreamSynchronize(b->sv);
    if (b->trace_n && b->trace_steps >= b->trace_n) {       // SVA_PIPE_TRACE: when each chain of the last steps could start / ended (us)
        const long s0 = b->trace_steps - b->trace_n;
        hipEvent_t base = b->trace_ev[(size_t)(s0 % b->trace_n) * 9];
        fprintf(stderr, "[sva pipe trace] step: main[start end] side[start] transformer[start end] ar[start end] vocoder[start end]  (us from the first row)\n");
        for (long q = s0; q < b->trace_steps; ++q) {
            float t[9];
            for (int k = 0; k < 9; ++k) { t[k] = 0.f; (void)hipEventElapsedTime(&t[k], base, b->trace_ev[(size_t)(q % b->trace_n) * 9 + k]); }
            fprintf(stderr, "[sva pipe trace] %ld: main %.0f %.0f | side %.0f | tr %.0f %.0f | ar %.0f %.0f | voc %.0f %.0f\n", q, t[0] * 1e3, t[1] * 1e3,
                    t[2] * 1e3, t[3] * 1e3, t[4] * 1e3, t[5] * 1e3, t[6] * 1e3, t[7] * 1e3, t[8] * 1e3);
        }
    }
    for (auto& t : b->trace_ev) (void)hipEventDestroy(t);
    if (b->graph_exec) (void)hipGraphExecDestroy(b->graph_exec);
    for (auto& ge : b->pipe_graph_a) if (ge) (void)hipGraphExecDestroy(ge);
    for (hipGraphExec_t ge : {b->gEm[0], b->gEm[1], b->gEs[0], b->gEs[1], b->gT0, b->gT1[0], b->gT1[1], b->gV}) if (ge) (void)hipGraphExecDestroy(ge);
    for (void* p : b->allocs.chunks) (void)hipFree(p);
    if (b->snap_image) (void)hipFree(b->snap_image);
    if (b->snap_table) (void)hipFree(b->snap_table);
    if (sva_batch* w = b->prime_ws) {        // the priming workspace: arena chunks and its event pool (streams and the overflow flag are the owner's)
        for (void* p : w->allocs.chunks) (void)hipFree(p);
        for (int i = 0; i < 64; ++i) if (w->evpool[i]) (void)hipEventDestroy(w->evpool[i]);
        delete w;
        b->prime_ws = nullptr;
    }
    if (b->h_ar_fail) (void)hipHostFree(b->h_ar_fail);
    if (b->h_mm_ovf) (void)hipHostFree(b->h_mm_ovf);
    if (b->hp_in) (void)hipHostFree(b->hp_in);
    if (b->hp_out) (void)hipHostFree(b->hp_out);
    for (int i = 0; i < 5; ++i) if (b->ev[i]) (void)hipEventDestroy(b->ev[i]);
    for (auto& ev : b->prof_ev) (void)hipEventDestroy(ev);
    for (int i = 0; i < 64; ++i) if (b->evpool[i]) (void)hipEventDestroy(b->evpool[i]);
    (void)hipGetLastError();          // the streams belong to the process-wide set and stay
    delete b;
}

// ============================================================================================
// prompt / begin
// ============================================================================================
namespace {
// All engine copies are ordered on the engine's (non-blocking) stream: a null-stream hipMemcpy from pageable
// memory may return before its DMA lands and is NOT ordered against kernels on a non-blocking stream.
int h2d(sva_batch* b, void* dst, const void* src, size_t bytes) {
    SVA_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, b->stream));
    SVA_HIP(hipStreamSynchronize(b->stream));
    return 0;
}
int stage_prompt(sva_batch* b, const std::vector<int64_t>& cc, const std::vector<int32_t>& ac, int R) {
    // cc [R] int64 -> d_prompt_cc int32; ac [8][R] -> d_prompt_ac [8][Pmax]
    const int ncb = b->e->cfg.num_codebooks;
    SVA_CHECK(R <= b->Pmax, "prompt longer than the staging buffer");
    std::vector<int> c32(R);
    for (int i = 0; i < R; ++i) c32[i] = (int)cc[i];
    SVA_HIP(hipMemcpyAsync(b->d_prompt_cc, c32.data(), sizeof(int) * R, hipMemcpyHostToDevice, b->stream));
    for (int q = 0; q < ncb; ++q)
        SVA_HIP(hipMemcpyAsync(b->d_prompt_ac + (long)q * b->Pmax, ac.data() + (long)q * R, sizeof(int) * R, hipMemcpyHostToDevice, b->stream));
    SVA_HIP(hipStreamSynchronize(b->stream));
    return 0;
}
}  // namespace

// the prompt of one slot on a drained batch: speaker operands, noise key, KV prefill, the stored (truncated) prompt
static int prefill_slot_impl(sva_batch* b, int slot, const int64_t* ref_content_codes, const int32_t* ref_audio_codes, int R, const float* style,
                             const float* timbre, uint64_t noise_seed, bool tap_logits) {
    const sva_config& c = b->e->cfg;
    const int ncb = c.num_codebooks;
    std::vector<int64_t> cc(ref_content_codes, ref_content_codes + R);
    std::vector<int32_t> ac(ref_audio_codes, ref_audio_codes + (size_t)ncb * R);
    SVA_TRY(h2d(b, b->d_style + (long)slot * c.style_dim, style, sizeof(float) * c.style_dim));
    SVA_TRY(h2d(b, b->d_timbre + (long)slot * c.timbre_tokens * c.timbre_dim, timbre, sizeof(float) * c.timbre_tokens * c.timbre_dim));
    unsigned long long sd = noise_seed;
    SVA_TRY(h2d(b, b->d_seed + slot, &sd, sizeof(sd)));
    // quirk (iv): the KV prefill uses the UNTRUNCATED prompt (infer_arvc.py:484-489) ...
    SVA_TRY(stage_prompt(b, cc, ac, R));
    SVA_TRY(ar_prefill_slot(b, slot, R, tap_logits));
    // ... while the stored prompt (re-prefill, vocoder fill) is truncated to max_prompt_frames (:469-470)
    const int Rt = std::min(R, b->p.max_prompt_frames);
    {   // the last max_delay frames of the stored prompt's audio codes, for the device-side re-prefill (right-aligned; a shorter prompt leaves the front unused)
        const int md = c.max_delay;
        std::vector<int32_t> tail((size_t)ncb * md, 0);
        for (int q = 0; q < ncb; ++q)
            for (int j = 0; j < md; ++j)
                if (Rt - md + j >= 0) tail[(size_t)q * md + j] = ac[(size_t)q * R + (Rt - md + j)];
        SVA_TRY(h2d(b, b->d_ref_tail + (long)slot * ncb * md, tail.data(), sizeof(int32_t) * tail.size()));
    }
    b->slots.prefilled(slot, c.timbre_tokens + 1, R, Rt, ncb, cc.data(), ac.data());
    return 0;
}

extern "C" int sva_prefill_prompt(sva_batch* b, int slot, const int64_t* ref_content_codes, const int32_t* ref_audio_codes, int R,
                                  const float* style, const float* timbre, uint64_t noise_seed) {
    SVA_CHECK(b && slot >= 0 && slot < b->B && ref_content_codes && ref_audio_codes && style && timbre, "bad argument");
    SVA_HIP(hipSetDevice(b->e->device));
    (void)hipGetLastError();
    SVA_TRY(quiesce(b));
    SVA_TRY(recover_ar_failure(b));
    return prefill_slot_impl(b, slot, ref_content_codes, ref_audio_codes, R, style, timbre, noise_seed, true);
}

extern "C" int sva_vocode_reset(sva_batch* b) {
    SVA_CHECK(b, "null batch");
    SVA_HIP(hipSetDevice(b->e->device));
    (void)hipGetLastError();
    SVA_TRY(quiesce(b));
    SVA_HIP(hipMemsetAsync(b->voc.d_frames, 0, sizeof(int), b->stream));
    SVA_TRY(for_each_voc_state(b->voc, [&](Act& a, unsigned short*& P, int, VocForm) -> int {
        SVA_HIP(hipMemsetAsync(a.p, 0, sizeof(float) * (size_t)b->B * a.bstride, b->stream));
        if (P) SVA_HIP(hipMemsetAsync(P, 0, sizeof(unsigned short) * (size_t)planes_count(b->voc.pmode) * b->B * a.bstride, b->stream));
        return 0;
    }));
    SVA_HIP(hipStreamSynchronize(b->stream));
    return 0;
}

namespace {
int upload_vcodes(sva_batch* b, const int32_t* codes, int T) {
    // host codes [B][8][T] -> d_vcodes [B][8][Tv]
    const int ncb = b->e->cfg.num_codebooks;
    SVA_HIP(hipMemcpy2DAsync(b->voc.d_vcodes, sizeof(int) * b->voc.Tv, codes, sizeof(int) * T, sizeof(int) * T, (size_t)b->B * ncb,
                             hipMemcpyHostToDevice, b->stream));
    return 0;
}
int download_pcm(sva_batch* b, int T, float* pcm_out) {
    SVA_HIP(hipMemcpy2DAsync(pcm_out, sizeof(float) * 2048 * T, b->voc.d_pcm, sizeof(float) * 2048 * b->voc.Tv, sizeof(float) * 2048 * T, b->B,
                             hipMemcpyDeviceToHost, b->stream));
    SVA_HIP(hipStreamSynchronize(b->stream));
    return 0;
}
}  // namespace

extern "C" int sva_vocode_stream(sva_batch* b, const int32_t* codes, int T, float* pcm_out) {
    SVA_CHECK(b && codes && pcm_out, "null argument");
    SVA_CHECK(T >= 1 && T <= b->voc.Tv, "vocode: T out of range (1 .. voc_max_frames)");
    SVA_HIP(hipSetDevice(b->e->device));
    (void)hipGetLastError();
    SVA_TRY(quiesce(b));
    SVA_TRY(upload_vcodes(b, codes, T));
    SVA_TRY(vocode(b, T, true));
    return download_pcm(b, T, pcm_out);
}

extern "C" int sva_vocode_window(sva_batch* b, const int32_t* codes, int T, float* pcm_out) {
    SVA_CHECK(b && codes && pcm_out, "null argument");
    SVA_CHECK(T >= 1 && T <= b->voc.Tv, "vocode: T out of range (1 .. voc_max_frames)");
    SVA_TRY(sva_vocode_reset(b));
    SVA_TRY(sva_vocode_stream(b, codes, T, pcm_out));
    return sva_vocode_reset(b);
}

// firefly.quantizer.decode (modules/vqgan/modules/fsq.py:112-116) as a seam of its own: codes int32[B][8][T] -> z float[B][4T][512]
// (channel-last; the reference tensor is [B, 512, 4T]), window semantics (zero history) like sva_vocode_window
extern "C" int sva_quantizer_decode(sva_batch* b, const int32_t* codes, int T, float* z_out) {
    SVA_CHECK(b && codes && z_out, "null argument");
    SVA_CHECK(T >= 1 && T <= b->voc.Tv, "quantizer_decode: T out of range (1 .. voc_max_frames)");
    SVA_TRY(sva_vocode_reset(b));
    SVA_TRY(upload_vcodes(b, codes, T));
    SVA_TRY(vocode(b, T, false, VocPart::QuantizerDecode));
    const int V = b->e->cfg.voc_dim;
    SVA_HIP(hipMemcpy2DAsync(z_out, sizeof(float) * 4 * T * V, b->voc.pin.p + (long)b->voc.pin.H * V, sizeof(float) * b->voc.pin.bstride, sizeof(float) * 4 * T * V, b->B,
                             hipMemcpyDeviceToHost, b->stream));
    SVA_HIP(hipStreamSynchronize(b->stream));
    return sva_vocode_reset(b);
}

// firefly.head (HiFiGANGenerator.forward, firefly.py:280-293) as a seam of its own: z float[B][4T][512] -> pcm float[B][2048 T]
extern "C" int sva_vocoder_head(sva_batch* b, const float* z, int T, float* pcm_out) {
    SVA_CHECK(b && z && pcm_out, "null argument");
    SVA_CHECK(T >= 1 && T <= b->voc.Tv, "vocoder_head: T out of range (1 .. voc_max_frames)");
    SVA_TRY(sva_vocode_reset(b));
    const int V = b->e->cfg.voc_dim;
    SVA_HIP(hipMemcpy2DAsync(b->voc.pin.p + (long)b->voc.pin.H * V, sizeof(float) * b->voc.pin.bstride, z, sizeof(float) * 4 * T * V, sizeof(float) * 4 * T * V, b->B,
                             hipMemcpyHostToDevice, b->stream));
    SVA_TRY(vocode(b, T, false, VocPart::Head));
    SVA_TRY(download_pcm(b, T, pcm_out));
    return sva_vocode_reset(b);
}

extern "C" int sva_streams_begin(sva_batch* b) {
    SVA_CHECK(b, "null batch");
    SVA_CHECK(!b->io, "sva_streams_begin: an I/O adaptor is open on this batch; close it first (its FIFOs belong to the running streams)");
    SVA_HIP(hipSetDevice(b->e->device));
    (void)hipGetLastError();
    SVA_TRY(quiesce(b));
    SVA_TRY(recover_ar_failure(b));
    const int B = b->B, ncb = b->e->cfg.num_codebooks, c = b->p.chunk_frames;
    SVA_CHECK(b->slots.all_prefilled(), "every slot needs sva_prefill_prompt before sva_streams_begin");
    // setup_stream_caches (infer_arvc.py:443-460)
    SVA_HIP(hipMemsetAsync(b->ring, 0, sizeof(float) * (size_t)B * b->N, b->stream));
    SVA_HIP(hipMemsetAsync(b->d_step, 0, sizeof(int), b->stream));
    SVA_HIP(hipMemsetAsync(b->d_nframes, 0, sizeof(int) * B, b->stream));
    SVA_HIP(hipMemsetAsync(b->d_ncontent, 0, sizeof(int) * B, b->stream));
    b->slots.begin();
    SVA_HIP(hipMemsetAsync(b->d_slot_flag, 0, sizeof(int) * B, b->stream));
    if (b->enc_incremental) {
        // The reference's window starts as all-zero audio (:451): initialise the per-layer histories and the steady
        // token cache with the network's response to silence by streaming zero frames until every history row and
        // every cached token is that steady response (receptive field 117 mel frames; T2 tokens in the cache).
        auto zero = [&](Act& a) -> int {
            SVA_HIP(hipMemsetAsync(a.p, 0, sizeof(float) * (size_t)B * a.bstride, b->stream));
            return 0;
        };
        SVA_TRY(zero(b->d2c));
        const int warm = 48 / c + 2;             // > receptive field (117 mel frames = 30 tokens) -> histories are steady
        EncMerged& M = b->em;
        SVA_TRY(zero(M.mel)); SVA_TRY(zero(M.d1)); SVA_TRY(zero(M.d2));
        for (auto& st_ : M.x) for (auto& a : st_) SVA_TRY(zero(a));
        sva_engine* e = b->e;
        std::vector<ShiftDesc> sd(M.n_shift);
        SVA_HIP(hipMemcpy(sd.data(), M.d_shift, sizeof(ShiftDesc) * M.n_shift, hipMemcpyDeviceToHost));
        const auto key = std::make_pair(B, c);
        auto it = e->silence.find(key);
        if (it == e->silence.end()) {
            for (int i = 0; i < warm; ++i) SVA_TRY(enc_frontend_merged(b, nullptr, 0, 0));     // (the ring is all zeros here)
            sva_engine::SilenceState ss;
            for (const ShiftDesc& d : sd) {          // keep the newest history row of item 0 per buffer, and the token row
                float* r = nullptr;
                SVA_TRY(dev_alloc(e->allocs, &r, (size_t)d.C, false));
                SVA_HIP(hipMemcpyAsync(r, d.ptr + (long)(d.H - 1) * d.C, sizeof(float) * d.C, hipMemcpyDeviceToDevice, b->stream));
                ss.rows.push_back(r);
            }
            SVA_TRY(dev_alloc(e->allocs, &ss.tok, (size_t)b->e->cfg.tr_dim, false));
            SVA_HIP(hipMemcpyAsync(ss.tok, b->d2c.p + (long)(b->T2 - 1) * b->e->cfg.tr_dim, sizeof(float) * b->e->cfg.tr_dim, hipMemcpyDeviceToDevice, b->stream));
            e->silence[key] = ss;
        } else {
            const sva_engine::SilenceState& ss = it->second;
            for (size_t i = 0; i < sd.size(); ++i) {
                const ShiftDesc& d = sd[i];
                SVA_TRY(launch_fill_rows(d.ptr, d.bstride, d.C, ss.rows[i], d.H, B, b->stream));
            }
            SVA_TRY(launch_fill_rows(b->d2c.p + (long)(b->T2 - 1) * b->e->cfg.tr_dim, b->d2c.bstride, b->e->cfg.tr_dim, ss.tok, 1, B, b->stream));
        }
        // every cached token of a silent window is that same steady response
        SVA_TRY(launch_broadcast_row(b->d2c.p, b->d2c.bstride, b->T2 - 1, 0, b->T2, b->e->cfg.tr_dim, B, b->stream));
        SVA_HIP(hipStreamSynchronize(b->stream));
    }
    // prime the streaming vocoder with the tail of the (truncated) prompt: the reference left-fills its
    // 64-frame vocoder window with the prompt's last frames (:567-571, quirk ix), and the newest frame only
    // depends on the newest 16 code frames, so running the last (window-1) prompt frames through the
    // ring-buffer vocoder reproduces the windowed output.
    SVA_TRY(sva_vocode_reset(b));
    int P = b->slots.priming_frames(0, b->p.decode_window_frames, c);       // (the shortest stored prompt of the batch decides)
    for (int i = 1; i < B; ++i) P = std::min(P, b->slots.priming_frames(i, b->p.decode_window_frames, c));
    SVA_CHECK(P >= 16 || P == b->p.decode_window_frames - 1, "prompt shorter than the vocoder receptive field (16 frames)");
    std::vector<int32_t> codes((size_t)B * ncb * c);
    std::vector<float> sink((size_t)B * 2048 * c);
    for (int f = 0; f < P; f += c) {
        for (int i = 0; i < B; ++i) b->slots.prompt_tail(i, ncb, P, f, c, codes.data() + (size_t)i * ncb * c);
        SVA_TRY(sva_vocode_stream(b, codes.data(), c, sink.data()));
    }
    b->begun = true;
    b->steady_eager_steps = 0;     // (a captured graph stays valid: every pointer / constant in it is unchanged)
    return 0;
}

// ============================================================================================
// the per-chunk step
// ============================================================================================
namespace {

int check_mm_overflow(sva_batch* b) {
    if (b->h_mm_ovf && *reinterpret_cast<volatile int*>(b->h_mm_ovf) != 0) {
        *b->h_mm_ovf = 0;
        if (b->e->cfg.enc_dtype == 1)
            SVA_CHECK(false, "a GEMM on fp16 operands produced a non-finite output: an activation or weight is outside the fp16 range (as it would be for "
                             "the reference under torch.autocast(fp16)); create the engine with sva_config.enc_dtype = 0 (and mm_mode = 0, voc_dtype = 0) for "
                             "the range-safe kernels -- the results since the last synchronisation are invalid");
        SVA_CHECK(false, "a batch-scale GEMM on fp16 operand planes produced a non-finite output: an activation or weight is outside the fp16 range "
                         "(as it would be for the reference under torch.autocast(fp16)); create the engine with sva_config.mm_mode = 0 (and voc_dtype = 0) "
                         "for the range-safe bf16 kernels -- the results since the last synchronisation are invalid");
    }
    return 0;
}

// every due slot in one pass over the layers, no host synchronisation (see build_reprefill_kernel)
int reprefill_slots(sva_batch* b, const std::vector<int>& due) {
    sva_engine* e = b->e;
    const sva_config& c = e->cfg;
    const int ncb = c.num_codebooks, d = b->p.delay, bf = b->p.buffer_frames, D = c.ar_dim, nspk = c.timbre_tokens + 1;
    hipStream_t st = b->stream;
    for (size_t lo = 0; lo < due.size(); lo += 128) {
        ReprefillArgs a;
        a.n = (int)std::min<size_t>(128, due.size() - lo);
        a.row_off[0] = 0;
        for (int i = 0; i < a.n; ++i) {
            const int slot = due[lo + i];
            const SlotHost& h = b->slots.s[slot];
            const int nf = h.nframes, ncon = h.ncontent;
            const int na = b->slots.reprefill_frames(slot, bf);
            SVA_CHECK(na == std::max(0, (ncon - d) - std::max(0, ncon - bf - d)) && na >= d, "re-prefill: content/audio history length mismatch");
            a.slot[i] = slot; a.Rt[i] = h.ref_len; a.nf[i] = nf; a.na[i] = na; a.ncon[i] = ncon;
            a.row_off[i + 1] = a.row_off[i] + 2 * na;
            // BEFORE anything is enqueued: rows past the slot's cache would land in the next slot's
            SVA_CHECK(nspk + 2 * (a.Rt[i] + na) + 2 * d <= c.max_seq_len, "re-prefill: prompt too long for the KV cache");
        }
        const int M = a.row_off[a.n];
        SVA_CHECK(M <= b->Mmax, "re-prefill: more rows than the AR scratch holds");
        SVA_TRY(launch_build_reprefill(a, e->content_emb, e->codebook_emb, b->d_content_hist, b->d_pred_hist, b->hist_cap, b->d_ref_tail, c.max_delay, d, ncb,
                                       c.codebook_size, D, nspk, b->ax, b->d_slot, b->d_pos, st));
        SVA_TRY(ar_layers_pass(b, e->ar_layers, M, b->d_slot, b->d_pos, e->rope_ar, (float*)b->kv_slow, b->kv_slow_layer, b->kv_slow_slot,
                               c.max_seq_len, b->ax));
        SVA_TRY(launch_finish_reprefill(a, e->codebook_emb, b->d_pred_hist, b->hist_cap, b->d_ref_tail, c.max_delay, d, ncb, c.codebook_size, D, nspk,
                                        b->cached_ref_emb, b->d_last_pos, st));
        for (int i = 0; i < a.n; ++i) b->slots.reprefilled(a.slot[i], b->slots.reprefill_end(a.slot[i], nspk, bf));
    }
    return 0;
}

int reprefill_slot(sva_batch* b, int slot) {
    // infer_arvc.py:547-564: prompt <- [ref (truncated), last buffer_frames predicted frames] /
    // [ref content, src content[-buffer-d:-d]]; then delay fill with src content[-d:]
    const sva_config& c = b->e->cfg;
    const int ncb = c.num_codebooks, d = b->p.delay, bf = b->p.buffer_frames;
    const SlotHost& h = b->slots.s[slot];
    const int R = h.ref_len;
    const int nf = h.nframes, ncon = h.ncontent;
    const int na = b->slots.reprefill_frames(slot, bf);                   // pred_codes[..., -bf:]
    const int c_hi = ncon - d, c_lo = std::max(0, ncon - bf - d);
    const int nc = std::max(0, c_hi - c_lo);
    SVA_CHECK(na == nc, "re-prefill: content/audio history length mismatch");
    std::vector<int> hc(nc), ha((size_t)ncb * na);
    SVA_HIP(hipStreamSynchronize(b->stream));
    {   // the histories are rings of hist_cap entries: fetch the slot's rows and index them on the host (rare path)
        const int cap = b->hist_cap;
        std::vector<int> ring(cap);
        if (nc) {
            SVA_HIP(hipMemcpy(ring.data(), b->d_content_hist + (long)slot * cap, sizeof(int) * cap, hipMemcpyDeviceToHost));
            for (int i = 0; i < nc; ++i) hc[i] = ring[(c_lo + i) & (cap - 1)];
        }
        for (int q = 0; q < ncb && na; ++q) {
            SVA_HIP(hipMemcpy(ring.data(), b->d_pred_hist + ((long)slot * ncb + q) * cap, sizeof(int) * cap, hipMemcpyDeviceToHost));
            for (int i = 0; i < na; ++i) ha[(size_t)q * na + i] = ring[(nf - na + i) & (cap - 1)];
        }
    }
    std::vector<int64_t> cc(h.ref_content);
    for (int i = 0; i < nc; ++i) cc.push_back(hc[i]);
    const int Rn = R + na;
    std::vector<int32_t> ac((size_t)ncb * Rn);
    for (int q = 0; q < ncb; ++q) {
        for (int i = 0; i < R; ++i) ac[(size_t)q * Rn + i] = h.ref_audio[(size_t)q * R + i];
        for (int i = 0; i < na; ++i) ac[(size_t)q * Rn + R + i] = ha[(size_t)q * na + i];
    }
    SVA_TRY(stage_prompt(b, cc, ac, Rn));
    SVA_TRY(ar_prefill_slot(b, slot, Rn));
    b->slots.reprefilled(slot, SlotBook::prefill_end(c.timbre_tokens + 1, Rn));
    return 0;
}

// device work of one steady-state chunk: E0..E8, c AR frames, streaming vocoder, history shift.  Only launches
// on b->stream with device-resident control state, so the sequence can be captured in a hipGraph.
int steady_launches(sva_batch* b, bool timing_events) {
    const sva_config& c = b->e->cfg;
    const int B = b->B, chunk = b->p.chunk_frames, n = 2048 * chunk, ncb = c.num_codebooks;
    hipStream_t st = b->stream;
    if (timing_events) SVA_HIP(hipEventRecord(b->ev[0], st));
    SVA_TRY(launch_ring_write(b->ring, b->d_step, B, b->N, b->step_src ? b->step_src : b->d_chunk, n, st, b->d_slot_flag));
    SVA_TRY(b->enc_incremental ? encode_incremental(b, b->d_step, n, 1) : encode(b, b->d_step, n, 1));
    SVA_TRY(launch_append_content(b->d_codes, b->T2, chunk, b->d_content_hist, b->hist_cap, b->d_ncontent, b->d_step_content, B, b->d_step, st));
    if (timing_events) SVA_HIP(hipEventRecord(b->ev[1], st));
    for (int ci = 0; ci < chunk; ++ci) SVA_TRY(ar_decode_frame(b, ci, b->d_codes, b->T2, b->T2 - chunk + ci));          // :534-538
    if (timing_events) SVA_HIP(hipEventRecord(b->ev[2], st));
    b->voc.codes = b->d_step_audio; b->voc.codes_bstride = (long)ncb * chunk; b->voc.codes_gstride = chunk;      // read in place
    const int vrc = vocode(b, chunk, true);
    b->voc.codes = nullptr;
    if (vrc) return vrc;
    if (timing_events) SVA_HIP(hipEventRecord(b->ev[3], st));
    return 0;
}

// Replays `body` (launches on stream st only, all arguments fixed device pointers / constants) as a hipGraph captured on first
// use; falls back to eager launches for good if the runtime cannot capture.
template <class F>
int stage_graph(sva_batch* b, hipGraphExec_t* slot, hipStream_t st, F&& body) {
    if (const int skip = debug_options().pipe_skip) {      // timing diagnostic only (tools/pipe_skip.sh): the chain's work is left out, its events stay
        static bool warned = false;
        if (!warned) { warned = true; fprintf(stderr, "[sva] SVA_DEBUG=pipe_skip=%d: chains of the pipelined step are LEFT OUT -- timing diagnostic, outputs are garbage\n", skip); }
        const int bit = (slot == &b->gEm[0] || slot == &b->gEm[1]) ? 1 : slot == &b->gV ? 8 : 2;
        if (skip & bit) return 0;
    }
    if (!b->stage_graphs) return body();
    if (!*slot) {
        hipGraph_t graph = nullptr;
        SVA_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        const int rc = body();
        const hipError_t ce = hipStreamEndCapture(st, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (ce != hipSuccess || hipGraphInstantiate(slot, graph, nullptr, nullptr, 0) != hipSuccess) {
            (void)hipGetLastError();
            *slot = nullptr;
            b->stage_graphs = false;
            if (graph) (void)hipGraphDestroy(graph);
            return body();
        }
        (void)hipGraphDestroy(graph);
    }
    SVA_HIP(hipGraphLaunch(*slot, st));
    return 0;
}

// Pipelined steady step (sva_step_device with p.pipeline): the three stages of chunk-step n go to three streams,
//   main: E(n)   ->   sa: A(n)   ->   sv: V(n)
// chained by events, so that E(n+1), A(n) and V(n-1) overlap on the GPU.  Hazards between consecutive steps:
//   * d_codes (E writes, A reads to the end of its frame): double-buffered, swapped per step;
//   * d_step_audio (A writes at the end of a frame, V reads it first thing): double-buffered like d_codes, A(n) waits for
//     V(n-2)'s read;
//   * content history (E appends, a re-prefill on sa reads): E(n+1) waits for the re-prefill of step n.
// Every other buffer is private to its stage.
int steady_pipelined(sva_batch* b) {
    const sva_config& c = b->e->cfg;
    const int B = b->B, chunk = b->p.chunk_frames, n = 2048 * chunk, ncb = c.num_codebooks;
    hipStream_t se = b->main_stream, sa = b->sa, sv = b->sv;
    // the stage-boundary events of sva_get_timings mean nothing under overlap and every event record is a barrier packet on its queue (~8 us of
    // the AR chain's period each: profiles/r06_ar_chain_events.txt) -- only the pipe trace keeps them
    const bool stage_ev = b->trace_n > 0;
    if (!b->pipe_dirty) {            // entering the pipelined regime: the side streams must see all serial work so far
        hipEvent_t ev = next_event(b);
        SVA_HIP(hipEventRecord(ev, se));
        SVA_HIP(hipStreamWaitEvent(sa, ev, 0));
        SVA_HIP(hipStreamWaitEvent(sv, ev, 0));
        SVA_HIP(hipMemcpyAsync(b->d_step_x, b->d_step, sizeof(int), hipMemcpyDeviceToDevice, se));      // the side chain's chunk counter
        b->pipe_evVc[0] = b->pipe_evVc[1] = nullptr; b->pipe_evR = nullptr; b->pipe_evA[0] = b->pipe_evA[1] = nullptr;
        b->pipe_evFeat[0] = b->pipe_evFeat[1] = nullptr;
    }
    const int par = b->pipe_parity;
    b->d_codes = b->d_codes_buf[par];
    b->d_step_audio = b->d_step_audio_buf[par];      // the frame's audio codes: A(n) writes them last, V(n) reads them first
    b->pipe_parity ^= 1;
    hipEvent_t evE = nullptr;
    // debug trace: k = 0 main start, 1 main end, 2 side start, 3 transformer start, 4 transformer end, 5 AR start, 6 AR end,
    // 7 vocoder start, 8 vocoder end (each recorded behind the waits of its chain, i.e. when the chain could really start)
    auto mark = [&](int k, hipStream_t st_) -> int {
        if (b->trace_n) SVA_HIP(hipEventRecord(b->trace_ev[(size_t)(b->trace_steps % b->trace_n) * 9 + k], st_));
        return 0;
    };
    if (b->enc_incremental && b->concurrency && b->aux0) {
        // As one in-order stage the encoder's latency (1.7 ms) was the period of the whole pipeline, so it is two chains, both replayed as
        // hipGraphs (stage_graph) and both near the AR frame time:
        //   main: the merged front-end's backbone (STFT .. final LayerNorm; the new frames ride in the head-pass launches) -> feat[par]
        //   sx:   slide d2c, the quantizer's downsampler -> d2c, transformer + BSQ(n)                                       -> evE
        // so backbone(n+1) overlaps downsampler + transformer(n).  The token cache d2c is written and read on ONE in-order stream (sx).  The
        // hand-over buffer feat[] alternates; main(n+2) waits until side(n) has read it.  The chunk counter (ring position) is read by the
        // first kernel of the main chain, whose last kernel advances it (step_bump; the append no longer does).
        hipStream_t sx = b->aux0;
        b->stream = se;
        if (stage_ev) SVA_HIP(hipEventRecord(b->ev[0], se));
        SVA_TRY(mark(0, se));
        if (b->pipe_evFeat[par]) SVA_HIP(hipStreamWaitEvent(se, b->pipe_evFeat[par], 0));
        SVA_TRY(stage_graph(b, &b->gEm[par], se, [&]() -> int {
            b->stream = se;
            SVA_TRY(launch_ring_write(b->ring, b->d_step, B, b->N, b->step_src ? b->step_src : b->d_chunk, n, se, b->d_slot_flag));
            b->step_bump = b->d_step;              // the history shift that ends the chain also advances the chunk counter
            const int frc = enc_frontend_merged(b, b->d_step, n, 1, 3, par);
            b->step_bump = nullptr;
            return frc;
        }));
        SVA_TRY(mark(1, se));
        SVA_TRY(mark(2, sx));
        SVA_TRY(stream_fork(b, se, sx));
        int src_ = stage_graph(b, &b->gEs[par], sx, [&]() -> int {
            b->stream = sx;
            SVA_TRY(launch_shift_history(b->d_shift_d2c, 1, B, sx, 16));               // steady tokens slide down by c
            return enc_frontend_merged(b, nullptr, n, 1, 4, par);
        });
        b->stream = se;
        if (src_) return src_;
        b->pipe_evFeat[par] = next_event(b);
        SVA_HIP(hipEventRecord(b->pipe_evFeat[par], sx));
        if (b->pipe_evA[par]) SVA_HIP(hipStreamWaitEvent(sx, b->pipe_evA[par], 0));  // back-pressure: BSQ overwrites the codes A(n-2) read
        if (b->pipe_evR) { SVA_HIP(hipStreamWaitEvent(sx, b->pipe_evR, 0)); b->pipe_evR = nullptr; }
        SVA_TRY(mark(3, sx));
        // (two graphs, cut behind the first layer: the cut once released the token cache to the main chain and releases nothing now)
        int trc = stage_graph(b, &b->gT0, sx, [&]() -> int { b->stream = sx; return enc_transformer(b, b->d2c, chunk, 1); });
        b->stream = se;
        if (trc) return trc;
        trc = stage_graph(b, &b->gT1[par], sx, [&]() -> int {
            b->stream = sx;
            SVA_TRY(enc_transformer(b, b->d2c, chunk, 2));
            return launch_append_content(b->d_codes, b->T2, chunk, b->d_content_hist, b->hist_cap, b->d_ncontent, b->d_step_content, B, nullptr, sx);
        });
        b->stream = se;
        if (trc) return trc;
        if (stage_ev) SVA_HIP(hipEventRecord(b->ev[1], sx));
        SVA_TRY(mark(4, sx));
        if (b->pipe_evVc[par]) SVA_HIP(hipStreamWaitEvent(sx, b->pipe_evVc[par], 0));     // V(n-2) has read the audio-code buffer A(n) will overwrite (long since)
        evE = next_event(b);
        SVA_HIP(hipEventRecord(evE, sx));
    } else {
        // back-pressure: this step's encoder overwrites the code buffer that A(n-2) read, so E may lead A by at most two steps
        if (b->pipe_evA[par]) SVA_HIP(hipStreamWaitEvent(se, b->pipe_evA[par], 0));
        if (b->pipe_evR) { SVA_HIP(hipStreamWaitEvent(se, b->pipe_evR, 0)); b->pipe_evR = nullptr; }
        b->stream = se;
        if (stage_ev) SVA_HIP(hipEventRecord(b->ev[0], se));
        SVA_TRY(launch_ring_write(b->ring, b->d_step, B, b->N, b->step_src ? b->step_src : b->d_chunk, n, se, b->d_slot_flag));
        SVA_TRY(b->enc_incremental ? encode_incremental(b, b->d_step, n, 1) : encode(b, b->d_step, n, 1));
        SVA_TRY(launch_append_content(b->d_codes, b->T2, chunk, b->d_content_hist, b->hist_cap, b->d_ncontent, b->d_step_content, B, b->d_step, se));
        if (stage_ev) SVA_HIP(hipEventRecord(b->ev[1], se));
        if (b->pipe_evVc[par]) SVA_HIP(hipStreamWaitEvent(se, b->pipe_evVc[par], 0));
        evE = next_event(b);
        SVA_HIP(hipEventRecord(evE, se));
    }
    // A(n)
    SVA_HIP(hipStreamWaitEvent(sa, evE, 0));       // (evE also carries "V(n-2) has read the code buffer": the encoder chain waited for that event above --
                                                   //  one barrier packet fewer on the AR queue, whose chain is the period of a one-stream pipeline)
    b->stream = sa;
    SVA_TRY(mark(5, sa));
    int rc = 0;
    if (debug_options().pipe_skip & 4) {
    } else if (b->pipe_graph_mode && (debug_options().ar_graph >= 0 ? debug_options().ar_graph != 0 : true)) {
        // The AR stage is ~210 launches on ONE stream whose arguments never change (positions, frame counters, noise keys
        // and teacher-forcing flags live in device memory; the code buffer alternates, hence one graph per parity): replaying
        // it as a hipGraph takes those launches off the enqueueing thread, whose launch rate is otherwise as tight a bound
        // on a single-stream step as the GPU (1.0-2.1 ms per step depending on the host core, vs 1.75 ms of GPU time).
        if (!b->pipe_graph_a[par]) {
            hipGraph_t graph = nullptr;
            SVA_HIP(hipStreamBeginCapture(sa, hipStreamCaptureModeThreadLocal));
            for (int ci = 0; ci < chunk && !rc; ++ci) rc = ar_decode_frame(b, ci, b->d_codes, b->T2, b->T2 - chunk + ci);
            const hipError_t ce = hipStreamEndCapture(sa, &graph);
            if (rc) { b->stream = se; return rc; }
            if (ce != hipSuccess || hipGraphInstantiate(&b->pipe_graph_a[par], graph, nullptr, nullptr, 0) != hipSuccess) {
                (void)hipGetLastError();                   // capture unavailable: enqueue this and every later AR stage kernel by kernel
                b->pipe_graph_a[par] = nullptr;
                b->pipe_graph_mode = 0;
            }
            if (graph) (void)hipGraphDestroy(graph);
        }
        if (b->pipe_graph_a[par]) {
            // the captured stage's persistent launches carry no cross-batch ordering of their own: chain the replay as a whole
            PersistentChain chain(b, sa, (b->use_mega || b->use_abatch) && !b->edits_on);
            rc = chain.rc;
            if (!rc) {
                SVA_HIP(hipGraphLaunch(b->pipe_graph_a[par], sa));
                rc = chain.finish();
            }
        } else for (int ci = 0; ci < chunk && !rc; ++ci) rc = ar_decode_frame(b, ci, b->d_codes, b->T2, b->T2 - chunk + ci);
    } else {
        for (int ci = 0; ci < chunk && !rc; ++ci) rc = ar_decode_frame(b, ci, b->d_codes, b->T2, b->T2 - chunk + ci);
    }
    if (rc) { b->stream = se; return rc; }
    if (stage_ev) SVA_HIP(hipEventRecord(b->ev[2], sa));
    SVA_TRY(mark(6, sa));
    hipEvent_t evA = next_event(b);
    SVA_HIP(hipEventRecord(evA, sa));
    b->pipe_evA[par] = evA;
    // V(n)
    SVA_HIP(hipStreamWaitEvent(sv, evA, 0));
    b->stream = sv;
    SVA_TRY(mark(7, sv));
    b->voc.codes = b->d_step_audio; b->voc.codes_bstride = (long)ncb * chunk; b->voc.codes_gstride = chunk;      // read in place ...
    b->pipe_evVc[par] = next_event(b);
    b->voc.codes_event = b->pipe_evVc[par];       // ... and A(n+1) may overwrite them once the FSQ decode has run
    if (b->stage_graphs && !b->voc.pcm_dst) {
        rc = vocode(b, chunk, true, VocPart::FsqOnly);           // FSQ decode (reads this parity's code buffer) + the release event, eagerly
        b->voc.codes_event = nullptr;
        if (!rc) rc = stage_graph(b, &b->gV, sv, [&]() -> int { b->stream = sv; return vocode(b, chunk, true, VocPart::AfterFsq); });
    } else {
        rc = vocode(b, chunk, true);
    }
    b->voc.codes = nullptr; b->voc.codes_event = nullptr;
    b->stream = se;
    if (rc) return rc;
    if (stage_ev) SVA_HIP(hipEventRecord(b->ev[3], sv));
    SVA_TRY(mark(8, sv));
    b->trace_steps += 1;
    b->n_pipe_steps += 1;
    b->pipe_dirty = true;
    b->out_stream = sv;
    return 0;
}

int quiesce(sva_batch* b) {
    if (!b || !b->pipe_dirty) return 0;
    hipStream_t se = b->main_stream;
    hipEvent_t e1 = next_event(b), e2 = next_event(b);
    SVA_HIP(hipEventRecord(e1, b->sa));
    SVA_HIP(hipEventRecord(e2, b->sv));
    SVA_HIP(hipStreamWaitEvent(se, e1, 0));
    SVA_HIP(hipStreamWaitEvent(se, e2, 0));
    if (b->aux0) {                         // (carries the encoder's transformer in the pipelined regime)
        hipEvent_t e3 = next_event(b);
        SVA_HIP(hipEventRecord(e3, b->aux0));
        SVA_HIP(hipStreamWaitEvent(se, e3, 0));
    }
    b->pipe_dirty = false;
    b->pipe_evVc[0] = b->pipe_evVc[1] = nullptr; b->pipe_evR = nullptr; b->pipe_evA[0] = b->pipe_evA[1] = nullptr;
        b->pipe_evFeat[0] = b->pipe_evFeat[1] = nullptr;
    b->out_stream = se;
    return 0;
}

// ---- per-slot restart (sva_stream_restart / sva_stream_retire): the rules are SlotBook's (slot_book.h), the device side is here ----
// the slot's flag as the book holds it -> d_slot_flag
int upload_slot_flag(sva_batch* b, int slot) {
    SVA_HIP(hipMemcpyAsync(b->d_slot_flag + slot, &b->slots.s[slot].flag, sizeof(int), hipMemcpyHostToDevice, b->stream));
    SVA_HIP(hipStreamSynchronize(b->stream));
    return 0;
}

// The restarted slot's front-end as sva_streams_begin leaves every slot: an all-zero audio window (origin-free: the ring position stays
// the batch's), every history row and every cached token at the network's steady response to silence, no content codes seen (device side).
int restart_encoder_state(sva_batch* b, int slot) {
    sva_engine* e = b->e;
    hipStream_t st = b->stream;
    const auto it = e->silence.find(std::make_pair(b->B, b->p.chunk_frames));
    SVA_CHECK(b->enc_incremental && it != e->silence.end(), "restart: no cached silence state for this encoder mode");
    const sva_engine::SilenceState& ss = it->second;
    EncMerged& M = b->em;
    std::vector<ShiftDesc> sd(M.n_shift);
    SVA_HIP(hipMemcpy(sd.data(), M.d_shift, sizeof(ShiftDesc) * M.n_shift, hipMemcpyDeviceToHost));
    SVA_CHECK(ss.rows.size() == sd.size(), "restart: silence state does not match the encoder's history buffers");
    SVA_HIP(hipMemsetAsync(b->ring + (long)slot * b->N, 0, sizeof(float) * (size_t)b->N, st));
    for (size_t i = 0; i < sd.size(); ++i) {
        const ShiftDesc& d = sd[i];
        SVA_TRY(launch_fill_rows(d.ptr + (long)slot * d.bstride, d.bstride, d.C, ss.rows[i], d.H, 1, st));
    }
    SVA_TRY(launch_fill_rows(b->d2c.p + (long)slot * b->d2c.bstride, b->d2c.bstride, e->cfg.tr_dim, ss.tok, b->T2, 1, st));
    SVA_HIP(hipMemsetAsync(b->d_ncontent + slot, 0, sizeof(int), st));
    return 0;
}

// The slot's streaming vocoder state becomes "zero state, then the last P frames of its prompt streamed in chunk-sized calls", as
// sva_streams_begin leaves every slot, through the production launches: save every slot's history rows, reset and prime the WHOLE batch
// with this slot's prompt tail, keep the slot's rows of the result and put everybody else's back.  Stalls all streams for P / chunk
// vocoder steps (tools/stream_restart_report.py measures it).
int prime_vocoder_slot(sva_batch* b, int slot) {
    const int B = b->B, c = b->p.chunk_frames, ncb = b->e->cfg.num_codebooks;
    const int nd = (int)b->voc.shift_host.size();
    hipStream_t st = b->stream;
    if (!b->voc_save) {
        std::vector<long> offs(nd);
        long tot = 0;
        for (int i = 0; i < nd; ++i) { offs[i] = tot; tot += (long)b->voc.shift_host[i].H * b->voc.shift_host[i].C; }
        b->voc_save_bstride = tot;
        SVA_TRY(dev_alloc(b->allocs, &b->d_voc_save_offs, (size_t)nd));
        SVA_HIP(hipMemcpy(b->d_voc_save_offs, offs.data(), sizeof(long) * nd, hipMemcpyHostToDevice));
        SVA_TRY(dev_alloc(b->allocs, &b->prime_pcm, (size_t)B * 2048 * c));
        SVA_TRY(dev_alloc(b->allocs, &b->voc_save, (size_t)B * tot));
    }
    const int P = b->slots.priming_frames(slot, b->p.decode_window_frames, c);
    int frames_kept = 0;
    SVA_HIP(hipMemcpy(&frames_kept, b->voc.d_frames, sizeof(int), hipMemcpyDeviceToHost));
    SVA_TRY(launch_history_rows_copy(b->voc.d_shift, nd, b->d_voc_save_offs, b->voc_save, b->voc_save_bstride, 0, B, 0, st));
    SVA_TRY(sva_vocode_reset(b));
    // the step that activates the slot may hold its PCM in d_pcm or in the caller's buffer: the priming run writes its own sink
    struct Keep {
        sva_batch* b; float* dst; long bs; bool done; double fl, by; long ln;
        ~Keep() { b->voc.pcm_dst = dst; b->voc.pcm_dst_bstride = bs; b->voc.pcm_direct_done = done; b->gemm_flops = fl; b->gemm_bytes = by; b->gemm_launches = ln; }
    } keep{b, b->voc.pcm_dst, b->voc.pcm_dst_bstride, b->voc.pcm_direct_done, b->gemm_flops, b->gemm_bytes, b->gemm_launches};
    b->voc.pcm_dst = b->prime_pcm; b->voc.pcm_dst_bstride = 2048L * c;
    std::vector<int32_t> codes((size_t)(P / c) * B * ncb * c);       // (alive until the copies have landed)
    for (int f = 0; f < P; f += c) {
        int32_t* cf = codes.data() + (size_t)(f / c) * B * ncb * c;
        for (int i = 0; i < B; ++i) b->slots.prompt_tail(slot, ncb, P, f, c, cf + (size_t)i * ncb * c);
        SVA_TRY(upload_vcodes(b, cf, c));
        SVA_TRY(vocode(b, c, true));
    }
    SVA_TRY(launch_history_rows_copy(b->voc.d_shift, nd, b->d_voc_save_offs, b->voc_save, b->voc_save_bstride, slot, 1, 0, st));
    SVA_TRY(launch_history_rows_copy(b->voc.d_shift, nd, b->d_voc_save_offs, b->voc_save, b->voc_save_bstride, 0, B, 1, st));
    SVA_HIP(hipMemcpyAsync(b->voc.d_frames, &frames_kept, sizeof(int), hipMemcpyHostToDevice, st));
    SVA_HIP(hipStreamSynchronize(st));
    return 0;
}

// Slot-local form of the above (sva_stream_params.slot_priming): the same state -- zero state, then the last P frames of the prompt -- built in
// the batch's one-stream workspace in ONE T = P pass, then moved into the slot by one kernel.  Nothing of the batch but the slot's history rows
// is written (voc.d_frames, the other slots, the PCM sinks and the GEMM counters stay), and the cost does not depend on the batch size.  The
// rows differ from the chunk-by-chunk ones by the rounding of other GEMM tilings only.  Runs on the batch's drained stream, never beside its steps.
int prime_vocoder_slot_local(sva_batch* b, int slot) {
    sva_batch* w = b->prime_ws;
    SVA_CHECK(w, "slot-local priming without a workspace");
    const int ncb = b->e->cfg.num_codebooks, nd = (int)b->voc.shift_host.size();
    SVA_CHECK(slot >= 0 && slot < b->B, "slot-local priming: slot out of range");
    const int P = b->slots.priming_frames(slot, b->p.decode_window_frames, b->p.chunk_frames);
    SVA_CHECK(P <= w->voc.Tv, "slot-local priming: prompt tail longer than the workspace");
    hipStream_t st = b->stream;
    w->stream = st;
    SVA_TRY(sva_vocode_reset(w));
    std::vector<int32_t> codes((size_t)ncb * std::max(P, 1));        // [1][8][P] (alive until the synchronisation below)
    b->slots.prompt_tail(slot, ncb, P, 0, P, codes.data());
    if (P > 0) {
        SVA_TRY(upload_vcodes(w, codes.data(), P));
        SVA_TRY(vocode(w, P, true));
    }
    SVA_TRY(launch_history_rows_move(w->voc.d_shift, b->voc.d_shift, nd, slot, st));
    SVA_HIP(hipStreamSynchronize(st));
    return 0;
}

// A restarted slot whose content count has reached the delay becomes a decoding stream: everything a parked step may have clobbered is
// rebuilt in the order a fresh stream sees it (sva_prefill_prompt, the delay fill of sva_streams_begin's first steps, the vocoder priming).
// Runs on drained streams.
int activate_slot(sva_batch* b, int slot) {
    const auto t0 = std::chrono::steady_clock::now();
    const PendingPrompt& P = b->slots.s[slot].pending;
    struct Keep { sva_batch* b; const float* src; ~Keep() { b->step_src = src; } } keep{b, b->step_src};
    b->step_src = nullptr;
    SVA_TRY(prefill_slot_impl(b, slot, P.cc.data(), P.ac.data(), P.R, P.style.data(), P.timbre.data(), P.seed, false));
    SVA_HIP(hipMemsetAsync(b->d_nframes + slot, 0, sizeof(int), b->stream));
    SVA_TRY(ar_delay_fill(b, std::vector<int>{slot}));
    SVA_TRY(b->prime_ws ? prime_vocoder_slot_local(b, slot) : prime_vocoder_slot(b, slot));
    b->slots.activated(slot);
    SVA_TRY(upload_slot_flag(b, slot));
    (b->prime_ws ? b->n_act_local : b->n_act_whole) += 1;
    b->last_act_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

int activate_due_slots(sva_batch* b) {
    const std::vector<int> due = b->slots.due_activations(b->p.delay);
    if (due.empty()) return 0;
    // rare: drain the stage streams of the pipelined mode and work on the main stream, as a re-prefill behind a host synchronisation does
    SVA_TRY(quiesce(b));
    b->stream = b->main_stream;
    SVA_HIP(hipStreamSynchronize(b->stream));
    for (int s_ : due) SVA_TRY(activate_slot(b, s_));
    return 0;
}

int step_body(sva_batch* b) {
    sva_engine* e = b->e;
    (void)e;
    if (b->h_ar_fail && *reinterpret_cast<volatile int*>(b->h_ar_fail) != 0) b->ar_failed = true;      // (a launch of an earlier step saw a wait time out)
    SVA_CHECK(!b->ar_failed, "this batch's persistent AR decode kernel timed out earlier: call sva_streams_begin to restart its streams");
    // callers of the stream-ordered API may never call sva_sync: the fp16-planes overflow flag is polled here too
    SVA_TRY(check_mm_overflow(b));
    const int B = b->B, chunk = b->p.chunk_frames, d = b->p.delay, n = 2048 * chunk;
    hipStream_t st = b->stream;
    const bool steady = b->slots.delay_filled;    // (set once the lock-step slots hold `delay` content codes; a restarted slot rides along parked)
    if (steady) {
        const bool graph_ok = b->p.use_graph && b->noise_on_device && !b->forced_now && !b->prof_on;
        const bool pipe_ok = b->p.pipeline && b->sa && b->allow_pipe && b->noise_on_device && !b->forced_now && !b->prof_on && !b->p.use_graph &&
                             b->steady_eager_steps >= 2;
        if (!pipe_ok) SVA_TRY(quiesce(b));
        if (pipe_ok) {
            SVA_TRY(steady_pipelined(b));
            b->graph_step = false;
        } else if (graph_ok && b->steady_eager_steps >= 2) {
            if (!b->graph_ready) {
                // capture once: every launch argument is a fixed device pointer or a constant; per-step variation
                // (ring position, KV positions, frame counters, sampler noise keys) lives in device memory
                hipGraph_t graph = nullptr;
                SVA_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
                int rc = steady_launches(b, false);
                hipError_t ce = hipStreamEndCapture(st, &graph);
                if (rc) return rc;
                SVA_HIP(ce);
                SVA_HIP(hipGraphInstantiate(&b->graph_exec, graph, nullptr, nullptr, 0));
                SVA_HIP(hipGraphDestroy(graph));
                b->graph_ready = true;
            }
            SVA_HIP(hipEventRecord(b->ev[0], st));
            {
                PersistentChain chain(b, st, (b->use_mega || b->use_abatch) && !b->edits_on);       // (as for the captured AR stage of the pipelined mode)
                SVA_TRY(chain.rc);
                SVA_HIP(hipGraphLaunch(b->graph_exec, st));
                SVA_TRY(chain.finish());
            }
            SVA_HIP(hipEventRecord(b->ev[3], st));
            b->graph_step = true;
        } else {
            SVA_TRY(steady_launches(b, true));
            b->steady_eager_steps += 1;
            b->graph_step = false;
        }
        // re-prefill when current_pos // 2 >= max_seq_frames (:547-564).  Positions are deterministic, so the book's mirrors decide without
        // a device round trip (SlotBook::steady_step); doing it after the vocoder instead of before (as the reference does) changes
        // nothing: the vocoder consumes the codes just decoded, the re-prefill only rewrites KV state.
        const StepPlan plan = b->slots.steady_step(chunk, b->p.max_seq_frames, e->cfg.timbre_tokens + 1);
        const std::vector<int>& redo = plan.redo;
        if (b->pipe_dirty) b->stream = b->sa;  // pipelined: the KV rewrite belongs to the AR stream (it already waited for E of this step)
        int rrc = 0;
        // a parked slot never becomes due: its position goes back to the end of its last stored prompt, over K / V rows that stay valid
        for (const auto& rw : plan.rewind)
            if (!rrc) rrc = launch_set_slot_i32(b->d_last_pos, rw.first, rw.second, b->stream);
        if (!rrc && !redo.empty()) {
            // one pass for all due slots against the cached prompt prefix (reprefill_slots); SVA_DEBUG reprefill=0: the round-3 path, one
            // whole-prompt prefill per slot behind a host synchronisation (A/B, parity of the two)
            const bool one_pass = debug_options().reprefill != 0 && b->slots.one_pass_ok(redo, b->p.buffer_frames, b->p.delay);
            if (one_pass) rrc = reprefill_slots(b, redo);
            else for (size_t i = 0; i < redo.size() && !rrc; ++i) rrc = reprefill_slot(b, redo[i]);
        }
        if (!rrc) rrc = ar_delay_fill(b, redo);       // prefill_src_condition4delay(src_content_codes[-d:]) for those slots only
        if (b->pipe_dirty) {
            b->stream = b->main_stream;
            if (!rrc && !redo.empty()) {       // E of the next step must not append to the content history before this has read it
                b->pipe_evR = next_event(b);
                SVA_HIP(hipEventRecord(b->pipe_evR, b->sa));
            }
        }
        if (!rrc) rrc = activate_due_slots(b);
        return rrc;
    }
    b->graph_step = false;
    SVA_TRY(quiesce(b));
    SVA_HIP(hipEventRecord(b->ev[0], st));
    // E0: shift window / append chunk (:495-496), then E1..E8
    SVA_TRY(launch_ring_write(b->ring, b->d_step, B, b->N, b->step_src ? b->step_src : b->d_chunk, n, st, b->d_slot_flag));
    SVA_TRY(b->enc_incremental ? encode_incremental(b, b->d_step, n, 1) : encode(b, b->d_step, n, 1));
    SVA_TRY(launch_append_content(b->d_codes, b->T2, chunk, b->d_content_hist, b->hist_cap, b->d_ncontent, b->d_step_content, B, b->d_step, st));
    SVA_HIP(hipEventRecord(b->ev[1], st));
    // the lock-step slots hold `delay` content codes: :521-525 -> zeros (else :519-520 -> zeros).  With every slot retired or restarted since
    // sva_streams_begin nothing is left to fill in lock step.
    if (b->slots.warmup_step(chunk, d)) SVA_TRY(ar_delay_fill(b));
    SVA_HIP(hipEventRecord(b->ev[2], st));
    SVA_HIP(hipMemsetAsync(b->voc.d_pcm, 0, sizeof(float) * (size_t)B * 2048 * b->voc.Tv, st));
    SVA_HIP(hipEventRecord(b->ev[3], st));
    return activate_due_slots(b);
}

}  // namespace

static int check_ar_fail(sva_batch* b);
static int io_restart_slot(sva_io* io, int slot);

// drained streams, main stream current: what the slot calls below change is read by the next step's launches
static int drain_for_slot_call(sva_batch* b) {
    SVA_HIP(hipSetDevice(b->e->device));
    (void)hipGetLastError();
    SVA_TRY(quiesce(b));
    b->stream = b->main_stream;
    SVA_HIP(hipStreamSynchronize(b->stream));
    return 0;
}
// the slot's position as the book holds it -> d_last_pos
static int upload_slot_position(sva_batch* b, int slot) {
    SVA_HIP(hipMemcpyAsync(b->d_last_pos + slot, &b->slots.s[slot].last_pos, sizeof(int), hipMemcpyHostToDevice, b->stream));
    SVA_HIP(hipStreamSynchronize(b->stream));
    return 0;
}
// the slot's sampling pair as the book holds it -> d_samp
static int upload_slot_sampling(sva_batch* b, int slot) {
    SVA_HIP(hipMemcpyAsync(b->d_samp + 2 * slot, b->slots.s[slot].samp, sizeof(float) * 2, hipMemcpyHostToDevice, b->stream));
    SVA_HIP(hipStreamSynchronize(b->stream));
    return 0;
}

extern "C" int sva_stream_restart(sva_batch* b, int slot, const int64_t* ref_content_codes, const int32_t* ref_audio_codes, int R, const float* style,
                                  const float* timbre, uint64_t noise_seed) {
    SVA_CHECK(b && ref_content_codes && ref_audio_codes && style && timbre, "sva_stream_restart: null argument");
    SVA_CHECK(b->begun, "sva_stream_restart: the batch has not begun (sva_prefill_prompt + sva_streams_begin start its first streams)");
    SVA_CHECK(slot >= 0 && slot < b->B, "sva_stream_restart: slot out of range");
    const sva_config& c = b->e->cfg;
    const int ncb = c.num_codebooks, nspk = c.timbre_tokens + 1;
    SVA_CHECK(R > b->p.delay, "sva_stream_restart: the prompt must be longer than the delay");
    SVA_CHECK(R <= b->Pmax && nspk + 2 * R <= b->Mmax && nspk + 2 * R <= c.max_seq_len, "sva_stream_restart: prompt too long for the KV cache");
    const int P = SlotBook::priming_frames_for(std::min(R, b->p.max_prompt_frames), b->p.decode_window_frames, b->p.chunk_frames);
    SVA_CHECK(P >= 16 || P == b->p.decode_window_frames - 1, "sva_stream_restart: prompt shorter than the vocoder receptive field (16 frames)");
    SVA_CHECK(b->enc_incremental,
              "sva_stream_restart: this batch runs the full-window encoder (encode_window_frames <= 40 + chunk_frames), which has no cached "
              "silence state to fill one slot from");
    SVA_CHECK(!b->ar_failed && !(b->h_ar_fail && *reinterpret_cast<volatile int*>(b->h_ar_fail) != 0),
              "sva_stream_restart: this batch's persistent AR decode kernel timed out: sva_streams_begin restarts its streams");
    SVA_TRY(drain_for_slot_call(b));
    SVA_TRY(restart_encoder_state(b, slot));           // (its own refusal -- no silence state -- comes before its first write)
    PendingPrompt P_;
    P_.cc.assign(ref_content_codes, ref_content_codes + R);
    P_.ac.assign(ref_audio_codes, ref_audio_codes + (size_t)ncb * R);
    P_.style.assign(style, style + c.style_dim);
    P_.timbre.assign(timbre, timbre + (size_t)c.timbre_tokens * c.timbre_dim);
    P_.R = R; P_.seed = noise_seed;
    b->slots.restart(slot, std::move(P_), nspk, kSlotOutputMuted);      // (... and back to the batch's sampling pair)
    if (b->io) SVA_TRY(io_restart_slot(b->io, slot));
    SVA_TRY(upload_slot_position(b, slot));
    SVA_TRY(upload_slot_sampling(b, slot));
    return upload_slot_flag(b, slot);
}

extern "C" int sva_stream_retire(sva_batch* b, int slot) {
    SVA_CHECK(b, "sva_stream_retire: null batch");
    SVA_CHECK(b->begun, "sva_stream_retire: the batch has not begun");
    SVA_CHECK(slot >= 0 && slot < b->B, "sva_stream_retire: slot out of range");
    SVA_TRY(drain_for_slot_call(b));
    b->slots.retire(slot, kSlotInputMuted | kSlotOutputMuted);
    return upload_slot_flag(b, slot);
}

extern "C" int sva_stream_set_sampling(sva_batch* b, int slot, float temperature, float top_p) {
    SVA_CHECK(b, "sva_stream_set_sampling: null batch");
    SVA_CHECK(slot >= 0 && slot < b->B, "sva_stream_set_sampling: slot out of range");
    SVA_CHECK(std::isfinite(temperature) && temperature >= 0.f, "sva_stream_set_sampling: temperature must be finite and >= 0");
    SVA_CHECK(std::isfinite(top_p) && top_p >= 0.f, "sva_stream_set_sampling: top_p must be finite and >= 0");
    SVA_TRY(drain_for_slot_call(b));
    b->slots.set_sampling(slot, temperature, top_p);
    return upload_slot_sampling(b, slot);
}

extern "C" int sva_stream_get_sampling(sva_batch* b, int slot, float* temperature, float* top_p) {
    SVA_CHECK(b, "sva_stream_get_sampling: null batch");
    SVA_CHECK(slot >= 0 && slot < b->B, "sva_stream_get_sampling: slot out of range");
    if (temperature) *temperature = b->slots.s[slot].temperature;
    if (top_p) *top_p = b->slots.s[slot].samp[1];
    return 0;
}

extern "C" int sva_stream_state(sva_batch* b, int slot, int* phase, long* frames) {
    SVA_CHECK(b && b->begun, "sva_stream_state: the batch has not begun");
    SVA_CHECK(slot >= 0 && slot < b->B, "sva_stream_state: slot out of range");
    if (phase) *phase = b->slots.s[slot].phase;
    if (frames) *frames = b->slots.stream_frames(slot);
    return 0;
}

extern "C" int sva_stream_activations(sva_batch* b, long counts[2], float* last_ms) {
    SVA_CHECK(b && counts, "sva_stream_activations: null argument");
    counts[0] = b->n_act_local;
    counts[1] = b->n_act_whole;
    if (last_ms) *last_ms = b->last_act_ms;
    return 0;
}

// ---- save / load single streams (sva_stream_save / sva_stream_load): the inventory is snapshot/slot_state.h, the container
// snapshot/snapshot_format.h, the kernels snapshot/slot_pack.hip; the mirrors change through SlotBook::adopt alone ----
namespace {
const char* snap_reason(int rc) {
    switch (rc) {
        case snap::kTruncated: return "the blob is truncated (fewer bytes than its header needs or states)";
        case snap::kBadMagic: return "not a stream snapshot (wrong magic)";
        case snap::kBadVersion: return "the blob has another format version";
        case snap::kBadHeader: return "the blob's header is corrupt (a length contradicts another, or its checksum fails)";
        case snap::kBadChecksum: return "the blob's payload fails its checksum";
        case snap::kConfigMismatch: return "the blob's configuration differs from the batch's";
        case snap::kLayoutMismatch: return "the blob's layout differs from the batch's";
        case snap::kSizeMismatch: return "the blob's payload length is not what this batch's segments hold at the blob's KV position";
        default: return "unknown refusal";
    }
}
int snap_cus(sva_batch* b, int* cus) {
    SVA_HIP(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, b->e->device));
    if (b->ar_partitioned && b->enc_cus > 0) *cus = std::min(*cus, b->enc_cus);      // the main stream's CU mask
    return 0;
}
// room for an image and a segment table in the batch's own device buffers; the table uploaded (the caller's stream is drained: plain copies)
int snap_prepare(sva_batch* b, const SlotSegments& L) {
    SVA_TRY(check_slot_segments(L));
    if (b->snap_image_cap < L.image_bytes) {
        if (b->snap_image) SVA_HIP(hipFree(b->snap_image));
        b->snap_image = nullptr; b->snap_image_cap = 0;
        SVA_HIP(hipMalloc(&b->snap_image, (size_t)L.image_bytes));
        b->snap_image_cap = L.image_bytes;
    }
    const long tb = (long)(sizeof(SlotSegment) * L.seg.size());
    if (b->snap_table_cap < tb) {
        if (b->snap_table) SVA_HIP(hipFree(b->snap_table));
        b->snap_table = nullptr; b->snap_table_cap = 0;
        SVA_HIP(hipMalloc(&b->snap_table, (size_t)tb));
        b->snap_table_cap = tb;
    }
    SVA_HIP(hipMemcpyAsync(b->snap_table, L.seg.data(), (size_t)tb, hipMemcpyHostToDevice, b->stream));
    SVA_HIP(hipStreamSynchronize(b->stream));
    return 0;
}
int snap_check_batch(sva_batch* b, int slot, const char* who) {
    const std::string w(who);
    SVA_CHECK(b, (w + ": null batch").c_str());
    SVA_CHECK(b->begun, (w + ": the batch has not begun").c_str());
    SVA_CHECK(slot >= 0 && slot < b->B, (w + ": slot out of range").c_str());
    SVA_CHECK(!b->io, (w + ": an I/O adaptor is open on this batch; its FIFOs and phase counters are batch-wide and do not travel (close it first)").c_str());
    SVA_CHECK(!b->ar_failed && !(b->h_ar_fail && *reinterpret_cast<volatile int*>(b->h_ar_fail) != 0),
              (w + ": this batch's persistent AR decode kernel timed out: sva_streams_begin restarts its streams").c_str());
    return 0;
}
// the split of the call that just ended: kernel between the events ev[0] / ev[1], copy = [c0, c1] on the wall clock, host work = the rest of the call
typedef std::chrono::steady_clock::time_point snap_tp;
void snap_record_times(sva_batch* b, snap_tp begin, snap_tp c0, snap_tp c1, long bytes) {
    float k = 0.f;
    if (hipEventElapsedTime(&k, b->ev[0], b->ev[1]) != hipSuccess) { (void)hipGetLastError(); k = 0.f; }
    const float copy = std::chrono::duration<float, std::milli>(c1 - c0).count();
    const float total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - begin).count();
    b->snap_ms[0] = k; b->snap_ms[1] = copy; b->snap_ms[2] = std::max(0.f, total - k - copy);
    b->snap_last_bytes = bytes;
}
snap::Fields snap_fields(sva_batch* b, int slot) {
    const SlotHost& h = b->slots.s[slot];
    snap::Fields f;
    f.nframes = h.nframes; f.last_pos = h.last_pos; f.ncontent = h.ncontent; f.ar_dtype = b->e->cfg.ar_dtype; f.chunk_frames = b->p.chunk_frames;
    f.temperature = h.temperature; f.inv_temp = h.samp[0]; f.top_p = h.samp[1];
    f.ncb = b->e->cfg.num_codebooks;
    f.ref_content = h.ref_content; f.ref_audio = h.ref_audio;
    return f;
}
}  // namespace

extern "C" long sva_stream_save_size(sva_batch* b, int slot) {
    SVA_TRY(snap_check_batch(b, slot, "sva_stream_save_size"));
    const SlotHost& h = b->slots.s[slot];
    SVA_CHECK(h.phase == kSlotDecoding, "sva_stream_save_size: only a decoding slot (phase 2) can be saved");
    SlotSegments L;
    SVA_TRY(slot_segments(b, h.last_pos + 1, &L));
    const size_t n_cfg = config_signature(b->e->cfg, b->p).size(), n_layout = layout_signature(b, L).size();
    return (long)snap::header_bytes_for(n_cfg, n_layout, h.ref_content.size(), (uint64_t)b->e->cfg.num_codebooks) + L.image_bytes;
}

extern "C" int sva_stream_save(sva_batch* b, int slot, void* blob, long cap, long* written) {
    SVA_TRY(snap_check_batch(b, slot, "sva_stream_save"));
    SVA_CHECK(written, "sva_stream_save: null argument");
    SVA_CHECK(b->slots.s[slot].phase == kSlotDecoding, "sva_stream_save: only a decoding slot (phase 2) can be saved");
    const auto t_begin = std::chrono::steady_clock::now();
    SVA_TRY(drain_for_slot_call(b));
    const SlotHost& h = b->slots.s[slot];
    SlotSegments L;
    SVA_TRY(slot_segments(b, h.last_pos + 1, &L));
    const std::vector<int64_t> cfg = config_signature(b->e->cfg, b->p), layout = layout_signature(b, L);
    const snap::Fields f = snap_fields(b, slot);
    const long hb = (long)snap::header_bytes_for(cfg.size(), layout.size(), f.ref_content.size(), (uint64_t)f.ncb);
    *written = hb + L.image_bytes;
    SVA_CHECK(blob && cap >= *written, "sva_stream_save: the buffer is smaller than the snapshot (*written holds the bytes needed)");
    SVA_TRY(snap_prepare(b, L));
    int cus = 0;
    SVA_TRY(snap_cus(b, &cus));
    // the three parts are timed (sva_test_snapshot_timings): the kernel between two events, the copy and the host work on the wall clock
    SVA_HIP(hipEventRecord(b->ev[0], b->stream));
    SVA_TRY(launch_slot_pack(static_cast<const SlotSegment*>(b->snap_table), (int)L.seg.size(), slot, b->d_step, b->snap_image, L.image_bytes, cus, b->stream));
    SVA_HIP(hipEventRecord(b->ev[1], b->stream));
    SVA_HIP(hipStreamSynchronize(b->stream));
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t* out = static_cast<uint8_t*>(blob);
    SVA_HIP(hipMemcpyAsync(out + hb, b->snap_image, (size_t)L.image_bytes, hipMemcpyDeviceToHost, b->stream));
    SVA_HIP(hipStreamSynchronize(b->stream));
    const auto t1 = std::chrono::steady_clock::now();
    snap::write_header(out, cfg, layout, f, (uint64_t)L.image_bytes, snap::fnv1a64_words(out + hb, (size_t)L.image_bytes));
    snap_record_times(b, t_begin, t0, t1, L.image_bytes);
    return 0;
}

extern "C" int sva_stream_blob_info(const void* blob, long nbytes, long* info) {
    SVA_CHECK(blob && info, "sva_stream_blob_info: null argument");
    snap::Header h;
    const int rc = snap::parse(blob, nbytes, true, &h);
    if (rc) { set_error(std::string("sva_stream_blob_info: ") + snap_reason(rc)); return rc; }
    info[0] = h.version; info[1] = h.f.nframes; info[2] = h.f.last_pos; info[3] = h.f.ncontent; info[4] = (long)h.f.ref_content.size();
    info[5] = h.f.ar_dtype; info[6] = h.f.chunk_frames; info[7] = (long)h.payload_bytes;
    return 0;
}

extern "C" int sva_stream_load(sva_batch* b, int slot, const void* blob, long nbytes) {
    SVA_TRY(snap_check_batch(b, slot, "sva_stream_load"));
    SVA_CHECK(blob, "sva_stream_load: null argument");
    const auto t_begin = std::chrono::steady_clock::now();
    SVA_CHECK(b->slots.delay_filled, "sva_stream_load: the batch's lock-step delay has not filled yet (step it ceil(delay / chunk) times first)");
    const sva_config& c = b->e->cfg;
    snap::Header h;
    int rc = snap::parse(blob, nbytes, true, &h);
    if (rc) { set_error(std::string("sva_stream_load: ") + snap_reason(rc)); return rc; }
    {
        std::vector<std::string> names;
        const std::vector<int64_t> cfg = config_signature(c, b->p, &names);
        const long d = snap::first_difference(h.cfg, cfg);
        if (d >= 0) {
            const std::string nm = d < (long)names.size() ? names[(size_t)d] : std::string("number of fields");
            set_error(std::string("sva_stream_load: ") + snap_reason(snap::kConfigMismatch) + ": first differing field " + std::to_string(d) + " (" + nm + ")" +
                      (d < (long)h.cfg.size() && d < (long)cfg.size() ? ": blob " + std::to_string(h.cfg[(size_t)d]) + ", batch " + std::to_string(cfg[(size_t)d]) : ""));
            return snap::kConfigMismatch;
        }
    }
    const snap::Fields& f = h.f;
    // a decoding stream's counters hang together: its position lies behind its stored prompt's prefill and delay fill, it has seen at least
    // `delay` content codes and has decoded no more frames than the codes beyond them
    const long ref_len = (long)f.ref_content.size(), nspk = c.timbre_tokens + 1;
    bool fields_ok = f.last_pos >= 0 && f.last_pos + 2 * b->p.chunk_frames < c.max_seq_len && f.nframes >= 0 && f.ncontent >= 0 && f.ncb == c.num_codebooks &&
                     ref_len >= 1 && ref_len <= b->p.max_prompt_frames && f.ar_dtype == c.ar_dtype && f.chunk_frames == b->p.chunk_frames &&
                     std::isfinite(f.temperature) && std::isfinite(f.inv_temp) && std::isfinite(f.top_p) && f.inv_temp > 0.f && f.top_p >= 0.f &&
                     f.last_pos >= nspk + 2 * ref_len - 1 + 2 * b->p.delay - 1 && f.ncontent >= b->p.delay && f.nframes <= f.ncontent - b->p.delay;
    // ... and the stored prompt's codes index the embedding tables (re-prefill, vocoder priming)
    for (size_t i = 0; fields_ok && i < f.ref_content.size(); ++i) fields_ok = f.ref_content[i] >= 0 && f.ref_content[i] < c.ar_vocab;
    for (size_t i = 0; fields_ok && i < f.ref_audio.size(); ++i) fields_ok = f.ref_audio[i] >= 0 && f.ref_audio[i] < c.codebook_size;
    if (!fields_ok) { set_error(std::string("sva_stream_load: ") + snap_reason(snap::kBadHeader) + ": a slot field is out of range for this batch"); return snap::kBadHeader; }
    SlotSegments L;
    SVA_TRY(slot_segments(b, f.last_pos + 1, &L));
    {
        std::vector<std::string> names;
        const std::vector<int64_t> layout = layout_signature(b, L, &names);
        const long d = snap::first_difference(h.layout, layout);
        if (d >= 0) {
            const std::string nm = d < (long)names.size() ? names[(size_t)d] : std::string("number of fields");
            set_error(std::string("sva_stream_load: ") + snap_reason(snap::kLayoutMismatch) + ": first differing field " + std::to_string(d) + " (" + nm + ")");
            return snap::kLayoutMismatch;
        }
    }
    if ((long)h.payload_bytes != L.image_bytes) { set_error(std::string("sva_stream_load: ") + snap_reason(snap::kSizeMismatch)); return snap::kSizeMismatch; }
    const uint8_t* in = static_cast<const uint8_t*>(blob);
    // The integer tables of the payload are gather indices of the delay fill and the re-prefill (content_emb[code], codebook_emb[q * size + code]):
    // a checksum is no proof of origin, so every entry is range-checked here, on the host, before anything changes.  (Unused ring entries are
    // zeros: the rings are allocated zeroed and only ever receive codes.)
    for (size_t i = 0; i < L.seg.size(); ++i) {
        const std::string& nm = L.name[i];
        const int hi = nm == "d_content_hist" ? c.ar_vocab : (nm == "d_pred_hist" || nm == "d_ref_tail") ? c.codebook_size : 0;
        if (!hi) continue;
        const uint8_t* q = in + h.header_bytes + L.seg[i].img_off;
        for (long k = 0; k < seg_payload(L.seg[i]); k += 4) {
            const int32_t v = (int32_t)snap::get_u32(q + k);
            if (v < 0 || v >= hi) {
                set_error(std::string("sva_stream_load: ") + snap_reason(snap::kBadHeader) + ": a code in " + nm + " is outside its embedding table");
                return snap::kBadHeader;
            }
        }
    }
    // ---- everything is validated: from here on state changes ----
    SVA_TRY(drain_for_slot_call(b));
    SVA_TRY(snap_prepare(b, L));
    int cus = 0;
    SVA_TRY(snap_cus(b, &cus));
    const auto t0 = std::chrono::steady_clock::now();
    SVA_HIP(hipMemcpyAsync(b->snap_image, in + h.header_bytes, (size_t)L.image_bytes, hipMemcpyHostToDevice, b->stream));
    SVA_HIP(hipStreamSynchronize(b->stream));
    const auto t1 = std::chrono::steady_clock::now();
    SVA_HIP(hipEventRecord(b->ev[0], b->stream));
    SVA_TRY(launch_slot_unpack(static_cast<const SlotSegment*>(b->snap_table), (int)L.seg.size(), slot, b->d_step, b->snap_image, L.image_bytes, cus, b->stream));
    SVA_HIP(hipEventRecord(b->ev[1], b->stream));
    SVA_HIP(hipStreamSynchronize(b->stream));
    std::vector<int64_t> rc_(f.ref_content);
    std::vector<int32_t> ra_(f.ref_audio);
    b->slots.adopt(slot, f.last_pos, f.nframes, f.ncontent, std::move(rc_), std::move(ra_), f.temperature, f.inv_temp, f.top_p);
    // the device words the mirrors stand for, from the mirrors (they arrived in the payload too: a blob cannot leave the two apart)
    const SlotHost& sh = b->slots.s[slot];
    SVA_HIP(hipMemcpyAsync(b->d_nframes + slot, &sh.nframes, sizeof(int), hipMemcpyHostToDevice, b->stream));
    SVA_HIP(hipMemcpyAsync(b->d_ncontent + slot, &sh.ncontent, sizeof(int), hipMemcpyHostToDevice, b->stream));
    SVA_TRY(upload_slot_position(b, slot));
    SVA_TRY(upload_slot_sampling(b, slot));
    SVA_TRY(upload_slot_flag(b, slot));
    snap_record_times(b, t_begin, t0, t1, L.image_bytes);
    return 0;
}

// Timings of the batch's last sva_stream_save / sva_stream_load (include/sva.h)
extern "C" int sva_test_snapshot_timings(sva_batch* b, int measure_d2d, float* ms, long* counts) {
    SVA_CHECK(b && ms && counts, "sva_test_snapshot_timings: null argument");
    ms[0] = b->snap_ms[0]; ms[1] = b->snap_ms[1]; ms[2] = b->snap_ms[2]; ms[3] = -1.f;
    counts[0] = b->snap_last_bytes; counts[1] = b->n_pipe_steps;
    if (!measure_d2d) return 0;
    SVA_CHECK(b->snap_image && b->snap_last_bytes > 0, "sva_test_snapshot_timings: no save or load has run on this batch");
    SVA_TRY(drain_for_slot_call(b));
    void* tmp = nullptr;
    SVA_HIP(hipMalloc(&tmp, (size_t)b->snap_last_bytes));
    hipError_t e1 = hipEventRecord(b->ev[0], b->stream);
    if (e1 == hipSuccess) e1 = hipMemcpyDtoDAsync(tmp, b->snap_image, (size_t)b->snap_last_bytes, b->stream);
    if (e1 == hipSuccess) e1 = hipEventRecord(b->ev[1], b->stream);
    if (e1 == hipSuccess) e1 = hipStreamSynchronize(b->stream);
    if (e1 == hipSuccess) e1 = hipEventElapsedTime(&ms[3], b->ev[0], b->ev[1]);
    (void)hipFree(tmp);
    SVA_HIP(e1);
    return 0;
}

extern "C" int sva_step(sva_batch* b, const float* pcm_in, float* pcm_out, const float* noise, const int32_t* forced_codes) {
    SVA_CHECK(b && pcm_in && pcm_out && b->begun, "sva_step: bad argument or sva_streams_begin not called");
    SVA_CHECK(!b->io, "sva_step: an I/O adaptor is open on this batch (sva_io_open): stepping it directly would desynchronise the adaptor's FIFOs -- use sva_io_process or close the adaptor");
    SVA_HIP(hipSetDevice(b->e->device));
    (void)hipGetLastError();
    SVA_TRY(quiesce(b));
    const sva_config& c = b->e->cfg;
    const int B = b->B, chunk = b->p.chunk_frames, n = 2048 * chunk, ncb = c.num_codebooks;
    hipStream_t st = b->stream;
    memcpy(b->hp_in, pcm_in, sizeof(float) * (size_t)B * n);
    SVA_HIP(hipMemcpyAsync(b->d_chunk, b->hp_in, sizeof(float) * (size_t)B * n, hipMemcpyHostToDevice, st));
    b->noise_on_device = (noise == nullptr);
    if (noise)
        SVA_HIP(hipMemcpyAsync(b->d_noise, noise, sizeof(float) * (size_t)B * chunk * (c.ar_vocab + ncb * c.codebook_size), hipMemcpyHostToDevice, st));
    b->forced_now = forced_codes != nullptr;
    const int uf = forced_codes ? 1 : 0;
    SVA_HIP(hipMemcpyAsync(b->d_use_forced, &uf, sizeof(int), hipMemcpyHostToDevice, st));
    b->h_use_forced = uf;
    if (forced_codes) SVA_HIP(hipMemcpyAsync(b->d_forced, forced_codes, sizeof(int) * (size_t)B * ncb * chunk, hipMemcpyHostToDevice, st));
    SVA_HIP(hipStreamSynchronize(st));
    b->gemm_flops = 0; b->gemm_launches = 0; b->gemm_bytes = 0;
    SVA_TRY(step_body(b));
    SVA_HIP(hipMemcpy2DAsync(b->hp_out, sizeof(float) * n, b->voc.d_pcm, sizeof(float) * 2048 * b->voc.Tv, sizeof(float) * n, B, hipMemcpyDeviceToHost, st));
    SVA_HIP(hipStreamSynchronize(st));
    SVA_TRY(check_ar_fail(b));
    memcpy(pcm_out, b->hp_out, sizeof(float) * (size_t)B * n);
    float t;
    if (!b->graph_step)
        for (int i = 0; i < 3; ++i) {
            if (hipEventElapsedTime(&t, b->ev[i], b->ev[i + 1]) == hipSuccess) b->last_ms[i] = t;
        }
    if (hipEventElapsedTime(&t, b->ev[0], b->ev[3]) == hipSuccess) b->last_ms[3] = t;
    return 0;
}

extern "C" int sva_step_device(sva_batch* b, const float* d_pcm_in, float* d_pcm_out) {
    SVA_CHECK(b && d_pcm_in && d_pcm_out && b->begun, "sva_step_device: bad argument");
    SVA_CHECK(!b->io || b->io_stepping, "sva_step_device: an I/O adaptor is open on this batch (sva_io_open): stepping it directly would desynchronise the adaptor's FIFOs -- use sva_io_process or close the adaptor");
    SVA_HIP(hipSetDevice(b->e->device));
    (void)hipGetLastError();
    const int B = b->B, n = 2048 * b->p.chunk_frames;
    hipStream_t st = b->main_stream;
    b->stream = st;
    // no staging: the ring write reads the caller's chunk, the vocoder's last kernel writes the caller's PCM buffer and
    // the FSQ decode reads the step's codes in place (each staging copy was a kernel of its own in a chain whose length is
    // what bounds the step)
    const bool direct = !b->p.use_graph && !(b->p.pipeline && b->stage_graphs);       // a captured graph bakes its pointers: it keeps the fixed staging buffers
    if (direct) b->step_src = d_pcm_in;
    else SVA_HIP(hipMemcpyAsync(b->d_chunk, d_pcm_in, sizeof(float) * (size_t)B * n, hipMemcpyDeviceToDevice, st));
    b->noise_on_device = true;
    b->forced_now = false;
    if (b->h_use_forced != 0) { SVA_HIP(hipMemsetAsync(b->d_use_forced, 0, sizeof(int), st)); b->h_use_forced = 0; }
    b->gemm_flops = 0; b->gemm_launches = 0; b->gemm_bytes = 0;
    b->allow_pipe = true;
    b->out_stream = st;
    b->voc.pcm_dst = direct ? d_pcm_out : nullptr; b->voc.pcm_dst_bstride = n; b->voc.pcm_direct_done = false;
    const int rc = step_body(b);
    b->allow_pipe = false;
    b->step_src = nullptr; b->voc.pcm_dst = nullptr;
    if (rc) return rc;
    if (!b->voc.pcm_direct_done)     // delay warm-up steps run no vocoder: their zeros come from d_pcm
        SVA_HIP(hipMemcpy2DAsync(d_pcm_out, sizeof(float) * n, b->voc.d_pcm, sizeof(float) * 2048 * b->voc.Tv, sizeof(float) * n, B, hipMemcpyDeviceToDevice,
                                 b->out_stream));
    return 0;
}

// Stream-ordered variants: the reference's process_one_chunk runs on the caller's current stream, so whatever filled the input
// buffer is ordered before it and whatever reads the output after it (evaluations/infer_arvc.py:495-508 on torch's stream).  The
// engine keeps streams of its own; these entry points tie them to the caller's stream with events instead of host synchronisation.
extern "C" int sva_step_device_on(sva_batch* b, const float* d_pcm_in, float* d_pcm_out, void* caller_stream, int join_output) {
    SVA_CHECK(b && b->begun, "sva_step_device_on: bad argument");
    SVA_CHECK(!b->io, "sva_step_device_on: an I/O adaptor is open on this batch (sva_io_open): stepping it directly would desynchronise the adaptor's FIFOs -- use sva_io_process or close the adaptor");
    SVA_HIP(hipSetDevice(b->e->device));
    hipStream_t cs = (hipStream_t)caller_stream;
    {   // everything already enqueued on the caller's stream happens before the engine's first access to d_pcm_in
        hipEvent_t ev = next_event(b);
        SVA_HIP(hipEventRecord(ev, cs));
        SVA_HIP(hipStreamWaitEvent(b->main_stream, ev, 0));
    }
    SVA_TRY(sva_step_device(b, d_pcm_in, d_pcm_out));
    if (join_output) return sva_join_stream(b, caller_stream);
    return 0;
}

extern "C" int sva_join_stream(sva_batch* b, void* caller_stream) {
    SVA_CHECK(b, "null batch");
    SVA_HIP(hipSetDevice(b->e->device));
    hipStream_t cs = (hipStream_t)caller_stream;
    // the caller's stream waits (on the device, not the host) for every chain of the engine: the stage streams of a pipelined batch,
    // the encoder's side stream and the main stream; the pipelined regime itself is left untouched
    hipStream_t all[4] = {b->main_stream, b->p.pipeline ? b->sa : nullptr, b->p.pipeline ? b->sv : nullptr, b->aux0};
    for (hipStream_t st_ : all) {
        if (!st_) continue;
        hipEvent_t ev = next_event(b);
        SVA_HIP(hipEventRecord(ev, st_));
        SVA_HIP(hipStreamWaitEvent(cs, ev, 0));
    }
    if (b->out_stream && b->out_stream != b->main_stream) {
        hipEvent_t ev = next_event(b);
        SVA_HIP(hipEventRecord(ev, b->out_stream));
        SVA_HIP(hipStreamWaitEvent(cs, ev, 0));
    }
    return 0;
}

extern "C" int sva_stream_chunks(sva_batch* b, const float* pcm_in, float* pcm_out, int n_chunks) {
    SVA_CHECK(b && pcm_in && pcm_out && b->begun && n_chunks >= 1, "sva_stream_chunks: bad argument");
    SVA_CHECK(!b->io, "sva_stream_chunks: an I/O adaptor is open on this batch (sva_io_open): stepping it directly would desynchronise the adaptor's FIFOs -- use sva_io_process or close the adaptor");
    SVA_HIP(hipSetDevice(b->e->device));
    (void)hipGetLastError();
    SVA_TRY(quiesce(b));
    const int B = b->B, n = 2048 * b->p.chunk_frames;
    const size_t per = (size_t)B * n;
    float *d_in = nullptr, *d_out = nullptr;
    SVA_HIP(hipMalloc((void**)&d_in, sizeof(float) * per * n_chunks));
    SVA_HIP(hipMalloc((void**)&d_out, sizeof(float) * per * n_chunks));
    hipStream_t st = b->main_stream;
    // [B][n_chunks*n] on the host <-> [n_chunks][B][n] on the device (one contiguous block per step)
    int rc = 0;
    for (int k = 0; k < n_chunks && !rc; ++k)
        if (hipMemcpy2DAsync(d_in + per * k, sizeof(float) * n, pcm_in + (size_t)k * n, sizeof(float) * n * n_chunks, sizeof(float) * n, B,
                             hipMemcpyHostToDevice, st) != hipSuccess) { set_error("sva_stream_chunks: upload failed"); rc = -2; }
    for (int k = 0; k < n_chunks && !rc; ++k) rc = sva_step_device(b, d_in + per * k, d_out + per * k);
    if (!rc) rc = sva_sync(b);
    for (int k = 0; k < n_chunks && !rc; ++k)
        if (hipMemcpy2DAsync(pcm_out + (size_t)k * n, sizeof(float) * n * n_chunks, d_out + per * k, sizeof(float) * n, sizeof(float) * n, B,
                             hipMemcpyDeviceToHost, st) != hipSuccess) { set_error("sva_stream_chunks: download failed"); rc = -2; }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) { set_error("sva_stream_chunks: sync failed"); rc = -2; }
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
}

// the persistent decode kernel gives up on a hand-off that does not arrive (bounded spin) and records where: surface it at the
// next synchronisation instead of returning garbage codes
static int check_ar_fail(sva_batch* b) {
    if ((!b->use_mega && !b->use_abatch) || !b->d_ar_fail) return 0;
    int f = 0;
    SVA_HIP(hipMemcpy(&f, b->d_ar_fail, sizeof(int), hipMemcpyDeviceToHost));
    if (f != 0) b->ar_failed = true;
    SVA_CHECK(f == 0, "persistent AR decode kernel timed out waiting for a workgroup hand-off (code " + std::to_string(f) +
                      "): its workgroups were not all resident (GPU shared with another process / a long kernel?).  The frames since the last "
                      "synchronisation are invalid; sva_streams_begin restarts the streams on the multi-launch decode");
    return 0;
}

// test / tool hook: change debug options of this process after start-up ("key=value,..." as in SVA_DEBUG; batches created afterwards
// see them -- the GEMM dispatch table and the autotune switch are read once, before the first launch)
extern "C" int sva_debug_configure(const char* kv) {
    SVA_CHECK(kv, "null argument");
    DebugOptions& o = sva::debug_options_mut();
    const int cap_before = o.hist_cap;
    parse_debug(o, kv);
    if (o.hist_cap < 1 || (o.hist_cap & (o.hist_cap - 1)) != 0) {       // (the other half of the rule, buffer_frames + delay + chunk < N, is the batch's to check)
        o.hist_cap = cap_before;
        SVA_CHECK(false, "sva_debug_configure: hist_cap must be a power of two");
    }
    return 0;
}

// test hook: make the batch look as if its persistent decode kernel had timed out (sets the device-side fail word)
extern "C" int sva_test_force_ar_timeout(sva_batch* b) {
    SVA_CHECK(b && (b->use_mega || b->use_abatch) && b->d_ar_fail, "sva_test_force_ar_timeout: the batch does not use the persistent decode kernel");
    SVA_HIP(hipSetDevice(b->e->device));
    SVA_TRY(quiesce(b));
    SVA_HIP(hipStreamSynchronize(b->stream));
    const int code = 99;
    SVA_HIP(hipMemcpy(b->d_ar_fail, &code, sizeof(int), hipMemcpyHostToDevice));
    return 0;
}
extern "C" int sva_batch_uses_persistent_decode(sva_batch* b) { return b && !b->edits_on ? (b->use_mega ? 1 : b->use_abatch ? 2 : 0) : 0; }

// previous_tokens / repetition_penalty / suppress_tokens of decode_one_token_ar (modules/dual_ar_stream.py:1099-1117, 1175-1213)
extern "C" int sva_set_sampler_edits(sva_batch* b, const int32_t* previous_tokens, int W, float repetition_penalty, const int32_t* suppress_tokens,
                                     int n_suppress) {
    SVA_CHECK(b, "sva_set_sampler_edits: null batch");
    SVA_CHECK(W >= 0 && W <= EDIT_CAP && n_suppress >= 0 && n_suppress <= EDIT_CAP, "sva_set_sampler_edits: at most 4096 previous tokens per head / suppressed tokens");
    SVA_CHECK((W == 0 || previous_tokens) && (n_suppress == 0 || suppress_tokens), "sva_set_sampler_edits: null list");
    SVA_CHECK(repetition_penalty > 0.f, "sva_set_sampler_edits: repetition_penalty must be positive");
    SVA_HIP(hipSetDevice(b->e->device));
    SVA_TRY(quiesce(b));
    SVA_HIP(hipStreamSynchronize(b->stream));
    const int heads = 1 + b->e->cfg.num_codebooks;
    const bool on = W > 0 || n_suppress > 0;
    if (on && !b->d_edit_prev) {
        SVA_TRY(dev_alloc(b->allocs, &b->d_edit_prev, (size_t)heads * EDIT_CAP));
        SVA_TRY(dev_alloc(b->allocs, &b->d_edit_suppress, (size_t)EDIT_CAP));
        SVA_TRY(dev_alloc(b->allocs, &b->d_edit_params, (size_t)heads * 4));
    }
    if (on) {
        for (int h = 0; h < heads && W > 0; ++h)
            SVA_HIP(hipMemcpy(b->d_edit_prev + (size_t)h * EDIT_CAP, previous_tokens + (size_t)h * W, sizeof(int) * (size_t)W, hipMemcpyHostToDevice));
        if (n_suppress) SVA_HIP(hipMemcpy(b->d_edit_suppress, suppress_tokens, sizeof(int) * (size_t)n_suppress, hipMemcpyHostToDevice));
        std::vector<int> prm((size_t)heads * 4, 0);
        int pbits;
        memcpy(&pbits, &repetition_penalty, 4);
        for (int h = 0; h < heads; ++h) { prm[h * 4] = W; prm[h * 4 + 1] = h == 0 ? n_suppress : 0; prm[h * 4 + 2] = pbits; }     // the list goes to the token head only (:1189)
        SVA_HIP(hipMemcpy(b->d_edit_params, prm.data(), sizeof(int) * prm.size(), hipMemcpyHostToDevice));
    }
    if (on != b->edits_on) {
        // the AR stage's captured launches change (edit kernels in / out, persistent kernel out / in): drop its graphs
        for (auto& ge : b->pipe_graph_a) if (ge) { (void)hipGraphExecDestroy(ge); ge = nullptr; }
        if (b->graph_exec) { (void)hipGraphExecDestroy(b->graph_exec); b->graph_exec = nullptr; }
        b->edits_on = on;
    }
    return 0;
}

extern "C" int sva_sync(sva_batch* b) {
    SVA_CHECK(b, "null batch");
    SVA_HIP(hipSetDevice(b->e->device));
    (void)hipGetLastError();
    SVA_TRY(quiesce(b));
    SVA_HIP(hipStreamSynchronize(b->stream));
    SVA_TRY(check_ar_fail(b));
    SVA_TRY(conv_gemm_check_errors());
    SVA_TRY(check_mm_overflow(b));
    float t;
    if (!b->graph_step)
        for (int i = 0; i < 3; ++i)
            if (hipEventElapsedTime(&t, b->ev[i], b->ev[i + 1]) == hipSuccess) b->last_ms[i] = t;
    if (hipEventElapsedTime(&t, b->ev[0], b->ev[3]) == hipSuccess) b->last_ms[3] = t;
    return 0;
}

// ---- AR seams: DualARWrapper.prefill_src_condition4delay / decode_one driven with caller-supplied content codes ----
extern "C" int sva_ar_delay_fill(sva_batch* b, const int64_t* codes) {
    SVA_CHECK(b && codes && b->begun, "sva_ar_delay_fill: bad argument");
    // the 2 * delay - 1 rows land on last_pos + 1 ..: refused before anything is uploaded or launched (the positions are the book's mirror)
    for (int i = 0; i < b->B; ++i)
        SVA_CHECK(b->slots.s[i].last_pos + 2 * b->p.delay - 1 < b->e->cfg.max_seq_len, "sva_ar_delay_fill: a slot's delay rows would run past the KV cache (max_seq_len)");
    SVA_HIP(hipSetDevice(b->e->device));
    (void)hipGetLastError();
    SVA_TRY(quiesce(b));
    const int B = b->B, d = b->p.delay;
    long long* tmp = (long long*)b->d_noise;       // scratch (>= B*d*8 bytes)
    SVA_TRY(h2d(b, tmp, codes, sizeof(int64_t) * (size_t)B * d));
    SVA_TRY(launch_put_codes(tmp, d, b->d_codes, b->T2, b->d_content_hist, b->hist_cap, b->d_ncontent, B, b->stream));
    b->slots.add_content(d);
    SVA_TRY(ar_delay_fill(b));
    b->slots.lockstep_filled();
    SVA_HIP(hipStreamSynchronize(b->stream));
    return 0;
}

extern "C" int sva_ar_decode_one(sva_batch* b, const int64_t* code, const float* noise, const int32_t* forced, int32_t* codes_out, int32_t* pos_out) {
    SVA_CHECK(b && code && codes_out && b->begun && b->slots.delay_filled, "sva_ar_decode_one: bad argument / delay not filled");
    SVA_CHECK(b->p.chunk_frames == 1, "sva_ar_decode_one needs chunk_frames == 1");
    // a frame writes the rows last_pos + 1, last_pos + 2 of every slot: refused before anything is uploaded or launched, the batch stays as it was
    // (sva_generate / sva_generate_many check the same bound on their whole run)
    for (int i = 0; i < b->B; ++i)
        SVA_CHECK(b->slots.s[i].last_pos + 2 < b->e->cfg.max_seq_len, "sva_ar_decode_one: a slot's frame would run past the KV cache (max_seq_len): re-prefill it first");
    SVA_HIP(hipSetDevice(b->e->device));
    (void)hipGetLastError();
    SVA_TRY(quiesce(b));
    const sva_config& c = b->e->cfg;
    const int B = b->B, ncb = c.num_codebooks;
    hipStream_t st = b->stream;
    long long* tmp = (long long*)b->d_tok_raw;     // scratch: B*8 ints >= B int64
    SVA_TRY(h2d(b, tmp, code, sizeof(int64_t) * (size_t)B));
    SVA_TRY(launch_put_codes(tmp, 1, b->d_codes, b->T2, b->d_content_hist, b->hist_cap, b->d_ncontent, B, st));
    b->slots.add_content(1);
    b->noise_on_device = (noise == nullptr);
    if (noise) SVA_TRY(h2d(b, b->d_noise, noise, sizeof(float) * (size_t)B * (c.ar_vocab + ncb * c.codebook_size)));
    const int uf = forced ? 1 : 0;
    SVA_TRY(h2d(b, b->d_use_forced, &uf, sizeof(int)));
    b->h_use_forced = uf;
    if (forced) SVA_TRY(h2d(b, b->d_forced, forced, sizeof(int) * (size_t)B * ncb));
    SVA_TRY(ar_decode_frame(b, 0, b->d_codes, b->T2, b->T2 - 1));
    for (int i = 0; i < B; ++i) b->slots.frame_decoded(i, 2);
    SVA_HIP(hipMemcpyAsync(codes_out, b->d_step_audio, sizeof(int) * (size_t)B * ncb, hipMemcpyDeviceToHost, st));
    if (pos_out) SVA_HIP(hipMemcpyAsync(pos_out, b->d_last_pos, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
    SVA_HIP(hipStreamSynchronize(st));
    return 0;
}

// ---- offline ARVCWrapper.generate (modules/arvc_wrapper.py:82-98 + DualARWrapper.generate, dual_ar_stream.py:698-762) for every slot of the
// batch at once: utterance i in slot i, one utterance per slot (the entries below check that and their own pointers).  The prompts run as
// packed passes over the rows of several slots, the frames through the batch's normal decode choice, finished slots ride along parked ----
static int offline_generate(sva_batch* b, const int64_t* const* ref_cc, const int32_t* const* ref_ac, const int* R, const int64_t* const* src_cc,
                            const int* S, const float* style, const float* timbre, const uint64_t* noise_seed, const float* noise,
                            int32_t* const* codes_out) {
    sva_engine* e = b->e;
    const sva_config& c = e->cfg;
    const int B = b->B, D = c.ar_dim, d = b->p.delay, ncb = c.num_codebooks, nspk = c.timbre_tokens + 1;
    std::vector<int> Mi(B);
    int Smax = 0;
    for (int i = 0; i < B; ++i) {
        SVA_CHECK(S[i] > d, "offline generate: source length must exceed the delay");
        // (a slot parks in ring column S[i] only while a longer one still runs: S[i] < Smax <= hist_cap, so that column exists)
        SVA_CHECK(S[i] <= b->hist_cap, "offline generate: source longer than the prediction history");
        Mi[i] = nspk + 2 * (R[i] + d) + 1;
        SVA_CHECK(Mi[i] <= b->Mmax && R[i] + d <= b->Pmax, "offline generate: prompt longer than the AR scratch");
        SVA_CHECK(Mi[i] + 2 * (S[i] - 1) <= c.max_seq_len, "offline generate: prompt + source exceed the 2048-position KV cache (the reference breaks there too)");
        Smax = std::max(Smax, S[i]);
    }
    std::vector<int> pass_of, row0_of;
    const int n_pass = prefill_pack(Mi.data(), B, b->Mmax, pass_of, row0_of);
    SVA_CHECK(n_pass >= 1, "offline generate: prompt longer than the AR scratch");
    SVA_HIP(hipSetDevice(e->device));
    (void)hipGetLastError();
    SVA_TRY(quiesce(b));
    hipStream_t st = b->stream;

    // remaining_cond of every slot = [src_cond[d:], wait4end[:d]] (wait4end_j addressed as vocab + j), padded with a valid row
    std::vector<long long> rem((size_t)B * Smax, 0);
    for (int i = 0; i < B; ++i)
        for (int f = 0; f < S[i]; ++f) rem[(size_t)i * Smax + f] = f < S[i] - d ? (long long)src_cc[i][d + f] : (long long)c.ar_vocab + (f - (S[i] - d));
    // slots in the order they finish; the gather index of each slot's last prompt row inside its pass
    std::vector<int> order(B), last_row(B), lp(B);
    for (int i = 0; i < B; ++i) { order[i] = i; last_row[i] = row0_of[i] + Mi[i] - 1; lp[i] = Mi[i] - 1; }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return S[x] < S[y]; });
    // one device block for the call: run + tile tables (16-byte rows first) | rem | staging rows | order | last_row
    PrefillTiles tt;
    tt.max_runs = (size_t)B; tt.max_tiles = (size_t)b->Mmax / 16 + (size_t)B;
    const size_t tab_bytes = sizeof(int) * (4 * tt.max_runs + 2 * tt.max_tiles), rem_bytes = sizeof(long long) * rem.size();
    const size_t stage_bytes = sizeof(float) * (size_t)B * D;
    struct DevGuard { char* p = nullptr; ~DevGuard() { if (p) (void)hipFree(p); } } guard;      // freed on every return path
    SVA_HIP(hipMalloc((void**)&guard.p, tab_bytes + rem_bytes + stage_bytes + sizeof(int) * 2 * B));
    tt.dev = (int*)guard.p;
    long long* d_rem = (long long*)(guard.p + tab_bytes);
    float* d_stage = (float*)(guard.p + tab_bytes + rem_bytes);
    int* d_order = (int*)(guard.p + tab_bytes + rem_bytes + stage_bytes);
    int* d_last_row = d_order + B;
    SVA_HIP(hipMemcpyAsync(d_rem, rem.data(), rem_bytes, hipMemcpyHostToDevice, st));
    SVA_HIP(hipMemcpyAsync(d_order, order.data(), sizeof(int) * B, hipMemcpyHostToDevice, st));
    SVA_HIP(hipMemcpyAsync(d_last_row, last_row.data(), sizeof(int) * B, hipMemcpyHostToDevice, st));
    SVA_HIP(hipMemcpyAsync(b->d_style, style, sizeof(float) * (size_t)B * c.style_dim, hipMemcpyHostToDevice, st));
    SVA_HIP(hipMemcpyAsync(b->d_timbre, timbre, sizeof(float) * (size_t)B * c.timbre_tokens * c.timbre_dim, hipMemcpyHostToDevice, st));
    SVA_HIP(hipMemcpyAsync(b->d_seed, noise_seed, sizeof(unsigned long long) * (size_t)B, hipMemcpyHostToDevice, st));
    SVA_HIP(hipMemcpyAsync(b->d_last_pos, lp.data(), sizeof(int) * B, hipMemcpyHostToDevice, st));
    SVA_HIP(hipMemsetAsync(b->d_nframes, 0, sizeof(int) * B, st));
    SVA_HIP(hipStreamSynchronize(st));

    // the prompts: as many whole slots per pass as fit Mmax rows, one ar_layers_pass per pack, the last prompt row of each slot gathered for frame 0
    std::vector<int> hs(b->Mmax), hp(b->Mmax), runs;
    for (int i0 = 0; i0 < B;) {
        int i1 = i0, rows = 0;
        runs.clear();
        for (; i1 < B && pass_of[i1] == pass_of[i0]; ++i1) {
            const int i = i1, Rp = R[i] + d, M = Mi[i], row0 = row0_of[i];
            // prefill_cond = [ref_cond, src_cond[:d]] interleaved with [wait4start[:d], embed(ref_audio)]  (dual_ar_stream.py:711-715)
            std::vector<int64_t> cc(ref_cc[i], ref_cc[i] + R[i]);
            for (int k = 0; k < d; ++k) cc.push_back(src_cc[i][k]);
            std::vector<int32_t> ac((size_t)ncb * Rp, 0);
            for (int q = 0; q < ncb; ++q)
                for (int k = 0; k < R[i]; ++k) ac[(size_t)q * Rp + k] = ref_ac[i][(size_t)q * R[i] + k];
            SVA_TRY(stage_prompt(b, cc, ac, Rp));
            // speaker prefix + prompt rows, then remaining_cond[0] as the last row
            SVA_TRY(ar_build_prompt_rows(b, i, Rp, b->ax + (long)row0 * D, M - 1));
            SVA_TRY(launch_put_row(e->content_emb, rem[(size_t)i * Smax], D, b->ax + (long)(row0 + M - 1) * D, st));
            for (int m = 0; m < M; ++m) { hs[row0 + m] = i; hp[row0 + m] = m; }
            runs.insert(runs.end(), {i, 0, M, row0});
            rows = row0 + M;
        }
        SVA_HIP(hipMemcpyAsync(b->d_slot, hs.data(), sizeof(int) * rows, hipMemcpyHostToDevice, st));
        SVA_HIP(hipMemcpyAsync(b->d_pos, hp.data(), sizeof(int) * rows, hipMemcpyHostToDevice, st));
        SVA_HIP(hipStreamSynchronize(st));            // (hs / hp are rewritten by the next pass)
        const PassRuns pr{runs.data(), (int)runs.size() / 4, &tt};
        SVA_TRY(ar_layers_pass(b, e->ar_layers, rows, b->d_slot, b->d_pos, e->rope_ar, (float*)b->kv_slow, b->kv_slow_layer, b->kv_slow_slot, c.max_seq_len,
                               b->ax, -1, 0, &pr));
        SVA_TRY(launch_gather_rows(b->ax, d_last_row + i0, 1, 0, i1 - i0, D, d_stage + (long)i0 * D, D, st));
        SVA_HIP(hipStreamSynchronize(st));            // the pass is done: its tile table's host copy may go, b->ax may be rebuilt
        tt.host.clear();
        i0 = i1;
    }
    for (int i = 0; i < B; ++i) b->slots.offline_prefilled(i, lp[i]);
    SVA_HIP(hipMemcpyAsync(b->ax, d_stage, stage_bytes, hipMemcpyDeviceToDevice, st));

    const int nstride = c.ar_vocab + ncb * c.codebook_size;
    const int zero = 0;
    SVA_TRY(h2d(b, b->d_use_forced, &zero, sizeof(int)));
    b->h_use_forced = 0;
    b->noise_on_device = (noise == nullptr);
    {   // frame 0 sits on the prefill's last row.  The prefill's decode ignores the caller's sampling settings (dual_ar_stream.py:722): temperature = top_p = 0.7,
        // no previous_tokens / suppress_tokens -- written into every slot's device pair for this one frame; the slots' own pairs come back from the book
        if (noise) SVA_TRY(h2d(b, b->d_noise, noise, sizeof(float) * (size_t)B * nstride));
        std::vector<float> pairs((size_t)2 * B);
        for (int i = 0; i < B; ++i) { pairs[2 * i] = 1.0f / 0.7f; pairs[2 * i + 1] = 0.7f; }
        SVA_TRY(h2d(b, b->d_samp, pairs.data(), sizeof(float) * pairs.size()));
        b->edits_skip = true;
        const int rc0 = ar_frame_tail(b, 0, (long)D, 0, d_rem, Smax, 0, 0);
        b->edits_skip = false;
        for (int i = 0; i < B; ++i) { pairs[2 * i] = b->slots.s[i].samp[0]; pairs[2 * i + 1] = b->slots.s[i].samp[1]; }
        const int rc1 = h2d(b, b->d_samp, pairs.data(), sizeof(float) * pairs.size());
        SVA_TRY(rc0);
        SVA_TRY(rc1);
        for (int i = 0; i < B; ++i) b->slots.frame_decoded(i, 0);
    }
    // frames 1 .. Smax - 1 of every slot: tokens [embed(previous codes), rem[f]] at the next two positions (dual_ar_stream.py:735-760).  A slot that
    // has produced its S[i] frames rides along parked: when it finishes, and after every throw-away frame, its position goes back by 2, so the
    // frame rewrites the two KV positions of the slot's own last frame (never a position past the cache); after a throw-away frame its frame
    // counter goes back by 1, so its codes land in ring column S[i], the spare one.  No launch while nobody has finished.
    int n_done = 0;                                   // slots order[0 .. n_done) have finished before frame f
    for (int f = 1; f < Smax; ++f) {
        if (noise) SVA_TRY(h2d(b, b->d_noise, noise + (size_t)f * B * nstride, sizeof(float) * (size_t)B * nstride));
        SVA_TRY(ar_decode_frame(b, 0, d_rem, Smax, f));
        for (int i = 0; i < B; ++i) b->slots.frame_decoded(i, 2);
        int n_now = n_done;
        while (n_now < B && S[order[n_now]] <= f + 1) ++n_now;
        if (f + 1 < Smax && n_now > 0) {
            SVA_TRY(launch_add_list(b->d_last_pos, d_order, n_now, -2, st));
            if (n_done > 0) SVA_TRY(launch_add_list(b->d_nframes, d_order, n_done, -1, st));
            for (int k = 0; k < n_now; ++k) b->slots.offline_parked(order[k], 2, k < n_done ? 1 : 0);
        }
        n_done = n_now;
    }
    SVA_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < B; ++i)
        for (int q = 0; q < ncb; ++q)
            SVA_HIP(hipMemcpy(codes_out[i] + (size_t)q * S[i], b->d_pred_hist + ((size_t)i * ncb + q) * b->hist_cap, sizeof(int) * (size_t)S[i], hipMemcpyDeviceToHost));
    return 0;
}

// one utterance on a one-stream batch: the n = 1 call of offline_generate
extern "C" int sva_generate(sva_batch* b, const int64_t* ref_cc, const int32_t* ref_ac, int R, const int64_t* src_cc, int S,
                            const float* style, const float* timbre, uint64_t noise_seed, const float* noise, int32_t* codes_out) {
    SVA_CHECK(b && ref_cc && ref_ac && src_cc && style && timbre && codes_out, "sva_generate: null argument");
    SVA_CHECK(b->B == 1 && b->p.chunk_frames == 1, "sva_generate: the offline path is batch 1 / chunk 1 like the reference");
    return offline_generate(b, &ref_cc, &ref_ac, &R, &src_cc, &S, style, timbre, &noise_seed, noise, &codes_out);
}

extern "C" int sva_generate_many(sva_batch* b, int n, const int64_t* const* ref_cc, const int32_t* const* ref_ac, const int* R,
                                 const int64_t* const* src_cc, const int* S, const float* style, const float* timbre,
                                 const uint64_t* noise_seed, const float* noise, int32_t* const* codes_out) {
    SVA_CHECK(b && ref_cc && ref_ac && R && src_cc && S && style && timbre && noise_seed && codes_out, "sva_generate_many: null argument");
    SVA_CHECK(b->p.chunk_frames == 1 && n == b->B, "sva_generate_many: needs chunk_frames == 1 and one utterance per slot (n == n_streams)");
    for (int i = 0; i < n; ++i) {
        SVA_CHECK(ref_cc[i] && ref_ac[i] && src_cc[i] && codes_out[i], "sva_generate_many: null argument");
        SVA_CHECK(R[i] >= 1, "sva_generate_many: empty prompt");
    }
    return offline_generate(b, ref_cc, ref_ac, R, src_cc, S, style, timbre, noise_seed, noise, codes_out);
}

extern "C" int sva_encode_window(sva_batch* b, const float* audio, int64_t* codes_out, float* u_out) {
    SVA_CHECK(b && audio && codes_out, "null argument");
    SVA_HIP(hipSetDevice(b->e->device));
    (void)hipGetLastError();
    SVA_TRY(quiesce(b));
    hipStream_t st = b->stream;
    SVA_HIP(hipMemcpyAsync(b->ring, audio, sizeof(float) * (size_t)b->B * b->N, hipMemcpyHostToDevice, st));
    b->gemm_flops = 0; b->gemm_launches = 0; b->gemm_bytes = 0;
    SVA_HIP(hipEventRecord(b->ev[0], st));
    SVA_TRY(encode(b, nullptr, 0, 0));
    SVA_HIP(hipEventRecord(b->ev[1], st));
    SVA_HIP(hipMemcpyAsync(codes_out, b->d_codes, sizeof(int64_t) * (size_t)b->B * b->T2, hipMemcpyDeviceToHost, st));
    if (u_out) SVA_HIP(hipMemcpyAsync(u_out, b->d_u, sizeof(float) * (size_t)b->B * b->T2 * b->e->cfg.bsq_bits, hipMemcpyDeviceToHost, st));
    SVA_HIP(hipStreamSynchronize(st));
    float t;
    if (hipEventElapsedTime(&t, b->ev[0], b->ev[1]) == hipSuccess) b->last_ms[0] = t;
    return 0;
}

// wav2target_fn (evaluations/infer_arvc.py:168-171) -> FireflyArchitecture.encode (firefly.py:560-574) on full windows:
// log-mel -> voc.backbone -> quantizer.downsample -> grouped FSQ indices.  Same front-end kernels as the content encoder
// with the vocoder's weight set; the window buffers are shared, so this does not interleave with a running stream.
extern "C" int sva_firefly_encode(sva_batch* b, const float* audio, int32_t* codes_out) {
    SVA_CHECK(b && audio && codes_out, "null argument");
    sva_engine* e = b->e;
    SVA_CHECK(e->vocf.loaded, "firefly.encode weights (voc.backbone.*, voc.quantizer.downsample.*, ...project_in) were not loaded");
    SVA_HIP(hipSetDevice(e->device));
    (void)hipGetLastError();
    SVA_TRY(quiesce(b));
    hipStream_t st = b->stream;
    const sva_config& c = e->cfg;
    SVA_HIP(hipMemcpyAsync(b->ring, audio, sizeof(float) * (size_t)b->B * b->N, hipMemcpyHostToDevice, st));
    b->gemm_flops = 0; b->gemm_launches = 0; b->gemm_bytes = 0;
    SVA_HIP(hipEventRecord(b->ev[0], st));
    SVA_TRY(enc_frontend_window(b, nullptr, 0, 0, b->T0, &e->vocf));
    SVA_TRY(launch_fsq_encode(b->d2.p, b->d2.bstride, (long)b->d2.H * c.voc_dim, c.voc_dim, b->B, b->T2, c.num_codebooks,
                              c.voc_dim / c.num_codebooks, e->fsq_in_W, e->fsq_in_b, b->d_fsq_codes, (long)c.num_codebooks * b->T2,
                              b->T2, st));
    SVA_HIP(hipEventRecord(b->ev[1], st));
    SVA_HIP(hipMemcpyAsync(codes_out, b->d_fsq_codes, sizeof(int32_t) * (size_t)b->B * c.num_codebooks * b->T2, hipMemcpyDeviceToHost, st));
    SVA_HIP(hipStreamSynchronize(st));
    float t;
    if (hipEventElapsedTime(&t, b->ev[0], b->ev[1]) == hipSuccess) b->last_ms[0] = t;
    return 0;
}

extern "C" long sva_get_tap(sva_batch* b, const char* what, void* out, long out_bytes) {
    if (!b || !what || !out) { set_error("null argument"); return -1; }
    hipSetDevice(b->e->device);
    if (quiesce(b)) return -2;            // pipelined mode: join the stage streams first
    const sva_config& c = b->e->cfg;
    const std::string w(what);
    const void* src = nullptr;
    long bytes = 0;
    const int B = b->B, chunk = b->p.chunk_frames;
    if (w == "content_codes") { src = b->d_step_content; bytes = sizeof(int) * (long)B * chunk; }
    else if (w == "audio_codes") { src = b->d_step_audio; bytes = sizeof(int) * (long)B * c.num_codebooks * chunk; }
    else if (w == "sampled_codes") { src = b->d_tok_raw; bytes = sizeof(int) * (long)B * c.num_codebooks; }
    else if (w == "slow_logits") { src = b->slow_logits; bytes = sizeof(float) * (long)B * c.ar_vocab; }
    else if (w == "fast_logits") { src = b->fast_logits; bytes = sizeof(float) * (long)B * c.num_codebooks * c.codebook_size; }
    else if (w == "hidden") { src = b->hidden; bytes = sizeof(float) * (long)B * c.ar_dim; }
    else if (w == "semantic") { src = b->d_sem; bytes = sizeof(int) * (long)B; }
    else if (w == "last_pos") { src = b->d_last_pos; bytes = sizeof(int) * (long)B; }
    else if (w == "cached_audio_emb") { src = b->cached_audio_emb; bytes = sizeof(float) * (long)B * c.ar_dim; }
    else if (w == "window_codes") { src = b->d_codes; bytes = sizeof(long long) * (long)B * b->T2; }
    else if (w == "u") { src = b->d_u; bytes = sizeof(float) * (long)B * b->T2 * c.bsq_bits; }
    else if (w == "mel") { src = b->mel.p; bytes = sizeof(float) * (long)B * b->mel.bstride; }
    else if (w == "feat") { src = b->feat.p; bytes = sizeof(float) * (long)B * b->feat.bstride; }
    else if (w == "mag") { src = b->mag; bytes = sizeof(float) * (long)B * b->T0 * 1088; }
    else if (w == "z") { src = b->tr_z; bytes = sizeof(float) * (long)B * b->T2 * c.tr_dim; }
    else if (w == "ar_fail") { src = b->d_ar_fail; bytes = b->d_ar_fail ? (long)sizeof(int) : 0; if (!src) { set_error("ar_fail: the persistent decode kernel is not in use"); return -1; } }
    else if (w == "ar_timing") { src = b->d_ar_dbg; bytes = b->d_ar_dbg ? 1024L * (long)sizeof(long long) : 0; if (!src) { set_error("ar_timing: set SVA_AR_TIMING=1"); return -1; } }
    else if (w == "voc_z") { src = b->voc.pin.p; bytes = sizeof(float) * (long)B * b->voc.pin.bstride; }
    else { set_error("unknown tap " + w); return -1; }
    if (out_bytes < bytes) { set_error("tap buffer too small"); return -1; }
    if (hipStreamSynchronize(b->stream) != hipSuccess || hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("tap copy failed");
        return -2;
    }
    return bytes;
}

extern "C" int sva_get_timings(sva_batch* b, float ms[4]) {
    SVA_CHECK(b && ms, "null argument");
    for (int i = 0; i < 4; ++i) ms[i] = b->last_ms[i];
    return 0;
}
extern "C" int sva_profile_gemm(sva_batch* b, int enable) {
    SVA_CHECK(b, "null batch");
    b->prof_on = enable != 0;
    b->prof_n = 0;
    if (enable) b->prof_shapes.clear();
    // per-launch durations are only meaningful when launches do not overlap: single stream while profiling
    static bool saved = true;
    if (enable) { saved = b->concurrency; b->concurrency = false; }
    else b->concurrency = saved;
    return 0;
}
extern "C" int sva_get_gemm_profile(sva_batch* b, double* total_ms, long* launches) {
    SVA_CHECK(b && total_ms && launches, "null argument");
    SVA_HIP(hipSetDevice(b->e->device));
    (void)hipGetLastError();
    SVA_TRY(quiesce(b));
    SVA_HIP(hipStreamSynchronize(b->stream));
    double tot = 0;
    for (int i = 0; i + 1 < b->prof_n; i += 2) {
        float t = 0;
        SVA_HIP(hipEventElapsedTime(&t, b->prof_ev[i], b->prof_ev[i + 1]));
        tot += t;
    }
    *total_ms = tot;
    *launches = b->prof_n / 2;
    return 0;
}
// per-launch table of the profiled steps: rows of (M, N, K, taps, mode, microseconds) as doubles; returns #rows
extern "C" long sva_get_gemm_profile_table(sva_batch* b, double* out, long max_rows) {
    if (!b || !out) return -1;
    hipSetDevice(b->e->device);
    hipStreamSynchronize(b->stream);
    long n = std::min<long>(max_rows, (long)b->prof_shapes.size());
    n = std::min<long>(n, b->prof_n / 2);
    for (long i = 0; i < n; ++i) {
        float t = 0;
        hipEventElapsedTime(&t, b->prof_ev[2 * i], b->prof_ev[2 * i + 1]);
        const auto& sh = b->prof_shapes[i];
        out[i * 6 + 0] = sh[0]; out[i * 6 + 1] = sh[1]; out[i * 6 + 2] = sh[2]; out[i * 6 + 3] = sh[3]; out[i * 6 + 4] = sh[4];
        out[i * 6 + 5] = t * 1e3;
    }
    return n;
}
extern "C" int sva_stream_codes(sva_batch* b, int slot, int n, int32_t* codes_out, long* n_frames_total) {
    SVA_CHECK(b && slot >= 0 && slot < b->B, "bad slot");
    const int nf = b->slots.s[slot].nframes, cap = b->hist_cap, ncb = b->e->cfg.num_codebooks;
    if (n_frames_total) *n_frames_total = nf;
    SVA_CHECK(n >= 0 && n <= nf && n <= cap, "more frames requested than the stream has decoded (or than the 4096-frame ring holds)");
    if (!n) return 0;
    SVA_CHECK(codes_out, "null argument");
    SVA_HIP(hipSetDevice(b->e->device));
    SVA_TRY(quiesce(b));
    SVA_HIP(hipStreamSynchronize(b->stream));
    std::vector<int> ring(cap);
    for (int q = 0; q < ncb; ++q) {
        SVA_HIP(hipMemcpy(ring.data(), b->d_pred_hist + ((long)slot * ncb + q) * cap, sizeof(int) * cap, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) codes_out[(size_t)q * n + i] = ring[(nf - n + i) & (cap - 1)];
    }
    return 0;
}
extern "C" int sva_get_gemm_bytes(sva_batch* b, double* bytes) {
    SVA_CHECK(b && bytes, "null argument");
    *bytes = b->gemm_bytes;
    return 0;
}
extern "C" int sva_get_gemm_stats(sva_batch* b, double* flops, long* launches) {
    SVA_CHECK(b && flops && launches, "null argument");
    *flops = b->gemm_flops;
    *launches = b->gemm_launches;
    return 0;
}

// ============================================================================================
// I/O adaptor (include/sva.h: sva_io_*): the plan is IoPlan's (io/io_plan.h), the two kernels are io/resample.hip's
// ============================================================================================
struct sva_io {
    sva_batch* b = nullptr;
    IoPlan plan;
    int fmt = 0;
    size_t esize = 4;                      // bytes of a caller sample
    ResampleDev din, dout;
    float* hist_in[2] = {nullptr, nullptr};      // [B][plan.hist_in], alternating per call
    float* hist_out[2] = {nullptr, nullptr};     // [B][plan.hist_out], alternating per step
    int par_in = 0, par_out = 0;
    float* stage = nullptr;                // [nbuf][B][2048c] chunk staging
    float* step_out = nullptr;             // [B][2048c] the step's PCM
    void* fifo = nullptr;                  // [B][fifo_cap] output FIFO (fmt)
    void *d_in = nullptr, *d_out = nullptr;      // [B][max_block] device copies of sva_io_process's host arrays
    bool failed = false;                   // a launch or a step failed behind the plan's counters: plan and device state have diverged
};

static int io_free(sva_io* io) {
    for (void* p : {(void*)io->hist_in[0], (void*)io->hist_in[1], (void*)io->hist_out[0], (void*)io->hist_out[1], (void*)io->stage, (void*)io->step_out,
                    io->fifo, io->d_in, io->d_out})
        if (p) (void)hipFree(p);
    resample_free(&io->din);
    resample_free(&io->dout);
    delete io;
    return 0;
}

extern "C" int sva_io_open(sva_batch* b, int io_rate, int fmt, int max_block, sva_io** out) {
    SVA_CHECK(b && out, "sva_io_open: null argument");
    SVA_CHECK(b->begun, "sva_io_open: the batch has not begun (sva_streams_begin)");
    SVA_CHECK(!b->io, "sva_io_open: this batch already has an adaptor (one per batch)");
    SVA_CHECK(fmt == kIoFmtF32 || fmt == kIoFmtI16, "sva_io_open: fmt is 0 (float32) or 1 (int16)");
    SVA_CHECK(max_block >= 1 && max_block <= (1 << 20), "sva_io_open: max_block outside 1 .. 2^20");
    SVA_CHECK(io_rate_supported(io_rate), std::string("sva_io_open: unsupported io_rate ") + std::to_string(io_rate) + ": " + kIoRateRule);
    SVA_TRY(drain_for_slot_call(b));
    sva_io* io = new sva_io();
    io->b = b; io->fmt = fmt; io->esize = fmt == kIoFmtI16 ? 2 : 4;
    if (!io->plan.open(io_rate, b->p.chunk_frames, max_block)) { delete io; SVA_CHECK(false, "sva_io_open: the planner refused this rate"); }
    const IoPlan& pl = io->plan;
    const size_t B = (size_t)b->B;
    auto zalloc = [&](void** p, size_t bytes) -> int {
        SVA_HIP(hipMalloc(p, bytes));
        SVA_HIP(hipMemset(*p, 0, bytes));
        return 0;
    };
    int rc = resample_upload(pl.in, &io->din);
    if (!rc) rc = resample_upload(pl.out, &io->dout);
    for (int k = 0; k < 2 && !rc; ++k) {
        rc = zalloc((void**)&io->hist_in[k], sizeof(float) * B * pl.hist_in);
        if (!rc) rc = zalloc((void**)&io->hist_out[k], sizeof(float) * B * pl.hist_out);
    }
    if (!rc) rc = zalloc((void**)&io->stage, sizeof(float) * B * pl.stage_cap);
    if (!rc) rc = zalloc((void**)&io->step_out, sizeof(float) * B * pl.chunk);
    if (!rc) rc = zalloc(&io->fifo, io->esize * B * pl.fifo_cap);              // (zeros: the L samples in front of the first output)
    if (!rc) rc = zalloc(&io->d_in, io->esize * B * max_block);
    if (!rc) rc = zalloc(&io->d_out, io->esize * B * max_block);
    if (rc) { io_free(io); return rc; }
    b->io = io;
    *out = io;
    return 0;
}

extern "C" void sva_io_close(sva_io* io) {
    if (!io) return;
    sva_batch* b = io->b;
    (void)hipSetDevice(b->e->device);
    (void)drain_for_slot_call(b);          // (the adaptor's kernels run on the batch's streams)
    b->io = nullptr;
    io_free(io);
}

// sva_stream_restart: what the slot received and produced so far counts as zeros
static int io_restart_slot(sva_io* io, int slot) {
    sva_batch* b = io->b;
    const IoPlan& pl = io->plan;
    hipStream_t st = b->stream;
    for (int k = 0; k < 2; ++k) {
        SVA_HIP(hipMemsetAsync(io->hist_in[k] + (size_t)slot * pl.hist_in, 0, sizeof(float) * pl.hist_in, st));
        SVA_HIP(hipMemsetAsync(io->hist_out[k] + (size_t)slot * pl.hist_out, 0, sizeof(float) * pl.hist_out, st));
    }
    for (int k = 0; k < pl.nbuf; ++k) SVA_HIP(hipMemsetAsync(io->stage + ((size_t)k * b->B + slot) * pl.chunk, 0, sizeof(float) * pl.chunk, st));
    SVA_HIP(hipStreamSynchronize(st));
    return 0;
}

// One call of the adaptor on device buffers.  ev_caller (may be null: the buffers are the adaptor's own, filled on the main stream): the main
// stream already waits for it, and so must the stream of the pop.  Runs behind the plan's counters: an error from here on leaves the adaptor failed.
static int io_run(sva_io* io, const void* d_in, void* d_out, int n, hipEvent_t ev_caller) {
    sva_batch* b = io->b;
    IoPlan& pl = io->plan;
    const int B = b->B, C = pl.chunk;
    hipStream_t se = b->main_stream;
    const long long n0 = pl.N, s0 = pl.S;
    const IoCall c = pl.push(n);
    {
        ResampleCall rc_;
        rc_.n0 = n0; rc_.j0 = c.m0; rc_.j1 = c.m1; rc_.n = n;
        rc_.hist_old = io->hist_in[io->par_in]; rc_.hist_new = io->hist_in[io->par_in ^ 1]; rc_.slot_flag = b->d_slot_flag;
        io->par_in ^= 1;
        SVA_TRY(launch_io_resample_in(io->din, rc_, B, d_in, io->fmt, io->stage, C, pl.nbuf, se));
    }
    for (int s_ = 0; s_ < c.steps; ++s_) {
        const long long k = s0 + s_;
        b->io_stepping = true;
        const int src = sva_step_device(b, io->stage + (size_t)(k % pl.nbuf) * B * C, io->step_out);
        b->io_stepping = false;
        if (src) return src;
        ResampleCall rc_;
        rc_.n0 = k * C; rc_.j0 = pl.out.ready(k * C); rc_.j1 = pl.out.ready((k + 1) * C); rc_.n = C;
        rc_.hist_old = io->hist_out[io->par_out]; rc_.hist_new = io->hist_out[io->par_out ^ 1];
        io->par_out ^= 1;
        // on the chain that holds the step's PCM: the next step's vocoder overwrites step_out behind this read
        SVA_TRY(launch_io_resample_out(io->dout, rc_, B, io->step_out, C, io->fifo, io->fmt, pl.fifo_cap, pl.L, b->out_stream ? b->out_stream : se));
    }
    // pop [n0, n0 + n) behind the last write of the FIFO
    hipStream_t so = b->out_stream ? b->out_stream : se;
    if (ev_caller && so != se) SVA_HIP(hipStreamWaitEvent(so, ev_caller, 0));
    const size_t es = io->esize;
    const int at = (int)(n0 % pl.fifo_cap), first = std::min(n, pl.fifo_cap - at);
    SVA_HIP(hipMemcpy2DAsync(d_out, es * n, (const char*)io->fifo + es * at, es * pl.fifo_cap, es * first, B, hipMemcpyDeviceToDevice, so));
    if (first < n)
        SVA_HIP(hipMemcpy2DAsync((char*)d_out + es * first, es * n, io->fifo, es * pl.fifo_cap, es * (n - first), B, hipMemcpyDeviceToDevice, so));
    return 0;
}
static int io_check_call(sva_io* io, const void* in, void* out, int n, const char* who) {
    SVA_CHECK(io && in && out, std::string(who) + ": null argument");
    SVA_CHECK(n >= 1 && n <= io->plan.max_block, std::string(who) + ": n outside 1 .. max_block");
    SVA_CHECK(!io->failed, std::string(who) + ": an earlier call of this adaptor failed after its counters had advanced; close it and open a new one");
    return 0;
}

extern "C" int sva_io_process_device(sva_io* io, const void* d_in, void* d_out, int n, void* caller_stream, int join_output) {
    SVA_TRY(io_check_call(io, d_in, d_out, n, "sva_io_process_device"));
    sva_batch* b = io->b;
    SVA_HIP(hipSetDevice(b->e->device));
    // everything already enqueued on the caller's stream (NULL is a stream too: the default one) happens before the engine's first access to
    // d_in and d_out, as in sva_step_device_on
    hipEvent_t ev_caller = next_event(b);
    SVA_HIP(hipEventRecord(ev_caller, (hipStream_t)caller_stream));
    SVA_HIP(hipStreamWaitEvent(b->main_stream, ev_caller, 0));
    io->failed = true;
    SVA_TRY(io_run(io, d_in, d_out, n, ev_caller));
    if (join_output) SVA_TRY(sva_join_stream(b, caller_stream));
    io->failed = false;
    return 0;
}

extern "C" int sva_io_process(sva_io* io, const void* pcm_in, void* pcm_out, int n, int* steps_run) {
    SVA_TRY(io_check_call(io, pcm_in, pcm_out, n, "sva_io_process"));
    sva_batch* b = io->b;
    SVA_HIP(hipSetDevice(b->e->device));
    (void)hipGetLastError();
    const size_t bytes = io->esize * (size_t)b->B * n;
    const long long s0 = io->plan.S;
    SVA_HIP(hipMemcpyAsync(io->d_in, pcm_in, bytes, hipMemcpyHostToDevice, b->main_stream));
    io->failed = true;
    SVA_TRY(io_run(io, io->d_in, io->d_out, n, nullptr));
    SVA_TRY(sva_sync(b));                  // (joins every chain into the main stream first)
    SVA_HIP(hipMemcpy(pcm_out, io->d_out, bytes, hipMemcpyDeviceToHost));
    io->failed = false;
    if (steps_run) *steps_run = (int)(io->plan.S - s0);
    return 0;
}

extern "C" int sva_io_latency(sva_io* io, int* total, int* filter_only) {
    SVA_CHECK(io, "sva_io_latency: null adaptor");
    if (total) *total = io->plan.L;
    if (filter_only) *filter_only = io->plan.L_filter;
    return 0;
}
