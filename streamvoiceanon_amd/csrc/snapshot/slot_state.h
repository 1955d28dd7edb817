// The whole per-slot state of a streaming batch, in one place: the ordered list of SEGMENTS that make up one slot (sva_stream_save /
// sva_stream_load; DESIGN.md 5d has the same inventory as a table).  Host-only: no kernels, no HIP calls -- slot_pack.hip moves the segments,
// engine.hip owns the calls.
//
// Derived from the code that writes per-slot state: sva_streams_begin / restart_encoder_state (ring, encoder histories, token cache, content
// count), prefill_slot_impl / ar_prefill_slot / ar_delay_fill / reprefill_slots (KV rows, speaker operands, cached embeddings, prompt tail,
// seed, position), ar_frame_tail and the persistent kernels (KV rows, cached_audio_emb, frame counter, prediction history),
// append_content_kernel (content history), alloc_vocoder's ShiftDesc table (the vocoder's history rows, in the form the level is in).
//
// NOT state, left out: everything a step writes before it reads it -- kv_fast / kv_fast_mega (the fast AR's 8 positions of one frame),
// the persistent kernels' granules and epochs, logits, hidden taps, d_tok / d_sem, d_step_content and the per-parity d_step_audio buffers
// (written by the AR stage, read by the same step's vocoder), feat / feat2 (the pipelined encoder's hand-over, written and read within a
// step), tr_x and every GEMM scratch.  d_codes is in the list although a step writes its newest rows before reading them: it is what the
// "content_codes" window of a slot shows between steps, and it is T2 words.  Both calls run on a drained batch, so "the current copy" of a
// double-buffered tensor is the one the batch's pointers name, and a load writes there: the next step swaps and overwrites as usual.
// Batch-wide and therefore not part of a slot: d_step (the ring origin: a ring segment is stored un-rotated), voc.d_frames, sampler edits,
// the I/O adaptor.
#pragma once
#include "../engine.h"
#include "../engine_internal.h"

#include <string>
#include <vector>

namespace sva {

enum SegKind : int {
    kSegPlain = 0,          // rows of row_bytes, row_stride apart
    kSegRing = 1,           // one row that is a ring: image byte j is ring byte (origin + j) mod row_bytes, origin = (*step * ring_step mod elements) * elem
    kSegKvPrefix = 2,       // rows 0 .. last_pos of one (layer, k / v, head) of the slow KV cache: the only kind whose row count varies
    kSegBlockedPlane = 3,   // history rows of one (plane, 32-k block) of a K-blocked operand plane, as its ShiftDesc lists them
};

// One segment of one slot, as slot_pack_kernel / slot_unpack_kernel read it from device memory.  The slot's first row is at
// base + slot * slot_stride; its image is rows * row_bytes bytes at img_off of the slot's image, padded with zeros to a multiple of 16.
struct SlotSegment {
    char* base;
    long slot_stride;       // bytes
    long row_stride;        // bytes
    long row_bytes;
    long img_off;           // bytes, a multiple of 16
    int rows;
    int kind;               // SegKind
    int elem;               // bytes of an element (2: fp16 KV rows, unsigned short planes; 4 otherwise): rows and strides are multiples of it.
                            // It is the granule of the element-wise arm, not a count: a plane's rows come from its ShiftDesc, which holds them in
                            // 4-byte units (C / 2 floats per row of C unsigned shorts), so such a row is always an even number of its elements.
    int ring_step;          // kSegRing: elements the ring's origin advances per step
};

inline long seg_payload(const SlotSegment& s) { return (long)s.rows * s.row_bytes; }
inline long seg_padded(const SlotSegment& s) { return (seg_payload(s) + 15) & ~15L; }

struct SlotSegments {
    std::vector<SlotSegment> seg;
    std::vector<std::string> name;
    long image_bytes = 0;
    void add(const std::string& nm, const void* base, long slot_stride, int rows, long row_bytes, long row_stride, int kind, int elem, int ring_step = 0) {
        SlotSegment s;
        s.base = const_cast<char*>(static_cast<const char*>(base));
        s.slot_stride = slot_stride; s.row_stride = row_stride; s.row_bytes = row_bytes; s.img_off = image_bytes;
        s.rows = rows; s.kind = kind; s.elem = elem; s.ring_step = ring_step;
        image_bytes += seg_padded(s);
        seg.push_back(s);
        name.push_back(nm);
    }
};

// The segments of one slot of `b` with `kv_rows` rows in every KV-prefix segment (last_pos + 1 of the stream to save, or of the blob to load).
inline int slot_segments(sva_batch* b, int kv_rows, SlotSegments* out) {
    const sva_config& c = b->e->cfg;
    const int D = c.ar_dim, ncb = c.num_codebooks, chunk = b->p.chunk_frames;
    SlotSegments& L = *out;
    L = SlotSegments();
    auto plain = [&](const std::string& nm, const void* base, long slot_elems, long n_elems, int elem) {
        L.add(nm, base, slot_elems * elem, 1, n_elems * elem, n_elems * elem, kSegPlain, elem);
    };
    // ---- encoder ----
    L.add("ring", b->ring, (long)b->N * 4, 1, (long)b->N * 4, (long)b->N * 4, kSegRing, 4, 2048 * chunk);
    if (b->enc_incremental) {
        const EncMerged& M = b->em;
        for (size_t i = 0; i < M.shift_host.size(); ++i) {
            const ShiftDesc& d = M.shift_host[i];
            L.add("enc_hist[" + std::to_string(i) + "]", d.ptr, d.bstride * 4, d.H, (long)d.C * 4, (long)d.C * 4, kSegPlain, 4);
        }
        L.add("d2c", b->d2c.p, b->d2c.bstride * 4, b->T2, (long)b->d2c.C * 4, (long)b->d2c.C * 4, kSegPlain, 4);
    }
    plain("d_codes", b->d_codes, b->T2 * 2L, b->T2 * 2L, 4);                      // int64 per token, moved as pairs of words
    plain("d_ncontent", b->d_ncontent, 1, 1, 4);
    plain("d_content_hist", b->d_content_hist, b->hist_cap, b->hist_cap, 4);
    // ---- AR ----
    {
        const int es = b->kv_half ? 2 : 4, H = c.ar_heads, S = c.max_seq_len;
        SVA_CHECK(kv_rows >= 0 && kv_rows <= S, "slot state: KV prefix longer than the cache");
        for (int l = 0; l < c.ar_layers; ++l)
            for (int k = 0; k < 2; ++k)
                for (int h = 0; h < H; ++h) {
                    const char* base = static_cast<const char*>(b->kv_slow) + ((long)l * b->kv_slow_layer + ((long)k * H + h) * S * 64) * es;
                    L.add("kv[" + std::to_string(l) + "][" + std::to_string(k) + "][" + std::to_string(h) + "]", base, b->kv_slow_slot * es, kv_rows, 64L * es,
                          64L * es, kSegKvPrefix, es);
                }
    }
    plain("cached_audio_emb", b->cached_audio_emb, D, D, 4);
    plain("cached_ref_emb", b->cached_ref_emb, (long)c.max_delay * D, (long)c.max_delay * D, 4);
    plain("d_ref_tail", b->d_ref_tail, (long)ncb * c.max_delay, (long)ncb * c.max_delay, 4);
    plain("d_style", b->d_style, c.style_dim, c.style_dim, 4);
    plain("d_timbre", b->d_timbre, (long)c.timbre_tokens * c.timbre_dim, (long)c.timbre_tokens * c.timbre_dim, 4);
    plain("d_last_pos", b->d_last_pos, 1, 1, 4);
    plain("d_nframes", b->d_nframes, 1, 1, 4);
    plain("d_seed", b->d_seed, 2, 2, 4);                                          // unsigned long long, moved as two words
    plain("d_samp", b->d_samp, 2, 2, 4);
    plain("d_pred_hist", b->d_pred_hist, (long)ncb * b->hist_cap, (long)ncb * b->hist_cap, 4);
    // ---- vocoder: the ShiftDesc table, entry by entry (alloc_vocoder builds it in the order of for_each_voc_state) ----
    VocWorkspace& v = b->voc;
    size_t di = 0;
    auto desc = [&](int kind, int elem) -> int {
        SVA_CHECK(di < v.shift_host.size(), "slot state: the vocoder's ShiftDesc table is shorter than its state walk");
        const ShiftDesc& d = v.shift_host[di];
        L.add("voc_hist[" + std::to_string(di) + "]", d.ptr, d.bstride * 4, d.H, (long)d.C * 4, (long)d.C * 4, kind, elem);
        ++di;
        return 0;
    };
    SVA_TRY(for_each_voc_state(v, [&](Act& a, unsigned short*& P, int, VocForm form) -> int {
        if (a.H == 0) return 0;
        if (!voc_form_planes(form)) return desc(kSegPlain, 4);
        (void)P;
        for (int p = 0; p < planes_count(v.pmode); ++p) {
            if (form == VocForm::PlanesHalo) { SVA_TRY(desc(kSegPlain, 2)); continue; }       // row-major plane
            for (int kb = 0; kb < a.C / 32; ++kb) SVA_TRY(desc(kSegBlockedPlane, 2));
        }
        return 0;
    }));
    SVA_CHECK(di == v.shift_host.size(), "slot state: the vocoder's ShiftDesc table is longer than its state walk");
    return 0;
}

// Layout signature: (rows, row bytes, kind) of every segment -- the KV prefix length left out -- then hist_cap, T2, the ring length, kv_half,
// every VocLevel::form and voc.pmode.  names (optional) receives one label per value, for the refusal message.
inline std::vector<int64_t> layout_signature(sva_batch* b, const SlotSegments& L, std::vector<std::string>* names = nullptr) {
    std::vector<int64_t> s;
    auto put = [&](const std::string& nm, int64_t v) { s.push_back(v); if (names) names->push_back(nm); };
    for (size_t i = 0; i < L.seg.size(); ++i) {
        const SlotSegment& g = L.seg[i];
        put(L.name[i] + ".rows", g.kind == kSegKvPrefix ? 0 : g.rows);
        put(L.name[i] + ".row_bytes", g.row_bytes);
        put(L.name[i] + ".kind", g.kind);
    }
    put("hist_cap", b->hist_cap); put("T2", b->T2); put("ring_length", b->N); put("kv_half", b->kv_half ? 1 : 0);
    for (size_t i = 0; i < sizeof(b->voc.lv) / sizeof(b->voc.lv[0]); ++i) put("voc_level_form[" + std::to_string(i) + "]", (int)b->voc.lv[i].form);
    put("voc_pmode", b->voc.pmode);
    return s;
}

// Configuration signature: every field of sva_config, then chunk_frames, delay, both windows, max_seq_frames, buffer_frames, max_prompt_frames.
inline std::vector<int64_t> config_signature(const sva_config& c, const sva_stream_params& p, std::vector<std::string>* names = nullptr) {
    std::vector<int64_t> s;
    auto put = [&](const char* nm, int64_t v) { s.push_back(v); if (names) names->push_back(nm); };
    put("n_mels", c.n_mels);
    for (int i = 0; i < 4; ++i) put("enc_depths", c.enc_depths[i]);
    for (int i = 0; i < 4; ++i) put("enc_dims", c.enc_dims[i]);
    put("tr_layers", c.tr_layers); put("tr_heads", c.tr_heads); put("tr_dim", c.tr_dim); put("tr_inter", c.tr_inter); put("bsq_bits", c.bsq_bits);
    put("ar_dim", c.ar_dim); put("ar_heads", c.ar_heads); put("ar_layers", c.ar_layers); put("ar_fast_layers", c.ar_fast_layers); put("ar_inter", c.ar_inter);
    put("ar_vocab", c.ar_vocab); put("codebook_size", c.codebook_size); put("num_codebooks", c.num_codebooks); put("max_delay", c.max_delay);
    put("max_seq_len", c.max_seq_len); put("timbre_dim", c.timbre_dim); put("timbre_tokens", c.timbre_tokens); put("style_dim", c.style_dim);
    put("voc_dim", c.voc_dim); put("ar_dtype", c.ar_dtype); put("mm_mode", c.mm_mode); put("voc_dtype", c.voc_dtype); put("enc_dtype", c.enc_dtype);
    static_assert(sizeof(sva_config) == 32 * sizeof(int), "a field was added to sva_config: add it to the configuration signature");
    put("chunk_frames", p.chunk_frames); put("delay", p.delay); put("encode_window_frames", p.encode_window_frames);
    put("decode_window_frames", p.decode_window_frames); put("max_seq_frames", p.max_seq_frames); put("buffer_frames", p.buffer_frames);
    put("max_prompt_frames", p.max_prompt_frames);
    return s;
}

}  // namespace sva
