// Host-side book of the deterministic per-slot stream state: phases, KV positions, frame and content counters, the stored prompt and the
// prompt of a pending restart.  Pure integer arithmetic on host mirrors -- no HIP, no sva_batch: engine.hip / stages.hip ask the book what
// is due, execute it on the device (launches, copies of d_last_pos / d_slot_flag ...) and tell the book what they did.  The rules are the
// reference's (evaluations/infer_arvc.py:443-596, modules/dual_ar_stream.py:764-837); tests/test_slot_book_cpu.py pins them without a GPU
// through sva_test_slot_book.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace sva {

// the prompt of a restart that has not been activated yet
struct PendingPrompt {
    std::vector<int64_t> cc;
    std::vector<int32_t> ac;
    std::vector<float> style, timbre;
    int R = 0;
    unsigned long long seed = 0;
};

enum SlotPhase { kSlotRetired = 0, kSlotDelayFilling = 1, kSlotDecoding = 2 };

struct SlotHost {
    int phase = kSlotDelayFilling;
    bool restarted = false;                // `pending` holds the prompt of a restart that has not been activated yet
    bool prefilled = false;
    int flag = 0;                          // host mirror of d_slot_flag[slot]
    int last_pos = -1;                     // last written slow-AR KV position
    int nframes = 0;                       // decoded frames (sampler noise counter)
    int ncontent = 0;                      // content codes seen (a restarted slot counts from its own start)
    int ref_len = 0;                       // frames of the stored prompt (truncated to max_prompt_frames)
    std::vector<int64_t> ref_content;      // [ref_len]      kept for re-prefill / vocoder priming
    std::vector<int32_t> ref_audio;        // [ncb][ref_len]
    PendingPrompt pending;
    float temperature = 0.7f;              // the slot's sampling pair as set (sva_stream_get_sampling) ...
    float samp[2] = {1.0f / 0.7f, 0.7f};   // ... and as the samplers read it: host mirror of d_samp[slot] = {inv_temp, top_p}
};

// what the end of a steady step asks of the device
struct StepPlan {
    std::vector<int> redo;                         // decoding slots due for a re-prefill (current_pos // 2 >= max_seq_frames, infer_arvc.py:547)
    std::vector<std::pair<int, int>> rewind;       // parked slots that would be due: (slot, position) to write into d_last_pos
};

// The slots that sva_streams_begin started together move delay filling -> decoding in lock step (`delay_filled`); a restarted slot carries
// its new prompt in `pending` while its own delay fills and is activated -- prefill, delay fill, vocoder priming, in the order a fresh stream
// sees them -- at the end of the step in which its content count reaches the delay.  A parked slot (retired, or filling its own delay) still
// rides through the AR launches and decodes throw-away frames; whenever it would become due for a re-prefill, and when it is restarted, its
// position goes back to where its last stored prompt ends: every K / V row up to there was written by that prompt's prefill.
struct SlotBook {
    std::vector<SlotHost> s;
    bool delay_filled = false;             // the lock-step slots hold `delay` content codes
    int h_step = 0;                        // chunks consumed since begin()
    float def_temperature = 0.7f, def_top_p = 0.7f;      // the batch's sampling pair (sva_stream_params): a restarted slot goes back to it

    // ---- positions (nspk = speaker prefix rows = timbre tokens + 1) ----
    static int prefill_end(int nspk, int R) { return nspk + 2 * R - 1; }                  // a prompt of R frames: rows 0 .. nspk + 2R - 1
    static int priming_frames_for(int Rt, int window, int chunk) { return (std::min(window - 1, Rt) / chunk) * chunk; }
    int parked_position(int slot, int nspk) const { return nspk - 1 + 2 * s[slot].ref_len; }
    // a re-prefill rebuilds [speaker prefix | 2 x (stored prompt + the last min(buffer_frames, nframes) frames)]
    int reprefill_frames(int slot, int buffer_frames) const { return std::min(buffer_frames, s[slot].nframes); }
    int reprefill_end(int slot, int nspk, int buffer_frames) const { return prefill_end(nspk, s[slot].ref_len + reprefill_frames(slot, buffer_frames)); }
    // vocoder frames a fresh stream is primed with: the last frames of its stored prompt, in whole chunks
    int priming_frames(int slot, int window, int chunk) const { return priming_frames_for(s[slot].ref_len, window, chunk); }
    // ... and those codes: frames [first, first + n) of the last P of `slot`'s stored prompt -> dst [ncb][n]
    void prompt_tail(int slot, int ncb, int P, int first, int n, int32_t* dst) const {
        const SlotHost& h = s[slot];
        const int R = h.ref_len;
        for (int q = 0; q < ncb; ++q)
            for (int k = 0; k < n; ++k) dst[(size_t)q * n + k] = h.ref_audio[(size_t)q * R + (R - P + first + k)];
    }

    // ---- sampling pair ----
    // temperature is clamped at 1e-5 like the batch value; inv_temp in float, the quotient every launcher used to form from the scalar
    void set_sampling(int slot, float temperature, float top_p) {
        SlotHost& h = s[slot];
        h.temperature = temperature;
        h.samp[0] = 1.0f / (temperature > 1e-5f ? temperature : 1e-5f);
        h.samp[1] = top_p;
    }
    void sampling_defaults(float temperature, float top_p) {
        def_temperature = temperature; def_top_p = top_p;
        for (size_t i = 0; i < s.size(); ++i) set_sampling((int)i, temperature, top_p);
    }

    // ---- batch life cycle ----
    void reset(int B) { s.assign((size_t)B, SlotHost()); delay_filled = false; h_step = 0; }
    void forget_prompts() { for (SlotHost& h : s) h.prefilled = false; }                 // (recovery from an AR failure: every slot needs a fresh prompt)
    bool all_prefilled() const { for (const SlotHost& h : s) if (!h.prefilled) return false; return true; }
    // sva_prefill_prompt / the activation of a restarted slot: a prompt of R frames, [ncb][R] audio codes; the stored copy keeps the first Rt frames
    void prefilled(int slot, int nspk, int R, int Rt, int ncb, const int64_t* cc, const int32_t* ac) {
        SlotHost& h = s[slot];
        h.ref_content.assign(cc, cc + Rt);
        h.ref_audio.resize((size_t)ncb * Rt);
        for (int q = 0; q < ncb; ++q)
            for (int i = 0; i < Rt; ++i) h.ref_audio[(size_t)q * Rt + i] = ac[(size_t)q * R + i];
        h.ref_len = Rt;
        h.last_pos = prefill_end(nspk, R);
        h.prefilled = true;
    }
    // sva_streams_begin: every slot starts in lock step, no restart pending, nothing muted
    void begin() {
        h_step = 0; delay_filled = false;
        for (SlotHost& h : s) { h.ncontent = 0; h.nframes = 0; h.phase = kSlotDelayFilling; h.restarted = false; h.flag = 0; }
    }

    // ---- steps ----
    void add_content(int n) { for (SlotHost& h : s) h.ncontent += n; }
    // a slot of the batch-wide start (they share one count), -1: every slot retired or restarted since begin()
    int lockstep_slot() const {
        for (size_t i = 0; i < s.size(); ++i)
            if (s[i].phase == kSlotDelayFilling && !s[i].restarted) return (int)i;
        return -1;
    }
    void lockstep_filled() {
        delay_filled = true;
        for (SlotHost& h : s)
            if (h.phase == kSlotDelayFilling && !h.restarted) h.phase = kSlotDecoding;
    }
    // a step before the delay is filled: true when the lock-step delay fill is due (over every slot of the batch: delay_filled_for), and
    // those slots then decode.  With nobody left to fill in lock step the batch is steady at once.
    bool warmup_step(int chunk, int delay) {
        h_step += 1;
        add_content(chunk);
        const int lock = lockstep_slot();
        if (lock >= 0 && s[lock].ncontent < delay) return false;
        lockstep_filled();
        return lock >= 0;
    }
    // prefill_src_condition4delay wrote 2 * delay - 1 rows for these slots
    void delay_filled_for(const std::vector<int>& slots, int delay) { for (int i : slots) s[i].last_pos += 2 * delay - 1; }
    // one decoded frame outside the chunk step (sva_ar_decode_one: pos_inc 2; the offline loop's first frame sits on the prefill's last row: 0)
    void frame_decoded(int slot, int pos_inc) { s[slot].last_pos += pos_inc; s[slot].nframes += 1; }
    void offline_prefilled(int slot, int last_pos) { s[slot].last_pos = last_pos; s[slot].nframes = 0; }
    // a finished slot of an offline batch rides along parked: its position is put back when it finishes and after every throw-away frame,
    // its frame counter after every throw-away frame (sva_generate_many)
    void offline_parked(int slot, int pos_back, int frames_back) { s[slot].last_pos -= pos_back; s[slot].nframes -= frames_back; }
    // a steady step decoded `chunk` frames for every slot (a parked slot's are thrown away).  Positions are deterministic, so the mirror decides
    // what is due without a device round trip; the rewinds are already applied to the mirror.
    StepPlan steady_step(int chunk, int max_seq_frames, int nspk) {
        StepPlan plan;
        h_step += 1;
        for (size_t i = 0; i < s.size(); ++i) {
            SlotHost& h = s[i];
            h.ncontent += chunk;
            h.last_pos += 2 * chunk;
            if (h.phase == kSlotDecoding) h.nframes += chunk;
            if (h.last_pos / 2 < max_seq_frames) continue;
            if (h.phase == kSlotDecoding) { plan.redo.push_back((int)i); continue; }
            h.last_pos = parked_position((int)i, nspk);
            plan.rewind.emplace_back((int)i, h.last_pos);
        }
        return plan;
    }
    // all due slots in one pass against the cached prompt prefix?  (a stream that has decoded fewer than `delay` frames -- a prompt about as
    // long as max_seq_frames -- keeps the general form, one whole-prompt prefill per slot; so does a stored prompt shorter than the delay: the
    // audio rows of its frames Rt .. delay - 1 are wait4start rows (prefill_prompt), which the one-pass row builder does not hold)
    bool one_pass_ok(const std::vector<int>& redo, int buffer_frames, int delay) const {
        for (int i : redo)
            if (reprefill_frames(i, buffer_frames) < delay || s[i].ref_len < delay) return false;
        return true;
    }
    void reprefilled(int slot, int last_pos) { s[slot].last_pos = last_pos; }

    // ---- restart / retire ----
    // restarted slots whose own content count has reached the delay
    std::vector<int> due_activations(int delay) const {
        std::vector<int> due;
        for (size_t i = 0; i < s.size(); ++i)
            if (s[i].restarted && s[i].phase == kSlotDelayFilling && s[i].ncontent >= delay) due.push_back((int)i);
        return due;
    }
    // parks the slot at the end of its last stored prompt with no content seen; `flag` mutes its output while its delay fills
    void restart(int slot, PendingPrompt&& prompt, int nspk, int flag) {
        SlotHost& h = s[slot];
        h.pending = std::move(prompt);
        h.restarted = true;
        h.phase = kSlotDelayFilling;
        h.ncontent = 0;
        h.last_pos = parked_position(slot, nspk);
        h.flag = flag;
        set_sampling(slot, def_temperature, def_top_p);      // like a slot of a fresh batch (the caller uploads the pair)
    }
    // (its position is rewound when it would become due for a re-prefill: steady_step)
    void retire(int slot, int flag) {
        SlotHost& h = s[slot];
        h.restarted = false;
        h.pending = PendingPrompt();
        h.phase = kSlotRetired;
        h.flag = flag;
    }
    // the pending prompt has been prefilled (prefilled) and delay-filled (delay_filled_for): a decoding stream with no frames yet, nothing muted
    void activated(int slot) {
        SlotHost& h = s[slot];
        h.nframes = 0;
        h.phase = kSlotDecoding;
        h.restarted = false;
        h.pending = PendingPrompt();
        h.flag = 0;
    }
    // sva_stream_load: whatever the slot held, it is now the decoding stream a snapshot describes -- its position, counters, stored prompt and
    // sampling pair (inv_temp as the source's samplers read it, not re-derived), no restart pending, nothing muted.  The lock-step state of the
    // batch is not touched (a load needs delay_filled).
    void adopt(int slot, int last_pos, int nframes, int ncontent, std::vector<int64_t>&& ref_content, std::vector<int32_t>&& ref_audio, float temperature,
               float inv_temp, float top_p) {
        SlotHost& h = s[slot];
        h.phase = kSlotDecoding;
        h.restarted = false;
        h.prefilled = true;
        h.pending = PendingPrompt();
        h.flag = 0;
        h.last_pos = last_pos; h.nframes = nframes; h.ncontent = ncontent;
        h.ref_len = (int)ref_content.size();
        h.ref_content = std::move(ref_content);
        h.ref_audio = std::move(ref_audio);
        h.temperature = temperature; h.samp[0] = inv_temp; h.samp[1] = top_p;
    }
    // decoded frames of a live stream (sva_stream_state)
    long stream_frames(int slot) const { return s[slot].phase == kSlotDecoding ? s[slot].nframes : 0; }
};

}  // namespace sva
