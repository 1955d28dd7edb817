/*
 * sva.h -- C ABI of the MI355X-native StreamVoiceAnon streaming voice-conversion engine.
 *
 * The reference (Plachtaa/StreamVoiceAnon) is pure Python and has no FFI of its own; this
 * header is the boundary a maintainer would bind (ctypes stub in INTEGRATION.md) to replace
 * the four per-chunk seams of evaluations/infer_arvc.py `process_one_chunk` (:492-596):
 *     speech_tokenizer.encode  (:506-508)   -> sva_encode_window / inside sva_step
 *     model.decode_one         (:535-537)   -> inside sva_step (sva_prefill_prompt for :484-489)
 *     firefly.quantizer.decode (:175)       -> sva_vocode_window / inside sva_step
 *     firefly.head             (:175)       -> sva_vocode_window / inside sva_step
 *
 * Conventions: every function returns 0 on success and a negative code on failure (message via
 * sva_last_error()); nothing throws across the ABI.  The caller owns all I/O buffers; the engine
 * owns weights and per-stream state.  Handles are not re-entrant (one host thread per handle).
 * All host pointers are plain C arrays; no torch / C++ types appear in any signature.
 */
#ifndef SVA_H
#define SVA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sva_engine sva_engine;
typedef struct sva_batch sva_batch;

/* Model dimensions.  sva_config_default() fills the values of the reference's Hydra YAMLs
 * (configs/hydra_arcs/{vc/firefly_arvc_bsq_8192_delay0_8, speech_tokenizers/causal-encoder-lfq-8192,
 * vocoders/firefly_gan_vq}.yaml). */
typedef struct sva_config {
    int n_mels;            /* 160 */
    int enc_depths[4];     /* 3,3,9,3 */
    int enc_dims[4];       /* 128,256,384,512 */
    int tr_layers;         /* 8   BSQ pre_module transformer */
    int tr_heads;          /* 8 */
    int tr_dim;            /* 512 */
    int tr_inter;          /* 1536 */
    int bsq_bits;          /* 13 */
    int ar_dim;            /* 768 */
    int ar_heads;          /* 12 */
    int ar_layers;         /* 12 */
    int ar_fast_layers;    /* 4 */
    int ar_inter;          /* 2304 */
    int ar_vocab;          /* 8192 */
    int codebook_size;     /* 1000 */
    int num_codebooks;     /* 8 */
    int max_delay;         /* 8 */
    int max_seq_len;       /* 2048 */
    int timbre_dim;        /* 128 */
    int timbre_tokens;     /* 32 */
    int style_dim;         /* 192 */
    int voc_dim;           /* 512 */
    int ar_dtype;          /* 0: fp32 AR weights + fp32 KV (parity mode); 1: fp16 AR weights (streamed as fp16 by the batch-1 decode kernel;
                            * the batched / prefill GEMMs use the same fp16-rounded values) + fp16 slow KV cache, as the reference
                            * decodes under torch.autocast(fp16) with fp16 caches (evaluations/infer_arvc.py:55-59, 483, 493) */
    int mm_mode;           /* fp32-grade batch-scale GEMMs (batches of 10+ streams) of the encoder / vocoder: 1 (default) = two pre-split fp16 planes per
                            * operand, three part products (csrc/gemm_planes.hip): half the matrix work of 0, for operands inside the fp16
                            * range -- which torch.autocast(fp16), infer_arvc.py:493, demands of the reference too; 0 = three bf16 parts split
                            * inside the K loop, six products (csrc/gemm_split.hip, the round-3 kernel): any fp32 range.  (2 -- three pre-split
                            * bf16 planes -- was an A/B arm of round 4, slower than 0, and is refused since round 5.)  NOTE: mode 1, the default,
                            * has fp16's RANGE: an operand beyond +-65504 raises an error at the next sva_step* / sva_sync naming mm_mode = 0 */
    int voc_dtype;         /* 0: vocoder (firefly.decode) GEMMs in the mm_mode grade; 1: fp16 operands, fp32 accumulate -- the reference's
                            * own precision for this stage (torch.autocast(fp16) around code2wav_fn, infer_arvc.py:493, 571-590) */
    int enc_dtype;         /* 0 (default): content encoder in fp32 grade, BSQ indices bit-equal to the fp32 oracle; 1: every groups = 1 conv / Linear of the
                            * tokenizer's content encoder takes both operands rounded once (nearest even) to fp16, exact products, fp32 accumulation; the A
                            * operand is the activation as its producer stores it (fp16(RMSNorm(x) w), ...); mel, depthwise convs, norms, attention, residuals and
                            * BSQ stay fp32.  NOT parity-preserving: a code bit may flip where its pre-sign value is near zero.  fp16 RANGE, reported as mm_mode's */
} sva_config;

/* evaluations/infer_arvc.py setup_stream_caches (:443-460) + stream_infer defaults (:598-613) */
typedef struct sva_stream_params {
    int n_streams;             /* B concurrent streams (the reference is hard-wired to 1) */
    int encode_window_frames;  /* 128 */
    int decode_window_frames;  /* 64  (used only to size vocoder priming = window - 1 frames) */
    int chunk_frames;          /* decode_chunk_frames, 1 */
    int delay;                 /* 2 */
    int max_seq_frames;        /* 768 */
    int buffer_frames;         /* 32 */
    int max_prompt_frames;     /* 256 */
    float temperature;         /* 0.7  (modules/dual_ar_stream.py:1103) */
    float top_p;               /* 0.7  (:1104) */
    int voc_max_frames;        /* largest T accepted by sva_vocode_window / one streaming call (>= chunk) */
    int use_graph;             /* capture the steady-state step in a hipGraph */
    int skip_semantic;         /* skip the semantic-token head whose sample every caller discards (:833) */
    int pipeline;              /* sva_step_device only: run encoder / AR / vocoder of consecutive chunk-steps on three streams
                                * (E(n+1) || A(n) || V(n-1)); same results, higher throughput for simulated streaming; a caller that
                                * synchronises per chunk sees the unpipelined latency */
    int slot_priming;          /* 0 (default): the step that activates a restarted slot primes its vocoder in a whole-batch run (below,
                                * sva_stream_restart).  1: slot-local activation -- the batch owns a one-stream vocoder workspace of
                                * ((decode_window_frames - 1) / chunk) * chunk code frames (allocated by sva_batch_create; measured
                                * at the default window: 624 / 766 / 1280 MiB of device memory beside a 2 / 8 / 64-stream batch); the slot's
                                * state is primed there in ONE pass over the prompt tail and moved into the slot.  Measured stall of the
                                * activating step: 5.0 / 5.1 / 4.1 ms at 2 / 8 / 64 streams against 38.5 / 61.8 / 100.3 ms with 0
                                * (profiles/slot_priming_report.txt).  Contract: codes, positions and frame
                                * counts of every slot are identical to slot_priming = 0; every OTHER slot is bit-identical; the restarted
                                * slot's PCM is within the vocoder tolerance of a fresh slot, not bit-identical to it (its state comes from a
                                * T = P pass instead of P / chunk chunk-sized passes: other GEMM tilings).  Inert until a restart. */
} sva_stream_params;

const char* sva_last_error(void);
int sva_config_default(sva_config* cfg);
int sva_stream_params_default(sva_stream_params* p);

/* ---- engine: weights ------------------------------------------------------------------ */
int sva_engine_create(const sva_config* cfg, int device, sva_engine** out);
/* name = reference state-dict key prefixed by its network: "arvc." (ARVCWrapper), "tok." (speech
 * tokenizer), "voc." (Firefly vocoder); data = fp32 host array of the given shape.  Unknown names
 * are ignored (strict=False, evaluations/infer_arvc.py:79-93,162).  Weight-norm pairs
 * (...parametrizations.weight.original0/1) are folded as g*v/||v|| (firefly.py:295-301). */
int sva_engine_load_weight(sva_engine* e, const char* name, int ndim, const int64_t* shape, const float* data);
/* pack to the compute layout and upload; after this the engine is immutable */
int sva_engine_finalize(sva_engine* e);
void sva_engine_destroy(sva_engine* e);

/* ---- batch of streams ------------------------------------------------------------------- */
int sva_batch_create(sva_engine* e, const sva_stream_params* p, sva_batch** out);
void sva_batch_destroy(sva_batch* b);

/* ARVCWrapper.prefill_prompt (modules/arvc_wrapper.py:100-112) + InferenceWrapper.prefill_prompt
 * bookkeeping (infer_arvc.py:463-489) for one stream slot: content codes int64[R], audio codes
 * int32[8][R] (row-major), style float[192], timbre float[32][128].  noise_seed keys the
 * on-device sampler noise of this utterance.  Call for every slot, then sva_streams_begin(). */
int sva_prefill_prompt(sva_batch* b, int slot, const int64_t* ref_content_codes, const int32_t* ref_audio_codes,
                       int R, const float* style, const float* timbre, uint64_t noise_seed);
/* zero the audio windows / histories and prime the streaming vocoder with the prompt tail */
int sva_streams_begin(sva_batch* b);

/* InferenceWrapper.process_one_chunk (infer_arvc.py:492-596) for all streams in lock step.
 *   pcm_in  host float[B][2048*chunk]      pcm_out host float[B][2048*chunk]
 *   noise   host float[B][chunk][vocab + 8*codebook_size] Exp(1) draws in the reference's RNG
 *           order (slow head first, then the 8 codebooks), or NULL = on-device counter RNG
 *   forced_codes host int32[B][8][chunk] teacher-forces the AR (parity tests), or NULL */
int sva_step(sva_batch* b, const float* pcm_in, float* pcm_out, const float* noise, const int32_t* forced_codes);
/* same with device pointers (no host copies); asynchronous: d_pcm_in must stay valid and d_pcm_out must not be read until
 * sva_sync() (or a later synchronous call on the handle) returns.  The engine runs on streams of its own and does NOT synchronise
 * with the caller's: whatever produced d_pcm_in (a kernel or copy on another stream) must have COMPLETED before this call.  With sva_stream_params.pipeline the stages of consecutive
 * calls overlap on three streams. */
int sva_step_device(sva_batch* b, const float* d_pcm_in, float* d_pcm_out);
/* Stream-ordered form -- what a torch caller wants: process_one_chunk in the reference runs on the caller's current stream
 * (evaluations/infer_arvc.py:495-508), so the producer of the input is ordered before it and the consumer of the output after it.
 * caller_stream is a hipStream_t (NULL = the legacy default stream; pass torch.cuda.current_stream().cuda_stream).  The engine's first
 * access to d_pcm_in waits (event, on the device) for everything enqueued on caller_stream so far; with join_output != 0 the
 * caller's stream then waits for the step's output, i.e. full same-stream semantics (and no overlap between consecutive steps);
 * with join_output == 0 consecutive steps keep overlapping, d_pcm_in must not be rewritten and d_pcm_out not read before a later
 * sva_join_stream(b, stream) (device-side wait for all engine work enqueued so far) or sva_sync(). */
int sva_step_device_on(sva_batch* b, const float* d_pcm_in, float* d_pcm_out, void* caller_stream, int join_output);
int sva_join_stream(sva_batch* b, void* caller_stream);
int sva_sync(sva_batch* b);
/* stream_infer's chunk loop (evaluations/infer_arvc.py:650-675) in one call: n_chunks consecutive sva_step_device steps over
 * host arrays pcm_in / pcm_out float[B][n_chunks * 2048 * chunk] (staged through device memory, stages pipelined when
 * sva_stream_params.pipeline is set), synchronised on return.  Same results as n_chunks calls of sva_step with noise = NULL. */
int sva_stream_chunks(sva_batch* b, const float* pcm_in, float* pcm_out, int n_chunks);

/* ---- seam-level entry points (parity tests, drop-in for the module calls) ------------------ */
/* speech_tokenizer.encode (firefly_encoder.py:553-566) on full windows: audio host float[B][W*2048]
 * -> codes int64[B][W] (+ optional L2-normalised pre-sign u float[B][W][13]) */
int sva_encode_window(sva_batch* b, const float* audio, int64_t* codes_out, float* u_out);
/* wav2target_fn (infer_arvc.py:168-171) -> FireflyArchitecture.encode (modules/vqgan/modules/firefly.py:560-574) of the
 * PROMPT on full windows: audio host float[B][W*2048] -> acoustic codes int32[B][8][W] (the ref_audio_codes operand of
 * sva_prefill_prompt).  Needs the optional voc.backbone.* / voc.quantizer.downsample.* / ...residual_fsq...project_in
 * tensors; fails with an error if the engine was finalized without them. */
int sva_firefly_encode(sva_batch* b, const float* audio, int32_t* codes_out);
/* code2wav_fn (infer_arvc.py:173-176) with the reference's window semantics (zero history):
 * codes host int32[B][8][T] -> pcm float[B][2048*T];  T <= voc_max_frames */
int sva_vocode_window(sva_batch* b, const int32_t* codes, int T, float* pcm_out);
/* the two halves of code2wav_fn as seams of their own (infer_arvc.py:175): firefly.quantizer.decode
 * (modules/vqgan/modules/fsq.py:112-116) codes int32[B][8][T] -> z float[B][4T][512] (channel-last; the reference tensor is
 * [B, 512, 4T]) and firefly.head (firefly.py:280-293) z -> pcm float[B][2048*T]; window semantics, T <= voc_max_frames */
int sva_quantizer_decode(sva_batch* b, const int32_t* codes, int T, float* z_out);
int sva_vocoder_head(sva_batch* b, const float* z, int T, float* pcm_out);
/* streaming-exact vocoder: continue from the ring-buffer state: codes int32[B][8][T] -> pcm[B][2048*T] */
int sva_vocode_stream(sva_batch* b, const int32_t* codes, int T, float* pcm_out);
int sva_vocode_reset(sva_batch* b);

/* ---- single streams inside a running batch ---------------------------------------------------------------------------------
 * Replace the stream in `slot` of a begun batch by a new utterance.  Same operands as sva_prefill_prompt.  From the next step on the slot
 * behaves exactly like a slot of a fresh batch after sva_prefill_prompt + sva_streams_begin: zero audio window, silence-steady encoder
 * state, ceil(delay / chunk) steps of zero output while its own delay fills, then decoding from frame 0 with noise keyed by noise_seed.
 * Every other slot is unaffected: all its later outputs are bit-identical to a run without the call.  Drains the batch's streams.
 * The step in which the slot's delay fills also prefills its prompt and primes its vocoder with the prompt's tail: that step stalls every
 * stream of the batch ("Restarting single streams").  With slot_priming = 0 the priming is a whole-batch vocoder run of
 * decode_window_frames - 1 frames in chunk-sized steps, and the stall grows with the batch; with slot_priming = 1 it is one pass over a
 * one-stream workspace plus a copy of the slot's history rows (sva_stream_params.slot_priming states what stays identical).
 * Fails, changing nothing, before sva_streams_begin, for a slot out of range, for R <= delay (or a prompt that does not fit the KV cache /
 * is shorter than the vocoder's 16-frame receptive field), and in the configurations that cannot fill one slot's encoder state:
 *   - encode_window_frames <= 40 + chunk_frames: the batch runs the full-window encoder, which keeps no cached silence state;
 *   - a batch whose persistent AR decode kernel has timed out (sva_streams_begin restarts all its streams). */
int sva_stream_restart(sva_batch* b, int slot, const int64_t* ref_content_codes, const int32_t* ref_audio_codes, int R,
                       const float* style, const float* timbre, uint64_t noise_seed);
/* Idle a slot: its input is no longer read (it counts as zeros, so the caller may leave anything there, NaN included), its output is zeros,
 * and it never raises an error of its own (re-prefill, range flag).  Only sva_stream_restart brings it back.  Fails before
 * sva_streams_begin and for a slot out of range.  Drains the batch's streams. */
int sva_stream_retire(sva_batch* b, int slot);
/* phase: 0 retired, 1 delay filling, 2 decoding; frames = frames decoded since the slot's stream began (0 unless decoding) */
int sva_stream_state(sva_batch* b, int slot, int* phase, long* frames);
/* The sampler settings of one slot.  Every slot owns a pair (temperature, top_p) in device memory, filled from sva_stream_params at
 * sva_batch_create and read by every sampler per stream, so slots with different settings share a batch and a captured graph stays valid
 * when a pair changes.  Valid any time after sva_batch_create, before or after sva_streams_begin; takes effect from the slot's next decoded
 * frame; every other slot is unaffected, and a slot holding the batch's values computes what it computed before.  temperature is clamped
 * at 1e-5 like the batch value; every top_p >= 0 is accepted, top_p = 0 keeps rank 0 only (the reference's rule: cum > top_p except
 * rank 0), i.e. the slot is greedy whatever the noise.  A slot keeps its pair until it is set again or the slot is restarted:
 * sva_stream_restart puts the batch's values back ("a slot of a fresh batch"), sva_streams_begin and sva_stream_retire leave the pair.
 * Drains the batch's streams.  Fails, changing nothing, for a slot out of range and for a NaN, negative or infinite argument. */
int sva_stream_set_sampling(sva_batch* b, int slot, float temperature, float top_p);
/* the slot's pair as it was set (temperature before the clamp); either pointer may be NULL */
int sva_stream_get_sampling(sva_batch* b, int slot, float* temperature, float* top_p);
/* activations since the batch was created: counts[0] slot-local ones (slot_priming = 1), counts[1] whole-batch ones; last_ms (may be NULL):
 * host wall time of the last activation -- prompt prefill, delay fill, vocoder priming -- taken after its final synchronise (0 before the first) */
int sva_stream_activations(sva_batch* b, long counts[2], float* last_ms);

/* ---- save and resume single streams ------------------------------------------------------------------------------------------
 * A snapshot ("blob") holds everything one slot's stream consists of -- csrc/snapshot/slot_state.h lists it, DESIGN.md 5d tabulates it: the
 * audio window, the encoder's histories and token cache, the content and prediction histories, the slow KV rows 0 .. last_pos, the speaker
 * operands and cached embeddings, position, frame and content counters, noise seed, sampling pair, the vocoder's history rows, and the stored
 * prompt -- in a versioned little-endian container (csrc/snapshot/snapshot_format.h: magic "SVASNAP1", two signatures, a checksum).  Two
 * saves of an unchanged slot are byte-identical.
 * Bit-identical continuation: run a stream for K0 steps in slot s of batch A, save it, load it into slot t of a batch D created from the same
 * engine with the same sva_config and sva_stream_params (n_streams included), feed it chunks K0, K0 + 1, ...: it produces bit for bit the PCM,
 * content codes, audio codes, positions and frame counts slot s of A produces for those chunks, whatever D's other slots carry and however
 * many steps D has run.  D may be A itself (the same slot at a later step is a rollback).
 * A batch with another n_streams is accepted exactly when its layout signature equals the blob's (the forms of its vocoder levels, the
 * history geometry); the state is then transferred bit-exactly, and the outputs agree with the source as two batches of different size
 * ever agree: their GEMM tilings differ.
 * What does not travel: sampler edits (a batch property; the sampling pair is a slot property and does travel -- unlike sva_stream_restart,
 * a load restores the blob's pair), the I/O adaptor's FIFOs and phase counters (batch-wide: both calls are refused while one is open), and
 * the weights: they are NOT fingerprinted, loading a blob into an engine with other weights is the caller's error.
 * Captured graphs stay valid: only device memory behind fixed pointers changes.  Both calls drain the batch's streams and run on its main
 * stream, never beside a step.
 * Refusals change nothing and name their reason through sva_last_error: a batch that has not begun, a slot out of range, an open I/O adaptor,
 * a batch whose persistent AR kernel has timed out; save: a slot that is not decoding (phase 2), a buffer that is too small; load: a batch
 * whose lock-step delay has not filled yet, a blob that is truncated, has a wrong magic or version or fails a checksum (-10 .. -14), a blob
 * whose configuration (-15) or layout (-16) signature differs from the batch's -- the message names the first differing field -- and a blob
 * whose slot fields contradict each other or whose code tables (content and prediction histories, prompt tail, stored prompt) hold a value
 * outside its embedding table (-13): a checksum is no proof of origin, so what a load installs as gather indices is range-checked. */
/* bytes sva_stream_save would write for this slot now (grows with the slot's KV position); < 0 on error */
long sva_stream_save_size(sva_batch* b, int slot);
/* Snapshot of one DECODING slot (phase 2) of a begun batch into caller memory.  Read-only: the slot and every other slot go on
 * bit-identically.  cap < needed: fails, *written = needed, nothing written. */
int sva_stream_save(sva_batch* b, int slot, void* blob, long cap, long* written);
/* Replace whatever `slot` holds (any phase) by the stream in the blob.  From the next step on the slot continues that stream: phase 2,
 * its frame count, KV position, content count, noise seed and counter, sampling pair, stored prompt, code history.  Every other slot is
 * bit-identical to a run without the call.  Everything is validated before any state changes. */
int sva_stream_load(sva_batch* b, int slot, const void* blob, long nbytes);
/* GPU-free: parse and validate a blob (header and payload checksums).  info[8] = {format version, frames decoded, last_pos, content count,
 * ref_len, ar_dtype, chunk_frames, payload bytes}; < 0 for a blob that is truncated, corrupt or of another version */
int sva_stream_blob_info(const void* blob, long nbytes, long* info);

/* ---- I/O adaptor: feed and read a running batch at a caller-chosen sample rate, in blocks of any length, as float32 or int16 ----
 * Every slot is fed n samples per call at io_rate and gets n samples back at io_rate; everything between the caller's buffer and the engine's
 * 44.1 kHz chunk runs on the device (csrc/io/).  The filter is the one audio_io.resample states: torchaudio 2.4 sinc_interp_hann,
 * lowpass_filter_width 6, rolloff 0.99, weights computed in float64 and rounded once to fp32.  Let x be everything pushed into a slot
 * (samples before the slot's last restart count as zeros): the engine's k-th chunk is resample(x, io_rate, 44100)[k * 2048c : (k + 1) * 2048c],
 * and the caller receives L zeros followed by resample(Y, 44100, io_rate), Y being the concatenated step outputs.  A sample is produced as
 * soon as the last input sample its phase reads has arrived (taps at the clip of the window, weight ~4e-33, are left out), each in one
 * fixed-order fmaf chain, so the result does not depend on how the signal is cut into calls.  L -- the smallest delay with which every call
 * that pushes n can pop n -- depends on io_rate and chunk_frames only.  io_rate == 44100 is a re-blocking pass-through: samples are copied.
 * int16: x / 32768 on load; round-to-nearest-even of y * 32768 saturated to [-32768, 32767] on store.
 * Accepted rates: an integer in 8000 .. 96000 whose ratio to 44100, reduced by their gcd, has both terms <= 640; others are refused.
 * One adaptor per batch, opened after sva_streams_begin.  While it is open, sva_step / sva_step_device / sva_step_device_on /
 * sva_stream_chunks and sva_streams_begin on the batch are refused (they would desynchronise the FIFOs); sva_stream_restart also zeroes the
 * slot's two filter histories and its share of the chunk staging, sva_stream_retire needs nothing beyond its flags (a retired slot's input
 * is not read); every other slot stays bit-identical.  sva_batch_destroy closes a forgotten adaptor.
 * The adaptor's FIFOs and phase counters are batch-wide, not a slot's: they are not part of a stream snapshot, and sva_stream_save /
 * sva_stream_load are refused while an adaptor is open. */
typedef struct sva_io sva_io;
/* fmt: 0 float32, 1 int16.  max_block: largest n of one call.  Opening finds L by walking three periods of the counters' pattern sample by
 * sample on the host (a period is io_rate / gcd * 2048c / gcd(44100 / gcd, 2048c) samples): 10-45 ms at chunk_frames 1-4, about 0.7 s at 64. */
int sva_io_open(sva_batch* b, int io_rate, int fmt, int max_block, sva_io** out);
void sva_io_close(sva_io* io);
/* host arrays [B][n] in and out; runs the planned steps (0, 1 or several, the sva_step_device path, pipelined if the batch is); synchronised on
 * return; steps_run may be NULL.  n outside 1 .. max_block is refused with the state unchanged. */
int sva_io_process(sva_io* io, const void* pcm_in, void* pcm_out, int n, int* steps_run);
/* device pointers; asynchronous, no host synchronisation; ordering as for sva_step_device_on: the engine waits on caller_stream before its
 * first access to d_in and d_out (NULL is the default stream, ordered like any other), join_output != 0 makes caller_stream wait for the
 * output; sva_sync / sva_join_stream apply.
 * Both process calls advance the adaptor's sample counters before they launch: if a launch or an engine step then fails, counters and
 * device state have diverged, and every later call on this adaptor is refused with an error that says so (close it, open a new one). */
int sva_io_process_device(sva_io* io, const void* d_in, void* d_out, int n, void* caller_stream, int join_output);
/* L in io-rate samples; the part of it that is filter delay (what L would be with an engine that consumed single samples) */
int sva_io_latency(sva_io* io, int* total, int* filter_only);

/* AR seams with caller-supplied content codes (chunk_frames == 1):
 *   ARVCWrapper.prefill_src_condition4delay (modules/arvc_wrapper.py:114-119): codes int64[B][delay]
 *   ARVCWrapper.decode_one (:121-126 -> dual_ar_stream.py:817-837): code int64[B] -> codes_out int32[B][8],
 *   pos_out int32[B] (kv_pos[-1]); noise float[B][vocab + 8*codebook_size] or NULL; forced int32[B][8] or NULL
 * Both refuse, before anything is uploaded or launched, a call whose rows would leave the KV cache: sva_ar_decode_one when any slot has
 * last_pos + 2 >= max_seq_len, sva_ar_delay_fill when last_pos + 2 * delay - 1 >= max_seq_len.  The error names the cache; positions and cache
 * rows are unchanged and the batch stays usable (sva_prefill_prompt + sva_streams_begin start the slot afresh). */
int sva_ar_delay_fill(sva_batch* b, const int64_t* codes);
int sva_ar_decode_one(sva_batch* b, const int64_t* code, const float* noise, const int32_t* forced, int32_t* codes_out,
                      int32_t* pos_out);

/* Offline conversion, ARVCWrapper.generate (modules/arvc_wrapper.py:82-98 -> DualARWrapper.generate, dual_ar_stream.py:698-762)
 * on a batch created with n_streams = 1, chunk_frames = 1: one prefill of 33 + 2(R+delay) + 1 tokens, then S-1 decode steps
 * (the last `delay` frames are driven by the wait4end embeddings).  ref_cc int64[R], ref_ac int32[8][R], src_cc int64[S],
 * noise float[S][vocab + 8*codebook_size] or NULL (device RNG keyed by noise_seed); codes_out int32[8][S].
 * This is the one-utterance call of the code behind sva_generate_many (same checks, same rules, same kernels).
 * Follow with sva_vocode_window(codes, S) for code2wav_fn (evaluations/infer_arvc.py:349-360). */
int sva_generate(sva_batch* b, const int64_t* ref_cc, const int32_t* ref_ac, int R, const int64_t* src_cc, int S,
                 const float* style, const float* timbre, uint64_t noise_seed, const float* noise, int32_t* codes_out);

/* ARVCWrapper.generate for every slot of a batch at once (chunk_frames == 1).  n == n_streams utterances; utterance i lives in slot i:
 * ref_cc[i] int64[R[i]], ref_ac[i] int32[8][R[i]], src_cc[i] int64[S[i]], style float[n][192], timbre float[n][32][128], noise_seed[n];
 * noise float[S_max][n][vocab + 8*codebook_size] (frame-major, S_max = max S[i]) or NULL = device RNG keyed per slot by noise_seed[i];
 * codes_out[i] int32[8][S[i]]: exactly 8 * S[i] ints are written.
 * Every slot follows the rules of generate on its own: frame 0 samples at temperature = top_p = 0.7, later frames with
 * the slot's own pair (sva_stream_set_sampling); sampler edits apply from frame 1.  The prompts run as packed passes over the rows of several
 * slots; a slot that has produced its S[i] frames rides along parked until the longest one ends.  Every argument is checked before any state
 * changes: delay < S[i] <= 4096, 33 + 2(R[i] + delay) + 1 + 2(S[i] - 1) <= 2048.  Afterwards sva_prefill_prompt + sva_streams_begin start streams afresh. */
int sva_generate_many(sva_batch* b, int n, const int64_t* const* ref_cc, const int32_t* const* ref_ac, const int* R,
                      const int64_t* const* src_cc, const int* S, const float* style, const float* timbre,
                      const uint64_t* noise_seed, const float* noise, int32_t* const* codes_out);

/* taps of the last step: "content_codes" int32[B][chunk], "audio_codes" int32[B][8][chunk] (as int32),
 * "slow_logits" float[B][vocab], "fast_logits" float[B][8][codebook_size], "hidden" float[B][dim],
 * "semantic" int32[B], "last_pos" int32[B], "cached_audio_emb" float[B][dim] (the embedding of the last decoded frame's codes: the
 * audio row of the next frame), "mel" float[B][T][160] ... ; returns #bytes or <0 */
long sva_get_tap(sva_batch* b, const char* what, void* out, long out_bytes);
/* the stream state `pred_codes[..., -n:]` of evaluations/infer_arvc.py:520-523 for one slot: the last n predicted frames
 * (n <= frames decoded so far, n <= 4096 = the device ring), int32 codes_out[8][n].  Drains the batch's streams first.
 * *n_frames_total (optional) receives the number of frames the slot has decoded since sva_streams_begin. */
int sva_stream_codes(sva_batch* b, int slot, int n, int32_t* codes_out, long* n_frames_total);
/* per-stage device time of the last sva_step in ms: [encoder, ar, vocoder, total] (hipEvents) */
int sva_get_timings(sva_batch* b, float ms[4]);
/* dominant-kernel bookkeeping for bench.py: number of conv-GEMM launches and their summed
 * algorithmic FLOPs in the last step */
int sva_get_gemm_stats(sva_batch* b, double* flops, long* launches);
/* ... and their summed ALGORITHMIC bytes (every operand element once: input rows incl. the tap halo, weights, outputs, residual) */
int sva_get_gemm_bytes(sva_batch* b, double* bytes);

/* roofline leg of bench.py: bracket every conv-GEMM launch of the following steps with hipEvents on the
 * engine stream; sva_get_gemm_profile returns the summed kernel time and the launch count since enabling */
int sva_profile_gemm(sva_batch* b, int enable);
int sva_get_gemm_profile(sva_batch* b, double* total_ms, long* launches);
/* per-launch rows (M, N, K, taps, mode bits, microseconds) of the profiled steps; returns the number of rows */
long sva_get_gemm_profile_table(sva_batch* b, double* out, long max_rows);

/* ---- prompt path: device primitives of the two speaker-embedding encoders (SURVEY.md 8f N1 iii / iv) --------------------------
 * calculate_style_vec (evaluations/infer_arvc.py:179-211: Kaldi fbank -> CAM++, modules/campplus/DTDNN.py:50-137) and
 * calculate_timbre_latent (:213-223: MelSpectrogram -> ECAPA-TDNN -> PerceiverResampler -> FSQ,
 * modules/bicodec_speaker_encoder/speaker_encoder.py:136-144) run once per utterance; the host mirror
 * (streamvoiceanon_amd/prompt_encoders.py) owns the activation buffers and the topology, these entry points do the arithmetic
 * on device arrays (channel-last rows [T][C], row strides in floats; every pointer below is a DEVICE pointer from sva_dev_alloc
 * unless it says host).  All of them run on ONE engine-owned stream, in call order (sva_dev_upload / _download are ordered with them and
 * return when their copy is done).  That stream is non-blocking: nothing here is ordered with the caller's own streams, the legacy default stream or
 * a batch's streams -- a buffer produced elsewhere must be complete (sva_sync / hipStreamSynchronize of its producer) before it is passed in, and a
 * result consumed elsewhere must be fetched with sva_dev_download (which waits) or after a hipDeviceSynchronize. */
int sva_dev_alloc(sva_engine* e, long n_floats, float** out);            /* zero-initialised */
int sva_dev_free(sva_engine* e, float* p);
int sva_dev_upload(sva_engine* e, float* dst, const float* host_src, long n_floats);
int sva_dev_download(sva_engine* e, float* host_dst, const float* src, long n_floats);
/* nn.Conv1d / nn.Linear: y[t][n] = bias[n] + sum_{tap,c} x[(t*stride + tap*dil)*ldx + c] * W[n][tap*Cin + c]; x points at tap 0 of
 * output row 0 (the caller pads); f32-MFMA conv-GEMM when Cin % 16 == 0, a plain kernel otherwise */
int sva_op_conv(sva_engine* e, const float* x, long ldx, int T, int stride, int dil, int taps, int Cin, const float* W, const float* bias, int N,
                float* y, long ldy);
/* y = post(scale[c] * pre(x) + shift[c]); relu_mode 0 none, 1 ReLU after (batchnorm-relu), 2 ReLU before (Conv1dReluBn); eval-mode
 * BatchNorm arrives folded into scale / shift (either may be NULL) */
int sva_op_affine(sva_engine* e, const float* x, long ldx, int T, int C, const float* scale, const float* shift, int relu_mode, float* y, long ldy);
int sva_op_unary(sva_engine* e, float* x, long n, int op /* 1 log(max(x, p0)), 2 FSQ level-4 quantise, 3 sigmoid, 4 negate */, float p0);
int sva_op_colstats(sva_engine* e, const float* x, long ldx, int T, int C, float* mean, float* std_or_null, int unbiased);
int sva_op_cam_context(sva_engine* e, const float* y, long ldy, int T, int C, int seg_len, const float* mean, float* ctx, long ldc);   /* layers.py:103-119 */
int sva_op_mul(sva_engine* e, float* y, long ldy, const float* m, long ldm /* 0 = broadcast one row */, int T, int C, int sigmoid);
int sva_op_add(sva_engine* e, float* y, long ldy, const float* x, long ldx, int T, int C);
/* Conv2d k x k (k = 1 or 3, padding k/2, stride (stride_f, 1)) + folded BatchNorm (+ residual) (+ ReLU) on channel-first [C][F][T] */
int sva_op_conv2d(sva_engine* e, const float* x, int Cin, int F, int T, const float* W, int Cout, int k, int stride_f, const float* scale,
                  const float* shift, const float* res_or_null, int relu, float* y);
int sva_op_cf_to_rows(sva_engine* e, const float* x, int CF, int T, float* y, long ldy);
int sva_op_fbank_power(sva_engine* e, const float* wave, long n, float* frames_scratch /* [m][512] */, float* out, int ldo, int* frames_out /* host */);
int sva_op_stft_mag(sva_engine* e, const float* wave, long n, int n_fft, int win, int hop, float* frames_scratch, float* out, int ldo, int* frames_out /* host */);
int sva_op_attention(sva_engine* e, const float* q, const float* kv, int Lq, int Lk, int n_valid, int H, float* out, float* scratch /* [Lq][H][Lk] */);
int sva_op_geglu(sva_engine* e, const float* h, long ldh, int T, int Dh, float* out, long ldo);
int sva_op_l2norm(sva_engine* e, const float* x, int T, int C, const float* gamma, float scale, float* y);
/* The op sequence of one speaker-encoder call as a hipGraph: between _begin and _end the sva_op_* calls are recorded, not run (no
 * sva_dev_alloc / _upload / _download in between); _end returns an executable graph that sva_ops_graph_launch replays on the ops stream.
 * The reference computes these encoders once per utterance (evaluations/infer_arvc.py:179-223); the host mirror keeps one graph per
 * reference length (prompt_encoders.py), ~600 launches -> 1. */
int sva_ops_capture_begin(sva_engine* e);
int sva_ops_capture_end(sva_engine* e, void** graph_exec);
int sva_ops_graph_launch(sva_engine* e, void* graph_exec);
int sva_ops_graph_free(sva_engine* e, void* graph_exec);

/* Which decode the batch runs per frame: 1 = the persistent kernel of ar_decode.hip (two streams per launch: <= 6 streams, <= 4 with
 * ar_dtype = 1), 2 = the batched persistent kernel of ar_batch.hip (every stream of the batch in one launch: the larger batches), 0 = the
 * multi-launch decode (sampler edits set, layer sizes other than the reference's, or the residency check at sva_batch_create failed:
 * all workgroups of a persistent launch must fit the AR stream's CUs at once).  A persistent launch whose workgroups are NOT all
 * resident (GPU shared with another process) times out after ~50 ms: the next sva_sync / sva_step returns an error, every later step
 * fails, and sva_prefill_prompt + sva_streams_begin restart the streams on the multi-launch decode. */
int sva_batch_uses_persistent_decode(sva_batch* b);
/* debug options of the process ("key=value,key=value"; the same keys as the SVA_DEBUG environment variable, the engine's only
 * environment input -- listed in csrc/sva_common.h: ar_timing, pipe_trace, concurrency, ar_persistent, voc_fused_mask, autotune,
 * tune_log, tune_table, tune_dump).  Profiling and test switches; batches created afterwards see the change. */
int sva_debug_configure(const char* kv);
/* test hook, read-only: rows pos0 .. pos0 + n - 1 of one slot's slow-AR KV cache as float out[ar_layers][2 (k, v)][ar_heads][n][64]; an fp16
 * cache (ar_dtype = 1) is widened exactly.  Drains the batch's streams first.  Fails for a slot outside the batch or rows outside the cache
 * (slot < 0, slot >= n_streams, pos0 < 0, n < 1, pos0 + n > max_seq_len). */
int sva_test_kv_rows(sva_batch* b, int slot, int pos0, int n, float* out);
/* test hook, read-only: rows row0 .. row0 + n - 1 of the engine's table of fast layer 0 (RMSNorm + wqkv of every fast_embeddings row, before
 * RoPE, in the engine's AR element type; csrc/ar_decode.h) as float out[n][3 * ar_dim].  Fails when the engine has no table (sizes the
 * persistent decode kernel is not built for) or for rows outside it (row0 < 0, n < 1, row0 + n > codebook_size). */
int sva_test_fast_qkv0(sva_engine* e, int row0, int n, float* out);
/* test hook: set the persistent kernel's device-side timeout word, as a launch with non-resident workgroups would */
int sva_test_force_ar_timeout(sva_batch* b);
/* test hook: do the four chain streams of a pipelined batch -- main, encoder side, AR, vocoder -- run concurrently, i.e. sit on four
 * hardware queues?  pair_ok[6], pairs in the order (main, side) (main, AR) (main, vocoder) (side, AR) (side, vocoder) (AR, vocoder):
 * 1 = a kernel on the second stream ran while one on the first was still running, 0 = the two streams serialise.  Each pair costs at
 * most 2 ms (the waiting kernel gives up by the clock); synchronises the device. */
int sva_test_stream_overlap(sva_batch* b, int* pair_ok);

/* The optional sampler edits of decode_one_token_ar (modules/dual_ar_stream.py:1175-1213 -> logits_to_probs :1099-1117):
 *   previous_tokens [1 + num_codebooks][W] int32 (row 0 edits the token head, row cb + 1 codebook cb; negative entries are
 *   skipped): repetition penalty  s < 0 ? s * p : s / p  on the listed tokens, each once;
 *   suppress_tokens [n_suppress]: token-head logits set to -inf (:1189 passes the list to the first sample() only).
 * They apply to every stream of the batch from the next decoded frame on (sva_generate: from frame 1 -- the prefill's decode
 * takes no sampling_kwargs, :722); W = 0 and n_suppress = 0 remove them.  While edits are set the batch decodes with the
 * multi-launch path (the persistent kernel has no edit stage); at most 4096 entries per list. */
int sva_set_sampler_edits(sva_batch* b, const int32_t* previous_tokens, int W, float repetition_penalty, const int32_t* suppress_tokens,
                          int n_suppress);

/* kernel unit-test hook: C = A[M,K] * W[N,K]^T (+bias) through the conv-GEMM kernel (host arrays) */
int sva_test_gemm(int device, int M, int N, int K, const float* A, const float* W, const float* bias, float* C);

/* same through one given plan instead of the dispatcher's: kind 0 / 1 / 3 / 4 / 7 = GemmFamily SmallM / Tiled / Ring / Split / Stream
 * (csrc/sva_common.h, where the parameters a, b, c of each family are documented); kind 2: SmallM with its K axis also split over c >> 4
 * workgroups, c & 15 = column tiles, launched twice; kind 6: Planes / PlanesDma, a = tile variant */
int sva_test_gemm_choice(int device, int M, int N, int K, const float* A, const float* W, const float* bias, float* C, int kind,
                         int a, int b, int c);
/* The dispatcher's decision for a problem, without launching it and without a GPU.  desc: n = 1..3 group members x 12 ints
 *   {B, T, N, Cin, taps, stride, dil, flags, operands, pmode, misaligned, 0}
 *   flags bits: 1 bias, 2 gamma, 4 residual, 8 GELU, 16 a_silu, 32 w13, 64 accumulate, 128 rms_w, 256 dw_wT (+ dw_b, ln_w, ln_b), 512 cp_silu
 *   operands bits: 1 Wk, 2 Wh, 4 Wkh, 8 Wp, 16 Ap, 32 Cp (planes over the tensor's dense rows); pmode: -1, 1 = H3, 2 = H1
 *   misaligned bits: 1 A (a_off), 2 C (ldc), 4 residual (ldr) not a multiple of 4 floats
 * out[6] = {family (GemmFamily of csrc/sva_common.h), a, b, c, z, family number of the profiling tables}; an error (sva_last_error) where the
 * dispatcher refuses the problem. */
int sva_test_gemm_plan(const int* desc, int n, int* out);
/* The conv-GEMM in its conv and epilogue forms (csrc/sva_common.h: ConvGemm), n = 1..3 group members, on the production path.  Host arrays in,
 * host arrays out; every array is the WHOLE array with the caller's strides, offsets and padding, and C is uploaded before the launch, so
 * `accumulate` reads the caller's values and a sentinel survives wherever nothing is stored.
 *   desc: n x 32 int64 {B, T, N, Cin, taps, stride, dil, lda, a_off, a_bstride, a_len, ldc, c_off, c_bstride, c_len, ldr, r_off, r_bstride, r_len,
 *         act (0 / 1 GELU / 2 log-clamp), accumulate, a_silu, w13, skip_lo, skip_hi, use_wk (fragment-major weights packed from W), pmode (-1, or
 *         1 = H3 / 2 = H1: weight planes made as at finalize), a_planes (1: A handed over as planes over the dense rows of its array, made by the
 *         engine's activation pass; 2: with SiLU), c_planes (1: C also as planes over the dense rows of its array, 2: as planes only), cp_silu, 0, 0}
 *   fpar: n x 4 floats {scale, ln_eps, rms_eps, 0}
 *   ptrs: n x 16 pointers {A [a_len], W [N][taps Cin], bias [N], gamma [N], res [r_len], rms_w [Cin], dw_wT [7][Cin], dw_b, ln_w, ln_b [Cin],
 *         C [c_len] in and out, Cp uint16 [planes][c_len / ldc x Nout] in and out (K-blocked, csrc/planes_split.h), Ap uint16 [planes][a_len] out
 *         (optional: the A planes as the kernel read them), 0, 0, 0}; optional operands may be NULL
 *   plan: {-1} = the dispatcher (launch_conv_gemm_group), else {GemmFamily, a, b, c, z} run under the plan check (launch_conv_gemm_group_plan)
 *   repeat != 0: the launch runs a second time from the same initial C / Cp; out[1] = 1 when the two results are bit-identical, 0 when not
 *   out[2] = {family number of the profiling tables of what ran, repeat verdict (-1: not asked)}
 * Returns 0 when it ran, 1 when the problem was REFUSED before any launch (the dispatcher, the plan check or a launcher's own check; the arrays
 * come back as they went in), -2 on a HIP error, -4 on arguments the hook declines (an index outside an array); sva_last_error has the text. */
int sva_test_conv_gemm(int device, int n, const long long* desc, const float* fpar, void* const* ptrs, const int* plan, int repeat, int* out);
/* The host-side book of the per-slot stream state (csrc/slot_book.h: phases, KV positions, frame and content counters, what a step plans),
 * scripted without a batch and without a GPU.  cfg[7] = {B, chunk_frames, delay, max_seq_frames, buffer_frames, decode_window_frames,
 * speaker prefix rows (timbre tokens + 1)}; ops: n_ops x 3 ints {op, slot, R} with op 0 = begin, 1 = prefilled(slot, R frames),
 * 2 = one chunk step, 3 = restart(slot, R frames), 4 = retire(slot), 5 = prefilled(slot, delay + 1 + R frames) stored truncated to R frames; the other prompts are stored untruncated;
 * 6 = stage the counters of the next adopt {last_pos = the slot field, nframes = the R field; ncontent = nframes + delay}, 7 = adopt(slot, a stored
 * prompt of R frames): the transition of sva_stream_load.  trace: n_ops rows of 8 B + 6 ints, the
 * state after the op:  B x {phase, last_pos, nframes, ncontent} | delay_filled | one-pass re-prefill possible (-1: none planned) |
 * n_redo, redo[B] | n_rewind, rewind[B] x {slot, position} | n_activated, activated[B] | vocoder priming frames (begin: of the batch; a step:
 * of its first activated slot; else -1).  Unused list entries are -1; the lists are what the step planned before it carried them out. */
int sva_test_slot_book(const int* cfg, const int* ops, int n_ops, int* trace);
/* slot_pack_kernel / slot_unpack_kernel alone (csrc/snapshot/slot_pack.hip), nothing of an engine involved.  table: n_seg x 9 longs {byte
 * offset of slot 0's first row in the source arena, the same in the destination arena, slot stride, row stride, row bytes, rows, kind (0 plain,
 * 1 ring, 2 KV prefix, 3 blocked plane), element bytes (2 | 4), ring: elements the origin advances per step}.  Packs slot_src of arena_src at
 * chunk counter step_src into image_out (image_bytes = the sum of the segments' lengths, each padded to 16), then unpacks that image into
 * slot_dst of arena_dst (uploaded as given, returned as the kernel left it) at chunk counter step_dst.  cus sizes the grid.  A table that
 * would leave an arena is refused before anything is launched. */
int sva_test_slot_pack(int device, const long* table, int n_seg, const void* arena_src, long src_bytes, void* arena_dst, long dst_bytes, int slot_src,
                       int slot_dst, int step_src, int step_dst, void* image_out, long image_bytes, int cus);
/* The snapshot container (csrc/snapshot/snapshot_format.h) without a GPU.  sig = n_cfg configuration values, then n_layout layout values.
 * op 0, build: desc[9] = {n_cfg, n_layout, frames, last_pos, content count, ar_dtype, chunk_frames, ncb, ref_len}; sig continues with ref_len
 *   stored content codes and ncb x ref_len stored audio codes; bytes / nbytes = the payload (a multiple of 16); the blob goes to out,
 *   result[0] = its length.
 * op 1, check: bytes / nbytes = a caller-supplied byte string, sig = the signatures of a scripted batch, desc[2] = the payload bytes its
 *   segments hold (< 0: not compared).  result[12] = {refusal code (0 accepted), index of the first differing signature value (-1 none),
 *   format version, frames, last_pos, content count, ref_len, ar_dtype, chunk_frames, payload bytes, ncb, header bytes} (-1 where unknown). */
/* The split of the batch's last sva_stream_save / sva_stream_load: ms[4] = {pack or unpack kernel (hipEvents around the launch), the host <->
 * device copy of the image (wall), everything else of the call (wall: drain, validation, table upload, checksum, header, mirrors), -1};
 * counts[2] = {image bytes of that call, steps this batch has run in the pipelined regime since it was created}.  measure_d2d != 0: ms[3] =
 * one hipMemcpyDtoDAsync of the same byte count out of the batch's image buffer, between the same events on the same stream. */
int sva_test_snapshot_timings(sva_batch* b, int measure_d2d, float* ms, long* counts);
int sva_test_snapshot_header(int op, const long* desc, const long* sig, const void* bytes, long nbytes, void* out, long out_cap, long* result);
/* The adaptor's planner (csrc/io/io_plan.h) without a batch and without a GPU: a stream at io_rate fed blocks[n_blocks] samples.
 * out: 12 header ints {L, filter part of L, chunk staging buffers, history samples at io_rate, history samples at 44100, output FIFO
 * samples, period of the counters' pattern in pushed samples, in orig, in new, in width, out width, max block}, then 5 ints per block:
 * {model-rate samples made ready, engine steps, io-rate samples produced, model-rate samples staged after the call, output FIFO fill after
 * the call's pop}.  Returns the ints written; < 0 for an unsupported rate or a short out. */
int sva_test_io_plan(int io_rate, int chunk_frames, const int* blocks, int n_blocks, int* out, int out_cap);
/* Kernel hook of the adaptor: one stream-free run over host arrays x [B][n] (fmt_in) -> y [B][y_cap] (fmt_out), the input cut into calls
 * at splits[n_splits] (ascending sample indices inside 0 .. n).  to_rate == 44100: io_resample_in_kernel through its chunk staging;
 * from_rate == 44100: io_resample_out_kernel through its FIFO; both 44100: one after the other, as the pass-through does.  int16 is
 * accepted where the adaptor has it: the input of the first, the output of the second.  n_out: samples per slot that were ready. */
int sva_test_resample(int device, int from_rate, int to_rate, int fmt_in, int fmt_out, int B, const void* x, long n, const int* splits,
                      int n_splits, void* y, long y_cap, long* n_out);
/* The book's stored prompt: a prompt of R frames (content code i at frame i, audio code 1000 q + i in codebook q) stored truncated to Rt
 * frames; out [ncb][n] = frames [first, first + n) of the last P stored frames (what primes a vocoder), stored[4] = {ref_len, content codes
 * kept, audio codes kept, last content code kept}. */
int sva_test_slot_prompt_tail(int R, int Rt, int ncb, int P, int first, int n, int* out, int* stored);
/* fp16-weight GEMM of the batched fp16 AR decode (csrc/gemm_f16w.hip; the reference's autocast(fp16) linear layers,
 * modules/dual_ar_stream.py:1168-1219): C = epi(A x fp16(W)^T), mode bits 1 = RMSNorm prologue, 2 = residual, 4 = SwiGLU pairs;
 * iters > 0 also returns the average microseconds per launch. */
int sva_test_gemm_f16w(int device, int M, int N, int K, const float* A, const float* W, const float* bias, const float* rms_w,
                       const float* res, int mode, float* C, int iters, float* out_us);
/* The fp16-operand weight-streaming conv-GEMM of an enc_dtype = 1 encoder below batch scale (csrc/gemm_stream_h.hip) through its production
 * launcher.  Dense host arrays: A [B][(T - 1) stride + (taps - 1) dil + 1][Cin], W [N][taps * Cin], bias [N] or null, gamma [N] / res [B][T][N]
 * (mode bit 2), C [B][T][N, or N / 2 with SwiGLU] in and out.  mode bits: 1 = GELU, 2 = gamma + residual, 4 = rows [T / 4, T / 2) of every item
 * skipped, 8 = SwiGLU, 16 = padded item strides and offsets on the device, 32 = range check (a non-finite output fails the call).  (mt, nt, kw) =
 * 16-row tiles, 16-column tiles, K-split waves per workgroup; mt = 0: the heuristic's.  iters > 0 also returns microseconds per launch. */
int sva_test_gemm_h16(int device, int B, int T, int N, int Cin, int taps, int dil, int stride, const float* A, const float* W, const float* bias,
                      const float* gamma, const float* res, int mode, int mt, int nt, int kw, float* C, int iters, float* out_us);
/* conv-GEMM fed from pre-split 16-bit operand planes (csrc/gemm_planes.hip; the Linear layers of firefly.py:421-440 and
 * windowed_transformer.py:134-143 at batch scale): mode 0 = three bf16 planes / six products (fp32-grade), 1 = two fp16 planes /
 * three products (fp32-grade inside the fp16 range), 2 = one fp16 plane (torch.autocast(fp16), evaluations/infer_arvc.py:493);
 * variant = tile variant 0..5; flags: 1 = A handed over as planes, 2 = C leaves as planes only (summed back to fp32 for the caller),
 * 4 = GELU epilogue, 8 = SiLU on load, 16 = range check (a non-finite output of the fp16 formats fails the call, as sva_sync does for a batch);
 * iters > 0 also returns the average microseconds per launch. */
int sva_test_gemm_planes(int device, int M, int N, int K, const float* A, const float* W, const float* bias, float* C, int mode,
                         int variant, int flags, int iters, float* out_us);
/* Prefill attention of the slow AR (modules/dual_ar_stream.py:338-356 with causal_mask[kv_pos]): M query rows [M][H*64] at positions
 * pos0 .. pos0 + M - 1 against keys / values [pos0 + M][H*64] placed in a cache of S positions (fp32, or fp16 when half_kv).
 * out_ref: the per-row kernel, out_mfma: the flash-style MFMA kernel; us[2] their launch times when iters > 0. */
int sva_test_prefill_attention(int device, int M, int H, int pos0, int S, const float* q, const float* keys, const float* vals,
                               int half_kv, float* out_ref, float* out_mfma, int iters, float* us);
/* the same rows through the decode frame's paired attention kernel (rows 2 i, 2 i + 1 share one pass over the slot's K / V; M even) */
int sva_test_pair_attention(int device, int M, int H, int pos0, int S, const float* q, const float* keys, const float* vals,
                               int half_kv, float* out_ref, float* out_mfma, int iters, float* us);
/* The runs arm of the same kernel (launch_ar_prefill_attention_runs): a packed pass of total_rows rows q [total_rows][H*64] holding n_runs runs
 * runs[r] = {slot, pos0, M, row0} against a cache [n_slots][2][H][S][64] (fp32, or rounded to fp16 when half_kv).  out [total_rows][H*64] is uploaded
 * first, so a sentinel survives where nothing is stored.  single_out (or NULL) receives the single-run launcher called once per run on the same
 * device data.  Returns 1 when the launcher refused (nothing written). */
int sva_test_prefill_attention_runs(int device, int n_runs, const int* runs, int total_rows, int H, int S, int n_slots, int half_kv, const float* q,
                                    const float* cache, float* out, float* single_out);
/* The packing of sva_generate_many's prompt passes, no GPU needed: out = pass index and row0 of each of the n slots (2 n ints), then for every
 * pass {number of tiles, then {run, q0} per tile} with run counted inside the pass; out_cap ints available.  Returns the number of passes,
 * < 0 for an M outside 1 .. Mmax or a short out. */
int sva_test_prefill_pack(const int* M, int n, int Mmax, int* out, int out_cap);

/* Per-kernel hooks of the non-GEMM launchers (csrc/kernels.h), for tests/test_gpu_kernels.py: host arrays in, the production launcher with the
 * caller's arguments, host arrays out.  Output arrays are uploaded before the launch, so a sentinel the caller wrote survives wherever the
 * kernel writes nothing; every index a launch touches is checked against the array lengths first.
 * Decode attention family over a cache [n_slots][2][H][S][64] (fp32 values; rounded to fp16 on upload and widened on return when half_kv) with
 * caller-chosen slot[M] / pos[M].  variant 0: launch_ar_attention, 1: split-key launch_ar_attention (8 splits) merged by the GEMV (mode 4:
 * out = x + W attention), 2: launch_ar_attention_pairs, 3: launch_ar_fast_attention (RoPE + cache write + attention, S <= 8), 4: GEMV mode 3
 * (out = x + W attention over <= 8 keys), 5: launch_rope_kvwrite (qkv rotated in place, cache written), 6: GEMV mode 2 (qkv[:, :D] = RoPE(W q-rows
 * RMSNorm(x)), k / v into the cache; W [3D][D]).  qkv [M][3 H 64] and cache are returned as the device left them; out [M][H 64]. */
int sva_test_decode_attention(int device, int variant, int M, int H, int S, int n_slots, const int* slot, const int* pos, int half_kv, float* qkv,
                              float* cache, const float* rope, int n_pos, const float* x, const float* W, const float* norm_w, float* out);
/* launch_enc_attention: qkv [B][T][3 H 64], rope [T][32][2] -> out [B][T][H 64] (rows below row0 untouched), or, n_planes = 1 / 2, the fp16 hi
 * (+ lo) planes uint16 [2][B T H 64] in the tensor's index space or K-blocked over B T rows (csrc/planes_split.h) */
int sva_test_enc_attention(int device, int B, int T, int H, int row0, const float* qkv, const float* rope, int n_planes, int blocked, float* out,
                           unsigned short* planes);
/* kind 0: launch_dwconv7_ln (p0 = taps [7][C], p1 = bias, p2 / p3 = LayerNorm weight / bias), 1: launch_layernorm_rows (p0 / p1 = weight / bias,
 * rows [skip_lo, skip_hi) of every item left alone), 2: launch_rmsnorm_rows (p0 = weight); x [x_len] and out [o_len] are whole arrays, the
 * strides and offsets are the launcher's; planes uint16 [2][p_len] as in sva_test_enc_attention */
int sva_test_rowop(int device, int kind, int B, int T, int C, const float* x, long x_len, long x_bstride, long x_off, int ldx, const float* p0,
                   const float* p1, const float* p2, const float* p3, float eps, float* out, long o_len, long o_bstride, long o_off, int ldo, int skip_lo,
                   int skip_hi, int n_planes, int blocked, unsigned short* planes, long p_len);
/* launch_bsq: norm_w (or NULL) = fused RMSNorm, zn_out (or NULL) [z_len], idx_out int64 [idx_len], u_out (or NULL) [idx_len][nbits] */
int sva_test_bsq(int device, int B, int T, int C, const float* z, long z_len, long z_bstride, long z_off, int ldz, const float* norm_w, float eps,
                 float* zn_out, const float* W, const float* bias, int nbits, long long* idx_out, long idx_len, int idx_bstride, int idx_off, float* u_out);
/* launch_stft_mag_ring (two = 0) / launch_stft_mag_ring2 over ring [B][N] with the engine's twiddle and window tables; step may be NULL;
 * mag [B][mag_rows][ldm] */
int sva_test_stft_ring(int device, int B, int N, const float* ring, const int* step, int n_chunk, int add, int m0, int nfr, int two, int m0b, int nfrb,
                       int row_b0, float* mag, int mag_rows, int ldm);
/* encode != 0: launch_fsq_encode (lat -> codes, Wt = project_in [G][4][gdim], bs [G][4]); else launch_fsq_decode (codes -> lat, Wt = project_out
 * [G][gdim][4], bs [G][gdim]) */
int sva_test_fsq(int device, int encode, int B, int T, int G, int gdim, float* lat, long l_len, long l_bstride, long l_off, int ld, const float* Wt,
                 const float* bs, int* codes, long c_len, long c_bstride, long c_gstride);
/* launch_conv_post_tanh: x rows [T + k - 1][C] per item -> pcm [T] per item; slot_flag [B] (per-slot flag words, kSlotOutputMuted = 2) or NULL */
int sva_test_conv_post(int device, int B, int T, int C, int k, const float* x, long x_len, long x_bstride, long x_off, const float* w, const float* bias,
                       float* pcm, long p_len, long p_bstride, long p_off, const int* slot_flag);

/* The tail of the AR decode, kernel by kernel (tests/test_gpu_decode_tail.py).  Arguments: desc (integers), fpar (floats), ptrs (host arrays, NULL =
 * absent), in the order listed.  Arrays marked in/out are uploaded first and downloaded whole, so a sentinel survives where nothing is written.
 * Returns 0 ran, 1 REFUSED by the launcher's own check (nothing launched, sva_last_error has its message), -2 HIP error, -4 declined by the hook
 * (an index outside an array).
 *
 * sva_test_sampler_launch: launch_sampler (small = 0) or launch_sampler_small (small = 1) with every argument, optionally after launch_logit_edits on
 * the same device rows.
 *   desc  0 small, 1 rows, 2 V, 3 ldl, 4 column offset of the rows in logits, 5 len(logits), 6 ldn, 7 offset of the rows in noise, 8 len(noise),
 *         9 kind, 10 noise_elem_off, 11 tok_stride, 12 offset into tok_raw / tok, 13 len(tok_raw) = len(tok), 14 forced_stride, 15 offset into forced,
 *         16 len(forced), 17 *use_forced (-1: NULL pointer), 18 rows of emb_table (>= V), 19 D, 20 ldo, 21 len(emb_out),
 *         22 edits first (0 / 1), 23 W, 24 prev_cap, 25 len(prev), 26 n_suppress, 27 len(suppress)
 *   fpar  temperature, top_p, repetition penalty
 *   ptrs  0 logits (in/out), 1 noise or NULL (device RNG), 2 seed uint64 [rows], 3 frame int [rows], 4 tok_raw (in/out), 5 tok (in/out, small only),
 *         6 forced, 7 emb_table, 8 emb_out (in/out), 9 prev, 10 suppress */
int sva_test_sampler_launch(int device, const long long* desc, const float* fpar, void* const* ptrs);
/* sva_test_sampler_rows: the same launchers and operands with per-row sampling pairs, as the engine hands them its per-slot pairs: samp float
 * [n_pairs][2] = {1 / max(temperature, 1e-5), top_p}, row r reads pair row_slot[r] (row_slot int [rows], NULL: pair r).  samp NULL: the scalars
 * of fpar, exactly sva_test_sampler_launch.  Declined (-4) for fewer pairs than rows or a row_slot entry outside the pairs. */
int sva_test_sampler_rows(int device, const long long* desc, const float* fpar, void* const* ptrs, const float* samp, int n_pairs,
                          const int* row_slot);
/* sva_test_ar_device: the device helpers of the persistent decode kernels (csrc/ar_device.h) in the instantiations their call sites use.
 *   op 0  nucleus_sample: inst 0 <4,4> at 256 threads, 1 <4,32> at 256, 2 <8,16> at 512 (one workgroup per row), 3 <1,16> at 512 (one wave per row)
 *     desc  0 inst, 1 rows, 2 V, 3 ldl, 4 len(logits), 5 ldn, 6 len(noise), 7 kind, 8 noise_elem_off;  fpar temperature, top_p
 *     ptrs  0 logits, 1 noise or NULL, 2 seed, 3 frame, 4 tok int [rows] (out), 5 same int [rows] (out: every participating thread returned tok)
 *   op 1  gemv<WT, K, ROWS, M, NORM>, one wave per group of ROWS weight rows: inst 0..9 = (768,6,2,norm) (768,2,2,-) (768,12,2,norm) (2304,2,2,-)
 *         (768,11,1,norm) (768,6,1,norm) (768,2,1,-) (768,12,1,norm) (2304,2,1,-) (768,3,1,norm)
 *     desc  0 inst, 1 WT = __half (weights rounded here), 2 groups, 3 index of the first weight row on the device (rows in front are allocated, never
 *           read), 4 ldx, 5 len(x), 6 ldo, 7 len(out);  fpar eps
 *     ptrs  0 W [groups ROWS][K], 1 x, 2 norm weight [K], 3 out [M][ldo] (in/out), 4 same int [groups] (out: all 64 lanes held the same values) */
int sva_test_ar_device(int device, int op, const long long* desc, const float* fpar, void* const* ptrs);
/* sva_test_gemv: launch_gemv modes 0 (plain) and 1 (SwiGLU over the w1 | w3 interleave); modes 3 / 4 with zero operands, to reach its refusals.
 *   desc  0 M, 1 N, 2 K, 3 ldx, 4 len(X), 5 rows of W, 6 ldy, 7 column offset into Y, 8 len(Y), 9 ldr, 10 len(res), 11 mode, 12 res = Y (alias), 13 S, 14 H
 *   fpar  eps;  ptrs  0 X, 1 W, 2 norm_w, 3 bias, 4 res, 5 Y (in/out) */
int sva_test_gemv(int device, const long long* desc, const float* fpar, void* const* ptrs);
/* sva_test_token_ops:
 *   kind 0 launch_logit_edits  desc rows, V, ldl, len(logits), W, prev_cap, len(prev), n_suppress, len(suppress); fpar penalty; ptrs logits (in/out), prev, suppress
 *   kind 1 launch_gather_rows  desc rows, D, ldo, len(out), table rows, len(idx), idx_stride, idx_offset; ptrs table, idx, out (in/out)
 *   kind 2 launch_audio_embed  desc rows, D, ldo, len(out), table rows, len(codes), code_stride, cb_stride, ncb, codebook_size; ptrs table, codes, out (in/out)
 *   kind 3 launch_shift_history  desc n_desc, B, col_slices, counter given, counter_add, len(buf), then (offset, bstride, H, T, C) per descriptor;
 *          ptrs buf (in/out), counter int [1] (in/out)
 *   kind 4 launch_ring_write   desc B, N, n, step given (0: NULL), step; ptrs ring [B][N] (in/out), chunk [B][n], slot_flag [B] or NULL */
int sva_test_token_ops(int device, int kind, const long long* desc, const float* fpar, void* const* ptrs);
/* sva_test_step_ops: the bookkeeping kernels of the chunk step (csrc/engine_kernels.h), each through its launcher -- the grid and block size the engine
 * uses.  Whole host arrays; "(io)" arrays go up with the caller's sentinels and come back whole.  Every code, slot, counter capacity and row count a
 * launch would index with is checked against the lengths below first: rc 1 (refused, nothing launched) when such a check or the launcher's own fails,
 * -4 for sizes the hook does not lay out.  int arrays are int32, codes / src / rem int64, everything else float32.
 *   kind 0  ar_prepare_step   desc B, T2, code_off, D, chunk, ci, content rows; ptrs cached_audio_emb [B][D], content_emb, codes [B][T2], last_pos [B],
 *                             x [2 B][D] (io), slot [2 B] (io), pos [2 B] (io), step_content [B][chunk] (io)
 *   kind 1  apply_forced      desc B, ncb, cb, chunk, ci, use_forced; ptrs raw [B][ncb], forced [B][ncb][chunk], tok [B][ncb] (io)
 *   kind 2  ar_finish_frame   desc B, ncb, hist_cap, chunk, ci, last_pos_inc; ptrs tok [B][ncb], last_pos [B] (io), nframes [B] (io), pred_hist [B][ncb][hist_cap] (io),
 *                             step_audio [B][ncb][chunk] (io)
 *   kind 3  append_content    desc B, T2, chunk, hist_cap, counter given; ptrs codes [B][T2], content_hist [B][hist_cap] (io), ncontent [B] (io),
 *                             step_content [B][chunk] (io), step counter [1] (io) or NULL
 *   kind 4  put_codes         desc B, T2, n_per, hist_cap; ptrs src [B][n_per], codes [B][T2] (io), content_hist (io), ncontent (io)
 *   kind 5  build_prompt      desc nspk, R, d, ncb, codebook_size, D, Pmax, content rows, max_delay, rows; ptrs spk [nspk][D], content_emb, codebook_emb
 *                             [ncb codebook_size][D], wait4start [max_delay][D], cc [R], ac [ncb][Pmax], x [rows][D] (io)
 *   kind 6  build_delayfill   desc B, n, d, D, hist_cap, max_delay, content rows; ptrs content_emb, content_hist, ncontent, cached_ref_emb [B][max_delay][D], last_pos,
 *                             slot_list [n], x [n (2 d - 1)][D] (io), slot (io), pos (io), cached_audio_emb [B][D] (io)
 *   kind 7  build_reprefill   desc B, n, d, ncb, codebook_size, D, nspk, hist_cap, max_delay, content rows; ptrs slot [n], Rt [n], nf [n], na [n], ncon [n], content_emb,
 *                             codebook_emb, content_hist, pred_hist, ref_tail [B][ncb][max_delay], x [sum 2 na][D] (io), slot_out (io), pos_out (io)
 *   kind 8  finish_reprefill  desc as kind 7; ptrs slot, Rt, nf, na, ncon, codebook_emb, pred_hist, ref_tail, cached_ref_emb [B][max_delay][D] (io), last_pos [B] (io)
 *   kind 9 / 10  copy_rows / copy_rows2   desc rows, D, src_stride, src_off, len(src); ptrs src, dst [rows][D] (io), (10) dst2 (io)
 *   kind 11 broadcast_row     desc B, bstride, C, len(p), src_row, lo, hi; ptrs p (io)
 *   kind 12 fill_rows         desc B, bstride, C, len(p), rows; ptrs p (io), src [C]
 *   kind 13 .. 16  inc / add_list / add_vec / set_slot_i32   desc len(p), v, (14, 15) n | (16) slot; ptrs p (io), (14) list [n]
 *   kind 17 history_rows_copy desc n_desc, n_slots, slot_lo, to_live, len(buf), len(save), save_bstride, then (offset, bstride, H, C, save offset) per descriptor;
 *                             ptrs buf (io), save (io)
 *   kind 18 history_rows_move desc n_desc, slot, len(src), len(dst), then (source offset, destination offset, destination bstride, H, C) per descriptor; ptrs src, dst (io)
 *   kind 19 put_row           desc table rows, code, D; ptrs table, dst [D] (io)
 *   kind 20 mean3             desc B, y_bstride, len(y), o_bstride, o_off, len(out), n4; ptrs y0, y1, y2, out (io)
 *   kind 21 copy_tokens     desc B, Ht, gap, c, T2, D, tok_bstride, len(tok), d_bstride, len(d2c); ptrs tok, d2c (io) */
int sva_test_step_ops(int device, int kind, const long long* desc, const float* fpar, void* const* ptrs);
/* sva_test_voc_level: launch_voc_level (the fused HiFiGAN level, C = 16 / 32) with the caller's arguments.
 *   desc C, B, Tl, xH, x_bstride, len(X), y_bstride, len(Y), dil0, dil1, dil2, rows_per_frame, frames_done
 *   ptrs X (xH history rows, then Tl rows per stream), Y3[0], Y3[1], Y3[2] (io, len(Y) each), the 18 weights back to back in (branch, conv) order
 *        ([C][k C], k = 3 / 7 / 11 per branch), bias [18][C], int [1] (out): the tile height the launcher chose.  rc 1: the launcher refused. */
int sva_test_voc_level(int device, const long long* desc, const float* fpar, void* const* ptrs);
/* sva_test_voc_conv: launch_voc_conv (voc_conv_kernel: one conv stage of 1..3 ResBlock branches of a narrow HiFiGAN level, C = 16 / 32, over
 * row-major operand planes) once, with the operands made as the engine makes them.
 *   desc 8 ints {C, mode (1 = H3, 2 = H1), B, T (output rows per stream), n members, cu_limit (0 = the device), repeat, 0}, then 16 ints per member
 *        {taps, dil, a_rows_b, a_row0, c_bstride, c_off, len(Cf), r_bstride, r_off, len(res), c_rows_b, c_row0, conv (0: Ap is used as handed in;
 *         1 / 2: rows [conv_row0, conv_row0 + conv_T) of every stream of A are first split into Ap by launch_to_planes_act's row-major arm, 2: of
 *         silu(A)), conv_row0, conv_T, drop (bit 0: the launcher gets no Ap, bit 1: no Wp)}
 *   ptrs {ovf int [1] (io, optional), int [1] (out): 1 when the repeated launch was bit-identical}, then 8 per member
 *        {A fp32 [B][a_rows_b][C] (with conv), Ap uint16 [planes][B a_rows_b C] (io: caller-filled, comes back as the kernel read it), W fp32 [C][taps C]
 *         (K index = tap C + channel), Wp uint16 [planes][C Kp] (out: the packed weight planes, K-blocked; Kp = taps C, at C = 16 padded to whole
 *         32-k blocks), bias [C], res [len(res)] (io), Cf [len(Cf)] (io), Cp uint16 [planes][B c_rows_b C] (io)}; bias, res, Cf, Cp may be NULL = absent
 *   repeat != 0: the launch runs a second time from the same initial Cf / Cp.
 * Returns 0 when it ran; 1 when a row of the launch would lie outside an array (for every stream a_row0 >= 0 and a_row0 + T + (taps - 1) dil <=
 * a_rows_b, likewise the Cf, Cp, res and converted rows) -- nothing was launched -- or when launch_voc_conv itself refused; no array is written back
 * then.  -2 on a HIP error, -4 on arguments the hook cannot lay out. */
int sva_test_voc_conv(int device, const long long* desc, const float* fpar, void* const* ptrs);

/* host cost (microseconds) of enqueueing one kernel from the calling thread, measured over `iters` launches of a one-element
 * kernel into an idle stream.  A synchronous single-stream step is ~170 launches (a pipelined one: four graph launches + the persistent
 * AR kernel), so the enqueueing thread's launch rate still matters for the synchronous mode
 * rate; on a multi-socket host it depends on the core the thread runs on -- see engine.py pin_enqueue_thread() */
int sva_host_launch_cost(int device, int iters, float* us_per_launch);

/* kernel unit-test hook: the nucleus sampler of decode_one (modules/dual_ar_stream.py:1092-1132) over logits[rows][V] with
 * explicit Exp(1) draws noise[rows][V], through one implementation: 1 LDS bitonic sort, 2 register sort, 3/4/5 threshold
 * bisection (workgroup shapes), 6/7 bisection with interpolated, key-snapped probes.  us_out (may be NULL) = average microseconds per launch over `iters` launches */
int sva_test_sampler(int device, int variant, int rows, int V, const float* logits, const float* noise, float temperature,
                     float top_p, int* tok_out, int iters, float* us_out);

/* microbenchmark of the conv-GEMM dispatcher: conv over [B][(taps-1)*dil + T][Cin] -> [B][T][N]; mode bits:
 * 1 GELU, 2 gamma+residual, 4 SiLU-on-load, 8 SwiGLU (w13); returns avg microseconds per launch in out_us[0] */
int sva_bench_gemm(int device, int B, int T, int N, int Cin, int taps, int dil, int mode, int iters, float* out_us);
/* One given plan of the same dispatcher on device-resident random data with `nrot` rotating weight copies (cold weights); kind -1 = the
   dispatcher, 0 / 1 / 2 / 4 = GemmFamily SmallM / Tiled / Ring / Split (csrc/sva_common.h), 6 = the weight-streaming kernel; parameters (a, b, c) as
   in csrc/testhooks.hip.  out[0] = us per launch eager, out[1] = replayed as one graph, out[2] = max |C - C_dispatcher|, out[3] = max |C_dispatcher|. */
int sva_bench_gemm_choice(int device, int B, int T, int N, int Cin, int taps, int dil, int mode, int kind, int a, int b, int c, int nrot, int iters,
                          float* out);

#ifdef __cplusplus
}
#endif
#endif /* SVA_H */
