// Bookkeeping kernels of the per-chunk step (csrc/engine_kernels.hip).  Every kernel has ONE launcher that owns its grid, its block size and
// the argument checks a host can make; engine.hip, stages.hip and the test hook (sva_test_step_ops) all go through it, so what the tests run
// is the production geometry.  A launcher only enqueues on `st` (capturable, no synchronisation); a failed check returns -1 before any launch.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

struct ReprefillArgs {
    int n;
    int slot[128], Rt[128], nf[128], na[128], ncon[128], row_off[129];      // ncon: content codes the slot has seen (per slot: a restarted slot counts from its own start)
};

// ---- one AR frame of the multi-launch decode ----
// rows [2 b, 2 b + 1] of x = [cached_audio_emb[b], content_emb[codes[b][code_off]]] at positions last_pos[b] + 1, + 2; step_content[b][ci] = the code
int launch_ar_prepare_step(const float* cached_audio_emb, const float* content_emb, const long long* codes, int T2, int code_off, const int* last_pos,
                           int D, float* x, int* slot, int* pos, int* step_content, int chunk, int ci, int B, hipStream_t st);
// tok[b][cb] = use_forced ? forced[b][cb][ci] : raw[b][cb]
int launch_apply_forced(const int* raw, const int* forced, const int* use_forced, int chunk, int ci, int cb, int ncb, int* tok, int B, hipStream_t st);
// the frame's codes into the prediction ring at nframes[b] (mod hist_cap) and into step_audio[b][.][ci]; nframes += 1, last_pos += last_pos_inc
int launch_ar_finish_frame(const int* tok, int ncb, int* last_pos, int* nframes, int* pred_hist, int hist_cap, int* step_audio, int chunk, int ci,
                           int B, int last_pos_inc, hipStream_t st);
// the step's `chunk` newest content codes (codes[b][T2 - chunk ..]) into the content ring at ncontent[b] and into step_content; step_counter (may be null) += 1
int launch_append_content(const long long* codes, int T2, int chunk, int* content_hist, int hist_cap, int* ncontent, int* step_content, int B,
                          int* step_counter, hipStream_t st);
// caller-supplied content codes (src [B][n_per]) into codes[b][T2 - n_per ..] and the content ring
int launch_put_codes(const long long* src, int n_per, long long* codes, int T2, int* content_hist, int hist_cap, int* ncontent, int B, hipStream_t st);

// ---- row builders ----
// rows [0, rows) of the prompt sequence (rows <= nspk + 2 R): speaker prefix, then content / audio rows interleaved
int launch_build_prompt(const float* spk, int nspk, const float* content_emb, const float* codebook_emb, const float* wait4start, const int* cc,
                        const int* ac, int Pmax, int R, int d, int ncb, int cbsize, int D, float* x, int rows, hipStream_t st);
// 2 d - 1 rows per listed slot
int launch_build_delayfill(const float* content_emb, const int* content_hist, int hist_cap, const int* ncontent, const float* cached_ref_emb,
                           int max_delay, const int* last_pos, int d, int D, float* x, int* slot, int* pos, float* cached_audio_emb,
                           const int* slot_list, int n, hipStream_t st);
// a.row_off[a.n] rows; refuses a.n outside 1 .. 128, a row_off that is not 2 na per slot, na < d and Rt < d (the first d audio rows of a prompt are
// wait4start rows, which only the whole-prompt prefill builds: SlotBook::one_pass_ok)
int launch_build_reprefill(const ReprefillArgs& a, const float* content_emb, const float* codebook_emb, const int* content_hist, const int* pred_hist,
                           int hist_cap, const int* ref_tail, int max_delay, int d, int ncb, int cbsize, int D, int nspk, float* x, int* slot_out,
                           int* pos_out, hipStream_t st);
int launch_finish_reprefill(const ReprefillArgs& a, const float* codebook_emb, const int* pred_hist, int hist_cap, const int* ref_tail, int max_delay,
                            int d, int ncb, int cbsize, int D, int nspk, float* cached_ref_emb, int* last_pos, hipStream_t st);
// dst [D] = table[code]
int launch_put_row(const float* table, long long code, int D, float* dst, hipStream_t st);

// ---- copies ----
// dst[r] = src[r * src_stride + src_off ..] for r < rows (D floats)
int launch_copy_rows(const float* src, long src_stride, long src_off, float* dst, int D, int rows, hipStream_t st);
int launch_copy_rows2(const float* src, long src_stride, long src_off, float* dst1, float* dst2, int D, int rows, hipStream_t st);
// rows [lo, hi) of every batch item <- row src_row of that item
int launch_broadcast_row(float* p, long bstride, int src_row, int lo, int hi, int C, int B, hipStream_t st);
// rows [0, rows) of every batch item <- src [C]
int launch_fill_rows(float* p, long bstride, int C, const float* src, int rows, int B, hipStream_t st);
// head tokens -> d2c rows [0, Ht); the c newest (behind `gap` rows) -> d2c rows [T2 - c, T2); D a multiple of 4
int launch_copy_tokens(const float* tok, long tok_bstride, int Ht, int gap, int c, float* d2c, long d_bstride, int T2, int D, int B, hipStream_t st);
// out[b][o_off + 4 i ..] = ((y0 + y1) + y2) / 3 over n4 float4 lanes per batch item
int launch_mean3(const float* y0, const float* y1, const float* y2, long y_bstride, float* out, long o_bstride, long o_off, long n4, int B, hipStream_t st);

// ---- counters ----
int launch_inc(int* p, int v, hipStream_t st);
int launch_add_list(int* p, const int* list, int n, int v, hipStream_t st);
int launch_add_vec(int* p, int n, int v, hipStream_t st);
int launch_set_slot_i32(int* p, int slot, int v, hipStream_t st);

// ---- vocoder history rows (ShiftDesc tables) ----
// slots [slot_lo, slot_lo + n_slots): live rows -> save (to_live == 0) or back
int launch_history_rows_copy(const sva::ShiftDesc* descs, int n_desc, const long* offs, float* save, long save_bstride, int slot_lo, int n_slots,
                             int to_live, hipStream_t st);
// slot 0 of the source table -> slot `slot` of the parallel destination table
int launch_history_rows_move(const sva::ShiftDesc* src_descs, const sva::ShiftDesc* dst_descs, int n_desc, int slot, hipStream_t st);
