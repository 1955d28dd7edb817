// Bookkeeping kernels of the per-chunk step: frame preparation / completion of the multi-launch AR decode, content and prediction
// history rings, prompt / delay-fill / re-prefill row builders (modules/dual_ar_stream.py:764-837, evaluations/infer_arvc.py:547-564).
#include "engine_kernels.h"

// small device helpers that live here because they touch the batch control block -------------------------
__global__ void ar_prepare_step_kernel(const float* __restrict__ cached_audio_emb, const float* __restrict__ content_emb,
                                       const long long* __restrict__ codes, int T2, int code_off, const int* __restrict__ last_pos,
                                       int D, float* __restrict__ x, int* __restrict__ slot, int* __restrict__ pos,
                                       int* __restrict__ step_content, int chunk, int ci) {
    // decode_one (dual_ar_stream.py:817-837): tokens [cached_new_audio_emb, src_cond] at (last+1, last+2)
    const int b = blockIdx.x;
    const int code = (int)codes[(long)b * T2 + code_off];
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
        x[((long)b * 2) * D + i] = cached_audio_emb[(long)b * D + i];
        x[((long)b * 2 + 1) * D + i] = content_emb[(long)code * D + i];
    }
    if (threadIdx.x == 0) {
        slot[2 * b] = b; slot[2 * b + 1] = b;
        pos[2 * b] = last_pos[b] + 1; pos[2 * b + 1] = last_pos[b] + 2;
        step_content[b * chunk + ci] = code;
    }
}

__global__ void copy_rows_kernel(const float* __restrict__ src, long src_stride, long src_off, float* __restrict__ dst, int D) {
    const int r = blockIdx.x;
    for (int i = threadIdx.x; i < D; i += blockDim.x) dst[(long)r * D + i] = src[(long)r * src_stride + src_off + i];
}

__global__ void copy_rows2_kernel(const float* __restrict__ src, long src_stride, long src_off, float* __restrict__ dst1,
                                  float* __restrict__ dst2, int D) {
    const int r = blockIdx.x;
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
        const float v = src[(long)r * src_stride + src_off + i];
        dst1[(long)r * D + i] = v;
        dst2[(long)r * D + i] = v;
    }
}

__global__ void apply_forced_kernel(const int* __restrict__ raw, const int* __restrict__ forced, const int* __restrict__ use_forced,
                                    int chunk, int ci, int cb, int ncb, int* __restrict__ tok, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int t = raw[b * ncb + cb];
    if (*use_forced) t = forced[((long)b * ncb + cb) * chunk + ci];
    tok[b * ncb + cb] = t;
}

__global__ void ar_finish_frame_kernel(const int* __restrict__ tok, int ncb, int* __restrict__ last_pos, int* __restrict__ nframes,
                                       int* __restrict__ pred_hist, int hist_cap, int* __restrict__ step_audio, int chunk, int ci,
                                       const long long* __restrict__ codes, int T2, int code_off, int* __restrict__ content_hist,
                                       int* __restrict__ ncontent, int B, int last_pos_inc) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int f = nframes[b];
    for (int i = 0; i < ncb; ++i) {
        const int t = tok[b * ncb + i];
        pred_hist[((long)b * ncb + i) * hist_cap + (f & (hist_cap - 1))] = t;     // ring (hist_cap is a power of two)
        step_audio[((long)b * ncb + i) * chunk + ci] = t;
    }
    nframes[b] = f + 1;
    last_pos[b] += last_pos_inc;
}

__global__ void append_content_kernel(const long long* __restrict__ codes, int T2, int chunk, int* __restrict__ content_hist,
                                      int hist_cap, int* __restrict__ ncontent, int* __restrict__ step_content, int B,
                                      int* __restrict__ step_counter) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0 && step_counter) *step_counter += 1;          // the chunk counter (ring position) advances with the step
    if (b >= B) return;
    const int n = ncontent[b];
    for (int i = 0; i < chunk; ++i) {
        const int code = (int)codes[(long)b * T2 + T2 - chunk + i];
        content_hist[(long)b * hist_cap + ((n + i) & (hist_cap - 1))] = code;
        step_content[b * chunk + i] = code;
    }
    ncontent[b] = n + chunk;
}

// dst rows [lo, hi) of every batch item <- row `src_row`
__global__ void broadcast_row_kernel(float* p, long bstride, int src_row, int lo, int hi, int C) {
    float* base = p + (long)blockIdx.y * bstride;
    const int r = lo + blockIdx.x;
    if (r >= hi || r == src_row) return;
    for (int i = threadIdx.x; i < C; i += blockDim.x) base[(long)r * C + i] = base[(long)src_row * C + i];
}

// rows [0, gridDim.x) of every batch item <- one source row
__global__ void fill_rows_kernel(float* p, long bstride, int C, const float* __restrict__ src) {
    float* dst = p + (long)blockIdx.y * bstride + (long)blockIdx.x * C;
    for (int i = threadIdx.x; i < C; i += blockDim.x) dst[i] = src[i];
}

__global__ void inc_kernel(int* p, int v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *p += v;
}

// prompt sequence builder (DualARWrapper.prefill_prompt, dual_ar_stream.py:764-796, layout in SURVEY.md A.1):
//   rows 0..32 = speaker prefix; then for i < R: row 33+2i = content_emb[cc[i]],
//   row 34+2i = (i < d ? wait4start[i] : audio_embed(ac[:, i-d]))
__global__ void build_prompt_kernel(const float* __restrict__ spk, int nspk, const float* __restrict__ content_emb,
                                    const float* __restrict__ codebook_emb, const float* __restrict__ wait4start,
                                    const int* __restrict__ cc, const int* __restrict__ ac, int Pmax, int R, int d, int ncb,
                                    int cbsize, int D, float* __restrict__ x) {
    const int r = blockIdx.x;
    float* o = x + (long)r * D;
    if (r < nspk) {
        for (int i = threadIdx.x; i < D; i += blockDim.x) o[i] = spk[(long)r * D + i];
        return;
    }
    const int i = (r - nspk) >> 1;
    if (((r - nspk) & 1) == 0) {
        const float* s = content_emb + (long)cc[i] * D;
        for (int k = threadIdx.x; k < D; k += blockDim.x) o[k] = s[k];
    } else if (i < d) {
        const float* s = wait4start + (long)i * D;
        for (int k = threadIdx.x; k < D; k += blockDim.x) o[k] = s[k];
    } else {
        for (int k = threadIdx.x; k < D; k += blockDim.x) {
            float acc = 0.f;
            for (int q = 0; q < ncb; ++q) acc += codebook_emb[((long)ac[(long)q * Pmax + i - d] + (long)q * cbsize) * D + k];
            o[k] = acc;
        }
    }
}

// delay fill (prefill_src_condition4delay, dual_ar_stream.py:798-815): per slot the interleave
// [c_0, r_0, c_1, r_1, ..., c_{d-1}] (2d-1 rows; the dropped last row r_{d-1} becomes cached_new_audio_emb)
__global__ void build_delayfill_kernel(const float* __restrict__ content_emb, const int* __restrict__ content_hist, int hist_cap,
                                       const int* __restrict__ ncontent, const float* __restrict__ cached_ref_emb, int max_delay,
                                       const int* __restrict__ last_pos, int d, int D, float* __restrict__ x, int* __restrict__ slot,
                                       int* __restrict__ pos, float* __restrict__ cached_audio_emb, const int* __restrict__ slot_list) {
    const int rows = 2 * d - 1;
    const int li = blockIdx.x / rows, r = blockIdx.x % rows;
    const int b = slot_list[li];
    const int i = r >> 1;
    float* o = x + ((long)li * rows + r) * D;
    if ((r & 1) == 0) {
        const int code = content_hist[(long)b * hist_cap + ((ncontent[b] - d + i) & (hist_cap - 1))];
        for (int k = threadIdx.x; k < D; k += blockDim.x) o[k] = content_emb[(long)code * D + k];
    } else {
        for (int k = threadIdx.x; k < D; k += blockDim.x) o[k] = cached_ref_emb[((long)b * max_delay + i) * D + k];
    }
    if (r == 0)
        for (int k = threadIdx.x; k < D; k += blockDim.x)
            cached_audio_emb[(long)b * D + k] = cached_ref_emb[((long)b * max_delay + d - 1) * D + k];
    if (threadIdx.x == 0) {
        slot[li * rows + r] = b;
        pos[li * rows + r] = last_pos[b] + 1 + r;
    }
}
// Re-prefill of the due slots of a batch in ONE pass (infer_arvc.py:547-564: prompt <- [ref (truncated), last buffer_frames predicted
// frames] / [ref content, src content[-buffer-d:-d]]).  The attention is causal, so the K / V rows of the reference part of that prompt
// -- positions 0 .. 32 + 2 Rt -- are the ones the slot's cache has held since its first prefill: only the 2 na rows of the appended
// frames are new.  They are built here from the device-resident history rings (no host round trip) for every due slot and then run
// through the layers as one (sum of rows)-row pass against the cached prefix.  Row layout per slot, i = Rt .. Rt + na - 1:
//   position 33 + 2 i = content_emb[content_hist[c_lo + i - Rt]],  34 + 2 i = audio_embed(ac'[:, i - d]),
//   ac'[:, j] = ref_audio[:, j] for j < Rt (the last d reference frames: ref_tail) and pred_hist[nf - na + j - Rt] beyond.
__global__ void build_reprefill_kernel(const ReprefillArgs a, const float* __restrict__ content_emb, const float* __restrict__ codebook_emb,
                                       const int* __restrict__ content_hist, const int* __restrict__ pred_hist, int hist_cap,
                                       const int* __restrict__ ref_tail, int max_delay, int d, int ncb, int cbsize, int D, int nspk,
                                       float* __restrict__ x, int* __restrict__ slot_out, int* __restrict__ pos_out) {
    const int row = blockIdx.x;
    int li = 0;
    while (li + 1 < a.n && row >= a.row_off[li + 1]) ++li;
    const int r = row - a.row_off[li], b = a.slot[li], Rt = a.Rt[li], nf = a.nf[li], na = a.na[li];
    const int i = Rt + (r >> 1);
    float* o = x + (long)row * D;
    const int mask = hist_cap - 1;
    if ((r & 1) == 0) {
        const int c_lo = a.ncon[li] - d - na;                      // src_content_codes[-buffer-d:-d]
        const int code = content_hist[(long)b * hist_cap + ((c_lo + (i - Rt)) & mask)];
        for (int k = threadIdx.x; k < D; k += blockDim.x) o[k] = content_emb[(long)code * D + k];
    } else {
        const int j = i - d;                                     // frame of the concatenated audio codes
        int code[8];
        for (int q = 0; q < ncb; ++q)
            code[q] = j < Rt ? ref_tail[((long)b * ncb + q) * max_delay + (max_delay - (Rt - j))]
                             : pred_hist[((long)b * ncb + q) * hist_cap + ((nf - na + (j - Rt)) & mask)];
        for (int k = threadIdx.x; k < D; k += blockDim.x) {
            float acc = 0.f;
            for (int q = 0; q < ncb; ++q) acc += codebook_emb[((long)code[q] + (long)q * cbsize) * D + k];      // codebooks summed in order (build_prompt_kernel)
            o[k] = acc;
        }
    }
    if (threadIdx.x == 0) {
        slot_out[row] = b;
        pos_out[row] = nspk + 2 * Rt + r;
    }
}
// cached_ref_emb = embed(ac')[-d:] of the new prompt (dual_ar_stream.py:775) and last_pos = its last position, per due slot
__global__ void finish_reprefill_kernel(const ReprefillArgs a, const float* __restrict__ codebook_emb, const int* __restrict__ pred_hist, int hist_cap,
                                        const int* __restrict__ ref_tail, int max_delay, int d, int ncb, int cbsize, int D, int nspk,
                                        float* __restrict__ cached_ref_emb, int* __restrict__ last_pos) {
    const int li = blockIdx.x / d, jj = blockIdx.x % d;
    const int b = a.slot[li], Rt = a.Rt[li], nf = a.nf[li], na = a.na[li];
    const int j = Rt + na - d + jj;
    const int mask = hist_cap - 1;
    int code[8];
    for (int q = 0; q < ncb; ++q)
        code[q] = j < Rt ? ref_tail[((long)b * ncb + q) * max_delay + (max_delay - (Rt - j))]
                         : pred_hist[((long)b * ncb + q) * hist_cap + ((nf - na + (j - Rt)) & mask)];
    for (int k = threadIdx.x; k < D; k += blockDim.x) {
        float acc = 0.f;
        for (int q = 0; q < ncb; ++q) acc += codebook_emb[((long)code[q] + (long)q * cbsize) * D + k];
        cached_ref_emb[((long)b * max_delay + jj) * D + k] = acc;
    }
    if (jj == 0 && threadIdx.x == 0) last_pos[b] = nspk + 2 * (Rt + na) - 1;
}

__global__ void add_list_kernel(int* p, const int* list, int n, int v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[list[i]] += v;
}
__global__ void add_vec_kernel(int* p, int n, int v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] += v;
}
__global__ void set_slot_i32_kernel(int* p, int slot, int v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) p[slot] = v;
}

// The streaming state of the vocoder is the H history rows in front of every tensor of its ShiftDesc table: desc blockIdx.x, slot slot_lo +
// blockIdx.y, H * C floats at ptr + slot * bstride <-> save + slot * save_bstride + offs[desc].  The K-blocked operand planes are in that
// table as one desc per (plane, 32-k block) -- [k / 32][B rows][32], plane_off_blocked of planes_split.h -- so a slot's rows of such a
// plane are reached through the same (ptr, bstride) pairs that shift them, never through one pointer offset into the plane.
__global__ __launch_bounds__(256) void history_rows_copy_kernel(const sva::ShiftDesc* __restrict__ descs, const long* __restrict__ offs,
                                                                float* __restrict__ save, long save_bstride, int slot_lo, int to_live) {
    const sva::ShiftDesc d = descs[blockIdx.x];
    const int slot = slot_lo + blockIdx.y;
    float* live = d.ptr + (long)slot * d.bstride;
    float* sv = save + (long)slot * save_bstride + offs[blockIdx.x];
    const long n = (long)d.H * d.C;
    if (to_live) for (long i = threadIdx.x; i < n; i += blockDim.x) live[i] = sv[i];
    else for (long i = threadIdx.x; i < n; i += blockDim.x) sv[i] = live[i];
}

// Slot-local activation: the H history rows of every desc, from slot 0 of a one-stream workspace's table into slot `slot` of the batch's
// table.  The two tables are parallel (same count, same H and C per entry: checked when the workspace is created), so desc blockIdx.x of
// one is desc blockIdx.x of the other and the K-blocked planes are reached per (plane, 32-k block) as above.  Writes the target slot's
// rows only.  float4 lanes where the block's length and both addresses allow.
__global__ __launch_bounds__(256) void history_rows_move_kernel(const sva::ShiftDesc* __restrict__ src_descs, const sva::ShiftDesc* __restrict__ dst_descs,
                                                                int slot) {
    const sva::ShiftDesc s = src_descs[blockIdx.x], d = dst_descs[blockIdx.x];
    const float* from = s.ptr;
    float* to = d.ptr + (long)slot * d.bstride;
    const long n = (long)d.H * d.C;
    if (n % 4 == 0 && ((reinterpret_cast<uintptr_t>(from) | reinterpret_cast<uintptr_t>(to)) & 15) == 0) {
        const float4* f4 = reinterpret_cast<const float4*>(from);
        float4* t4 = reinterpret_cast<float4*>(to);
        for (long i = threadIdx.x; i < n / 4; i += blockDim.x) t4[i] = f4[i];
    } else {
        for (long i = threadIdx.x; i < n; i += blockDim.x) to[i] = from[i];
    }
}

// ---- kernels of the AR seams, the offline loop and the stage hand-overs (launched from engine.hip / stages.hip through the launchers below) ----
__global__ void put_codes_kernel(const long long* __restrict__ src, int n_per, long long* __restrict__ codes, int T2, int* __restrict__ content_hist,
                                 int hist_cap, int* __restrict__ ncontent, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int n = ncontent[b];
    for (int i = 0; i < n_per; ++i) {
        const long long c = src[(long)b * n_per + i];
        codes[(long)b * T2 + T2 - n_per + i] = c;
        content_hist[(long)b * hist_cap + ((n + i) & (hist_cap - 1))] = (int)c;
    }
    ncontent[b] = n + n_per;
}

__global__ void put_row_kernel(const float* __restrict__ table, long long code, int D, float* __restrict__ dst) {
    for (int i = threadIdx.x; i < D; i += blockDim.x) dst[i] = table[code * D + i];
}

__global__ void mean3_kernel(const float* __restrict__ y0, const float* __restrict__ y1, const float* __restrict__ y2, long y_bstride,
                             float* __restrict__ out, long o_bstride, long o_off, long n4) {
    // ParallelBlock: torch.stack([...]).mean(0) (firefly.py:214-215) of the three branch outputs, float4 lanes
    const int b = blockIdx.y;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4 a = reinterpret_cast<const float4*>(y0 + (long)b * y_bstride)[i];
    const float4 c = reinterpret_cast<const float4*>(y1 + (long)b * y_bstride)[i];
    const float4 d = reinterpret_cast<const float4*>(y2 + (long)b * y_bstride)[i];
    float4 r;
    r.x = ((a.x + c.x) + d.x) / 3.0f; r.y = ((a.y + c.y) + d.y) / 3.0f; r.z = ((a.z + c.z) + d.z) / 3.0f; r.w = ((a.w + c.w) + d.w) / 3.0f;
    reinterpret_cast<float4*>(out + (long)b * o_bstride + o_off)[i] = r;
}

__global__ void copy_tokens_kernel(const float* __restrict__ tok, long tok_bstride, int Ht, int gap, int c, float* __restrict__ d2c, long d_bstride,
                                   int T2, int D) {
    // head tokens -> d2c rows [0, Ht); newest c tokens -> d2c rows [T2 - c, T2)
    const int r = blockIdx.x, bi = blockIdx.y;
    const int src = r < Ht ? r : Ht + gap + (r - Ht);
    const int dst = r < Ht ? r : T2 - c + (r - Ht);
    const float4* s = reinterpret_cast<const float4*>(tok + (long)bi * tok_bstride + (long)src * D);
    float4* d = reinterpret_cast<float4*>(d2c + (long)bi * d_bstride + (long)dst * D);
    for (int i = threadIdx.x; i < D / 4; i += blockDim.x) d[i] = s[i];
}

// ============================================================================================
// launchers: grid, block and the host-checkable arguments of every kernel above, in one place each
// ============================================================================================
namespace {
inline bool pow2(int v) { return v >= 1 && (v & (v - 1)) == 0; }
inline unsigned per_slot_blocks(int B) { return (unsigned)((B + 63) / 64); }          // the one-thread-per-slot kernels: 64 slots a block
}  // namespace

int launch_ar_prepare_step(const float* cached_audio_emb, const float* content_emb, const long long* codes, int T2, int code_off, const int* last_pos,
                           int D, float* x, int* slot, int* pos, int* step_content, int chunk, int ci, int B, hipStream_t st) {
    SVA_CHECK(B >= 1 && D >= 1 && code_off >= 0 && code_off < T2 && ci >= 0 && ci < chunk, "ar_prepare_step: bad arguments");
    hipLaunchKernelGGL(ar_prepare_step_kernel, dim3(B), dim3(256), 0, st, cached_audio_emb, content_emb, codes, T2, code_off, last_pos, D, x, slot, pos,
                       step_content, chunk, ci);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_apply_forced(const int* raw, const int* forced, const int* use_forced, int chunk, int ci, int cb, int ncb, int* tok, int B, hipStream_t st) {
    SVA_CHECK(B >= 1 && cb >= 0 && cb < ncb && ci >= 0 && ci < chunk, "apply_forced: bad arguments");
    hipLaunchKernelGGL(apply_forced_kernel, dim3(per_slot_blocks(B)), dim3(64), 0, st, raw, forced, use_forced, chunk, ci, cb, ncb, tok, B);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_ar_finish_frame(const int* tok, int ncb, int* last_pos, int* nframes, int* pred_hist, int hist_cap, int* step_audio, int chunk, int ci,
                           int B, int last_pos_inc, hipStream_t st) {
    SVA_CHECK(B >= 1 && ncb >= 1 && pow2(hist_cap) && ci >= 0 && ci < chunk, "ar_finish_frame: bad arguments (the history capacity is a power of two)");
    hipLaunchKernelGGL(ar_finish_frame_kernel, dim3(per_slot_blocks(B)), dim3(64), 0, st, tok, ncb, last_pos, nframes, pred_hist, hist_cap, step_audio, chunk,
                       ci, (const long long*)nullptr, 0, 0, (int*)nullptr, (int*)nullptr, B, last_pos_inc);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_append_content(const long long* codes, int T2, int chunk, int* content_hist, int hist_cap, int* ncontent, int* step_content, int B,
                          int* step_counter, hipStream_t st) {
    SVA_CHECK(B >= 1 && chunk >= 1 && chunk <= T2 && pow2(hist_cap) && chunk <= hist_cap, "append_content: bad arguments (the history capacity is a power of two)");
    hipLaunchKernelGGL(append_content_kernel, dim3(per_slot_blocks(B)), dim3(64), 0, st, codes, T2, chunk, content_hist, hist_cap, ncontent, step_content, B,
                       step_counter);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_put_codes(const long long* src, int n_per, long long* codes, int T2, int* content_hist, int hist_cap, int* ncontent, int B, hipStream_t st) {
    SVA_CHECK(B >= 1 && n_per >= 1 && n_per <= T2 && pow2(hist_cap) && n_per <= hist_cap, "put_codes: bad arguments (the history capacity is a power of two)");
    hipLaunchKernelGGL(put_codes_kernel, dim3(per_slot_blocks(B)), dim3(64), 0, st, src, n_per, codes, T2, content_hist, hist_cap, ncontent, B);
    SVA_HIP(hipGetLastError());
    return 0;
}

int launch_build_prompt(const float* spk, int nspk, const float* content_emb, const float* codebook_emb, const float* wait4start, const int* cc,
                        const int* ac, int Pmax, int R, int d, int ncb, int cbsize, int D, float* x, int rows, hipStream_t st) {
    SVA_CHECK(rows >= 1 && rows <= nspk + 2 * R && nspk >= 0 && d >= 1 && R <= Pmax && ncb >= 1 && D >= 1, "build_prompt: bad arguments");
    hipLaunchKernelGGL(build_prompt_kernel, dim3(rows), dim3(256), 0, st, spk, nspk, content_emb, codebook_emb, wait4start, cc, ac, Pmax, R, d, ncb, cbsize, D, x);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_build_delayfill(const float* content_emb, const int* content_hist, int hist_cap, const int* ncontent, const float* cached_ref_emb,
                           int max_delay, const int* last_pos, int d, int D, float* x, int* slot, int* pos, float* cached_audio_emb,
                           const int* slot_list, int n, hipStream_t st) {
    SVA_CHECK(n >= 1 && d >= 1 && d <= max_delay && d <= hist_cap && pow2(hist_cap) && D >= 1, "build_delayfill: bad arguments (the history capacity is a power of two)");
    hipLaunchKernelGGL(build_delayfill_kernel, dim3(n * (2 * d - 1)), dim3(256), 0, st, content_emb, content_hist, hist_cap, ncontent, cached_ref_emb, max_delay,
                       last_pos, d, D, x, slot, pos, cached_audio_emb, slot_list);
    SVA_HIP(hipGetLastError());
    return 0;
}
namespace {
int check_reprefill_args(const ReprefillArgs& a, int hist_cap, int max_delay, int d, int ncb) {
    SVA_CHECK(a.n >= 1 && a.n <= 128, "re-prefill: 1 .. 128 slots per pass");
    SVA_CHECK(ncb >= 1 && ncb <= 8 && d >= 1 && d <= max_delay && pow2(hist_cap), "re-prefill: bad arguments (at most 8 codebooks, a power-of-two history capacity)");
    SVA_CHECK(a.row_off[0] == 0, "re-prefill: row offsets start at 0");
    for (int i = 0; i < a.n; ++i) {
        SVA_CHECK(a.row_off[i + 1] == a.row_off[i] + 2 * a.na[i], "re-prefill: row offsets are the running sum of 2 na");
        SVA_CHECK(a.na[i] >= d && a.na[i] <= a.nf[i] && a.na[i] + d <= a.ncon[i] && a.na[i] + d <= hist_cap, "re-prefill: the appended frames lie inside the histories (d <= na <= nf, na + d <= ncontent)");
        SVA_CHECK(a.Rt[i] >= d, "re-prefill: a stored prompt shorter than the delay needs the whole-prompt prefill (its wait4start rows)");
    }
    return 0;
}
}  // namespace
int launch_build_reprefill(const ReprefillArgs& a, const float* content_emb, const float* codebook_emb, const int* content_hist, const int* pred_hist,
                           int hist_cap, const int* ref_tail, int max_delay, int d, int ncb, int cbsize, int D, int nspk, float* x, int* slot_out,
                           int* pos_out, hipStream_t st) {
    SVA_TRY_RC(check_reprefill_args(a, hist_cap, max_delay, d, ncb));
    hipLaunchKernelGGL(build_reprefill_kernel, dim3(a.row_off[a.n]), dim3(256), 0, st, a, content_emb, codebook_emb, content_hist, pred_hist, hist_cap, ref_tail,
                       max_delay, d, ncb, cbsize, D, nspk, x, slot_out, pos_out);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_finish_reprefill(const ReprefillArgs& a, const float* codebook_emb, const int* pred_hist, int hist_cap, const int* ref_tail, int max_delay,
                            int d, int ncb, int cbsize, int D, int nspk, float* cached_ref_emb, int* last_pos, hipStream_t st) {
    SVA_TRY_RC(check_reprefill_args(a, hist_cap, max_delay, d, ncb));
    hipLaunchKernelGGL(finish_reprefill_kernel, dim3(a.n * d), dim3(256), 0, st, a, codebook_emb, pred_hist, hist_cap, ref_tail, max_delay, d, ncb, cbsize, D,
                       nspk, cached_ref_emb, last_pos);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_put_row(const float* table, long long code, int D, float* dst, hipStream_t st) {
    SVA_CHECK(code >= 0 && D >= 1, "put_row: bad arguments");
    hipLaunchKernelGGL(put_row_kernel, dim3(1), dim3(256), 0, st, table, code, D, dst);
    SVA_HIP(hipGetLastError());
    return 0;
}

int launch_copy_rows(const float* src, long src_stride, long src_off, float* dst, int D, int rows, hipStream_t st) {
    SVA_CHECK(rows >= 1 && D >= 1 && src_stride >= 0 && src_off >= 0, "copy_rows: bad arguments");
    hipLaunchKernelGGL(copy_rows_kernel, dim3(rows), dim3(256), 0, st, src, src_stride, src_off, dst, D);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_copy_rows2(const float* src, long src_stride, long src_off, float* dst1, float* dst2, int D, int rows, hipStream_t st) {
    SVA_CHECK(rows >= 1 && D >= 1 && src_stride >= 0 && src_off >= 0, "copy_rows2: bad arguments");
    hipLaunchKernelGGL(copy_rows2_kernel, dim3(rows), dim3(256), 0, st, src, src_stride, src_off, dst1, dst2, D);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_broadcast_row(float* p, long bstride, int src_row, int lo, int hi, int C, int B, hipStream_t st) {
    SVA_CHECK(B >= 1 && B <= 65535 && C >= 1 && lo >= 0 && hi > lo && src_row >= 0, "broadcast_row: bad arguments");
    hipLaunchKernelGGL(broadcast_row_kernel, dim3(hi - lo, B), dim3(256), 0, st, p, bstride, src_row, lo, hi, C);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_fill_rows(float* p, long bstride, int C, const float* src, int rows, int B, hipStream_t st) {
    SVA_CHECK(B >= 1 && B <= 65535 && C >= 1 && rows >= 0, "fill_rows: bad arguments");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(fill_rows_kernel, dim3(rows, B), dim3(128), 0, st, p, bstride, C, src);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_copy_tokens(const float* tok, long tok_bstride, int Ht, int gap, int c, float* d2c, long d_bstride, int T2, int D, int B, hipStream_t st) {
    SVA_CHECK(B >= 1 && B <= 65535 && Ht >= 0 && gap >= 0 && c >= 1 && Ht + c <= T2 && D >= 4 && D % 4 == 0 && tok_bstride % 4 == 0 && d_bstride % 4 == 0,
              "copy_tokens: bad arguments (float4 rows; head and newest tokens do not overlap)");
    hipLaunchKernelGGL(copy_tokens_kernel, dim3(Ht + c, B), dim3(128), 0, st, tok, tok_bstride, Ht, gap, c, d2c, d_bstride, T2, D);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_mean3(const float* y0, const float* y1, const float* y2, long y_bstride, float* out, long o_bstride, long o_off, long n4, int B, hipStream_t st) {
    SVA_CHECK(B >= 1 && B <= 65535 && n4 >= 1 && y_bstride % 4 == 0 && o_bstride % 4 == 0 && o_off >= 0 && o_off % 4 == 0, "mean3: bad arguments (float4 lanes)");
    hipLaunchKernelGGL(mean3_kernel, dim3((unsigned)((n4 + 255) / 256), B), dim3(256), 0, st, y0, y1, y2, y_bstride, out, o_bstride, o_off, n4);
    SVA_HIP(hipGetLastError());
    return 0;
}

int launch_inc(int* p, int v, hipStream_t st) {
    hipLaunchKernelGGL(inc_kernel, dim3(1), dim3(64), 0, st, p, v);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_add_list(int* p, const int* list, int n, int v, hipStream_t st) {
    SVA_CHECK(n >= 1, "add_list: bad arguments");
    hipLaunchKernelGGL(add_list_kernel, dim3(per_slot_blocks(n)), dim3(64), 0, st, p, list, n, v);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_add_vec(int* p, int n, int v, hipStream_t st) {
    SVA_CHECK(n >= 1, "add_vec: bad arguments");
    hipLaunchKernelGGL(add_vec_kernel, dim3(per_slot_blocks(n)), dim3(64), 0, st, p, n, v);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_set_slot_i32(int* p, int slot, int v, hipStream_t st) {
    SVA_CHECK(slot >= 0, "set_slot_i32: bad arguments");
    hipLaunchKernelGGL(set_slot_i32_kernel, dim3(1), dim3(64), 0, st, p, slot, v);
    SVA_HIP(hipGetLastError());
    return 0;
}

int launch_history_rows_copy(const sva::ShiftDesc* descs, int n_desc, const long* offs, float* save, long save_bstride, int slot_lo, int n_slots,
                             int to_live, hipStream_t st) {
    SVA_CHECK(n_desc >= 0 && slot_lo >= 0 && n_slots >= 1 && n_slots <= 65535 && save_bstride >= 0, "history_rows_copy: bad arguments");
    if (n_desc == 0) return 0;
    hipLaunchKernelGGL(history_rows_copy_kernel, dim3(n_desc, n_slots), dim3(256), 0, st, descs, offs, save, save_bstride, slot_lo, to_live);
    SVA_HIP(hipGetLastError());
    return 0;
}
int launch_history_rows_move(const sva::ShiftDesc* src_descs, const sva::ShiftDesc* dst_descs, int n_desc, int slot, hipStream_t st) {
    SVA_CHECK(n_desc >= 0 && slot >= 0, "history_rows_move: bad arguments");
    if (n_desc == 0) return 0;
    hipLaunchKernelGGL(history_rows_move_kernel, dim3(n_desc), dim3(256), 0, st, src_descs, dst_descs, slot);
    SVA_HIP(hipGetLastError());
    return 0;
}
