"""Cases of test_gpu_step_ops.py: the bookkeeping kernels of the chunk step (csrc/engine_kernels.hip) and the fused HiFiGAN level (csrc/voc_fused.hip).
A case is a dict: op (a key of engine.STEP_OPS), id, desc and arrays as sva_test_step_ops takes them (include/sva.h), io (indices of the arrays the
kernel may write: they go up carrying sentinels and come back whole) and want (index -> the whole expected array, from tests/kernel_refs.py: untouched
entries keep their sentinel).  `validate` restates, in Python, everything a launch indexes with; tests/test_kernel_refs.py runs it over every generator
on the CPU, so no case can ask a kernel for an entry outside its arrays, and every re-prefill case has na >= d.

Shapes are the smallest at which a kernel can still go wrong: ring capacities of 16 and 64 with the counters placed around their multiples, 1 / 3 / 65
slots (65 crosses the 64-thread block of the one-thread-per-slot kernels), D = 1024 and a D that is no multiple of the 256-thread block."""
import numpy as np

import kernel_refs as R

F32, I32, I64 = np.float32, np.int32, np.int64
SENT, ISENT = F32(777.0), -7
NC, CBS, MD = 50, 20, 8          # content table rows, codebook size, max_delay
CAPS, BS = (16, 64), (1, 3, 65)
PLACEMENTS = ("ends before a multiple", "ends on a multiple", "straddles a multiple", "several multiples above")
# the arrays of every kind, in the order sva_test_step_ops takes them (include/sva.h)
ARRAYS = {
    "ar_prepare_step": ("cached_audio_emb", "content_emb", "codes", "last_pos", "x", "slot", "pos", "step_content"),
    "apply_forced": ("raw", "forced", "tok"),
    "ar_finish_frame": ("tok", "last_pos", "nframes", "pred_hist", "step_audio"),
    "append_content": ("codes", "content_hist", "ncontent", "step_content", "step_counter"),
    "put_codes": ("src", "codes", "content_hist", "ncontent"),
    "build_prompt": ("spk", "content_emb", "codebook_emb", "wait4start", "cc", "ac", "x"),
    "build_delayfill": ("content_emb", "content_hist", "ncontent", "cached_ref_emb", "last_pos", "slot_list", "x", "slot", "pos", "cached_audio_emb"),
    "build_reprefill": ("slot", "Rt", "nf", "na", "ncon", "content_emb", "codebook_emb", "content_hist", "pred_hist", "ref_tail", "x", "slot_out", "pos_out"),
    "finish_reprefill": ("slot", "Rt", "nf", "na", "ncon", "codebook_emb", "pred_hist", "ref_tail", "cached_ref_emb", "last_pos"),
    "copy_rows": ("src", "dst"), "copy_rows2": ("src", "dst1", "dst2"), "broadcast_row": ("p",), "fill_rows": ("p", "src"),
    "inc": ("p",), "add_list": ("p", "list"), "add_vec": ("p",), "set_slot_i32": ("p",),
    "history_rows_copy": ("live", "save"), "history_rows_move": ("src", "dst"), "put_row": ("table", "dst"),
    "mean3": ("y0", "y1", "y2", "out"), "copy_tokens": ("tok", "d2c"),
}


def counter_at(cap, n, placement, k=1):
    """a counter c such that the n entries [c, c + n) end before / on / across the multiple k cap, or lie several multiples above it"""
    return {0: k * cap - n - 1, 1: k * cap - n, 2: k * cap - max(n // 2, 1) if n > 1 else k * cap, 3: (k + 4) * cap + 3}[placement]


def counters(cap, B, n, p):
    """per slot: the placements rotate over the slots from p, on rising multiples of the capacity"""
    return np.array([counter_at(cap, n, (p + b) % 4, 1 + b // 4 % 3) for b in range(B)], I32)


def _tables(rng, D, ncb):
    return (rng.standard_normal((NC, D)).astype(F32), rng.standard_normal((ncb * CBS, D)).astype(F32), rng.standard_normal((MD, D)).astype(F32))


def _case(op, cid, desc, arrays, io, want):
    arrays = [None if a is None else np.ascontiguousarray(a) for a in arrays]
    return dict(op=op, id="%s %s" % (op, cid), desc=[int(v) for v in desc], arrays=arrays, io=tuple(io),
                want={i: np.ascontiguousarray(w, dtype=arrays[i].dtype).reshape(arrays[i].shape) for i, w in want.items()})


# ---- rings -------------------------------------------------------------------------------------------------------------------------------------
def ring_cases():
    out = []
    for cap in CAPS:
        for B in BS:
            for p in range(4):
                rng = np.random.default_rng(1000 * cap + 10 * B + p)
                tag = "cap %d B %d %s" % (cap, B, PLACEMENTS[p])
                # ar_finish_frame: one entry per codebook at nframes mod cap
                ncb, chunk, ci = (8, 3, 1) if p % 2 == 0 else (1, 1, 0)
                tok = rng.integers(0, CBS, (B, ncb)).astype(I32)
                nfr, lp = counters(cap, B, 1, p), rng.integers(40, 900, B).astype(I32)
                ph, sa = np.full((B, ncb, cap), ISENT, I32), np.full((B, ncb, chunk), ISENT, I32)
                w = R.finish_frame(tok, lp, nfr, ph, sa, ci, 2)
                out.append(_case("ar_finish_frame", tag, [B, ncb, cap, chunk, ci, 2], [tok, lp, nfr, ph, sa], (1, 2, 3, 4), dict(zip((1, 2, 3, 4), w))))
                # append_content: the chunk's newest codes, with and without the step counter
                T2, chunk = 7, 3
                codes = rng.integers(0, NC, (B, T2)).astype(I64)
                ncon = counters(cap, B, chunk, p)
                ch, sc = np.full((B, cap), ISENT, I32), np.full((B, chunk), ISENT, I32)
                cnt = np.array([41], I32) if p % 2 == 0 else None
                wh, wn = R.ring_append(ch, ncon, codes[:, T2 - chunk:])
                want = {1: wh, 2: wn, 3: codes[:, T2 - chunk:]}
                if cnt is not None:
                    want[4] = cnt + 1
                out.append(_case("append_content", tag + (" counter" if cnt is not None else " no counter"), [B, T2, chunk, cap, int(cnt is not None)],
                                 [codes, ch, ncon, sc, cnt], (1, 2, 3) + ((4,) if cnt is not None else ()), want))
                # put_codes: n_per caller-supplied codes (the delay of sva_ar_delay_fill, 1 of sva_ar_decode_one)
                n_per = (1, 2, MD, 2)[p]
                src = rng.integers(0, NC, (B, n_per)).astype(I64)
                ncon = counters(cap, B, n_per, p)
                cod, ch = np.full((B, T2 + 2), ISENT, I64), np.full((B, cap), ISENT, I32)
                wc = cod.copy()
                wc[:, T2 + 2 - n_per:] = src
                wh, wn = R.ring_append(ch, ncon, src)
                out.append(_case("put_codes", tag + " n_per %d" % n_per, [B, T2 + 2, n_per, cap], [src, cod, ch, ncon], (1, 2, 3), {1: wc, 2: wh, 3: wn}))
    return out


# ---- row builders ----------------------------------------------------------------------------------------------------------------------------------
def prompt_cases():
    out = []
    for D, ncb, d, R0, nspk, short in [(1024, 8, 2, 5, 33, 0), (300, 1, 1, 3, 33, 0), (300, 8, MD, 11, 2, 0), (257, 8, 2, 4, 33, 1)]:
        rng = np.random.default_rng(D + ncb + d)
        ce, cbe, w4s = _tables(rng, D, ncb)
        spk = rng.standard_normal((nspk, D)).astype(F32)
        Pmax = R0 + 3
        cc, ac = rng.integers(0, NC, R0).astype(I32), rng.integers(0, CBS, (ncb, Pmax)).astype(I32)
        ac[:, R0:] = CBS + 5          # staging entries behind the prompt: never read
        rows = nspk + 2 * R0 - short          # (short: the offline prefill builds one row less and puts its own last row)
        x = np.full((rows + 1, D), SENT, F32)
        want = x.copy()
        want[:rows] = np.concatenate([spk, R.prompt_rows(ce, cbe, w4s, cc, ac, d, CBS)[0]])[:rows]
        out.append(_case("build_prompt", "D %d ncb %d d %d R %d rows %d" % (D, ncb, d, R0, rows), [nspk, R0, d, ncb, CBS, D, Pmax, NC, MD, rows],
                         [spk, ce, cbe, w4s, cc, ac, x[:rows]], (6,), {6: want[:rows]}))
    return out


def delayfill_cases():
    out = []
    for cap in CAPS:
        for p in range(4):
            for B, D, d in [(1, 300, (1, 2, MD, 2)[p]), (3, 1024 if (cap == 16 and p == 0) else 300, (2, MD, 1, 2)[p]), (65, 257, (MD, 1, 2, 2)[p])]:
                rng = np.random.default_rng(7000 + 100 * cap + 10 * p + B)
                ce = _tables(rng, D, 1)[0]
                slot_list = np.array([0], I32) if B == 1 else rng.permutation(B)[:B - 1 - B // 3].astype(I32)          # a shuffled proper subset
                ncon = counters(cap, B, d, p) + d          # the d-row read [ncon - d, ncon) sits where the placement says
                ch = rng.integers(0, NC, (B, cap)).astype(I32)
                cre, lp = rng.standard_normal((B, MD, D)).astype(F32), rng.integers(40, 900, B).astype(I32)
                n, rows = len(slot_list), 2 * d - 1
                x, so, po, cae = np.full((n * rows, D), SENT, F32), np.full(n * rows, ISENT, I32), np.full(n * rows, ISENT, I32), np.full((B, D), SENT, F32)
                wx, ws, wp, wc = R.delayfill_rows(ce, ch, ncon, cre, lp, d, slot_list)
                wcae = cae.copy()
                wcae[slot_list] = wc
                out.append(_case("build_delayfill", "cap %d B %d D %d d %d %s" % (cap, B, D, d, PLACEMENTS[p]), [B, n, d, D, cap, MD, NC],
                                 [ce, ch, ncon, cre, lp, slot_list, x, so, po, cae], (6, 7, 8, 9), {6: wx, 7: ws, 8: wp, 9: wcae}))
    return out


def reprefill_cases():
    """build_reprefill and finish_reprefill over the same slots: each slot has its own stored prompt length, frame count and content count (a restarted
    slot counts from its own start), na = d or na = buffer_frames, slots in non-monotone order"""
    out = []
    for cap in CAPS:
        bf = 6 if cap == 16 else 32
        for p in range(4):
            n, B, D, ncb, d = [(1, 1, 300, 8, 2), (3, 5, 1024 if cap == 16 else 300, 8, MD if cap == 64 else 2), (128, 130, 257, 1, 1), (3, 65, 300, 8, 2)][p]
            if cap == 64 and n == 128:
                n, B = 3, 3          # (the 128-slot pass once, at the small capacity)
            rng = np.random.default_rng(9000 + 100 * cap + p)
            ce, cbe, w4s = _tables(rng, D, ncb)
            slots = rng.permutation(B)[:n].astype(I32)
            if n >= 3 and np.all(np.diff(slots) > 0):
                slots = slots[::-1].copy()
            na = np.array([d if i % 2 == 0 else bf for i in range(n)], I32)
            Rt = np.array([d + (3 * i) % 5 for i in range(n)], I32)          # (d itself included: every ref_tail row of the slot is read)
            # the na-row reads: [nf - na, nf) of the prediction ring and [ncon - d - na, ncon - d) of the content ring, placed per slot
            nf = np.array([counter_at(cap, int(na[i]), (p + i) % 4, 1 + i % 3) + int(na[i]) for i in range(n)], I32)
            ncon = np.array([counter_at(cap, int(na[i]), (p + i + 1) % 4, 1 + (i + 1) % 3) + int(na[i]) + d for i in range(n)], I32)
            ch, ph = rng.integers(0, NC, (B, cap)).astype(I32), rng.integers(0, CBS, (B, ncb, cap)).astype(I32)
            rt = rng.integers(0, CBS, (B, ncb, MD)).astype(I32)
            M = int(2 * na.sum())
            x, so, po = np.full((M, D), SENT, F32), np.full(M, ISENT, I32), np.full(M, ISENT, I32)
            tag = "cap %d n %d B %d D %d ncb %d d %d bf %d rotation %d" % (cap, n, B, D, ncb, d, bf, p)
            desc = [B, n, d, ncb, CBS, D, 33, cap, MD, NC]
            wx, ws, wp = R.reprefill_rows(ce, cbe, w4s, ch, ph, rt, slots, Rt, nf, na, ncon, d, CBS, 33)
            out.append(_case("build_reprefill", tag, desc, [slots, Rt, nf, na, ncon, ce, cbe, ch, ph, rt, x, so, po], (10, 11, 12), {10: wx, 11: ws, 12: wp}))
            cre, lp = np.full((B, MD, D), SENT, F32), np.full(B, ISENT, I32)
            we, wl = R.reprefill_finish(cbe, ph, rt, slots, Rt, nf, na, d, CBS, 33)
            wcre, wlp = cre.copy(), lp.copy()
            wcre[slots, :d] = we
            wlp[slots] = wl
            out.append(_case("finish_reprefill", tag, desc, [slots, Rt, nf, na, ncon, cbe, ph, rt, cre, lp], (8, 9), {8: wcre, 9: wlp}))
    return out


def frame_cases():
    """ar_prepare_step, apply_forced, put_row"""
    out = []
    for B, D, chunk, ci in [(1, 1024, 1, 0), (3, 300, 3, 2), (65, 257, 2, 1)]:
        rng = np.random.default_rng(300 + B)
        ce = _tables(rng, D, 1)[0]
        T2 = 6
        codes, lp = rng.integers(0, NC, (B, T2)).astype(I64), rng.integers(40, 900, B).astype(I32)
        cae = rng.standard_normal((B, D)).astype(F32)
        x, so, po, sc = np.full((2 * B, D), SENT, F32), np.full(2 * B, ISENT, I32), np.full(2 * B, ISENT, I32), np.full((B, chunk), ISENT, I32)
        code_off = T2 - chunk + ci
        w = R.prepare_step(cae, ce, codes, code_off, lp, sc, ci)
        out.append(_case("ar_prepare_step", "B %d D %d chunk %d ci %d" % (B, D, chunk, ci), [B, T2, code_off, D, chunk, ci, NC], [cae, ce, codes, lp, x, so, po, sc],
                         (4, 5, 6, 7), dict(zip((4, 5, 6, 7), w))))
        for use in (0, 1):
            ncb, cb = (8, 5) if B != 3 else (1, 0)
            raw, forced = rng.integers(0, CBS, (B, ncb)).astype(I32), rng.integers(0, CBS, (B, ncb, chunk)).astype(I32)
            tok = np.full((B, ncb), ISENT, I32)
            out.append(_case("apply_forced", "B %d ncb %d cb %d chunk %d ci %d use_forced %d" % (B, ncb, cb, chunk, ci, use), [B, ncb, cb, chunk, ci, use], [raw, forced, tok], (2,),
                             {2: R.apply_forced(raw, forced, use, ci, cb, tok)}))
    for D, code in [(1024, NC - 1), (300, 0)]:
        rng = np.random.default_rng(D)
        ce = _tables(rng, D, 1)[0]
        out.append(_case("put_row", "D %d code %d" % (D, code), [NC, code, D], [ce, np.full(D, SENT, F32)], (1,), {1: ce[code]}))
    return out


# ---- copies, fills, counters -------------------------------------------------------------------------------------------------------------------------
def copy_cases():
    out = []
    rng = np.random.default_rng(5)
    for rows, D, stride, off in [(1, 1024, 1024, 3 * 1024), (3, 300, 600, 300), (65, 257, 514, 257)]:          # (the prefill's last row; the frame tail's row pairs)
        src = rng.standard_normal(off + rows * stride + 5).astype(F32)
        want = np.stack([src[off + r * stride:off + r * stride + D] for r in range(rows)])
        out.append(_case("copy_rows", "rows %d D %d stride %d off %d" % (rows, D, stride, off), [rows, D, stride, off, src.size], [src, np.full((rows, D), SENT, F32)], (1,), {1: want}))
        out.append(_case("copy_rows2", "rows %d D %d stride %d off %d" % (rows, D, stride, off), [rows, D, stride, off, src.size],
                         [src, np.full((rows, D), SENT, F32), np.full((rows, D), SENT, F32)], (1, 2), {1: want, 2: want}))
    for B, C, rows_alloc, src_row, lo, hi in [(1, 1024, 6, 5, 0, 6), (3, 300, 9, 4, 2, 7), (2, 257, 8, 7, 1, 5)]:          # src_row: last of, inside, outside [lo, hi)
        bs = rows_alloc * C + 3
        p = rng.standard_normal((B, bs)).astype(F32)
        want = p.copy()
        for b in range(B):
            v = want[b, :rows_alloc * C].reshape(rows_alloc, C)
            v[lo:hi] = v[src_row].copy()
        out.append(_case("broadcast_row", "B %d C %d src_row %d rows [%d, %d) of %d" % (B, C, src_row, lo, hi, rows_alloc), [B, bs, C, p.size, src_row, lo, hi], [p.reshape(-1)], (0,),
                         {0: want.reshape(-1)}))
        src = rng.standard_normal(C).astype(F32)
        p = np.full((B, bs), SENT, F32)
        want = p.copy()
        want[:, :hi * C] = np.tile(src, hi)
        out.append(_case("fill_rows", "B %d C %d rows %d of %d" % (B, C, hi, rows_alloc), [B, bs, C, p.size, hi], [p.reshape(-1), src], (0,), {0: want.reshape(-1)}))
    for B, Ht, gap, c, T2, D in [(1, 0, 6, 1, 5, 1024), (3, 2, 6, 3, 9, 300), (2, 4, 0, 2, 6, 260)]:
        tb, db = (Ht + gap + c) * D + 8, T2 * D + 4
        tok, d2c = rng.standard_normal((B, tb)).astype(F32), np.full((B, db), SENT, F32)
        want = d2c.copy()
        want[:, :T2 * D] = R.copy_tokens(tok[:, :(Ht + gap + c) * D].reshape(B, -1, D), d2c[:, :T2 * D].reshape(B, T2, D), Ht, gap, c).reshape(B, -1)
        out.append(_case("copy_tokens", "B %d Ht %d gap %d c %d T2 %d D %d" % (B, Ht, gap, c, T2, D), [B, Ht, gap, c, T2, D, tb, tok.size, db, d2c.size],
                         [tok.reshape(-1), d2c.reshape(-1)], (1,), {1: want.reshape(-1)}))
    for B, n4, o_off in [(1, 64, 0), (2, 300, 8), (3, 513, 256 * 4)]:          # n4: below, not a multiple of, and past the 256-lane block
        yb, ob = 4 * n4 + 4, o_off + 4 * n4 + 8
        y = [rng.standard_normal((B, yb)).astype(F32) * F32(3.0) for _ in range(3)]
        o = np.full((B, ob), SENT, F32)
        want = o.copy()
        want[:, o_off:o_off + 4 * n4] = R.mean3(*(v[:, :4 * n4] for v in y))
        out.append(_case("mean3", "B %d n4 %d o_off %d" % (B, n4, o_off), [B, yb, y[0].size, ob, o_off, o.size, n4], [v.reshape(-1) for v in y] + [o.reshape(-1)], (3,),
                         {3: want.reshape(-1)}))
    for n in (1, 64, 65, 130):
        p = rng.integers(-50, 50, n + 3).astype(I32)
        want = p.copy()
        want[:n] += 5
        out.append(_case("add_vec", "n %d" % n, [p.size, 5, n], [p], (0,), {0: want}))
        lst = rng.permutation(n + 3)[:n].astype(I32)
        want = p.copy()
        want[lst] += -3
        out.append(_case("add_list", "n %d" % n, [p.size, -3, n], [p, lst], (0,), {0: want}))
    p = np.arange(10, 17).astype(I32)
    out.append(_case("inc", "by 9", [p.size, 9], [p], (0,), {0: p + np.array([9, 0, 0, 0, 0, 0, 0], I32)}))
    want = p.copy()
    want[6] = -4
    out.append(_case("set_slot_i32", "slot 6", [p.size, -4, 6], [p], (0,), {0: want}))
    return out


def history_cases():
    """history_rows_copy (both directions, a slot range that does not start at 0) and history_rows_move (the float4 arm, the scalar arm through a
    misaligned address and through H C % 4 != 0)"""
    out = []
    rng = np.random.default_rng(11)
    descs = [(0, 400, 4, 32), (1700, 200, 3, 5), (2901, 160, 6, 16)]          # (offset, bstride, H, C) of the live tensors, B = 4 slots
    B, b_len = 4, 3700
    offs, tot = [], 0
    for _, _, H, C in descs:
        offs.append(tot)
        tot += H * C
    sbs = tot + 3
    for slot_lo, ns, to_live in [(0, 4, 0), (1, 2, 0), (2, 1, 1), (1, 3, 1)]:
        buf, save = rng.standard_normal(b_len).astype(F32), rng.standard_normal(B * sbs).astype(F32)
        wb, ws = buf.copy(), save.copy()
        for (off, bs, H, C), so in zip(descs, offs):
            for s in range(slot_lo, slot_lo + ns):
                live, sv = slice(off + s * bs, off + s * bs + H * C), slice(s * sbs + so, s * sbs + so + H * C)
                if to_live:
                    wb[live] = save[sv]
                else:
                    ws[sv] = buf[live]
        desc = [len(descs), ns, slot_lo, to_live, b_len, save.size, sbs] + [v for (off, bs, H, C), so in zip(descs, offs) for v in (off, bs, H, C, so)]
        out.append(_case("history_rows_copy", "slots [%d, %d) %s" % (slot_lo, slot_lo + ns, "save -> live" if to_live else "live -> save"), desc, [buf, save], (0, 1), {0: wb, 1: ws}))
    # (source offset, destination offset, destination bstride, H, C): 16-byte aligned pair; misaligned destination; misaligned source; H C % 4 != 0
    moves = [(0, 0, 400, 4, 32), (128, 1201, 100, 4, 8), (163, 1700, 64, 2, 16), (200, 2000, 20, 3, 5)]
    for slot in (0, 2):
        src, dst = rng.standard_normal(300).astype(F32), np.full(2300, SENT, F32)
        want = dst.copy()
        for so, to, bs, H, C in moves:
            want[to + slot * bs:to + slot * bs + H * C] = src[so:so + H * C]
        out.append(_case("history_rows_move", "slot %d float4 and scalar arms" % slot, [len(moves), slot, src.size, dst.size] + [v for m in moves for v in m], [src, dst], (1,), {1: want}))
    return out


GENERATORS = (ring_cases, prompt_cases, delayfill_cases, reprefill_cases, frame_cases, copy_cases, history_cases)


def all_cases():
    return [c for g in GENERATORS for c in g()]


def move_arm(src_off, dst_off, dst_bstride, slot, H, C):
    """which arm of history_rows_move a descriptor takes (device allocations are 256-byte aligned)"""
    return "float4" if (H * C) % 4 == 0 and src_off % 4 == 0 and (dst_off + slot * dst_bstride) % 4 == 0 else "scalar"


# ---- preconditions ------------------------------------------------------------------------------------------------------------------------------------
def _within(v, lo, hi):
    v = np.asarray(v)
    return v.size == 0 or (int(v.min()) >= lo and int(v.max()) < hi)


def validate(c):
    """everything the launch of case c indexes with lies inside its arrays (the hook checks the same before it launches)"""
    op, d, a = c["op"], c["desc"], c["arrays"]
    pow2 = lambda v: v >= 1 and v & (v - 1) == 0
    assert len(a) == len(ARRAYS[op]), c["id"]
    for i in c["io"]:
        assert a[i] is not None and c["want"][i].shape == a[i].shape and c["want"][i].dtype == a[i].dtype, (c["id"], i)
    if op == "ar_finish_frame":
        B, ncb, cap, chunk, ci, _ = d
        assert pow2(cap) and 1 <= ncb <= 8 and 0 <= ci < chunk and a[3].shape == (B, ncb, cap) and a[4].shape == (B, ncb, chunk) and a[0].shape == (B, ncb) and a[2].shape == (B,)
    elif op == "append_content":
        B, T2, chunk, cap, has = d
        assert pow2(cap) and chunk <= T2 and chunk <= cap and a[0].shape == (B, T2) and a[1].shape == (B, cap) and a[3].shape == (B, chunk) and (a[4] is not None) == bool(has)
    elif op == "put_codes":
        B, T2, n_per, cap = d
        assert pow2(cap) and n_per <= T2 and n_per <= cap and a[0].shape == (B, n_per) and a[1].shape == (B, T2) and a[2].shape == (B, cap)
    elif op == "build_prompt":
        nspk, R0, dl, ncb, cbs, D, Pmax, nc, md, rows = d
        assert ncb <= 8 and dl <= md and R0 > dl and R0 <= Pmax and rows <= nspk + 2 * R0 and a[6].shape == (rows, D) and a[0].shape == (nspk, D)
        assert _within(a[4], 0, nc) and _within(a[5][:, :R0], 0, cbs) and a[1].shape == (nc, D) and a[2].shape == (ncb * cbs, D) and a[3].shape == (md, D)
    elif op == "build_delayfill":
        B, n, dl, D, cap, md, nc = d
        assert pow2(cap) and dl <= md and dl <= cap and _within(a[5], 0, B) and len(set(a[5].tolist())) == n and (n < B or B == 1) and _within(a[1], 0, nc)
        assert a[6].shape == (n * (2 * dl - 1), D) and a[3].shape == (B, md, D) and a[9].shape == (B, D) and (a[2] >= dl).all()
    elif op in ("build_reprefill", "finish_reprefill"):
        B, n, dl, ncb, cbs, D, nspk, cap, md, nc = d
        slots, Rt, nf, na, ncon = a[:5]
        assert 1 <= n <= 128 and pow2(cap) and ncb <= 8 and dl <= md and _within(slots, 0, B) and len(set(slots.tolist())) == n
        assert (na >= dl).all() and (na <= nf).all() and (na + dl <= ncon).all() and (na + dl < cap).all() and (Rt >= dl).all()
        ph, rt = (a[8], a[9]) if op == "build_reprefill" else (a[6], a[7])
        assert _within(ph, 0, cbs) and _within(rt, 0, cbs) and ph.shape == (B, ncb, cap) and rt.shape == (B, ncb, md)
        if op == "build_reprefill":
            assert _within(a[7], 0, nc) and a[10].shape == (2 * int(na.sum()), D)
    elif op == "ar_prepare_step":
        B, T2, code_off, D, chunk, ci, nc = d
        assert 0 <= code_off < T2 and 0 <= ci < chunk and _within(a[2], 0, nc) and a[4].shape == (2 * B, D)
    elif op == "apply_forced":
        B, ncb, cb, chunk, ci, _ = d
        assert ncb <= 8 and 0 <= cb < ncb and 0 <= ci < chunk and a[1].shape == (B, ncb, chunk)
    elif op == "put_row":
        assert 0 <= d[1] < d[0] and a[0].shape == (d[0], d[2])
    elif op in ("copy_rows", "copy_rows2"):
        rows, D, stride, off, n = d
        assert off + (rows - 1) * stride + D <= n == a[0].size
    elif op == "broadcast_row":
        B, bs, C, n, src_row, lo, hi = d
        assert (B - 1) * bs + max(hi, src_row + 1) * C <= n == a[0].size and 0 <= lo < hi
    elif op == "fill_rows":
        B, bs, C, n, rows = d
        assert (B - 1) * bs + rows * C <= n == a[0].size
    elif op == "copy_tokens":
        B, Ht, gap, cc, T2, D, tb, tn, db, dn = d
        assert D % 4 == 0 and tb % 4 == 0 and db % 4 == 0 and Ht + cc <= T2 and (B - 1) * tb + (Ht + gap + cc) * D <= tn == a[0].size and (B - 1) * db + T2 * D <= dn == a[1].size
    elif op == "mean3":
        B, yb, yn, ob, o_off, on, n4 = d
        assert yb % 4 == 0 and ob % 4 == 0 and o_off % 4 == 0 and (B - 1) * yb + 4 * n4 <= yn and (B - 1) * ob + o_off + 4 * n4 <= on
    elif op in ("add_vec", "add_list"):
        assert d[2] <= d[0] and (op == "add_vec" or (_within(a[1], 0, d[0]) and len(set(a[1].tolist())) == d[2]))
    elif op == "set_slot_i32":
        assert 0 <= d[2] < d[0]
    elif op == "history_rows_copy":
        nd, ns, lo, _, bn, sn, sbs = d[:7]
        for i in range(nd):
            off, bs, H, C, so = d[7 + 5 * i:12 + 5 * i]
            assert off + (lo + ns - 1) * bs + H * C <= bn and (lo + ns - 1) * sbs + so + H * C <= sn
    elif op == "history_rows_move":
        nd, slot, sn, tn = d[:4]
        for i in range(nd):
            so, to, bs, H, C = d[4 + 5 * i:9 + 5 * i]
            assert so + H * C <= sn and to + slot * bs + H * C <= tn
    else:
        assert op == "inc", op


# ---- fused HiFiGAN level -------------------------------------------------------------------------------------------------------------------------------
DIL = (1, 3, 5)
RF_MAX = 20 * sum(DIL)          # 180 rows: the six-conv chain at kernel size 11


def voc_tile_rows(C, B, Tl):
    """the launcher's rule (csrc/voc_fused.hip): 64 rows, doubled while the launch still fills the chip, up to what LDS holds"""
    tr_max, TR = (256 if C == 16 else 128), 64
    while TR < tr_max and ((Tl + 2 * TR - 1) // (2 * TR)) * 3 * B >= 256:
        TR *= 2
    return TR


def voc_next_tile_Tl(C, B):
    """the smallest Tl at which the launcher leaves TR = 64"""
    Tl = 1
    while voc_tile_rows(C, B, Tl) == 64:
        Tl += 127 if voc_tile_rows(C, B, Tl + 127) == 64 else 1
    return Tl


def voc_weights(C, seed=0):
    """18 convs as the engine keeps them ([C, k C], tap-major columns), He-like scale so that the six-conv chain keeps its magnitude"""
    rng = np.random.default_rng(50 + C + seed)
    W = [[(rng.standard_normal((C, k * C)) * np.sqrt(1.0 / (k * C))).astype(F32) for _ in range(6)] for k in R.VOC_LEVEL_K]
    bias = [[(rng.standard_normal(C) * 0.1).astype(F32) for _ in range(6)] for _ in R.VOC_LEVEL_K]
    return W, bias


# (C, B, Tl, frames_done, rows_per_frame, kind): tile and 16-row edges at TR = 64, both channel counts, one and three streams, the stream start, the
# first continuation frame and the steady state, input scales and the saturation of SiLU
VOC_TL = (1, 15, 16, 17, 63, 64, 65, 129)


def voc_cases():
    out = []
    for C in (16, 32):
        for i, Tl in enumerate(VOC_TL):
            out.append(dict(C=C, B=(1, 3)[i % 2], Tl=Tl, frames_done=(0, 1, 5)[i % 3], rows_per_frame=(180, 256)[i % 2], kind="normal"))
        out.append(dict(C=C, B=3, Tl=129, frames_done=0, rows_per_frame=200, kind="normal"))          # three streams at the stream start, a ragged last tile
        out.append(dict(C=C, B=1, Tl=65, frames_done=0, rows_per_frame=180, kind="scaled 1e-4"))
        out.append(dict(C=C, B=1, Tl=65, frames_done=1, rows_per_frame=180, kind="scaled 30"))
        out.append(dict(C=C, B=3, Tl=17, frames_done=5, rows_per_frame=180, kind="saturating rows"))
        out.append(dict(C=C, B=1, Tl=64, frames_done=0, rows_per_frame=180, kind="zero"))
        out.append(dict(C=C, B=3, Tl=voc_next_tile_Tl(C, 3) + 5, frames_done=1, rows_per_frame=180, kind="next tile height"))
    return out


def voc_input(c):
    """-> X [B, x_bstride / C rows, C] (RF_MAX history rows, Tl new rows, padding rows), the padded strides in floats; history rows in front of the stream
    start are NaN (frames_done = 0: all of them)"""
    C, B, Tl, kind = c["C"], c["B"], c["Tl"], c["kind"]
    rng = np.random.default_rng(C * 1000 + Tl + 7 * c["frames_done"])
    x = rng.standard_normal((B, RF_MAX + Tl + 3, C)).astype(F32)
    if kind == "scaled 1e-4":
        x *= F32(1e-4)
    elif kind == "scaled 30":
        x *= F32(30.0)
    elif kind == "saturating rows":
        x[:, RF_MAX - 2] = 90.0
        x[:, RF_MAX + 3] = -90.0
        x[:, RF_MAX + Tl - 1, ::2] = 90.0
    elif kind == "zero":
        x[:] = 0.0
    if c["frames_done"] == 0:
        x[:, :RF_MAX] = np.nan
    x[:, RF_MAX + Tl:] = SENT          # the padding of x_bstride: never read
    return x


def validate_voc(c):
    assert c["C"] in (16, 32) and c["rows_per_frame"] >= RF_MAX and c["Tl"] >= 1 and c["frames_done"] >= 0
    if c["kind"] == "next tile height":
        assert voc_tile_rows(c["C"], c["B"], c["Tl"]) == 128 and voc_tile_rows(c["C"], c["B"], voc_next_tile_Tl(c["C"], c["B"]) - 1) == 64 and c["Tl"] < 8000
    else:
        assert voc_tile_rows(c["C"], c["B"], c["Tl"]) == 64


# ---- the ring wrap through the real decode paths (test_gpu_parity.py) --------------------------------------------------------------------------------
# max_seq_frames = 160 / buffer_frames = 16 streams at hist_cap = 32: (streams, SVA_DEBUG decode selection, the decode path it must give).  Slot s takes the
# prompt length WRAP_PROMPTS[s]: 112 frames re-prefills at frame 31 (its delay fill reads content entries 31, 32) and at frame 46 (its 16-frame windows
# read entries 30 .. 45 of both rings); the others re-prefill at steps of their own.
WRAP_CAP, WRAP_CHUNKS, WRAP_KW = 32, 50, dict(max_seq_frames=160, buffer_frames=16, delay=2, chunk_frames=1)
WRAP_PROMPTS = (112, 122, 107, 104, 112, 99, 122, 112)          # (every one re-prefills within WRAP_CHUNKS)
WRAP_RUNS = ((1, "ar_batch=1,ar_persistent=1", 1), (2, "ar_batch=1,ar_persistent=1", None), (8, "ar_batch=1,ar_persistent=1", 2), (3, "ar_batch=0,ar_persistent=0", 0))


def wrap_straddles(reprefills, cap, d):
    """reprefills: (frames decoded nf, content codes seen ncon, appended frames na) of every re-prefill of a stream -> which accesses crossed a multiple of
    the capacity: the na-frame window of the prediction ring, that of the content ring, the d entries of the delay fill behind it"""
    cross = lambda lo, hi: lo // cap != (hi - 1) // cap
    return dict(pred=any(cross(nf - na, nf) for nf, ncon, na in reprefills), content=any(cross(ncon - d - na, ncon - d) for nf, ncon, na in reprefills),
                fill=any(cross(ncon - d, ncon) for nf, ncon, na in reprefills))
