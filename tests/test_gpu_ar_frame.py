"""Whole decode frames of the three AR paths -- ar_decode_kernel (ar_decode.hip), ar_batch_kernel (ar_batch.hip) and the multi-launch chain
(ar_layers_pass + ar_frame_tail) -- against the float64 frame of tests/ar_frame_ref.py, one frame at a time from the engine's own state.

Before a compared frame the test reads back everything the frame reads: the slot's slow K / V rows [0, last_pos] of all 12 layers
(Batch.kv_rows), its cached_audio_emb row and last_pos.  frame_fp64 evaluates the frame from that state, so the prefill's and earlier frames'
errors are in the state and the frame is judged alone: all 8192 slow logits, all 8 x 1000 fast logits, the whole pre-norm hidden state, the
two new K and V rows of every layer and the new cached_audio_emb, each within
    4 * ORACLE_K[q] * EPS32 * max |ref q| + 4 ulp32(max |ref q|)
where ORACLE_K is the float32 oracle's own measured distance from frame_fp64 (tests/test_ar_frame_ref_cpu.py); a new row of the fp16 cache
(ar_dtype = 1) gets one fp16 ulp of its float64 value on top.  LOGIT_TOL plays no part.

Batches are ragged inside one launch: every slot has its own prompt seed and length -- the shortest prompt the engine takes (delay + 1 = 3
frames), 4, 100 and odd lengths in between -- and in most cases one slot carries the LONG prompt whose first decoded frame starts at
last_pos = max_seq_len - 33 and whose 16th frame writes positions max_seq_len - 2 and max_seq_len - 1.  That slot is the first, the last or
the second of a two-stream launch.  Frames come from sva_ar_delay_fill + teacher-forced sva_ar_decode_one with host noise.

Every slot of every frame: last_pos advances by 2, audio_codes are the forced codes, the persistent kernels' timeout word stays 0, and the
sampled codes (tok_raw) are the oracle's sample_token in float64 on the engine's OWN logits row with the slot's noise and sampling pair (two
slots carry a non-default pair, one of them greedy) unless that draw is within 1e-5 of a tie; at most 1 % may be.  Compared slots: the rows
below the new ones (the 8 preceding rows and rows 0 .. 7) are bit-identical before and after, the two rows beyond are untouched.

The frame's own two rows under an fp16 cache (ar_dtype = 1) -- a finding of this file.  The persistent kernels feed the attention the two
new K / V rows as computed (float32, from the hand-off granules) and round them only into the cache; the multi-launch chain writes them to the
fp16 cache first (rope_kvwrite_kernel) and its attention reads them back rounded.  Both are legitimate readings of "write the rows, attend over
[0, pos]", they differ by half an fp16 ulp on two keys of every row, and that is 10 - 16 x this file's bound on the logits (measured: the chain
against the as-computed frame 12.4 x, the persistent kernels against rounded rows 15.4 x / 16.2 x).  Each path is therefore held to the reading it
implements, which keeps the bound at the float32 size for both; making the paths agree changes what an ar_dtype = 1 stream computes and is left
to a change of its own.  For the chain the reference attends the rows the cache HOLDS after the frame (frame_fp64's kv_stored), not its own
float64 rows rounded to fp16: rounding is a step function, and a float32 value within its own rounding error of an fp16 tie is stored a whole
fp16 ulp from where the float64 value rounds.  A reference that re-rounded put path0-fp16-B33 at 1.28 x the bound on the slow logits of a
3-frame prompt (a few such elements among 2 x 12 x 1536, heavy where the context is short); on the stored rows the case measures 0.25 x.  The
stored rows themselves are compared with the float64 rows to one fp16 ulp, so a wrong write is still seen.

The cache end: the frame that ends on max_seq_len - 1 matches float64; the next sva_ar_decode_one (and sva_ar_delay_fill) is refused with an
error that names the cache, nothing having been uploaded or launched -- positions and the cache tail are unchanged -- and after a fresh
prefill_prompt + begin the batch decodes normally.  No frame runs past the cache."""
import numpy as np
import pytest
import torch

import ar_frame_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DELAY = 2
# 33 + 2 (1000 + 4) + 4 <= 2048: the long prompt fits the batch's re-prefill constraint.  decode_window_frames = 4: sva_streams_begin primes the
# vocoder with min(window - 1, R) prompt frames and refuses fewer than 16 of them unless that is the whole window -- the AR never reads it
BATCH_KW = dict(chunk_frames=1, delay=DELAY, max_prompt_frames=1000, buffer_frames=4, decode_window_frames=4)
FRAMES = 4
MODE_DEFAULT = "ar_batch=1,ar_persistent=1"
MODE_PER_STREAM = "ar_batch=0,ar_persistent=1"          # ar_decode.hip up to its 6 (fp16: 4) streams
MODE_CHAIN = "ar_batch=0,ar_persistent=0"
PAIRS = ((1.1, 0.9), (0.7, 0.0))                        # the two non-default sampling pairs: a warm wide nucleus, and greedy (top_p = 0)

_WORST = {}                                             # case id -> {quantity: worst err / bound}


@pytest.fixture(scope="module")
def engines(weights0):
    from streamvoiceanon_amd import engine as E
    made = {}

    def get(half):
        if half not in made:
            made[half] = E.Engine(weights0, ar_dtype=1 if half else 0)
        return made[half]

    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def w64s(weights0):
    """float64 weights per precision variant (about 1 GB each): built on first use, dropped at module teardown"""
    from oracle import sva_oracle as O
    made = {}

    def get(half):
        if half not in made:
            made[half] = R.build_w64(weights0, O.ARConfig(), half=half)
        return made[half]

    yield get
    for w in made.values():
        w.clear()
    made.clear()


def _prompt_lengths(B, long_slot, rng):
    """distinct lengths: 3 (= delay + 1, the shortest the engine and the oracle take), 100, 4, then odd ones; the long slot gets the prompt that
    puts its first decode at last_pos = max_seq_len - 33"""
    from oracle import sva_oracle as O
    cfg = O.ARConfig()
    Rs = ([3, 100, 4] + [5 + 2 * i for i in range(B)])[:B]
    if long_slot is not None:
        if long_slot == 0 and B > 1:
            Rs[1] = 3                                  # the shortest prompt stays in the batch
        Rs[long_slot] = R.long_prompt_frames(cfg.max_seq_len, DELAY, cfg.n_spk_tokens)
        assert R.last_pos_after_fill(Rs[long_slot], DELAY, cfg.n_spk_tokens) == cfg.max_seq_len - 33
    assert len(set(Rs)) == B
    return Rs


def _make_batch(eng, B, mode):
    from streamvoiceanon_amd import engine as E
    lib = E.load_library()
    assert lib.sva_debug_configure(mode.encode()) == 0           # (read at batch creation)
    try:
        return E.Batch(eng, n_streams=B, **BATCH_KW)
    finally:
        lib.sva_debug_configure(MODE_DEFAULT.encode())


def _start(b, Rs, seed, rng):
    from streamvoiceanon_amd.synth_audio import synth_prompt
    for s, Rf in enumerate(Rs):
        ac, cc, style, timbre = synth_prompt(seed * 1000 + s, Rf)
        b.prefill_prompt(s, cc, ac, style, timbre, noise_seed=seed * 1000 + s)
    b.begin()
    b.ar_delay_fill(rng.integers(0, 8192, (b.B, DELAY)))


def _check_frame(ref, got, half, where, worst, failures):
    """one compared (slot, frame): every quantity against its bound; failures carry the per-layer evidence"""
    for q in R.QUANTITIES:
        if q == "kv":
            err = np.maximum(np.abs(got["k_new"] - ref["k_new"]), np.abs(got["v_new"] - ref["v_new"]))       # [L, 2, H, 64]
            lim = np.full(err.shape, R.bound("kv", np.concatenate([ref["k_new"].ravel(), ref["v_new"].ravel()])))
            if half:
                lim = lim + np.maximum(R.ulp16(ref["k_new"]), R.ulp16(ref["v_new"]))
            ratio = err / lim
        else:
            ratio = np.abs(got[q] - ref[q]) / R.bound(q, ref[q])
        w = float(ratio.max())
        worst[q] = max(worst.get(q, 0.0), w)
        if not w <= 1.0:
            ev = dict(where=where, quantity=q, worst_ratio=round(w, 3))
            if q == "kv":
                ev["per_layer"] = [round(float(ratio[l].max()), 2) for l in range(ratio.shape[0])]
                ev["row0_row1"] = [round(float(ratio[:, m].max()), 2) for m in range(2)]
            failures.append(ev)


def _run_case(engines, w64s, record_property, half, B, mode, path, long_slot, seed, recheck=False):
    from oracle import sva_oracle as O
    cfg = O.ARConfig()
    S, ncb, cbs, V, D = cfg.max_seq_len, cfg.num_codebooks, cfg.codebook_size, cfg.vocab, cfg.dim
    eng, W64 = engines(half), w64s(half)
    kv_store = half and path == 0                                   # the chain's attention reads the frame's own rows back from the fp16 cache
    rng = np.random.default_rng(seed)
    Rs = _prompt_lengths(B, long_slot, rng)
    b = _make_batch(eng, B, mode)
    case = f"path{path}-{'fp16' if half else 'fp32'}-B{B}"
    worst, failures, n_near, n_samp = {}, [], 0, 0
    try:
        assert b.decode_path() == path, (b.decode_path(), path)
        _start(b, Rs, seed, rng)
        pairs = {}
        if B >= 2:
            pairs = {B - 1: PAIRS[0], B // 2 if B // 2 != B - 1 else 0: PAIRS[1]}
        else:
            pairs = {0: PAIRS[0]}
        for s, (t, tp) in pairs.items():
            b.set_sampling(s, t, tp)
        compared = sorted({Rs.index(3) if 3 in Rs else 0, 0, B - 1, int(rng.integers(0, B))} | ({long_slot} if long_slot is not None else set()))
        n_frames = 16 if long_slot is not None else FRAMES
        lp = b.tap("last_pos", (B,), np.int32).copy()
        np.testing.assert_array_equal(lp, [R.last_pos_after_fill(r, DELAY, cfg.n_spk_tokens) for r in Rs])
        for f in range(n_frames):
            full = [s for s in compared if f in (0, FRAMES - 1) or (s == long_slot and f == n_frames - 1)]
            emb = b.tap("cached_audio_emb", (B, D))
            states = {s: R.state_from_batch(b, s, int(lp[s]), emb[s]) for s in full}
            # rows a frame must leave alone: the 8 below the new ones, rows 0 .. 7, and the two beyond the new ones
            guard = {s: (b.kv_rows(s, int(lp[s]) - 7, 8), b.kv_rows(s, 0, 8), b.kv_rows(s, int(lp[s]) + 3, 2) if lp[s] + 5 <= S else None) for s in compared}
            code = rng.integers(0, V, B)
            forced = rng.integers(0, cbs, (B, ncb)).astype(np.int32)
            noise = (rng.exponential(size=(B, V + ncb * cbs)) + 1e-9).astype(np.float32)
            codes, pos = b.ar_decode_one(code, noise=noise, forced=forced)
            if path != 0:
                assert int(b.tap("ar_fail", (1,), np.int32)[0]) == 0, (case, f)
            np.testing.assert_array_equal(pos, lp + 2)
            np.testing.assert_array_equal(b.tap("last_pos", (B,), np.int32), lp + 2)
            np.testing.assert_array_equal(codes, forced)
            np.testing.assert_array_equal(b.tap("audio_codes", (B, ncb, 1), np.int32)[:, :, 0], forced)
            slow = b.tap("slow_logits", (B, V))
            fast = b.tap("fast_logits", (B, ncb, cbs))
            hidden = b.tap("hidden", (B, D))
            emb_new = b.tap("cached_audio_emb", (B, D))
            raw = b.tap("sampled_codes", (B, ncb), np.int32)
            assert np.isfinite(slow).all() and np.isfinite(fast).all()
            for s in range(B):                          # the sampler wiring: this slot's logits row, noise row and pair
                t, tp = pairs.get(s, (0.7, 0.7))
                for cb in range(ncb):
                    tok, near = R.sample_f64(fast[s, cb], noise[s, V + cb * cbs:V + (cb + 1) * cbs], t, tp)
                    n_samp += 1
                    n_near += int(near)
                    assert near or tok == int(raw[s, cb]), (case, "sampled code", dict(frame=f, slot=s, codebook=cb, want=tok, got=int(raw[s, cb])))
            for s in compared:
                below, first, beyond = guard[s]
                assert b.kv_rows(s, int(lp[s]) - 7, 8).tobytes() == below.tobytes(), (case, f, s, "rows below the new ones changed")
                assert b.kv_rows(s, 0, 8).tobytes() == first.tobytes(), (case, f, s, "rows 0 .. 7 changed")
                if beyond is not None:
                    assert b.kv_rows(s, int(lp[s]) + 3, 2).tobytes() == beyond.tobytes(), (case, f, s, "rows beyond the new ones were written")
            for s in full:
                new = b.kv_rows(s, int(lp[s]) + 1, 2).astype(np.float64)                  # [L, 2 (k, v), H, 2, 64]
                k_got, v_got = new[:, 0].transpose(0, 2, 1, 3), new[:, 1].transpose(0, 2, 1, 3)
                ref = R.frame_fp64(W64, states[s], int(code[s]), forced[s], kv_stored=(k_got, v_got) if kv_store else None)
                got = dict(slow_logits=slow[s].astype(np.float64), fast_logits=fast[s].astype(np.float64), hidden=hidden[s].astype(np.float64),
                           emb=emb_new[s].astype(np.float64), k_new=new[:, 0].transpose(0, 2, 1, 3), v_new=new[:, 1].transpose(0, 2, 1, 3))
                assert ref["last_pos"] == int(lp[s]) + 2
                _check_frame(ref, got, half, dict(case=case, slot=s, frame=f, R=Rs[s], last_pos=int(lp[s])), worst, failures)
            lp = lp + 2
        if long_slot is not None:
            assert int(lp[long_slot]) == S - 1
            _cache_end(b, case, long_slot, Rs, seed, rng, W64, half, worst, failures, recheck, path, kv_store)
    finally:
        b.close()
    _WORST[case] = dict(worst)
    rec = dict(case=case, prompts=Rs if B <= 8 else f"{Rs[:4]}..", compared_worst_ratio={q: round(v, 3) for q, v in worst.items()},
               sampled=n_samp, near_ties=n_near)
    record_property("ar_frame", rec)
    print("[ar frame]", rec)
    assert not failures, failures
    assert n_near <= 0.01 * n_samp, (n_near, n_samp)


def _cache_end(b, case, long_slot, Rs, seed, rng, W64, half, worst, failures, recheck, path, kv_store):
    """the long slot's last frame ended on max_seq_len - 1: the next frame and a delay fill are refused on the host, nothing changes, and the
    batch starts afresh"""
    B = b.B
    lp = b.tap("last_pos", (B,), np.int32).copy()
    tail = b.kv_rows(long_slot, 2048 - 8, 8)
    emb = b.tap("cached_audio_emb", (B, 768)).copy()
    noise = (rng.exponential(size=(B, 8192 + 8000)) + 1e-9).astype(np.float32)
    with pytest.raises(RuntimeError, match="KV cache"):
        b.ar_decode_one(rng.integers(0, 8192, B), noise=noise, forced=rng.integers(0, 1000, (B, 8)))
    with pytest.raises(RuntimeError, match="KV cache"):
        b.ar_delay_fill(rng.integers(0, 8192, (B, DELAY)))
    np.testing.assert_array_equal(b.tap("last_pos", (B,), np.int32), lp)
    assert b.kv_rows(long_slot, 2048 - 8, 8).tobytes() == tail.tobytes()
    assert b.tap("cached_audio_emb", (B, 768)).tobytes() == emb.tobytes()
    # afresh: short prompts in every slot, one frame
    Rs2 = [3 + s for s in range(B)]
    _start(b, Rs2, seed + 1, rng)
    lp = b.tap("last_pos", (B,), np.int32).copy()
    np.testing.assert_array_equal(lp, [R.last_pos_after_fill(r, DELAY) for r in Rs2])
    st = R.state_from_batch(b, 0, int(lp[0]), b.tap("cached_audio_emb", (B, 768))[0]) if recheck else None
    code, forced = rng.integers(0, 8192, B), rng.integers(0, 1000, (B, 8)).astype(np.int32)
    codes, pos = b.ar_decode_one(code, noise=noise, forced=forced)
    np.testing.assert_array_equal(pos, lp + 2)
    np.testing.assert_array_equal(codes, forced)
    if path != 0:
        assert int(b.tap("ar_fail", (1,), np.int32)[0]) == 0
    if recheck:
        new = b.kv_rows(0, int(lp[0]) + 1, 2).astype(np.float64)
        ref = R.frame_fp64(W64, st, int(code[0]), forced[0],
                           kv_stored=(new[:, 0].transpose(0, 2, 1, 3), new[:, 1].transpose(0, 2, 1, 3)) if kv_store else None)
        got = dict(slow_logits=b.tap("slow_logits", (B, 8192))[0].astype(np.float64), fast_logits=b.tap("fast_logits", (B, 8, 1000))[0].astype(np.float64),
                   hidden=b.tap("hidden", (B, 768))[0].astype(np.float64), emb=b.tap("cached_audio_emb", (B, 768))[0].astype(np.float64),
                   k_new=new[:, 0].transpose(0, 2, 1, 3), v_new=new[:, 1].transpose(0, 2, 1, 3))
        _check_frame(ref, got, half, dict(case=case, slot=0, frame="after the restart", R=Rs2[0], last_pos=int(lp[0])), worst, failures)


# (half, B, mode, path, long slot, recheck after the cache end)
CASES = [
    # ar_decode.hip: two streams per launch -- 3 gives a second launch with slot_base = 2, 6 is the most it serves
    (False, 1, MODE_PER_STREAM, 1, 0, True), (False, 2, MODE_PER_STREAM, 1, 1, False), (False, 3, MODE_PER_STREAM, 1, 2, False),
    (False, 6, MODE_PER_STREAM, 1, 0, False),
    (True, 1, MODE_PER_STREAM, 1, None, False), (True, 4, MODE_PER_STREAM, 1, 3, False),
    # ar_batch.hip: 5 = 10 rows in a 16-row tile, 8 = one full tile, 9 = 18 rows (a tile edge), 24 = several tiles
    (False, 5, MODE_DEFAULT, 2, 4, True), (False, 8, MODE_DEFAULT, 2, None, False), (False, 9, MODE_DEFAULT, 2, 0, False),
    (False, 24, MODE_DEFAULT, 2, 13, False),
    (True, 5, MODE_DEFAULT, 2, None, False), (True, 12, MODE_DEFAULT, 2, 11, False),
    # the multi-launch chain: 3 streams with the persistent kernels off; 64 = the paired attention and the stream GEMMs
    (False, 3, MODE_CHAIN, 0, 1, True), (False, 64, MODE_DEFAULT, 0, 63, False),
    (True, 33, MODE_DEFAULT, 0, 0, False),
]


@pytest.mark.parametrize("half,B,mode,path,long_slot,recheck", CASES, ids=[f"path{c[3]}-{'fp16' if c[0] else 'fp32'}-B{c[1]}" for c in CASES])
def test_decode_frames_match_fp64(engines, w64s, record_property, half, B, mode, path, long_slot, recheck):
    _run_case(engines, w64s, record_property, half, B, mode, path, long_slot, seed=100 + 7 * B + (50 if half else 0) + path, recheck=recheck)


def test_kv_rows_and_the_embedding_tap_refuse_what_is_outside(engines):
    """the read-only seams: a slot outside the batch or rows outside the cache are refused; the tap has the batch's shape"""
    b = _make_batch(engines(False), 2, MODE_DEFAULT)
    try:
        for slot, pos0, n in ((-1, 0, 1), (2, 0, 1), (0, -1, 1), (0, 0, 0), (0, 2047, 2), (0, 2048, 1), (0, 0, 2049)):
            with pytest.raises(RuntimeError, match="sva_test_kv_rows"):
                b.kv_rows(slot, pos0, n)
        assert b.kv_rows(1, 2046, 2).shape == (12, 2, 12, 2, 64)
        assert b.tap("cached_audio_emb", (2, 768)).shape == (2, 768)
        with pytest.raises(RuntimeError, match="too small"):
            b.tap("cached_audio_emb", (1, 768))
    finally:
        b.close()


def test_worst_ratios_summary(record_property):
    """runs last: the table of profiles/ar_frame_parity.txt"""
    print("[ar frame] bounds: 4 x ORACLE_K x EPS32 x max|ref| + 4 ulp32(max|ref|), ORACLE_K =", R.ORACLE_K)
    for case, w in _WORST.items():
        print("[ar frame] worst err / bound", case, {q: round(v, 3) for q, v in w.items()})
    record_property("ar_frame_worst", _WORST)
    assert _WORST, "no case of this file ran before its summary"
